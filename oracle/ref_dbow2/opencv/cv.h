// opencv/cv.h stand-in — TEST INFRASTRUCTURE ONLY, our own text.
//
// The least of OpenCV that DBoW2's ORB vocabulary (TemplatedVocabulary<FORB::TDescriptor, FORB>)
// needs to compile and run: cv::Mat as a reference-counted byte matrix (a descriptor is one
// 1 x 32 CV_8U row), and cv::FileStorage / cv::FileNode as inert types for the YAML members
// that only have to compile (the driver never calls them).  Mat::create zero-fills, where
// OpenCV leaves the bytes unwritten.  Not to be widened towards the rest of OpenCV.
#ifndef REF_DBOW2_OPENCV_CV_H
#define REF_DBOW2_OPENCV_CV_H
#include <cmath>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#define CV_8U 0
#define CV_32F 5

namespace cv {

class Mat {
public:
    int rows, cols;
    Mat() : rows(0), cols(0) {}
    void create(int r, int c, int type) {
        const size_t bytes = (size_t)r * (size_t)c * (type == CV_32F ? 4 : 1);
        if (buf && r == rows && c == cols && buf->size() == bytes) return;
        buf = std::make_shared<std::vector<unsigned char>>(bytes, (unsigned char)0);
        rows = r;
        cols = c;
    }
    static Mat zeros(int r, int c, int type) {
        Mat m;
        m.create(r, c, type);
        return m;
    }
    Mat clone() const {
        Mat m;
        m.rows = rows;
        m.cols = cols;
        if (buf) m.buf = std::make_shared<std::vector<unsigned char>>(*buf);
        return m;
    }
    void release() {
        buf.reset();
        rows = cols = 0;
    }
    bool empty() const { return !buf || buf->empty(); }
    template <class T> T* ptr(int row = 0) { return (T*)(buf->data() + (size_t)row * rowBytes()); }
    template <class T> const T* ptr(int row = 0) const { return (const T*)(buf->data() + (size_t)row * rowBytes()); }

private:
    size_t rowBytes() const { return rows ? buf->size() / (size_t)rows : 0; }
    std::shared_ptr<std::vector<unsigned char>> buf;  // copies share the bytes, as cv::Mat's do
};

class FileNode {
public:
    FileNode operator[](const std::string&) const { return FileNode(); }
    FileNode operator[](const char*) const { return FileNode(); }
    FileNode operator[](int) const { return FileNode(); }
    size_t size() const { return 0; }
    operator int() const { return 0; }
    operator double() const { return 0.0; }
    operator std::string() const { return std::string(); }
};

class FileStorage {
public:
    enum { READ = 0, WRITE = 1 };
    FileStorage(const std::string&, int) {}
    bool isOpened() const { return false; }
    FileNode operator[](const std::string&) const { return FileNode(); }
};
template <class T> FileStorage& operator<<(FileStorage& fs, const T&) { return fs; }

}  // namespace cv
#endif
