// orb_staging.h — the layout of one block of memory as 256-byte aligned regions handed out in call
// order.  No HIP here: the arithmetic is plain C++ (tests/native/staging_host.cpp pins it).
#pragma once
#include <assert.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

// Sizes of the regions of a staging buffer or a scratch allocation: rounded up to 256 B.
inline size_t orb_align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Regions of one block.  Without a base it only counts (the sizing pass: take() gives NULL and `end`
// is the block's size); with one it gives the pointers.  A function that names its regions on an
// OrbLayout& therefore yields both, from the same statements.  A region of 0 bytes occupies nothing.
struct OrbLayout {
    uint8_t* base;
    size_t end = 0;
    explicit OrbLayout(void* b = nullptr) : base((uint8_t*)b) {}
    size_t add(size_t bytes) {
        const size_t o = end;
        end = orb_align256(end + bytes);
        return o;
    }
    template <class T>
    T* take(size_t count) {
        const size_t o = add(count * sizeof(T));
        return base ? (T*)(base + o) : nullptr;
    }
    // the caller's array where it gave one, else `count` elements of this block
    template <class T>
    T* given_or_take(T* given, size_t count) {
        return given ? given : take<T>(count);
    }
};

// The size of the block whose regions `regions(OrbLayout&)` names.
template <class F>
size_t orb_layout_size(F&& regions) {
    OrbLayout L;
    regions(L);
    return L.end;
}

// `count` elements of T at `off` of a planned arena.  Only an OrbStage turns it into a pointer.
template <class T>
struct OrbRegion {
    size_t off, count;
    size_t bytes() const { return count * sizeof(T); }
};

// The arena of one host call, declared before any memory is touched: the inputs (copied to the device in
// one piece), then the outputs (copied back in one piece), then scratch that only the device holds.
// A plan has no pointers to give: the arena is grow-only and may move until the call has reserved it.
class OrbStagePlan {
    OrbLayout L_;
    size_t in_end_ = 0, out_end_ = 0;
    int span_ = 0;
    template <class T>
    OrbRegion<T> add(int span, size_t count) {
        assert(span >= span_ && "regions are declared in the order in, out, scratch");
        span_ = span;
        const OrbRegion<T> r{L_.add(count * sizeof(T)), count};
        if (span == 0) in_end_ = L_.end;
        if (span <= 1) out_end_ = L_.end;
        return r;
    }

public:
    template <class T>
    OrbRegion<T> in(size_t count) {
        return add<T>(0, count);
    }
    template <class T>
    OrbRegion<T> out(size_t count) {
        return add<T>(1, count);
    }
    template <class T>
    OrbRegion<T> scratch(size_t count) {
        return add<T>(2, count);
    }
    size_t in_end() const { return in_end_; }    // [0, in_end): host -> device
    size_t out_end() const { return out_end_; }  // [in_end, out_end): device -> host; the host staging ends here
    size_t total() const { return L_.end; }      // the device arena
};

// A plan bound to the memory that was reserved for it: `dev` of total() bytes, `host` of out_end().
class OrbStage {
protected:
    uint8_t *d_ = nullptr, *h_ = nullptr;
    size_t in_end_ = 0, out_end_ = 0;
    OrbStage() = default;
    void bind(const OrbStagePlan& p, uint8_t* dev, uint8_t* host) {
        d_ = dev, h_ = host, in_end_ = p.in_end(), out_end_ = p.out_end();
    }

public:
    OrbStage(const OrbStagePlan& p, void* dev, void* host) { bind(p, (uint8_t*)dev, (uint8_t*)host); }
    template <class T>
    T* dev(OrbRegion<T> r) const {
        return (T*)(d_ + r.off);
    }
    // the staged copy of an in or out region (scratch has none)
    template <class T>
    T* host(OrbRegion<T> r) const {
        assert(r.off + r.bytes() <= out_end_);
        return (T*)(h_ + r.off);
    }
    void zero_in() const { memset(h_, 0, in_end_); }
    // the first `count` elements from `src`, or zeros where `src` is NULL
    template <class T>
    void put(OrbRegion<T> r, const T* src, size_t count) const {
        assert(count <= r.count && r.off + r.bytes() <= in_end_);
        if (!count) return;
        if (src) memcpy(h_ + r.off, src, count * sizeof(T));
        else memset(h_ + r.off, 0, count * sizeof(T));
    }
    template <class T>
    void put(OrbRegion<T> r, const T* src) const {
        put(r, src, r.count);
    }
    // put(), and the region's device pointer for the argument struct
    template <class T>
    const T* send(OrbRegion<T> r, const T* src) const {
        put(r, src);
        return dev(r);
    }
    // `count` elements from element `first` on to `dst`, unless it is NULL
    template <class T>
    void get(OrbRegion<T> r, T* dst, size_t count, size_t first = 0) const {
        assert(first + count <= r.count && r.off >= in_end_);
        if (dst && count) memcpy(dst, host(r) + first, count * sizeof(T));
    }
    template <class T>
    void get(OrbRegion<T> r, T* dst) const {
        get(r, dst, r.count);
    }
};
