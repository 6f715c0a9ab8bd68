// csrc/orb_rot_hist.h, the matchers' rotation filter, compiled for the host (build/librot_hist_host.so,
// tests/test_rot_hist_host.py; with -DROT_HIST_HOST_MAIN a program that runs both functions on heap
// buffers of exactly the sizes they read and write, which is what the sanitizer run executes).
#include <stdio.h>

#include <vector>

#include "../../orbslam_jpminipc_amd/csrc/orb_rot_hist.h"

extern "C" {

int rot_hist_length() { return orb_rot::HISTO_LENGTH; }

// out[i] = rot_bin(a1[i], a2[i])
void rot_hist_rot_bin(const float* a1, const float* a2, int n, int* out) {
    for (int i = 0; i < n; ++i) out[i] = orb_rot::rot_bin(a1[i], a2[i]);
}

// ind[3 i .. 3 i + 2] = three_maxima of the HISTO_LENGTH counts at hist[HISTO_LENGTH * i]
void rot_hist_three_maxima(const int* hist, int n, int* ind) {
    for (int i = 0; i < n; ++i) orb_rot::three_maxima(hist + (size_t)orb_rot::HISTO_LENGTH * i, ind + 3 * i);
}

}  // extern "C"

#ifdef ROT_HIST_HOST_MAIN
int main() {
    constexpr int H = orb_rot::HISTO_LENGTH;
    int bad = 0;
    // every boundary 15 + 30 k and its neighbours, the -0 and the 360 wrap
    std::vector<float> a1, a2;
    for (int k = 0; k < 12; ++k)
        for (float d : {-1.0f, 0.0f, 1.0f}) a1.push_back(15.0f + 30.0f * k + d), a2.push_back(0.0f);
    a1.push_back(-0.0f), a2.push_back(0.0f);
    a1.push_back(0.0f), a2.push_back(1e-40f);
    a1.push_back(0.0f), a2.push_back(15.0f);
    std::vector<int> bins(a1.size());
    rot_hist_rot_bin(a1.data(), a2.data(), (int)a1.size(), bins.data());
    for (int k = 0; k < 12; ++k) bad += bins[3 * k] != k || bins[3 * k + 1] != k + 1 || bins[3 * k + 2] != k + 1;
    bad += bins[36] != 0 || bins[37] != 12 || bins[38] != 12;
    for (int b : bins) bad += b < 0 || b >= H;
    // empty, one bin, the last bin the largest (every earlier one shifted), a dropped third
    std::vector<int> hist(4 * H, 0), ind(4 * 3, 7);
    hist[H + 29] = 1;
    for (int i = 0; i < H; ++i) hist[2 * H + i] = i + 1;
    hist[3 * H + 4] = 30, hist[3 * H + 9] = 3, hist[3 * H + 20] = 2;
    rot_hist_three_maxima(hist.data(), 4, ind.data());
    const int want[12] = {-1, -1, -1, 29, -1, -1, 29, 28, 27, 4, 9, -1};
    for (int i = 0; i < 12; ++i) bad += ind[i] != want[i];
    printf("status %d\n", bad);
    return bad ? 1 : 0;
}
#endif
