// orb_extract_geom.h — the HIP-free part of what the extraction units share: the geometry structs
// the host plans (orb_extract_plan.h) and the kernels take by value, the size constants both sides
// use, and the border rule.  No HIP header: it compiles with a plain C++ compiler, so the planner
// can be tested and sanitized on the host (tests/native/extract_plan_host.cpp).  orb_extract.h adds
// the device helpers and orb_ilp.hip's launchers; orb_device.h takes EDGE and reflect101 from here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define ORB_HOST_DEVICE __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define ORB_HOST_DEVICE inline
#endif

namespace orbdev {

constexpr int EDGE = 16;           // EDGE_THRESHOLD, ORBextractor.cc:77

// cv::borderInterpolate(p, len, BORDER_REFLECT_101) (OpenCV 2.4).
ORB_HOST_DEVICE int reflect101(int p, int len) {
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        p = p < 0 ? -p : 2 * len - 2 - p;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

}  // namespace orbdev

#define ORB_MAX_LEVELS 16
#define ORB_MAX_CELLS_PER_LEVEL 256

// ---- geometry (host-computed, passed to kernels by value) ---------------------------------
struct LevelGeom {
    int w, h, pitch, ph;    // ROI size, padded row pitch, padded rows (h + 32)
    long long base;         // byte offset of this level's frame-0 buffer in the pyramid
    long long fstride;      // bytes per frame of this level (pitch * ph)
    int rows, cols;         // cell grid (reference naming: levelRows x levelCols)
    int cell0;              // first cell of the level in the per-frame cell table
    int nDesired, nfc;      // mnFeaturesPerLevel[l], nfeaturesCell
    int kpBase;             // offset of the level's slot in the per-frame keypoint list
    int xsimd_blur;         // 4 * floor(w / 4): GaussianBlur SSE2 columns
    int xs_resize, xmax;    // VResizeLinear SSE2 columns, HResizeLinear xmax (l >= 1)
    int rtab;               // offset of this level's resize table (int32 units), l >= 1
    int rtile;              // offset of this level's resize tile table (4 ints per tile), l >= 1
    int rtileS;             // the same for the short tiles of small batches (RZ_THS rows)
    float scale;            // mvScaleFactor[l]
    float size;             // (int)(31 * mvScaleFactor[l])
    int cellW, cellH;       // detection-area size of the (non-last) cells: corner -> cell bucket
    int cellWm, cellHm;     // ceil(2^32 / cellW), ceil(2^32 / cellH): n / cell = umulhi(n, m), n < 4096
                            // (2^32 - 1 for a 1-px cell, applied to n + 1: ceil(2^32 / 1) does not fit)
    int candBase, capMax;   // cell c of the level owns candidate slots candBase + c * capMax (capMax = the
                            // level's largest NMS-survivor bound), so k_fast needs no cell table
    int detX1, detY1;       // FAST detection region [16, detX1) x [16, detY1): union of the cells' areas
    int ringX1, ringY1;     // rBRIEF samples (reach 18) of detection-region keypoints stay in
                            // [-3, ringX1) x [-3, ringY1), inside the 16-px padding
};

struct Geom {
    int L;
    int nCells;        // cells per frame (all levels)
    int candPerFrame;  // candidate slots per frame (u32)
    int kpCap;         // keypoint slots per frame (sum of nDesired)
    int selCap;        // k_select: survivors per level held in LDS (select_cap)
    int fastTh;        // clamped to [0, 255]
    int scoreType;
    int taps[4];       // Gaussian 7-tap fixed-point kernel, centre first: 55, 49, 34, 18
    int umax[16];
    unsigned long long umaxNib;  // umax[0..15] as 4-bit nibbles (k_orient_desc's disc mask)
    uint32_t odDivMagic;          // k_orient_desc: ceil(2^32 / slot groups per frame) (exact division)
    int fastCl;                   // k_fast: per-wave corner-list capacity used (FT_CL; smaller only via
                                  // orb_debug_set_fast_corner_list, to exercise the plane-scan fallback)
    LevelGeom lv[ORB_MAX_LEVELS];
};

struct CellGeom {
    int level;
    int x0, y0, hx, hy;  // ROI in level coordinates (reference iniX, iniY, hX, hY)
    int cap;             // max NMS survivors: ceil(dw/2) * ceil(dh/2)
    int candOff;         // offset in the frame's candidate area
    int skipped;         // reference `continue` on hX/hY <= 0 (nTotal stays 0, bNoMore false)
    int cornerOff;       // bucket of this cell's FAST corners in the frame's corner area (dw*dh slots)
};

// ---- k_pyr_stream: the plan plan_stream makes for it (orb_extract_plan.h) -------------------
struct StreamLevel {
    int nq;             // tasks per row: 16-B chunks (level 0) / 4-px quads (l >= 1) of the padded row
    uint32_t nqm;       // ceil(2^32 / nq): row = umulhi(task, nqm) (exact for the task counts used)
    int ringOff;        // LDS byte offset of the level's ring of ROI rows (levels < L-1)
    int ringPitch;      // its row pitch (bytes, multiple of 16)
    int colOff;         // LDS byte offset of the level's column words (l >= 1; 16 B per quad)
    int waveStart, nWaves;  // the workgroup's waves that build this level
    int w, h, pitch;
    long long base, fstride;
};
struct StreamGeom {
    int L, nRounds;
    int u0;             // 16-B units per level-0 ROI row
    uint32_t u0m;       // ceil(2^32 / u0)
    int align;          // input alignment: 16 / 4 / 1 (pointer, stride and frame pitch)
    int colWords;       // u32 column words of all levels (LDS-resident)
    int colOff;         // LDS byte offset of the column words
    int rowOff;         // LDS byte offset of the two row-entry stages (rowStride uint2 each)
    int rowStride;      // row entries per stage (the most any round has)
    int cap0;           // level-0 ring rows (row r in slot r % cap0)
};
#define PS_THREADS 1024
#ifndef PS_LOADERS
#define PS_LOADERS 2  // loader waves per workgroup
#endif
#define PS_NPF 8     // level-0 units (and row entries) per loader lane and round: K0 * u0 <= 1024

// ---- k_fast: tile sizes and the host-built tile table ---------------------------------------
#define FT_TW_MAX 256     // detection columns per tile at most (64 lanes x 4 pixels)
#define FT_IN_BYTES 12672  // staged-tile LDS budget (44 rows of 288 B at TW = 256)
#define FT_S_BYTES 10032   // strength-plane LDS budget (38 rows of 264 B at TW = 256; a multiple of 16)
static_assert(FT_S_BYTES % 16 == 0 && FT_IN_BYTES % 16 == 0, "k_fast's LDS buffers are cleared / staged in 16-B units");
#define FT_Q 512           // per-wave queue (u16 entries): dwords, then the NMS corner list
#define FT_CQ 320          // per-wave pixel list (u16 entries): < 64 carried + 256 expanded
#define FT_CL 256          // per-wave corner list (u16 entries) filled by the strength passes; a
                           // workgroup where a wave has more corners scans the strength plane instead
                           // (Geom::fastCl lowers the cap for the fallback's parity test)
struct FastTile {
    int level, x0, y0;  // detection origin (level coordinates); x0 = 16 + k TW, a multiple of 4
    int tw4, th;        // dwords per row (>= 2), rows (clipped to the detection region)
    int sp, sx;         // staged row pitch (bytes, a multiple of 16); x0 - first staged column (8 .. 23)
    uint32_t rcpF;      // ceil(2^32 / (tw4 + 2)): flattened ring index -> plane row
    uint32_t rcpI;      // ceil(2^32 / tw4): interior index -> row
    uint32_t rcpU;      // ceil(2^32 / (sp / 16)): staged unit -> row
};
