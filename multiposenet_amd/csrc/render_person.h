// Per-person tables of the Gaussian target blobs (reference detector/input_pipeline/heatmap_creation.py), shared by the
// batched renderer (render.hip) and the PRN example generator (prn_examples.hip):
//   g[p][d]      = exp(-d^2 / (2 sigma_p^2)), d = 0..k_p (float64), 0 beyond k_p
//   half[p]      = k_p = ceil(sqrt(-2 sigma_p^2 ln 0.01))
//   centre[p][j] = (cy, cx) of keypoint j on the downsampled map; cy == kInvisible for an invisible keypoint
// A map value is max(0, max over visible persons of float32(g[|y-cy|] * g[|x-cx|])) for |dy|, |dx| <= k.
#pragma once
#include "common.h"

namespace {

constexpr int kParts = 17;
constexpr int kMaxHalf = 13;                 // sigma <= 4  ->  k = ceil(sqrt(2*16*ln 100)) = 13
constexpr int kG = 16;                       // doubles per person in the window table (g[0..13], padded)
constexpr int kChunk = 60;                   // persons per culling pass (60*17 = 1020 candidate blobs)
constexpr int kInvisible = 0x7fffffff;

struct RenderTables {
    double* g;      // [P][kG]
    int2* centre;   // [P][17]  (cy, cx); cy == kInvisible for an invisible keypoint
    int* half;      // [P]
};

__host__ __device__ inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

inline size_t render_tables_bytes(int total_persons) {
    if (total_persons <= 0) return 16;
    const size_t P = (size_t)total_persons;
    return align16(P * kG * sizeof(double)) + align16(P * kParts * sizeof(int2)) + align16(P * sizeof(int));
}

inline RenderTables carve(void* ws, int P) {
    RenderTables t;
    unsigned char* p = reinterpret_cast<unsigned char*>(ws);
    t.g = reinterpret_cast<double*>(p);
    p += align16((size_t)P * kG * sizeof(double));
    t.centre = reinterpret_cast<int2*>(p);
    p += align16((size_t)P * kParts * sizeof(int2));
    t.half = reinterpret_cast<int*>(p);
    return t;
}

// Entry i = p * 17 + j of the tables. heatmap_creation.py:30-37,78-84: per-person sigma, half window k and the 1-D
// window; :23-24,57,104-107: centres, with hm1 = float(height - 1), wm1 = float(width - 1) of the person's image and
// oh1 = float(h - 1), ow1 = float(w - 1) of its map.
__device__ __forceinline__ void render_prepare_entry(const int32_t* __restrict__ keypoints,
                                                     const float* __restrict__ boxes, int i, float hm1, float wm1,
                                                     float oh1, float ow1, const RenderTables& t) {
    // Every operation below is one IEEE-754 round-to-nearest step of the numpy code: no contraction into FMAs, and
    // sqrtf / operator/ are the correctly rounded forms (the __f*_rn intrinsics map to the approximate native ops).
#pragma clang fp contract(off)
    const int p = i / kParts, j = i - p * kParts;
    const float ymin = boxes[p * 4 + 0], xmin = boxes[p * 4 + 1], ymax = boxes[p * 4 + 2], xmax = boxes[p * 4 + 3];
    const float area = (ymax - ymin) * (xmax - xmin);
    float s = sqrtf(area) * 0.007f;
    s = fminf(fmaxf(s, 1.0f), 4.0f);
    const float s2 = s * s;
    // k = ceil(sqrt(float32(-2 s^2) * ln(0.01)))  in float64
    const double arg = (double)(-2.0f * s2) * -0x1.26bb1bbb55515p+2;
    int k = (int)ceil(sqrt(arg));
    k = k > kMaxHalf ? kMaxHalf : k;
    if (j == 0) t.half[p] = k;
    if (j <= kMaxHalf) {
        const double sig2 = (double)((2.0f * s) * s);
        t.g[p * kG + j] = j <= k ? exp(-(double)(j * j) / sig2) : 0.0;
    }
    const int32_t* kp = keypoints + (size_t)i * 3;   // (y, x, visibility)
    int2 c;
    if (kp[2] > 0) {
        const float ny = (float)kp[0] / hm1, nx = (float)kp[1] / wm1;
        c.x = (int)rintf(ny * oh1);
        c.y = (int)rintf(nx * ow1);
    } else {
        c.x = kInvisible;
        c.y = 0;
    }
    t.centre[i] = c;
}

}  // namespace
