// The point that stands for a person of the record - the anchor C of mpn_zone_events (include/mpn.h) - in one place for every
// stage that asks where a person is: zone_events.hip, trails.hip, density.hip. Every operation is one IEEE f64 operation in the
// order written here, f32 inputs widened first; the including file turns contraction off (#pragma clang fp contract(off)).
#pragma once

namespace mpn_anchor {

constexpr int kOffBox = 1, kOffKeypoints = 57;                    // of a record row, in f32 words
constexpr int kLeftAnkle = 15, kRightAnkle = 16;
constexpr unsigned kFlagAnkles = 2u, kFlagNoAnchor = 4u;          // bits 1 and 2 of every stage's row flags

__device__ __forceinline__ bool finite64(double v) { return v - v == 0.0; }      // (inf - inf and nan - nan are nan)

// row: a record row. anchor_mode: 0 feet, 2 box_centre, anything else box_bottom. -> kFlagAnkles, kFlagNoAnchor or 0; cx, cy are
// the anchor, (0, 0) where there is none.
__device__ __forceinline__ unsigned person_anchor(const float* row, int anchor_mode, double min_score, double height, double width,
                                                 double& cx, double& cy) {
    const double ymin = (double)row[kOffBox], xmin = (double)row[kOffBox + 1];
    const double ymax = (double)row[kOffBox + 2], xmax = (double)row[kOffBox + 3];
    const float* la = row + kOffKeypoints + 3 * kLeftAnkle;
    const float* ra = row + kOffKeypoints + 3 * kRightAnkle;
    const bool left = anchor_mode == 0 && (double)la[2] >= min_score;
    const bool right = anchor_mode == 0 && (double)ra[2] >= min_score;
    if (left && right) {
        cx = ((double)la[0] + (double)ra[0]) * 0.5;
        cy = ((double)la[1] + (double)ra[1]) * 0.5;
    } else if (left) {
        cx = (double)la[0]; cy = (double)la[1];
    } else if (right) {
        cx = (double)ra[0]; cy = (double)ra[1];
    } else {
        cx = (xmin + xmax) * 0.5 * width;
        cy = anchor_mode == 2 ? (ymin + ymax) * 0.5 * height : ymax * height;
    }
    if (!finite64(cx) || !finite64(cy)) { cx = 0.0; cy = 0.0; return kFlagNoAnchor; }
    return (left || right) ? kFlagAnkles : 0u;
}

}  // namespace mpn_anchor
