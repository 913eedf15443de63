// The arithmetic of object keypoint similarity that oks.hip and track_eval.hip (detections against ground truth) and
// pose_track.hip (detections against the tracks of the previous frames) share: COCO's per-keypoint variances, one keypoint's exp term and the area of a
// keypoint set's bounding box. IEEE float64 in COCOeval's order, contraction off; exp is the device library's (<= 1 ulp).
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kOksKeypoints = 17;

// cocoeval.py Params.setKpParams: kpt_oks_sigmas; computeOks: vars = (sigmas * 2)**2
#define S(x) (((x) / 10.0 * 2) * ((x) / 10.0 * 2))
__constant__ double kVars[kOksKeypoints] = {S(.26), S(.25), S(.25), S(.35), S(.35), S(.79), S(.79), S(.72), S(.72), S(.62), S(.62),
                                            S(1.07), S(1.07), S(.87), S(.87), S(.89), S(.89)};
#undef S
constexpr double kEps = 2.220446049250313e-16;      // np.spacing(1)

// computeOks, one keypoint: exp(-e), e = (dx^2 + dy^2) / vars[k] / (area + eps) / 2; denom = area + eps
__device__ __forceinline__ double oks_term(double dx, double dy, int k, double denom) {
    const double e = (dx * dx + dy * dy) / kVars[k] / denom / 2;
    return exp(-e);
}

// The score a record row's detection is ordered by (mpn_oks_match's and mpn_pose_nms's score_mode), in f32: 0 the box score;
// 1 the box score * (sum of the row's 17 keypoint_scores in order / 17)
__device__ __forceinline__ float order_score(float box_score, const float* keypoint_scores, int score_mode) {
    if (score_mode != 1) return box_score;
    float m = 0.f;
    for (int k = 0; k < kOksKeypoints; ++k) m += keypoint_scores[k];
    return box_score * (m / 17.0f);
}

// (max x - min x) * (max y - min y) of keypoints[17][3] = (x, y, score): min / max in f32, the differences and the product in f64
// (kStride = 2: of keypoints[17][2] = (x, y))
template <int kStride = 3>
__device__ __forceinline__ double keypoint_extent_area(const float* kp) {
    float xl = kp[0], xh = kp[0], yl = kp[1], yh = kp[1];
    for (int k = 1; k < kOksKeypoints; ++k) {
        xl = fminf(xl, kp[kStride * k]); xh = fmaxf(xh, kp[kStride * k]);
        yl = fminf(yl, kp[kStride * k + 1]); yh = fmaxf(yh, kp[kStride * k + 1]);
    }
    return ((double)xh - (double)xl) * ((double)yh - (double)yl);
}

// a ground-truth row of mpn_oks_match and mpn_track_eval, in doubles: keypoints[17][3] (x, y, v), bbox (x, y, w, h), area,
// ignore, iscrowd, padding
constexpr int kGtDoubles = 64, kGtBox = 51, kGtArea = 55, kGtIgnore = 56, kGtCrowd = 57;

// computeOks for one (detection, ground truth): kp = the record row's keypoints[17][3] (f32), g = the ground-truth row
__device__ inline double oks_of(const float* kp, const double* g) {
    int k1 = 0;
    for (int k = 0; k < kOksKeypoints; ++k) k1 += g[3 * k + 2] > 0.0;
    const double bx = g[kGtBox], by = g[kGtBox + 1], bw = g[kGtBox + 2], bh = g[kGtBox + 3];
    const double x0 = bx - bw, x1 = bx + bw * 2, y0 = by - bh, y1 = by + bh * 2;
    const double denom = g[kGtArea] + kEps;
    double sum = 0.0;
    for (int k = 0; k < kOksKeypoints; ++k) {
        const double xd = (double)kp[3 * k], yd = (double)kp[3 * k + 1];
        double dx, dy;
        if (k1 > 0) {
            if (!(g[3 * k + 2] > 0.0)) continue;
            dx = xd - g[3 * k];
            dy = yd - g[3 * k + 1];
        } else {
            dx = fmax(0.0, x0 - xd) + fmax(0.0, xd - x1);
            dy = fmax(0.0, y0 - yd) + fmax(0.0, yd - y1);
        }
        sum += oks_term(dx, dy, k, denom);
    }
    return sum / (double)(k1 > 0 ? k1 : kOksKeypoints);
}

}  // namespace
