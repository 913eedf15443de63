// COCO keypoint evaluation on the device: object keypoint similarity (OKS) and COCOeval's greedy matching for
// iouType='keypoints' (pycocotools cocoeval.py, computeOks and evaluateImg), over the record mpn_pose_gather wrote.
//   mpn_oks_match   record (read in place) + ground truth f64 [B, max_gt, 64] -> one fixed-stride row per record row:
//                   {rank, score, area, match[3][10], ignore[3]}; optionally the OKS matrix [row][max_gt].
// ONE block per image; an image's result depends on nothing but its own rows, there are no atomics.
//   phase 0  detection score (box, or box * mean keypoint score), area of the keypoints' bounding box, rank = the place in the
//            stable descending order of the scores (a count over the image's <= 256 detections)
//   phase 1  the OKS of the first max_dets detections against every ground truth -> LDS (20 x 64 doubles = 10 KB)
//   phase 2  per area range the ground-truth order (not ignored first, stable); then ONE lane per (range, threshold), 30
//            lanes, each walks COCOeval's greedy loop over LDS with its matched set in a 64-bit mask
//   phase 3  the rows: ignore flags gathered into bitmasks, matches as indices in the image's original ground-truth order
// All arithmetic is IEEE float64 in COCOeval's order, contraction off; exp is the device library's (<= 1 ulp).
// Latency-bound glue like mpn_pose_gather (B blocks of work measured in microseconds): not tuned, and not worth tuning.
#include "common.h"
#include "oks_math.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxGt = 64;              // the matched set of a lane is one 64-bit mask
constexpr int kMaxDets = 20;            // rows of the OKS matrix in LDS
constexpr int kMaxT = 10;               // thresholds a row has room for
constexpr int kRanges = 3;
constexpr int kMaxBoxes = 256;          // detections of one image (LDS tables of scores and ranks)
constexpr int kMaxRows = 4096;          // mpn_pose_gather's own limit on B * max_boxes
// the record's row (pose_gather.hip), in 32-bit words
constexpr int kRowWords = 108, kOffScore = 5, kOffKScore = 6, kOffKeypoints = 57;
// an output row, in bytes: int32 rank, f32 score, f64 area, int32 match[3][10], uint32 ignore[3], 4 bytes of padding
constexpr int kOutBytes = 152, kOutMatch = 16, kOutIgnore = kOutMatch + 4 * kRanges * kMaxT;
static_assert(kOutIgnore + 4 * kRanges + 4 == kOutBytes && kOutBytes % 8 == 0, "output row layout");

inline size_t header_words(int B) { return ((size_t)(2 * B + 2) + 3) / 4 * 4; }

// Params.setKpParams: areaRng all, medium, large
__constant__ double kAreaLo[kRanges] = {0.0, 32.0 * 32.0, 96.0 * 96.0};
__constant__ double kAreaHi[kRanges] = {1e5 * 1e5, 96.0 * 96.0, 1e5 * 1e5};

struct OksArgs {
    const int* header;
    const float* rows;
    const double* gt;
    const int* gt_counts;
    const double* thresholds;
    unsigned char* out;
    double* oks_out;
    int B, max_boxes, max_gt, num_thresholds, score_mode, max_dets;
};

__global__ __launch_bounds__(kThreads) void oks_match_kernel(OksArgs a) {
    __shared__ double oks[kMaxDets][kMaxGt];
    __shared__ double area[kMaxBoxes];
    __shared__ float score[kMaxBoxes];
    __shared__ int rank[kMaxBoxes];
    __shared__ int order[kMaxDets];                       // detection of rank r
    __shared__ int gorder[kRanges][kMaxGt];               // ground truth at place p of a range's order
    __shared__ unsigned char gignore[kRanges][kMaxGt];    // ignore flag of ground truth g in a range (original order)
    __shared__ unsigned char dignore[kRanges][kMaxT][kMaxDets];
    __shared__ int dmatch[kRanges][kMaxT][kMaxDets];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int all_rows = a.B * a.max_boxes;
    const int T = a.num_thresholds;

    // this image's rows of the record (counts are the gather's own; clamped, so that nothing is indexed out of range)
    int total = a.header[0], first = 0;
    total = total < 0 ? 0 : (total > all_rows ? all_rows : total);
    for (int i = 0; i < b; ++i) first += a.header[1 + i] > 0 ? a.header[1 + i] : 0;
    int n = a.header[1 + b];
    n = n < 0 ? 0 : (n > a.max_boxes ? a.max_boxes : n);
    if (first > total) first = total;
    if (first + n > total) n = total - first;
    int ng = a.gt_counts[b];
    ng = ng < 0 ? 0 : (ng > a.max_gt ? a.max_gt : ng);
    const double* gt = a.gt + (size_t)b * a.max_gt * kGtDoubles;
    const int nd = n < a.max_dets ? n : a.max_dets;

    // rows behind the record's total are zero: the blocks share them
    for (long long w = (long long)total * (kOutBytes / 4) + b * kThreads + tid; w < (long long)all_rows * (kOutBytes / 4);
         w += (long long)a.B * kThreads)
        ((unsigned*)a.out)[w] = 0u;
    if (a.oks_out)
        for (long long w = (long long)total * a.max_gt + b * kThreads + tid; w < (long long)all_rows * a.max_gt;
             w += (long long)a.B * kThreads)
            a.oks_out[w] = 0.0;

    // phase 0
    for (int i = tid; i < n; i += kThreads) {
        const float* row = a.rows + (size_t)(first + i) * kRowWords;
        score[i] = order_score(row[kOffScore], row + kOffKScore, a.score_mode);
        area[i] = keypoint_extent_area(row + kOffKeypoints);
    }
    __syncthreads();
    for (int i = tid; i < n; i += kThreads) {
        const float s = score[i];
        int r = 0;
        for (int j = 0; j < n; ++j) r += (score[j] > s) || (score[j] == s && j < i);
        rank[i] = r;
        if (r < nd) order[r] = i;
    }
    // the ground-truth ignore flags and orders of the three ranges
    for (int i = tid; i < kRanges * ng; i += kThreads) {
        const int r = i / ng, g = i - r * ng;
        const double ga = gt[g * kGtDoubles + kGtArea];
        gignore[r][g] = (gt[g * kGtDoubles + kGtIgnore] != 0.0) || ga < kAreaLo[r] || ga > kAreaHi[r];
    }
    __syncthreads();
    for (int i = tid; i < kRanges * ng; i += kThreads) {
        const int r = i / ng, g = i - r * ng;
        int kept_before = 0, ignored_before = 0, kept = 0;
        for (int j = 0; j < ng; ++j) {
            const int ig = gignore[r][j];
            kept += !ig;
            if (j < g) { kept_before += !ig; ignored_before += ig; }
        }
        gorder[r][gignore[r][g] ? kept + ignored_before : kept_before] = g;
    }
    // phase 1
    for (int i = tid; i < nd * ng; i += kThreads) {
        const int d = i / ng, g = i - d * ng;
        const float* kp = a.rows + (size_t)(first + order[d]) * kRowWords + kOffKeypoints;
        oks[d][g] = oks_of(kp, gt + g * kGtDoubles);
    }
    __syncthreads();

    // phase 2: evaluateImg's loops for one (range, threshold)
    if (tid < kRanges * T) {
        const int r = tid / T, t = tid - r * T;
        const double thr = fmin(a.thresholds[t], 1 - 1e-10);
        unsigned long long matched = 0ull;
        for (int d = 0; d < nd; ++d) {
            double iou = thr;
            int m = -1;
            for (int p = 0; p < ng; ++p) {
                const int g = gorder[r][p];
                if (((matched >> p) & 1ull) && !(gt[g * kGtDoubles + kGtCrowd] != 0.0)) continue;
                if (m >= 0 && !gignore[r][gorder[r][m]] && gignore[r][g]) break;
                if (oks[d][g] < iou) continue;
                iou = oks[d][g];
                m = p;
            }
            int ig;
            if (m >= 0) {
                matched |= 1ull << m;
                ig = gignore[r][gorder[r][m]];
            } else {
                const double da = area[order[d]];
                ig = da < kAreaLo[r] || da > kAreaHi[r];
            }
            dmatch[r][t][d] = m >= 0 ? gorder[r][m] : -1;
            dignore[r][t][d] = (unsigned char)ig;
        }
    }
    __syncthreads();

    // phase 3
    for (int i = tid; i < n; i += kThreads) {
        unsigned char* o = a.out + (size_t)(first + i) * kOutBytes;
        const int d = rank[i];
        *(int*)o = d;
        *(float*)(o + 4) = score[i];
        *(double*)(o + 8) = area[i];
        int* mt = (int*)(o + kOutMatch);
        unsigned* ig = (unsigned*)(o + kOutIgnore);
        for (int r = 0; r < kRanges; ++r) {
            unsigned bits = 0u;
            for (int t = 0; t < kMaxT; ++t) {
                const bool live = d < nd && t < T;
                mt[r * kMaxT + t] = live ? dmatch[r][t][d] : -1;
                if (live && dignore[r][t][d]) bits |= 1u << t;
            }
            ig[r] = bits;
        }
        ig[kRanges] = 0u;
        if (a.oks_out) {
            double* q = a.oks_out + (size_t)(first + i) * a.max_gt;
            for (int g = 0; g < a.max_gt; ++g) q[g] = (d < nd && g < ng) ? oks[d][g] : 0.0;
        }
    }
}

}  // namespace

extern "C" size_t mpn_oks_gt_row_bytes(void) { return kGtDoubles * sizeof(double); }

extern "C" size_t mpn_oks_match_out_bytes(int B, int max_boxes) {
    if (B < 1 || max_boxes < 1 || max_boxes > kMaxBoxes || (long long)B * max_boxes > kMaxRows) return 0;
    return (size_t)B * max_boxes * kOutBytes;
}

extern "C" int mpn_oks_match(const void* record, int B, int max_boxes, const double* gt, const int* gt_counts, int max_gt,
                             const double* thresholds, int num_thresholds, int score_mode, int max_dets, void* out,
                             double* oks_out, mpn_stream_t stream) {
    MPN_REQUIRE(max_gt >= 1 && max_gt <= kMaxGt, MPN_ERR_BAD_SHAPE,
                "oks_match: max_gt = %d, a lane keeps its matched set in %d bits", max_gt, kMaxGt);
    MPN_REQUIRE(record && gt && gt_counts && thresholds && out, MPN_ERR_BAD_ARG, "oks_match: null pointer");
    MPN_REQUIRE(B >= 1 && max_boxes >= 1 && max_boxes <= kMaxBoxes && (long long)B * max_boxes <= kMaxRows, MPN_ERR_BAD_SHAPE,
                "oks_match: B = %d, max_boxes = %d (at most %d per image, %d rows)", B, max_boxes, kMaxBoxes, kMaxRows);
    MPN_REQUIRE(num_thresholds >= 1 && num_thresholds <= kMaxT, MPN_ERR_BAD_SHAPE,
                "oks_match: num_thresholds = %d, a row holds %d", num_thresholds, kMaxT);
    MPN_REQUIRE(max_dets >= 1 && max_dets <= kMaxDets, MPN_ERR_BAD_SHAPE,
                "oks_match: max_dets = %d, the OKS matrix in LDS has %d rows", max_dets, kMaxDets);
    MPN_REQUIRE(score_mode == 0 || score_mode == 1, MPN_ERR_BAD_ARG, "oks_match: score_mode must be 0 or 1");
    MPN_REQUIRE(mpn_aligned16(record) && (((uintptr_t)gt | (uintptr_t)thresholds | (uintptr_t)out | (uintptr_t)oks_out) & 7u) == 0,
                MPN_ERR_BAD_ALIGN, "oks_match: record must be 16-byte, gt / thresholds / out / oks_out 8-byte aligned");
    OksArgs a = {(const int*)record, (const float*)((const char*)record + header_words(B) * 4), gt, gt_counts, thresholds,
                 (unsigned char*)out, oks_out, B, max_boxes, max_gt, num_thresholds, score_mode, max_dets};
    oks_match_kernel<<<B, kThreads, 0, (hipStream_t)stream>>>(a);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
