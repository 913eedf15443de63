// Result packing of the batched joint inference graph (inference/detector.py:54-59 of the reference + the live-slot gather of
// create_pb.py:96-104, for a whole batch in one launch):
//   mpn_pose_gather   padded per-slot outputs of B images (NMS boxes / scores / counts, PRN keypoint scores / positions)
//                     -> ONE contiguous record: int32 header {total, counts[B], num_boxes[B], overflow} and B * max_boxes
//                     rows in (image, slot) order, kept rows first and dense, the rest zero.
//   mpn_pose_gather_sized   the same kernel body (template flag) for images resized onto the network canvas: per-image box
//                     scales and pixel sizes come from device memory (`extent`), the box is scaled to the source image first.
// A row is kept iff slot < num_boxes[image] and score > score_threshold. B * max_boxes is small (25 x 64 = 1 600 at the largest
// batch worth supporting): ONE block; a ballot / popcount exclusive scan over the keep flags (wave totals through LDS, in wave
// order: the destination of a row is a function of the flags alone - no atomics), then a cooperative copy in 16-byte stores.
// Slots >= num_boxes are never read. Latency-bound glue; arithmetic is plain IEEE f32 in the documented order (no contraction).
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxRows = 4096;          // LDS: two int tables of this many rows (32 KB)
constexpr int kK = 17;                  // keypoints per person
// a row, in 32-bit words: image_index (int32), box[4], score, keypoint_scores[17], keypoint_positions[17][2], keypoints[17][3]
constexpr int kOffBox = 1, kOffScore = 5, kOffKScore = 6, kOffKPos = kOffKScore + kK, kOffKeypoints = kOffKPos + 2 * kK;
constexpr int kRowWords = kOffKeypoints + 3 * kK;   // 108 words = 432 bytes = 27 16-byte vectors
static_assert(kRowWords % 4 == 0, "rows are written in 16-byte vectors");

// header words {total, counts[B], num_boxes[B], overflow}, rounded up to whole 16-byte vectors (the rows stay aligned)
inline size_t header_words(int B) { return ((size_t)(2 * B + 2) + 3) / 4 * 4; }

struct GatherArgs {
    const float* boxes;
    const float* scores;
    const int* num_boxes;
    const float* kscores;
    const float* kpos;
    const int* overflow;
    const float* extent;        // kSized: [B,4] (box_scale_y, box_scale_x, pixel_height, pixel_width); else height / width below
    float threshold, height, width;
    int B, max_boxes, header_words;
};

// coordinate j (ymin, xmin, ymax, xmax) of the record's box of slot r: mpn_pose_gather_sized scales it to the source image
template <bool kSized>
__device__ __forceinline__ float box_out(const GatherArgs& a, int r, int j) {
    const float v = a.boxes[r * 4 + j];
    if (!kSized) return v;
    return v * a.extent[(r / a.max_boxes) * 4 + (j & 1)];
}

// word f of the record row of source slot r
template <bool kSized>
__device__ __forceinline__ unsigned row_word(const GatherArgs& a, int r, int f) {
    if (f == 0) return (unsigned)(r / a.max_boxes);
    if (f < kOffScore) return __float_as_uint(box_out<kSized>(a, r, f - kOffBox));
    if (f == kOffScore) return __float_as_uint(a.scores[r]);
    if (f < kOffKPos) return a.kscores ? __float_as_uint(a.kscores[r * kK + (f - kOffKScore)]) : 0u;
    if (f < kOffKeypoints) return a.kpos ? __float_as_uint(a.kpos[r * 2 * kK + (f - kOffKPos)]) : 0u;
    const int k = (f - kOffKeypoints) / 3, c = (f - kOffKeypoints) - 3 * k;
    if (c == 2) return a.kscores ? __float_as_uint(a.kscores[r * kK + k]) : 0u;
    if (!a.kpos) return 0u;
    // inference/predict.ipynb, draw_everything: x = xmin * width + pos_x * (xmax * width - xmin * width); positions are (y, x)
    const float size = kSized ? a.extent[(r / a.max_boxes) * 4 + 3 - c] : (c == 0 ? a.width : a.height);
    const float lo = box_out<kSized>(a, r, 1 - c) * size;
    const float hi = box_out<kSized>(a, r, 3 - c) * size;
    const float p = a.kpos[(r * kK + k) * 2 + (1 - c)];
    const float span = hi - lo;
    const float off = p * span;
    return __float_as_uint(lo + off);
}

template <bool kSized>
__global__ __launch_bounds__(kThreads) void pose_gather_kernel(GatherArgs a, int* __restrict__ header, uint4* __restrict__ rows) {
    __shared__ int before[kMaxRows + 1];    // kept rows ahead of row r (exclusive scan; [n] = total)
    __shared__ int source[kMaxRows];        // record row j <- source slot
    __shared__ int wave_total[kWaves];
    const int n = a.B * a.max_boxes;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += kThreads) {     // (uniform trip count: every thread reaches the barriers)
        const int r = base + tid;
        bool keep = false;
        if (r < n) {
            const int img = r / a.max_boxes;
            if (r - img * a.max_boxes < a.num_boxes[img]) keep = a.scores[r] > a.threshold;    // strict; a NaN score is dropped
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_total[wave] = __popcll(m);
        __syncthreads();
        int ahead = 0, all = 0;
        for (int k = 0; k < kWaves; ++k) {
            const int t = wave_total[k];
            all += t;
            if (k < wave) ahead += t;
        }
        const int at = carry + ahead + __popcll(m & ((1ull << lane) - 1ull));
        if (r < n) {
            before[r] = at;
            if (keep) source[at] = r;
        }
        carry += all;
        __syncthreads();
    }
    const int total = carry;
    if (tid == 0) before[n] = total;
    __syncthreads();
    for (int i = tid; i < a.header_words; i += kThreads) {
        int v = 0;
        if (i == 0) v = total;
        else if (i <= a.B) v = before[i * a.max_boxes] - before[(i - 1) * a.max_boxes];
        else if (i <= 2 * a.B) v = a.num_boxes[i - 1 - a.B];
        else if (i == 2 * a.B + 1) v = a.overflow ? *a.overflow : 0;
        header[i] = v;
    }
    constexpr int kRowVecs = kRowWords / 4;
    const int nvec = n * kRowVecs;
    for (int v = tid; v < nvec; v += kThreads) {
        const int j = v / kRowVecs, f = (v - j * kRowVecs) * 4;
        uint4 o = make_uint4(0u, 0u, 0u, 0u);
        if (j < total) {
            const int r = source[j];
            o = make_uint4(row_word<kSized>(a, r, f), row_word<kSized>(a, r, f + 1), row_word<kSized>(a, r, f + 2), row_word<kSized>(a, r, f + 3));
        }
        rows[v] = o;
    }
}

}  // namespace

extern "C" size_t mpn_pose_gather_row_offset(int B, int max_boxes, int row) {
    if (B < 1 || max_boxes < 1 || row < 0 || (long long)row > (long long)B * max_boxes) return 0;
    return (header_words(B) + (size_t)row * kRowWords) * 4;
}

extern "C" size_t mpn_pose_gather_record_bytes(int B, int max_boxes) {
    if (B < 1 || max_boxes < 1 || (long long)B * max_boxes > kMaxRows) return 0;
    return mpn_pose_gather_row_offset(B, max_boxes, B * max_boxes);
}

extern "C" int mpn_pose_gather(const float* boxes, const float* scores, const int* num_boxes, const float* keypoint_scores,
                               const float* keypoint_positions, const int* overflow, int B, int max_boxes, float score_threshold,
                               int height, int width, void* record, size_t record_bytes, mpn_stream_t stream) {
    MPN_REQUIRE(boxes && scores && num_boxes && record, MPN_ERR_BAD_ARG, "pose_gather: null pointer");
    MPN_REQUIRE(B >= 1 && max_boxes >= 1 && height >= 1 && width >= 1, MPN_ERR_BAD_SHAPE, "pose_gather: bad shape");
    MPN_REQUIRE((long long)B * max_boxes <= kMaxRows, MPN_ERR_BAD_SHAPE,
                "pose_gather: B * max_boxes = %lld rows, the single block covers %d", (long long)B * max_boxes, kMaxRows);
    MPN_REQUIRE(mpn_aligned16(record), MPN_ERR_BAD_ALIGN, "pose_gather: record must be 16-byte aligned");
    MPN_REQUIRE(record_bytes >= mpn_pose_gather_record_bytes(B, max_boxes), MPN_ERR_WORKSPACE,
                "pose_gather: record of %zu bytes, %zu needed", record_bytes, mpn_pose_gather_record_bytes(B, max_boxes));
    GatherArgs a = {boxes, scores, num_boxes, keypoint_scores, keypoint_positions, overflow, nullptr, score_threshold, (float)height,
                    (float)width, B, max_boxes, (int)header_words(B)};
    int* header = (int*)record;
    uint4* rows = (uint4*)((char*)record + mpn_pose_gather_row_offset(B, max_boxes, 0));
    pose_gather_kernel<false><<<1, kThreads, 0, (hipStream_t)stream>>>(a, header, rows);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}

extern "C" int mpn_pose_gather_sized(const float* boxes, const float* scores, const int* num_boxes, const float* keypoint_scores,
                                     const float* keypoint_positions, const int* overflow, int B, int max_boxes,
                                     float score_threshold, const float* extent, void* record, size_t record_bytes,
                                     mpn_stream_t stream) {
    MPN_REQUIRE(boxes && scores && num_boxes && record && extent, MPN_ERR_BAD_ARG, "pose_gather_sized: null pointer");
    MPN_REQUIRE(B >= 1 && max_boxes >= 1, MPN_ERR_BAD_SHAPE, "pose_gather_sized: bad shape");
    MPN_REQUIRE((long long)B * max_boxes <= kMaxRows, MPN_ERR_BAD_SHAPE,
                "pose_gather_sized: B * max_boxes = %lld rows, the single block covers %d", (long long)B * max_boxes, kMaxRows);
    MPN_REQUIRE(mpn_aligned16(record), MPN_ERR_BAD_ALIGN, "pose_gather_sized: record must be 16-byte aligned");
    MPN_REQUIRE(record_bytes >= mpn_pose_gather_record_bytes(B, max_boxes), MPN_ERR_WORKSPACE,
                "pose_gather_sized: record of %zu bytes, %zu needed", record_bytes, mpn_pose_gather_record_bytes(B, max_boxes));
    GatherArgs a = {boxes, scores, num_boxes, keypoint_scores, keypoint_positions, overflow, extent, score_threshold, 0.f, 0.f,
                    B, max_boxes, (int)header_words(B)};
    int* header = (int*)record;
    uint4* rows = (uint4*)((char*)record + mpn_pose_gather_row_offset(B, max_boxes, 0));
    pose_gather_kernel<true><<<1, kThreads, 0, (hipStream_t)stream>>>(a, header, rows);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
