// Keypoint-similarity NMS of the record mpn_pose_gather wrote: the duplicate poses that box NMS cannot see (two boxes on one
// person with an IoU below its threshold, to which the PRN gives nearly the same 17 keypoints) are dropped on the device.
//   mpn_pose_nms   record_in (read in place) -> record_out of the same layout holding the kept persons, dense, in record
//                  order; info: per image the number suppressed, per kept row its index in record_in and how many it
//                  absorbed; optionally the similarity matrix [B, max_boxes, max_boxes].
// A PURE function of record_in: nothing is updated in place, so launching it twice (the Detector's eager pass, then the replay
// of the captured graph) changes nothing. Two launches, neither with atomics:
//   pose_nms_image_kernel   ONE block per image: keypoints, order scores and areas -> LDS; the n (n - 1) / 2 similarities
//            spread over the block (each unordered pair once); the visit order by counting; per person the 64-bit mask of the
//            persons it would suppress; one lane walks the greedy loop over the masks -> keep flag and absorbed count per slot
//   pose_nms_compact_kernel   ONE block: pose_gather_kernel's ballot / popcount exclusive scan over the keep flags (and over
//            the live flags, which gives a slot's row in record_in), then header, info and the rows in 16-byte copies
// Arithmetic is IEEE float64 in the documented order (oks_math.h), contraction off; exp is the device library's (<= 1 ulp).
// Latency-bound glue like mpn_oks_match (B blocks of at most 2016 pairs x 17 exp): not tuned.
#include "common.h"
#include "oks_math.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;               // pose_nms_image_kernel
constexpr int kCompactThreads = 1024;       // pose_nms_compact_kernel
constexpr int kWaves = kCompactThreads / 64;
constexpr int kK = kOksKeypoints;
constexpr int kMaxBoxes = 64;               // a person's suppression set is one 64-bit mask
constexpr int kMaxRows = 4096;              // mpn_pose_gather's own limit on B * max_boxes
// the record's row (pose_gather.hip), in 32-bit words
constexpr int kRowWords = 108, kOffScore = 5, kOffKScore = 6, kOffKeypoints = 57;
constexpr int kRowVecs = kRowWords / 4;

inline size_t header_words(int B) { return ((size_t)(2 * B + 2) + 3) / 4 * 4; }
// info: int32 suppressed[B] padded to 16 bytes; {source, absorbed} per record row; {keep, absorbed} per slot (the workspace)
inline size_t info_head_bytes(int B) { return ((size_t)B * 4 + 15) / 16 * 16; }

struct NmsArgs {
    const int* header;          // record_in
    const float* rows;
    int2* work;                 // {keep, absorbed} of slot image * max_boxes + person
    double* sim_out;
    double threshold;
    float min_keypoint_score;
    int B, max_boxes, score_mode;
};

__device__ __forceinline__ int clamped_count(const int* header, int image, int max_boxes) {
    const int n = header[1 + image];
    return n < 0 ? 0 : (n > max_boxes ? max_boxes : n);
}

// whether person j (order score sj) is visited before person i: descending, equal scores in record order, NaN last
__device__ __forceinline__ bool visited_before(float sj, int j, float si, int i) {
    if (sj != sj) return si != si && j < i;
    if (si != si) return true;
    return sj > si || (sj == si && j < i);
}

__global__ __launch_bounds__(kThreads) void pose_nms_image_kernel(NmsArgs a) {
    __shared__ double sim[kMaxBoxes][kMaxBoxes];
    __shared__ float kp[kMaxBoxes][3 * kK];
    __shared__ double area[kMaxBoxes];
    __shared__ float score[kMaxBoxes];
    __shared__ unsigned counting[kMaxBoxes];            // bit k: keypoints[k][2] >= min_keypoint_score
    __shared__ int order[kMaxBoxes];                    // the person visited at place r
    __shared__ unsigned long long over[kMaxBoxes];      // bit q: similarity(p, q) > threshold
    __shared__ unsigned long long kept_mask;
    __shared__ int absorbed[kMaxBoxes];
    __shared__ int partial[kThreads];
    const int b = blockIdx.x, tid = threadIdx.x, mb = a.max_boxes;

    // this image's rows of record_in: behind the (clamped) counts of the images before it
    int ahead = 0;
    for (int i = tid; i < b; i += kThreads) ahead += clamped_count(a.header, i, mb);
    partial[tid] = ahead;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) partial[tid] += partial[tid + s];
        __syncthreads();
    }
    const int first = partial[0];
    const int n = clamped_count(a.header, b, mb);

    for (int i = tid; i < n * 3 * kK; i += kThreads) {
        const int p = i / (3 * kK), f = i - p * (3 * kK);
        kp[p][f] = a.rows[(size_t)(first + p) * kRowWords + kOffKeypoints + f];
    }
    __syncthreads();
    if (tid < n) {
        const float* row = a.rows + (size_t)(first + tid) * kRowWords;
        score[tid] = order_score(row[kOffScore], row + kOffKScore, a.score_mode);
        area[tid] = keypoint_extent_area(kp[tid]);
        unsigned bits = 0u;
        for (int k = 0; k < kK; ++k) bits |= (kp[tid][3 * k + 2] >= a.min_keypoint_score ? 1u : 0u) << k;
        counting[tid] = bits;
        absorbed[tid] = 0;
    }
    __syncthreads();
    if (tid < n) {
        const float s = score[tid];
        int r = 0;
        for (int j = 0; j < n; ++j) r += j != tid && visited_before(score[j], j, s, tid);
        order[r] = tid;
    }
    // every unordered pair once
    for (int i = tid; i < n * n; i += kThreads) {
        const int p = i / n, q = i - p * n;
        if (p > q) continue;
        double s = 0.0;
        if (p < q) {
            const unsigned both = counting[p] & counting[q];
            const int m = __popc(both);
            if (m > 0) {
                const double denom = (area[p] + area[q]) / 2 + kEps;
                double sum = 0.0;
                for (int k = 0; k < kK; ++k) {
                    if (!((both >> k) & 1u)) continue;
                    const double dx = (double)kp[q][3 * k] - (double)kp[p][3 * k];
                    const double dy = (double)kp[q][3 * k + 1] - (double)kp[p][3 * k + 1];
                    sum += oks_term(dx, dy, k, denom);
                }
                s = sum / (double)m;
            }
        }
        sim[p][q] = s;
        sim[q][p] = s;
    }
    __syncthreads();
    if (tid < n) {
        unsigned long long bits = 0ull;
        for (int q = 0; q < n; ++q)
            if (q != tid && sim[tid][q] > a.threshold) bits |= 1ull << q;
        over[tid] = bits;
    }
    __syncthreads();
    if (tid == 0) {             // the greedy walk: a kept person suppresses those behind it that nobody suppressed yet
        unsigned long long kept = 0ull, suppressed = 0ull;
        for (int r = 0; r < n; ++r) {
            const int p = order[r];
            if ((suppressed >> p) & 1ull) continue;
            kept |= 1ull << p;
            const unsigned long long now = over[p] & ~suppressed & ~kept;
            suppressed |= now;
            absorbed[p] = __popcll(now);
        }
        kept_mask = kept;
    }
    __syncthreads();
    for (int p = tid; p < mb; p += kThreads) {
        const bool keep = p < n && ((kept_mask >> p) & 1ull);
        a.work[(size_t)b * mb + p] = make_int2(keep ? 1 : 0, keep ? absorbed[p] : 0);
    }
    if (a.sim_out) {
        double* out = a.sim_out + (size_t)b * mb * mb;
        for (int i = tid; i < mb * mb; i += kThreads) {
            const int p = i / mb, q = i - p * mb;
            out[i] = (p < n && q < n) ? sim[p][q] : 0.0;
        }
    }
}

struct CompactArgs {
    const int* header_in;
    const uint4* rows_in;
    const int2* work;
    int* header_out;
    uint4* rows_out;
    int* suppressed;            // info's head
    int2* info_rows;
    int B, max_boxes, header_words, info_head_words;
};

__global__ __launch_bounds__(kCompactThreads) void pose_nms_compact_kernel(CompactArgs a) {
    __shared__ int before[kMaxRows + 1];    // kept slots ahead of slot r (exclusive scan; [n] = total)
    __shared__ int row_of[kMaxRows];        // row j of record_out <- this row of record_in
    __shared__ int slot_of[kMaxRows];       //                     <- this slot
    __shared__ int kept_total[kWaves], live_total[kWaves];
    const int n = a.B * a.max_boxes;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0, live_carry = 0;
    for (int base = 0; base < n; base += kCompactThreads) {     // (uniform trip count: every thread reaches the barriers)
        const int r = base + tid;
        bool live = false, keep = false;
        if (r < n) {
            const int img = r / a.max_boxes;
            live = r - img * a.max_boxes < clamped_count(a.header_in, img, a.max_boxes);
            keep = live && a.work[r].x != 0;
        }
        const unsigned long long mk = __ballot(keep), ml = __ballot(live);
        if (lane == 0) { kept_total[wave] = __popcll(mk); live_total[wave] = __popcll(ml); }
        __syncthreads();
        int ahead = 0, all = 0, live_ahead = 0, live_all = 0;
        for (int k = 0; k < kWaves; ++k) {
            const int t = kept_total[k], l = live_total[k];
            all += t;
            live_all += l;
            if (k < wave) { ahead += t; live_ahead += l; }
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        const int at = carry + ahead + __popcll(mk & below);
        if (r < n) {
            before[r] = at;
            if (keep) {
                row_of[at] = live_carry + live_ahead + __popcll(ml & below);
                slot_of[at] = r;
            }
        }
        carry += all;
        live_carry += live_all;
        __syncthreads();
    }
    const int total = carry;
    if (tid == 0) before[n] = total;
    __syncthreads();
    for (int i = tid; i < a.header_words; i += kCompactThreads) {
        int v = 0;
        if (i == 0) v = total;
        else if (i <= a.B) v = before[i * a.max_boxes] - before[(i - 1) * a.max_boxes];
        else if (i <= 2 * a.B + 1) v = a.header_in[i];          // num_boxes[B] and the overflow word: copied through
        a.header_out[i] = v;
    }
    for (int i = tid; i < a.info_head_words; i += kCompactThreads) {
        int v = 0;
        if (i < a.B) v = clamped_count(a.header_in, i, a.max_boxes) - (before[(i + 1) * a.max_boxes] - before[i * a.max_boxes]);
        a.suppressed[i] = v;
    }
    for (int j = tid; j < n; j += kCompactThreads) {
        int2 o = make_int2(0, 0);
        if (j < total) {
            const int r = slot_of[j];
            o = make_int2(r - (r / a.max_boxes) * a.max_boxes, a.work[r].y);
        }
        a.info_rows[j] = o;
    }
    const int nvec = n * kRowVecs;
    for (int v = tid; v < nvec; v += kCompactThreads) {
        const int j = v / kRowVecs, f = v - j * kRowVecs;
        uint4 o = make_uint4(0u, 0u, 0u, 0u);
        if (j < total) o = a.rows_in[row_of[j] * kRowVecs + f];
        a.rows_out[v] = o;
    }
}

}  // namespace

extern "C" size_t mpn_pose_nms_info_bytes(int B, int max_boxes) {
    if (B < 1 || max_boxes < 1 || max_boxes > kMaxBoxes || (long long)B * max_boxes > kMaxRows) return 0;
    return info_head_bytes(B) + (size_t)B * max_boxes * 16;
}

extern "C" int mpn_pose_nms(const void* record_in, int B, int max_boxes, float threshold, float min_keypoint_score, int score_mode,
                            void* record_out, size_t record_bytes, void* info, size_t info_bytes, double* sim_out,
                            mpn_stream_t stream) {
    MPN_REQUIRE(record_in && record_out && info, MPN_ERR_BAD_ARG, "pose_nms: null pointer");
    MPN_REQUIRE(score_mode == 0 || score_mode == 1, MPN_ERR_BAD_ARG, "pose_nms: score_mode must be 0 or 1");
    MPN_REQUIRE(threshold == threshold && min_keypoint_score == min_keypoint_score, MPN_ERR_BAD_ARG,
                "pose_nms: threshold and min_keypoint_score must not be NaN");
    MPN_REQUIRE(B >= 1 && max_boxes >= 1 && max_boxes <= kMaxBoxes && (long long)B * max_boxes <= kMaxRows, MPN_ERR_BAD_SHAPE,
                "pose_nms: B = %d, max_boxes = %d (at most %d per image: a suppression set is one 64-bit mask; %d rows)", B,
                max_boxes, kMaxBoxes, kMaxRows);
    const size_t need = mpn_pose_gather_record_bytes(B, max_boxes), info_need = mpn_pose_nms_info_bytes(B, max_boxes);
    const uintptr_t in = (uintptr_t)record_in, out = (uintptr_t)record_out;
    MPN_REQUIRE(in + need <= out || out + need <= in, MPN_ERR_BAD_ARG, "pose_nms: record_out must not overlap record_in");
    MPN_REQUIRE(mpn_aligned16(record_in) && mpn_aligned16(record_out), MPN_ERR_BAD_ALIGN,
                "pose_nms: the records must be 16-byte aligned");
    MPN_REQUIRE((((uintptr_t)info | (uintptr_t)sim_out) & 7u) == 0, MPN_ERR_BAD_ALIGN,
                "pose_nms: info and sim_out must be 8-byte aligned");
    MPN_REQUIRE(record_bytes >= need, MPN_ERR_WORKSPACE, "pose_nms: record_out of %zu bytes, %zu needed", record_bytes, need);
    MPN_REQUIRE(info_bytes >= info_need, MPN_ERR_WORKSPACE, "pose_nms: info of %zu bytes, %zu needed", info_bytes, info_need);
    const size_t head = header_words(B) * 4, slots = (size_t)B * max_boxes;
    int2* info_rows = (int2*)((char*)info + info_head_bytes(B));
    int2* work = info_rows + slots;
    NmsArgs a = {(const int*)record_in, (const float*)((const char*)record_in + head), work, sim_out, (double)threshold,
                 min_keypoint_score, B, max_boxes, score_mode};
    pose_nms_image_kernel<<<B, kThreads, 0, (hipStream_t)stream>>>(a);
    MPN_LAUNCH_CHECK();
    CompactArgs c = {(const int*)record_in, (const uint4*)((const char*)record_in + head), work, (int*)record_out,
                     (uint4*)((char*)record_out + head), (int*)info, info_rows, B, max_boxes, (int)header_words(B),
                     (int)(info_head_bytes(B) / 4)};
    pose_nms_compact_kernel<<<1, kCompactThreads, 0, (hipStream_t)stream>>>(c);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
