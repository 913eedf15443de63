// Tracking accuracy on the device: a frame's tracked persons (the record mpn_pose_gather wrote and the rows mpn_pose_track wrote
// for it) against annotated persons with identities, by the CLEAR-MOT mapping rule (Bernardin & Stiefelhagen 2008) under keypoint
// OKS. What MOTA, MOTP and IDF1 are accumulated from on the host (multiposenet_amd/track_metrics.py).
//   mpn_track_eval   record + track rows (read in place) + ground truth + prev state -> next state + a 48-byte row per image, a
//                    32-byte row per (image, ground truth) and an 8-byte row per record row. PURE like mpn_pose_track: prev is
//                    never written; the caller advances the state by copying next over prev.
// ONE block per stream (B = streams * F images, stream s owns images s*F .. s*F+F-1 in time order); the block walks its F frames
// in order with the stream's state - per identity the track id it was last matched to - in LDS. Per frame:
//   phase A  the frame's track ids, the ground truths' ignore flags, identity indices and stored ids -> LDS
//   phase B  the OKS of every (ground truth, record row) pair -> LDS [ground truth][row]: 64 x 64 f64 = 32 KB
//   phase C  the overlap masks: per ground truth one ballot over the rows (tracked and similarity >= threshold)
//   phase D  wave 0, lane = record row: the kept correspondences (a ballot per ground truth, in row order), the rows of the
//            ground truths that are out of the assignment set to NaN, assign_optimal (hungarian.h) with the bias 2^27 over the
//            rows that still have an eligible pair, the
//            hypotheses an ignored ground truth absorbs (an OR butterfly), the rows' flags and the frame's hypothesis counts
//   phase E  wave 0, lane = ground truth: switches, the ground-truth rows, the frame's counts; lane 0 sums the similarities in
//            row order and stores the matched ids
// Latency-bound glue like mpn_pose_track (microseconds behind a network pass of milliseconds): not tuned beyond that.
#include "common.h"
#include "hungarian.h"
#include "oks_math.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxGt = 64;              // one lane of wave 0 per ground truth
constexpr int kMaxBoxes = 64;           // one lane of wave 0 per record row; an overlap mask is one 64-bit word
constexpr int kMaxRows = 4096;          // mpn_pose_gather's own limit on B * max_boxes
constexpr int kMaxIdentities = 1024;
static_assert(kMaxGt == kAssignSide && kMaxBoxes == kAssignSide, "one lane of the wave per ground truth and per record row");
// the record's row (pose_gather.hip), in 32-bit words; a row of mpn_pose_track's out in bytes (track_id first)
constexpr int kRowWords = 108, kOffKeypoints = 57, kTrackRowBytes = 24;
// the state of one stream, in 32-bit words: {frames, 0, 0, 0}, then max_identities track ids
constexpr int kStateHeaderWords = 4;
// the output rows, in bytes
constexpr int kFrameBytes = 48, kGtBytes = 32, kHypBytes = 8;
constexpr int kGtMatched = 1, kGtSwitch = 2, kGtKept = 4, kGtIgnored = 8;
constexpr int kHypFalsePositive = 1, kHypIgnored = 2, kHypUntracked = 4;
// with this bias on every weight a matching with more pairs outweighs any with fewer: 64 quanta sum to less than 2^27
constexpr long long kPairBias = 1ll << 27;

inline size_t header_words(int B) { return ((size_t)(2 * B + 2) + 3) / 4 * 4; }
__host__ __device__ inline size_t stream_words(int max_identities) { return kStateHeaderWords + (size_t)max_identities; }

struct EvalArgs {
    const int* header;
    const float* rows;
    const unsigned char* track_rows;
    const double* gt;
    const int* gt_counts;
    const int* gt_identity;
    const int* prev;
    int* next;
    unsigned char* out;
    double threshold;
    int B, max_boxes, streams, max_gt, max_identities;
};

__global__ __launch_bounds__(kThreads) void track_eval_kernel(EvalArgs a) {
    __shared__ double sim[kMaxGt][kMaxBoxes];             // [ground truth][record row]: lane = row reads consecutive doubles
    __shared__ int ident[kMaxIdentities];                 // the track id an identity was last matched to, 0 = never
    __shared__ unsigned long long gmask[kMaxGt];          // the overlap mask of a ground truth
    __shared__ double gsim[kMaxGt];                       // similarity of a matched ground truth
    __shared__ int htid[kMaxBoxes];                       // the track id of a record row, 0 = untracked
    __shared__ int gidx[kMaxGt], gstored[kMaxGt], gignored[kMaxGt], grow[kMaxGt], gkept[kMaxGt];
    __shared__ int hyp_counts[4];                         // tracked, ignored, false positives, untracked
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = a.B / a.streams, I = a.max_identities;
    const int all_rows = a.B * a.max_boxes;
    const int* pst = a.prev + (size_t)s * stream_words(I);
    int* nst = a.next + (size_t)s * stream_words(I);
    unsigned char* frame_out = a.out;
    unsigned char* gt_out = frame_out + (size_t)a.B * kFrameBytes;
    unsigned char* hyp_out = gt_out + (size_t)a.B * a.max_gt * kGtBytes;

    for (int i = tid; i < I; i += kThreads) ident[i] = pst[kStateHeaderWords + i];

    // the record's counts, clamped as mpn_pose_track clamps them: nothing is indexed out of range
    int total = a.header[0];
    total = total < 0 ? 0 : (total > all_rows ? all_rows : total);
    // rows behind the record's total are zero: the blocks share them
    for (long long w = (long long)total * (kHypBytes / 4) + s * kThreads + tid; w < (long long)all_rows * (kHypBytes / 4);
         w += (long long)a.streams * kThreads)
        ((unsigned*)hyp_out)[w] = 0u;
    int ahead = 0;                                        // kept rows of the images before the frame
    for (int i = 0; i < s * F; ++i) {
        ahead += a.header[1 + i] > 0 ? a.header[1 + i] : 0;
        if (ahead > all_rows) ahead = all_rows;           // (past the total either way; the sum cannot wrap)
    }
    __syncthreads();

    for (int f = 0; f < F; ++f) {
        const int b = s * F + f;
        int n = a.header[1 + b];
        int first = ahead;
        ahead += n > 0 ? n : 0;
        if (ahead > all_rows) ahead = all_rows;
        n = n < 0 ? 0 : (n > a.max_boxes ? a.max_boxes : n);
        if (first > total) first = total;
        if (first + n > total) n = total - first;
        const float* rows = a.rows + (size_t)first * kRowWords;
        int ng = a.gt_counts[b];
        ng = ng < 0 ? 0 : (ng > a.max_gt ? a.max_gt : ng);
        const double* gt = a.gt + (size_t)b * a.max_gt * kGtDoubles;

        // phase A
        if (tid < kMaxBoxes) htid[tid] = tid < n ? *(const int*)(a.track_rows + (size_t)(first + tid) * kTrackRowBytes) : 0;
        if (tid < kMaxGt) {
            int idx = -1, stored = 0, ignored = 0;
            if (tid < ng) {
                idx = a.gt_identity[(size_t)b * a.max_gt + tid];
                if (idx < 0 || idx >= I) idx = -1;        // no memory: never kept, never a switch, never stored
                stored = idx >= 0 ? ident[idx] : 0;
                ignored = gt[tid * kGtDoubles + kGtIgnore] != 0.0;
            }
            gidx[tid] = idx; gstored[tid] = stored; gignored[tid] = ignored;
            grow[tid] = -1; gkept[tid] = 0; gsim[tid] = 0.0;
        }
        // phase B
        for (int i = tid; i < ng * n; i += kThreads) {
            const int g = i / n, h = i - g * n;
            sim[g][h] = oks_of(rows + (size_t)h * kRowWords + kOffKeypoints, gt + g * kGtDoubles);
        }
        __syncthreads();

        // phase C (a NaN never passes >=)
        for (int g = wave; g < ng; g += kThreads / 64) {
            const unsigned long long m = __ballot(lane < n && htid[lane] != 0 && sim[g][lane] >= a.threshold);
            if (lane == 0) gmask[g] = m;
        }
        __syncthreads();

        // phase D
        if (wave == 0) {
            const int h = lane;
            const bool tracked = h < n && htid[h] != 0;
            unsigned long long taken = 0ull, kept_gts = 0ull;   // (the same value in every lane)
            int mine = -1;
            double mine_sim = 0.0;
            bool kept = false;
            for (int g = 0; g < kMaxGt; ++g) {            // 1. the kept correspondences, in ground-truth row order
                if (g >= ng) break;
                const int stored = gstored[g];
                if (gignored[g] || stored == 0) continue; // (uniform)
                const bool cand = tracked && htid[h] == stored && ((gmask[g] >> h) & 1ull) && !((taken >> h) & 1ull);
                const unsigned long long c = __ballot(cand);
                if (c == 0ull) continue;
                const int hit = __ffsll(c) - 1;           // (a frame's track ids are distinct: the lowest row if not)
                taken |= 1ull << hit;
                kept_gts |= 1ull << g;
                if (h == hit) { mine = g; mine_sim = sim[g][h]; kept = true; }
            }
            // 2. the ground truths that are ignored or already matched leave the assignment (their row becomes NaN, which is
            // never eligible; a lane writes and reads its own column only), and so do the rows that are taken or untracked
            const unsigned long long out_of_it = kept_gts | __ballot(lane < ng && gignored[lane] != 0);
            for (int g = 0; g < kMaxGt; ++g) {
                if (g >= ng) break;
                if ((out_of_it >> g) & 1ull) sim[g][h] = __longlong_as_double(0x7ff8000000000000ll);
            }
            // (the rows that still have an eligible pair with an open record row; the others would only walk to their dummies)
            const unsigned long long with_pairs =
                __ballot(lane < ng && !((out_of_it >> lane) & 1ull) && (gmask[lane] & ~taken) != 0ull);
            assign_optimal<kPairBias>(sim, ng, n, lane, tracked && !kept, a.threshold, mine, mine_sim, with_pairs);
            if (mine >= 0) { grow[mine] = h; gsim[mine] = mine_sim; gkept[mine] = kept ? 1 : 0; }
            // 3. an unmatched tracked row that an ignored ground truth overlaps is ignored
            unsigned long long absorb = (lane < ng && gignored[lane] != 0) ? gmask[lane] : 0ull;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) absorb |= __shfl_xor(absorb, o, 64);
            const bool matched = mine >= 0;
            const bool ignored = tracked && !matched && ((absorb >> h) & 1ull);
            const bool fp = tracked && !matched && !ignored;
            const bool untracked = h < n && !tracked;
            if (h < n) {
                int* o = (int*)(hyp_out + (size_t)(first + h) * kHypBytes);
                o[0] = mine;
                o[1] = (fp ? kHypFalsePositive : 0) | (ignored ? kHypIgnored : 0) | (untracked ? kHypUntracked : 0);
            }
            const int num_tracked = __popcll(__ballot(tracked)), num_ignored = __popcll(__ballot(ignored));
            const int num_fp = __popcll(__ballot(fp)), num_untracked = __popcll(__ballot(untracked));
            if (lane == 0) {
                hyp_counts[0] = num_tracked; hyp_counts[1] = num_ignored; hyp_counts[2] = num_fp; hyp_counts[3] = num_untracked;
            }
        }
        __syncthreads();

        // phase E
        if (wave == 0) {
            const int g = lane;
            const bool valid = g < ng, ignored = valid && gignored[g] != 0;
            const int h = valid ? grow[g] : -1;
            const bool matched = h >= 0;
            const int id = matched ? htid[h] : 0, stored = valid ? gstored[g] : 0;
            const bool is_switch = matched && stored != 0 && stored != id;
            if (valid) {
                unsigned char* o = gt_out + ((size_t)b * a.max_gt + g) * kGtBytes;
                ((int*)o)[0] = id;
                ((int*)o)[1] = h;
                ((int*)o)[2] = (matched ? kGtMatched : 0) | (is_switch ? kGtSwitch : 0) | (gkept[g] ? kGtKept : 0) |
                               (ignored ? kGtIgnored : 0);
                ((int*)o)[3] = stored;
                *(double*)(o + 16) = gsim[g];
                *(unsigned long long*)(o + 24) = gmask[g];
            }
            const int num_gt = __popcll(__ballot(valid && !ignored)), num_matched = __popcll(__ballot(matched));
            const int num_switch = __popcll(__ballot(is_switch)), num_miss = __popcll(__ballot(valid && !ignored && !matched));
            if (lane == 0) {
                double sum = 0.0;
                for (int j = 0; j < ng; ++j) {            // in ground-truth row order; 4. every matched identity stores its id
                    const int r = grow[j];
                    if (r < 0) continue;
                    sum += gsim[j];
                    if (gidx[j] >= 0) ident[gidx[j]] = htid[r];
                }
                unsigned char* o = frame_out + (size_t)b * kFrameBytes;
                ((int*)o)[0] = num_gt;
                ((int*)o)[1] = hyp_counts[0] - hyp_counts[1];
                ((int*)o)[2] = num_matched;
                ((int*)o)[3] = num_switch;
                ((int*)o)[4] = num_miss;
                ((int*)o)[5] = hyp_counts[2];
                ((int*)o)[6] = hyp_counts[1];
                ((int*)o)[7] = hyp_counts[3];
                *(double*)(o + 32) = sum;
                *(unsigned long long*)(o + 40) = 0ull;
            }
        }
        // the image's ground-truth rows behind its count are zero
        for (int w = ng * (kGtBytes / 4) + tid; w < a.max_gt * (kGtBytes / 4); w += kThreads)
            ((unsigned*)(gt_out + (size_t)b * a.max_gt * kGtBytes))[w] = 0u;
        __syncthreads();
    }

    for (int i = tid; i < I; i += kThreads) nst[kStateHeaderWords + i] = ident[i];
    if (tid < kStateHeaderWords) nst[tid] = tid == 0 ? pst[0] + F : 0;
}

}  // namespace

extern "C" size_t mpn_track_eval_state_bytes(int streams, int max_identities) {
    if (streams < 1 || streams > kMaxRows || max_identities < 1 || max_identities > kMaxIdentities) return 0;
    return (size_t)streams * stream_words(max_identities) * 4;
}

extern "C" size_t mpn_track_eval_out_bytes(int B, int max_boxes, int max_gt) {
    if (B < 1 || max_boxes < 1 || max_boxes > kMaxBoxes || (long long)B * max_boxes > kMaxRows || max_gt < 1 || max_gt > kMaxGt)
        return 0;
    return (size_t)B * kFrameBytes + (size_t)B * max_gt * kGtBytes + (size_t)B * max_boxes * kHypBytes;
}

extern "C" int mpn_track_eval(const void* record, const void* track_rows, int B, int max_boxes, int streams, const double* gt,
                              const int* gt_counts, const int* gt_identity, int max_gt, int max_identities, double threshold,
                              const void* prev, void* next, size_t state_bytes, void* out, size_t out_bytes,
                              mpn_stream_t stream) {
    MPN_REQUIRE(record && track_rows && gt && gt_counts && gt_identity && prev && next && out, MPN_ERR_BAD_ARG,
                "track_eval: null pointer");
    MPN_REQUIRE(streams >= 1 && B >= 1 && B % streams == 0, MPN_ERR_BAD_SHAPE,
                "track_eval: B = %d images are not streams = %d times a whole number of frames", B, streams);
    MPN_REQUIRE(max_boxes >= 1 && max_boxes <= kMaxBoxes && (long long)B * max_boxes <= kMaxRows, MPN_ERR_BAD_SHAPE,
                "track_eval: B = %d, max_boxes = %d (at most %d per image, %d rows)", B, max_boxes, kMaxBoxes, kMaxRows);
    MPN_REQUIRE(max_gt >= 1 && max_gt <= kMaxGt, MPN_ERR_BAD_SHAPE,
                "track_eval: max_gt = %d, one lane of a wave per ground truth takes 1..%d", max_gt, kMaxGt);
    MPN_REQUIRE(max_identities >= 1 && max_identities <= kMaxIdentities, MPN_ERR_BAD_SHAPE,
                "track_eval: max_identities = %d, the state of a stream in LDS takes 1..%d", max_identities, kMaxIdentities);
    MPN_REQUIRE(threshold == threshold, MPN_ERR_BAD_ARG, "track_eval: threshold is not a number");
    MPN_REQUIRE(mpn_aligned16(record) && (((uintptr_t)track_rows | (uintptr_t)gt | (uintptr_t)prev | (uintptr_t)next |
                                           (uintptr_t)out) & 7u) == 0 &&
                    (((uintptr_t)gt_counts | (uintptr_t)gt_identity) & 3u) == 0,
                MPN_ERR_BAD_ALIGN,
                "track_eval: record must be 16-byte, track_rows / gt / prev / next / out 8-byte, gt_counts / gt_identity 4-byte aligned");
    MPN_REQUIRE(prev != next, MPN_ERR_BAD_ARG,
                "track_eval: prev and next are one buffer; the launch is a pure function of (record, track_rows, gt, prev)");
    MPN_REQUIRE(state_bytes >= mpn_track_eval_state_bytes(streams, max_identities), MPN_ERR_WORKSPACE,
                "track_eval: state_bytes = %zu, the state of %d streams x %d identities takes %zu", state_bytes, streams,
                max_identities, mpn_track_eval_state_bytes(streams, max_identities));
    MPN_REQUIRE(out_bytes >= mpn_track_eval_out_bytes(B, max_boxes, max_gt), MPN_ERR_WORKSPACE,
                "track_eval: out_bytes = %zu, the rows take %zu", out_bytes, mpn_track_eval_out_bytes(B, max_boxes, max_gt));
    EvalArgs a = {(const int*)record, (const float*)((const char*)record + header_words(B) * 4), (const unsigned char*)track_rows,
                  gt, gt_counts, gt_identity, (const int*)prev, (int*)next, (unsigned char*)out, threshold, B, max_boxes, streams,
                  max_gt, max_identities};
    track_eval_kernel<<<streams, kThreads, 0, (hipStream_t)stream>>>(a);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
