// Person identities across the frames of a video, on the device: greedy matching of a frame's detections (the record
// mpn_pose_gather wrote) against the tracks the earlier frames left, by box IoU (f32) or keypoint OKS (f64).
//   mpn_pose_track   record (read in place) + prev state -> next state + one 24-byte row per record row
//                    {track_id, slot, hits, flags, similarity}. PURE: prev is never written; the caller advances the state by
//                    copying next over prev (include/mpn.h says why: a captured launch runs twice on an entry's first call).
//   mpn_pose_track_optimal   the same entry with phase C the optimal (Hungarian) assignment under integer weights; every
//                    other phase is the same code (pose_track_kernel<kOptimal, false>).
//   mpn_pose_track_motion    either assignment with a constant-velocity prediction in the track's role (pose_track_kernel<.,
//                    true>): a velocity state of its own (prev / next, pure in the same way) and one 160-byte row per
//                    coasting track (live, not detected in the frame) at its predicted pose.
// ONE block per stream (B = streams * F images, stream s owns images s*F .. s*F+F-1 in time order); the block walks its F frames
// in order with the working state in LDS. Per frame:
//   phase A  (motion: step 0, the predicted box and keypoints of every live slot -> LDS, which take the stored pose's place in
//            phases A and B;) the extent area of every live track's keypoints (OKS), the per-detection tables cleared
//   phase B  the similarity of every (live track, detection) pair -> LDS, transposed [detection][track]: 64 x 64 f64 = 32 KB
//   phase C  greedy matching by wave 0, lane = track slot: every lane keeps the best open detection of its row (ties: the
//            smaller detection), a 6-step xor butterfly takes the largest (ties: the smaller slot); a lane rescans its row
//            only when the detection it held was taken. No barrier inside the rounds, at most min(tracks, detections) of them.
//            (optimal: assign_optimal of hungarian.h, also wave 0 alone and without a barrier)
//   phase D  hits / age / misses of the live tracks, tracks past max_misses freed (motion: the velocities of the matched slots
//            updated from the detection and the pose it replaces, those of the others damped; the coasting slots ranked)
//   phase E  births in row order into the lowest free slots: two ballots and popcounts, no serial walk
//   phase F  the detections' box, score and keypoints copied into their slots, free slots zeroed, the output rows (motion: and
//            the frame's coasting rows)
// Latency-bound glue like mpn_oks_match (microseconds behind a network pass of milliseconds): not tuned beyond that.
#include "common.h"
#include "hungarian.h"
#include "oks_math.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxTracks = 64;          // one lane of wave 0 per slot; the free set is one 64-bit ballot
constexpr int kMaxBoxes = 64;           // the taken set of a frame's detections is one 64-bit mask
constexpr int kMaxRows = 4096;          // mpn_pose_gather's own limit on B * max_boxes
// the record's row (pose_gather.hip), in 32-bit words
constexpr int kRowWords = 108, kOffBox = 1, kOffScore = 5, kOffKeypoints = 57;
// the state of one stream, in 32-bit words: {next_id, dropped, 0, 0}, then max_tracks slots of
// {id, hits, age, misses, box[4], score, keypoints[17][3]}
constexpr int kStateHeaderWords = 4, kSlotInts = 4, kSlotData = 5 + 3 * kOksKeypoints, kSlotWords = kSlotInts + kSlotData;
constexpr int kDataKeypoints = 5;       // keypoints within a slot's data words (behind box[4] and score)
static_assert(kSlotWords == 60 && kSlotWords % 4 == 0 && kOffScore == kOffBox + 4, "state slot layout");
// an output row: int32 track_id, slot, hits, flags, f64 similarity
constexpr int kOutBytes = 24;
constexpr int kFlagNew = 1, kFlagOverflow = 2;
// motion: the state of one stream is four zero words, then max_tracks slots of {id, seen, vel[6]}: the velocity per frame of
// box[4] and of the keypoint centroid (x, y)
constexpr int kMotionHeaderWords = 4, kVelocities = 6, kMotionSlotWords = 2 + kVelocities;
// a predicted pose, box[4] and keypoints[17][2]; a coasting row is {id, misses} and that pose
constexpr int kPredWords = 4 + 2 * kOksKeypoints, kPredKeypoints = 4, kCoastWords = 2 + kPredWords;
static_assert(kMotionSlotWords == 8 && kCoastWords == 40, "motion state slot and coasting row layout");

inline size_t header_words(int B) { return ((size_t)(2 * B + 2) + 3) / 4 * 4; }
__host__ __device__ inline size_t stream_words(int max_tracks) { return kStateHeaderWords + (size_t)max_tracks * kSlotWords; }
__host__ __device__ inline size_t motion_stream_words(int max_tracks) {
    return kMotionHeaderWords + (size_t)max_tracks * kMotionSlotWords;
}

struct TrackArgs {
    const int* header;
    const float* rows;
    const int* prev;
    int* next;
    unsigned char* out;
    int B, max_boxes, streams, max_tracks, similarity, max_misses;
    float match_threshold, new_track_score;
    // mpn_pose_track_motion only
    const int* motion_prev;
    int* motion_next;
    unsigned* coast;
    float velocity_gain, damping;
};

// IoU of two record boxes (ymin, xmin, ymax, xmax) in f32; every min / max is a comparison (a NaN operand takes the other
// branch the same way in the numpy transcription), every operation correctly rounded
__device__ __forceinline__ float iou_of(const float* a, const float* b) {
    const float x0 = a[1] > b[1] ? a[1] : b[1], x1 = a[3] < b[3] ? a[3] : b[3];
    const float y0 = a[0] > b[0] ? a[0] : b[0], y1 = a[2] < b[2] ? a[2] : b[2];
    float iw = x1 - x0, ih = y1 - y0;
    iw = iw > 0.f ? iw : 0.f;
    ih = ih > 0.f ? ih : 0.f;
    const float inter = iw * ih;
    const float area_a = (a[3] - a[1]) * (a[2] - a[0]), area_b = (b[3] - b[1]) * (b[2] - b[0]);
    const float uni = area_a + area_b - inter;
    return uni > 0.f ? inter / uni : 0.f;
}

// computeOks with the track's stored keypoints in the ground-truth role, all 17 visible; area = their extent area
// (kStride = 2: the track's predicted keypoints[17][2])
template <int kStride = 3>
__device__ __forceinline__ double oks_track(const float* track_kp, double area, const float* det_kp) {
    const double denom = area + kEps;
    double sum = 0.0;
    for (int k = 0; k < kOksKeypoints; ++k) {
        const double dx = (double)det_kp[3 * k] - (double)track_kp[kStride * k];
        const double dy = (double)det_kp[3 * k + 1] - (double)track_kp[kStride * k + 1];
        sum += oks_term(dx, dy, k, denom);
    }
    return sum / (double)kOksKeypoints;
}

// the centroid of keypoints[17][3]: the sums in keypoint order from the first keypoint on, then / 17, in f32
__device__ __forceinline__ void centroid_of(const float* kp, float& cx, float& cy) {
    float sx = kp[0], sy = kp[1];
    for (int k = 1; k < kOksKeypoints; ++k) {
        sx = sx + kp[3 * k];
        sy = sy + kp[3 * k + 1];
    }
    cx = sx / 17.0f;
    cy = sy / 17.0f;
}

// Phase C of mpn_pose_track: the greedy rounds. Wave 0, lane = track slot t; `mine` is the detection the slot takes, -1 = none.
__device__ __forceinline__ void assign_greedy(const double (*sim)[kMaxTracks], int n, int t, bool live, double thr, int& mine,
                                              double& mine_sim) {
    unsigned long long taken = 0ull;
    bool open = live, rescan = true;
    double best = 0.0;
    int best_d = -1;
    for (int round = 0; round < n; ++round) {
        if (open && rescan) {
            best_d = -1;
            for (int d = 0; d < n; ++d) {
                if ((taken >> d) & 1ull) continue;
                const double v = sim[d][t];
                if (v >= thr && (best_d < 0 || v > best)) { best = v; best_d = d; }   // a NaN never passes v >= thr
            }
            rescan = false;
        }
        double v = best;
        int ct = (open && best_d >= 0) ? t : -1, cd = best_d;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double v2 = __shfl_xor(v, o, 64);
            const int t2 = __shfl_xor(ct, o, 64), d2 = __shfl_xor(cd, o, 64);
            if (t2 >= 0 && (ct < 0 || v2 > v || (v2 == v && t2 < ct))) { v = v2; ct = t2; cd = d2; }
        }
        if (ct < 0) break;                        // (every lane holds the same winner: a uniform exit)
        taken |= 1ull << cd;
        if (ct == t) { open = false; mine = cd; mine_sim = v; }
        else if (best_d == cd) rescan = true;
    }
}

// Phase C of mpn_pose_track_optimal: assign_optimal of hungarian.h with the weight quantum + 1 (no bias). Wave 0; rows are the
// detections 1..n, columns 1..T the slots (lane = slot), T+1..T+n the rows' dummies.
static_assert(kMaxTracks == kAssignSide && kMaxBoxes == kAssignSide, "one lane of the wave per slot and per detection");

template <bool kOptimal, bool kMotion>
__global__ __launch_bounds__(kThreads) void pose_track_kernel(TrackArgs a) {
    __shared__ double sim[kMaxBoxes][kMaxTracks];         // [detection][slot]: lane = slot reads consecutive doubles
    __shared__ float data[kMaxTracks][kSlotData];         // box[4], score, keypoints[17][3] of every slot
    __shared__ int id[kMaxTracks], hits[kMaxTracks], age[kMaxTracks], misses[kMaxTracks];
    __shared__ double tarea[kMaxTracks];
    __shared__ double dsim[kMaxBoxes];                    // similarity of a matched detection
    __shared__ int dslot[kMaxBoxes];                      // the slot a detection's data goes to, -1 = untracked
    __shared__ int dflags[kMaxBoxes];
    __shared__ int free_slot[kMaxTracks];                 // the r-th free slot
    __shared__ int counters[2];                           // next_id, dropped
    // motion (no instantiation without it names these: they take no LDS there)
    __shared__ float vel[kMotion ? kMaxTracks : 1][kVelocities];
    __shared__ int seen[kMotion ? kMaxTracks : 1];
    __shared__ float pred[kMotion ? kMaxTracks : 1][kPredWords];     // step 0: box[4], keypoints[17][2] of every live slot
    __shared__ int coast_row[kMotion ? kMaxTracks : 1];   // the frame's coasting row of a slot, -1 = none
    __shared__ int num_coast;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.max_tracks, F = a.B / a.streams;
    const int all_rows = a.B * a.max_boxes;
    const int* pst = a.prev + (size_t)s * stream_words(T);
    int* nst = a.next + (size_t)s * stream_words(T);

    for (int i = tid; i < T * kSlotData; i += kThreads) {
        const int t = i / kSlotData, w = i - t * kSlotData;
        data[t][w] = __int_as_float(pst[kStateHeaderWords + t * kSlotWords + kSlotInts + w]);
    }
    if (tid < T) {
        const int* p = pst + kStateHeaderWords + tid * kSlotWords;
        id[tid] = p[0]; hits[tid] = p[1]; age[tid] = p[2]; misses[tid] = p[3];
        if constexpr (kMotion) {                          // a slot whose velocities belong to another track, or to none, starts anew
            const int* m = a.motion_prev + (size_t)s * motion_stream_words(T) + kMotionHeaderWords + tid * kMotionSlotWords;
            const bool own = p[0] != 0 && m[0] == p[0];
            seen[tid] = own ? m[1] : 0;
            for (int c = 0; c < kVelocities; ++c) vel[tid][c] = own ? __int_as_float(m[2 + c]) : 0.f;
        }
    }
    if (tid == 0) {
        counters[0] = pst[0] < 1 ? 1 : pst[0];            // an all-zero state is the empty state: next_id reads as 1
        counters[1] = pst[1];
    }

    // the record's counts, clamped as mpn_oks_match clamps them: nothing is indexed out of range
    int total = a.header[0];
    total = total < 0 ? 0 : (total > all_rows ? all_rows : total);
    // rows behind the record's total are zero: the blocks share them
    for (long long w = (long long)total * (kOutBytes / 4) + s * kThreads + tid; w < (long long)all_rows * (kOutBytes / 4);
         w += (long long)a.streams * kThreads)
        ((unsigned*)a.out)[w] = 0u;
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

        // phase A
        if constexpr (kMotion) {
            for (int i = tid; i < T * kPredWords; i += kThreads) {
                const int t = i / kPredWords, w = i - t * kPredWords;
                if (id[t] == 0) continue;
                const float gap = (float)(misses[t] + 1);
                const int xy = (w - kPredKeypoints) & 1;
                const int c = w < kPredKeypoints ? w : 4 + xy;
                const int from = w < kPredKeypoints ? w : kDataKeypoints + 3 * ((w - kPredKeypoints) >> 1) + xy;
                pred[t][w] = data[t][from] + vel[t][c] * gap;
            }
            __syncthreads();
            if (tid < T && a.similarity == 1 && id[tid] != 0) tarea[tid] = keypoint_extent_area<2>(&pred[tid][kPredKeypoints]);
        } else {
            if (tid < T && a.similarity == 1 && id[tid] != 0) tarea[tid] = keypoint_extent_area(&data[tid][kDataKeypoints]);
        }
        if (tid < kMaxBoxes) { dslot[tid] = -1; dflags[tid] = 0; dsim[tid] = 0.0; }
        __syncthreads();

        // phase B
        for (int i = tid; i < T * n; i += kThreads) {
            const int d = i / T, t = i - d * T;
            double v = 0.0;
            if (id[t] != 0) {
                const float* row = rows + (size_t)d * kRowWords;
                if constexpr (kMotion)
                    v = a.similarity == 0 ? (double)iou_of(&pred[t][0], row + kOffBox)
                                          : oks_track<2>(&pred[t][kPredKeypoints], tarea[t], row + kOffKeypoints);
                else
                    v = a.similarity == 0 ? (double)iou_of(&data[t][0], row + kOffBox)
                                          : oks_track(&data[t][kDataKeypoints], tarea[t], row + kOffKeypoints);
            }
            sim[d][t] = v;
        }
        __syncthreads();

        // phases C and D
        if (wave == 0) {
            const int t = lane;
            const bool live = t < T && id[t] != 0;
            const double thr = (double)a.match_threshold;
            double mine_sim = 0.0;
            int mine = -1;
            if (kOptimal) assign_optimal<0>(sim, n, T, lane, live, thr, mine, mine_sim);
            else assign_greedy(sim, n, t, live, thr, mine, mine_sim);
            if (live) {
                if (mine >= 0) {
                    if constexpr (kMotion) {              // the observed velocity: the detection against the pose it replaces
                        const float gap = (float)(misses[t] + 1);
                        const float* z = rows + (size_t)mine * kRowWords;
                        float last[kVelocities], obs[kVelocities];
                        for (int c = 0; c < 4; ++c) { last[c] = data[t][c]; obs[c] = z[kOffBox + c]; }
                        centroid_of(&data[t][kDataKeypoints], last[4], last[5]);
                        centroid_of(z + kOffKeypoints, obs[4], obs[5]);
                        const float g = (seen[t] == 0 && a.velocity_gain > 0.f) ? 1.0f : a.velocity_gain;
                        for (int c = 0; c < kVelocities; ++c) {
                            const float vobs = (obs[c] - last[c]) / gap;
                            vel[t][c] = vel[t][c] + g * (vobs - vel[t][c]);
                        }
                        seen[t] += 1;
                    }
                    misses[t] = 0; hits[t] += 1; age[t] += 1;
                    dslot[mine] = t; dsim[mine] = mine_sim;
                } else {
                    misses[t] += 1; age[t] += 1;
                    const bool freed = misses[t] > a.max_misses;
                    if (freed) { id[t] = 0; hits[t] = 0; age[t] = 0; misses[t] = 0; }
                    if constexpr (kMotion) {
                        if (freed) seen[t] = 0;
                        for (int c = 0; c < kVelocities; ++c) vel[t][c] = freed ? 0.f : vel[t][c] * a.damping;
                    }
                }
            }
            if constexpr (kMotion) {                      // the coasting slots, in slot order
                const bool coasting = live && mine < 0 && id[t] != 0;
                const unsigned long long coast_mask = __ballot(coasting);
                if (t < T) coast_row[t] = coasting ? __popcll(coast_mask & ((1ull << lane) - 1ull)) : -1;
                if (lane == 0) num_coast = __popcll(coast_mask);
            }
        }
        __syncthreads();

        // phase E
        bool want = false;
        unsigned long long want_mask = 0ull;
        int num_free = 0;
        if (wave == 0) {
            want = lane < n && dslot[lane] < 0 && rows[(size_t)lane * kRowWords + kOffScore] >= a.new_track_score;
            const bool is_free = lane < T && id[lane] == 0;
            want_mask = __ballot(want);
            const unsigned long long free_mask = __ballot(is_free);
            num_free = __popcll(free_mask);
            if (is_free) free_slot[__popcll(free_mask & ((1ull << lane) - 1ull))] = lane;
        }
        __syncthreads();
        if (wave == 0) {
            const int next_id = counters[0];
            const int r = __popcll(want_mask & ((1ull << lane) - 1ull)), num_want = __popcll(want_mask);
            if (want) {
                if (r < num_free) {
                    const int t = free_slot[r];
                    id[t] = next_id + r; hits[t] = 1; age[t] = 1; misses[t] = 0;
                    if constexpr (kMotion) {              // (a free slot's are zero already)
                        seen[t] = 0;
                        for (int c = 0; c < kVelocities; ++c) vel[t][c] = 0.f;
                    }
                    dslot[lane] = t; dflags[lane] = kFlagNew;
                } else {
                    dflags[lane] = kFlagOverflow;
                }
            }
            if (lane == 0) {
                counters[0] = next_id + (num_want < num_free ? num_want : num_free);
                counters[1] += num_want > num_free ? num_want - num_free : 0;
            }
        }
        __syncthreads();

        // phase F (a free slot and a slot that takes a detection are never the same one)
        for (int i = tid; i < T * kSlotData; i += kThreads) {
            const int t = i / kSlotData, w = i - t * kSlotData;
            if (id[t] == 0) data[t][w] = 0.f;
        }
        for (int i = tid; i < n * kSlotData; i += kThreads) {
            const int d = i / kSlotData, w = i - d * kSlotData;
            const int t = dslot[d];
            if (t >= 0) data[t][w] = rows[(size_t)d * kRowWords + (w < kDataKeypoints ? kOffBox + w : kOffKeypoints + w - kDataKeypoints)];
        }
        if (tid < n) {
            unsigned char* o = a.out + (size_t)(first + tid) * kOutBytes;
            const int t = dslot[tid];
            ((int*)o)[0] = t >= 0 ? id[t] : 0;
            ((int*)o)[1] = t;
            ((int*)o)[2] = t >= 0 ? hits[t] : 0;
            ((int*)o)[3] = dflags[tid];
            *(double*)(o + 16) = dsim[tid];
        }
        if constexpr (kMotion) {                          // the image's max_tracks coasting rows: step 0's pose, the rest zero
            unsigned* rows_out = a.coast + (size_t)b * T * kCoastWords;
            for (int i = tid; i < T * kCoastWords; i += kThreads) {
                const int t = i / kCoastWords, w = i - t * kCoastWords;
                const int r = coast_row[t];
                if (r >= 0)
                    rows_out[r * kCoastWords + w] = w == 0 ? (unsigned)id[t] : w == 1 ? (unsigned)misses[t] : __float_as_uint(pred[t][w - 2]);
                if (t >= num_coast) rows_out[i] = 0u;
            }
        }
        __syncthreads();
    }

    for (int i = tid; i < T * kSlotData; i += kThreads) {
        const int t = i / kSlotData, w = i - t * kSlotData;
        nst[kStateHeaderWords + t * kSlotWords + kSlotInts + w] = __float_as_int(data[t][w]);
    }
    if (tid < T) {
        int* p = nst + kStateHeaderWords + tid * kSlotWords;
        p[0] = id[tid]; p[1] = hits[tid]; p[2] = age[tid]; p[3] = misses[tid];
    }
    if (tid < kStateHeaderWords) nst[tid] = tid < 2 ? counters[tid] : 0;
    if constexpr (kMotion) {
        int* mst = a.motion_next + (size_t)s * motion_stream_words(T);
        if (tid < T) {
            int* m = mst + kMotionHeaderWords + tid * kMotionSlotWords;
            m[0] = id[tid]; m[1] = seen[tid];
            for (int c = 0; c < kVelocities; ++c) m[2 + c] = __float_as_int(vel[tid][c]);
        }
        if (tid < kMotionHeaderWords) mst[tid] = 0;
    }
}

}  // namespace

extern "C" size_t mpn_pose_track_state_bytes(int streams, int max_tracks) {
    if (streams < 1 || streams > kMaxRows || max_tracks < 1 || max_tracks > kMaxTracks) return 0;
    return (size_t)streams * stream_words(max_tracks) * 4;
}

extern "C" size_t mpn_pose_track_out_bytes(int B, int max_boxes) {
    if (B < 1 || max_boxes < 1 || max_boxes > kMaxBoxes || (long long)B * max_boxes > kMaxRows) return 0;
    return (size_t)B * max_boxes * kOutBytes;
}

extern "C" size_t mpn_pose_track_motion_state_bytes(int streams, int max_tracks) {
    if (streams < 1 || streams > kMaxRows || max_tracks < 1 || max_tracks > kMaxTracks) return 0;
    return (size_t)streams * motion_stream_words(max_tracks) * 4;
}

extern "C" size_t mpn_pose_track_coast_bytes(int B, int max_tracks) {
    if (B < 1 || B > kMaxRows || max_tracks < 1 || max_tracks > kMaxTracks) return 0;
    return (size_t)B * max_tracks * kCoastWords * 4;
}

// what mpn_pose_track_motion passes on top of its siblings' arguments
struct MotionLaunch {
    float velocity_gain, damping;
    const void* prev;
    void* next;
    void* coast;
};

// the checks and the launch of all entries; `who` is the entry's name in the messages, `m` is null for the entries without motion
static int launch_pose_track(const char* who, int assignment, const MotionLaunch* m, const void* record, int B, int max_boxes,
                             int streams, int max_tracks, int similarity, float match_threshold, float new_track_score,
                             int max_misses, const void* prev, void* next, void* out, mpn_stream_t stream) {
    MPN_REQUIRE(record && prev && next && out && (!m || (m->prev && m->next && m->coast)), MPN_ERR_BAD_ARG, "%s: null pointer", who);
    MPN_REQUIRE(streams >= 1 && B >= 1 && B % streams == 0, MPN_ERR_BAD_SHAPE,
                "%s: B = %d images are not streams = %d times a whole number of frames", who, B, streams);
    MPN_REQUIRE(max_tracks >= 1 && max_tracks <= kMaxTracks, MPN_ERR_BAD_SHAPE,
                "%s: max_tracks = %d, one lane of a wave per slot takes 1..%d", who, max_tracks, kMaxTracks);
    MPN_REQUIRE(max_boxes >= 1 && max_boxes <= kMaxBoxes && (long long)B * max_boxes <= kMaxRows, MPN_ERR_BAD_SHAPE,
                "%s: B = %d, max_boxes = %d (at most %d per image, %d rows)", who, B, max_boxes, kMaxBoxes, kMaxRows);
    MPN_REQUIRE(similarity == 0 || similarity == 1, MPN_ERR_BAD_SHAPE, "%s: similarity must be 0 (IoU) or 1 (OKS)", who);
    MPN_REQUIRE(assignment == 0 || assignment == 1, MPN_ERR_BAD_SHAPE, "%s: assignment must be 0 (greedy) or 1 (optimal)", who);
    MPN_REQUIRE(max_misses >= 0, MPN_ERR_BAD_SHAPE, "%s: max_misses = %d is negative", who, max_misses);
    if (m) {                                              // (a NaN fails both comparisons)
        MPN_REQUIRE(m->velocity_gain >= 0.f && m->velocity_gain <= 1.f, MPN_ERR_BAD_ARG,
                    "%s: velocity_gain = %g must be in 0..1", who, (double)m->velocity_gain);
        MPN_REQUIRE(m->damping >= 0.f && m->damping <= 1.f, MPN_ERR_BAD_ARG, "%s: damping = %g must be in 0..1", who,
                    (double)m->damping);
    }
    MPN_REQUIRE(mpn_aligned16(record) && (((uintptr_t)prev | (uintptr_t)next | (uintptr_t)out) & 7u) == 0, MPN_ERR_BAD_ALIGN,
                "%s: record must be 16-byte, prev / next / out 8-byte aligned", who);
    MPN_REQUIRE(!m || (((uintptr_t)m->prev | (uintptr_t)m->next | (uintptr_t)m->coast) & 7u) == 0, MPN_ERR_BAD_ALIGN,
                "%s: motion_prev / motion_next / coast_out must be 8-byte aligned", who);
    MPN_REQUIRE(prev != next, MPN_ERR_BAD_ARG,
                "%s: prev and next are one buffer; the launch is a pure function of (record, prev)", who);
    MPN_REQUIRE(!m || m->prev != m->next, MPN_ERR_BAD_ARG,
                "%s: motion_prev and motion_next are one buffer; the launch is a pure function of (record, prev, motion_prev)", who);
    TrackArgs a = {(const int*)record, (const float*)((const char*)record + header_words(B) * 4), (const int*)prev, (int*)next,
                   (unsigned char*)out, B, max_boxes, streams, max_tracks, similarity, max_misses, match_threshold,
                   new_track_score, nullptr, nullptr, nullptr, 0.f, 0.f};
    if (m) {
        a.motion_prev = (const int*)m->prev; a.motion_next = (int*)m->next; a.coast = (unsigned*)m->coast;
        a.velocity_gain = m->velocity_gain; a.damping = m->damping;
        if (assignment == 1) pose_track_kernel<true, true><<<streams, kThreads, 0, (hipStream_t)stream>>>(a);
        else pose_track_kernel<false, true><<<streams, kThreads, 0, (hipStream_t)stream>>>(a);
    } else {
        if (assignment == 1) pose_track_kernel<true, false><<<streams, kThreads, 0, (hipStream_t)stream>>>(a);
        else pose_track_kernel<false, false><<<streams, kThreads, 0, (hipStream_t)stream>>>(a);
    }
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}

extern "C" int mpn_pose_track(const void* record, int B, int max_boxes, int streams, int max_tracks, int similarity,
                              float match_threshold, float new_track_score, int max_misses, const void* prev, void* next,
                              void* out, mpn_stream_t stream) {
    return launch_pose_track("pose_track", 0, nullptr, record, B, max_boxes, streams, max_tracks, similarity, match_threshold,
                             new_track_score, max_misses, prev, next, out, stream);
}

extern "C" int mpn_pose_track_optimal(const void* record, int B, int max_boxes, int streams, int max_tracks, int similarity,
                                      float match_threshold, float new_track_score, int max_misses, const void* prev,
                                      void* next, void* out, mpn_stream_t stream) {
    return launch_pose_track("pose_track_optimal", 1, nullptr, record, B, max_boxes, streams, max_tracks, similarity,
                             match_threshold, new_track_score, max_misses, prev, next, out, stream);
}

extern "C" int mpn_pose_track_motion(const void* record, int B, int max_boxes, int streams, int max_tracks, int similarity,
                                     int assignment, float match_threshold, float new_track_score, int max_misses,
                                     float velocity_gain, float damping, const void* prev, void* next, const void* motion_prev,
                                     void* motion_next, void* out, void* coast_out, mpn_stream_t stream) {
    const MotionLaunch m = {velocity_gain, damping, motion_prev, motion_next, coast_out};
    return launch_pose_track("pose_track_motion", assignment, &m, record, B, max_boxes, streams, max_tracks, similarity,
                             match_threshold, new_track_score, max_misses, prev, next, out, stream);
}
