// One-Euro smoothing (Casiez, Roussel, Vogel, CHI 2012) of the tracked persons' keypoints on the device, and the per-joint
// velocities its derivative estimate gives: one first-order low-pass per (stream, track slot, joint) whose cutoff rises with
// the estimated speed.
//   mpn_pose_smooth   record + mpn_pose_track's rows (both read in place) + prev state -> next state + one 340-byte row per
//                     record row {keypoints[17][3], velocities[17][2]}. PURE as mpn_pose_track is: prev is never written, the
//                     caller advances the state by copying next over prev (include/mpn.h has the definition in full).
// ONE block per stream, as in pose_track.hip; the stream's filters live in LDS (64 slots x 88 words = 22 KB). The block walks
// its F frames in order. Per frame:
//   phase A  the (row, joint) items strided over the block (up to 64 x 17 = 1088 of them): an item reads its slot's id, steps
//            its own joint's filter in LDS and puts its five output words into the frame's staging rows. Distinct rows of a
//            frame name distinct slots and an item touches only its joint's group: no atomics.
//   phase B  the rows' track ids written into their slots (phase A only read them: a slot given to another track restarts all
//            17 joints); the staging rows copied to `out`, consecutive lanes to consecutive words.
// Every float operation is one IEEE f32 operation in the documented order (no contraction, correctly rounded division):
// tests/smooth_ref.py is the same arithmetic in numpy and the comparison is of bytes.
// Latency-bound glue like mpn_pose_track (microseconds behind a network pass of milliseconds): not tuned beyond that.
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxTracks = 64, kMaxBoxes = 64, kMaxRows = 4096;   // mpn_pose_track's limits
constexpr int kJoints = 17;
// the record's row (pose_gather.hip) and mpn_pose_track's output row, in 32-bit words
constexpr int kRowWords = 108, kOffKeypoints = 57;
constexpr int kTrackWords = 6, kTrackId = 0, kTrackSlot = 1;
// the state of one stream, in 32-bit words: {frames, 0, 0, 0}, then max_tracks slots of {id, 17 x {last, x_hat, y_hat, dx_hat,
// dy_hat}, 0, 0}
constexpr int kStateHeaderWords = 4, kGroupWords = 5, kSlotWords = 88;
static_assert(1 + kJoints * kGroupWords + 2 == kSlotWords && kSlotWords % 4 == 0, "state slot layout");
// an output row: f32 keypoints[17][3], velocities[17][2]
constexpr int kOutWords = 5 * kJoints, kOutVelocities = 3 * kJoints;
constexpr float kTwoPi = 6.2831855f;

inline size_t header_words(int B) { return ((size_t)(2 * B + 2) + 3) / 4 * 4; }
__host__ __device__ inline size_t stream_words(int max_tracks) { return kStateHeaderWords + (size_t)max_tracks * kSlotWords; }

struct SmoothArgs {
    const int* header;
    const float* rows;
    const int* track;
    const int* prev;
    int* next;
    float* out;
    int B, max_boxes, streams, max_tracks;
    float rate, min_cutoff, beta, d_cutoff, min_score;
};

__device__ __forceinline__ float alpha_of(float fc, float te) {
    const float r = (kTwoPi * fc) * te;
    return r / (r + 1.f);
}

// one coordinate: (sample, the filter's value and derivative) -> both advanced
__device__ __forceinline__ void one_euro(float x, float te, float alpha_d, float min_cutoff, float beta, float& x_hat, float& dx_hat) {
    const float dx = (x - x_hat) / te;
    dx_hat = dx_hat + alpha_d * (dx - dx_hat);
    const float fc = min_cutoff + beta * fabsf(dx_hat);
    x_hat = x_hat + alpha_of(fc, te) * (x - x_hat);
}

__global__ __launch_bounds__(kThreads) void pose_smooth_kernel(SmoothArgs a) {
    __shared__ int st[kMaxTracks * kSlotWords];           // the stream's slots, as words
    __shared__ float stage[kMaxBoxes * kOutWords];        // the frame's output rows
    __shared__ int new_id[kMaxBoxes], new_slot[kMaxBoxes];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int T = a.max_tracks, F = a.B / a.streams;
    const int all_rows = a.B * a.max_boxes;
    const int* pst = a.prev + (size_t)s * stream_words(T);
    int* nst = a.next + (size_t)s * stream_words(T);

    for (int i = tid; i < T * kSlotWords; i += kThreads) st[i] = pst[kStateHeaderWords + i];
    const unsigned frames = (unsigned)pst[0];             // (unsigned: the count is not guarded against wrap, and must not trap)

    // the record's counts, clamped as mpn_pose_track clamps them: nothing is indexed out of range
    int total = a.header[0];
    total = total < 0 ? 0 : (total > all_rows ? all_rows : total);
    // rows behind the record's total are zero: the blocks share them
    for (long long w = (long long)total * kOutWords + s * kThreads + tid; w < (long long)all_rows * kOutWords;
         w += (long long)a.streams * kThreads)
        a.out[w] = 0.f;
    int ahead = 0;                                        // kept rows of the images before the frame
    for (int i = 0; i < s * F; ++i) {
        ahead += a.header[1 + i] > 0 ? a.header[1 + i] : 0;
        if (ahead > all_rows) ahead = all_rows;
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
        const int now = (int)(frames + (unsigned)f + 1u);

        // phase A
        for (int i = tid; i < n * kJoints; i += kThreads) {
            const int d = i / kJoints, k = i - d * kJoints;
            const float* kp = a.rows + (size_t)(first + d) * kRowWords + kOffKeypoints + 3 * k;
            const int* tr = a.track + (size_t)(first + d) * kTrackWords;
            const int track_id = tr[kTrackId], slot = tr[kTrackSlot];
            const bool tracked = track_id > 0 && slot >= 0 && slot < T;    // any other slot value indexes nothing
            float x = kp[0], y = kp[1], vx = 0.f, vy = 0.f;
            const float score = kp[2];
            if (tracked) {
                int* g = st + slot * kSlotWords + 1 + kGroupWords * k;
                const int last = st[slot * kSlotWords] == track_id ? g[0] : 0;    // another track's filters: restarted
                if (!(score >= a.min_score)) {
                    g[0] = 0;
                } else if (last == 0) {
                    g[0] = now;
                    g[1] = __float_as_int(x); g[2] = __float_as_int(y);
                    g[3] = 0; g[4] = 0;
                } else {
                    const float te = (float)(now - last) / a.rate;
                    const float alpha_d = alpha_of(a.d_cutoff, te);
                    float x_hat = __int_as_float(g[1]), y_hat = __int_as_float(g[2]);
                    vx = __int_as_float(g[3]); vy = __int_as_float(g[4]);
                    one_euro(x, te, alpha_d, a.min_cutoff, a.beta, x_hat, vx);
                    one_euro(y, te, alpha_d, a.min_cutoff, a.beta, y_hat, vy);
                    g[0] = now;
                    g[1] = __float_as_int(x_hat); g[2] = __float_as_int(y_hat);
                    g[3] = __float_as_int(vx); g[4] = __float_as_int(vy);
                    x = x_hat; y = y_hat;
                }
            }
            if (k == 0) { new_id[d] = tracked ? track_id : 0; new_slot[d] = slot; }
            float* o = stage + d * kOutWords;
            o[3 * k] = x; o[3 * k + 1] = y; o[3 * k + 2] = score;
            o[kOutVelocities + 2 * k] = vx; o[kOutVelocities + 2 * k + 1] = vy;
        }
        __syncthreads();

        // phase B
        if (tid < n && new_id[tid] != 0) st[new_slot[tid] * kSlotWords] = new_id[tid];
        float* out = a.out + (size_t)first * kOutWords;
        for (int i = tid; i < n * kOutWords; i += kThreads) out[i] = stage[i];
        __syncthreads();
    }

    for (int i = tid; i < T * kSlotWords; i += kThreads) nst[kStateHeaderWords + i] = st[i];
    if (tid < kStateHeaderWords) nst[tid] = tid == 0 ? (int)(frames + (unsigned)F) : 0;
}

}  // namespace

extern "C" size_t mpn_pose_smooth_state_bytes(int streams, int max_tracks) {
    if (streams < 1 || streams > kMaxRows || max_tracks < 1 || max_tracks > kMaxTracks) return 0;
    return (size_t)streams * stream_words(max_tracks) * 4;
}

extern "C" size_t mpn_pose_smooth_out_bytes(int B, int max_boxes) {
    if (B < 1 || max_boxes < 1 || max_boxes > kMaxBoxes || (long long)B * max_boxes > kMaxRows) return 0;
    return (size_t)B * max_boxes * kOutWords * 4;
}

extern "C" int mpn_pose_smooth(const void* record, const void* track_rows, int B, int max_boxes, int streams, int max_tracks,
                               float rate, float min_cutoff, float beta, float d_cutoff, float min_keypoint_score,
                               const void* prev, void* next, void* out, mpn_stream_t stream) {
    MPN_REQUIRE(record && track_rows && prev && next && out, MPN_ERR_BAD_ARG, "pose_smooth: null pointer");
    MPN_REQUIRE(prev != next, MPN_ERR_BAD_ARG,
                "pose_smooth: prev and next are one buffer; the launch is a pure function of (record, track_rows, prev)");
    MPN_REQUIRE(std::isfinite(rate) && rate > 0.f && std::isfinite(min_cutoff) && min_cutoff > 0.f && std::isfinite(d_cutoff) &&
                    d_cutoff > 0.f, MPN_ERR_BAD_ARG,
                "pose_smooth: rate = %g, min_cutoff = %g and d_cutoff = %g must be finite and > 0", (double)rate,
                (double)min_cutoff, (double)d_cutoff);
    MPN_REQUIRE(std::isfinite(beta) && beta >= 0.f, MPN_ERR_BAD_ARG, "pose_smooth: beta = %g must be finite and >= 0", (double)beta);
    MPN_REQUIRE(std::isfinite(min_keypoint_score), MPN_ERR_BAD_ARG, "pose_smooth: min_keypoint_score = %g must be finite",
                (double)min_keypoint_score);
    MPN_REQUIRE(streams >= 1 && B >= 1 && B % streams == 0, MPN_ERR_BAD_SHAPE,
                "pose_smooth: B = %d images are not streams = %d times a whole number of frames", B, streams);
    MPN_REQUIRE(max_tracks >= 1 && max_tracks <= kMaxTracks, MPN_ERR_BAD_SHAPE,
                "pose_smooth: max_tracks = %d, mpn_pose_track takes 1..%d", max_tracks, kMaxTracks);
    MPN_REQUIRE(max_boxes >= 1 && max_boxes <= kMaxBoxes && (long long)B * max_boxes <= kMaxRows, MPN_ERR_BAD_SHAPE,
                "pose_smooth: B = %d, max_boxes = %d (at most %d per image, %d rows)", B, max_boxes, kMaxBoxes, kMaxRows);
    MPN_REQUIRE(mpn_aligned16(record) && (((uintptr_t)track_rows | (uintptr_t)prev | (uintptr_t)next | (uintptr_t)out) & 7u) == 0,
                MPN_ERR_BAD_ALIGN, "pose_smooth: record must be 16-byte, track_rows / prev / next / out 8-byte aligned");
    SmoothArgs a = {(const int*)record, (const float*)((const char*)record + header_words(B) * 4), (const int*)track_rows,
                    (const int*)prev, (int*)next, (float*)out, B, max_boxes, streams, max_tracks,
                    rate, min_cutoff, beta, d_cutoff, min_keypoint_score};
    pose_smooth_kernel<<<streams, kThreads, 0, (hipStream_t)stream>>>(a);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
