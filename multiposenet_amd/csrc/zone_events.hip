// Zones and counting lines: which tracked persons stand inside which polygon, who entered and who left, how long each stayed,
// and how many crossed a line in each direction. What a camera user reads off the identities of mpn_pose_track.
//   mpn_zone_events   record + track rows (read in place) + the geometry table + prev state -> next state + a 104-byte row per
//                     record row and a 576-byte row per image. PURE like mpn_pose_smooth: prev is never written; the caller
//                     advances the state by copying next over prev.
// ONE block per stream (B = streams * F images, stream s owns images s*F .. s*F+F-1 in time order); the block walks its F frames
// in order with the stream's state - the counters and 64 slots keyed by track id - and the geometry in LDS. Per frame:
//   phase A  wave 0, lane = record row: the row's anchor, flags and track id -> LDS
//   phase B  all four waves, lane = record row, wave q = zones 4q .. 4q+3: the crossing-number test -> a partial mask in LDS
//   phase C  wave 0, lane = slot: the rows take their slots, serially in row order (a ballot for the match, a wave minimum for
//            the eviction); slot ids, last frames and the taken flags stay in registers
//   phase D  wave 0, lane = record row: the debounced membership, the dwell, the line crossings, the slot's new anchor; the
//            person rows; a ballot per zone and line for the image row and the cumulative counters
// Latency-bound glue like mpn_pose_smooth (microseconds behind a network pass of milliseconds): not tuned beyond that.
#include "common.h"
#include "person_anchor.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBoxes = 64;           // one lane of wave 0 per record row
constexpr int kMaxRows = 4096;          // mpn_pose_gather's own limit on B * max_boxes
constexpr int kSlots = 64;              // always: mpn_pose_track's largest table; one lane of wave 0 per slot
constexpr int kMaxZones = 16, kMaxLines = 16, kMaxVertices = 16;
// the record's row (pose_gather.hip), in 32-bit words; a row of mpn_pose_track's out in bytes (track_id first)
constexpr int kRowWords = 108, kTrackRowBytes = 24;
// the table, in bytes
constexpr int kTabHeight = 16, kTabCounts = 40, kTabVertices = 104, kTabLines = kTabVertices + kMaxZones * kMaxVertices * 16;
constexpr int kTableBytes = kTabLines + kMaxLines * 32;                                  // 4712
// the state of one stream, in 32-bit words: {frames, 0, 0, 0}, four counters of 16, then 64 slots of 28 words
constexpr int kStateHeaderWords = 4, kOffEntries = 4, kOffExits = 20, kOffPositive = 36, kOffNegative = 52, kOffSlots = 68;
constexpr int kSlotWords = 28;          // id, inside, last, 0; f64 ax, ay; int32 entered_frame[16]; uint8 run[16]
constexpr int kSlotId = 0, kSlotInside = 1, kSlotLast = 2, kSlotAnchor = 4, kSlotEntered = 8, kSlotRun = 24;
constexpr int kStreamWords = kOffSlots + kSlots * kSlotWords;                            // 1860 words = 7440 bytes
static_assert(kStreamWords % 2 == 0 && kOffSlots % 2 == 0 && kSlotWords % 2 == 0, "the anchors are aligned doubles");
// the output rows, in bytes: a person row {inside, entered, exited, positive, negative, flags; f64 anchor[2]; int32 dwell[16]}
constexpr int kPersonBytes = 104, kPersonWords = kPersonBytes / 4, kImageWords = 9 * 16, kImageBytes = kImageWords * 4;
constexpr unsigned kFlagTracked = 1u, kFlagNoAnchor = mpn_anchor::kFlagNoAnchor;     // (bit 1: the anchor came from the ankles)

inline size_t header_words(int B) { return ((size_t)(2 * B + 2) + 3) / 4 * 4; }

struct ZoneArgs {
    const int* header;
    const float* rows;
    const unsigned char* track_rows;
    const unsigned char* table;
    const unsigned* prev;
    unsigned* next;
    unsigned char* out;
    int B, max_boxes, streams;
};

__global__ __launch_bounds__(kThreads) void zone_events_kernel(ZoneArgs a) {
    __shared__ double state64[kStreamWords / 2];                  // the stream's state, addressed in words below
    __shared__ double vx[kMaxZones][kMaxVertices], vy[kMaxZones][kMaxVertices];
    __shared__ double line[kMaxLines][4];                         // Px, Py, Qx, Qy
    __shared__ int vcount[kMaxZones];
    __shared__ double ancx[kMaxBoxes], ancy[kMaxBoxes];           // the frame's staging rows
    __shared__ int rtid[kMaxBoxes];                               // the track id of a row that can take a slot, else 0
    __shared__ unsigned rawpart[kThreads / 64][kMaxBoxes];        // wave q's four zones of the raw mask of a row
    unsigned* st = (unsigned*)state64;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = a.B / a.streams;
    const int all_rows = a.B * a.max_boxes;
    const unsigned* pst = a.prev + (size_t)s * kStreamWords;
    unsigned* nst = a.next + (size_t)s * kStreamWords;
    unsigned char* image_out = a.out + (size_t)all_rows * kPersonBytes;

    // the table, every count clamped: a bad table cannot index out of range
    const int* ti = (const int*)a.table;
    int Z = ti[0], L = ti[1], min_frames = ti[2];
    const int anchor_mode = ti[3];
    Z = Z < 0 ? 0 : (Z > kMaxZones ? kMaxZones : Z);
    L = L < 0 ? 0 : (L > kMaxLines ? kMaxLines : L);
    min_frames = min_frames < 1 ? 1 : (min_frames > 255 ? 255 : min_frames);
    const double height = *(const double*)(a.table + kTabHeight), width = *(const double*)(a.table + kTabHeight + 8);
    const double min_score = *(const double*)(a.table + kTabHeight + 16);
    if (tid < kMaxZones) {
        const int c = ((const int*)(a.table + kTabCounts))[tid];
        vcount[tid] = c < 3 ? 3 : (c > kMaxVertices ? kMaxVertices : c);
    }
    for (int i = tid; i < kMaxZones * kMaxVertices; i += kThreads) {
        const double* v = (const double*)(a.table + kTabVertices) + 2 * i;
        vx[i / kMaxVertices][i % kMaxVertices] = v[0];
        vy[i / kMaxVertices][i % kMaxVertices] = v[1];
    }
    if (tid < kMaxLines * 4) line[tid / 4][tid % 4] = ((const double*)(a.table + kTabLines))[tid];
    for (int i = tid; i < kStreamWords; i += kThreads) st[i] = pst[i];

    // the record's counts, clamped as mpn_pose_track clamps them: nothing is indexed out of range
    int total = a.header[0];
    total = total < 0 ? 0 : (total > all_rows ? all_rows : total);
    // rows behind the record's total are zero: the blocks share them
    for (long long w = (long long)total * kPersonWords + s * kThreads + tid; w < (long long)all_rows * kPersonWords;
         w += (long long)a.streams * kThreads)
        ((unsigned*)a.out)[w] = 0u;
    int ahead = 0;                                                // kept rows of the images before the frame
    for (int i = 0; i < s * F; ++i) {
        ahead += a.header[1 + i] > 0 ? a.header[1 + i] : 0;
        if (ahead > all_rows) ahead = all_rows;                   // (past the total either way; the sum cannot wrap)
    }
    const int frames_before = (int)pst[0];
    __syncthreads();

    for (int f = 0; f < F; ++f) {
        const int b = s * F + f;
        const int now = frames_before + f + 1;
        int n = a.header[1 + b];
        int first = ahead;
        ahead += n > 0 ? n : 0;
        if (ahead > all_rows) ahead = all_rows;
        n = n < 0 ? 0 : (n > a.max_boxes ? a.max_boxes : n);
        if (first > total) first = total;
        if (first + n > total) n = total - first;

        // phase A
        unsigned flags = 0u;                                      // (wave 0: of row `lane`)
        double cx = 0.0, cy = 0.0;
        if (wave == 0) {
            int id = 0;
            if (lane < n) {
                flags = mpn_anchor::person_anchor(a.rows + (size_t)(first + lane) * kRowWords, anchor_mode, min_score, height, width,
                                                  cx, cy);
                id = *(const int*)(a.track_rows + (size_t)(first + lane) * kTrackRowBytes);
                if (id < 0 || (flags & kFlagNoAnchor)) id = 0;
            }
            ancx[lane] = cx; ancy[lane] = cy; rtid[lane] = id;
        }
        __syncthreads();

        // phase B: the crossing number of the row's anchor against zones 4 * wave .. 4 * wave + 3
        {
            unsigned mask = 0u;
            if (lane < n) {
                const double ax = ancx[lane], ay = ancy[lane];
                for (int z = 4 * wave; z < 4 * wave + 4 && z < Z; ++z) {
                    const int nv = vcount[z];
                    int crossed = 0;
                    double x1 = vx[z][nv - 1], y1 = vy[z][nv - 1];
                    for (int e = 0; e < nv; ++e) {
                        const double x2 = vx[z][e], y2 = vy[z][e];
                        if ((y1 > ay) != (y2 > ay)) {
                            const double t = (x2 - x1) * (ay - y1) - (ax - x1) * (y2 - y1);
                            crossed += (y2 > y1 ? t > 0.0 : t < 0.0) ? 1 : 0;
                        }
                        x1 = x2; y1 = y2;
                    }
                    mask |= (unsigned)(crossed & 1) << z;
                }
            }
            rawpart[wave][lane] = mask;                           // (a row without an anchor is masked out in phase D)
        }
        __syncthreads();

        if (wave == 0) {
            // phase C: lane = slot. The values that decide are the same in every lane (ballots, the butterfly's minimum).
            int slot_id = (int)st[kOffSlots + lane * kSlotWords + kSlotId];
            int slot_last = (int)st[kOffSlots + lane * kSlotWords + kSlotLast];
            bool slot_taken = false;
            int my_slot = -1;                                     // lane = row again: the slot row `lane` took
            bool my_fresh = false;
            for (int r = 0; r < n; ++r) {
                const int id = rtid[r];
                if (id <= 0) continue;                            // (uniform)
                const unsigned long long match = __ballot(slot_id == id);
                int k;
                bool fresh = false;
                if (match != 0ull) {
                    k = __ffsll(match) - 1;
                    if ((__ballot(slot_taken) >> k) & 1ull) continue;     // an earlier row of the frame has this id: untracked
                } else {
                    long long key = slot_taken ? 0x7fffffffffffffffll : (((long long)slot_last << 6) | lane);
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const long long other = __shfl_xor(key, o, 64);
                        key = other < key ? other : key;
                    }
                    k = (int)(key & 63);                          // 64 slots, at most 64 rows: one is always free
                    fresh = true;
                }
                if (lane == k) {
                    slot_taken = true;
                    if (fresh) { slot_id = id; slot_last = 0; }
                }
                if (lane == r) { my_slot = k; my_fresh = fresh; }
            }

            // phase D: lane = row; the rows' slots are distinct
            const bool valid = lane < n;
            const bool has_anchor = valid && !(flags & kFlagNoAnchor);
            const unsigned raw = has_anchor ? (rawpart[0][lane] | rawpart[1][lane] | rawpart[2][lane] | rawpart[3][lane]) : 0u;
            unsigned inside = raw, entered = 0u, exited = 0u, positive = 0u, negative = 0u;
            int dwell[kMaxZones];
#pragma unroll
            for (int z = 0; z < kMaxZones; ++z) dwell[z] = 0;
            if (my_slot >= 0) {
                unsigned* slot = st + kOffSlots + my_slot * kSlotWords;
                if (my_fresh) {
                    for (int w = 0; w < kSlotWords; ++w) slot[w] = 0u;
                    slot[kSlotId] = (unsigned)rtid[lane];
                }
                flags |= kFlagTracked;
                inside = slot[kSlotInside];
                const int last = (int)slot[kSlotLast];
                int* entered_frame = (int*)(slot + kSlotEntered);
                unsigned char* run = (unsigned char*)(slot + kSlotRun);
#pragma unroll
                for (int z = 0; z < kMaxZones; ++z) {
                    if (z >= Z) break;
                    const unsigned bit = 1u << z;
                    if (((raw ^ inside) & bit) == 0u) {
                        run[z] = 0;
                    } else {
                        const int steps = (int)run[z] + 1;
                        if (steps >= min_frames) {
                            inside ^= bit;
                            run[z] = 0;
                            if (inside & bit) { entered |= bit; entered_frame[z] = now; }
                            else { exited |= bit; entered_frame[z] = 0; }
                        } else {
                            run[z] = (unsigned char)steps;
                        }
                    }
                    dwell[z] = (inside & bit) ? now - entered_frame[z] + 1 : 0;
                }
                double* slot_anchor = (double*)(slot + kSlotAnchor);
                if (last != 0) {
                    const double ax = slot_anchor[0], ay = slot_anchor[1];
                    for (int l = 0; l < L; ++l) {
                        const double px = line[l][0], py = line[l][1], qx = line[l][2], qy = line[l][3];
                        const double da = (qx - px) * (ay - py) - (qy - py) * (ax - px);
                        const double dc = (qx - px) * (cy - py) - (qy - py) * (cx - px);
                        const double ep = (cx - ax) * (py - ay) - (cy - ay) * (px - ax);
                        const double eq = (cx - ax) * (qy - ay) - (cy - ay) * (qx - ax);
                        if ((da > 0.0) != (dc > 0.0) && (ep > 0.0) != (eq > 0.0)) {
                            if (dc > 0.0) positive |= 1u << l; else negative |= 1u << l;
                        }
                    }
                }
                slot[kSlotInside] = inside;
                slot[kSlotLast] = (unsigned)now;
                slot_anchor[0] = cx; slot_anchor[1] = cy;
            }
            if (valid) {
                unsigned char* o = a.out + (size_t)(first + lane) * kPersonBytes;
                unsigned* ow = (unsigned*)o;
                ow[0] = inside; ow[1] = entered; ow[2] = exited; ow[3] = positive; ow[4] = negative; ow[5] = flags;
                *(double*)(o + 24) = cx;
                *(double*)(o + 32) = cy;
#pragma unroll
                for (int z = 0; z < kMaxZones; ++z) ((int*)(o + 40))[z] = dwell[z];
            }
            // the image row and the cumulative counters: lane i of the first 16 keeps zone i and line i
            unsigned occupancy = 0u, entries = 0u, exits = 0u, pos = 0u, neg = 0u;
            for (int i = 0; i < kMaxZones; ++i) {
                const unsigned c0 = __popcll(__ballot(valid && ((inside >> i) & 1u)));
                const unsigned c1 = __popcll(__ballot(valid && ((entered >> i) & 1u)));
                const unsigned c2 = __popcll(__ballot(valid && ((exited >> i) & 1u)));
                const unsigned c3 = __popcll(__ballot(valid && ((positive >> i) & 1u)));
                const unsigned c4 = __popcll(__ballot(valid && ((negative >> i) & 1u)));
                if (lane == i) { occupancy = c0; entries = c1; exits = c2; pos = c3; neg = c4; }
            }
            if (lane < 16) {
                unsigned* o = (unsigned*)(image_out + (size_t)b * kImageBytes);
                const unsigned te = st[kOffEntries + lane] + entries, tx = st[kOffExits + lane] + exits;
                const unsigned tp = st[kOffPositive + lane] + pos, tn = st[kOffNegative + lane] + neg;
                st[kOffEntries + lane] = te; st[kOffExits + lane] = tx; st[kOffPositive + lane] = tp; st[kOffNegative + lane] = tn;
                o[0 * 16 + lane] = occupancy; o[1 * 16 + lane] = entries; o[2 * 16 + lane] = exits;
                o[3 * 16 + lane] = pos; o[4 * 16 + lane] = neg;
                o[5 * 16 + lane] = te; o[6 * 16 + lane] = tx; o[7 * 16 + lane] = tp; o[8 * 16 + lane] = tn;
            }
        }
        // (wave 0 writes the staging rows of the next frame only behind this frame's phase B: the two barriers suffice)
    }
    __syncthreads();

    for (int i = tid; i < kStreamWords; i += kThreads)
        nst[i] = i == 0 ? (unsigned)(frames_before + F) : (i < kStateHeaderWords ? 0u : st[i]);
}

}  // namespace

extern "C" size_t mpn_zone_table_bytes(void) { return kTableBytes; }

extern "C" size_t mpn_zone_state_bytes(int streams) {
    if (streams < 1 || streams > kMaxRows) return 0;
    return (size_t)streams * kStreamWords * 4;
}

extern "C" size_t mpn_zone_out_bytes(int B, int max_boxes) {
    if (B < 1 || max_boxes < 1 || max_boxes > kMaxBoxes || (long long)B * max_boxes > kMaxRows) return 0;
    return (size_t)B * max_boxes * kPersonBytes + (size_t)B * kImageBytes;
}

extern "C" int mpn_zone_events(const void* record, const void* track_rows, int B, int max_boxes, int streams, const void* table,
                               const void* prev, void* next, void* out, mpn_stream_t stream) {
    MPN_REQUIRE(record && track_rows && table && prev && next && out, MPN_ERR_BAD_ARG, "zone_events: null pointer");
    MPN_REQUIRE(prev != next, MPN_ERR_BAD_ARG,
                "zone_events: prev and next are one buffer; the launch is a pure function of (record, track_rows, table, prev)");
    MPN_REQUIRE(streams >= 1 && B >= 1 && B % streams == 0, MPN_ERR_BAD_SHAPE,
                "zone_events: B = %d images are not streams = %d times a whole number of frames", B, streams);
    MPN_REQUIRE(max_boxes >= 1 && max_boxes <= kMaxBoxes && (long long)B * max_boxes <= kMaxRows, MPN_ERR_BAD_SHAPE,
                "zone_events: B = %d, max_boxes = %d (at most %d per image, %d rows)", B, max_boxes, kMaxBoxes, kMaxRows);
    MPN_REQUIRE(mpn_aligned16(record) && (((uintptr_t)track_rows | (uintptr_t)table | (uintptr_t)prev | (uintptr_t)next |
                                           (uintptr_t)out) & 7u) == 0,
                MPN_ERR_BAD_ALIGN, "zone_events: record must be 16-byte, track_rows / table / prev / next / out 8-byte aligned");
    ZoneArgs a = {(const int*)record, (const float*)((const char*)record + header_words(B) * 4), (const unsigned char*)track_rows,
                  (const unsigned char*)table, (const unsigned*)prev, (unsigned*)next, (unsigned char*)out, B, max_boxes, streams};
    zone_events_kernel<<<streams, kThreads, 0, (hipStream_t)stream>>>(a);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
