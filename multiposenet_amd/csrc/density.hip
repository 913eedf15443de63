// Density maps: where in the picture persons stand, accumulated per grid cell in device state, and laid over the annotated frames.
//   mpn_density_map    record (+ track rows, optional) + prev state -> next state + a row per record row and per image + a
//                      snapshot of the shown plane per image. PURE like mpn_track_trails: prev is never written. ONE block per
//                      stream; the block walks its F frames in order. The 64 slots (1 KB) live in LDS; the two planes live in
//                      GLOBAL memory: frame 0 reads them from prev, every later frame from next, and every frame writes next.
//                      Cell i belongs to thread i % 256 in every frame, so the planes need no barrier of their own. Per frame:
//                        phases A, C  wave 0: anchors and slots, word for word as in zone_events.hip
//                        phase D      wave 0, lane = record row: the visit, the row's footprint as a rectangle of cells -> LDS
//                        the pass     all threads, one cell each per step: halve, count the rows whose rectangle holds the cell
//                                     (and whose visit is the cell), add saturating, store, copy to the snapshot. No atomics: a
//                                     cell is one thread's, the adds commute. Eight cells a step, so that their loads are in
//                                     flight together: every frame reads what the frame before stored.
//                      NOT free: the frames of a stream run in series inside one block, each a pass over all G cells against
//                      all its rows - 0.29 ms for 16 frames of 20 persons over 45 x 80 cells (profiles/density.json).
//   mpn_draw_density   the snapshots -> a colour wash blended IN PLACE over the RGBA frames. Two launches:
//                        density_levels_kernel  one thread per (image, cell): the cell's level 0..255 as a byte
//                        density_raster_kernel  an image as a flat array of pixels, 4 per thread as one 16-byte access; per
//                                               pixel the (bilinear) level, the table's ink and alpha, BLEND8
#include "common.h"
#include "person_anchor.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxRows = 4096;          // mpn_pose_gather's own limit on B * max_boxes
constexpr int kSlots = 64;              // always, as in mpn_zone_events: one lane of wave 0 per slot
constexpr int kMaxBoxes = 64;           // one lane of wave 0 per record row
constexpr int kChunk = 8;               // cells per thread and step of the pass over the planes
constexpr int kMaxCells = 16384, kMinCell = 4, kMaxCell = 256, kMaxSide = 8192, kMaxHalfLife = 65535;
constexpr int kRowWords = 108, kTrackRowBytes = 24;
// the state of one stream, in 32-bit words: {frames, max_dwell, max_visits, 0 x 5}, 64 slots {id, last, cell1, 0}, dwell[G], visits[G]
constexpr int kHeaderWords = 8, kSlotWords = 4, kSlotId = 0, kSlotLast = 1, kSlotCell = 2;
constexpr int kOffPlanes = kHeaderWords + kSlots * kSlotWords;
constexpr unsigned kFlagTracked = 1u, kFlagNoAnchor = mpn_anchor::kFlagNoAnchor, kFlagOutside = 8u, kFlagVisit = 16u;
constexpr int kOutRowWords = 4, kImageRowWords = 4;

inline size_t header_words(int B) { return ((size_t)(2 * B + 2) + 3) / 4 * 4; }
inline int cells_of(int side, int cell) { return (side + cell - 1) / cell; }

struct DensityArgs {
    const int* header;
    const float* rows;
    const unsigned char* track_rows;    // or nullptr
    const unsigned* prev;
    unsigned* next;
    unsigned* out;
    unsigned* snapshots;                // or nullptr
    int B, max_boxes, streams, height, width, cell, gh, gw, footprint, anchor_mode, half_life, show;
    double min_score;
};

__device__ __forceinline__ unsigned sat_add(unsigned v, unsigned n) {
    const unsigned s = v + n;
    return s < v ? 0xFFFFFFFFu : s;
}

// the first cell index c in 0..n whose centre (2c + 1) * cell * 0.5 is >= x (n when none is); the products are exact
__device__ __forceinline__ int first_centre_at_or_behind(double x, int cell, int n) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((double)((2 * mid + 1) * cell) * 0.5 >= x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void density_map_kernel(DensityArgs a) {
    __shared__ unsigned slots[kSlots * kSlotWords];
    __shared__ int rtid[kMaxBoxes];                               // the track id of a row that can take a slot, else 0
    __shared__ int4 rect[kMaxBoxes];                              // the row's cells: columns x..y-1, rows z..w-1
    __shared__ int visit[kMaxBoxes];                              // the cell the row visits, else -1
    __shared__ unsigned frame_counts[2];                          // counted, visits
    __shared__ unsigned part[2][kWaves];
    __shared__ unsigned maxima[2];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = a.B / a.streams, G = a.gh * a.gw, gw = a.gw;
    const size_t stream_words = (size_t)kOffPlanes + 2 * (size_t)G;
    const int all_rows = a.B * a.max_boxes;
    const unsigned* pst = a.prev + (size_t)s * stream_words;
    unsigned* nst = a.next + (size_t)s * stream_words;
    for (int i = tid; i < kSlots * kSlotWords; i += kThreads) slots[i] = pst[kHeaderWords + i];
    if (tid < 2) maxima[tid] = pst[1 + tid];

    // the record's counts, clamped as mpn_zone_events clamps them: nothing is indexed out of range
    int total = a.header[0];
    total = total < 0 ? 0 : (total > all_rows ? all_rows : total);
    // rows behind the record's total are zero: the blocks share them
    for (long long w = (long long)total * kOutRowWords + s * kThreads + tid; w < (long long)all_rows * kOutRowWords;
         w += (long long)a.streams * kThreads)
        a.out[w] = 0u;
    int ahead = 0;                                                // kept rows of the images before the frame
    for (int i = 0; i < s * F; ++i) {
        ahead += a.header[1 + i] > 0 ? a.header[1 + i] : 0;
        if (ahead > all_rows) ahead = all_rows;
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

        if (wave == 0) {
            // phase A: lane = row
            unsigned flags = 0u;
            int id = 0, k = -1, row_cell = -1, col_cell = -1;
            int4 cells = make_int4(0, 0, 0, 0);
            if (lane < n) {
                const float* row = a.rows + (size_t)(first + lane) * kRowWords;
                double cx, cy;
                flags = mpn_anchor::person_anchor(row, a.anchor_mode, a.min_score, (double)a.height, (double)a.width, cx, cy);
                if (!(flags & kFlagNoAnchor)) {
                    if (cx >= 0.0 && cx < (double)a.width && cy >= 0.0 && cy < (double)a.height) {
                        col_cell = (int)cx / a.cell; row_cell = (int)cy / a.cell;
                        k = row_cell * gw + col_cell;
                    } else {
                        flags |= kFlagOutside;
                    }
                    if (a.footprint == 0) {
                        if (k >= 0) cells = make_int4(col_cell, col_cell + 1, row_cell, row_cell + 1);
                    } else {
                        const double y0 = (double)row[mpn_anchor::kOffBox] * (double)a.height;
                        const double x0 = (double)row[mpn_anchor::kOffBox + 1] * (double)a.width;
                        const double y1 = (double)row[mpn_anchor::kOffBox + 2] * (double)a.height;
                        const double x1 = (double)row[mpn_anchor::kOffBox + 3] * (double)a.width;
                        if (mpn_anchor::finite64(x0) && mpn_anchor::finite64(x1) && mpn_anchor::finite64(y0) && mpn_anchor::finite64(y1))
                            cells = make_int4(first_centre_at_or_behind(x0, a.cell, gw), first_centre_at_or_behind(x1, a.cell, gw),
                                              first_centre_at_or_behind(y0, a.cell, a.gh), first_centre_at_or_behind(y1, a.cell, a.gh));
                        if (cells.y <= cells.x || cells.w <= cells.z) cells = make_int4(0, 0, 0, 0);
                    }
                    if (a.track_rows) id = *(const int*)(a.track_rows + (size_t)(first + lane) * kTrackRowBytes);
                    if (id < 0) id = 0;
                }
            }
            rtid[lane] = id;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");    // (one wave: LDS operations stay in program order)
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

            // phase C: lane = slot. The values that decide are the same in every lane (ballots, the butterfly's minimum).
            int slot_id = (int)slots[lane * kSlotWords + kSlotId];
            int slot_last = (int)slots[lane * kSlotWords + kSlotLast];
            bool slot_taken = false;
            int my_slot = -1;                                     // lane = row again: the slot row `lane` took
            bool my_fresh = false;
            for (int r = 0; r < n; ++r) {
                const int rid = rtid[r];
                if (rid <= 0) continue;                           // (uniform)
                const unsigned long long match = __ballot(slot_id == rid);
                int t;
                bool fresh = false;
                if (match != 0ull) {
                    t = __ffsll(match) - 1;
                    if ((__ballot(slot_taken) >> t) & 1ull) continue;     // an earlier row of the frame has this id: untracked
                } else {
                    long long key = slot_taken ? 0x7fffffffffffffffll : (((long long)slot_last << 6) | lane);
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const long long other = __shfl_xor(key, o, 64);
                        key = other < key ? other : key;
                    }
                    t = (int)(key & 63);                          // 64 slots, at most 64 rows: one is always free
                    fresh = true;
                }
                if (lane == t) {
                    slot_taken = true;
                    if (fresh) { slot_id = rid; slot_last = 0; }
                }
                if (lane == r) { my_slot = t; my_fresh = fresh; }
            }

            // phase D: lane = row; the rows' slots are distinct
            bool visits_here = false;
            if (lane < n && my_slot >= 0) {
                unsigned* slot = slots + my_slot * kSlotWords;
                if (my_fresh) { slot[kSlotId] = (unsigned)id; slot[kSlotCell] = 0u; slot[3] = 0u; }
                flags |= kFlagTracked;
                if (k >= 0) {
                    visits_here = slot[kSlotCell] != (unsigned)(k + 1);
                    slot[kSlotCell] = (unsigned)(k + 1);
                } else {
                    slot[kSlotCell] = 0u;
                }
                slot[kSlotLast] = (unsigned)now;
            }
            if (visits_here) flags |= kFlagVisit;
            const unsigned ncells = (unsigned)((cells.y - cells.x) * (cells.w - cells.z));
            rect[lane] = cells;
            visit[lane] = visits_here ? k : -1;
            if (lane < n) {
                uint4* o = reinterpret_cast<uint4*>(a.out + (size_t)(first + lane) * kOutRowWords);
                *o = make_uint4((unsigned)row_cell, (unsigned)col_cell, flags, ncells);
            }
            const unsigned long long counted = __ballot(ncells > 0u), visited = __ballot(visits_here);
            if (lane == 0) { frame_counts[0] = (unsigned)__popcll(counted); frame_counts[1] = (unsigned)__popcll(visited); }
        }
        __syncthreads();

        // the pass over the planes: cell i is thread i % kThreads' in every frame
        const bool halve = a.half_life > 0 && now % a.half_life == 0;
        const unsigned* src = f == 0 ? pst + kOffPlanes : nst + kOffPlanes;
        unsigned* dst = nst + kOffPlanes;
        unsigned* snap = a.snapshots ? a.snapshots + (size_t)b * G : nullptr;
        unsigned most_dwell = 0u, most_visits = 0u;               // over the cells this frame added to
        // kChunk cells a step: their loads are in flight together (a frame reads what the frame before stored, so each step is a
        // round trip to memory), and a row's rectangle is read from LDS once for all of them
        for (int i0 = tid; i0 < G; i0 += kChunk * kThreads) {
            unsigned d[kChunk], v[kChunk], nd[kChunk], nv[kChunk];
            int r[kChunk], c[kChunk];
#pragma unroll
            for (int j = 0; j < kChunk; ++j) {
                const int i = i0 + j * kThreads;
                const bool live = i < G;
                d[j] = live ? src[i] : 0u; v[j] = live ? src[G + i] : 0u;
                r[j] = i / gw; c[j] = i - r[j] * gw;              // (a cell behind G lies below every rectangle)
                nd[j] = 0u; nv[j] = 0u;
            }
            for (int p = 0; p < n; ++p) {
                const int4 q = rect[p];
                const int at = visit[p];                          // < G or -1
#pragma unroll
                for (int j = 0; j < kChunk; ++j) {
                    nd[j] += (c[j] >= q.x && c[j] < q.y && r[j] >= q.z && r[j] < q.w) ? 1u : 0u;
                    nv[j] += at == i0 + j * kThreads ? 1u : 0u;
                }
            }
#pragma unroll
            for (int j = 0; j < kChunk; ++j) {
                const int i = i0 + j * kThreads;
                if (i < G) {
                    const unsigned dj = sat_add(halve ? d[j] >> 1 : d[j], nd[j]), vj = sat_add(halve ? v[j] >> 1 : v[j], nv[j]);
                    if (nd[j] && dj > most_dwell) most_dwell = dj;
                    if (nv[j] && vj > most_visits) most_visits = vj;
                    dst[i] = dj; dst[G + i] = vj;
                    if (snap) snap[i] = a.show ? vj : dj;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned od = (unsigned)__shfl_xor((int)most_dwell, o, 64), ov = (unsigned)__shfl_xor((int)most_visits, o, 64);
            most_dwell = od > most_dwell ? od : most_dwell;
            most_visits = ov > most_visits ? ov : most_visits;
        }
        if (lane == 0) { part[0][wave] = most_dwell; part[1][wave] = most_visits; }
        __syncthreads();
        if (tid < 2) {
            unsigned m = halve ? maxima[tid] >> 1 : maxima[tid];
#pragma unroll
            for (int w = 0; w < kWaves; ++w) m = part[tid][w] > m ? part[tid][w] : m;
            maxima[tid] = m;
        }
        __syncthreads();                                          // the maxima, and the rows' staging is free for the next frame
        if (tid == 0) {
            uint4* o = reinterpret_cast<uint4*>(a.out + (size_t)all_rows * kOutRowWords + (size_t)b * kImageRowWords);
            *o = make_uint4(maxima[0], maxima[1], frame_counts[0], frame_counts[1]);
        }
    }

    __syncthreads();
    for (int i = tid; i < kOffPlanes; i += kThreads)
        nst[i] = i == 0 ? (unsigned)(frames_before + F) : (i < 3 ? maxima[i - 1] : (i < kHeaderWords ? 0u : slots[i - kHeaderWords]));
}

// ---------------------------------------------------------------------------------------------------------------- the picture
constexpr int kTabFlags = 0, kTabFullScale = 1, kTabHeaderWords = 8, kTabWords = kTabHeaderWords + 256;
constexpr int kTabBytes = kTabWords * 4;
static_assert(kTabBytes == MPN_DRAW_DENSITY_TABLE_BYTES, "the table's layout is part of the ABI");
constexpr int kFlagSmooth = 1, kFlagShowVisits = 2;
constexpr int kRasterBlocks = 2048;     // blocks per image of the raster kernel at most (grid-stride over the groups of 4 pixels)

typedef mpn_draw_desc Desc;

__device__ __forceinline__ bool out_desc_ok(const Desc& d, size_t out_bytes) {
    if (d.h < 1 || d.w < 1 || d.h > 65536 || d.w > 65536) return false;
    const unsigned long long npix = (unsigned long long)d.h * (unsigned long long)d.w;
    if (npix > (1ull << 29)) return false;
    if (d.out_offset < 0 || (d.out_offset & 15)) return false;
    return (unsigned long long)d.out_offset + ((npix * 4 + 15) / 16 * 16) <= out_bytes;
}

// BLEND8 of include/mpn.h per colour channel: t = m * ink + (255 - m) * under + 128; ((t >> 8) + t) >> 8. Alpha is 255.
__device__ __forceinline__ unsigned blend8(unsigned m, unsigned under, unsigned ink) {
    unsigned res = 0xFF000000u;
#pragma unroll
    for (int s = 0; s < 24; s += 8) {
        const unsigned t = m * ((ink >> s) & 255u) + (255u - m) * ((under >> s) & 255u) + 128u;
        res |= (((t >> 8) + t) >> 8) << s;
    }
    return res;
}

// M of image b: the table's full_scale, or the image row's maximum of the shown plane
__device__ __forceinline__ unsigned scale_of(const unsigned* __restrict__ tables, const unsigned* __restrict__ image_rows, int b) {
    const unsigned full = tables[kTabFullScale];
    if (full) return full;
    return image_rows[(size_t)b * kImageRowWords + ((tables[kTabFlags] & kFlagShowVisits) ? 1 : 0)];
}

__global__ void __launch_bounds__(kThreads) density_levels_kernel(const unsigned* __restrict__ snapshots,
                                                                  const unsigned* __restrict__ image_rows,
                                                                  const unsigned* __restrict__ tables, int B, int G,
                                                                  uint8_t* __restrict__ levels) {
    const int t = blockIdx.x * kThreads + threadIdx.x;            // B * G <= 65535 * 16384 < 2^31
    if (t >= B * G) return;
    const unsigned long long M = scale_of(tables, image_rows, t / G);
    unsigned long long level = 0ull;
    if (M) {
        level = (255ull * snapshots[t] + M / 2) / M;
        level = level > 255ull ? 255ull : level;
    }
    levels[t] = (uint8_t)level;
}

// v of 0..n*s-1 along an axis of n cells of s pixels -> the two cells it lies between (i0 <= i1, clamped) and its weight f of
// 2s towards i1. Without smooth: the cell it lies in, f = 0.
__device__ __forceinline__ void between(int v, int s, int n, bool smooth, int& i0, int& i1, int& f) {
    if (!smooth) { i0 = i1 = min(v / s, n - 1); f = 0; return; }
    const int u = 2 * v + 1 - s;                                  // > -2s
    const int q = (u + 2 * s) / (2 * s) - 1;                      // floor(u / 2s)
    f = u - q * 2 * s;
    i0 = min(max(q, 0), n - 1); i1 = min(max(q + 1, 0), n - 1);
}

__global__ void __launch_bounds__(kThreads) density_raster_kernel(const Desc* __restrict__ descs,
                                                                  const unsigned* __restrict__ image_rows,
                                                                  const unsigned* __restrict__ tables,
                                                                  const uint8_t* __restrict__ levels, int height, int width, int cell,
                                                                  int gh, int gw, uint8_t* out, size_t out_bytes) {
    __shared__ unsigned ink[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const Desc d = descs[b];
    if (!out_desc_ok(d, out_bytes) || d.h != height || d.w != width) return;       // (uniform)
    if (scale_of(tables, image_rows, b) == 0u) return;                              // nothing was counted: no wash
    ink[tid] = tables[kTabHeaderWords + tid];                                       // kThreads == 256
    __syncthreads();
    const bool smooth = (tables[kTabFlags] & kFlagSmooth) != 0;
    const uint8_t* lv = levels + (size_t)b * gh * gw;
    const int s2 = 2 * cell, round_up = 2 * cell * cell, shift_to = 4 * cell * cell;
    const int npix = height * width;                                               // <= 2^26
    const int groups = (npix + 3) >> 2;
    uint4* dst = reinterpret_cast<uint4*>(out + d.out_offset);
    for (int g = blockIdx.x * kThreads + tid; g < groups; g += gridDim.x * kThreads) {
        const int p0 = g * 4;
        int y = p0 / width, x = p0 - y * width;
        int r0, r1, fy, c0, c1, fx;
        between(y, cell, gh, smooth, r0, r1, fy);
        uint4 px = dst[g];                                                          // (the frame's bytes are padded to 16)
        unsigned* pv = reinterpret_cast<unsigned*>(&px);
        bool changed = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (p0 + i < npix) {
                between(x, cell, gw, smooth, c0, c1, fx);
                const int l00 = lv[r0 * gw + c0], l01 = lv[r0 * gw + c1], l10 = lv[r1 * gw + c0], l11 = lv[r1 * gw + c1];
                const int level = (l00 * (s2 - fx) * (s2 - fy) + l01 * fx * (s2 - fy) + l10 * (s2 - fx) * fy + l11 * fx * fy + round_up) /
                                  shift_to;
                const unsigned entry = ink[min(max(level, 0), 255)];
                const unsigned m = entry >> 24;
                if (m) { pv[i] = blend8(m, pv[i], entry); changed = true; }
                if (++x == width) {
                    x = 0; ++y;
                    if (y < height) between(y, cell, gh, smooth, r0, r1, fy);
                }
            }
        }
        if (changed) dst[g] = px;
    }
}

inline bool grid_ok(int height, int width, int cell) {
    return cell >= kMinCell && cell <= kMaxCell && height >= 1 && height <= kMaxSide && width >= 1 && width <= kMaxSide &&
           (long long)cells_of(height, cell) * cells_of(width, cell) <= kMaxCells;
}

}  // namespace

extern "C" size_t mpn_density_state_bytes(int streams, int gh, int gw) {
    if (streams < 1 || streams > kMaxRows || gh < 1 || gw < 1 || gh > kMaxCells || gw > kMaxCells || (long long)gh * gw > kMaxCells)
        return 0;
    return (size_t)streams * ((size_t)kOffPlanes * 4 + 8 * (size_t)gh * gw);
}

extern "C" size_t mpn_density_out_bytes(int B, int max_boxes) {
    if (B < 1 || max_boxes < 1 || max_boxes > kMaxBoxes || (long long)B * max_boxes > kMaxRows) return 0;
    return (size_t)B * max_boxes * kOutRowWords * 4 + (size_t)B * kImageRowWords * 4;
}

extern "C" size_t mpn_density_snapshot_bytes(int B, int gh, int gw) {
    if (B < 1 || B > kMaxRows || gh < 1 || gw < 1 || gh > kMaxCells || gw > kMaxCells || (long long)gh * gw > kMaxCells) return 0;
    return (size_t)B * gh * gw * 4;
}

extern "C" int mpn_density_map(const void* record, const void* track_rows, int B, int max_boxes, int streams, int height, int width,
                               int cell, int footprint, int anchor, double min_keypoint_score, int with_keypoints, int half_life,
                               int show, const void* prev, void* next, void* out, void* snapshots, mpn_stream_t stream) {
    MPN_REQUIRE(record && prev && next && out, MPN_ERR_BAD_ARG, "density_map: null pointer");
    MPN_REQUIRE(prev != next, MPN_ERR_BAD_ARG,
                "density_map: prev and next are one buffer; the launch is a pure function of (record, track_rows, prev)");
    MPN_REQUIRE(cell >= kMinCell && cell <= kMaxCell, MPN_ERR_BAD_ARG, "density_map: cell must be in %d..%d (got %d)", kMinCell,
                kMaxCell, cell);
    MPN_REQUIRE(height >= 1 && height <= kMaxSide && width >= 1 && width <= kMaxSide, MPN_ERR_BAD_ARG,
                "density_map: height and width must be in 1..%d (got %d, %d)", kMaxSide, height, width);
    MPN_REQUIRE(grid_ok(height, width, cell), MPN_ERR_BAD_ARG, "density_map: a grid of %d x %d cells, at most %d in all",
                cells_of(height, cell), cells_of(width, cell), kMaxCells);
    MPN_REQUIRE(footprint == 0 || footprint == 1, MPN_ERR_BAD_ARG, "density_map: footprint must be 0 (anchor) or 1 (box) (got %d)",
                footprint);
    MPN_REQUIRE(half_life >= 0 && half_life <= kMaxHalfLife, MPN_ERR_BAD_ARG, "density_map: half_life must be in 0..%d (got %d)",
                kMaxHalfLife, half_life);
    MPN_REQUIRE(show == 0 || (show == 1 && track_rows), MPN_ERR_BAD_ARG,
                "density_map: show must be 0 (dwell) or, with track_rows, 1 (visits) (got %d)", show);
    MPN_REQUIRE(min_keypoint_score - min_keypoint_score == 0.0, MPN_ERR_BAD_ARG,
                "density_map: min_keypoint_score must be finite (got %g)", min_keypoint_score);
    MPN_REQUIRE(streams >= 1 && B >= 1 && B % streams == 0, MPN_ERR_BAD_SHAPE,
                "density_map: B = %d images are not streams = %d times a whole number of frames", B, streams);
    MPN_REQUIRE(max_boxes >= 1 && max_boxes <= kMaxBoxes && (long long)B * max_boxes <= kMaxRows, MPN_ERR_BAD_SHAPE,
                "density_map: B = %d, max_boxes = %d (at most %d per image, %d rows)", B, max_boxes, kMaxBoxes, kMaxRows);
    MPN_REQUIRE(mpn_aligned16(record) && mpn_aligned16(out) &&
                    (((uintptr_t)track_rows | (uintptr_t)prev | (uintptr_t)next | (uintptr_t)snapshots) & 7u) == 0,
                MPN_ERR_BAD_ALIGN, "density_map: record and out must be 16-byte, track_rows / prev / next / snapshots 8-byte aligned");
    DensityArgs a = {(const int*)record, (const float*)((const char*)record + header_words(B) * 4), (const unsigned char*)track_rows,
                     (const unsigned*)prev, (unsigned*)next, (unsigned*)out, (unsigned*)snapshots, B, max_boxes, streams, height,
                     width, cell, cells_of(height, cell), cells_of(width, cell), footprint,
                     (anchor == 0 && !with_keypoints) ? 1 : anchor, half_life, show, min_keypoint_score};
    density_map_kernel<<<streams, kThreads, 0, (hipStream_t)stream>>>(a);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}

extern "C" size_t mpn_draw_density_tables_bytes(void) { return kTabBytes; }

extern "C" size_t mpn_draw_density_workspace_bytes(int B, int gh, int gw) {
    if (B < 1 || B > 65535 || gh < 1 || gw < 1 || gh > kMaxCells || gw > kMaxCells || (long long)gh * gw > kMaxCells) return 0;
    return ((size_t)B * gh * gw + 15) / 16 * 16;
}

extern "C" int mpn_draw_density(const void* descs, const void* snapshots, const void* rows, const void* tables, size_t tables_bytes,
                                int B, int max_boxes, int height, int width, int cell, uint8_t* out_rgba, size_t out_bytes,
                                void* workspace, size_t workspace_bytes, mpn_stream_t stream) {
    MPN_REQUIRE(descs && snapshots && rows && tables && out_rgba && workspace, MPN_ERR_BAD_ARG, "draw_density: null pointer");
    MPN_REQUIRE(B >= 1 && B <= 65535, MPN_ERR_BAD_SHAPE, "draw_density: B must be in [1, 65535] (got %d)", B);
    MPN_REQUIRE(max_boxes >= 1 && max_boxes <= kMaxBoxes && (long long)B * max_boxes <= kMaxRows, MPN_ERR_BAD_SHAPE,
                "draw_density: B = %d, max_boxes = %d (at most %d per image, %d rows)", B, max_boxes, kMaxBoxes, kMaxRows);
    MPN_REQUIRE(grid_ok(height, width, cell), MPN_ERR_BAD_SHAPE,
                "draw_density: height, width in 1..%d, cell in %d..%d and at most %d cells (got %d, %d, %d)", kMaxSide, kMinCell,
                kMaxCell, kMaxCells, height, width, cell);
    MPN_REQUIRE(mpn_aligned16(descs) && mpn_aligned16(rows) && mpn_aligned16(out_rgba) && mpn_aligned16(workspace), MPN_ERR_BAD_ALIGN,
                "draw_density: descs, rows, out_rgba and workspace must be 16-byte aligned");
    MPN_REQUIRE((((uintptr_t)snapshots | (uintptr_t)tables) & 3u) == 0, MPN_ERR_BAD_ALIGN,
                "draw_density: snapshots and tables must be 4-byte aligned");
    const int gh = cells_of(height, cell), gw = cells_of(width, cell);
    MPN_REQUIRE(workspace_bytes >= mpn_draw_density_workspace_bytes(B, gh, gw), MPN_ERR_WORKSPACE,
                "draw_density: workspace of %zu bytes, %zu needed", workspace_bytes, mpn_draw_density_workspace_bytes(B, gh, gw));
    MPN_REQUIRE(out_bytes >= 16, MPN_ERR_WORKSPACE, "draw_density: out_rgba of %zu bytes", out_bytes);
    MPN_REQUIRE(tables_bytes >= (size_t)kTabBytes, MPN_ERR_WORKSPACE, "draw_density: tables of %zu bytes, %d needed", tables_bytes,
                kTabBytes);
    const unsigned* image_rows = reinterpret_cast<const unsigned*>(rows) + (size_t)B * max_boxes * kOutRowWords;
    const int G = gh * gw;
    density_levels_kernel<<<mpn_div_up((long long)B * G, kThreads), kThreads, 0, (hipStream_t)stream>>>(
        reinterpret_cast<const unsigned*>(snapshots), image_rows, reinterpret_cast<const unsigned*>(tables), B, G,
        reinterpret_cast<uint8_t*>(workspace));
    MPN_LAUNCH_CHECK();
    const int groups = (height * width + 3) / 4;
    const int blocks = mpn_div_up(groups, kThreads) < kRasterBlocks ? mpn_div_up(groups, kThreads) : kRasterBlocks;
    density_raster_kernel<<<dim3((unsigned)blocks, (unsigned)B), kThreads, 0, (hipStream_t)stream>>>(
        reinterpret_cast<const Desc*>(descs), image_rows, reinterpret_cast<const unsigned*>(tables),
        reinterpret_cast<const uint8_t*>(workspace), height, width, cell, gh, gw, out_rgba, out_bytes);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
