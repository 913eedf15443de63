// Motion trails: where each tracked person has been, kept per identity in device state, and drawn into the annotated frames.
//   mpn_track_trails   record + track rows (read in place) + prev state -> next state + a row of up to K + 1 points per record
//                      row. PURE like mpn_zone_events: prev is never written; the caller advances the state by copying next over
//                      prev. ONE block per stream; the block walks its F frames in order with the stream's state - 64 slots keyed
//                      by track id, each a ring of K anchors - in LDS (34.8 KB at K = 64). Per frame:
//                        phase A  wave 0, lane = record row: the row's anchor (mpn_zone_events' rule, then one rounding to f32),
//                                 flags and track id -> LDS
//                        phase C  wave 0, lane = slot: the rows take their slots, serially in row order, word for word as in
//                                 zone_events.hip (a ballot for the match, a wave minimum for the eviction)
//                        phase D  wave 0, lane = record row: restart, append, the row's points newest first
//                      Latency-bound glue, microseconds behind a network pass of milliseconds: not tuned beyond that.
//   mpn_draw_trails    the trail rows -> polylines blended IN PLACE into the RGBA frames mpn_draw_detections / mpn_draw_tracks
//                      wrote. Two launches:
//                        trails_build_kernel   one thread per (record row, segment): the segment's integer end points, bounding
//                                              box, ink and alpha (48 bytes); the thread of segment 0 also writes the trail's
//                                              entry: the bounding box of all its points, its ink and its segment count
//                        trails_raster_kernel  shaped like draw.hip's raster: an image as a flat array of pixels, 4 per thread, a
//                                              block's tile 1024 pixels, a wave's part 256. Per tile the image's trails are binned
//                                              by bounding box against each wave's run into a bit mask in LDS. A wave then walks
//                                              its trails in record order; per trail lane s tests segment s's box against the
//                                              wave's run (K <= 64: one ballot) and the wave walks the surviving segments from
//                                              the oldest to the newest. A pixel is read when its first segment covers it,
//                                              blended once per covering segment in draw order, and written once: one thread
//                                              owns it, so overlapping segments cannot race. Untouched pixels are neither read
//                                              nor written.
//                      The Bresenham membership test is draw.hip's `line` rule, restated here on the same closed form.
#include "common.h"
#include "person_anchor.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxRows = 4096;          // mpn_pose_gather's own limit on B * max_boxes
constexpr int kSlots = 64;              // always, as in mpn_zone_events: one lane of wave 0 per slot
constexpr int kMaxLength = 64;          // K: ring entries per slot; one lane per segment in the raster
constexpr int kTrailMaxBoxes = 64;      // mpn_track_trails: one lane of wave 0 per record row
constexpr int kRowWords = 108, kTrackRowBytes = 24, kTrackRowWords = 6;
// the state of one stream, in 32-bit words: {frames, 0, 0, 0}, then 64 slots of 8 + 2K words
constexpr int kStateHeaderWords = 4, kSlotHeaderWords = 8;
constexpr int kSlotId = 0, kSlotLast = 1, kSlotLastAppend = 2, kSlotCount = 3, kSlotHead = 4;
constexpr int slot_words(int K) { return kSlotHeaderWords + 2 * K; }
constexpr int stream_words(int K) { return kStateHeaderWords + kSlots * slot_words(K); }
constexpr unsigned kFlagTracked = 1u, kFlagNoAnchor = mpn_anchor::kFlagNoAnchor, kFlagAppended = 8u, kFlagRestarted = 16u;
constexpr int trail_row_words(int K) { return 2 * (K + 2); }

inline size_t header_words(int B) { return ((size_t)(2 * B + 2) + 3) / 4 * 4; }

struct TrailArgs {
    const int* header;
    const float* rows;
    const unsigned char* track_rows;
    const unsigned* prev;
    unsigned* next;
    unsigned* out;
    int B, max_boxes, streams, K, every, max_gap, anchor_mode;
    double min_score, height, width;
};

__device__ __forceinline__ bool finite32(float v) { return v - v == 0.0f; }

__global__ __launch_bounds__(kThreads) void track_trails_kernel(TrailArgs a) {
    __shared__ unsigned st[stream_words(kMaxLength)];             // the stream's state
    __shared__ int rtid[kTrailMaxBoxes];                          // the track id of a row that can take a slot, else 0
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, F = a.B / a.streams;
    const int kSlotW = slot_words(K), kStreamW = stream_words(K), kRowW = trail_row_words(K);
    const int all_rows = a.B * a.max_boxes;
    const unsigned* pst = a.prev + (size_t)s * kStreamW;
    unsigned* nst = a.next + (size_t)s * kStreamW;
    for (int i = tid; i < kStreamW; i += kThreads) st[i] = pst[i];

    // the record's counts, clamped as mpn_zone_events clamps them: nothing is indexed out of range
    int total = a.header[0];
    total = total < 0 ? 0 : (total > all_rows ? all_rows : total);
    // rows behind the record's total are zero: the blocks share them
    for (long long w = (long long)total * kRowW + s * kThreads + tid; w < (long long)all_rows * kRowW;
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
        if (wave == 0) {
            const int b = s * F + f;
            const int now = frames_before + f + 1;
            int n = a.header[1 + b];
            int first = ahead;
            ahead += n > 0 ? n : 0;
            if (ahead > all_rows) ahead = all_rows;
            n = n < 0 ? 0 : (n > a.max_boxes ? a.max_boxes : n);
            if (first > total) first = total;
            if (first + n > total) n = total - first;

            // phase A: lane = row
            unsigned flags = 0u;
            float fx = 0.0f, fy = 0.0f;
            int id = 0;
            if (lane < n) {
                double cx, cy;
                flags = mpn_anchor::person_anchor(a.rows + (size_t)(first + lane) * kRowWords, a.anchor_mode, a.min_score, a.height,
                                                  a.width, cx, cy);
                fx = (float)cx; fy = (float)cy;                   // the one rounding to f32
                if ((flags & kFlagNoAnchor) || !finite32(fx) || !finite32(fy)) { flags = kFlagNoAnchor; fx = 0.0f; fy = 0.0f; }
                id = *(const int*)(a.track_rows + (size_t)(first + lane) * kTrackRowBytes);
                if (id < 0 || (flags & kFlagNoAnchor)) id = 0;
            }
            rtid[lane] = id;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");    // (one wave: LDS operations stay in program order)
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

            // phase C: lane = slot. The values that decide are the same in every lane (ballots, the butterfly's minimum).
            int slot_id = (int)st[kStateHeaderWords + lane * kSlotW + kSlotId];
            int slot_last = (int)st[kStateHeaderWords + lane * kSlotW + kSlotLast];
            bool slot_taken = false;
            int my_slot = -1;                                     // lane = row again: the slot row `lane` took
            bool my_fresh = false;
            for (int r = 0; r < n; ++r) {
                const int rid = rtid[r];
                if (rid <= 0) continue;                           // (uniform)
                const unsigned long long match = __ballot(slot_id == rid);
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
                    if (fresh) { slot_id = rid; slot_last = 0; }
                }
                if (lane == r) { my_slot = k; my_fresh = fresh; }
            }

            // phase D: lane = row; the rows' slots are distinct
            if (lane < n) {
                unsigned* o = a.out + (size_t)(first + lane) * kRowW;
                int np = 0;                                       // points written
                if (!(flags & kFlagNoAnchor)) {
                    const unsigned ux = __float_as_uint(fx), uy = __float_as_uint(fy);
                    if (my_slot >= 0) {
                        unsigned* slot = st + kStateHeaderWords + my_slot * kSlotW;
                        unsigned* ring = slot + kSlotHeaderWords;
                        if (my_fresh) {
                            for (int w = 0; w < kSlotW; ++w) slot[w] = 0u;
                            slot[kSlotId] = (unsigned)id;
                        }
                        flags |= kFlagTracked;
                        int last = (int)slot[kSlotLast], last_append = (int)slot[kSlotLastAppend];
                        int count = (int)slot[kSlotCount], head = (int)slot[kSlotHead];
                        // a state that is not one this kernel wrote indexes nothing out of range
                        count = count < 0 ? 0 : (count > K ? K : count);
                        head = head < 0 ? 0 : (head >= K ? K - 1 : head);
                        if (count > 0 && a.max_gap > 0 && now - last > a.max_gap) {
                            for (int w = 1; w < kSlotW; ++w) slot[w] = 0u;
                            last_append = 0; count = 0; head = 0;
                            flags |= kFlagRestarted;
                        }
                        const bool append = count == 0 || now - last_append >= a.every;
                        if (append) {
                            head = count == 0 ? 0 : (head + 1) % K;
                            ring[2 * head] = ux; ring[2 * head + 1] = uy;
                            count = count + 1 < K ? count + 1 : K;
                            last_append = now;
                            flags |= kFlagAppended;
                        } else {
                            o[2] = ux; o[3] = uy;
                            np = 1;
                        }
                        slot[kSlotLast] = (unsigned)now; slot[kSlotLastAppend] = (unsigned)last_append;
                        slot[kSlotCount] = (unsigned)count; slot[kSlotHead] = (unsigned)head;
                        for (int i = 0; i < count; ++i, ++np) {
                            const int e = (head - i + K) % K;
                            o[2 + 2 * np] = ring[2 * e]; o[3 + 2 * np] = ring[2 * e + 1];
                        }
                    } else {
                        o[2] = ux; o[3] = uy;
                        np = 1;
                    }
                }
                o[0] = (unsigned)np; o[1] = flags;
                for (int w = 2 + 2 * np; w < kRowW; ++w) o[w] = 0u;
            }
        }
        __syncthreads();                                          // the slots' words are in LDS before the next frame reads them
    }

    for (int i = tid; i < kStreamW; i += kThreads)
        nst[i] = i == 0 ? (unsigned)(frames_before + F) : (i < kStateHeaderWords ? 0u : st[i]);
}

// ---------------------------------------------------------------------------------------------------------------- the picture
constexpr int kDrawMaxBoxes = MPN_DRAW_MAX_BOXES;
constexpr int kTileBlocks = 1024;       // blocks per image of the raster kernel (grid-stride over the image's tiles)
constexpr int kCoordMax = 1 << 29;
constexpr int kMaxPalette = MPN_DRAW_TRACKS_MAX_PALETTE;
// the table in 32-bit words
constexpr int kTabFlags = 0, kTabMinAlpha = 1, kTabLength = 2, kTabPalette = 3, kTabColours = 4;
constexpr int kTabHeaderBytes = kTabColours * 4;
static_assert(kTabHeaderBytes == MPN_DRAW_TRAILS_TABLE_HEADER_BYTES, "the table's layout is part of the ABI");
constexpr int kFlagFade = 1;
constexpr int kTrailMaskWords = kDrawMaxBoxes / 32;

typedef mpn_draw_desc Desc;

struct Seg {
    int bx0, by0, bx1, by1;             // bounding box, inclusive; bx1 < bx0: nothing to draw
    int x0, y0, x1, y1;                 // from the older point to the newer one
    unsigned ink, alpha, pad0, pad1;
};
static_assert(sizeof(Seg) == 48, "three 16-byte vectors");
struct Trail {
    int bx0, by0, bx1, by1;             // the bounding box of all its points; bx1 < bx0: nothing to draw
    unsigned ink;
    int segments;
    int pad0, pad1;
};
static_assert(sizeof(Trail) == 32, "two 16-byte vectors");

__device__ __forceinline__ bool out_desc_ok(const Desc& d, size_t out_bytes) {
    if (d.h < 1 || d.w < 1 || d.h > 65536 || d.w > 65536) return false;
    const unsigned long long npix = (unsigned long long)d.h * (unsigned long long)d.w;
    if (npix > (1ull << 29)) return false;                                          // pixels are indexed in 32 bits
    if (d.out_offset < 0 || (d.out_offset & 15)) return false;
    return (unsigned long long)d.out_offset + ((npix * 4 + 15) / 16 * 16) <= out_bytes;
}

// C's (int) of a float, toward zero; clamped (a NaN becomes the lower bound)
__device__ __forceinline__ int trunc_int(float v) { return (int)fmin(fmax((double)v, -(double)kCoordMax), (double)kCoordMax); }

// is pixel (x, y), which lies inside the segment's bounding box, on the line from (c.x, c.y) to (c.z, c.w)? mpn_draw_detections'
// `line`: at step i of the major axis the minor axis has moved floor((2*m*i + n) / (2*n)) steps
__device__ __forceinline__ bool on_line(const int4& c, int x, int y) {
    const int dx = abs(c.z - c.x), dy = abs(c.w - c.y);
    const int xs = c.z >= c.x ? 1 : -1, ys = c.w >= c.y ? 1 : -1;
    if (dx > dy) {
        const long long i = (long long)(x - c.x) * xs;
        return y == c.y + ys * (int)((2LL * dy * i + dx) / (2LL * dx));
    }
    if (dy == 0) return true;
    const long long i = (long long)(y - c.y) * ys;
    return x == c.x + xs * (int)((2LL * dx * i + dy) / (2LL * dy));
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

__global__ void __launch_bounds__(kThreads) trails_build_kernel(const int* __restrict__ header, const int* __restrict__ track_rows,
                                                                const unsigned* __restrict__ trail_rows,
                                                                const int* __restrict__ tables, size_t tables_bytes, int B,
                                                                int max_boxes, int K, Seg* __restrict__ segs,
                                                                Trail* __restrict__ trails) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    const int rows = B * max_boxes;
    if (t >= rows * K) return;
    const int j = t / K, s = t - j * K;
    if (j >= min(max(header[0], 0), rows)) return;      // rows behind `total` are never read by the raster kernel
    const unsigned* row = trail_rows + (size_t)j * trail_row_words(K);
    const int n = min(max((int)row[0], 0), K + 1);
    const int id = track_rows[(size_t)j * kTrackRowWords];
    const int P = tables[kTabPalette];
    const bool drawn = (row[1] & kFlagTracked) && n >= 2 && id > 0 && P >= 1 && P <= kMaxPalette &&
                       (size_t)kTabHeaderBytes + (size_t)P * 4 <= tables_bytes;
    const unsigned ink = drawn ? ((unsigned)tables[kTabColours + (id - 1) % P] & 0xFFFFFFu) : 0u;
    const float* pts = reinterpret_cast<const float*>(row + 2);
    Seg g = {1, 1, 0, 0, 0, 0, 0, 0, ink, 255u, 0u, 0u};
    if (drawn && s < n - 1) {
        g.x0 = trunc_int(pts[2 * (s + 1)]); g.y0 = trunc_int(pts[2 * (s + 1) + 1]);
        g.x1 = trunc_int(pts[2 * s]); g.y1 = trunc_int(pts[2 * s + 1]);
        g.bx0 = min(g.x0, g.x1); g.bx1 = max(g.x0, g.x1); g.by0 = min(g.y0, g.y1); g.by1 = max(g.y0, g.y1);
        if (tables[kTabFlags] & kFlagFade) {
            const int min_alpha = min(max(tables[kTabMinAlpha], 0), 255);
            const int length = min(max(tables[kTabLength], 1), kMaxLength);
            const int alpha = 255 - (s * (255 - min_alpha)) / max(length - 1, 1);
            g.alpha = (unsigned)min(max(alpha, 0), 255);
        }
    }
    uint4* dst = reinterpret_cast<uint4*>(segs + t);
    dst[0] = make_uint4((unsigned)g.bx0, (unsigned)g.by0, (unsigned)g.bx1, (unsigned)g.by1);
    dst[1] = make_uint4((unsigned)g.x0, (unsigned)g.y0, (unsigned)g.x1, (unsigned)g.y1);
    dst[2] = make_uint4(g.ink, g.alpha, 0u, 0u);
    if (s == 0) {
        Trail tr = {1, 1, 0, 0, ink, 0, 0, 0};
        if (drawn) {
            tr.bx0 = tr.by0 = kCoordMax; tr.bx1 = tr.by1 = -kCoordMax;
            for (int i = 0; i < n; ++i) {
                const int x = trunc_int(pts[2 * i]), y = trunc_int(pts[2 * i + 1]);
                tr.bx0 = min(tr.bx0, x); tr.bx1 = max(tr.bx1, x); tr.by0 = min(tr.by0, y); tr.by1 = max(tr.by1, y);
            }
            tr.segments = n - 1;
        }
        uint4* td = reinterpret_cast<uint4*>(trails + j);
        td[0] = make_uint4((unsigned)tr.bx0, (unsigned)tr.by0, (unsigned)tr.bx1, (unsigned)tr.by1);
        td[1] = make_uint4(tr.ink, (unsigned)tr.segments, 0u, 0u);
    }
}

__global__ void __launch_bounds__(kThreads) trails_raster_kernel(const Desc* __restrict__ descs, const int* __restrict__ header,
                                                                 int B, int max_boxes, int K, const Seg* __restrict__ segs,
                                                                 const Trail* __restrict__ trails, uint8_t* out, size_t out_bytes) {
    __shared__ unsigned mask[kWaves][kTrailMaskWords];
    __shared__ int run[kWaves][4];          // a wave's pixels as a box: xa, ya, xb, yb (xb < xa: none)
    __shared__ int person_range[2];
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const Desc d = descs[b];
    if (!out_desc_ok(d, out_bytes)) return;
    if (tid == 0) {
        // this image's rows of the record: counts are clamped so that no index leaves the workspace
        const int cap = B * max_boxes, total = min(max(header[0], 0), cap);
        int first = 0;
        for (int i = 0; i < b; ++i) first += min(max(header[1 + i], 0), max_boxes);
        first = min(first, total);
        person_range[0] = first;
        person_range[1] = min(min(max(header[1 + b], 0), max_boxes), total - first);
    }
    __syncthreads();
    const int first = person_range[0], ntrails = person_range[1];
    if (ntrails == 0) return;               // (uniform)
    const Trail* mine = trails + first;
    const int w = d.w;
    const int npix = d.h * d.w;             // <= 2^29 (out_desc_ok)
    const int groups = (npix + 3) >> 2, tiles = (groups + kThreads - 1) / kThreads;
    unsigned* dst = reinterpret_cast<unsigned*>(out + d.out_offset);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {      // (uniform per block: every thread reaches the barriers)
        __syncthreads();                    // the previous tile's masks have been read
        if (tid < kWaves * kTrailMaskWords) mask[tid / kTrailMaskWords][tid % kTrailMaskWords] = 0u;
        if (tid < kWaves) {
            const int p0 = (tile * kThreads + tid * 64) * 4, p1 = min(p0 + 256, npix) - 1;
            int xa = 1, ya = 0, xb = 0, yb = 0;
            if (p0 <= p1) {
                ya = p0 / w; yb = p1 / w;
                xa = ya == yb ? p0 - ya * w : 0;
                xb = ya == yb ? p1 - yb * w : w - 1;
            }
            run[tid][0] = xa; run[tid][1] = ya; run[tid][2] = xb; run[tid][3] = yb;
        }
        __syncthreads();
        if (tid < ntrails) {                // ntrails <= max_boxes <= 128
            const int4 bb = *reinterpret_cast<const int4*>(mine + tid);
            if (bb.z >= bb.x) {
#pragma unroll
                for (int v = 0; v < kWaves; ++v) {
                    if (bb.x <= run[v][2] && bb.z >= run[v][0] && bb.y <= run[v][3] && bb.w >= run[v][1])
                        atomicOr(&mask[v][tid >> 5], 1u << (tid & 31));
                }
            }
        }
        __syncthreads();
        const int rxa = run[wave][0], rya = run[wave][1], rxb = run[wave][2], ryb = run[wave][3];
        const int g = tile * kThreads + tid;
        const int p0 = g * 4;
        const int count = g < groups ? min(4, npix - p0) : 0;       // (a lane without pixels stays for the ballots)
        int xs[4], ys[4];
        {
            int y = p0 / w, x = p0 - y * w;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                xs[i] = x; ys[i] = y;
                if (++x == w) { x = 0; ++y; }
            }
        }
        unsigned px[4] = {0u, 0u, 0u, 0u};
        unsigned have = 0u;                 // pixels read, blended and to be written
        for (int wd = 0; wd < kTrailMaskWords; ++wd) {
            unsigned m = mask[wave][wd];    // (uniform in the wave)
            while (m) {
                const int bit = __ffs(m) - 1;
                m &= m - 1u;
                const int p = wd * 32 + bit;                        // < ntrails
                const int4 tb = *reinterpret_cast<const int4*>(mine + p);
                const uint4 tv = *(reinterpret_cast<const uint4*>(mine + p) + 1);
                const int nseg = min((int)tv.y, K);
                const Seg* sg = segs + (size_t)(first + p) * K;
                // lane s: does segment s's box meet the wave's run?
                bool meets = false;
                if (lane < nseg) {
                    const int4 sb = *reinterpret_cast<const int4*>(sg + lane);
                    meets = sb.z >= sb.x && sb.x <= rxb && sb.z >= rxa && sb.y <= ryb && sb.w >= rya;
                }
                unsigned long long live = __ballot(meets);
                // the thread's pixels lie in rows ys[0]..ys[3], mostly one row: reject on the trail's box first
                const bool mine_too = count > 0 && !(tb.y > ys[3] || tb.w < ys[0] || (ys[0] == ys[3] && (tb.x > xs[3] || tb.z < xs[0])));
                if (!mine_too) live = 0ull;  // (nothing below crosses lanes)
                while (live) {              // from the oldest segment, the highest s, to the newest
                    const int s = 63 - __clzll(live);
                    live &= ~(1ull << s);
                    const int4 sb = *reinterpret_cast<const int4*>(sg + s);
                    if (sb.y > ys[3] || sb.w < ys[0] || (ys[0] == ys[3] && (sb.x > xs[3] || sb.z < xs[0]))) continue;
                    const int4 c = *(reinterpret_cast<const int4*>(sg + s) + 1);
                    const uint4 ia = *(reinterpret_cast<const uint4*>(sg + s) + 2);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (!(i < count && xs[i] >= sb.x && xs[i] <= sb.z && ys[i] >= sb.y && ys[i] <= sb.w)) continue;
                        if (!on_line(c, xs[i], ys[i])) continue;
                        if (!((have >> i) & 1u)) { px[i] = dst[p0 + i]; have |= 1u << i; }
                        px[i] = blend8(ia.y, px[i], ia.x);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if ((have >> i) & 1u) dst[p0 + i] = px[i];
    }
}

inline bool trails_shape_ok(int B, int max_boxes, int length, int most_boxes) {
    return B >= 1 && max_boxes >= 1 && max_boxes <= most_boxes && (long long)B * max_boxes <= kMaxRows && length >= 1 &&
           length <= kMaxLength;
}

inline size_t draw_workspace_bytes(int B, int max_boxes, int length) {
    if (!trails_shape_ok(B, max_boxes, length, kDrawMaxBoxes)) return 0;
    const size_t rows = (size_t)B * max_boxes;
    return rows * length * sizeof(Seg) + rows * sizeof(Trail);
}

}  // namespace

extern "C" size_t mpn_track_trails_state_bytes(int streams, int length) {
    if (streams < 1 || streams > kMaxRows || length < 1 || length > kMaxLength) return 0;
    return (size_t)streams * stream_words(length) * 4;
}

extern "C" size_t mpn_track_trails_out_bytes(int B, int max_boxes, int length) {
    if (!trails_shape_ok(B, max_boxes, length, kTrailMaxBoxes)) return 0;
    return (size_t)B * max_boxes * trail_row_words(length) * 4;
}

extern "C" int mpn_track_trails(const void* record, const void* track_rows, int B, int max_boxes, int streams, int length,
                                int every, int max_gap, int anchor, double min_keypoint_score, double height, double width,
                                int with_keypoints, const void* prev, void* next, void* out, mpn_stream_t stream) {
    MPN_REQUIRE(record && track_rows && prev && next && out, MPN_ERR_BAD_ARG, "track_trails: null pointer");
    MPN_REQUIRE(prev != next, MPN_ERR_BAD_ARG,
                "track_trails: prev and next are one buffer; the launch is a pure function of (record, track_rows, prev)");
    MPN_REQUIRE(length >= 1 && length <= kMaxLength, MPN_ERR_BAD_ARG, "track_trails: length must be in 1..%d (got %d)", kMaxLength,
                length);
    MPN_REQUIRE(every >= 1 && every <= 255, MPN_ERR_BAD_ARG, "track_trails: every must be in 1..255 (got %d)", every);
    MPN_REQUIRE(max_gap >= 0 && max_gap <= 65535, MPN_ERR_BAD_ARG, "track_trails: max_gap must be in 0..65535 (got %d)", max_gap);
    MPN_REQUIRE(height - height == 0.0 && width - width == 0.0 && min_keypoint_score - min_keypoint_score == 0.0, MPN_ERR_BAD_ARG,
                "track_trails: height, width and min_keypoint_score must be finite (got %g, %g, %g)", height, width,
                min_keypoint_score);
    MPN_REQUIRE(streams >= 1 && B >= 1 && B % streams == 0, MPN_ERR_BAD_SHAPE,
                "track_trails: B = %d images are not streams = %d times a whole number of frames", B, streams);
    MPN_REQUIRE(max_boxes >= 1 && max_boxes <= kTrailMaxBoxes && (long long)B * max_boxes <= kMaxRows, MPN_ERR_BAD_SHAPE,
                "track_trails: B = %d, max_boxes = %d (at most %d per image, %d rows)", B, max_boxes, kTrailMaxBoxes, kMaxRows);
    MPN_REQUIRE(mpn_aligned16(record) && (((uintptr_t)track_rows | (uintptr_t)prev | (uintptr_t)next | (uintptr_t)out) & 7u) == 0,
                MPN_ERR_BAD_ALIGN, "track_trails: record must be 16-byte, track_rows / prev / next / out 8-byte aligned");
    TrailArgs a = {(const int*)record, (const float*)((const char*)record + header_words(B) * 4), (const unsigned char*)track_rows,
                   (const unsigned*)prev, (unsigned*)next, (unsigned*)out, B, max_boxes, streams, length, every, max_gap,
                   (anchor == 0 && !with_keypoints) ? 1 : anchor, min_keypoint_score, height, width};
    track_trails_kernel<<<streams, kThreads, 0, (hipStream_t)stream>>>(a);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}

extern "C" size_t mpn_draw_trails_tables_bytes(int palette_size) {
    if (palette_size < 1 || palette_size > kMaxPalette) return 0;
    return ((size_t)kTabHeaderBytes + (size_t)palette_size * 4 + 15) / 16 * 16;
}

extern "C" size_t mpn_draw_trails_workspace_bytes(int B, int max_boxes, int length) {
    return draw_workspace_bytes(B, max_boxes, length);
}

extern "C" int mpn_draw_trails(const void* descs, const void* record, size_t record_bytes, const void* track_rows,
                               const void* trail_rows, const void* tables, size_t tables_bytes, int B, int max_boxes, int length,
                               uint8_t* out_rgba, size_t out_bytes, void* workspace, size_t workspace_bytes, mpn_stream_t stream) {
    MPN_REQUIRE(descs && record && track_rows && trail_rows && tables && out_rgba && workspace, MPN_ERR_BAD_ARG,
                "draw_trails: null pointer");
    MPN_REQUIRE(B >= 1 && B <= 65535, MPN_ERR_BAD_SHAPE, "draw_trails: B must be in [1, 65535] (got %d)", B);
    MPN_REQUIRE(max_boxes >= 1 && max_boxes <= kDrawMaxBoxes, MPN_ERR_BAD_SHAPE, "draw_trails: max_boxes must be in [1, %d] (got %d)",
                kDrawMaxBoxes, max_boxes);
    MPN_REQUIRE((long long)B * max_boxes <= kMaxRows, MPN_ERR_BAD_SHAPE,
                "draw_trails: B * max_boxes = %lld rows, mpn_pose_gather's record holds %d", (long long)B * max_boxes, kMaxRows);
    MPN_REQUIRE(length >= 1 && length <= kMaxLength, MPN_ERR_BAD_SHAPE, "draw_trails: length must be in [1, %d] (got %d)", kMaxLength,
                length);
    MPN_REQUIRE(mpn_aligned16(descs) && mpn_aligned16(record) && mpn_aligned16(out_rgba) && mpn_aligned16(workspace),
                MPN_ERR_BAD_ALIGN, "draw_trails: descs, record, out_rgba and workspace must be 16-byte aligned");
    MPN_REQUIRE((((uintptr_t)track_rows | (uintptr_t)trail_rows | (uintptr_t)tables) & 3u) == 0, MPN_ERR_BAD_ALIGN,
                "draw_trails: track_rows, trail_rows and tables must be 4-byte aligned");
    MPN_REQUIRE(mpn_pose_gather_row_offset(B, max_boxes, 0) == header_words(B) * 4, MPN_ERR_BAD_ARG,
                "draw_trails: the record's layout is not the one this kernel was written against");
    MPN_REQUIRE(record_bytes >= mpn_pose_gather_record_bytes(B, max_boxes), MPN_ERR_WORKSPACE,
                "draw_trails: record of %zu bytes, %zu needed", record_bytes, mpn_pose_gather_record_bytes(B, max_boxes));
    MPN_REQUIRE(workspace_bytes >= draw_workspace_bytes(B, max_boxes, length), MPN_ERR_WORKSPACE,
                "draw_trails: workspace of %zu bytes, %zu needed", workspace_bytes, draw_workspace_bytes(B, max_boxes, length));
    MPN_REQUIRE(out_bytes >= 16, MPN_ERR_WORKSPACE, "draw_trails: out_rgba of %zu bytes", out_bytes);
    MPN_REQUIRE(tables_bytes >= (size_t)kTabHeaderBytes, MPN_ERR_WORKSPACE, "draw_trails: tables of %zu bytes, the header alone is %d",
                tables_bytes, kTabHeaderBytes);
    const size_t rows = (size_t)B * max_boxes;
    Seg* segs = reinterpret_cast<Seg*>(workspace);
    Trail* trails = reinterpret_cast<Trail*>(segs + rows * length);
    trails_build_kernel<<<mpn_div_up((long long)rows * length, kThreads), kThreads, 0, (hipStream_t)stream>>>(
        reinterpret_cast<const int*>(record), reinterpret_cast<const int*>(track_rows), reinterpret_cast<const unsigned*>(trail_rows),
        reinterpret_cast<const int*>(tables), tables_bytes, B, max_boxes, length, segs, trails);
    MPN_LAUNCH_CHECK();
    trails_raster_kernel<<<dim3(kTileBlocks, (unsigned)B), kThreads, 0, (hipStream_t)stream>>>(
        reinterpret_cast<const Desc*>(descs), reinterpret_cast<const int*>(record), B, max_boxes, length, segs, trails, out_rgba,
        out_bytes);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
