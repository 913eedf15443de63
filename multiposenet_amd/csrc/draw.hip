// `draw_everything` of the reference's inference/predict.ipynb (cells 10 and 12) for a batch of RAGGED frames, on the device:
// out = the source frame as RGBA (alpha 255) with, per kept person of mpn_pose_gather's record in record order, the box outline
// (red), the 16 skeleton lines (white, one pixel) and the 17 keypoint dots (red), each an opaque overwrite, clipped per pixel -
// byte for byte what Pillow draws for the notebook (tests/draw_ref.py restates it, tests/test_draw_host.py proves the
// restatement against Pillow).
//
//   draw_prims_kernel    one thread per (record row, primitive): the notebook's mixed float64 / float32 coordinate arithmetic
//                        from the row's box and keypoint_positions, Pillow's truncation toward zero -> workspace: the
//                        primitive's integer bounding box and its integer corners / end points (32 bytes).
//   draw_raster_kernel   a GATHER: every pixel's colour is the LAST primitive in draw order that covers it, else the source.
//                        Nothing scatters, so overlapping primitives cannot race and the output is a function of the inputs.
//
// The raster kernel walks an image as a FLAT array of pixels, 4 pixels per thread: 12 source bytes in (three dword loads;
// the packed sources have no alignment), one aligned 16-byte store out - whatever the width, odd ones included. A block's tile
// is 1024 consecutive pixels, a wave's part 256 of them: mostly a run inside one row. Per tile the image's primitives (at most
// max_boxes * 34) are binned by bounding box against each WAVE's run into a bit mask in LDS (atomic OR: order-free); a thread
// then walks its wave's mask from the highest bit down and tests its pixels with closed forms:
//   rectangle  on the border of [x0,x1] x [y0,y1]   (+ Pillow's two pixels below a box whose rows coincide)
//   line       Bresenham from the first point, end point included: at step i of the major axis the minor axis has moved
//              floor((2*m*i + n) / (2*n))   (n = max(|dx|,|dy|), m = min)
//   dot        a row bit table per (x1-x0, y1-y0) in {3,4}^2 (MPN_DRAW_DOT_STAMPS, the ellipse Pillow draws at "radius" 2)
// Most waves find an empty mask and copy. Grids depend on (B, max_boxes) alone: sizes, offsets and persons reach the kernels
// through device memory, so a captured graph serves any later batch that fits its buffers. No descriptor makes a kernel read
// outside `sources` or write outside `out`: desc_ok() rejects it and the image is left unwritten.
//
// mpn_draw_tracks is the same two launches (the kernels are templates, kTracks) for persons with identities: a person's inks
// come from its row of mpn_pose_track's output and the style table instead of the two constants, its keypoints optionally from
// mpn_pose_smooth's rows, and a 35th primitive per person is the id label: a filled rectangle whose pixels under a digit's
// stamp are BLEND8(mask, identity colour, text colour). The prims kernel resolves each person's inks once into a 16-byte
// entry behind the primitives (the raster kernel reads it only for a pixel a primitive covers: nothing is added to the
// "empty mask -> copy" path) and validates everything of the table a label needs; the raster kernel checks the one byte index
// it derives from the table against tables_bytes again. A table that fails a check leaves the primitive undrawn.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTileBlocks = 1024;       // blocks per image of the raster kernel (grid-stride over the image's tiles)
constexpr int kK = 17;
constexpr int kEdges = 16;
constexpr int kPrims = 1 + kEdges + kK; // per person, in draw order: box, lines, dots
constexpr int kMaxBoxes = MPN_DRAW_MAX_BOXES;
constexpr int kMaxRows = 4096;          // mpn_pose_gather's one-block limit
constexpr int kLabel = kPrims;          // mpn_draw_tracks: the id label, a person's last primitive
constexpr int kPrimsT = kPrims + 1;
constexpr int prims_per_person(bool tracks) { return tracks ? kPrimsT : kPrims; }
constexpr int mask_words(bool tracks) { return (kMaxBoxes * prims_per_person(tracks) + 31) / 32; }
constexpr int kTrackRowWords = 6, kSmoothRowWords = 85;         // rows of mpn_pose_track's and mpn_pose_smooth's output
// the style table of mpn_draw_tracks in 32-bit words (include/mpn.h)
constexpr int kTabFlags = 0, kTabLine = 1, kTabText = 2, kTabPalette = 3, kTabCell = 4, kTabTop = 5, kTabBot = 6;
constexpr int kTabStamps = 8, kStampWords = 5, kTabColours = kTabStamps + 10 * kStampWords;
constexpr int kTabHeaderBytes = kTabColours * 4;
static_assert(kTabHeaderBytes == MPN_DRAW_TRACKS_TABLE_HEADER_BYTES, "the table's layout is part of the ABI");
constexpr int kMaxPalette = MPN_DRAW_TRACKS_MAX_PALETTE, kMaxCell = MPN_DRAW_TRACKS_MAX_CELL;
constexpr int kMaxStampH = MPN_DRAW_TRACKS_MAX_STAMP_H, kLabelPad = 1, kMaxDigits = 10;
constexpr int kFlagLabels = 1, kFlagHide = 2;
constexpr int kRowWords = 108, kOffBox = 1, kOffKPos = 23;      // a row of mpn_pose_gather's record, in 32-bit words
constexpr int kCoordMax = 1 << 29;      // coordinates are clamped here: differences stay inside int32
constexpr unsigned kRed = 0xFF0000FFu, kWhite = 0xFFFFFFFFu, kAlpha = 0xFF000000u;

typedef mpn_draw_desc Desc;
static_assert(sizeof(Desc) == MPN_DRAW_DESC_BYTES, "descriptor layout is part of the ABI");

// the skeleton of the notebook (cell 10), sorted: every line of a person is white and they follow each other, so the order
// among them does not show; the direction of a line does (the tie rule)
__device__ const unsigned char kEdgeFrom[kEdges] = {0, 0, 1, 2, 3, 4, 5, 5, 6, 6, 7, 8, 11, 12, 13, 14};
__device__ const unsigned char kEdgeTo[kEdges] = {1, 2, 3, 4, 5, 6, 7, 11, 8, 12, 9, 10, 13, 14, 15, 16};

const unsigned char kStampsHost[4][5] = MPN_DRAW_DOT_STAMPS;
__device__ const unsigned char kStamps[4][5] = MPN_DRAW_DOT_STAMPS;

struct Prim {
    int bx0, by0, bx1, by1;     // bounding box, inclusive; bx1 < bx0: nothing to draw
    int x0, y0, x1, y1;
};
static_assert(sizeof(Prim) == 32, "two 16-byte vectors");

// what mpn_draw_tracks adds to the kernels' arguments; the plain launch passes an empty NoTracks
struct Tracks {
    const int* track_rows;          // [B * max_boxes][6] words: track_id first
    const float* smooth_rows;       // [B * max_boxes][85] floats: keypoints (x, y, score) first; null: the frame's own
    const int* tables;              // the style table
    size_t tables_bytes;
    uint4* persons;                 // workspace behind the primitives, one entry per record row: Person
};
struct NoTracks {};

// a person's inks, resolved once by the prims kernel
struct Person {
    unsigned ink;                   // box, dots and label: red, or the identity colour
    unsigned line_ink;
    int track_id;                   // > 0: tracked
    int digits;                     // decimal digits of track_id
};
static_assert(sizeof(Person) == sizeof(uint4), "one 16-byte vector");

__device__ const int kPow10[kMaxDigits] = {1, 10, 100, 1000, 10000, 100000, 1000000, 10000000, 100000000, 1000000000};

inline size_t round16(size_t n) { return (n + 15) / 16 * 16; }
inline size_t record_header_words(int B) { return ((size_t)(2 * B + 2) + 3) / 4 * 4; }

__device__ __forceinline__ bool desc_ok(const Desc& d, size_t sources_bytes, size_t out_bytes) {
    if (d.h < 1 || d.w < 1 || d.h > 65536 || d.w > 65536) return false;
    const unsigned long long npix = (unsigned long long)d.h * (unsigned long long)d.w;
    if (npix > (1ull << 29)) return false;                                          // pixels are indexed in 32 bits
    if (d.src_offset < 0 || d.out_offset < 0 || (d.out_offset & 15)) return false;
    if ((unsigned long long)d.src_offset + npix * 3 > sources_bytes) return false;
    return (unsigned long long)d.out_offset + ((npix * 4 + 15) / 16 * 16) <= out_bytes;
}

// C's (int) of a double, toward zero; clamped (a NaN becomes the lower bound)
__device__ __forceinline__ int trunc_int(double v) { return (int)fmin(fmax(v, -(double)kCoordMax), (double)kCoordMax); }

// the inks of record row j from its track row and the table; false: the person is not drawn (untracked and hidden, or a
// palette that does not lie inside the table)
__device__ __forceinline__ bool person_of(const Tracks& tr, int j, Person& who) {
    const int id = tr.track_rows[(size_t)j * kTrackRowWords];
    who = {kRed, kWhite, 0, 0};
    if (id <= 0) return !(tr.tables[kTabFlags] & kFlagHide);
    const int P = tr.tables[kTabPalette];
    if (P < 1 || P > kMaxPalette || (size_t)kTabHeaderBytes + (size_t)P * 4 > tr.tables_bytes) return false;
    who.ink = (unsigned)tr.tables[kTabColours + (id - 1) % P] | kAlpha;
    who.line_ink = (unsigned)tr.tables[kTabLine] | kAlpha;
    who.track_id = id;
    who.digits = 1;
    while (who.digits < kMaxDigits && id >= kPow10[who.digits]) ++who.digits;
    return true;
}

// the label of a tracked person whose box has the corner (x0, y0): its rectangle, or false when the table's sizes or the
// stamp of one of the id's digits fail a check (every stamp at most the padding outside its cell, so that the rectangle
// encloses it and it reaches into the neighbouring cells only; the cell inside the table's limits; the stamp's bytes inside
// the table) - the raster kernel then never sees the label
__device__ __forceinline__ bool label_of(const Tracks& tr, const Person& who, int x0, int y0, Prim& p) {
    const int* tab = tr.tables;
    const int cell = tab[kTabCell], top = tab[kTabTop], bot = tab[kTabBot];
    if (cell < 1 || cell > kMaxCell || top < -kMaxStampH || top > kMaxStampH || bot < top || bot - top > kMaxStampH) return false;
    for (int i = 0; i < who.digits; ++i) {
        const int* s = tab + kTabStamps + (who.track_id / kPow10[i]) % 10 * kStampWords;    // w, h, ox, oy, byte offset
        if (s[0] < 0 || s[1] < 0 || s[2] < -kLabelPad || s[0] > cell + kLabelPad - s[2] || s[3] < top || s[1] > bot - s[3])
            return false;
        if (s[4] < kTabHeaderBytes || (size_t)s[4] + (size_t)(s[0] * s[1]) > tr.tables_bytes) return false;
    }
    const int lw = 2 * kLabelPad + who.digits * cell, lh = 2 * kLabelPad + (bot - top);
    p.x0 = x0; p.y0 = y0 - lh >= 0 ? y0 - lh : y0;      // above the box, or inside it at the top of the frame
    p.x1 = p.x0 + lw - 1; p.y1 = p.y0 + lh - 1;
    p.bx0 = p.x0; p.by0 = p.y0; p.bx1 = p.x1; p.by1 = p.y1;
    return true;
}

template <bool kTracks, typename TrackArgs>
__global__ void __launch_bounds__(kThreads) draw_prims_kernel(const Desc* __restrict__ descs, const int* __restrict__ header,
                                                              const float* __restrict__ rows, int B, int max_boxes,
                                                              int with_keypoints, Prim* __restrict__ prims, const TrackArgs tr) {
    constexpr int kPer = prims_per_person(kTracks);
    const int t = blockIdx.x * kThreads + threadIdx.x;
    const int n = B * max_boxes;
    if (t >= n * kPer) return;
    const int j = t / kPer, k = t - j * kPer;
    if (j >= min(max(header[0], 0), n)) return;         // rows behind `total` are never read by the raster kernel
    const float* row = rows + (size_t)j * kRowWords;
    Prim p = {1, 1, 0, 0, 0, 0, 0, 0};
    const int img = __float_as_int(row[0]);
    bool drawn = img >= 0 && img < B && (k == 0 || (kTracks && k == kLabel) || with_keypoints);
    Person who = {kRed, kWhite, 0, 0};
    const float* smooth = nullptr;
    if constexpr (kTracks) {
        drawn = person_of(tr, j, who) && drawn;
        if (k == 0) tr.persons[j] = make_uint4(who.ink, who.line_ink, (unsigned)who.track_id, (unsigned)who.digits);
        if (k == kLabel) drawn = drawn && who.track_id > 0 && (tr.tables[kTabFlags] & kFlagLabels);
        if (tr.smooth_rows) smooth = tr.smooth_rows + (size_t)j * kSmoothRowWords;
    }
    if (drawn) {
        const Desc d = descs[img];
        // scaler * boxes: int64 * float32 -> float64
        const double ymin = (double)d.h * (double)row[kOffBox], xmin = (double)d.w * (double)row[kOffBox + 1];
        const double ymax = (double)d.h * (double)row[kOffBox + 2], xmax = (double)d.w * (double)row[kOffBox + 3];
        if (k == 0 || (kTracks && k == kLabel)) {
            p.x0 = trunc_int(xmin); p.y0 = trunc_int(ymin); p.x1 = trunc_int(xmax); p.y1 = trunc_int(ymax);
            p.bx0 = p.x0; p.by0 = p.y0; p.bx1 = p.x1;
            p.by1 = p.y1 == p.y0 ? p.y0 + 1 : p.y1;
            if (p.y1 < p.y0) p.bx1 = p.bx0 - 1;         // (Pillow refuses such a box)
            if constexpr (kTracks) {
                if (k == kLabel) {                      // only a box that is drawn has a label
                    const bool box = p.bx1 >= p.bx0;
                    const int x0 = p.x0, y0 = p.y0;
                    p = {1, 1, 0, 0, 0, 0, 0, 0};
                    if (box) label_of(tr, who, x0, y0, p);
                }
            }
        } else {
            const float* pos = row + kOffKPos;          // (y, x) normalised to the box
            // keypoints *= [xmax - xmin, ymax - ymin]; keypoints += [xmin, ymin]: float64 results rounded to float32;
            // or the smoothed (x, y) as they are
            auto kx = [&](int q) {
                return smooth ? smooth[3 * q] : (float)((double)(float)((double)pos[2 * q + 1] * (xmax - xmin)) + xmin);
            };
            auto ky = [&](int q) {
                return smooth ? smooth[3 * q + 1] : (float)((double)(float)((double)pos[2 * q] * (ymax - ymin)) + ymin);
            };
            if (k <= kEdges) {
                const int a = kEdgeFrom[k - 1], b = kEdgeTo[k - 1];
                p.x0 = trunc_int(kx(a)); p.y0 = trunc_int(ky(a)); p.x1 = trunc_int(kx(b)); p.y1 = trunc_int(ky(b));
                p.bx0 = min(p.x0, p.x1); p.bx1 = max(p.x0, p.x1); p.by0 = min(p.y0, p.y1); p.by1 = max(p.y0, p.y1);
            } else {
                const float x = kx(k - 1 - kEdges), y = ky(k - 1 - kEdges);
                p.x0 = trunc_int(x - 2.0f); p.y0 = trunc_int(y - 2.0f); p.x1 = trunc_int(x + 2.0f); p.y1 = trunc_int(y + 2.0f);
                const int dw = p.x1 - p.x0, dh = p.y1 - p.y0;
                // another difference needs |x| beyond 2^22, where float32 no longer resolves x +- 2: outside any frame
                if (dw >= 3 && dw <= 4 && dh >= 3 && dh <= 4) { p.bx0 = p.x0; p.by0 = p.y0; p.bx1 = p.x1; p.by1 = p.y1; }
            }
        }
    }
    uint4* dst = reinterpret_cast<uint4*>(prims + t);
    dst[0] = make_uint4((unsigned)p.bx0, (unsigned)p.by0, (unsigned)p.bx1, (unsigned)p.by1);
    dst[1] = make_uint4((unsigned)p.x0, (unsigned)p.y0, (unsigned)p.x1, (unsigned)p.y1);
}

// is pixel (x, y), which lies inside the primitive's bounding box, drawn by primitive `kind` (index within its person)?
__device__ __forceinline__ bool covers(int kind, const int4& c, int x, int y) {
    if (kind == 0) return x == c.x || x == c.z || y == c.y || y == c.w;
    if (kind <= kEdges) {
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
    return (kStamps[(c.z - c.x - 3) * 2 + (c.w - c.y - 3)][y - c.y] >> (x - c.x)) & 1;
}

// BLEND8 of Pillow per colour channel: t = m * text + (255 - m) * under + 128; ((t >> 8) + t) >> 8. Alpha stays 255.
__device__ __forceinline__ unsigned blend8(unsigned m, unsigned under, unsigned text) {
    unsigned res = kAlpha;
#pragma unroll
    for (int s = 0; s < 24; s += 8) {
        const unsigned t = m * ((text >> s) & 255u) + (255u - m) * ((under >> s) & 255u) + 128u;
        res |= (((t >> 8) + t) >> 8) << s;
    }
    return res;
}

// the colour of pixel (x, y) of a label whose rectangle starts at (lx0, ly0): the identity colour, with the text colour
// blended over it under the stamp of every digit that holds the pixel, from the left as Pillow draws them - the digit whose
// cell holds x and, where a glyph is wider than its advance, a neighbour. Every index is checked again here: whatever the
// table holds, a byte that is read lies inside it.
__device__ __forceinline__ unsigned label_ink(const Tracks& tr, const Person& who, int lx0, int ly0, int x, int y) {
    const int* tab = tr.tables;
    const int cell = tab[kTabCell];
    const int rx = x - lx0 - kLabelPad;     // >= -pad
    if (cell < 1) return who.ink;
    const int at = rx < 0 ? -1 : rx / cell; // digit cells from the left
    const long long ry = (long long)(y - ly0 - kLabelPad) + tab[kTabTop];          // the text sits at ly0 + pad - top
    unsigned colour = who.ink;
    for (int k = max(at - 1, 0); k <= min(at + 1, who.digits - 1); ++k) {
        const int* s = tab + kTabStamps + (who.track_id / kPow10[who.digits - 1 - k]) % 10 * kStampWords;
        const long long sx = (long long)rx - (long long)k * cell - s[2], sy = ry - s[3];
        if (sx < 0 || sx >= s[0] || sy < 0 || sy >= s[1] || s[4] < kTabHeaderBytes) continue;
        const unsigned long long at_byte = (unsigned long long)s[4] + (unsigned long long)sy * (unsigned)s[0] + (unsigned long long)sx;
        if (at_byte >= tr.tables_bytes) continue;
        colour = blend8(reinterpret_cast<const uint8_t*>(tab)[at_byte], colour, (unsigned)tab[kTabText]);
    }
    return colour;
}

template <bool kTracks, typename TrackArgs>
__global__ void __launch_bounds__(kThreads) draw_raster_kernel(const uint8_t* __restrict__ sources, size_t sources_bytes,
                                                               const Desc* __restrict__ descs, const int* __restrict__ header,
                                                               int B, int max_boxes, const Prim* __restrict__ prims,
                                                               uint8_t* __restrict__ out, size_t out_bytes, const TrackArgs tr) {
    constexpr int kPer = prims_per_person(kTracks);
    __shared__ unsigned mask[kWaves][mask_words(kTracks)];
    __shared__ int run[kWaves][4];          // a wave's pixels as a box: xa, ya, xb, yb (xb < xa: none)
    __shared__ int person_range[2];
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
    const Desc d = descs[b];
    if (!desc_ok(d, sources_bytes, out_bytes)) return;
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
    const Prim* mine = prims + (size_t)person_range[0] * kPer;
    const int nprims = person_range[1] * kPer, words = (nprims + 31) >> 5;
    const int w = d.w;
    const int npix = d.h * d.w;             // <= 2^29 (desc_ok)
    const int groups = (npix + 3) >> 2, tiles = (groups + kThreads - 1) / kThreads;
    const uint8_t* img = sources + d.src_offset;
    uint4* dst = reinterpret_cast<uint4*>(out + d.out_offset);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {      // (uniform per block: every thread reaches the barriers)
        __syncthreads();                    // the previous tile's masks have been read
        for (int i = tid; i < kWaves * words; i += kThreads) mask[i / words][i % words] = 0u;
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
        for (int p = tid; p < nprims; p += kThreads) {
            const int4 bb = *reinterpret_cast<const int4*>(mine + p);
            if (bb.z < bb.x) continue;
#pragma unroll
            for (int v = 0; v < kWaves; ++v) {
                if (bb.x <= run[v][2] && bb.z >= run[v][0] && bb.y <= run[v][3] && bb.w >= run[v][1])
                    atomicOr(&mask[v][p >> 5], 1u << (p & 31));
            }
        }
        __syncthreads();
        const int g = tile * kThreads + tid;
        if (g >= groups) continue;
        const int p0 = g * 4;
        const int count = min(4, npix - p0);
        unsigned px[4] = {0u, 0u, 0u, 0u};
        const uint8_t* q = img + (size_t)p0 * 3;
        if (count == 4) {                   // 12 bytes inside the image
            unsigned u[3];
            __builtin_memcpy(u, q, 12);
            px[0] = u[0] & 0xFFFFFFu;
            px[1] = (u[0] >> 24) | ((u[1] & 0xFFFFu) << 8);
            px[2] = (u[1] >> 16) | ((u[2] & 0xFFu) << 16);
            px[3] = u[2] >> 8;
        } else {
            for (int i = 0; i < count; ++i) px[i] = (unsigned)q[3 * i] | ((unsigned)q[3 * i + 1] << 8) | ((unsigned)q[3 * i + 2] << 16);
        }
        int xs[4], ys[4];
        int y = p0 / w, x = p0 - y * w;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            xs[i] = x; ys[i] = y;
            px[i] = i < count ? (px[i] | kAlpha) : 0u;
            if (++x == w) { x = 0; ++y; }
        }
        unsigned open = (1u << count) - 1u;     // pixels no primitive has claimed yet
        for (int wd = words - 1; wd >= 0 && open; --wd) {
            unsigned m = mask[wave][wd];
            while (m && open) {
                const int bit = 31 - __clz(m);
                m &= ~(1u << bit);
                const int p = wd * 32 + bit;
                const int4 bb = *reinterpret_cast<const int4*>(mine + p);
                // the thread's pixels lie in rows ys[0]..ys[3], mostly one row: reject on the primitive's box first
                if (bb.y > ys[3] || bb.w < ys[0] || (ys[0] == ys[3] && (bb.x > xs[3] || bb.z < xs[0]))) continue;
                const int4 c = *(reinterpret_cast<const int4*>(mine + p) + 1);
                const int kind = p % kPer;
                unsigned ink = (kind >= 1 && kind <= kEdges) ? kWhite : kRed;
                [[maybe_unused]] Person who = {kRed, kWhite, 0, 0};
                // the inks of the primitive's person, read beside the primitive's second half whether or not a pixel turns out
                // to be covered: reading them only behind a hit put a dependent load into the pixel loop and measured slower
                if constexpr (kTracks) {
                    const uint4 v = tr.persons[person_range[0] + p / kPer];
                    who = {v.x, v.y, (int)v.z, (int)v.w};
                    ink = (kind >= 1 && kind <= kEdges) ? who.line_ink : who.ink;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (!(((open >> i) & 1u) && xs[i] >= bb.x && xs[i] <= bb.z && ys[i] >= bb.y && ys[i] <= bb.w)) continue;
                    if constexpr (kTracks) {
                        if (kind == kLabel) {           // filled: every pixel of the rectangle
                            px[i] = label_ink(tr, who, c.x, c.y, xs[i], ys[i]);
                            open &= ~(1u << i);
                            continue;
                        }
                    }
                    if (covers(kind, c, xs[i], ys[i])) {
                        px[i] = ink;
                        open &= ~(1u << i);
                    }
                }
            }
        }
        dst[g] = make_uint4(px[0], px[1], px[2], px[3]);
    }
}

inline size_t workspace_bytes_for(int B, int max_boxes, bool tracks) {
    if (B < 1 || max_boxes < 1 || max_boxes > kMaxBoxes || (long long)B * max_boxes > kMaxRows) return 0;
    const size_t rows = (size_t)B * max_boxes;
    return rows * prims_per_person(tracks) * sizeof(Prim) + (tracks ? rows * sizeof(Person) : 0);
}

// the argument checks both entry points share (`who` names the entry point in the message), before any HIP call
int check_draw(const char* who, const void* sources, size_t sources_bytes, const void* descs, const void* record,
               size_t record_bytes, int B, int max_boxes, const void* out_rgba, size_t out_bytes, const void* workspace,
               size_t workspace_bytes, bool tracks) {
    MPN_REQUIRE(sources && descs && record && out_rgba && workspace, MPN_ERR_BAD_ARG, "%s: null pointer", who);
    MPN_REQUIRE(B >= 1 && B <= 65535, MPN_ERR_BAD_SHAPE, "%s: B must be in [1, 65535] (got %d)", who, B);
    MPN_REQUIRE(max_boxes >= 1 && max_boxes <= kMaxBoxes, MPN_ERR_BAD_SHAPE, "%s: max_boxes must be in [1, %d] (got %d)", who,
                kMaxBoxes, max_boxes);
    MPN_REQUIRE((long long)B * max_boxes <= kMaxRows, MPN_ERR_BAD_SHAPE,
                "%s: B * max_boxes = %lld rows, mpn_pose_gather's record holds %d", who, (long long)B * max_boxes, kMaxRows);
    MPN_REQUIRE(mpn_aligned16(descs) && mpn_aligned16(record) && mpn_aligned16(out_rgba) && mpn_aligned16(workspace),
                MPN_ERR_BAD_ALIGN, "%s: descs, record, out_rgba and workspace must be 16-byte aligned", who);
    MPN_REQUIRE(mpn_pose_gather_row_offset(B, max_boxes, 0) == record_header_words(B) * 4 &&
                    mpn_pose_gather_row_offset(B, max_boxes, 1) - mpn_pose_gather_row_offset(B, max_boxes, 0) == kRowWords * 4,
                MPN_ERR_BAD_ARG, "%s: the record's layout is not the one this kernel was written against", who);
    MPN_REQUIRE(record_bytes >= mpn_pose_gather_record_bytes(B, max_boxes), MPN_ERR_WORKSPACE,
                "%s: record of %zu bytes, %zu needed", who, record_bytes, mpn_pose_gather_record_bytes(B, max_boxes));
    MPN_REQUIRE(workspace_bytes >= workspace_bytes_for(B, max_boxes, tracks), MPN_ERR_WORKSPACE,
                "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, workspace_bytes_for(B, max_boxes, tracks));
    MPN_REQUIRE(sources_bytes >= 3 && out_bytes >= 16, MPN_ERR_WORKSPACE, "%s: sources of %zu bytes, out_rgba of %zu bytes", who,
                sources_bytes, out_bytes);
    return MPN_OK;
}

// the two launches; tr: a Tracks (its `persons` is set here, behind the primitives) or a NoTracks
template <bool kTracks, typename TrackArgs>
int launch_draw(const uint8_t* sources, size_t sources_bytes, const void* descs, const void* record, int B, int max_boxes,
                int with_keypoints, uint8_t* out_rgba, size_t out_bytes, void* workspace, TrackArgs tr, mpn_stream_t stream) {
    const Desc* dd = reinterpret_cast<const Desc*>(descs);
    const int* header = reinterpret_cast<const int*>(record);
    const float* rows = reinterpret_cast<const float*>(reinterpret_cast<const char*>(record) + record_header_words(B) * 4);
    Prim* prims = reinterpret_cast<Prim*>(workspace);
    const long long count = (long long)B * max_boxes * prims_per_person(kTracks);
    if constexpr (kTracks) tr.persons = reinterpret_cast<uint4*>(prims + count);
    draw_prims_kernel<kTracks><<<mpn_div_up(count, kThreads), kThreads, 0, (hipStream_t)stream>>>(
        dd, header, rows, B, max_boxes, with_keypoints, prims, tr);
    MPN_LAUNCH_CHECK();
    draw_raster_kernel<kTracks><<<dim3(kTileBlocks, (unsigned)B), kThreads, 0, (hipStream_t)stream>>>(
        sources, sources_bytes, dd, header, B, max_boxes, prims, out_rgba, out_bytes, tr);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}

}  // namespace

extern "C" size_t mpn_draw_desc_bytes(void) { return sizeof(Desc); }

extern "C" int mpn_draw_dot_stamp(int dw, int dh, int row) {
    if (dw < 3 || dw > 4 || dh < 3 || dh > 4 || row < 0 || row > dh) return -1;
    return kStampsHost[(dw - 3) * 2 + (dh - 3)][row];
}

extern "C" size_t mpn_draw_detections_workspace_bytes(int B, int max_boxes) { return workspace_bytes_for(B, max_boxes, false); }

extern "C" int mpn_draw_detections(const uint8_t* sources, size_t sources_bytes, const void* descs, const void* record,
                                   size_t record_bytes, int B, int max_boxes, int with_keypoints, uint8_t* out_rgba,
                                   size_t out_bytes, void* workspace, size_t workspace_bytes, mpn_stream_t stream) {
    const int rc = check_draw("draw_detections", sources, sources_bytes, descs, record, record_bytes, B, max_boxes, out_rgba,
                              out_bytes, workspace, workspace_bytes, false);
    if (rc != MPN_OK) return rc;
    return launch_draw<false>(sources, sources_bytes, descs, record, B, max_boxes, with_keypoints, out_rgba, out_bytes, workspace,
                              NoTracks{}, stream);
}

extern "C" size_t mpn_draw_tracks_tables_bytes(int palette_size, int cell_w, int stamp_h) {
    if (palette_size < 1 || palette_size > kMaxPalette || cell_w < 1 || cell_w > kMaxCell || stamp_h < 0 || stamp_h > kMaxStampH)
        return 0;
    return round16((size_t)kTabHeaderBytes + (size_t)palette_size * 4 + (size_t)10 * (cell_w + 2 * kLabelPad) * stamp_h);
}

extern "C" size_t mpn_draw_tracks_workspace_bytes(int B, int max_boxes) { return workspace_bytes_for(B, max_boxes, true); }

extern "C" int mpn_draw_tracks(const uint8_t* sources, size_t sources_bytes, const void* descs, const void* record,
                               size_t record_bytes, const void* track_rows, const void* smooth_rows, const void* tables,
                               size_t tables_bytes, int B, int max_boxes, int with_keypoints, uint8_t* out_rgba, size_t out_bytes,
                               void* workspace, size_t workspace_bytes, mpn_stream_t stream) {
    MPN_REQUIRE(track_rows && tables, MPN_ERR_BAD_ARG, "draw_tracks: null pointer");
    const int rc = check_draw("draw_tracks", sources, sources_bytes, descs, record, record_bytes, B, max_boxes, out_rgba, out_bytes,
                              workspace, workspace_bytes, true);
    if (rc != MPN_OK) return rc;
    MPN_REQUIRE((((uintptr_t)track_rows | (uintptr_t)smooth_rows | (uintptr_t)tables) & 3u) == 0, MPN_ERR_BAD_ALIGN,
                "draw_tracks: track_rows, smooth_rows and tables must be 4-byte aligned");
    MPN_REQUIRE(tables_bytes >= (size_t)kTabHeaderBytes, MPN_ERR_WORKSPACE, "draw_tracks: tables of %zu bytes, the header alone is %d",
                tables_bytes, kTabHeaderBytes);
    Tracks tr = {reinterpret_cast<const int*>(track_rows), reinterpret_cast<const float*>(smooth_rows),
                 reinterpret_cast<const int*>(tables), tables_bytes, nullptr};
    return launch_draw<true>(sources, sources_bytes, descs, record, B, max_boxes, with_keypoints, out_rgba, out_bytes, workspace, tr,
                             stream);
}
