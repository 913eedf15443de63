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
constexpr int kMaskWords = (kMaxBoxes * kPrims + 31) / 32;
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

__global__ void __launch_bounds__(kThreads) draw_prims_kernel(const Desc* __restrict__ descs, const int* __restrict__ header,
                                                              const float* __restrict__ rows, int B, int max_boxes,
                                                              int with_keypoints, Prim* __restrict__ prims) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    const int n = B * max_boxes;
    if (t >= n * kPrims) return;
    const int j = t / kPrims, k = t - j * kPrims;
    if (j >= min(max(header[0], 0), n)) return;         // rows behind `total` are never read by the raster kernel
    const float* row = rows + (size_t)j * kRowWords;
    Prim p = {1, 1, 0, 0, 0, 0, 0, 0};
    const int img = __float_as_int(row[0]);
    if (img >= 0 && img < B && (k == 0 || with_keypoints)) {
        const Desc d = descs[img];
        // scaler * boxes: int64 * float32 -> float64
        const double ymin = (double)d.h * (double)row[kOffBox], xmin = (double)d.w * (double)row[kOffBox + 1];
        const double ymax = (double)d.h * (double)row[kOffBox + 2], xmax = (double)d.w * (double)row[kOffBox + 3];
        if (k == 0) {
            p.x0 = trunc_int(xmin); p.y0 = trunc_int(ymin); p.x1 = trunc_int(xmax); p.y1 = trunc_int(ymax);
            p.bx0 = p.x0; p.by0 = p.y0; p.bx1 = p.x1;
            p.by1 = p.y1 == p.y0 ? p.y0 + 1 : p.y1;
            if (p.y1 < p.y0) p.bx1 = p.bx0 - 1;         // (Pillow refuses such a box)
        } else {
            const float* pos = row + kOffKPos;          // (y, x) normalised to the box
            // keypoints *= [xmax - xmin, ymax - ymin]; keypoints += [xmin, ymin]: float64 results rounded to float32
            auto kx = [&](int q) { return (float)((double)(float)((double)pos[2 * q + 1] * (xmax - xmin)) + xmin); };
            auto ky = [&](int q) { return (float)((double)(float)((double)pos[2 * q] * (ymax - ymin)) + ymin); };
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

__global__ void __launch_bounds__(kThreads) draw_raster_kernel(const uint8_t* __restrict__ sources, size_t sources_bytes,
                                                               const Desc* __restrict__ descs, const int* __restrict__ header,
                                                               int B, int max_boxes, const Prim* __restrict__ prims,
                                                               uint8_t* __restrict__ out, size_t out_bytes) {
    __shared__ unsigned mask[kWaves][kMaskWords];
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
    const Prim* mine = prims + (size_t)person_range[0] * kPrims;
    const int nprims = person_range[1] * kPrims, words = (nprims + 31) >> 5;
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
                const int kind = p % kPrims;
                const unsigned ink = (kind >= 1 && kind <= kEdges) ? kWhite : kRed;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (((open >> i) & 1u) && xs[i] >= bb.x && xs[i] <= bb.z && ys[i] >= bb.y && ys[i] <= bb.w &&
                        covers(kind, c, xs[i], ys[i])) {
                        px[i] = ink;
                        open &= ~(1u << i);
                    }
                }
            }
        }
        dst[g] = make_uint4(px[0], px[1], px[2], px[3]);
    }
}

}  // namespace

extern "C" size_t mpn_draw_desc_bytes(void) { return sizeof(Desc); }

extern "C" int mpn_draw_dot_stamp(int dw, int dh, int row) {
    if (dw < 3 || dw > 4 || dh < 3 || dh > 4 || row < 0 || row > dh) return -1;
    return kStampsHost[(dw - 3) * 2 + (dh - 3)][row];
}

extern "C" size_t mpn_draw_detections_workspace_bytes(int B, int max_boxes) {
    if (B < 1 || max_boxes < 1 || max_boxes > kMaxBoxes || (long long)B * max_boxes > kMaxRows) return 0;
    return (size_t)B * max_boxes * kPrims * sizeof(Prim);
}

extern "C" int mpn_draw_detections(const uint8_t* sources, size_t sources_bytes, const void* descs, const void* record,
                                   size_t record_bytes, int B, int max_boxes, int with_keypoints, uint8_t* out_rgba,
                                   size_t out_bytes, void* workspace, size_t workspace_bytes, mpn_stream_t stream) {
    MPN_REQUIRE(sources && descs && record && out_rgba && workspace, MPN_ERR_BAD_ARG, "draw_detections: null pointer");
    MPN_REQUIRE(B >= 1 && B <= 65535, MPN_ERR_BAD_SHAPE, "draw_detections: B must be in [1, 65535] (got %d)", B);
    MPN_REQUIRE(max_boxes >= 1 && max_boxes <= kMaxBoxes, MPN_ERR_BAD_SHAPE,
                "draw_detections: max_boxes must be in [1, %d] (got %d)", kMaxBoxes, max_boxes);
    MPN_REQUIRE((long long)B * max_boxes <= kMaxRows, MPN_ERR_BAD_SHAPE,
                "draw_detections: B * max_boxes = %lld rows, mpn_pose_gather's record holds %d", (long long)B * max_boxes, kMaxRows);
    MPN_REQUIRE(mpn_aligned16(descs) && mpn_aligned16(record) && mpn_aligned16(out_rgba) && mpn_aligned16(workspace),
                MPN_ERR_BAD_ALIGN, "draw_detections: descs, record, out_rgba and workspace must be 16-byte aligned");
    MPN_REQUIRE(mpn_pose_gather_row_offset(B, max_boxes, 0) == record_header_words(B) * 4 &&
                    mpn_pose_gather_row_offset(B, max_boxes, 1) - mpn_pose_gather_row_offset(B, max_boxes, 0) == kRowWords * 4,
                MPN_ERR_BAD_ARG, "draw_detections: the record's layout is not the one this kernel was written against");
    MPN_REQUIRE(record_bytes >= mpn_pose_gather_record_bytes(B, max_boxes), MPN_ERR_WORKSPACE,
                "draw_detections: record of %zu bytes, %zu needed", record_bytes, mpn_pose_gather_record_bytes(B, max_boxes));
    MPN_REQUIRE(workspace_bytes >= mpn_draw_detections_workspace_bytes(B, max_boxes), MPN_ERR_WORKSPACE,
                "draw_detections: workspace of %zu bytes, %zu needed", workspace_bytes, mpn_draw_detections_workspace_bytes(B, max_boxes));
    MPN_REQUIRE(sources_bytes >= 3 && out_bytes >= 16, MPN_ERR_WORKSPACE,
                "draw_detections: sources of %zu bytes, out_rgba of %zu bytes", sources_bytes, out_bytes);
    const Desc* dd = reinterpret_cast<const Desc*>(descs);
    const int* header = reinterpret_cast<const int*>(record);
    const float* rows = reinterpret_cast<const float*>(reinterpret_cast<const char*>(record) + record_header_words(B) * 4);
    Prim* prims = reinterpret_cast<Prim*>(workspace);
    draw_prims_kernel<<<mpn_div_up((long long)B * max_boxes * kPrims, kThreads), kThreads, 0, (hipStream_t)stream>>>(
        dd, header, rows, B, max_boxes, with_keypoints, prims);
    MPN_LAUNCH_CHECK();
    draw_raster_kernel<<<dim3(kTileBlocks, (unsigned)B), kThreads, 0, (hipStream_t)stream>>>(
        sources, sources_bytes, dd, header, B, max_boxes, prims, out_rgba, out_bytes);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
