// Persons made unrecognisable on the device (mpn_anonymize, include/mpn.h states the arithmetic, tests/anonymize_ref.py restates
// it as plain loops): out_rgb = the packed RGB sources with, per kept person of mpn_pose_gather's record, a region - the head
// from the five face joints, or the box - pixelated, blurred or filled. A pixel takes the LAST person of its image that covers
// it, and that person always reads the ORIGINAL sources.
//
//   anon_regions_kernel  one thread per record row: the f64 bounds, the integer region [x0,x1) x [y0,y1), the mosaic's cell
//                        size, the row's image and where that image's rows end -> workspace (32 bytes a row; img < 0: none).
//   anon_copy_kernel     every valid frame's bytes, sources -> out_rgb at the same offset: 16 bytes a lane from the first
//                        16-byte boundary of the destination, the head and the tail byte by byte (offsets are arbitrary).
//   anon_cells_kernel    pixelate only: one wave per (row, cell) sums the cell's source pixels inside the frame and writes the
//                        rounded mean -> workspace. At most blocks^2 cells a region.
//   anon_paint_kernel    blocks (x, row) walk the 32 x 32 tiles of the row's region clipped to its frame. A pixel is written iff
//                        the row's region covers it and no LATER row of the same image does (those rows' own blocks write it):
//                        every pixel has one writer behind the copy, nothing scatters, no global atomics. Blur: the tile and a
//                        margin of 3 * radius go to LDS as one dword a pixel and the six 1-D box means run there, every sample
//                        index clamped to the frame; what the margin's outer columns and rows hold after a pass is wrong where
//                        the window's edge is not the frame's, and that grows by `radius` a pass - it ends at the tile's edge.
//
// Mosaic means and blur are computed only where a region lies; the rest of a frame is the streaming copy. Grids depend on
// (B, max_boxes, params) alone. No descriptor makes a kernel read outside `sources` or write outside `out_rgb`: desc_ok()
// rejects it, the image is left unwritten and its rows have no region.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBoxes = MPN_DRAW_MAX_BOXES;
constexpr int kMaxRows = 4096;          // mpn_pose_gather's one-block limit
constexpr int kRowWords = 108, kOffBox = 1, kOffKeypoints = 57;     // a row of mpn_pose_gather's record, in 32-bit words
constexpr int kFace = 5;                // nose, eyes, ears: joints 0..4
constexpr int kMaxBlocks = MPN_ANONYMIZE_MAX_BLOCKS, kMaxRadius = MPN_ANONYMIZE_MAX_RADIUS;
constexpr int kMaxCells = kMaxBlocks * kMaxBlocks;
constexpr int kTile = 32;
constexpr int kCopyBlocks = 512;        // blocks per image of the copy (grid-stride over the frame's 16-byte vectors)
constexpr int kPaintBlocks = 32;        // blocks per record row of the paint kernel (grid-stride over the region's tiles)
constexpr double kBound = 1048576.0;    // bounds are clamped to +-2^20
constexpr int kEllipseMax = 32768;      // a larger region is a rectangle: the ellipse test stays inside 62 bits
constexpr int kLaterBytes = kMaxBoxes * 16;
constexpr int kMaxWindow = kTile + 6 * kMaxRadius;
constexpr int kBlurLdsBytes = kLaterBytes + 2 * 4 * kMaxWindow * kMaxWindow;

enum { kHead = 0, kBox = 1 };
enum { kPixelate = 0, kBlur = 1, kFill = 2 };
enum { kEllipse = 0, kRectangle = 1 };

typedef mpn_draw_desc Desc;
typedef mpn_anonymize_params Params;

struct Region {
    int x0, y0, x1, y1;     // half-open
    int cell;               // the mosaic's cell size
    int img;                // < 0: no region
    int end;                // one past the last record row of the image
    int reserved;
};
static_assert(sizeof(Region) == 32, "two 16-byte vectors");

inline size_t record_header_words(int B) { return ((size_t)(2 * B + 2) + 3) / 4 * 4; }

__device__ __forceinline__ bool desc_ok(const Desc& d, size_t sources_bytes, size_t out_bytes) {
    if (d.h < 1 || d.w < 1 || d.h > 65536 || d.w > 65536) return false;
    const unsigned long long npix = (unsigned long long)d.h * (unsigned long long)d.w;
    if (npix > (1ull << 29)) return false;                                          // what mpn_draw_detections accepts
    if (d.src_offset < 0) return false;
    const unsigned long long end = (unsigned long long)d.src_offset + npix * 3;
    return end <= sources_bytes && end <= out_bytes;
}

__device__ __forceinline__ Region load_region(const Region* regions, int j) {
    const int4 a = reinterpret_cast<const int4*>(regions + j)[0], b = reinterpret_cast<const int4*>(regions + j)[1];
    return {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}

__global__ void __launch_bounds__(kThreads) anon_regions_kernel(const Desc* __restrict__ descs, size_t sources_bytes,
                                                                size_t out_bytes, const int* __restrict__ header,
                                                                const float* __restrict__ rows, int B, int max_boxes,
                                                                int with_keypoints, const Params p, Region* __restrict__ regions) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    const int n = B * max_boxes;
    if (t >= n) return;
    Region r = {0, 0, 0, 0, 1, -1, 0, 0};
    const int total = min(max(header[0], 0), n);
    const float* row = rows + (size_t)t * kRowWords;
    const int img = t < total ? __float_as_int(row[0]) : -1;
    if (img >= 0 && img < B) {
        // the image's rows by the header, counts clamped as the drawing clamps them
        int first = 0;
        for (int i = 0; i < img; ++i) first += min(max(header[1 + i], 0), max_boxes);
        const int end = min(first + min(max(header[1 + img], 0), max_boxes), total);
        const Desc d = descs[img];
        if (t >= first && t < end && desc_ok(d, sources_bytes, out_bytes)) {
            const double h = (double)d.h, w = (double)d.w;
            const double by0 = (double)row[kOffBox] * h, bx0 = (double)row[kOffBox + 1] * w;
            const double by1 = (double)row[kOffBox + 2] * h, bx1 = (double)row[kOffBox + 3] * w;
            double fx0 = bx0, fy0 = by0, fx1 = bx1, fy1 = by1;
            if (p.region == kHead) {
                const float* kp = row + kOffKeypoints;      // (x, y, score) in image pixels
                bool in[kFace];
                int count = 0;
                double cx = 0.0, cy = 0.0;
                for (int j = 0; j < kFace; ++j) {
                    in[j] = with_keypoints != 0 && kp[3 * j + 2] >= p.min_keypoint_score;     // (a NaN score: false)
                    if (in[j]) { cx += (double)kp[3 * j]; cy += (double)kp[3 * j + 1]; ++count; }
                }
                if (count > 0) {
                    cx /= (double)count; cy /= (double)count;
                    double e = 0.0;
                    for (int j = 0; j < kFace; ++j) {
                        if (!in[j]) continue;
                        const double dx = fabs((double)kp[3 * j] - cx), dy = fabs((double)kp[3 * j + 1] - cy);
                        if (dx > e) e = dx;
                        if (dy > e) e = dy;
                    }
                    double s = e * p.scale;
                    const double least = (by1 - by0) * p.min_size;
                    if (least > s) s = least;
                    fx0 = cx - s; fy0 = cy - s; fx1 = cx + s; fy1 = cy + s;
                } else {
                    fy1 = by0 + (by1 - by0) * p.fallback;
                }
            }
            if (isfinite(fx0) && isfinite(fy0) && isfinite(fx1) && isfinite(fy1)) {
                const int x0 = (int)floor(fmin(fmax(fx0, -kBound), kBound)), y0 = (int)floor(fmin(fmax(fy0, -kBound), kBound));
                const int x1 = (int)ceil(fmin(fmax(fx1, -kBound), kBound)), y1 = (int)ceil(fmin(fmax(fy1, -kBound), kBound));
                if (x1 > x0 && y1 > y0) {
                    const int side = max(x1 - x0, y1 - y0);
                    r = {x0, y0, x1, y1, (side + p.blocks - 1) / p.blocks, img, end, 0};
                }
            }
        }
    }
    int4* dst = reinterpret_cast<int4*>(regions + t);
    dst[0] = make_int4(r.x0, r.y0, r.x1, r.y1);
    dst[1] = make_int4(r.cell, r.img, r.end, 0);
}

__global__ void __launch_bounds__(kThreads) anon_copy_kernel(const uint8_t* __restrict__ sources, size_t sources_bytes,
                                                             const Desc* __restrict__ descs, uint8_t* __restrict__ out,
                                                             size_t out_bytes) {
    const Desc d = descs[blockIdx.y];
    if (!desc_ok(d, sources_bytes, out_bytes)) return;
    const size_t nbytes = (size_t)d.h * (size_t)d.w * 3;
    const uint8_t* src = sources + d.src_offset;
    uint8_t* dst = out + d.src_offset;
    size_t head = (size_t)((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u);
    if (head > nbytes) head = nbytes;
    const size_t nvec = (nbytes - head) / 16, tail_at = head + nvec * 16;
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x, stride = (size_t)gridDim.x * kThreads;
    uint4* vdst = reinterpret_cast<uint4*>(dst + head);
    if ((((uintptr_t)(src + head)) & 15u) == 0) {
        const uint4* vsrc = reinterpret_cast<const uint4*>(src + head);
        for (size_t v = g; v < nvec; v += stride) vdst[v] = vsrc[v];
    } else {                                // the two buffers differ in alignment: unaligned loads, aligned stores
        for (size_t v = g; v < nvec; v += stride) {
            uint4 q;
            __builtin_memcpy(&q, src + head + v * 16, 16);
            vdst[v] = q;
        }
    }
    if (blockIdx.x == 0) {                  // head and tail: fewer than 16 bytes each
        if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
        if (tail_at + threadIdx.x < nbytes) dst[tail_at + threadIdx.x] = src[tail_at + threadIdx.x];
    }
}

__device__ __forceinline__ unsigned rounded_mean(unsigned long long s, unsigned long long n) { return (unsigned)((2 * s + n) / (2 * n)); }

__global__ void __launch_bounds__(kThreads) anon_cells_kernel(const uint8_t* __restrict__ sources, const Desc* __restrict__ descs,
                                                              const Region* __restrict__ regions, int n, int blocks,
                                                              unsigned* __restrict__ cells) {
    const int per = blocks * blocks;
    const long long wave = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int j = (int)(wave / per), k = (int)(wave - (long long)j * per);
    if (j >= n) return;
    const Region r = load_region(regions, j);       // (uniform over the wave)
    unsigned result = 0u;
    if (r.img >= 0) {
        const Desc d = descs[r.img];
        const int ci = k % blocks, cj = k / blocks;
        const int ox = r.x0 + ci * r.cell, oy = r.y0 + cj * r.cell;     // |x0| <= 2^20, cell <= 2^21, ci < 32: inside int32
        const int xa = max(ox, 0), xb = min(ox + r.cell, d.w), ya = max(oy, 0), yb = min(oy + r.cell, d.h);
        if (ox < r.x1 && oy < r.y1 && xa < xb && ya < yb) {
            const int cw = xb - xa, count = cw * (yb - ya);             // inside the frame: <= 2^29
            const uint8_t* img = sources + d.src_offset;
            unsigned sr = 0u, sg = 0u, sb = 0u;                         // a lane sums at most 2^23 pixels
            for (int idx = lane; idx < count; idx += 64) {
                const int y = ya + idx / cw, x = xa + idx % cw;
                const uint8_t* q = img + ((size_t)y * d.w + x) * 3;
                sr += q[0]; sg += q[1]; sb += q[2];
            }
            unsigned long long tr = sr, tg = sg, tb = sb;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                tr += __shfl_xor(tr, o, 64); tg += __shfl_xor(tg, o, 64); tb += __shfl_xor(tb, o, 64);
            }
            const unsigned long long cnt = (unsigned long long)count;
            result = rounded_mean(tr, cnt) | (rounded_mean(tg, cnt) << 8) | (rounded_mean(tb, cnt) << 16);
        }
    }
    if (lane == 0) cells[(size_t)j * per + k] = result;
}

// is frame pixel (x, y) covered by the region c = (x0, y0, x1, y1)?
__device__ __forceinline__ bool covers(const int4& c, bool ellipse, int x, int y) {
    if (x < c.x || x >= c.z || y < c.y || y >= c.w) return false;
    const long long a = c.z - c.x, b = c.w - c.y;
    if (!ellipse || a > kEllipseMax || b > kEllipseMax) return true;
    const long long u = 2LL * x + 1 - ((long long)c.x + c.z), v = 2LL * y + 1 - ((long long)c.y + c.w);     // |u| <= a, |v| <= b
    return u * u * b * b + v * v * a * a <= a * a * b * b;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// one 1-D box mean of radius R over `from` (a window of ww x wh pixels whose corner is frame pixel (wx0, wy0)) into `to`,
// along x (dx = 1) or y; sample positions are clamped to [lo, hi], the part of the frame the window holds along that axis
__device__ __forceinline__ void blur_pass(const unsigned* from, unsigned* to, int ww, int wh, int origin, int lo, int hi, int R,
                                          bool along_x) {
    const unsigned n = 2u * (unsigned)R + 1u;
    for (int idx = threadIdx.x; idx < ww * wh; idx += kThreads) {
        const int wy = idx / ww, wx = idx - wy * ww;
        unsigned rb = 0u, g = 0u;
        for (int k = -R; k <= R; ++k) {
            const int at = clampi(origin + (along_x ? wx : wy) + k, lo, hi) - origin;
            const unsigned v = from[along_x ? wy * ww + at : at * ww + wx];
            rb += v & 0x00FF00FFu;          // at most 25 * 255 a half
            g += (v >> 8) & 0xFFu;
        }
        const unsigned r = rb & 0xFFFFu, b = rb >> 16;
        to[idx] = ((2u * r + n) / (2u * n)) | (((2u * g + n) / (2u * n)) << 8) | (((2u * b + n) / (2u * n)) << 16);
    }
}

__global__ void __launch_bounds__(kThreads) anon_paint_kernel(const uint8_t* __restrict__ sources, const Desc* __restrict__ descs,
                                                              const Region* __restrict__ regions, const unsigned* __restrict__ cells,
                                                              const Params p, uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int4* later = reinterpret_cast<int4*>(smem);            // the regions of the image's later rows
    const int j = blockIdx.y, tid = threadIdx.x;
    const Region r = load_region(regions, j);               // (uniform over the block)
    if (r.img < 0) return;
    const Desc d = descs[r.img];                            // checked by the regions kernel: the row has a region
    const int w = d.w, h = d.h;
    const int cx0 = max(r.x0, 0), cy0 = max(r.y0, 0), cx1 = min(r.x1, w), cy1 = min(r.y1, h);
    if (cx0 >= cx1 || cy0 >= cy1) return;
    const int nlater = min(max(r.end - (j + 1), 0), kMaxBoxes);
    for (int i = tid; i < nlater; i += kThreads) {
        const Region q = load_region(regions, j + 1 + i);
        later[i] = q.img == r.img ? make_int4(q.x0, q.y0, q.x1, q.y1) : make_int4(0, 0, 0, 0);
    }
    __syncthreads();
    const bool ellipse = p.shape == kEllipse;
    const int4 mine = make_int4(r.x0, r.y0, r.x1, r.y1);
    const uint8_t* img = sources + d.src_offset;
    uint8_t* dst = out + d.src_offset;
    const int R = p.radius, margin = 3 * R;
    unsigned* bufa = reinterpret_cast<unsigned*>(smem + kLaterBytes);
    unsigned* bufb = bufa + (kTile + 2 * margin) * (kTile + 2 * margin);
    const int tiles_x = (cx1 - cx0 + kTile - 1) / kTile, tiles_y = (cy1 - cy0 + kTile - 1) / kTile;
    const int ntiles = tiles_x * tiles_y;                   // a frame has at most 2048 x 2048 tiles
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {         // (uniform: every thread reaches the barriers)
        const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
        const int tx = cx0 + txi * kTile, ty = cy0 + tyi * kTile;
        const int tw = min(kTile, cx1 - tx), th = min(kTile, cy1 - ty);
        const int wx0 = tx - margin, wy0 = ty - margin, ww = tw + 2 * margin, wh = th + 2 * margin;
        if (p.mode == kBlur) {
            __syncthreads();                                // the previous tile's result has been read
            for (int idx = tid; idx < ww * wh; idx += kThreads) {
                const int wy = idx / ww, wx = idx - wy * ww;
                const uint8_t* q = img + ((size_t)clampi(wy0 + wy, 0, h - 1) * w + clampi(wx0 + wx, 0, w - 1)) * 3;
                bufa[idx] = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
            }
            const int lox = max(wx0, 0), hix = min(wx0 + ww, w) - 1, loy = max(wy0, 0), hiy = min(wy0 + wh, h) - 1;
            for (int pass = 0; pass < 3; ++pass) {
                __syncthreads();
                blur_pass(bufa, bufb, ww, wh, wx0, lox, hix, R, true);
                __syncthreads();
                blur_pass(bufb, bufa, ww, wh, wy0, loy, hiy, R, false);
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < kTile * kTile / kThreads; ++k) {
            const int at = tid + k * kThreads, ly = at / kTile, lx = at % kTile;
            if (lx >= tw || ly >= th) continue;
            const int x = tx + lx, y = ty + ly;
            if (!covers(mine, ellipse, x, y)) continue;
            bool hidden = false;
            for (int i = 0; i < nlater && !hidden; ++i) hidden = covers(later[i], ellipse, x, y);
            if (hidden) continue;                           // a later person's block writes this pixel
            unsigned colour = (unsigned)p.color;
            if (p.mode == kPixelate)
                colour = cells[(size_t)j * (p.blocks * p.blocks) + (size_t)((y - r.y0) / r.cell) * p.blocks + (x - r.x0) / r.cell];
            else if (p.mode == kBlur)
                colour = bufa[(y - wy0) * ww + (x - wx0)];
            uint8_t* q = dst + ((size_t)y * w + x) * 3;
            q[0] = (uint8_t)colour; q[1] = (uint8_t)(colour >> 8); q[2] = (uint8_t)(colour >> 16);
        }
    }
}

inline size_t workspace_bytes_for(int B, int max_boxes) {
    if (B < 1 || max_boxes < 1 || max_boxes > kMaxBoxes || (long long)B * max_boxes > kMaxRows) return 0;
    const size_t rows = (size_t)B * max_boxes;
    return rows * sizeof(Region) + rows * kMaxCells * sizeof(unsigned);
}

mpn_attr_mask_t g_paint_lds;

}  // namespace

extern "C" size_t mpn_anonymize_params_bytes(void) { return sizeof(Params); }

extern "C" size_t mpn_anonymize_workspace_bytes(int B, int max_boxes) { return workspace_bytes_for(B, max_boxes); }

extern "C" int mpn_anonymize(const uint8_t* sources, size_t sources_bytes, const void* descs, const void* record, size_t record_bytes,
                             int B, int max_boxes, int with_keypoints, const mpn_anonymize_params* params, uint8_t* out_rgb,
                             size_t out_bytes, void* workspace, size_t workspace_bytes, mpn_stream_t stream) {
    MPN_REQUIRE(sources && descs && record && params && out_rgb && workspace, MPN_ERR_BAD_ARG, "anonymize: null pointer");
    MPN_REQUIRE(B >= 1 && B <= 65535, MPN_ERR_BAD_SHAPE, "anonymize: B must be in [1, 65535] (got %d)", B);
    MPN_REQUIRE(max_boxes >= 1 && max_boxes <= kMaxBoxes, MPN_ERR_BAD_SHAPE, "anonymize: max_boxes must be in [1, %d] (got %d)",
                kMaxBoxes, max_boxes);
    MPN_REQUIRE((long long)B * max_boxes <= kMaxRows, MPN_ERR_BAD_SHAPE,
                "anonymize: B * max_boxes = %lld rows, mpn_pose_gather's record holds %d", (long long)B * max_boxes, kMaxRows);
    MPN_REQUIRE(mpn_aligned16(descs) && mpn_aligned16(record) && mpn_aligned16(workspace), MPN_ERR_BAD_ALIGN,
                "anonymize: descs, record and workspace must be 16-byte aligned");
    MPN_REQUIRE(mpn_pose_gather_row_offset(B, max_boxes, 0) == record_header_words(B) * 4 &&
                    mpn_pose_gather_row_offset(B, max_boxes, 1) - mpn_pose_gather_row_offset(B, max_boxes, 0) == kRowWords * 4,
                MPN_ERR_BAD_ARG, "anonymize: the record's layout is not the one this kernel was written against");
    MPN_REQUIRE(record_bytes >= mpn_pose_gather_record_bytes(B, max_boxes), MPN_ERR_WORKSPACE,
                "anonymize: record of %zu bytes, %zu needed", record_bytes, mpn_pose_gather_record_bytes(B, max_boxes));
    MPN_REQUIRE(workspace_bytes >= workspace_bytes_for(B, max_boxes), MPN_ERR_WORKSPACE,
                "anonymize: workspace of %zu bytes, %zu needed", workspace_bytes, workspace_bytes_for(B, max_boxes));
    MPN_REQUIRE(sources_bytes >= 3 && out_bytes >= 3, MPN_ERR_WORKSPACE, "anonymize: sources of %zu bytes, out_rgb of %zu bytes",
                sources_bytes, out_bytes);
    const Params p = *params;
    MPN_REQUIRE(p.region == kHead || p.region == kBox, MPN_ERR_BAD_ARG, "anonymize: region must be 0 (head) or 1 (box) (got %d)",
                p.region);
    MPN_REQUIRE(p.mode == kPixelate || p.mode == kBlur || p.mode == kFill, MPN_ERR_BAD_ARG,
                "anonymize: mode must be 0 (pixelate), 1 (blur) or 2 (fill) (got %d)", p.mode);
    MPN_REQUIRE(p.shape == kEllipse || p.shape == kRectangle, MPN_ERR_BAD_ARG,
                "anonymize: shape must be 0 (ellipse) or 1 (rectangle) (got %d)", p.shape);
    MPN_REQUIRE(p.blocks >= 2 && p.blocks <= kMaxBlocks, MPN_ERR_BAD_ARG, "anonymize: blocks must be in [2, %d] (got %d)",
                kMaxBlocks, p.blocks);
    MPN_REQUIRE(p.radius >= 1 && p.radius <= kMaxRadius, MPN_ERR_BAD_ARG, "anonymize: radius must be in [1, %d] (got %d)",
                kMaxRadius, p.radius);
    MPN_REQUIRE(p.color >= 0 && p.color <= 0xFFFFFF, MPN_ERR_BAD_ARG, "anonymize: color must be R | G << 8 | B << 16 (got %d)",
                p.color);
    MPN_REQUIRE(std::isfinite(p.scale) && p.scale > 0, MPN_ERR_BAD_ARG, "anonymize: scale must be finite and > 0 (got %g)", p.scale);
    MPN_REQUIRE(std::isfinite(p.min_size) && p.min_size >= 0, MPN_ERR_BAD_ARG, "anonymize: min_size must be finite and >= 0 (got %g)",
                p.min_size);
    MPN_REQUIRE(std::isfinite(p.fallback) && p.fallback > 0 && p.fallback <= 1, MPN_ERR_BAD_ARG,
                "anonymize: fallback must be in (0, 1] (got %g)", p.fallback);
    MPN_REQUIRE(std::isfinite(p.min_keypoint_score), MPN_ERR_BAD_ARG, "anonymize: min_keypoint_score must be finite (got %g)",
                (double)p.min_keypoint_score);

    const Desc* dd = reinterpret_cast<const Desc*>(descs);
    const int* header = reinterpret_cast<const int*>(record);
    const float* rows = reinterpret_cast<const float*>(reinterpret_cast<const char*>(record) + record_header_words(B) * 4);
    const int n = B * max_boxes;
    Region* regions = reinterpret_cast<Region*>(workspace);
    unsigned* cells = reinterpret_cast<unsigned*>(regions + n);
    hipStream_t s = (hipStream_t)stream;
    anon_regions_kernel<<<mpn_div_up(n, kThreads), kThreads, 0, s>>>(dd, sources_bytes, out_bytes, header, rows, B, max_boxes,
                                                                     with_keypoints, p, regions);
    MPN_LAUNCH_CHECK();
    anon_copy_kernel<<<dim3(kCopyBlocks, (unsigned)B), kThreads, 0, s>>>(sources, sources_bytes, dd, out_rgb, out_bytes);
    MPN_LAUNCH_CHECK();
    if (p.mode == kPixelate) {
        anon_cells_kernel<<<mpn_div_up((long long)n * p.blocks * p.blocks, kWaves), kThreads, 0, s>>>(sources, dd, regions, n,
                                                                                                      p.blocks, cells);
        MPN_LAUNCH_CHECK();
    }
    size_t lds = kLaterBytes;
    if (p.mode == kBlur) {
        const size_t side = (size_t)kTile + 6 * (size_t)p.radius;
        lds += 2 * 4 * side * side;
        MPN_HIP(mpn_ensure_dynamic_lds(reinterpret_cast<const void*>(anon_paint_kernel), kBlurLdsBytes, &g_paint_lds));
    }
    anon_paint_kernel<<<dim3(kPaintBlocks, (unsigned)n), kThreads, lds, s>>>(sources, dd, regions, cells, p, out_rgb);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
