// The picture of every person of a record, cut from its frame and resized to H x W on the device (mpn_person_crops,
// include/mpn.h states the arithmetic, tests/crops_ref.py restates it as plain loops): Pillow's bicubic
// `resize((new_w, new_h), box=(x0, y0, x1, y1))` of the whole frame, byte for byte, with the tap tables of every crop built
// on the device from the record's box - the boxes never reach the host before the crops are made.
//
//   crops_taps_kernel    one thread per (slot, axis, output coordinate): the slot's rectangle and placement (every thread of
//                        a slot computes the same f64 values; thread 0 writes the info row), then its own tap row: first,
//                        count and at most 65 fixed-point coefficients -> workspace. The weight sum is sequential.
//   crops_resize_kernel  one block per (slot, tile of output rows): the horizontal pass over the source rows the tile's
//                        vertical taps need -> LDS as uint8, new_w * 3 bytes a row; the vertical pass LDS -> crops_out, one
//                        dword of 4 output bytes a thread. Unused slots are zeros, empty and refused ones `fill`.
//
// The tile height comes from (H, W) on the host: the largest whose rows at a 16x reduction, tile * 16 + 64, of W * 3 bytes fit
// kLdsBytes; a slot that reduces less uses fewer of them (the row count is a device value). Grids depend on (B, max_boxes, H,
// W) alone. Every index a kernel derives from device memory is clamped before use: tap counts to kMaxKsize and the frame, LDS
// rows to the rows the block holds, frames to sources_bytes (desc_ok) - nothing is written outside crops_out, info_out and the
// workspace, nothing read outside sources.
#include "common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int kTapThreads = 256;
constexpr int kThreads = 512;
constexpr int kMaxBoxes = MPN_DRAW_MAX_BOXES;
constexpr int kMaxRows = 4096;          // mpn_pose_gather's one-block limit
constexpr int kRowWords = 108, kOffBox = 1;     // a row of mpn_pose_gather's record, in 32-bit words
constexpr int kBits = 22;               // Pillow's PRECISION_BITS
constexpr int kHalf = 1 << (kBits - 1);
constexpr int kMaxKsize = MPN_IMAGE_RESIZE_MAX_KSIZE;
constexpr int kTapWords = MPN_PERSON_CROPS_TAP_WORDS;
constexpr int kLdsBytes = MPN_PERSON_CROPS_LDS_BYTES;
constexpr int kMaxH = MPN_PERSON_CROPS_MAX_H, kMaxW = MPN_PERSON_CROPS_MAX_W;
static_assert(kTapWords >= 3 + kMaxKsize && kTapWords % 4 == 0, "a tap row holds first, count, a zero and the coefficients");

enum { kEmpty = MPN_PERSON_CROPS_EMPTY, kTooLarge = MPN_PERSON_CROPS_TOO_LARGE, kClipped = MPN_PERSON_CROPS_CLIPPED,
       kUsed = MPN_PERSON_CROPS_USED };
enum { kStretch = 0, kPad = 1 };

typedef mpn_draw_desc Desc;
typedef mpn_person_crops_info Info;
static_assert(sizeof(Info) == 64, "four 16-byte vectors");

inline size_t record_header_words(int B) { return ((size_t)(2 * B + 2) + 3) / 4 * 4; }

__device__ __forceinline__ bool desc_ok(const Desc& d, size_t sources_bytes) {
    if (d.h < 1 || d.w < 1 || d.h > 65536 || d.w > 65536) return false;
    const unsigned long long npix = (unsigned long long)d.h * (unsigned long long)d.w;
    if (npix > (1ull << 29)) return false;                                          // what mpn_draw_detections accepts
    if (d.src_offset < 0) return false;
    return (unsigned long long)d.src_offset + npix * 3 <= sources_bytes;
}

__device__ __forceinline__ int ksize_of(double in0, double in1, int out) {
    const double scale = (in1 - in0) / (double)out;
    const double support = 2.0 * fmax(scale, 1.0);
    return (int)fmin(ceil(support), 1048576.0) * 2 + 1;
}

// min(most, max(1, rint(v))): half to even; an infinite v gives most
__device__ __forceinline__ int rounded(double v, int most) { return (int)fmin((double)most, fmax(1.0, rint(v))); }

// the info row of slot s, and the size of its frame
__device__ Info slot_info(const Desc* __restrict__ descs, size_t sources_bytes, const int* __restrict__ header,
                          const float* __restrict__ rows, int B, int max_boxes, int s, int H, int W, double pad, int fit,
                          int& src_h, int& src_w) {
    Info r = {{0.0, 0.0, 0.0, 0.0}, {0, 0, 0, 0}, 0, 0, 0, 0};
    src_h = src_w = 0;
    const int n = B * max_boxes;
    const int total = min(max(header[0], 0), n);
    if (s >= total) return r;               // an unused slot: a row of zeros
    r.flags = kUsed | kEmpty;
    r.image = -1;
    const float* row = rows + (size_t)s * kRowWords;
    const int img = __float_as_int(row[0]);
    if (img < 0 || img >= B) return r;
    int first = 0;                          // the image's rows by the header, counts clamped as the drawing clamps them
    for (int i = 0; i < img; ++i) first += min(max(header[1 + i], 0), max_boxes);
    const int end = min(first + min(max(header[1 + img], 0), max_boxes), total);
    const Desc d = descs[img];
    if (s < first || s >= end || !desc_ok(d, sources_bytes)) return r;
    r.image = img;
    src_h = d.h;
    src_w = d.w;
    const double h = (double)d.h, w = (double)d.w;
    const double ymin = h * (double)row[kOffBox], xmin = w * (double)row[kOffBox + 1];
    const double ymax = h * (double)row[kOffBox + 2], xmax = w * (double)row[kOffBox + 3];
    const double bw = xmax - xmin, bh = ymax - ymin;
    const double px = pad * bw, py = pad * bh;
    double x0 = xmin - px, x1 = xmax + px, y0 = ymin - py, y1 = ymax + py;
    if (!(isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1))) return r;
    if (x0 < 0.0) { x0 = 0.0; r.flags |= kClipped; }
    if (x1 > w) { x1 = w; r.flags |= kClipped; }
    if (y0 < 0.0) { y0 = 0.0; r.flags |= kClipped; }
    if (y1 > h) { y1 = h; r.flags |= kClipped; }
    r.rect[0] = x0; r.rect[1] = y0; r.rect[2] = x1; r.rect[3] = y1;
    const double rw = x1 - x0, rh = y1 - y0;
    if (!(rw > 0.0) || !(rh > 0.0)) return r;
    r.flags &= ~kEmpty;
    int new_h = H, new_w = W;
    if (fit == kPad) {
        const double sy = (double)H / rh, sx = (double)W / rw;
        const double sc = fmin(sy, sx);
        new_h = rounded(rh * sc, H);
        new_w = rounded(rw * sc, W);
    }
    r.placed[0] = (H - new_h) / 2; r.placed[1] = (W - new_w) / 2; r.placed[2] = new_h; r.placed[3] = new_w;
    r.ksize_x = ksize_of(x0, x1, new_w);
    r.ksize_y = ksize_of(y0, y1, new_h);
    if (r.ksize_x > kMaxKsize || r.ksize_y > kMaxKsize) r.flags |= kTooLarge;
    return r;
}

__device__ __forceinline__ double bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
    return 0.0;
}

__global__ void __launch_bounds__(kTapThreads) crops_taps_kernel(const Desc* __restrict__ descs, size_t sources_bytes,
                                                                 const int* __restrict__ header, const float* __restrict__ rows,
                                                                 int B, int max_boxes, int H, int W, double pad, int fit,
                                                                 Info* __restrict__ info, int* __restrict__ taps) {
    const int s = blockIdx.y;
    const int t = blockIdx.x * kTapThreads + threadIdx.x;           // W columns, then H rows
    if (t >= H + W) return;
    int src_h, src_w;
    const Info r = slot_info(descs, sources_bytes, header, rows, B, max_boxes, s, H, W, pad, fit, src_h, src_w);
    if (t == 0) info[s] = r;
    int* tap = taps + ((size_t)s * (size_t)(H + W) + (size_t)t) * kTapWords;
    const bool along_x = t < W;
    const int xx = along_x ? t : t - W;
    const int out = along_x ? r.placed[3] : r.placed[2];
    int first = 0, count = 0;
    if (r.flags == kUsed || r.flags == (kUsed | kClipped)) {        // neither empty nor too large
        if (xx < out) {
            const double in0 = along_x ? r.rect[0] : r.rect[1], in1 = along_x ? r.rect[2] : r.rect[3];
            const int in_size = along_x ? src_w : src_h;
            const double scale = (in1 - in0) / (double)out;
            const double filterscale = fmax(scale, 1.0);
            const double support = 2.0 * filterscale;
            const double ss = 1.0 / filterscale;
            const double center = in0 + ((double)xx + 0.5) * scale;
            first = max((int)(center - support + 0.5), 0);
            const int last = min((int)(center + support + 0.5), in_size);
            count = min(max(last - first, 0), kMaxKsize);           // (ksize <= kMaxKsize: the clamp never cuts)
            double total = 0.0;
            for (int k = 0; k < count; ++k) total += bicubic(((double)(k + first) - center + 0.5) * ss);
            for (int k = 0; k < count; ++k) {
                double v = bicubic(((double)(k + first) - center + 0.5) * ss);
                if (total != 0.0) v = v / total;
                tap[3 + k] = v < 0.0 ? (int)(-0.5 + v * 4194304.0) : (int)(0.5 + v * 4194304.0);
            }
        }
    }
    tap[0] = first;
    tap[1] = count;
    tap[2] = 0;
}

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> kBits, 0), 255); }

// pixel p of an image as a dword (bits 0..23 = r, g, b); the last pixel byte by byte
__device__ __forceinline__ unsigned load_pixel(const uint8_t* __restrict__ img, long long p, long long last) {
    const uint8_t* q = img + p * 3;
    if (p < last) {
        unsigned v;
        __builtin_memcpy(&v, q, 4);
        return v;
    }
    return (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
}

__global__ void __launch_bounds__(kThreads) crops_resize_kernel(const uint8_t* __restrict__ sources, size_t sources_bytes,
                                                                const Desc* __restrict__ descs, int B, int H, int W, int tile,
                                                                int lds_rows, int fill, const Info* __restrict__ info,
                                                                const int* __restrict__ taps, uint8_t* __restrict__ crops) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rows_lds[];
    const int s = blockIdx.y, tid = threadIdx.x;
    const int ty0 = blockIdx.x * tile, ty1 = min(ty0 + tile, H);
    if (ty0 >= H) return;
    const int flags = info[s].flags, img = info[s].image;           // (uniform over the block)
    const int top = info[s].placed[0], left = info[s].placed[1], new_h = info[s].placed[2], new_w = info[s].placed[3];
    const int row_dwords = W * 3 / 4;
    unsigned* out = reinterpret_cast<unsigned*>(crops + (size_t)s * (size_t)H * (size_t)W * 3);
    const unsigned fill_bytes[3] = {(unsigned)fill & 255u, ((unsigned)fill >> 8) & 255u, ((unsigned)fill >> 16) & 255u};
    const bool used = (flags & kUsed) != 0;
    bool resized = flags == kUsed || flags == (kUsed | kClipped);
    // what launch 1 wrote is checked again: the placed part inside the crop, the image and its descriptor
    resized = resized && img >= 0 && img < B && new_h >= 1 && new_w >= 1 && top >= 0 && left >= 0 && top + new_h <= H &&
              left + new_w <= W;
    Desc d = {0, 0, 0, 0, {0, 0}};
    if (resized) {
        d = descs[img];
        resized = desc_ok(d, sources_bytes);
    }
    // the tile's rows inside the placed part, as rows of the resized picture
    const int ya = max(ty0, top) - top, yb = min(ty1, top + new_h) - top;
    const int* taps_x = taps + (size_t)s * (size_t)(H + W) * kTapWords;
    const int* taps_y = taps_x + (size_t)W * kTapWords;
    int lo = 0, nrows = 0;
    if (resized && ya < yb) {
        // first and first + count never decrease with the output row: the tile needs [first of its first row, end of its last)
        lo = min(max(taps_y[(size_t)ya * kTapWords], 0), d.h);
        const int* tl = taps_y + (size_t)(yb - 1) * kTapWords;
        const int hi = min(max(tl[0], 0) + min(max(tl[1], 0), kMaxKsize), d.h);
        nrows = min(max(hi - lo, 0), lds_rows);
        const int row_bytes = new_w * 3;
        const uint8_t* src = sources + d.src_offset;
        const long long last = (long long)d.h * d.w - 1;
        for (int idx = tid; idx < nrows * new_w; idx += kThreads) {
            const int r = idx / new_w, xx = idx - r * new_w;
            const int* tap = taps_x + (size_t)xx * kTapWords;
            const int first = min(max(tap[0], 0), d.w);
            const int n = min(min(max(tap[1], 0), kMaxKsize), d.w - first);
            const long long at = (long long)(lo + r) * d.w + first;
            int a0 = kHalf, a1 = kHalf, a2 = kHalf;
            for (int k = 0; k < n; ++k) {
                const int c = tap[3 + k];
                const unsigned v = load_pixel(src, at + k, last);
                a0 += (int)(v & 255u) * c;
                a1 += (int)((v >> 8) & 255u) * c;
                a2 += (int)((v >> 16) & 255u) * c;
            }
            unsigned char* q = rows_lds + (size_t)r * row_bytes + (size_t)xx * 3;
            q[0] = (unsigned char)clip8(a0);
            q[1] = (unsigned char)clip8(a1);
            q[2] = (unsigned char)clip8(a2);
        }
    }
    __syncthreads();                        // (every thread reaches it: the conditions above are uniform over the block)
    const int xa = left * 3, xb = (left + new_w) * 3;               // the placed bytes of a crop row
    for (int idx = tid; idx < (ty1 - ty0) * row_dwords; idx += kThreads) {
        const int y = ty0 + idx / row_dwords, v = idx % row_dwords;
        unsigned word = 0u;
        if (used) {
            const int yy = y - top;
            const bool inside = resized && yy >= ya && yy < yb;
            int first = 0, n = 0;
            const int* tap = taps_y;
            if (inside) {
                tap = taps_y + (size_t)yy * kTapWords;
                first = max(tap[0], 0);
                n = min(max(tap[1], 0), kMaxKsize);
            }
            // the dword's bytes inside the placed part: columns [c0, c1) of the LDS rows, at bytes j0 .. of the dword
            const int c0 = max(v * 4, xa) - xa, c1 = min(v * 4 + 4, xb) - xa, j0 = max(v * 4, xa) - v * 4;
            int acc[4] = {kHalf, kHalf, kHalf, kHalf};
            if (inside && c0 < c1) {
                for (int k = 0; k < n; ++k) {
                    const int r = first + k - lo;
                    if (r < 0 || r >= nrows) continue;              // (never: the block holds every row its taps name)
                    const int c = tap[3 + k];
                    const unsigned char* q = rows_lds + (size_t)r * (new_w * 3) + c0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (j < c1 - c0) acc[j] += (int)q[j] * c;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int byte = v * 4 + j;
                unsigned value = fill_bytes[byte % 3];
                if (inside && byte >= xa && byte < xb) {
                    const int m = j - j0;                           // 0 .. c1 - c0 - 1
                    value = (unsigned)clip8(m == 0 ? acc[0] : m == 1 ? acc[1] : m == 2 ? acc[2] : acc[3]);
                }
                word |= value << (8 * j);
            }
        }
        out[(size_t)y * row_dwords + v] = word;
    }
}

// the largest tile whose rows at a 16x reduction fit the LDS budget
inline int tile_rows(int H, int W) {
    const int rows = kLdsBytes / (W * 3);
    return std::min(H, std::max(1, (rows - 64) / 16));
}

inline bool shape_ok(int B, int max_boxes, int H, int W) {
    return B >= 1 && B <= 65535 && max_boxes >= 1 && max_boxes <= kMaxBoxes && (long long)B * max_boxes <= kMaxRows &&
           H >= 8 && H <= kMaxH && W >= 8 && W <= kMaxW && H % 8 == 0 && W % 8 == 0;
}

mpn_attr_mask_t g_resize_lds;

}  // namespace

extern "C" size_t mpn_person_crops_desc_bytes(void) { return sizeof(Desc); }

extern "C" size_t mpn_person_crops_info_bytes(int B, int max_boxes) {
    if (B < 1 || max_boxes < 1 || max_boxes > kMaxBoxes || (long long)B * max_boxes > kMaxRows) return 0;
    return (size_t)B * max_boxes * sizeof(Info);
}

extern "C" size_t mpn_person_crops_workspace_bytes(int B, int max_boxes, int H, int W) {
    if (!shape_ok(B, max_boxes, H, W)) return 0;
    return (size_t)B * max_boxes * (size_t)(H + W) * kTapWords * sizeof(int);
}

extern "C" int mpn_person_crops(const uint8_t* sources, size_t sources_bytes, const void* descs, const void* record,
                                size_t record_bytes, int B, int max_boxes, int H, int W, double pad, int fit, int fill,
                                uint8_t* crops_out, void* info_out, void* workspace, size_t workspace_bytes, mpn_stream_t stream) {
    MPN_REQUIRE(sources && descs && record && crops_out && info_out && workspace, MPN_ERR_BAD_ARG, "person_crops: null pointer");
    MPN_REQUIRE(B >= 1 && B <= 65535, MPN_ERR_BAD_SHAPE, "person_crops: B must be in [1, 65535] (got %d)", B);
    MPN_REQUIRE(max_boxes >= 1 && max_boxes <= kMaxBoxes, MPN_ERR_BAD_SHAPE, "person_crops: max_boxes must be in [1, %d] (got %d)",
                kMaxBoxes, max_boxes);
    MPN_REQUIRE((long long)B * max_boxes <= kMaxRows, MPN_ERR_BAD_SHAPE,
                "person_crops: B * max_boxes = %lld rows, mpn_pose_gather's record holds %d", (long long)B * max_boxes, kMaxRows);
    MPN_REQUIRE(H >= 8 && H <= kMaxH && H % 8 == 0, MPN_ERR_BAD_SHAPE, "person_crops: H must be a multiple of 8 in [8, %d] (got %d)",
                kMaxH, H);
    MPN_REQUIRE(W >= 8 && W <= kMaxW && W % 8 == 0, MPN_ERR_BAD_SHAPE, "person_crops: W must be a multiple of 8 in [8, %d] (got %d)",
                kMaxW, W);
    MPN_REQUIRE(std::isfinite(pad) && pad >= 0.0 && pad <= 4.0, MPN_ERR_BAD_ARG, "person_crops: pad must be in [0, 4] (got %g)", pad);
    MPN_REQUIRE(fit == kStretch || fit == kPad, MPN_ERR_BAD_ARG, "person_crops: fit must be 0 (stretch) or 1 (pad) (got %d)", fit);
    MPN_REQUIRE(fill >= 0 && fill <= 0xFFFFFF, MPN_ERR_BAD_ARG, "person_crops: fill must be R | G << 8 | B << 16 (got %d)", fill);
    MPN_REQUIRE(mpn_aligned16(descs) && mpn_aligned16(record) && mpn_aligned16(crops_out) && mpn_aligned16(info_out) &&
                    mpn_aligned16(workspace), MPN_ERR_BAD_ALIGN,
                "person_crops: descs, record, crops_out, info_out and workspace must be 16-byte aligned");
    MPN_REQUIRE(mpn_pose_gather_row_offset(B, max_boxes, 0) == record_header_words(B) * 4 &&
                    mpn_pose_gather_row_offset(B, max_boxes, 1) - mpn_pose_gather_row_offset(B, max_boxes, 0) == kRowWords * 4,
                MPN_ERR_BAD_ARG, "person_crops: the record's layout is not the one this kernel was written against");
    MPN_REQUIRE(record_bytes >= mpn_pose_gather_record_bytes(B, max_boxes), MPN_ERR_WORKSPACE,
                "person_crops: record of %zu bytes, %zu needed", record_bytes, mpn_pose_gather_record_bytes(B, max_boxes));
    MPN_REQUIRE(workspace_bytes >= mpn_person_crops_workspace_bytes(B, max_boxes, H, W), MPN_ERR_WORKSPACE,
                "person_crops: workspace of %zu bytes, %zu needed", workspace_bytes,
                mpn_person_crops_workspace_bytes(B, max_boxes, H, W));
    MPN_REQUIRE(sources_bytes >= 3, MPN_ERR_WORKSPACE, "person_crops: sources of %zu bytes", sources_bytes);

    const Desc* dd = reinterpret_cast<const Desc*>(descs);
    const int* header = reinterpret_cast<const int*>(record);
    const float* rows = reinterpret_cast<const float*>(reinterpret_cast<const char*>(record) + record_header_words(B) * 4);
    const int n = B * max_boxes;
    Info* info = reinterpret_cast<Info*>(info_out);
    int* taps = reinterpret_cast<int*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    crops_taps_kernel<<<dim3((unsigned)mpn_div_up(H + W, kTapThreads), (unsigned)n), kTapThreads, 0, s>>>(
        dd, sources_bytes, header, rows, B, max_boxes, H, W, pad, fit, info, taps);
    MPN_LAUNCH_CHECK();
    const int tile = tile_rows(H, W);
    const int lds_rows = tile * 16 + 64;
    const size_t lds = (size_t)lds_rows * (size_t)W * 3;            // <= kLdsBytes by tile_rows; a multiple of 8
    if (lds > 65536) MPN_HIP(mpn_ensure_dynamic_lds(reinterpret_cast<const void*>(crops_resize_kernel), kLdsBytes, &g_resize_lds));
    crops_resize_kernel<<<dim3((unsigned)mpn_div_up(H, tile), (unsigned)n), kThreads, lds, s>>>(
        sources, sources_bytes, dd, B, H, W, tile, lds_rows, fill, info, taps, crops_out);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
