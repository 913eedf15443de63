// Pillow's `Image.resize` of 8-bit RGB images (default filter: antialiased bicubic) for a batch of RAGGED sources, onto the
// network canvas [B,H,W,3] uint8 - the host step of the reference's inference/predict.ipynb (cell 6) moved into the captured
// inference graph. The host (multiposenet_amd/inference/resample.py) builds Pillow's fixed-point coefficient tables and one
// mpn_image_resize_desc per image; the device does the integer part only, so the output equals Pillow's byte for byte:
//
//   resize_rows_kernel   horizontal pass: source [src_h, src_w, 3] -> intermediate uint8 [src_h, new_w*3 padded to 16 bytes]
//   resize_cols_kernel   vertical pass:   intermediate -> out [H, W, 3], zero outside new_h x new_w (every byte written)
//
// each `clip8((sum_k pixel * coeff + 2^21) >> 22)` in int32 (sum |coeff| * 255 stays below 2^31: the weights are normalised and
// the bicubic's negative lobes add about 0.3 to the sum of magnitudes). A pass between equal sizes is a copy through the same
// code (one tap of weight 2^22), which is what Pillow's skipping it leaves.
//
// Both run inside a hipGraph: grids depend on (B, H, W) alone. The horizontal pass walks its image's src_h * ceil(new_w / 4)
// work items with a grid-stride loop (source sizes come from the descriptor); the vertical pass has one thread per 16 output
// bytes. Bandwidth-shaped:
//   - a source pixel is ONE dword load (3 bytes + 1 of the neighbour, unaligned; the last pixel of an image byte by byte, so
//     only the 1 byte behind the last image of the buffer is ever touched), overlapping taps of neighbouring lanes hit L1;
//   - a thread of the horizontal pass produces 4 pixels = 3 dword stores; the vertical pass is elementwise over the BYTES of a
//     row (every byte of an output row uses the same taps), so it reads the 16-byte-aligned intermediate rows in 16-byte
//     vectors and writes 16-byte vectors;
//   - the horizontal pass runs once per source row (no tile overlap to recompute).
// No descriptor makes a kernel write outside workspace / out: desc_ok() rejects it and the image becomes zeros.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRowBlocks = 1024;        // blocks per image of the horizontal pass (grid-stride over the image's work items)
constexpr int kBits = 22;               // Pillow's PRECISION_BITS
constexpr int kHalf = 1 << (kBits - 1);
constexpr int kOne = 1 << kBits;
constexpr int kMaxKsize = MPN_IMAGE_RESIZE_MAX_KSIZE;

typedef mpn_image_resize_desc Desc;
static_assert(sizeof(Desc) == MPN_IMAGE_RESIZE_DESC_BYTES, "descriptor layout is part of the ABI");

inline size_t round16(size_t n) { return (n + 15) / 16 * 16; }

__device__ __forceinline__ bool desc_ok(const Desc& d, int H, int W, size_t work_bytes) {
    if (d.src_h < 1 || d.src_w < 1 || d.new_h < 1 || d.new_w < 1 || d.new_h > H || d.new_w > W) return false;
    if (d.ksize_x < 1 || d.ksize_y < 1 || d.ksize_x > kMaxKsize || d.ksize_y > kMaxKsize) return false;
    if (d.src_offset < 0 || d.tmp_offset < 0 || (d.tmp_offset & 15) || (d.tmp_stride & 15) || d.tmp_stride < d.new_w * 3) return false;
    if ((long long)d.src_h * ((d.new_w + 3) >> 2) > 0x7fffffffLL) return false;     // the work items are indexed in 32 bits
    return (unsigned long long)d.tmp_offset + (unsigned long long)d.src_h * (unsigned long long)d.tmp_stride <= work_bytes;
}

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> kBits, 0), 255); }

// pixel p of an image as a dword (bits 0..23 = r, g, b)
__device__ __forceinline__ unsigned load_pixel(const uint8_t* __restrict__ img, long long p, long long last) {
    const uint8_t* q = img + p * 3;
    if (p < last) {
        unsigned v;
        __builtin_memcpy(&v, q, 4);
        return v;
    }
    return (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
}

__global__ void __launch_bounds__(kThreads) resize_rows_kernel(const uint8_t* __restrict__ sources, const int32_t* __restrict__ tables,
                                                               const Desc* __restrict__ descs, int H, int W,
                                                               uint8_t* __restrict__ work, size_t work_bytes) {
    const Desc d = descs[blockIdx.y];
    if (!desc_ok(d, H, W, work_bytes)) return;
    const uint8_t* img = sources + d.src_offset;
    uint8_t* tmp = work + d.tmp_offset;
    const int groups = (d.new_w + 3) >> 2;
    const unsigned items = (unsigned)d.src_h * (unsigned)groups;    // < 2^31 (desc_ok)
    const long long last = (long long)d.src_h * d.src_w - 1;
    const bool copy = d.src_w == d.new_w;
    const int32_t* bounds = tables + d.bounds_x;
    const int32_t* coeffs = tables + d.coeffs_x;
    for (unsigned it = blockIdx.x * kThreads + threadIdx.x; it < items; it += gridDim.x * kThreads) {   // (step 2^18: no wrap)
        const int y = (int)(it / (unsigned)groups), g = (int)(it - (unsigned)y * (unsigned)groups);
        const long long row = (long long)y * d.src_w;
        unsigned bytes[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int x = g * 4 + i;
            int r0 = 0, r1 = 0, r2 = 0;
            if (x < d.new_w) {
                int first = x, n = 1;
                const int32_t* c = nullptr;
                if (!copy) {
                    first = max(bounds[2 * x], 0);
                    n = min(min(bounds[2 * x + 1], d.ksize_x), d.src_w - first);
                    c = coeffs + (long long)x * d.ksize_x;
                }
                int a0 = kHalf, a1 = kHalf, a2 = kHalf;
                for (int k = 0; k < n; ++k) {
                    const int w = c ? c[k] : kOne;
                    const unsigned v = load_pixel(img, row + first + k, last);
                    a0 += (int)(v & 255u) * w;
                    a1 += (int)((v >> 8) & 255u) * w;
                    a2 += (int)((v >> 16) & 255u) * w;
                }
                r0 = clip8(a0);
                r1 = clip8(a1);
                r2 = clip8(a2);
            }
            bytes[3 * i] = (unsigned)r0;
            bytes[3 * i + 1] = (unsigned)r1;
            bytes[3 * i + 2] = (unsigned)r2;
        }
        // 3 dwords at byte g*12 of the row; tmp_stride is a multiple of 16 >= new_w*3, so every dword that holds a valid byte
        // lies inside the row and the others are dropped
        unsigned* dst = reinterpret_cast<unsigned*>(tmp + (size_t)y * d.tmp_stride + (size_t)g * 12);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (g * 12 + 4 * j + 4 <= d.tmp_stride)
                dst[j] = bytes[4 * j] | (bytes[4 * j + 1] << 8) | (bytes[4 * j + 2] << 16) | (bytes[4 * j + 3] << 24);
        }
    }
}

__global__ void __launch_bounds__(kThreads) resize_cols_kernel(const int32_t* __restrict__ tables, const Desc* __restrict__ descs,
                                                               int H, int W, const uint8_t* __restrict__ work, size_t work_bytes,
                                                               uint8_t* __restrict__ out) {
    const int b = blockIdx.y;
    const int vecs = W * 3 / 16;
    const unsigned idx = blockIdx.x * kThreads + threadIdx.x;       // H * vecs < 2^31 (H, W <= 65536: the launcher's check)
    if (idx >= (unsigned)H * (unsigned)vecs) return;
    const int y = (int)(idx / (unsigned)vecs), v = (int)(idx - (unsigned)y * (unsigned)vecs);
    const Desc d = descs[b];
    uint4 o = make_uint4(0u, 0u, 0u, 0u);
    if (desc_ok(d, H, W, work_bytes) && y < d.new_h && v * 16 < d.new_w * 3) {
        int first = y, n = 1;
        const int32_t* c = nullptr;
        if (d.src_h != d.new_h) {
            first = max(tables[d.bounds_y + 2 * y], 0);
            n = min(min(tables[d.bounds_y + 2 * y + 1], d.ksize_y), d.src_h - first);
            c = tables + d.coeffs_y + (long long)y * d.ksize_y;
        }
        int acc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = kHalf;
        const uint8_t* col = work + d.tmp_offset + (size_t)first * d.tmp_stride + (size_t)v * 16;
        for (int k = 0; k < n; ++k) {
            const int w = c ? c[k] : kOne;
            const uint4 q = *reinterpret_cast<const uint4*>(col + (size_t)k * d.tmp_stride);
            const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] += (int)((u[j >> 2] >> (8 * (j & 3))) & 255u) * w;
        }
        const int valid = d.new_w * 3 - v * 16;          // bytes of this vector inside the resized image
        unsigned r[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j < valid) r[j >> 2] |= (unsigned)clip8(acc[j]) << (8 * (j & 3));
        }
        o = make_uint4(r[0], r[1], r[2], r[3]);
    }
    *reinterpret_cast<uint4*>(out + (((size_t)b * H + y) * W) * 3 + (size_t)v * 16) = o;
}

}  // namespace

extern "C" size_t mpn_image_resize_desc_bytes(void) { return sizeof(Desc); }

extern "C" size_t mpn_image_resize_workspace_bytes(int B, int H, int W, long long src_rows) {
    if (B < 1 || H < 1 || W < 1 || src_rows < B) return 0;
    return (size_t)src_rows * round16((size_t)W * 3);
}

extern "C" int mpn_image_resize(const uint8_t* sources, const int32_t* tables, const void* descs, int B, int H, int W,
                                uint8_t* out_u8, void* workspace, size_t workspace_bytes, mpn_stream_t stream) {
    MPN_REQUIRE(sources && tables && descs && out_u8 && workspace, MPN_ERR_BAD_ARG, "image_resize: null pointer");
    MPN_REQUIRE(B >= 1 && B <= 65535, MPN_ERR_BAD_SHAPE, "image_resize: B must be in [1, 65535] (got %d)", B);
    MPN_REQUIRE(H >= 1 && W >= 1 && (W * 3LL) % 16 == 0 && H <= 65536 && W <= 65536, MPN_ERR_BAD_SHAPE,
                "image_resize: H, W must be in [1, 65536] and W * 3 a multiple of 16 (got %d x %d)", H, W);
    MPN_REQUIRE(mpn_aligned16(tables) && mpn_aligned16(descs) && mpn_aligned16(out_u8) && mpn_aligned16(workspace), MPN_ERR_BAD_ALIGN,
                "image_resize: tables, descs, out_u8 and workspace must be 16-byte aligned");
    MPN_REQUIRE(workspace_bytes >= 16, MPN_ERR_WORKSPACE, "image_resize: workspace of %zu bytes", workspace_bytes);
    const Desc* dd = reinterpret_cast<const Desc*>(descs);
    resize_rows_kernel<<<dim3(kRowBlocks, (unsigned)B), kThreads, 0, (hipStream_t)stream>>>(
        sources, tables, dd, H, W, reinterpret_cast<uint8_t*>(workspace), workspace_bytes);
    MPN_LAUNCH_CHECK();
    const long long vec_items = (long long)H * (W * 3 / 16);
    resize_cols_kernel<<<dim3((unsigned)mpn_div_up(vec_items, kThreads), (unsigned)B), kThreads, 0, (hipStream_t)stream>>>(
        tables, dd, H, W, reinterpret_cast<const uint8_t*>(workspace), workspace_bytes, out_u8);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
