// Test-time augmentation of the joint inference graph: the averaged heatmaps never leave the device.
//   mpn_mirror_images   uint8 [n,h,w,3] -> the same images mirrored left to right: the second half of a 2b network input
//                       from its first half.
//   mpn_tta_merge       up to MPN_TTA_MAX_SOURCES (heatmaps, mask) pairs of the SAME b images - the plain pass, the pass over
//                       the mirrored input, passes at other input sizes - un-mirrored, resized to the first size and averaged,
//                       in ONE launch: one thread per output value, the sources by value in the kernel's arguments.
// Both are memory-bound glue. The merge is a DEFINITION, not an approximation (include/mpn.h states it, tests/tta_ref.py is
// its numpy transcription): every operation is one separately rounded IEEE f32 operation in the documented order. That is
// what plain operators are under the pragma below, and ONLY they: HIP's __fmul_rn / __fadd_rn / __fsub_rn are inline
// functions of the runtime's headers, compiled with hipcc's default contraction wherever they are inlined - written with them,
// the multiply and the subtraction of `axis` and both halves of `lerp` came out as v_fma_f32 / v_fmac_f32. With operators the
// only fused instructions left in the kernel are those inside the correctly rounded division sequences (v_div_scale ..
// v_div_fixup).
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kK = 17;                  // heatmap channels; channel kK of the merge's index space is the mask

// keypoint_augment.FLIP_ORDER: the nose stays, every left / right pair swaps (flip_part of prn_examples.hip)
__device__ __forceinline__ int flip_part(int c) { return c == 0 ? 0 : ((c & 1) ? c + 1 : c - 1); }

// ---------------------------------------------------------------- mirror
// one thread per pixel: any width
__global__ __launch_bounds__(kThreads) void mirror_pixels_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                 long long rows, int w) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= rows * w) return;
    const long long row = i / w;
    const int x = (int)(i - row * w);
    const uint8_t* s = in + (row * w + (w - 1 - x)) * 3;
    uint8_t* d = out + i * 3;
    d[0] = s[0];
    d[1] = s[1];
    d[2] = s[2];
}

// w a multiple of 4 (every row then starts on a dword in both buffers): one thread per 4 pixels = 3 dwords in, the pixels
// reversed in registers, 3 dwords out
__global__ __launch_bounds__(kThreads) void mirror_quads_kernel(const unsigned* __restrict__ in, unsigned* __restrict__ out,
                                                                long long rows, int quads) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= rows * quads) return;
    const long long row = i / quads;
    const int q = (int)(i - row * quads);
    const unsigned* s = in + (row * quads + (quads - 1 - q)) * 3;
    const unsigned a = s[0], b = s[1], c = s[2];        // bytes i0..i11 = pixels P0 P1 P2 P3; out = P3 P2 P1 P0
    unsigned* d = out + i * 3;
    d[0] = (c >> 8) | ((b & 0x00ff0000u) << 8);                                         // i9 i10 i11 i6
    d[1] = (b >> 24) | ((c & 0xffu) << 8) | ((a >> 24) << 16) | ((b & 0xffu) << 24);    // i7 i8 i3 i4
    d[2] = ((b >> 8) & 0xffu) | (a << 8);                                               // i5 i0 i1 i2
}

// ---------------------------------------------------------------- merge
struct MergeArgs {
    mpn_tta_source src[MPN_TTA_MAX_SOURCES];
    float* heat_out;
    float* seg_out;
    int num_sources, h0, w0;
    long long total;                    // b * h0 * w0 * (kK + 1)
};

// the source coordinate of output index i along an axis of n_out outputs over n_in inputs: half-pixel centres, clamped edges
__device__ __forceinline__ void axis(int i, int n_in, int n_out, int& i0, int& i1, float& f) {
    const float scale = (float)n_in / (float)n_out;
    float s = ((float)i + 0.5f) * scale - 0.5f;
    s = fminf(fmaxf(s, 0.0f), (float)(n_in - 1));
    i0 = (int)s;                        // s >= 0: the truncation is floor
    i1 = min(i0 + 1, n_in - 1);
    f = s - (float)i0;
}

__device__ __forceinline__ float lerp(float a, float b, float f) { return a + (b - a) * f; }

__global__ __launch_bounds__(kThreads) void tta_merge_kernel(MergeArgs a) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.total) return;
    const int c = (int)(i % (kK + 1));
    const long long pix = i / (kK + 1);
    const int x = (int)(pix % a.w0);
    const int y = (int)((pix / a.w0) % a.h0);
    const long long img = pix / ((long long)a.w0 * a.h0);
    float sum = 0.0f;
    for (int k = 0; k < a.num_sources; ++k) {
        const mpn_tta_source& s = a.src[k];
        const int hk = s.h, wk = s.w;
        const bool mirrored = s.mirrored != 0;
        // element (yy, xx) of the UN-MIRRORED map of this channel: the column flip and the channel swap go to the index
        const float* base;
        int stride;
        if (c < kK) {
            base = s.heat + img * hk * wk * kK + (mirrored ? flip_part(c) : c);
            stride = kK;
        } else {
            base = s.seg + img * hk * wk;
            stride = 1;
        }
        auto at = [&](int yy, int xx) { return base[((long long)yy * wk + (mirrored ? wk - 1 - xx : xx)) * stride]; };
        float v;
        if (hk == a.h0 && wk == a.w0) {
            v = at(y, x);
        } else {
            int y0, y1, x0, x1;
            float fy, fx;
            axis(y, hk, a.h0, y0, y1, fy);
            axis(x, wk, a.w0, x0, x1, fx);
            const float top = lerp(at(y0, x0), at(y0, x1), fx);
            const float bot = lerp(at(y1, x0), at(y1, x1), fx);
            v = lerp(top, bot, fy);
        }
        sum = k == 0 ? v : sum + v;                     // left to right, from the first value (no zero to add it to)
    }
    const float r = sum / (float)a.num_sources;
    if (c < kK) a.heat_out[pix * kK + c] = r;
    else a.seg_out[pix] = r;
}

}  // namespace

extern "C" int mpn_mirror_images(const uint8_t* in, int n, int h, int w, uint8_t* out, mpn_stream_t stream) {
    MPN_REQUIRE(in && out, MPN_ERR_BAD_ARG, "mirror_images: null pointer");
    MPN_REQUIRE(in != out, MPN_ERR_BAD_ARG, "mirror_images: in and out must be different buffers");
    MPN_REQUIRE(n >= 1 && h >= 1 && w >= 1, MPN_ERR_BAD_SHAPE, "mirror_images: bad shape %d x %d x %d", n, h, w);
    const long long rows = (long long)n * h;
    MPN_REQUIRE(rows * w <= 0x7fffffffll, MPN_ERR_BAD_SHAPE, "mirror_images: %lld pixels, the grid covers 2^31 - 1", rows * w);
    if (w % 4 == 0 && (((uintptr_t)in | (uintptr_t)out) & 3u) == 0) {
        const int quads = w / 4;
        mirror_quads_kernel<<<mpn_div_up(rows * quads, kThreads), kThreads, 0, (hipStream_t)stream>>>(
            (const unsigned*)in, (unsigned*)out, rows, quads);
    } else {
        mirror_pixels_kernel<<<mpn_div_up(rows * w, kThreads), kThreads, 0, (hipStream_t)stream>>>(in, out, rows, w);
    }
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}

extern "C" int mpn_tta_merge(const mpn_tta_source* sources, int num_sources, int B, int h0, int w0, float* heat_out,
                             float* seg_out, mpn_stream_t stream) {
    MPN_REQUIRE(sources && heat_out && seg_out, MPN_ERR_BAD_ARG, "tta_merge: null pointer");
    MPN_REQUIRE(num_sources >= 1 && num_sources <= MPN_TTA_MAX_SOURCES, MPN_ERR_BAD_ARG,
                "tta_merge: %d sources, 1 .. %d are taken", num_sources, MPN_TTA_MAX_SOURCES);
    MPN_REQUIRE(B >= 1 && h0 >= 1 && w0 >= 1, MPN_ERR_BAD_SHAPE, "tta_merge: bad shape %d x %d x %d", B, h0, w0);
    MergeArgs a = {};
    a.total = (long long)B * h0 * w0 * (kK + 1);
    MPN_REQUIRE(a.total <= 0x7fffffffll, MPN_ERR_BAD_SHAPE, "tta_merge: %lld output values, the grid covers 2^31 - 1", a.total);
    for (int k = 0; k < num_sources; ++k) {
        const mpn_tta_source& s = sources[k];
        MPN_REQUIRE(s.heat && s.seg, MPN_ERR_BAD_ARG, "tta_merge: source %d has a null pointer", k);
        MPN_REQUIRE(s.h >= 1 && s.w >= 1 && (long long)B * s.h * s.w * kK <= 0x7fffffffll, MPN_ERR_BAD_SHAPE,
                    "tta_merge: source %d is %d x %d x %d", k, B, s.h, s.w);
        MPN_REQUIRE(s.heat != heat_out && s.seg != seg_out, MPN_ERR_BAD_ARG, "tta_merge: source %d is the output", k);
        a.src[k] = s;
    }
    a.heat_out = heat_out;
    a.seg_out = seg_out;
    a.num_sources = num_sources;
    a.h0 = h0;
    a.w0 = w0;
    tta_merge_kernel<<<mpn_div_up(a.total, kThreads), kThreads, 0, (hipStream_t)stream>>>(a);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
