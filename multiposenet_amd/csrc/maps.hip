// `plot_maps` of the reference's inference/predict.ipynb (the cells under "Show heatmaps") for a batch of frames of one size:
// the frame at half size with each of the 17 keypoint heatmaps and the segmentation mask laid over it, 18 labelled panels
// stacked vertically, [B, 18*h, w, 4] RGBA, equal byte for byte to what Pillow and matplotlib make there. The host
// (multiposenet_amd/inference/maps.py) builds Pillow's fixed-point Lanczos tables, the colormap's 256 entries already
// premultiplied by their alpha, and the label stamps; the device does the integer part:
//
//   frame_rows_kernel   horizontal pass of the frame:  [H, W, 3] -> workspace [H, w4, 4] (RGB + one unused byte)
//   map_rows_kernel     horizontal pass of the 18 overlays: heatmap -> (normalise) -> colormap entry, premultiplied ->
//                       taps -> workspace [hh, 18, w4, 4]; the mask band is stored four times, so that the second pass
//                       treats all 18 alike
//   panels_kernel       per 4 output pixels of a row: vertical taps of the frame (once) and of each overlay, un-premultiply,
//                       alpha_composite over the frame, the label's blend, one 16-byte store per panel
//
// each pass `clip8((sum_k pixel * coeff + 2^21) >> 22)` in int32 through a uint8 intermediate, as Pillow's. w4 = w rounded up
// to 4 pixels, so every workspace row and every 4-pixel group is 16-byte aligned.
//
// Bandwidth-shaped: a few bytes in, 18 x 4 bytes per output pixel out. A block is one wave over one row (frame_rows,
// panels) or one (row, panel) (map_rows): the row's tap window and coefficients, the channel's min / max and the label's
// descriptor are wave-uniform and come through the scalar cache; the colormap lies in LDS. Lanes are neighbouring groups:
// 16-byte loads and stores of a wave are contiguous. Grids depend on (B, H, W, hh, hw) alone.
//
// Nothing read from device memory becomes an address unchecked: tap windows are clamped to the source, a stamp whose
// descriptor leaves the packed pixels is not blended. Where each table lies comes in a HOST descriptor, which the launcher
// checks against the size of the tables.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 64;            // one wave per row segment of 256 output pixels
constexpr int kPanels = MPN_PLOT_MAPS_PANELS;
constexpr int kHeat = kPanels - 1;      // panels 0..16: heatmaps; 17: the mask
constexpr int kBits = 22;               // Pillow's PRECISION_BITS
constexpr int kHalf = 1 << (kBits - 1);
constexpr int kMaxKsize = MPN_IMAGE_RESIZE_MAX_KSIZE;

typedef mpn_plot_maps_desc Desc;
static_assert(sizeof(Desc) == MPN_PLOT_MAPS_DESC_BYTES, "descriptor layout is part of the ABI");

struct Axis {
    int bounds, coeffs, ksize;          // word offsets into the tables, row length of coeffs
};

// the stamp of one label inside the tables: its L8 pixels [sh, sw] at byte `offset` of the packed pixels, blended at
// (ox, panel top + oy)
struct Stamp {
    int offset, sw, sh, ox, oy, reserved[3];
};

// clip8(acc >> 22) without an arithmetic shift: negative sums clip to 0 before the shift
__device__ __forceinline__ int clip8(int acc) { return (int)min((unsigned)max(acc, 0) >> kBits, 255u); }

// Pillow's DIV255 / MULDIV255 rounding: (t + 128 + ((t + 128) >> 8)) >> 8
__device__ __forceinline__ int div255(int t) {
    t += 128;
    return ((t >> 8) + t) >> 8;
}

// mpn_heatmap_minmax's order-preserving key -> float (csrc/prn_post.hip: f2key)
__device__ __forceinline__ float key2f(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// the taps of output i of an axis with in_size inputs: the first tap and the count, clamped to the source whatever the table holds
__device__ __forceinline__ int taps_of(const int32_t* __restrict__ tables, const Axis a, int i, int in_size, int& first,
                                       const int32_t*& c) {
    first = min(max(tables[a.bounds + 2 * i], 0), in_size - 1);
    c = tables + a.coeffs + (long long)i * a.ksize;
    return max(min(min(tables[a.bounds + 2 * i + 1], a.ksize), in_size - first), 0);
}

__device__ __forceinline__ unsigned pack4(int r, int g, int b, int a) {
    return (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16) | ((unsigned)a << 24);
}

// grid (ceil(w4 / 4 / 64), H, B)
__global__ void __launch_bounds__(kThreads) frame_rows_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ tables,
                                                              const Axis ax, int H, int W, int w, int w4,
                                                              uint8_t* __restrict__ work) {
    const int g = blockIdx.x * kThreads + threadIdx.x;
    if (g * 4 >= w4) return;
    const int r = blockIdx.y, b = blockIdx.z;
    const uint8_t* row = frames + ((size_t)b * H + r) * (size_t)W * 3;
    unsigned px[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = g * 4 + i;
        px[i] = 0u;
        if (x < w) {
            int first;
            const int32_t* c;
            const int n = taps_of(tables, ax, x, W, first, c);
            int a0 = kHalf, a1 = kHalf, a2 = kHalf;
            const uint8_t* p = row + (size_t)first * 3;
            for (int k = 0; k < n; ++k) {
                const int cw = c[k];
                a0 += (int)p[3 * k] * cw;
                a1 += (int)p[3 * k + 1] * cw;
                a2 += (int)p[3 * k + 2] * cw;
            }
            px[i] = pack4(clip8(a0), clip8(a1), clip8(a2), 255);
        }
    }
    *reinterpret_cast<uint4*>(work + (((size_t)b * H + r) * w4 + (size_t)g * 4) * 4) = make_uint4(px[0], px[1], px[2], px[3]);
}

// grid (ceil(w4 / 4 / 64), hh * 18, B)
__global__ void __launch_bounds__(kThreads) map_rows_kernel(const float* __restrict__ heat, const float* __restrict__ mask,
                                                            const unsigned* __restrict__ keys, const int32_t* __restrict__ tables,
                                                            const Axis ax, int lut_at, int hh, int hw, int w, int w4,
                                                            uint8_t* __restrict__ work) {
    __shared__ unsigned lut[256];
    for (int i = threadIdx.x; i < 256; i += kThreads) lut[i] = (unsigned)tables[lut_at + i];
    __syncthreads();
    const int g = blockIdx.x * kThreads + threadIdx.x;
    if (g * 4 >= w4) return;
    const int r = blockIdx.y / kPanels, j = blockIdx.y - r * kPanels, b = blockIdx.z;
    float lo = 0.f, range = 1.f;
    const bool normalise = keys != nullptr && j < kHeat;
    if (normalise) {
        lo = key2f(keys[((size_t)b * kHeat + j) * 2]);
        range = key2f(keys[((size_t)b * kHeat + j) * 2 + 1]) - lo;
    }
    const size_t row = ((size_t)b * hh + r) * (size_t)hw;
    unsigned px[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = g * 4 + i;
        px[i] = 0u;
        if (x < w) {
            int first;
            const int32_t* c;
            const int n = taps_of(tables, ax, x, hw, first, c);
            int a0 = kHalf, a1 = kHalf, a2 = kHalf, a3 = kHalf;
            for (int k = 0; k < n; ++k) {
                unsigned p;
                if (j < kHeat) {
                    float v = heat[(row + first + k) * kHeat + j];
                    if (normalise) v = __fdiv_rn(v - lo, range);     // (x - m) / (M - m) in f32, correctly rounded; 0 / 0 = NaN
                    const float t = v * 256.f;                       // exact
                    // matplotlib's lookup: NaN -> transparent; below 0 the first entry; x == 1 and above the last; else trunc
                    p = (t != t) ? 0u : lut[t < 0.f ? 0 : (t >= 256.f ? 255 : (int)t)];
                } else {
                    const float v = mask ? mask[row + first + k] : 0.f;
                    p = (unsigned)(int)(255.f * fminf(fmaxf(v, 0.f), 1.f)) * 0x01010101u;   // clip, * 255 in f32, truncate
                }
                const int cw = c[k];
                a0 += (int)(p & 255u) * cw;
                a1 += (int)((p >> 8) & 255u) * cw;
                a2 += (int)((p >> 16) & 255u) * cw;
                a3 += (int)(p >> 24) * cw;
            }
            px[i] = pack4(clip8(a0), clip8(a1), clip8(a2), clip8(a3));
        }
    }
    *reinterpret_cast<uint4*>(work + ((((size_t)b * hh + r) * kPanels + j) * w4 + (size_t)g * 4) * 4) =
        make_uint4(px[0], px[1], px[2], px[3]);
}

// grid (ceil(w4 / 4 / 64), h, B)
__global__ void __launch_bounds__(kThreads) panels_kernel(const int32_t* __restrict__ tables, const Axis fy, const Axis my,
                                                          int stamps_at, int pixels_at, int pixel_bytes, int H, int hh, int h,
                                                          int w, int w4, const uint8_t* __restrict__ frame_rows,
                                                          const uint8_t* __restrict__ map_rows, uint8_t* __restrict__ out) {
    const int g = blockIdx.x * kThreads + threadIdx.x;
    if (g * 4 >= w4) return;
    const int y = blockIdx.y, b = blockIdx.z;
    int first;
    const int32_t* c;
    // the frame's 4 pixels at (y, 4g ..)
    int bg[4][3];
    {
        const int n = taps_of(tables, fy, y, H, first, c);
        int acc[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] = kHalf;
        const uint8_t* col = frame_rows + (((size_t)b * H + first) * w4 + (size_t)g * 4) * 4;
        for (int k = 0; k < n; ++k) {
            const int cw = c[k];
            const uint4 q = *reinterpret_cast<const uint4*>(col + (size_t)k * w4 * 4);
            const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc[3 * i] += (int)(u[i] & 255u) * cw;
                acc[3 * i + 1] += (int)((u[i] >> 8) & 255u) * cw;
                acc[3 * i + 2] += (int)((u[i] >> 16) & 255u) * cw;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bg[i][0] = clip8(acc[3 * i]);
            bg[i][1] = clip8(acc[3 * i + 1]);
            bg[i][2] = clip8(acc[3 * i + 2]);
        }
    }
    const int n = taps_of(tables, my, y, hh, first, c);
    const Stamp* stamps = reinterpret_cast<const Stamp*>(tables + stamps_at);
    const uint8_t* pixels = reinterpret_cast<const uint8_t*>(tables + pixels_at);
    const bool vec = (w & 3) == 0;                                      // rows of the output are 16-byte aligned
    for (int j = 0; j < kPanels; ++j) {
        int acc[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = kHalf;
        const uint8_t* col = map_rows + ((((size_t)b * hh + first) * kPanels + j) * w4 + (size_t)g * 4) * 4;
        for (int k = 0; k < n; ++k) {
            const int cw = c[k];
            const uint4 q = *reinterpret_cast<const uint4*>(col + (size_t)k * kPanels * w4 * 4);
            const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] += (int)((u[i >> 2] >> (8 * (i & 3))) & 255u) * cw;
        }
        // the label of this panel, clipped to the panel (the notebook's next paste covers what leaves it, the picture's
        // edge clips the last)
        const Stamp st = stamps[j];
        const int sy = y - st.oy;
        const bool stamp_row = st.sw > 0 && st.sh > 0 && st.offset >= 0 && (long long)st.offset + (long long)st.sw * st.sh <= pixel_bytes &&
                               sy >= 0 && sy < st.sh;
        unsigned res[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int r = clip8(acc[4 * i]), gg = clip8(acc[4 * i + 1]), bb = clip8(acc[4 * i + 2]);
            const int a = clip8(acc[4 * i + 3]);
            if (j < kHeat && a != 0 && a != 255) {
                // Pillow's RGBa -> RGBA: clip8(255 * c / a) in integers. 255 * c <= 65025 and a <= 254: the correctly rounded
                // f32 quotient lies within 65025 * 2^-24 < 1 / 254 of the true one, so its truncation is the integer quotient
                const float fa = (float)a;
                r = min((int)__fdiv_rn((float)(255 * r), fa), 255);
                gg = min((int)__fdiv_rn((float)(255 * gg), fa), 255);
                bb = min((int)__fdiv_rn((float)(255 * bb), fa), 255);
            }
            // Image.alpha_composite(frame, overlay) with the frame's alpha 255 (AlphaComposite.c): outa255 = 255 * 255, so
            // coef1 = a * 255 * 255 * 128 / outa255 = a * 128 exactly, and the result's alpha is 255
            int o0 = bg[i][0], o1 = bg[i][1], o2 = bg[i][2], o3 = 255;
            if (a != 0) {
                const int c1 = a * 128, c2 = 255 * 128 - c1;
                int t = r * c1 + o0 * c2 + (0x80 << 7);
                o0 = (((t >> 8) + t) >> 8) >> 7;
                t = gg * c1 + o1 * c2 + (0x80 << 7);
                o1 = (((t >> 8) + t) >> 8) >> 7;
                t = bb * c1 + o2 * c2 + (0x80 << 7);
                o2 = (((t >> 8) + t) >> 8) >> 7;
            }
            const int sx = g * 4 + i - st.ox;
            if (stamp_row && sx >= 0 && sx < st.sw) {
                // ImageDraw.text on an RGBA image: BLEND8 of the ink (255, 0, 0, 255) on all four bands
                const int m = pixels[st.offset + sy * st.sw + sx];
                o0 = div255(o0 * (255 - m) + 255 * m);
                o1 = div255(o1 * (255 - m));
                o2 = div255(o2 * (255 - m));
                o3 = div255(o3 * (255 - m) + 255 * m);
            }
            res[i] = pack4(o0, o1, o2, o3);
        }
        uint8_t* dst = out + ((((size_t)b * kPanels + j) * h + y) * w + (size_t)g * 4) * 4;
        if (vec) {
            *reinterpret_cast<uint4*>(dst) = make_uint4(res[0], res[1], res[2], res[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (g * 4 + i < w) reinterpret_cast<unsigned*>(dst)[i] = res[i];
            }
        }
    }
}

inline long long round4(long long n) { return (n + 3) / 4 * 4; }

inline bool shape_ok(int B, int H, int W, int hh, int hw) {
    // grid limits: B, H and hh * 18 are grid dimensions y / z
    return B >= 1 && B <= 65535 && H >= 2 && H <= 65535 && W >= 2 && W <= 65536 && hh >= 1 && hh * (long long)kPanels <= 65535 &&
           hw >= 1 && hw <= 65536;
}

// an axis of the host descriptor against the size of the tables: bounds [out, 2] and coeffs [out, ksize] lie inside
inline bool axis_ok(int bounds, int coeffs, int ksize, int out, size_t words) {
    if (bounds < 0 || coeffs < 0 || ksize < 1 || ksize > kMaxKsize) return false;
    return (unsigned long long)bounds + 2ull * out <= words && (unsigned long long)coeffs + (unsigned long long)out * ksize <= words;
}

}  // namespace

extern "C" size_t mpn_plot_maps_desc_bytes(void) { return sizeof(Desc); }

extern "C" size_t mpn_plot_maps_workspace_bytes(int B, int H, int W, int hh, int hw) {
    if (!shape_ok(B, H, W, hh, hw)) return 0;
    return (size_t)B * (size_t)round4(W / 2) * 4 * ((size_t)H + (size_t)kPanels * hh);
}

extern "C" int mpn_plot_maps(const uint8_t* frames, const float* heatmaps, const float* mask, const void* minmax_keys,
                             const int32_t* tables, size_t table_words, const void* desc, int B, int H, int W, int hh, int hw,
                             uint8_t* out_rgba, void* workspace, size_t workspace_bytes, mpn_stream_t stream) {
    MPN_REQUIRE(frames && heatmaps && tables && desc && out_rgba && workspace, MPN_ERR_BAD_ARG, "plot_maps: null pointer");
    MPN_REQUIRE(shape_ok(B, H, W, hh, hw), MPN_ERR_BAD_SHAPE,
                "plot_maps: B, H in [1, 65535] (H >= 2), W in [2, 65536], hh in [1, 3640], hw in [1, 65536] (got %d x %d x %d, %d x %d)",
                B, H, W, hh, hw);
    MPN_REQUIRE(mpn_aligned16(tables) && mpn_aligned16(out_rgba) && mpn_aligned16(workspace), MPN_ERR_BAD_ALIGN,
                "plot_maps: tables, out_rgba and workspace must be 16-byte aligned");
    const size_t need = mpn_plot_maps_workspace_bytes(B, H, W, hh, hw);
    MPN_REQUIRE(workspace_bytes >= need, MPN_ERR_WORKSPACE, "plot_maps: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const Desc d = *reinterpret_cast<const Desc*>(desc);
    const int h = H / 2, w = W / 2, w4 = (int)round4(w);
    MPN_REQUIRE(axis_ok(d.bounds_fx, d.coeffs_fx, d.ksize_fx, w, table_words) && axis_ok(d.bounds_fy, d.coeffs_fy, d.ksize_fy, h, table_words) &&
                    axis_ok(d.bounds_mx, d.coeffs_mx, d.ksize_mx, w, table_words) && axis_ok(d.bounds_my, d.coeffs_my, d.ksize_my, h, table_words),
                MPN_ERR_BAD_ARG, "plot_maps: a coefficient table of the descriptor leaves the %zu words of tables (or has more than %d taps)",
                table_words, kMaxKsize);
    MPN_REQUIRE(d.lut >= 0 && (size_t)d.lut + 256 <= table_words && d.stamps >= 0 && (d.stamps & 3) == 0 &&
                    (size_t)d.stamps + kPanels * sizeof(Stamp) / 4 <= table_words && d.stamp_pixels >= 0 && d.stamp_bytes >= 0 &&
                    (size_t)d.stamp_pixels + ((size_t)d.stamp_bytes + 3) / 4 <= table_words,
                MPN_ERR_BAD_ARG, "plot_maps: the colour table or the stamps of the descriptor leave the %zu words of tables", table_words);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* frame_rows = reinterpret_cast<uint8_t*>(workspace);
    uint8_t* map_rows = frame_rows + (size_t)B * H * w4 * 4;
    const unsigned gx = (unsigned)mpn_div_up(w4 / 4, kThreads);
    frame_rows_kernel<<<dim3(gx, (unsigned)H, (unsigned)B), kThreads, 0, st>>>(frames, tables, Axis{d.bounds_fx, d.coeffs_fx, d.ksize_fx},
                                                                             H, W, w, w4, frame_rows);
    MPN_LAUNCH_CHECK();
    map_rows_kernel<<<dim3(gx, (unsigned)(hh * kPanels), (unsigned)B), kThreads, 0, st>>>(
        heatmaps, mask, reinterpret_cast<const unsigned*>(minmax_keys), tables, Axis{d.bounds_mx, d.coeffs_mx, d.ksize_mx}, d.lut, hh, hw,
        w, w4, map_rows);
    MPN_LAUNCH_CHECK();
    panels_kernel<<<dim3(gx, (unsigned)h, (unsigned)B), kThreads, 0, st>>>(
        tables, Axis{d.bounds_fy, d.coeffs_fy, d.ksize_fy}, Axis{d.bounds_my, d.coeffs_my, d.ksize_my}, d.stamps, d.stamp_pixels,
        d.stamp_bytes, H, hh, h, w, w4, frame_rows, map_rows, out_rgba);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
