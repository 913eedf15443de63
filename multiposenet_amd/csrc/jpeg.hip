// The device half of the JPEG decode: the host front end (jpeg_host.hip, plain C++) turns a file into raw int16 coefficients,
// 64 per 8x8 block in natural order, one plane of blocks per component, and a fixed-size descriptor; the kernels here turn
// those into pixels equal byte for byte to what libjpeg(-turbo) - and so Pillow - returns for the same bytes.
//
//   mpn_jpeg_decode          jpeg_idct_kernel    dequantise + 8x8 inverse DCT -> uint8 component planes in `work`
//                            jpeg_colour_kernel  "fancy" chroma upsampling + YCbCr->RGB -> packed HWC uint8 at src_offset
//                            (four components - Adobe CMYK - : four planes, and Pillow's inversion and CMYK->RGB in place of
//                            YCbCr->RGB)
//
// The arithmetic is libjpeg's, all integer:
//   - inverse DCT: the "slow integer" method (13-bit constants, 2 extra bits after pass 1, COLUMNS first, then rows),
//     descale = (x + 2^(n-1)) >> n, +128 and the range limit through the 10-bit index of the library's table;
//   - chroma: the triangle filter of h2v1 / h2v2 "fancy" upsampling with its alternating rounding constants, edges taken at
//     the component's TRUE down-sampled size; a component of width <= 2 is replicated (the library's own rule);
//   - colour: the 16-bit fixed-point YCbCr->RGB tables with their rounding terms.
#include "common.h"

namespace {

typedef mpn_jpeg_desc Desc;
static_assert(sizeof(Desc) == MPN_JPEG_DESC_BYTES, "descriptor layout is part of the ABI");

constexpr long long kMaxPixels = 1ll << 28;    // keeps every index of an image in 32 bits (a descriptor is checked on its own)

// ------------------------------------------------------------------------------------------------ device
struct DevGeometry {
    int ncomp, hs, vs, total;
    int bw[4], bh[4], base[4];  // (base[c] = total for a component the image does not have)
    int cw, ch;                 // true size of a chroma component
};

// The geometry of a descriptor, recomputed from (width, height, components, sampling) alone, and every range it makes the
// kernels touch: false = the image is skipped.
__device__ __forceinline__ bool dev_geometry(const Desc& d, DevGeometry& g, size_t coef_bytes, size_t work_bytes, size_t sources_bytes) {
    if (d.width < 1 || d.height < 1 || d.width > 65535 || d.height > 65535 || (long long)d.width * d.height > kMaxPixels) return false;
    if (d.components != 1 && d.components != 3 && d.components != 4) return false;
    const bool samp_ok = (d.h_samp == 1 && d.v_samp == 1) || (d.components == 3 && d.h_samp == 2 && (d.v_samp == 1 || d.v_samp == 2));
    if (!samp_ok) return false;
    if (d.components == 4 && (d.quant3 < 0 || d.quant3 > 2)) return false;      // the table the fourth component shares
    g.ncomp = d.components;
    g.hs = d.h_samp;
    g.vs = d.v_samp;
    const int mx = (d.width + 8 * g.hs - 1) / (8 * g.hs), my = (d.height + 8 * g.vs - 1) / (8 * g.vs);
    g.bw[0] = mx * g.hs;
    g.bh[0] = my * g.vs;
    g.base[0] = 0;
    g.base[1] = g.bw[0] * g.bh[0];
    g.bw[1] = g.bw[2] = g.ncomp >= 3 ? mx : 0;
    g.bh[1] = g.bh[2] = g.ncomp >= 3 ? my : 0;
    g.bw[3] = g.ncomp == 4 ? mx : 0;
    g.bh[3] = g.ncomp == 4 ? my : 0;
    g.base[2] = g.base[1] + g.bw[1] * g.bh[1];
    g.base[3] = g.base[2] + g.bw[2] * g.bh[2];
    g.total = g.base[3] + g.bw[3] * g.bh[3];
    g.cw = (d.width + g.hs - 1) / g.hs;
    g.ch = (d.height + g.vs - 1) / g.vs;
    if (d.src_offset < 0 || d.coef_offset < 0 || d.work_offset < 0 || ((d.src_offset | d.coef_offset | d.work_offset) & 15)) return false;
    if ((unsigned long long)d.coef_offset + (unsigned long long)g.total * 128ull > coef_bytes) return false;
    if ((unsigned long long)d.work_offset + (unsigned long long)g.total * 64ull > work_bytes) return false;
    return (unsigned long long)d.src_offset + (unsigned long long)d.width * d.height * 3ull <= sources_bytes;
}

// One pass of the slow-integer inverse DCT over 8 values (jidctint.c): CONST_BITS = 13.
__device__ __forceinline__ void idct8(const int (&in)[8], int (&out)[8], int shift) {
    const int round = 1 << (shift - 1);
    int z2 = in[2], z3 = in[6];
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 + z3 * (-15137);
    int tmp3 = z1 + z2 * 6270;
    z2 = in[0];
    z3 = in[4];
    int tmp0 = (z2 + z3) * 8192;
    int tmp1 = (z2 - z3) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7];
    tmp1 = in[5];
    tmp2 = in[3];
    tmp3 = in[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446;
    tmp1 *= 16819;
    tmp2 *= 25172;
    tmp3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 *= -16069;
    z4 *= -3196;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    out[0] = (tmp10 + tmp3 + round) >> shift;
    out[7] = (tmp10 - tmp3 + round) >> shift;
    out[1] = (tmp11 + tmp2 + round) >> shift;
    out[6] = (tmp11 - tmp2 + round) >> shift;
    out[2] = (tmp12 + tmp1 + round) >> shift;
    out[5] = (tmp12 - tmp1 + round) >> shift;
    out[3] = (tmp13 + tmp0 + round) >> shift;
    out[4] = (tmp13 - tmp0 + round) >> shift;
}

// +128 and the library's range-limit table, which is indexed with the low 10 bits: a sign-extended 10-bit value, clamped
__device__ __forceinline__ unsigned range_limit(int v) {
    const int s = ((v & 1023) ^ 512) - 512;
    return (unsigned)min(max(s + 128, 0), 255);
}

constexpr int kThreads = 256;
constexpr int kSlots = kThreads / 8;        // 8x8 blocks of a workgroup: eight lanes each
constexpr int kIdctGroups = 128;            // workgroups per image (grid-stride over the image's blocks)
constexpr int kColourGroups = 256;

// Eight lanes per 8x8 block: lane r loads coefficient row r (16 bytes) and dequantises it; rows meet columns through LDS
// (lane c runs pass 1 on column c and writes it back in place), then lane r runs pass 2 on row r and stores 8 bytes.
__global__ void __launch_bounds__(kThreads) jpeg_idct_kernel(const int16_t* __restrict__ coefs, size_t coef_bytes,
                                                             const Desc* __restrict__ descs, uint8_t* __restrict__ work,
                                                             size_t work_bytes, size_t sources_bytes) {
    __shared__ int tile[kSlots][8][9];
    const Desc& d = descs[blockIdx.y];
    DevGeometry g;
    if (!dev_geometry(d, g, coef_bytes, work_bytes, sources_bytes)) return;      // (uniform over the workgroup)
    const int lane = threadIdx.x & 7, slot = threadIdx.x >> 3;
    const int16_t* src = coefs + d.coef_offset / 2;
    uint8_t* planes = work + d.work_offset;
    for (int first = blockIdx.x * kSlots; first < g.total; first += gridDim.x * kSlots) {       // (uniform trip count)
        const int blk = first + slot;
        const bool on = blk < g.total;
        const int c = !on ? 0 : blk >= g.base[3] ? 3 : blk >= g.base[2] ? 2 : blk >= g.base[1] ? 1 : 0;     // (a missing component's base = total)
        const int qc = c == 3 ? d.quant3 : c;
        int v[8], o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = 0;
        if (on) {
            const uint4 cq = *reinterpret_cast<const uint4*>(src + (size_t)blk * 64 + lane * 8);
            const uint4 qq = *reinterpret_cast<const uint4*>(&d.quant[qc][lane * 8]);
            const unsigned cu[4] = {cq.x, cq.y, cq.z, cq.w}, qu[4] = {qq.x, qq.y, qq.z, qq.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[2 * i] = (int)(short)(cu[i] & 0xffffu) * (int)(qu[i] & 0xffffu);
                v[2 * i + 1] = (int)(short)(cu[i] >> 16) * (int)(qu[i] >> 16);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[slot][lane][i] = v[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = tile[slot][i][lane];
        idct8(v, o, 11);                                        // CONST_BITS - PASS1_BITS
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[slot][i][lane] = o[i];  // (the elements this lane read: no hazard)
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = tile[slot][lane][i];
        idct8(v, o, 18);                                        // CONST_BITS + PASS1_BITS + 3
        if (on) {
            const int bi = blk - g.base[c], by = bi / g.bw[c], bx = bi - by * g.bw[c];
            uint2 px;
            px.x = range_limit(o[0]) | (range_limit(o[1]) << 8) | (range_limit(o[2]) << 16) | (range_limit(o[3]) << 24);
            px.y = range_limit(o[4]) | (range_limit(o[5]) << 8) | (range_limit(o[6]) << 16) | (range_limit(o[7]) << 24);
            // plane c: rows of bw*8 bytes at block base[c] * 64 (work_offset is a multiple of 16: the store is aligned)
            *reinterpret_cast<uint2*>(planes + (size_t)g.base[c] * 64 + ((size_t)(by * 8 + lane) * g.bw[c] + bx) * 8) = px;
        }
        // the next iteration writes row `lane`, which only this lane reads above: no barrier needed here
    }
}

// chroma sample of pixel (x, y): libjpeg's fancy upsampling of one component plane (stride in bytes)
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ plane, int stride, const DevGeometry& g, int x, int y) {
    if (g.hs == 1) return plane[(size_t)y * stride + x];
    const int i = x >> 1;
    if (g.cw <= 2) return plane[(size_t)(g.vs == 2 ? y >> 1 : y) * stride + i];       // replicated (the library's rule)
    const int left = max(i - 1, 0), right = min(i + 1, g.cw - 1);
    const int nb = (x & 1) ? right : left;
    if (g.vs == 1) {
        const uint8_t* row = plane + (size_t)y * stride;
        return nb == i ? row[i] : (3 * row[i] + row[nb] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int r = y >> 1;
    const int rn = (y & 1) ? min(r + 1, g.ch - 1) : max(r - 1, 0);
    const uint8_t* row0 = plane + (size_t)r * stride;
    const uint8_t* row1 = plane + (size_t)rn * stride;
    const int here = 3 * row0[i] + row1[i], there = 3 * row0[nb] + row1[nb];
    return (3 * here + there + ((x & 1) ? 7 : 8)) >> 4;
}

__device__ __forceinline__ unsigned clip255(int v) { return (unsigned)min(max(v, 0), 255); }

// Pillow's MULDIV255: a * b / 255, rounded, for a, b in 0..255
__device__ __forceinline__ int muldiv255(int a, int b) {
    const int t = a * b + 128;
    return ((t >> 8) + t) >> 8;
}

// One thread per 4 consecutive pixels of the packed image = 12 bytes = three aligned dword stores (src_offset is a multiple
// of 16); the last, partial group of an image is stored byte by byte so that nothing behind the image is touched.
__global__ void __launch_bounds__(kThreads) jpeg_colour_kernel(const Desc* __restrict__ descs, const uint8_t* __restrict__ work,
                                                               size_t coef_bytes, size_t work_bytes,
                                                               uint8_t* __restrict__ sources, size_t sources_bytes) {
    const Desc& d = descs[blockIdx.y];
    DevGeometry g;
    if (!dev_geometry(d, g, coef_bytes, work_bytes, sources_bytes)) return;
    const int w = d.width;
    const unsigned npix = (unsigned)w * (unsigned)d.height, groups = (npix + 3u) >> 2;
    const uint8_t* yp = work + d.work_offset;
    const uint8_t* cbp = yp + (size_t)g.base[1] * 64;
    const uint8_t* crp = yp + (size_t)g.base[2] * 64;
    const uint8_t* kp = yp + (size_t)g.base[3] * 64;            // (read only when the image has four components)
    const int ys = g.bw[0] * 8, cs = g.bw[1] * 8;
    uint8_t* dst = sources + d.src_offset;
    for (unsigned it = blockIdx.x * kThreads + threadIdx.x; it < groups; it += gridDim.x * kThreads) {
        const unsigned p0 = it * 4u;
        int y = (int)(p0 / (unsigned)w), x = (int)(p0 - (unsigned)y * (unsigned)w);
        unsigned bytes[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned r = 0, gg = 0, b = 0;
            if (p0 + i < npix) {
                const int lum = yp[(size_t)y * ys + x];
                if (g.ncomp == 1) {
                    r = gg = b = (unsigned)lum;
                } else if (g.ncomp == 4) {
                    // Adobe CMYK, stored inverted: the library passes the four samples through, Pillow inverts them on load
                    // (C = 255 - sample) and converts with nk = 255 - K = the fourth sample
                    const size_t at = (size_t)y * ys + x;       // (four planes of one size)
                    const int nk = kp[at];
                    r = clip255(nk - muldiv255(255 - lum, nk));
                    gg = clip255(nk - muldiv255(255 - (int)cbp[at], nk));
                    b = clip255(nk - muldiv255(255 - (int)crp[at], nk));
                } else {
                    const int cb = chroma_at(cbp, cs, g, x, y) - 128, cr = chroma_at(crp, cs, g, x, y) - 128;
                    r = clip255(lum + ((91881 * cr + 32768) >> 16));
                    gg = clip255(lum + ((-22554 * cb - 46802 * cr + 32768) >> 16));
                    b = clip255(lum + ((116130 * cb + 32768) >> 16));
                }
            }
            bytes[3 * i] = r;
            bytes[3 * i + 1] = gg;
            bytes[3 * i + 2] = b;
            if (++x == w) {
                x = 0;
                ++y;
            }
        }
        if (p0 + 4u <= npix) {
            unsigned* q = reinterpret_cast<unsigned*>(dst + (size_t)it * 12);
#pragma unroll
            for (int j = 0; j < 3; ++j) q[j] = bytes[4 * j] | (bytes[4 * j + 1] << 8) | (bytes[4 * j + 2] << 16) | (bytes[4 * j + 3] << 24);
        } else {
            const int valid = (int)(npix - p0) * 3;
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                if (j < valid) dst[(size_t)it * 12 + j] = (uint8_t)bytes[j];
            }
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ entry points
extern "C" size_t mpn_jpeg_desc_bytes(void) { return sizeof(Desc); }

extern "C" size_t mpn_jpeg_decode_workspace_bytes(int B, long long total_blocks) {
    if (B < 1 || total_blocks < B) return 0;
    return (size_t)total_blocks * 64;
}

extern "C" int mpn_jpeg_decode(const int16_t* coefs, size_t coef_bytes, const void* descs, int B, uint8_t* sources_out,
                               size_t sources_bytes, void* work, size_t work_bytes, mpn_stream_t stream) {
    MPN_REQUIRE(coefs && descs && sources_out && work, MPN_ERR_BAD_ARG, "jpeg_decode: null pointer");
    MPN_REQUIRE(B >= 1 && B <= 65535, MPN_ERR_BAD_SHAPE, "jpeg_decode: B must be in [1, 65535] (got %d)", B);
    MPN_REQUIRE(mpn_aligned16(coefs) && mpn_aligned16(descs) && mpn_aligned16(sources_out) && mpn_aligned16(work), MPN_ERR_BAD_ALIGN,
                "jpeg_decode: coefs, descs, sources_out and work must be 16-byte aligned");
    MPN_REQUIRE(coef_bytes >= 128 && work_bytes >= 64 && sources_bytes >= 3, MPN_ERR_WORKSPACE,
                "jpeg_decode: coefficients of %zu, workspace of %zu, sources of %zu bytes", coef_bytes, work_bytes, sources_bytes);
    const Desc* dd = reinterpret_cast<const Desc*>(descs);
    jpeg_idct_kernel<<<dim3(kIdctGroups, (unsigned)B), kThreads, 0, (hipStream_t)stream>>>(
        coefs, coef_bytes, dd, reinterpret_cast<uint8_t*>(work), work_bytes, sources_bytes);
    MPN_LAUNCH_CHECK();
    jpeg_colour_kernel<<<dim3(kColourGroups, (unsigned)B), kThreads, 0, (hipStream_t)stream>>>(
        dd, reinterpret_cast<const uint8_t*>(work), coef_bytes, work_bytes, sources_out, sources_bytes);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
