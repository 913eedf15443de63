// The pieces that the register sliding-window walks of dwconv.hip share: the storage-type accessors, the block / lane decode, the
// producer affine, the weight load, the window's column offsets with its row load and activation, the batch-norm reduction that
// rides on a data gradient, and the two block epilogues. Everything is inlined; what differs between the walks (window width,
// storage type, which column needs no select) is a template parameter. The walks themselves - the rotation of the raw row
// buffers, the order of loads against activations - stay in the kernels.
// A helper is NOT free of effect on the code around it: the same statements inside an inlined function reach the optimiser in
// another order than spelled out in the kernel, registers are allocated differently, and - where a sum has two products - the
// other one may get fused into the sum, which changes the last bit. The kernels therefore keep a copy of their own where a helper
// cost registers or changed a result; each such place says so.
#pragma once
#include "common.h"

namespace {

constexpr int kThreads = 256;
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

// 4 consecutive channels of the storage type, as loaded (8 or 16 bytes): the COMPUTE granule. 72 weight registers per thread
// (9 taps x 8 channels) pushed an 8-channel version to 2 waves/SIMD; 4 channels per lane need 36 and keep every global access a
// contiguous 8/16-byte piece of a fully used line.
template <typename T> struct Raw4;
template <> struct Raw4<float> { float4 v; };
template <> struct Raw4<bf16_t> { uint2 v; };
__device__ __forceinline__ void raw_load(Raw4<float>& r, const float* p) { r.v = *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void raw_load(Raw4<bf16_t>& r, const bf16_t* p) { r.v = *reinterpret_cast<const uint2*>(p); }
__device__ __forceinline__ void raw_unpack(const Raw4<float>& r, float (&f)[4]) { f[0] = r.v.x; f[1] = r.v.y; f[2] = r.v.z; f[3] = r.v.w; }
__device__ __forceinline__ void raw_unpack(const Raw4<bf16_t>& r, float (&f)[4]) {
    f[0] = __uint_as_float(r.v.x << 16); f[1] = __uint_as_float(r.v.x & 0xffff0000u);
    f[2] = __uint_as_float(r.v.y << 16); f[3] = __uint_as_float(r.v.y & 0xffff0000u);
}
template <typename T> __device__ __forceinline__ void raw_unpack2(const Raw4<T>& r, f32x2_t& v01, f32x2_t& v23) {
    float f[4];
    raw_unpack(r, f);
    v01 = (f32x2_t){f[0], f[1]};
    v23 = (f32x2_t){f[2], f[3]};
}
// two packed channel pairs -> 4 consecutive channels of the storage type (one v_cvt_pk_bf16_f32 per pair)
__device__ __forceinline__ void store4x2(float* p, f32x2_t a, f32x2_t b) {
    *reinterpret_cast<float4*>(p) = make_float4(a.x, a.y, b.x, b.y);
}
__device__ __forceinline__ void store4x2(bf16_t* p, f32x2_t a, f32x2_t b) {
    const bf16x2_t lo = __builtin_convertvector(a, bf16x2_t), hi = __builtin_convertvector(b, bf16x2_t);
    uint2 q;
    q.x = __builtin_bit_cast(unsigned, lo);
    q.y = __builtin_bit_cast(unsigned, hi);
    *reinterpret_cast<uint2*>(p) = q;
}
// the value a consumer reads back after the store (bf16 storage rounds, f32 does not)
template <typename T> __device__ __forceinline__ f32x2_t round_storage(f32x2_t a);
template <> __device__ __forceinline__ f32x2_t round_storage<float>(f32x2_t a) { return a; }
template <> __device__ __forceinline__ f32x2_t round_storage<bf16_t>(f32x2_t a) {
    return __builtin_convertvector(__builtin_convertvector(a, bf16x2_t), f32x2_t);
}

// XCD-aware work id: the dispatcher deals consecutive block ids round-robin over the 8 XCDs (each with its own L2), so
// blocks that share an XCD (same id % 8) get a contiguous range of work ids - neighbouring strips, which share halo
// columns and rows, then hit in one L2 instead of fetching the halo once per XCD. Bijective for any grid size.
__device__ __forceinline__ int xcd_work_id() {
    const int wid = blockIdx.x, nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = wid & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (wid >> 3);
}

// One block = one (image, row strip, column block, channel block) unit; lanes run over (column, 4-channel group) with the
// channels fastest, so every wave access is a contiguous run of pixels. XT: adjacent output columns per lane.
// CB_INNER: the channel block is the fastest part of the work id and `unit` numbers the rows of a [unit][9][C] weight slab (the
// kernels that write one); otherwise it is the slowest and `unit` = (image, strip, column block) numbers the [unit][2][C] rows.
struct SwLane {
    int img, yb, cgb, unit;
    int ox;    // the lane's first output column (0 in a lane without work)
    int cc;    // its first channel (0 in a lane without work)
    bool ok;   // the lane has work: loads of the others are clamped to valid addresses, their results dropped
};
template <int XT, bool CB_INNER>
__device__ __forceinline__ SwLane sw_lane(int C, int OW, int ncg, int cols, int xblocks, int yblocks, int cblocks) {
    SwLane l;
    int b = xcd_work_id(), xb;
    if (CB_INNER) {
        l.cgb = b % cblocks; b /= cblocks;
        l.unit = b;
        xb = b % xblocks; b /= xblocks;
        l.yb = b % yblocks;
        l.img = b / yblocks;
    } else {
        xb = b % xblocks; b /= xblocks;
        l.yb = b % yblocks; b /= yblocks;
        l.cgb = b % cblocks;
        l.img = b / cblocks;
        l.unit = (l.img * yblocks + l.yb) * xblocks + xb;
    }
    const int cgl = threadIdx.x % ncg, col = threadIdx.x / ncg;
    const int c = (l.cgb * ncg + cgl) * 4, ox = (xb * cols + col) * XT;
    l.ok = c < C && ox < OW && col < cols;
    l.cc = l.ok ? c : 0;
    l.ox = l.ok ? ox : 0;
    return l;
}

// the producer's batch-norm affine + activation on the way in: clamp(x * sc + sh, lo, hi) of the lane's 4 channels.
// NULLABLE: scale == nullptr means no producer (identity); the fused backward walks always have one.
struct InAffine {
    f32x2_t sc01, sc23, sh01, sh23;
    float lo, hi;
    template <bool NULLABLE>
    __device__ __forceinline__ void load(const float* scale, const float* shift, int act, int cc) {
        const bool on = !NULLABLE || scale != nullptr;
        float4 s4 = make_float4(1.f, 1.f, 1.f, 1.f), h4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on) { s4 = *reinterpret_cast<const float4*>(scale + cc); h4 = *reinterpret_cast<const float4*>(shift + cc); }
        sc01 = (f32x2_t){s4.x, s4.y}; sc23 = (f32x2_t){s4.z, s4.w};
        sh01 = (f32x2_t){h4.x, h4.y}; sh23 = (f32x2_t){h4.z, h4.w};
        lo = (on && act != MPN_ACT_NONE) ? 0.f : -INFINITY;
        hi = (on && act == MPN_ACT_RELU6) ? 6.f : INFINITY;
    }
    __device__ __forceinline__ void apply(float (&f)[4]) const {
        const f32x2_t v01 = (f32x2_t){f[0], f[1]} * sc01 + sh01, v23 = (f32x2_t){f[2], f[3]} * sc23 + sh23;
        f[0] = __builtin_amdgcn_fmed3f(v01.x, lo, hi); f[1] = __builtin_amdgcn_fmed3f(v01.y, lo, hi);
        f[2] = __builtin_amdgcn_fmed3f(v23.x, lo, hi); f[3] = __builtin_amdgcn_fmed3f(v23.y, lo, hi);
    }
};

// the lane's 9 x 4 weights as packed pairs; flip: tap t takes w[8 - t] (the stride-1 data gradient is a correlation with it)
// (for the forward walks. The three gradient walks whose sums have two products per term - dwconv_bwd_sw2_kernel,
//  dwconv_dgrad_s2_sw_kernel, dwconv_bwd_s2_kernel - spell the loop out: loaded through this function, the optimiser lists those
//  products in another order and fuses the other one of each pair; fused and separate launches then differ in the last bit)
__device__ __forceinline__ void load_weights(const float* w, int C, int cc, bool flip, f32x2_t (&w01)[9], f32x2_t (&w23)[9]) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const float4 q = *reinterpret_cast<const float4*>(w + (flip ? 8 - t : t) * C + cc);
        w01[t] = (f32x2_t){q.x, q.y};
        w23[t] = (f32x2_t){q.z, q.w};
    }
}

// An element on its way into a window stays 4 scalars (unpack, affine, zero outside the image) and becomes two packed pairs with
// one store at the end. Built up in place through references to the window array's elements, the f32 two-column forward needed
// 18 VGPRs more (188 -> 206) and, with the reduction, fell from two waves per SIMD to one.
__device__ __forceinline__ void zero_unless(bool ok, float (&f)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = ok ? f[j] : 0.f;
}
__device__ __forceinline__ void store_pairs(f32x2_t (&a)[2], const float (&f)[4]) {
    a[0] = (f32x2_t){f[0], f[1]};
    a[1] = (f32x2_t){f[2], f[3]};
}

// The NC input columns ix0 .. ix0 + NC - 1 of a lane's window: which of them are inside the image, and their element offsets in
// a row (clamped, so that every load is unpredicated: `if (ok) load else zero` is lowered to load + select, which waits for
// the data where the load stands - nothing would be in flight under the arithmetic).
template <typename T, int NC> struct WinCols {
    bool ok[NC];
    int off[NC];
    int H;
    long long rstep;   // elements per image row
    __device__ __forceinline__ void init(int ix0, bool lane_ok, int H_, int W, int C) {
        H = H_;
        rstep = (long long)W * C;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const int ix = ix0 + k;
            ok[k] = lane_ok && ix >= 0 && ix < W;
            off[k] = (ok[k] ? ix : 0) * C;
        }
    }
    // the raw pieces of row iy (clamped into the image) of the image at `img` (already offset to the lane's channels)
    __device__ __forceinline__ void load(Raw4<T> (&r)[NC], const T* img, int iy) const {
        const T* rowp = img + (long long)min(max(iy, 0), H - 1) * rstep;
#pragma unroll
        for (int k = 0; k < NC; ++k) raw_load(r[k], rowp + off[k]);
    }
    // raw pieces -> the activated window row [column][channel pair], zeros outside the image (the padding of the ACTIVATED
    // tensor). Row validity is uniform over the block: a scalar branch. AFF: apply the producer affine (without one the
    // affine + clamp of every element compiles away: 24 VALU operations and 8 registers per row); EDGE: some column of the wave
    // may be outside the image; INSIDE: a column that is inside whenever the lane has work and needs no select (-1: none).
    template <bool AFF, bool EDGE, int INSIDE>
    __device__ __forceinline__ void act(const Raw4<T> (&r)[NC], int iy, const InAffine& aff, f32x2_t (&a)[NC][2]) const {
        if (iy < 0 || iy >= H) {
#pragma unroll
            for (int k = 0; k < NC; ++k) { a[k][0] = (f32x2_t){0.f, 0.f}; a[k][1] = (f32x2_t){0.f, 0.f}; }
            return;
        }
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            float f[4];
            raw_unpack(r[k], f);
            if constexpr (AFF) aff.apply(f);
            if (EDGE && k != INSIDE) zero_unless(ok[k], f);
            store_pairs(a[k], f);
        }
    }
};

// Per-channel sums a walk leaves in one [2][C] partial row: the forward's batch statistics sum(y), sum(y^2), or - riding on a data
// gradient - the batch-norm backward reduction of the layer whose input gradient dA the walk produces: sum(g), sum(g * xhat) with
// g = dA * act'(x * scale + shift), xhat = (x - mean) * invstd, x that layer's raw conv output.
// The running sums s01, s23, q01, q23 and the weight gradient's a01[9], a23[9] are separate locals of the kernels and not members
// of a struct: in adjacent memory the optimiser widens their loads into overlapping 32-byte ones and the struct stays in memory.
__device__ __forceinline__ void add_stats(f32x2_t y01, f32x2_t y23, f32x2_t& s01, f32x2_t& s23, f32x2_t& q01, f32x2_t& q23) {
    s01 += y01; s23 += y23;
    q01 += y01 * y01; q23 += y23 * y23;
}
template <typename T> struct BnReduce {
    f32x2_t sc01, sc23, sh01, sh23, is01, is23, nm01, nm23;   // scale, shift, invstd, -mean * invstd
    float lo, hi;
    __device__ __forceinline__ void load(const float* scale, const float* shift, const float* mean, const float* invstd, int act, int cc) {
        const float4 s4 = *reinterpret_cast<const float4*>(scale + cc), h4 = *reinterpret_cast<const float4*>(shift + cc);
        const float4 m4 = *reinterpret_cast<const float4*>(mean + cc), i4 = *reinterpret_cast<const float4*>(invstd + cc);
        sc01 = (f32x2_t){s4.x, s4.y}; sc23 = (f32x2_t){s4.z, s4.w};
        sh01 = (f32x2_t){h4.x, h4.y}; sh23 = (f32x2_t){h4.z, h4.w};
        is01 = (f32x2_t){i4.x, i4.y}; is23 = (f32x2_t){i4.z, i4.w};
        nm01 = (f32x2_t){-m4.x * i4.x, -m4.y * i4.y}; nm23 = (f32x2_t){-m4.z * i4.z, -m4.w * i4.w};
        lo = (act != MPN_ACT_NONE) ? 0.f : -INFINITY;
        hi = (act == MPN_ACT_RELU6) ? 6.f : INFINITY;
    }
    // d: the gradient as computed (g uses the ROUNDED value a separate reduction would read back); xr: the raw x at its pixel
    __device__ __forceinline__ void add(f32x2_t d01, f32x2_t d23, const Raw4<T>& xr, f32x2_t& s01, f32x2_t& s23, f32x2_t& q01, f32x2_t& q23) const {
        f32x2_t x01, x23;
        raw_unpack2(xr, x01, x23);
        const f32x2_t p01 = x01 * sc01 + sh01, p23 = x23 * sc23 + sh23;
        d01 = round_storage<T>(d01); d23 = round_storage<T>(d23);
        f32x2_t g01, g23;
        g01.x = (p01.x > lo && p01.x < hi) ? d01.x : 0.f; g01.y = (p01.y > lo && p01.y < hi) ? d01.y : 0.f;
        g23.x = (p23.x > lo && p23.x < hi) ? d23.x : 0.f; g23.y = (p23.y > lo && p23.y < hi) ? d23.y : 0.f;
        s01 += g01; s23 += g23;
        q01 += g01 * (x01 * is01 + nm01); q23 += g23 * (x23 * is23 + nm23);
    }
};
// The batch-norm backward APPLY pass of the depthwise conv's OWN batch-norm on the way into a gradient walk's dY window: the piece
// becomes what mpn_bn_bwd_apply would have stored over it and the walk read back, bit for bit, rounded to the storage type.
// NO mask test: g is already zero where that batch-norm's activation blocks (the producers of g that reduce for it mask with the
// same expression on the same y), so the test of the separate pass changes nothing - shift, lo and hi would be 6 registers the
// walks do not have.
// "What the separate pass would have stored" is what bn_bwd_apply_kernel<bf16_t> (bn.hip) computes AS COMPILED, and that is not one
// expression: sc * g + (cb * y + cc) is two nested fused multiply-adds for channels 0 .. 5 of a 16-byte vector, and for channels
// 6, 7 of the third of the four vectors a thread takes per iteration (vector index / 256 % 4 == 2); in the other three the
// vectoriser left that pair out of the packed operations and it is evaluated as (cc + cb * y) + sc * g with every product and sum
// rounded. The two differ in the last bit of an f32, i.e. in the stored bf16 of about one element in 10^5 - and behind such an
// element the whole backward pass below it. The walk therefore evaluates the pair both ways in the lanes that hold channels 6, 7
// and selects by the piece's element index; tests/test_dw_bwd_apply_gpu.py pins the equality (it fails when a compiler lays that
// kernel out differently - then this selection has to follow).
template <typename T> struct DyApply {
    f32x2_t sc01, sc23, cb01, cb23, cc01, cc23;
    bool pair67;   // the lane's second pair is channels 6, 7 of a 16-byte vector
    __device__ __forceinline__ void load(const float* scale, const float* mean, const float* invstd, const float* k1, const float* k2, int cc) {
        const float4 s4 = *reinterpret_cast<const float4*>(scale + cc), m4 = *reinterpret_cast<const float4*>(mean + cc);
        const float4 i4 = *reinterpret_cast<const float4*>(invstd + cc);
        const float4 a4 = *reinterpret_cast<const float4*>(k1 + cc), b4 = *reinterpret_cast<const float4*>(k2 + cc);
        const float ss[4] = {s4.x, s4.y, s4.z, s4.w}, mm[4] = {m4.x, m4.y, m4.z, m4.w}, ii[4] = {i4.x, i4.y, i4.z, i4.w};
        const float aa[4] = {a4.x, a4.y, a4.z, a4.w}, bb[4] = {b4.x, b4.y, b4.z, b4.w};
        float cb[4], cc_[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {   // (the expressions of bn_bwd_apply_body: they contract alike - aa - (mm * ii) * bb is one fma)
            cb[j] = -ss[j] * bb[j] * ii[j];
            cc_[j] = -ss[j] * (aa[j] - mm[j] * ii[j] * bb[j]);
        }
        sc01 = (f32x2_t){ss[0], ss[1]}; sc23 = (f32x2_t){ss[2], ss[3]};
        cb01 = (f32x2_t){cb[0], cb[1]}; cb23 = (f32x2_t){cb[2], cb[3]};
        cc01 = (f32x2_t){cc_[0], cc_[1]}; cc23 = (f32x2_t){cc_[2], cc_[3]};
        pair67 = (cc & 4) != 0;
    }
    static __device__ __forceinline__ f32x2_t unfused(f32x2_t sc, f32x2_t g, f32x2_t cb, f32x2_t y, f32x2_t cc) {
#pragma clang fp contract(off)
        const f32x2_t t = cb * y, u = sc * g;
        return (cc + t) + u;
    }
    // f: the unpacked piece of g, in place; yr: the conv's raw output at the same pixel; elem: the piece's element index in the
    // tensor (its low 32 bits)
    __device__ __forceinline__ void apply(float (&f)[4], const Raw4<T>& yr, unsigned elem) const {
        f32x2_t y01, y23;
        raw_unpack2(yr, y01, y23);
        const f32x2_t g01 = {f[0], f[1]}, g23 = {f[2], f[3]};
        const f32x2_t o01 = __builtin_elementwise_fma(sc01, g01, __builtin_elementwise_fma(cb01, y01, cc01));
        f32x2_t o23 = __builtin_elementwise_fma(sc23, g23, __builtin_elementwise_fma(cb23, y23, cc23));
        const f32x2_t v23 = unfused(sc23, g23, cb23, y23, cc23);
        if (pair67 && ((elem >> 11) & 3u) != 2u) o23 = v23;   // (elem >> 3: the 16-byte vector; / 256 % 4: which of the thread's four)
        const f32x2_t r01 = round_storage<T>(o01), r23 = round_storage<T>(o23);
        f[0] = r01.x; f[1] = r01.y; f[2] = r23.x; f[3] = r23.y;
    }
};

// block epilogue of the sums: the block's columns summed per 4-channel group in a fixed order -> row `l.unit` of part [units][2][C].
// red: kThreads * 8 floats of LDS, [thread][8] (barrier first where it held something else).
__device__ __forceinline__ void write_sums_row(float* red, const SwLane& l, int ncg, int cols, int C, float* part, f32x2_t s01, f32x2_t s23,
                                               f32x2_t q01, f32x2_t q23) {
    float st[8] = {s01.x, s01.y, s23.x, s23.y, q01.x, q01.y, q23.x, q23.y};
#pragma unroll
    for (int j = 0; j < 8; ++j) red[threadIdx.x * 8 + j] = l.ok ? st[j] : 0.f;
    __syncthreads();
    if ((int)threadIdx.x < ncg && (l.cgb * ncg + (int)threadIdx.x) * 4 < C) {
        float acc8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int cidx = 0; cidx < cols; ++cidx)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc8[j] += red[(cidx * ncg + threadIdx.x) * 8 + j];
        float* dst = part + (long long)l.unit * 2 * C + (l.cgb * ncg + threadIdx.x) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) { dst[j] = acc8[j]; dst[C + j] = acc8[4 + j]; }
    }
}
// block epilogue of the weight gradient's 36 accumulators of a lane: the columns that share a 4-channel group summed in a fixed
// order -> row `l.unit` of part [units][9][C]. red: 9 * kThreads * 4 floats of LDS, [tap][thread][4 channels].
__device__ __forceinline__ void write_taps_row(float* red, const SwLane& l, int ncg, int cols, int C, float* part, const f32x2_t (&a01)[9],
                                               const f32x2_t (&a23)[9]) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        float4 v = make_float4(a01[t].x, a01[t].y, a23[t].x, a23[t].y);
        if (!l.ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(&red[(t * kThreads + threadIdx.x) * 4]) = v;
    }
    __syncthreads();
    const int nch = ncg * 4;
    float* dst = part + (long long)l.unit * 9 * C + l.cgb * nch;
    for (int o = threadIdx.x; o < 9 * nch; o += kThreads) {
        const int t = o / nch, cj = o - t * nch;
        if (l.cgb * nch + cj < C) {
            float sum = 0.f;
            for (int cidx = 0; cidx < cols; ++cidx) sum += red[(t * kThreads + cidx * ncg) * 4 + cj];
            dst[t * C + cj] = sum;
        }
    }
}

// the raw pieces of a tensor of dx's shape at the 2 x 2 block dx[2a..2a+1][2b..2b+1] (q: the block's first element)
template <typename T> __device__ __forceinline__ void quad_load(Raw4<T> (&r)[4], const T* q, long long xrow, int C) {
    raw_load(r[0], q); raw_load(r[1], q + C); raw_load(r[2], q + xrow); raw_load(r[3], q + xrow + C);
}
template <typename T> __device__ __forceinline__ void add_raw4(const Raw4<T>& r, f32x2_t& o01, f32x2_t& o23) {
    float f[4];
    raw_unpack(r, f);
    o01 += (f32x2_t){f[0], f[1]};
    o23 += (f32x2_t){f[2], f[3]};
}

}  // namespace
