// The mask feature of a COCO keypoint record on the device (the pixel work of the reference's data/create_tfrecords.py):
// person segmentations -> full-resolution loss / segmentation masks -> Lanczos4 to quarter size -> threshold -> packed bits.
//   mpn_coco_masks   a ragged batch of images in THREE launches, whatever the batch size:
//     1  zero     the workspace: per image two column-major bitmaps (rows in the bits of a word, ceil(h / 32) words per
//                 column): plane 0 = union of the DROPPED persons' masks, plane 1 = union of the KEPT persons' masks
//     2  parts    one block per polygon or run-length code. A polygon is COCO maskApi's rleFrPoly, transcribed: vertices
//                 scaled by 5 and cast to int, every edge walked in unit steps along its longer axis, a boundary crossing
//                 wherever the dense walk changes its x; the crossings toggle bits of a column-major bitmap in LDS (atomic
//                 XOR), an inclusive prefix XOR in flat column-major order turns them into the mask (parity resolved PER
//                 POLYGON), and the mask is ORed into the image's plane. Only the polygon's column range is worked on, in
//                 chunks of what 32 KB of LDS hold. A run-length code (crowd regions) is a prefix sum over its runs and the
//                 odd runs ORed into the plane.
//                 seg = OR over kept annotations of (OR over polygons) and loss = AND over dropped annotations of NOT(OR over
//                 polygons) = NOT(OR over all dropped polygons): the annotation level needs no pass of its own.
//     3  finish   per image: OpenCV's resize(INTER_LANCZOS4) for uint8 as integer arithmetic over host-built tap tables (8 x 8
//                 taps, 11-bit weights, replicate border, (x + 2^21) >> 22), `> 0`, and numpy.packbits of [mh, mw, 2] (MSB
//                 first, the stream running across row ends); optionally the full-resolution pair as uint8 [h, w, 2].
// The descriptors live on the device, so the launcher cannot read them: every offset, count and size in them is checked in
// the kernels against the totals the launcher was given, and a part or image that fails is skipped - nothing is indexed out
// of range whatever the tables hold. float64 steps are single IEEE operations in maskApi's order (contraction off).
// Latency-bound glue (a few hundred small blocks per batch): not tuned.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSide = MPN_COCO_MASKS_MAX_SIDE;
constexpr int kChunkWords = 8192;              // the LDS bitmap of one column chunk: 32 KB
constexpr int kMaxChunkCols = 1024;
constexpr int kTapWords = 5;                   // int32 first, int16 weight[8]
// a vertex is at most one image side outside the image (the Python layer refuses others): 5 * [-1024, 2048], with a margin.
// Clamping bounds the length of an edge walk whatever the vertex list holds.
constexpr double kCoordLo = -5.0 * kMaxSide - 8.0, kCoordHi = 10.0 * kMaxSide + 8.0;

struct Args {
    const mpn_coco_image_desc* images;
    const mpn_coco_part_desc* parts;
    const double* xy;
    const unsigned* runs;
    const int* taps;
    unsigned* planes;
    unsigned char* packed;
    unsigned char* full;
    long long num_xy, num_runs, num_taps, plane_words, packed_bytes, full_bytes;
    int num_images, num_parts, max_side;
};

__device__ bool image_ok(const Args& a, const mpn_coco_image_desc& im) {
    if (im.h < 1 || im.w < 1 || im.h > a.max_side || im.w > a.max_side) return false;
    const long long words = 2LL * im.w * ((im.h + 31) >> 5);
    return im.plane_offset >= 0 && im.plane_offset <= a.plane_words - words;
}

// exclusive prefix sum of one value per thread; `sh` holds kThreads values
template <typename T> __device__ T block_scan(T v, T* sh, T* total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int o = 1; o < kThreads; o <<= 1) {
        const T t = tid >= o ? sh[tid - o] : (T)0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    *total = sh[kThreads - 1];
    const T inclusive = sh[tid];
    __syncthreads();
    return inclusive - v;
}

// rows [row, row + n) of one column (n >= 1, row + n <= h)
__device__ void set_rows(unsigned* column, int row, int n) {
    const int last = row + n - 1;
    for (int i = row >> 5; i <= last >> 5; ++i) {
        unsigned m = 0xffffffffu;
        if (i == row >> 5) m &= 0xffffffffu << (row & 31);
        if (i == last >> 5) m &= 0xffffffffu >> (31 - (last & 31));
        atomicOr(column + i, m);
    }
}

// ---------------------------------------------------------------- a run-length code
__device__ void rle_part(const Args& a, const mpn_coco_part_desc& p, int h, int w, int wpc, unsigned* plane,
                         unsigned long long* scan) {
    const int tid = threadIdx.x;
    const unsigned* runs = a.runs + p.offset;
    const unsigned long long hw = (unsigned long long)h * w;
    unsigned long long base = 0;
    for (int g = 0; g < p.count && base < hw; g += kThreads) {       // base is the same in every thread
        const int i = g + tid;
        const unsigned long long len = i < p.count ? runs[i] : 0u;
        unsigned long long total;
        unsigned long long a0 = base + block_scan<unsigned long long>(len, scan, &total);
        unsigned long long a1 = a0 + len;
        if ((i & 1) && a0 < hw) {
            if (a1 > hw) a1 = hw;
            while (a0 < a1) {
                const int col = (int)(a0 / h), row = (int)(a0 - (unsigned long long)col * h);
                const int n = (int)(a1 - a0 < (unsigned long long)(h - row) ? a1 - a0 : (unsigned long long)(h - row));
                set_rows(plane + (size_t)col * wpc, row, n);
                a0 += n;
            }
        }
        base += total;
    }
}

// ---------------------------------------------------------------- a polygon
__device__ int scaled(double v) {
    double s = 5.0 * v + .5;
    s = fmin(fmax(s, kCoordLo), kCoordHi);           // (a NaN becomes kCoordLo)
    return (int)s;
}

struct Edges {                                       // slot 0: the edge before the group; slot 1 + t: edge (group + t)
    int xs[kThreads + 1], ys[kThreads + 1], xe[kThreads + 1], ye[kThreads + 1];
    double slope[kThreads + 1];
};

__device__ void load_edge(const double* xy, int k, int e, Edges& E, int slot) {
    const int n = e + 1 < k ? e + 1 : 0;
    int xs = scaled(xy[2 * e]), ys = scaled(xy[2 * e + 1]), xe = scaled(xy[2 * n]), ye = scaled(xy[2 * n + 1]);
    E.xs[slot] = xs; E.ys[slot] = ys; E.xe[slot] = xe; E.ye[slot] = ye;
    const int dx = abs(xe - xs), dy = abs(ys - ye);
    if ((dx >= dy && xs > xe) || (dx < dy && ys > ye)) {
        int t = xs; xs = xe; xe = t;
        t = ys; ys = ye; ye = t;
    }
    // (an edge of no length: maskApi divides 0 by 0; here it emits its one point)
    E.slope[slot] = dx >= dy ? (dx > 0 ? (double)(ye - ys) / dx : 0.0) : (double)(xe - xs) / dy;
}

__device__ int edge_points(const Edges& E, int slot) {
    const int dx = abs(E.xe[slot] - E.xs[slot]), dy = abs(E.ys[slot] - E.ye[slot]);
    return (dx > dy ? dx : dy) + 1;
}

// point d of the edge in `slot`, in the edge's original direction
__device__ void edge_point(const Edges& E, int slot, int d, int* u, int* v) {
    int xs = E.xs[slot], ys = E.ys[slot], xe = E.xe[slot], ye = E.ye[slot];
    const int dx = abs(xe - xs), dy = abs(ys - ye);
    const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
    if (flip) {
        xs = xe;
        ys = ye;
    }
    const double s = E.slope[slot];
    if (dx >= dy) {
        const int t = flip ? dx - d : d;
        *u = t + xs;
        *v = (int)((double)ys + s * (double)t + .5);
    } else {
        const int t = flip ? dy - d : d;
        *v = t + ys;
        *u = (int)((double)xs + s * (double)t + .5);
    }
}

struct PolyShared {
    unsigned bits[kChunkWords];
    Edges edges;
    int start[kThreads];
    int scan[kThreads];
    unsigned char colpar[kMaxChunkCols];
    int lo, hi;
    unsigned carry;
};

__device__ void poly_part(const Args& a, const mpn_coco_part_desc& p, int h, int w, int wpc, unsigned* plane, PolyShared& S) {
    const int tid = threadIdx.x;
    const double* xy = a.xy + p.offset;
    const int k = p.count;
    if (k < 1) return;
    // the column range the crossings can fall in
    if (tid == 0) {
        S.lo = 0x7fffffff;
        S.hi = -0x7fffffff;
        S.carry = 0u;
    }
    __syncthreads();
    for (int i = tid; i < k; i += kThreads) {
        const int x = scaled(xy[2 * i]);
        atomicMin(&S.lo, x);
        atomicMax(&S.hi, x);
    }
    __syncthreads();
    // a crossing's column is (u' - 2) / 5 for a u' in [lo - 1, hi]; one more column for a crossing clamped to y == h
    const int c0 = S.lo - 10 > 0 ? (S.lo - 10) / 5 : 0;
    const int c1 = S.hi + 10 < 0 ? -1 : min(w - 1, (S.hi + 10) / 5 + 1);
    const int stride = wpc | 1;                      // odd: a thread per column hits every LDS bank
    const int chunk_cols = min(kChunkWords / stride, kMaxChunkCols);
    const unsigned last_mask = (h & 31) ? (1u << (h & 31)) - 1u : 0xffffffffu;

    for (int cb = c0; cb <= c1; cb += chunk_cols) {
        const int nc = min(chunk_cols, c1 - cb + 1);
        for (int i = tid; i < nc * stride; i += kThreads) S.bits[i] = 0u;
        __syncthreads();
        for (int g = 0; g < k; g += kThreads) {
            const int e = g + tid;
            if (e < k) load_edge(xy, k, e, S.edges, tid + 1);
            if (tid == 0 && g > 0) load_edge(xy, k, g - 1, S.edges, 0);
            __syncthreads();
            int total;
            const int len = e < k ? edge_points(S.edges, tid + 1) : 0;
            S.start[tid] = block_scan<int>(len, S.scan, &total);
            __syncthreads();
            for (int j = tid; j < total; j += kThreads) {
                int t = 0;                           // the last edge of the group that starts at or before point j
                for (int o = kThreads >> 1; o > 0; o >>= 1)
                    if (t + o < kThreads && S.start[t + o] <= j) t += o;
                const int d = j - S.start[t];
                int cu, cv, pu, pv;
                edge_point(S.edges, t + 1, d, &cu, &cv);
                if (d > 0)
                    edge_point(S.edges, t + 1, d - 1, &pu, &pv);
                else if (g + t > 0)
                    edge_point(S.edges, t, edge_points(S.edges, t) - 1, &pu, &pv);
                else
                    continue;                        // the first point of the walk has no predecessor
                if (cu == pu) continue;
                double xd = (double)(cu < pu ? cu : cu - 1);
                xd = (xd + .5) / 5.0 - .5;
                if (floor(xd) != xd || xd < 0 || xd > (double)(w - 1)) continue;
                double yd = (double)(cv < pv ? cv : pv);
                yd = (yd + .5) / 5.0 - .5;
                if (yd < 0) yd = 0; else if (yd > (double)h) yd = (double)h;
                yd = ceil(yd);
                int col = (int)xd, row = (int)yd;
                if (row >= h) {                      // flat index x * h + h: the first pixel of the next column
                    col += 1;
                    row = 0;
                }
                if (col >= cb && col < cb + nc) atomicXor(&S.bits[(col - cb) * stride + (row >> 5)], 1u << (row & 31));
            }
            __syncthreads();
        }
        // parity in flat column-major order: a column's carry-in is the parity of everything before it
        for (int c = tid; c < nc; c += kThreads) {
            unsigned x = 0u;
            for (int i = 0; i < wpc; ++i) x ^= S.bits[c * stride + i];
            S.colpar[c] = (unsigned char)(__popc(x) & 1);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned carry = S.carry;
            for (int c = 0; c < nc; ++c) {
                const unsigned t = S.colpar[c];
                S.colpar[c] = (unsigned char)carry;
                carry ^= t;
            }
            S.carry = carry;
        }
        __syncthreads();
        for (int c = tid; c < nc; c += kThreads) {
            unsigned carry = S.colpar[c];
            unsigned* column = plane + (size_t)(cb + c) * wpc;
            for (int i = 0; i < wpc; ++i) {
                unsigned x = S.bits[c * stride + i];
                x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;      // bit r: parity of bits 0..r
                if (carry) x = ~x;
                carry = x >> 31;
                if (i == wpc - 1) x &= last_mask;
                if (x) atomicOr(column + i, x);
            }
        }
        __syncthreads();
    }
    // parity still odd behind the polygon's columns: the run goes on to the end of the image (no closed polygon does this)
    if (S.carry & 1u) {
        const int first = c1 + 1 > 0 ? c1 + 1 : 0;
        for (long long i = tid; i < (long long)(w - first) * wpc; i += kThreads) {
            const int word = (int)(i % wpc);
            atomicOr(plane + (size_t)first * wpc + i, word == wpc - 1 ? last_mask : 0xffffffffu);
        }
    }
}

__global__ __launch_bounds__(kThreads) void coco_parts_kernel(Args a) {
    __shared__ PolyShared S;
    __shared__ unsigned long long scan64[kThreads];
    // (every return below depends on the block's part alone: no barrier is left behind)
    const mpn_coco_part_desc p = a.parts[blockIdx.x];
    if (p.image < 0 || p.image >= a.num_images || p.count < 0 || p.offset < 0) return;
    const mpn_coco_image_desc im = a.images[p.image];
    if (!image_ok(a, im)) return;
    const int wpc = (im.h + 31) >> 5;
    unsigned* plane = a.planes + im.plane_offset + ((p.flags & MPN_COCO_PART_DROPPED) ? (size_t)0 : (size_t)im.w * wpc);
    if (p.flags & MPN_COCO_PART_RLE) {
        if (p.offset > a.num_runs - p.count) return;
        rle_part(a, p, im.h, im.w, wpc, plane, scan64);
    } else {
        if (p.offset > a.num_xy - 2LL * p.count) return;
        poly_part(a, p, im.h, im.w, wpc, plane, S);
    }
}

// ---------------------------------------------------------------- Lanczos4, threshold, packbits
__device__ __forceinline__ int tap_weight(const int* t, int k) { return (int)(short)((unsigned)t[1 + (k >> 1)] >> (16 * (k & 1))); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(kThreads) void coco_finish_kernel(Args a) {
    const mpn_coco_image_desc im = a.images[blockIdx.y];
    if (!image_ok(a, im)) return;
    const int h = im.h, w = im.w, wpc = (h + 31) >> 5, mh = (h + 3) >> 2, mw = (w + 3) >> 2;
    const unsigned* dropped = a.planes + im.plane_offset;
    const unsigned* kept = dropped + (size_t)w * wpc;
    const int first = blockIdx.x * kThreads + threadIdx.x, step = gridDim.x * kThreads;
    const int pixels = mh * mw, nbytes = (pixels * 2 + 7) >> 3;
    const bool tables_ok = im.tap_x >= 0 && im.tap_y >= 0 && im.tap_x <= a.num_taps - mw && im.tap_y <= a.num_taps - mh;
    if (tables_ok && im.packed_offset >= 0 && im.packed_offset <= a.packed_bytes - nbytes) {
        for (int byte = first; byte < nbytes; byte += step) {
            unsigned out = 0u;
            for (int q = 0; q < 4; ++q) {
                const int pix = byte * 4 + q;
                if (pix >= pixels) break;
                const int dy = pix / mw, dx = pix - dy * mw;
                const int* tx = a.taps + (size_t)(im.tap_x + dx) * kTapWords;
                const int* ty = a.taps + (size_t)(im.tap_y + dy) * kTapWords;
                const int sx = clampi(tx[0], -8, kMaxSide + 8), sy = clampi(ty[0], -8, kMaxSide + 8);
                int wy[8], rows[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    wy[k] = tap_weight(ty, k);
                    rows[k] = clampi(sy - 3 + k, 0, h - 1);
                }
                int loss = 0, seg = 0;
#pragma unroll
                for (int kx = 0; kx < 8; ++kx) {
                    const size_t col = (size_t)clampi(sx - 3 + kx, 0, w - 1) * wpc;
                    int vl = 0, vs = 0;
#pragma unroll
                    for (int ky = 0; ky < 8; ++ky) {
                        const int r = rows[ky];
                        vl += wy[ky] * (int)(1u - ((dropped[col + (r >> 5)] >> (r & 31)) & 1u));
                        vs += wy[ky] * (int)((kept[col + (r >> 5)] >> (r & 31)) & 1u);
                    }
                    const int wx = tap_weight(tx, kx);
                    loss += wx * vl;
                    seg += wx * vs;
                }
                if (((loss + (1 << 21)) >> 22) > 0) out |= 0x80u >> (2 * q);
                if (((seg + (1 << 21)) >> 22) > 0) out |= 0x40u >> (2 * q);
            }
            a.packed[im.packed_offset + byte] = (unsigned char)out;
        }
    }
    if (a.full && im.full_offset >= 0 && im.full_offset <= a.full_bytes - 2LL * h * w) {
        unsigned char* full = a.full + im.full_offset;
        for (int pix = first; pix < h * w; pix += step) {
            const int y = pix / w, x = pix - y * w;
            const size_t at = (size_t)x * wpc + (y >> 5);
            full[2 * (size_t)pix] = (unsigned char)(1u - ((dropped[at] >> (y & 31)) & 1u));
            full[2 * (size_t)pix + 1] = (unsigned char)((kept[at] >> (y & 31)) & 1u);
        }
    }
}

__global__ __launch_bounds__(kThreads) void coco_zero_kernel(uint4* p, long long n) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads)
        p[i] = make_uint4(0u, 0u, 0u, 0u);
}

inline bool side_ok(int v) { return v >= 1 && v <= kMaxSide; }

}  // namespace

extern "C" size_t mpn_coco_masks_image_desc_bytes(void) { return sizeof(mpn_coco_image_desc); }
extern "C" size_t mpn_coco_masks_part_desc_bytes(void) { return sizeof(mpn_coco_part_desc); }

extern "C" size_t mpn_coco_masks_plane_words(int h, int w) {
    if (!side_ok(h) || !side_ok(w)) return 0;
    return (size_t)2 * w * ((h + 31) / 32);
}

extern "C" size_t mpn_coco_masks_packed_bytes(int h, int w) {
    if (!side_ok(h) || !side_ok(w)) return 0;
    return ((size_t)((h + 3) / 4) * ((w + 3) / 4) * 2 + 7) / 8;
}

extern "C" int mpn_coco_masks(const mpn_coco_image_desc* images, int num_images, int max_side, const mpn_coco_part_desc* parts,
                              int num_parts, const double* xy, long long num_xy, const uint32_t* runs, long long num_runs,
                              const int32_t* taps, long long num_taps, void* workspace, size_t workspace_bytes, void* packed,
                              size_t packed_bytes, void* full, size_t full_bytes, mpn_stream_t stream) {
    MPN_REQUIRE(max_side >= 1 && max_side <= kMaxSide, MPN_ERR_BAD_SHAPE,
                "coco_masks: max_side = %d, an image side is 1..%d (a column of the bitmap is at most %d words)", max_side,
                kMaxSide, kMaxSide / 32);
    MPN_REQUIRE(num_images >= 1 && num_images <= 65535, MPN_ERR_BAD_SHAPE, "coco_masks: num_images = %d (1..65535)", num_images);
    MPN_REQUIRE(num_parts >= 0 && num_xy >= 0 && num_runs >= 0 && num_taps >= 1, MPN_ERR_BAD_SHAPE,
                "coco_masks: num_parts = %d, num_xy = %lld, num_runs = %lld, num_taps = %lld", num_parts, num_xy, num_runs, num_taps);
    MPN_REQUIRE(images && taps && workspace && packed && (parts || num_parts == 0) && (xy || num_xy == 0) && (runs || num_runs == 0),
                MPN_ERR_BAD_ARG, "coco_masks: null pointer");
    MPN_REQUIRE((((uintptr_t)images | (uintptr_t)parts | (uintptr_t)xy) & 7u) == 0 && (((uintptr_t)runs | (uintptr_t)taps) & 3u) == 0 &&
                    mpn_aligned16(workspace),
                MPN_ERR_BAD_ALIGN, "coco_masks: images / parts / xy must be 8-byte, runs / taps 4-byte, workspace 16-byte aligned");
    MPN_REQUIRE(workspace_bytes >= 16 && workspace_bytes % 16 == 0 && packed_bytes >= 1 && (!full || full_bytes >= 2),
                MPN_ERR_WORKSPACE, "coco_masks: workspace_bytes = %zu (a multiple of 16), packed_bytes = %zu, full_bytes = %zu",
                workspace_bytes, packed_bytes, full_bytes);
    Args a = {images, parts, xy, runs, taps, (unsigned*)workspace, (unsigned char*)packed, (unsigned char*)full,
              num_xy, num_runs, num_taps, (long long)(workspace_bytes / 4), (long long)packed_bytes, full ? (long long)full_bytes : 0,
              num_images, num_parts, max_side};
    hipStream_t s = (hipStream_t)stream;
    const long long vecs = (long long)(workspace_bytes / 16);
    coco_zero_kernel<<<(unsigned)(vecs / kThreads < 1 ? 1 : (vecs / kThreads > 1024 ? 1024 : vecs / kThreads)), kThreads, 0, s>>>(
        (uint4*)workspace, vecs);
    MPN_LAUNCH_CHECK();
    if (num_parts > 0) {
        coco_parts_kernel<<<num_parts, kThreads, 0, s>>>(a);
        MPN_LAUNCH_CHECK();
    }
    const int mside = (max_side + 3) / 4;
    const int per_image = full ? max_side * max_side : (mside * mside * 2 + 7) / 8;
    const int gx = per_image / (kThreads * 4) < 1 ? 1 : (per_image / (kThreads * 4) > 64 ? 64 : per_image / (kThreads * 4));
    coco_finish_kernel<<<dim3(gx, num_images), kThreads, 0, s>>>(a);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
