// Training examples of the pose residual network, from annotations alone (reference
// detector/input_pipeline/prn_pipeline.py:46-203). One call writes a batch of
//
//   crops [N, CH, CW, 17]   tf.image.crop_and_resize (bilinear, extrapolation 0) of the target heatmap of the example's
//                           source image around the person's box                                     (:91-103)
//   labels[N, CH, CW, 17]   a single 1.0 per visible keypoint of the person, at its rounded position in the box (:105-151)
//
// optionally flipped left-right with the left / right parts exchanged (:159-203). The source images are ragged in size
// and their heatmaps are never materialised: a crop pixel needs four taps of its image's heatmap, and a tap is
//   max(0, max over the image's visible blobs of float32(g_p[|dy|] * g_p[|dx|]),  |dy|, |dx| <= k_p)
// evaluated from the per-person tables of render_person.h - the values mpn_heatmap_render writes, so the result is
// bit-identical to get_heatmaps + crop_and_resize. Arithmetic and order of the interpolation are those of
// prn_post.hip's crop_kernel (crop_and_resize_op.cc); every float step is one IEEE operation (no contraction).
// Store-bound: N * CH * CW * 17 * 8 bytes written once (8.8 MB at N = 32), a few KB read.
#include "common.h"
#include "render_person.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPix = 128;                    // crop pixels (flattened y * CW + x) per block, one per thread
constexpr int kEThreads = kPix;

struct ExampleDesc {                         // == mpn_prn_example_desc
    int32_t image, person, flip, reserved;
};
static_assert(sizeof(ExampleDesc) == MPN_PRN_EXAMPLE_DESC_BYTES, "descriptor size is fixed");
static_assert(sizeof(mpn_prn_example_desc) == sizeof(ExampleDesc), "descriptor layout");

// prn_pipeline.py:193: the part that takes the place of part c after a left-right flip (an involution)
__device__ __forceinline__ int flip_part(int c) { return c == 0 ? 0 : ((c & 1) ? c + 1 : c - 1); }

// Tables of all Q persons; the centres of person p are scaled by the size of ITS image (the r with
// first_person[r] <= p < first_person[r+1]).
__global__ void __launch_bounds__(256) examples_prepare_kernel(const int32_t* __restrict__ keypoints,
                                                                const float* __restrict__ boxes, int Q,
                                                                const int32_t* __restrict__ first_person,
                                                                const int32_t* __restrict__ width,
                                                                const int32_t* __restrict__ height, int R,
                                                                int downsample, RenderTables t) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Q * kParts) return;
    const int p = i / kParts;
    int lo = 0, hi = R;                      // the last r in [0, R) with first_person[r] <= p
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first_person[mid] <= p) lo = mid; else hi = mid;
    }
    const int H = height[lo], W = width[lo];
    const int h = (H + downsample - 1) / downsample, w = (W + downsample - 1) / downsample;
    render_prepare_entry(keypoints, boxes, i, (float)(H - 1.0), (float)(W - 1.0), (float)(h - 1), (float)(w - 1), t);
}

__device__ __forceinline__ void store_tile(const float* tile, float* __restrict__ dst, int count, int tid) {
    if ((((uintptr_t)dst) & 15) == 0) {
        const int nv = count >> 2;
        const float4* src = reinterpret_cast<const float4*>(tile);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int i = tid; i < nv; i += kEThreads) d4[i] = src[i];
        for (int i = (nv << 2) + tid; i < count; i += kEThreads) dst[i] = tile[i];
    } else {
        for (int i = tid; i < count; i += kEThreads) dst[i] = tile[i];
    }
}

// grid = N * tiles blocks; block (n, tile) owns pixels [tile * kPix, +kPix) of example n, all 17 channels.
__global__ void __launch_bounds__(kEThreads) examples_kernel(const int32_t* __restrict__ keypoints,
                                                            const float* __restrict__ boxes, int Q,
                                                            const int32_t* __restrict__ first_person,
                                                            const int32_t* __restrict__ width,
                                                            const int32_t* __restrict__ height, int R,
                                                            const ExampleDesc* __restrict__ examples, int tiles, int CH,
                                                            int CW, int downsample, RenderTables t,
                                                            float* __restrict__ crops, float* __restrict__ labels) {
    // the four taps (tl, tr, bl, br) of every (pixel, part): lane stride 17 float4 = 68 dwords, conflict-free for
    // 16-byte LDS accesses. The finished [pixel][17] tile reuses the front of the same memory.
    __shared__ float4 acc[kPix * kParts];
    __shared__ double gl[kChunk * (kMaxHalf + 1)];
    __shared__ int4 hits[kChunk * kParts];              // (cy, cx, k, part | local person << 8)
    __shared__ int nhits;
    float* tile = reinterpret_cast<float*>(acc);

    const int tid = threadIdx.x;
    const int n = blockIdx.x / tiles, t0 = (blockIdx.x - n * tiles) * kPix;
    const int npix = min(kPix, CH * CW - t0);
    const ExampleDesc e = examples[n];
    const bool live = e.image >= 0 && e.image < R && e.person >= 0 && e.person < Q;
    const bool flip = e.flip != 0;
    const size_t base = ((size_t)n * CH * CW + t0) * kParts;

#pragma unroll
    for (int j = 0; j < kParts; ++j) acc[tid * kParts + j] = make_float4(0.f, 0.f, 0.f, 0.f);

    // ---- crops (prn_pipeline.py:91-103)
    const int p = t0 + tid;
    const int y = p / CW, x = p - y * CW;
    const int xs = flip ? CW - 1 - x : x;               // the column before the flip
    bool ok = false;
    int ty = 0, by = 0, lx = 0, rx = 0;
    float yl = 0.f, xl = 0.f;
    if (live) {
        const int H = height[e.image], W = width[e.image];
        const int h = (H + downsample - 1) / downsample, w = (W + downsample - 1) / downsample;
        // boxes / scaler (:66,99), then crop_and_resize_op.cc over the [h, w] map
        const float fH = (float)H, fW = (float)W;
        const float y1 = boxes[e.person * 4 + 0] / fH, x1 = boxes[e.person * 4 + 1] / fW;
        const float y2 = boxes[e.person * 4 + 2] / fH, x2 = boxes[e.person * 4 + 3] / fW;
        const float hm = (float)(h - 1), wm = (float)(w - 1);
        const float hs = (CH > 1) ? (y2 - y1) * hm / (float)(CH - 1) : 0.f;
        const float ws = (CW > 1) ? (x2 - x1) * wm / (float)(CW - 1) : 0.f;
        auto src_y = [&](int yy) { return (CH > 1) ? y1 * hm + (float)yy * hs : 0.5f * (y1 + y2) * hm; };
        auto src_x = [&](int xx) { return (CW > 1) ? x1 * wm + (float)xx * ws : 0.5f * (x1 + x2) * wm; };
        const float in_y = src_y(y), in_x = src_x(xs);
        ok = tid < npix && !(in_y < 0.f || in_y > hm || in_x < 0.f || in_x > wm);
        if (ok) {
            ty = (int)floorf(in_y); by = (int)ceilf(in_y);
            lx = (int)floorf(in_x); rx = (int)ceilf(in_x);
            yl = in_y - (float)ty; xl = in_x - (float)lx;
        }
        // the block's source window, for culling: its rows, every column (in_y, in_x are monotone in y, x)
        const float ya = src_y(t0 / CW), yb = src_y((t0 + npix - 1) / CW);
        const float xa = src_x(0), xb = src_x(CW - 1);
        const float wy0 = floorf(fminf(ya, yb)), wy1 = ceilf(fmaxf(ya, yb));
        const float wx0 = floorf(fminf(xa, xb)), wx1 = ceilf(fmaxf(xa, xb));
        const int p_begin = min(max(first_person[e.image], 0), Q);
        const int p_end = min(max(first_person[e.image + 1], p_begin), Q);

        for (int p0 = p_begin; p0 < p_end; p0 += kChunk) {
            const int np = min(kChunk, p_end - p0);
            if (tid == 0) nhits = 0;
            __syncthreads();
            for (int i = tid; i < np * kParts; i += kEThreads) {
                const int lp = i / kParts, j = i - lp * kParts;
                const int2 c = t.centre[(size_t)p0 * kParts + i];
                const int k = t.half[p0 + lp];
                if (c.x != kInvisible && (float)c.x + (float)k >= wy0 && (float)c.x - (float)k <= wy1 &&
                    (float)c.y + (float)k >= wx0 && (float)c.y - (float)k <= wx1) {
                    const int slot = atomicAdd(&nhits, 1);
                    hits[slot] = make_int4(c.x, c.y, k, j | (lp << 8));
                }
            }
            __syncthreads();
            const int nh = nhits;
            if (nh > 0) {
                for (int i = tid; i < np * (kMaxHalf + 1); i += kEThreads) {
                    const int lp = i / (kMaxHalf + 1), d = i - lp * (kMaxHalf + 1);
                    gl[i] = t.g[(size_t)(p0 + lp) * kG + d];
                }
                __syncthreads();
                if (ok) {
                    for (int i = 0; i < nh; ++i) {
                        const int4 hit = hits[i];
                        const int dy0 = abs(ty - hit.x), dy1 = abs(by - hit.x);
                        const int dx0 = abs(lx - hit.y), dx1 = abs(rx - hit.y);
                        if ((dy0 > hit.z && dy1 > hit.z) || (dx0 > hit.z && dx1 > hit.z)) continue;
                        const double* g = gl + (hit.w >> 8) * (kMaxHalf + 1);
                        // outside the blob's window the map holds 0 (g[d] is only defined for d <= k <= 13)
                        const double gy0 = dy0 <= hit.z ? g[dy0] : 0.0, gy1 = dy1 <= hit.z ? g[dy1] : 0.0;
                        const double gx0 = dx0 <= hit.z ? g[dx0] : 0.0, gx1 = dx1 <= hit.z ? g[dx1] : 0.0;
                        float4* cell = acc + tid * kParts + (hit.w & 255);
                        float4 v = *cell;
                        v.x = fmaxf(v.x, (float)(gy0 * gx0));
                        v.y = fmaxf(v.y, (float)(gy0 * gx1));
                        v.z = fmaxf(v.z, (float)(gy1 * gx0));
                        v.w = fmaxf(v.w, (float)(gy1 * gx1));
                        *cell = v;
                    }
                }
            }
            __syncthreads();
        }
    }
    float res[kParts];
#pragma unroll
    for (int j = 0; j < kParts; ++j) {
        const float4 v = acc[tid * kParts + j];           // (tl, tr, bl, br)
        const float top = v.x + (v.y - v.x) * xl;
        const float bot = v.z + (v.w - v.z) * xl;
        res[j] = ok ? top + (bot - top) * yl : 0.f;     // extrapolation value 0
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kParts; ++j) tile[tid * kParts + (flip ? flip_part(j) : j)] = res[j];
    __syncthreads();
    store_tile(tile, crops + base, npix * kParts, tid);
    __syncthreads();

    // ---- labels (prn_pipeline.py:105-151)
#pragma unroll
    for (int j = 0; j < kParts; ++j) tile[j * kEThreads + tid] = 0.f;
    __syncthreads();
    if (live && tid < kParts) {
        const int32_t* kp = keypoints + ((size_t)e.person * kParts + tid) * 3;   // (y, x, visibility)
        if (kp[2] > 0) {
            const float ymin = boxes[e.person * 4 + 0], xmin = boxes[e.person * 4 + 1];
            const float ymax = boxes[e.person * 4 + 2], xmax = boxes[e.person * 4 + 3];
            const float sy = (float)CH / (ymax - ymin), sx = (float)CW / (xmax - xmin);
            // round half to even, then clip (clipped as floats: equal for every value an int32 holds)
            const float fy = fminf(fmaxf(rintf(((float)kp[0] - ymin) * sy), 0.f), (float)(CH - 1));
            const float fx = fminf(fmaxf(rintf(((float)kp[1] - xmin) * sx), 0.f), (float)(CW - 1));
            const int yy = (int)fy, xx = (int)fx;
            const int q = yy * CW + (flip ? CW - 1 - xx : xx) - t0;
            if (q >= 0 && q < npix) tile[q * kParts + (flip ? flip_part(tid) : tid)] = 1.0f;
        }
    }
    __syncthreads();
    store_tile(tile, labels + base, npix * kParts, tid);
}

}  // namespace

extern "C" size_t mpn_prn_example_desc_bytes(void) { return sizeof(mpn_prn_example_desc); }

extern "C" size_t mpn_prn_examples_workspace_bytes(int total_persons) { return render_tables_bytes(total_persons); }

extern "C" int mpn_prn_examples(const int32_t* keypoints, const float* boxes, int total_persons,
                                const int32_t* first_person, const int32_t* width, const int32_t* height,
                                int num_images, const void* examples, int N, int crop_h, int crop_w, int downsample,
                                float* crops, float* labels, void* workspace, size_t workspace_bytes,
                                mpn_stream_t stream) {
    MPN_REQUIRE(N >= 0, MPN_ERR_BAD_SHAPE, "prn_examples: N must be >= 0 (got %d)", N);
    MPN_REQUIRE(crop_h > 0 && crop_w > 0, MPN_ERR_BAD_SHAPE, "prn_examples: crop size must be positive (got %d x %d)",
                crop_h, crop_w);
    MPN_REQUIRE(total_persons >= 0 && num_images >= 0 && downsample >= 1, MPN_ERR_BAD_SHAPE,
                "prn_examples: bad persons=%d images=%d downsample=%d", total_persons, num_images, downsample);
    MPN_REQUIRE((long long)crop_h * crop_w <= (1 << 20), MPN_ERR_BAD_SHAPE, "prn_examples: crop too large");
    if (N == 0) return MPN_OK;
    const int tiles = mpn_div_up((long long)crop_h * crop_w, kPix);
    MPN_REQUIRE((long long)N * tiles <= 0x7fffffffLL, MPN_ERR_BAD_SHAPE, "prn_examples: N too large");
    MPN_REQUIRE(examples && crops && labels && workspace, MPN_ERR_BAD_ARG, "prn_examples: null pointer");
    MPN_REQUIRE(num_images == 0 || (first_person && width && height), MPN_ERR_BAD_ARG, "prn_examples: null pointer");
    MPN_REQUIRE(total_persons == 0 || (keypoints && boxes), MPN_ERR_BAD_ARG, "prn_examples: null pointer");
    MPN_REQUIRE(mpn_aligned16(crops) && mpn_aligned16(labels) && mpn_aligned16(workspace) && mpn_aligned16(examples),
                MPN_ERR_BAD_ALIGN, "prn_examples: crops, labels, examples and workspace must be 16-byte aligned");
    MPN_REQUIRE(workspace_bytes >= mpn_prn_examples_workspace_bytes(total_persons), MPN_ERR_WORKSPACE,
                "prn_examples: workspace too small (%zu < %zu)", workspace_bytes,
                mpn_prn_examples_workspace_bytes(total_persons));
    hipStream_t st = (hipStream_t)stream;
    const RenderTables t = carve(workspace, total_persons);
    if (total_persons > 0 && num_images > 0) {
        examples_prepare_kernel<<<mpn_div_up((long long)total_persons * kParts, 256), 256, 0, st>>>(
            keypoints, boxes, total_persons, first_person, width, height, num_images, downsample, t);
        MPN_LAUNCH_CHECK();
    }
    examples_kernel<<<(unsigned)(N * tiles), kEThreads, 0, st>>>(
        keypoints, boxes, total_persons, first_person, width, height, num_images,
        reinterpret_cast<const ExampleDesc*>(examples), tiles, crop_h, crop_w, downsample, t, crops, labels);
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
