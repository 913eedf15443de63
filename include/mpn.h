/* libmpn_hip.so - C ABI of the MI355X-native keypoint hot path of MultiPoseNet.
 *
 * The reference (TropComplique/MultiPoseNet) has no FFI of its own: the hot path sits
 * behind plain Python callables that delegate all arithmetic to TensorFlow 1.15 ops.
 * Each entry point below replaces the TF op call sites listed in its comment
 * (paths relative to the reference root), so a maintainer can bind them with ctypes
 * (see INTEGRATION.md).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless marked "host";
 *   - activations are NHWC (channels innermost). The reference computes in NCHW
 *     (detector/constants.py:7) but its API edge is NHWC (images in, heatmaps out);
 *   - `dtype` selects activation storage: MPN_F32 or MPN_BF16 (accumulation is f32);
 *   - parameters, batch-norm statistics, gradients and optimizer state are f32;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), never
 *     synchronises, never allocates: scratch memory comes in through `workspace`;
 *   - return value: 0 = ok, negative = MPN_ERR_*; mpn_last_error() has the text.
 */
#ifndef MPN_H_
#define MPN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPN_VERSION 600   /* r6: see INTEGRATION.md "ABI revisions" */

enum { MPN_F32 = 0, MPN_BF16 = 1, MPN_F16 = 2 /* dense 1x1 / 3x3 convolutions (forward, weight gradient, pack), the PRN entry points and the decode input; the BN / depthwise / loss kernels of the keypoint step take F32 and BF16 only */ };

enum {
    MPN_OK = 0,
    MPN_ERR_BAD_SHAPE = -1,
    MPN_ERR_BAD_DTYPE = -2,
    MPN_ERR_BAD_ALIGN = -3,
    MPN_ERR_HIP = -4,
    MPN_ERR_BAD_ARG = -5,
    MPN_ERR_WORKSPACE = -6,
    MPN_ERR_BAD_DATA = -7   /* host stages that parse a byte stream: the stream is damaged or not supported */
};

/* activation applied after the batch-norm affine */
enum { MPN_ACT_NONE = 0, MPN_ACT_RELU = 1, MPN_ACT_RELU6 = 2 };

typedef void* mpn_stream_t; /* hipStream_t */

int mpn_version(void);
/* copies the calling thread's last error message into buf (host), returns its length */
int mpn_last_error(char* buf, size_t n);

/* ------------------------------------------------------------------------------------
 * K14  heatmap peak decode.
 * Replaces inference/utils.py:29-52 `get_keypoints` (numpy: per-channel max > threshold,
 * first-occurrence argmax, scale into the box, int truncation) for a whole batch, and
 * the tie rule of create_pb.py:120-142 `argmax_2d` (smallest flat index).
 *
 *   heatmaps  [B,h,w,C] NHWC, C == 17, dtype f32 / bf16 / f16
 *   box_hw    [B,2] f64: (height, width) = (ymax-ymin, xmax-xmin) of each image's box
 *   threshold compared as `max > threshold` in f32 (the shim rounds it the way numpy does)
 *   out_xyv   [B,C,3] int32 (x, y, visible) - zeros where the channel is skipped
 *   out_score [B,C] f32 per-channel max (NaN if the channel holds a NaN)   (may be NULL)
 *   out_index [B,C] int32 flat argmax y*w+x of every channel               (may be NULL)
 *   workspace mpn_heatmap_decode_workspace_bytes(B) bytes, ZERO-FILLED once by the
 *             caller when it is allocated; the kernel leaves it zeroed again.
 */
size_t mpn_heatmap_decode_workspace_bytes(int B);
int mpn_heatmap_decode(const void* heatmaps, int dtype, int B, int h, int w, int C,
                       const double* box_hw, float threshold,
                       int32_t* out_xyv, float* out_score, int32_t* out_index,
                       void* workspace, size_t workspace_bytes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K5/K6/K8  dense convolution on the MFMA matrix cores (NHWC, stride 1; 3x3 uses pad 1).
 * Replaces slim.conv2d 1x1 (detector/backbones/mobilenet_v1.py:73) and conv2d_same
 * (detector/utils/layer_utils.py:19-39; call sites detector/fpn.py:38,39,50,52 and
 * detector/keypoint_subnet.py:38,75,77). The same kernel computes data-gradients when it is
 * given weights packed with transpose=1 (flipped taps, Cin/Cout swapped).
 *
 *   x        [N,H,W,Cin]  raw output of the producing conv (or any tensor)
 *   in_scale, in_shift [Cin] f32 or NULL: the producer's batch-norm affine, applied on load
 *            together with in_act (MPN_ACT_*), so normalised activations never touch HBM
 *   w_packed weights from mpn_conv_pack_weights (same dtype as x)
 *   y        [N,H,W,Cout]
 *   stats_part NULL or [mpn_conv_num_parts()][2][Cout] f32: partial sums and sums of squares of y for the
 *            following batch-norm; mpn_conv_stats_rows() rows are written (mpn_bn_finalize reduces them)
 *   up_res   NULL or [N,H/2,W/2,Cout]: y += nearest-2x-upsample(up_res)  (detector/fpn.py:51,58-76)
 */
size_t mpn_conv_packed_bytes(int Cin, int Cout, int ksize, int transpose, int dtype);
/* w_hwio: f32 [ksize,ksize,Cin,Cout] in the reference's variable layout (HWIO) */
int mpn_conv_pack_weights(const float* w_hwio, int Cin, int Cout, int ksize, int transpose,
                          int dtype, void* out, mpn_stream_t stream);
/* Batched packing (one launch for every conv of the network after an optimizer step): fill one host descriptor
 * per (conv, direction) with mpn_conv_pack_desc_fill (returns the job's block count; block_begin = running sum),
 * copy the array to the device once, then launch mpn_conv_pack_weights_batched each step. */
size_t mpn_conv_pack_desc_bytes(void);
int mpn_conv_pack_desc_fill(void* desc_host, const float* w_hwio, int Cin, int Cout, int ksize, int transpose,
                            int dtype, void* out, int block_begin);
int mpn_conv_pack_weights_batched(const void* descs_device, int ndesc, int total_blocks, int dtype,
                                  mpn_stream_t stream);
/* rows to SIZE a statistics slab with: one per 8 x 16-pixel tile (3x3) / per 128 pixels (1x1) */
int mpn_conv_num_parts(int N, int H, int W, int ksize);
/* rows a convolution of this shape WRITES (what mpn_bn_finalize / the finalize descriptors must be given as nparts): the persistent
 * 3x3 kernel (16-bit storage, Cin % 64 == 0, Cout % 64 == 0) sums the rows of a block's tiles and writes one row per block - the same
 * count alone and inside a group -, every other kernel mpn_conv_num_parts rows. Never more than mpn_conv_num_parts; < 0 without a device. */
int mpn_conv_stats_rows(int N, int H, int W, int Cin, int Cout, int ksize, int dtype);
/* x_stride / y_stride: elements between consecutive pixels of x / y; 0 = dense (Cin / Cout). A larger stride reads /
 * writes a channel slice of a wider NHWC tensor in place - phi_subnet_2's second conv writes straight into the first 128
 * channels of the 512-channel concat tensor (keypoint_subnet.py:37: tf.concat with upsample factor 1 is a copy). */
int mpn_conv_fwd(const void* x, const void* w_packed, void* y, int N, int H, int W, int Cin,
                 int Cout, int x_stride, int y_stride, int ksize, int dtype, const float* in_scale,
                 const float* in_shift, int in_act, float* stats_part, const void* up_res,
                 mpn_stream_t stream);
/* Up to five independent 3x3 convolutions of the same channel geometry in ONE grid, largest first (the four pyramid levels
 * of a keypoint-subnet stage, keypoint_subnet.py:64-91: as launches of their own the small levels are latency-bound tails
 * of 15-45 us). Per job: x, w_packed, y, H, W, x_stride / y_stride (arrays or NULL = dense), in_scale / in_shift (or NULL), stats_part
 * (or NULL); shared: N, Cin, Cout, ksize, dtype, in_act. Results are those of mpn_conv_fwd per job, bit for bit;
 * configurations the grouped grid does not cover (f32, 1x1, more than five jobs) run as the separate launches they replace. */
int mpn_conv_fwd_grouped(int njobs, const void* const* x, const void* const* w_packed, void* const* y, int N, const int* H,
                         const int* W, int Cin, int Cout, const int* x_stride, const int* y_stride, int ksize, int dtype,
                         const float* const* in_scale, const float* const* in_shift, int in_act,
                         float* const* stats_part, mpn_stream_t stream);
/* Data gradients of up to five independent 3x3 convolutions in ONE grid (as mpn_conv_fwd_grouped on the transposed packed
 * weights) that ALSO do the first pass of the batch-norm backward of the layer they feed (keypoint_subnet.py:75-78: conv ->
 * bn -> relu -> conv; layer_utils.py:9-16): dx[j] is written MASKED - g = dx where lo < bn_x[j] * bn_scale[j] + bn_shift[j] < hi
 * (the activation bn_act passed), else 0, so mpn_bn_bwd_apply's own mask is a no-op on it - and part[j]
 * ([mpn_conv_num_parts(N,H[j],W[j],3)][2][C] floats, mpn_conv_stats_rows of them written) receives the partial sums of g and of g * bn_x with the RAW x: finish
 * with a finalize built by mpn_bn_bwd_fin_desc_fill_raw. One tensor read and one launch less than mpn_bn_bwd_reduce behind
 * the data gradient. dy [N,H,W,K], dx / bn_x [N,H,W,C] (pixel strides as arrays or NULL = dense); 16-bit storage,
 * K % 64 == 0, K <= 512, C % 64 == 0, C <= 512: mpn_conv_bwd_data_bn_supported(K, C, ksize, dtype) != 0. */
int mpn_conv_bwd_data_bn_supported(int K, int C, int ksize, int dtype);
/* One layer: 3x3 as above, or a 1x1 layer (bf16, K and C multiples of 8: the data gradients of Conv2d_1..13_pointwise, which
 * feed the depthwise layers' batch-norms, mobilenet_v1.py:66-74, and of the FPN's lateral of c5, fpn.py:38) - through the GEMM
 * kernel where mpn_conv_fwd routes the geometry there, else the tiled kernel. part: [mpn_conv_num_parts(N,H,W,ksize)][2][C] (mpn_conv_stats_rows written);
 * finish with mpn_bn_bwd_finalize_raw. */
int mpn_conv_bwd_data_bn(const void* dy, const void* w_packed_t, void* dx, int N, int H, int W, int K, int C, int dy_stride,
                         int dx_stride, int ksize, int dtype, const void* bn_x, int bn_x_stride, const float* bn_scale,
                         const float* bn_shift, int bn_act, float* part, mpn_stream_t stream);
int mpn_conv_bwd_data_bn_grouped(int njobs, const void* const* dy, const void* const* w_packed_t, void* const* dx, int N,
                                 const int* H, const int* W, int K, int C, const int* dy_stride, const int* dx_stride,
                                 int dtype, const void* const* bn_x, const int* bn_x_stride, const float* const* bn_scale,
                                 const float* const* bn_shift, int bn_act, float* const* part, mpn_stream_t stream);

/* Weight gradient of mpn_conv_fwd: dW[tap][ci][co] = sum_pixels act(bn(x))[pixel+tap][ci]*dy[pixel][co].
 * Split-K over pixel tiles: part [mpn_conv_wgrad_num_parts()][ksize*ksize][Cin][Cout] f32 (one HWIO slab
 * per split), summed in a fixed order by mpn_reduce_partials. */
int mpn_conv_wgrad_num_parts(int N, int H, int W, int Cin, int Cout, int ksize, int dtype);
/* x_stride / dy_stride: pixel strides in elements, 0 = dense (channel slices of wider tensors, as for mpn_conv_fwd) */
int mpn_conv_bwd_weight(const void* x, const void* dy, float* part, int N, int H, int W, int Cin,
                        int Cout, int x_stride, int dy_stride, int ksize, int dtype, const float* in_scale,
                        const float* in_shift, int in_act, mpn_stream_t stream);

/* A thin 1x1 convolution's backward in ONE pass over x and dy (Cin <= 128, Cout <= 128, bf16: Conv2d_1..3_pointwise,
 * /root/reference/detector/backbones/mobilenet_v1.py:66-74: tf.gradients of slim.conv2d w.r.t. its kernel and its input, and the
 * reduction of the batch-norm below, mobilenet_v1.py:29-38): wpart [mpn_conv_wgrad_num_parts(N,H,W,Cin,Cout,1,dtype)][Cin][Cout] =
 * weight-gradient partials over act(x * in_scale + in_shift) (finish with mpn_reduce_partials); dx [N,H,W,Cin] = dy . w^T MASKED by that
 * activation (lo < x * in_scale + in_shift < hi on the raw x); bn_part [same rows][2][Cin] = partial sums of the masked gradient g and
 * of g * x with the RAW x (finish with mpn_bn_bwd_finalize_raw). What mpn_conv_bwd_weight + mpn_conv_bwd_data_bn give in two passes over
 * both tensors. bn_part == NULL: no reduction and dx is the plain, unmasked data gradient (an FPN lateral, /root/reference/detector/fpn.py:36-47).
 * w: the layer's f32 kernel [Cin][Cout] (HWIO of a 1x1). Strides in elements, 0 = dense. dx must not alias x or dy. */
int mpn_conv1x1_bwd_fused_supported(int Cin, int Cout, int dtype);
int mpn_conv1x1_bwd_fused(const void* x, const void* dy, const float* w, void* dx, float* wpart, float* bn_part, int N, int H, int W,
                          int Cin, int Cout, int x_stride, int dy_stride, int dx_stride, int dtype, const float* in_scale,
                          const float* in_shift, int in_act, mpn_stream_t stream);
/* ... with the batch-norm backward APPLY pass of the layer's OWN batch-norm folded into the staging of dY (Cin <= 64, Cout <= 128):
 * g = the gradient w.r.t. the layer's activated output (what mpn_bn_bwd_apply would turn into dy in place),
 * y_raw = the layer's raw output, ap_* that batch-norm's affine, saved statistics and the k1 / k2 of mpn_bn_bwd_finalize. The slabs and dx of
 * mpn_bn_bwd_apply followed by mpn_conv1x1_bwd_fused (to the storage rounding of a rare staged element); g and y_raw are not written. */
int mpn_conv1x1_bwd_fused_apply_supported(int Cin, int Cout, int dtype);
int mpn_conv1x1_bwd_fused_apply(const void* x, const void* g, const void* y_raw, const float* w, void* dx, float* wpart, float* bn_part,
                                int N, int H, int W, int Cin, int Cout, int x_stride, int g_stride, int y_stride, int dx_stride,
                                int dtype, const float* in_scale, const float* in_shift, int in_act, const float* ap_scale,
                                const float* ap_shift, const float* ap_mean, const float* ap_invstd, const float* ap_k1,
                                const float* ap_k2, int ap_act, mpn_stream_t stream);
/* The weight gradients of njobs independent layers of one (Cin, Cout, ksize, dtype) in ONE grid - the pyramid levels of a
 * subnet stage (keypoint_subnet.py:66-79: one phi_subnet per level; fpn.py:38-52: one 3x3 per level). The 256 blocks are
 * divided among the jobs by their pixel counts, so a stage leaves 128 partial slabs in all instead of 128 per level, and the
 * small levels stop being latency-bound launches of their own. mpn_conv_wgrad_grouped_num_parts fills nparts[j] (the slab
 * count of job j in THAT grid; f32 / more than 5 jobs: the counts of the separate launches, which the grouped call then
 * performs); part[j]: [nparts[j]][ksize*ksize][Cin][Cout] f32. Arrays of njobs entries; x_stride / dy_stride may be NULL. */
int mpn_conv_wgrad_grouped_num_parts(int njobs, int N, const int* H, const int* W, int Cin, int Cout, int ksize, int dtype,
                                     int* nparts);
int mpn_conv_bwd_weight_grouped(int njobs, const void* const* x, const void* const* dy, float* const* part, int N,
                                const int* H, const int* W, int Cin, int Cout, const int* x_stride, const int* dy_stride,
                                int ksize, int dtype, const float* const* in_scale, const float* const* in_shift,
                                int in_act, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K4  batch normalisation (tf.layers.batch_normalization(fused=True, momentum=.95, eps=1e-3):
 * detector/backbones/mobilenet_v1.py:29-38, detector/utils/layer_utils.py:9-16).
 * Producers emit partial sums [nparts][2][C] (sum, sum of squares); mpn_bn_finalize turns them
 * into the per-channel affine (scale = gamma*invstd, shift = beta - mean*scale) that CONSUMERS
 * apply on load, and updates the moving statistics (unbiased variance, TF-1.15 semantic) when
 * moving_mean/moving_var are non-NULL. x is viewed as [M rows][C channels] (NHWC).
 */
/* (The finalizes take `part` as SCRATCH: from 4096 partial rows on they first add groups of 32 consecutive rows in place -
 * a 1x1 layer at 256 x 256 leaves 16 384 rows, a 45-55 us finalize in a handful of blocks otherwise. The slab's contents are
 * consumed; results do not depend on the launch (fixed orders, no atomics).) */
int mpn_bn_stats_num_parts(long long M);
int mpn_bn_stats(const void* x, long long M, int C, int dtype, float* part, mpn_stream_t stream);
int mpn_bn_finalize(float* part, int nparts, int C, long long count, const float* gamma,
                    const float* beta, float* moving_mean, float* moving_var, float momentum,
                    float eps, float* scale, float* shift, float* save_mean, float* save_invstd,
                    mpn_stream_t stream);
/* is_training=False path: affine from the moving statistics */
/* The two backward passes of up to five independent layers of one channel count in ONE grid each, largest first (the
 * pyramid levels of a subnet stage). Arrays per job; results are those of mpn_bn_bwd_reduce / mpn_bn_bwd_apply per layer,
 * bit for bit; part[j] holds mpn_bn_stats_num_parts(M[j]) rows. dA_stride / x_stride (arrays or NULL = dense): elements
 * between consecutive rows of dA[j] / x[j] - the level-2 tensors of phi_subnet's second batch-norm live in channel slices
 * of the 512-channel concat tensor and of its gradient (keypoint_subnet.py:37). */
int mpn_bn_bwd_reduce_grouped(int njobs, void* const* dA, const void* const* x, const long long* M, int C, int dtype,
                              const float* const* scale, const float* const* shift, const float* const* mean,
                              const float* const* invstd, int act, float* const* part, const int* dA_stride,
                              const int* x_stride, mpn_stream_t stream);
int mpn_bn_bwd_apply_grouped(int njobs, void* const* dA, const void* const* x, const long long* M, int C, int dtype,
                             const float* const* scale, const float* const* shift, const float* const* mean,
                             const float* const* invstd, const float* const* k1, const float* const* k2, int act,
                             const float* const* add_ch0, const int* dA_stride, const int* x_stride,
                             mpn_stream_t stream);
/* Several independent layers' finalizes in ONE launch (the four pyramid levels of the keypoint subnet,
 * keypoint_subnet.py:64-91, produce their statistics side by side). Descriptor tables as for the batched slab reduction:
 * mpn_bn_fin_desc_fill / mpn_bn_bwd_fin_desc_fill write one host-side descriptor each (mpn_*_desc_bytes() bytes; return the
 * number of blocks of the job, -1 on bad arguments; block_begin = running sum); the caller copies the array to the device
 * once. Same arithmetic, bit for bit, as mpn_bn_finalize / mpn_bn_bwd_finalize per layer BELOW 4096 partial rows; from 4096 rows
 * on the per-layer entry points first add groups of 32 rows in place (f64 inside a group, the group's sum rounded to f32: `part`
 * is scratch and is DESTROYED - finalizing the same slab twice double-counts), which the batched kernels do not: the two then
 * agree to f32 rounding of the group sums (tests/test_ops_bwd_gpu.py::test_batched_and_per_layer_finalize_from_4096_rows). */
size_t mpn_bn_fin_desc_bytes(void);
size_t mpn_bn_bwd_fin_desc_bytes(void);
int mpn_bn_fin_desc_fill(void* desc_host, const float* part, int nparts, int C, long long count, const float* gamma,
                         const float* beta, float* moving_mean, float* moving_var, float* scale, float* shift,
                         float* save_mean, float* save_invstd, int block_begin);
int mpn_bn_bwd_fin_desc_fill(void* desc_host, const float* part, int nparts, int C, long long count, float* dgamma,
                             float* dbeta, float* k1, float* k2, int block_begin);
/* The same for a slab whose second row holds sum g * x with the RAW x (mpn_conv_bwd_data_bn_grouped): mean / invstd = the
 * layer's saved batch statistics; the finalize forms sum g * xhat = invstd * (sum g x - mean * sum g) in f64. */
int mpn_bn_bwd_fin_desc_fill_raw(void* desc_host, const float* part, int nparts, int C, long long count, float* dgamma,
                                 float* dbeta, float* k1, float* k2, const float* mean, const float* invstd,
                                 int block_begin);
int mpn_bn_finalize_batched(const void* descs_device, int ndesc, int total_blocks, float momentum, float eps,
                            mpn_stream_t stream);
int mpn_bn_bwd_finalize_batched(const void* descs_device, int ndesc, int total_blocks, mpn_stream_t stream);
int mpn_bn_inference_affine(int C, const float* gamma, const float* beta, const float* moving_mean,
                            const float* moving_var, float eps, float* scale, float* shift,
                            mpn_stream_t stream);
/* y = act(x*scale + shift), materialised (only needed at the API edge) */
int mpn_bn_act_apply(const void* x, void* y, long long M, int C, int dtype, const float* scale,
                     const float* shift, int act, mpn_stream_t stream);
/* backward: g = dA*act'(.), partials of sum(g), sum(g*xhat) -> [mpn_bn_stats_num_parts(M)][2][C] */
int mpn_bn_bwd_reduce(const void* dA, const void* x, long long M, int C, int dtype,
                      const float* scale, const float* shift, const float* mean,
                      const float* invstd, int act, float* part, mpn_stream_t stream);
int mpn_bn_bwd_finalize(float* part, int nparts, int C, long long count, float* dgamma,
                        float* dbeta, float* k1, float* k2, mpn_stream_t stream);
/* mpn_bn_bwd_finalize for a slab whose second row holds sum g * x with the RAW x (mpn_conv_bwd_data_bn): mean / invstd = the
 * layer's saved batch statistics. */
int mpn_bn_bwd_finalize_raw(float* part, int nparts, int C, long long count, float* dgamma, float* dbeta, float* k1,
                            float* k2, const float* mean, const float* invstd, mpn_stream_t stream);
/* dA <- scale*(g - k1 - xhat*k2) in place; add_ch0 (NULL or [M] f32) is added to channel 0 */
int mpn_bn_bwd_apply(void* dA, const void* x, long long M, int C, int dtype, const float* scale,
                     const float* shift, const float* mean, const float* invstd, const float* k1,
                     const float* k2, int act, const float* add_ch0, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K3  depthwise 3x3, TF 'SAME' padding, stride 1|2 (tf.nn.depthwise_conv2d,
 * detector/backbones/mobilenet_v1.py:82-104). w = `depthwise_weights` [3,3,C,1] f32 as is.
 * x [N,H,W,C] -> y [N,OH,OW,C], OH = ceil(H/stride). in_scale/in_shift/in_act as for mpn_conv_fwd.
 * stats_part: NULL or [mpn_dwconv_num_parts()][2][C].
 */
int mpn_dwconv_out_size(int size, int stride);
int mpn_dwconv_num_parts(int N, int H, int W, int C, int stride, int dtype);
int mpn_dwconv_fwd(const void* x, const float* w, void* y, int N, int H, int W, int C, int stride,
                   int dtype, const float* in_scale, const float* in_shift, int in_act, int flip,
                   float* stats_part, mpn_stream_t stream);
/* dy [N,OH,OW,C] -> dx [N,H,W,C]  (H, W: forward input size) */
int mpn_dwconv_bwd_data(const void* dy, const float* w, void* dx, int N, int H, int W, int C,
                        int stride, int dtype, mpn_stream_t stream);
/* The same with the batch-norm backward REDUCTION of the layer that dx feeds fused in (the pointwise conv + batch-norm whose
 * activated output the depthwise conv read, mobilenet_v1.py:88-110): dx is that layer's dA, x_bn its raw conv output
 * [N,H,W,C]; part [mpn_dwconv_bwd_data_bn_num_parts][2][C] receives sum(g) and sum(g*xhat) per block in the layout of
 * mpn_bn_bwd_reduce (finish with mpn_bn_bwd_finalize(part, rows, C, N*H*W, ...), then mpn_bn_bwd_apply) - one tensor read
 * and one launch less than reducing afterwards. num_parts == 0: not available for this shape (odd H / W at stride 2). */
int mpn_dwconv_bwd_data_bn_num_parts(int N, int H, int W, int C, int stride, int dtype);
int mpn_dwconv_bwd_data_bn(const void* dy, const float* w, void* dx, int N, int H, int W, int C, int stride, int dtype,
                           const void* x_bn, const float* scale, const float* shift, const float* mean,
                           const float* invstd, int act, float* part, mpn_stream_t stream);
/* dx = data gradient + addend, addend [N,H,W,C] of dx's type and not aliasing it: the gradient an FPN lateral sends into
 * the same backbone feature map (the sum of the two consumers of c2..c4, mobilenet_v1.py:76-79 / fpn.py:48) - one read
 * instead of a separate read-modify-write pass and a single rounding of the sum. x_bn != NULL: also the batch-norm
 * backward reduction of mpn_dwconv_bwd_data_bn, over the SUM (part: mpn_dwconv_bwd_data_bn_num_parts rows); x_bn == NULL:
 * scale .. part are ignored. Stride-2 layers with even H, W only (mpn_dwconv_bwd_data_add_supported == 1). */
int mpn_dwconv_bwd_data_add_supported(int N, int H, int W, int C, int stride, int dtype);
int mpn_dwconv_bwd_data_add(const void* dy, const float* w, void* dx, int N, int H, int W, int C, int stride, int dtype,
                            const void* addend, const void* x_bn, const float* scale, const float* shift,
                            const float* mean, const float* invstd, int act, float* part, mpn_stream_t stream);
int mpn_dwconv_wgrad_num_parts(int N, int H, int W, int C, int stride, int dtype);
/* part [mpn_dwconv_wgrad_num_parts()][9][C]; finish with mpn_reduce_partials */
int mpn_dwconv_bwd_weight(const void* x, const void* dy, float* part, int N, int H, int W, int C,
                          int stride, int dtype, const float* in_scale, const float* in_shift,
                          int in_act, mpn_stream_t stream);

/* Stride-1 depthwise backward in ONE pass over dy, x and dx - both gradients of tf.nn.depthwise_conv2d
 * (/root/reference/detector/backbones/mobilenet_v1.py:101) and the batch-norm backward reduction of the layer that produced x
 * (mobilenet_v1.py:29-38): dx [N,H,W,C] = data gradient; wpart [mpn_dwconv_wgrad_num_parts][9][C] = weight-gradient partials over
 * act(x * in_scale + in_shift) (finish with mpn_reduce_partials); bn_part (NULL: no reduction) [mpn_dwconv_wgrad_num_parts][2][C] =
 * sum(g), sum(g * xhat) with g = dx where in_act passes, xhat = (x - mean) * invstd (finish with mpn_bn_bwd_finalize). Replaces
 * mpn_dwconv_bwd_weight + mpn_dwconv_bwd_data_bn (five tensor passes) by three. dx must not alias x or dy. */
int mpn_dwconv_bwd_fused_supported(int N, int H, int W, int C, int stride, int dtype);
int mpn_dwconv_bwd_fused(const void* x, const void* dy, const float* w, void* dx, float* wpart, int N, int H, int W, int C,
                         int dtype, const float* in_scale, const float* in_shift, int in_act, const float* mean,
                         const float* invstd, float* bn_part, mpn_stream_t stream);
/* The stride-2 counterpart (even H and W; mpn_dwconv_bwd_fused_supported(.., 2, ..) == 1): dy [N,H/2,W/2,C]; dx [N,H,W,C] = data gradient
 * (+ addend when not NULL: a tensor of dx's shape - the FPN lateral's gradient into the same backbone feature map - added before
 * the store and before the reduction, as mpn_dwconv_bwd_data_add does); wpart [mpn_dwconv_wgrad_num_parts(.., 2, ..)][9][C]; bn_part
 * (NULL: no reduction) [same rows][2][C]. The input and dy are read once instead of twice. dx must not alias x, dy or addend. */
int mpn_dwconv_bwd_fused_s2(const void* x, const void* dy, const float* w, void* dx, float* wpart, int N, int H, int W, int C,
                            int dtype, const float* in_scale, const float* in_shift, int in_act, const float* mean,
                            const float* invstd, float* bn_part, const void* addend, mpn_stream_t stream);
/* ... with the backward APPLY pass of the depthwise conv's OWN batch-norm folded into the loads of dy (16-bit storage;
 * mpn_dwconv_bwd_fused_apply_supported == 1: the shapes of mpn_dwconv_bwd_fused_supported, 0 for f32): g [dy's shape] = the gradient that
 * mpn_bn_bwd_apply would turn into dy in place, y_raw = the conv's raw output (same shape), ap_* that batch-norm's affine, saved
 * statistics and the k1 / k2 of mpn_bn_bwd_finalize. dx, wpart and bn_part are those of mpn_bn_bwd_apply followed by
 * mpn_dwconv_bwd_fused[_s2], bit for bit; g and y_raw are not written. CONTRACT: g is already zero where ap_act blocks
 * y_raw * ap_scale + ap_shift - the producers that reduce for this batch-norm (mpn_conv_bwd_data_bn, mpn_conv1x1_bwd_fused) write it
 * so; the walk does not repeat the test (ap_shift and ap_act describe the batch-norm and are not read). */
int mpn_dwconv_bwd_fused_apply_supported(int N, int H, int W, int C, int stride, int dtype);
int mpn_dwconv_bwd_fused_apply(const void* x, const void* g, const void* y_raw, const float* w, void* dx, float* wpart, int N, int H,
                               int W, int C, int dtype, const float* in_scale, const float* in_shift, int in_act, const float* mean,
                               const float* invstd, float* bn_part, const float* ap_scale, const float* ap_shift,
                               const float* ap_mean, const float* ap_invstd, const float* ap_k1, const float* ap_k2, int ap_act,
                               mpn_stream_t stream);
int mpn_dwconv_bwd_fused_s2_apply(const void* x, const void* g, const void* y_raw, const float* w, void* dx, float* wpart, int N, int H,
                                  int W, int C, int dtype, const float* in_scale, const float* in_shift, int in_act,
                                  const float* mean, const float* invstd, float* bn_part, const void* addend, const float* ap_scale,
                                  const float* ap_shift, const float* ap_mean, const float* ap_invstd, const float* ap_k1,
                                  const float* ap_k2, int ap_act, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K1+K2  `2*x-1` + Conv2d_0 (3x3 stride 2 'SAME', 3 -> C0) fused
 * (detector/backbones/mobilenet_v1.py:41,53,56). images NHWC f32 in [0,1], or uint8
 * (images_u8=1: scaled by 1/255 first, create_pb.py:167). w = `Conv2d_0/weights` [3,3,3,C0] f32.
 */
int mpn_stem_conv_fwd(const void* images, int images_u8, const float* w, void* y, int N, int H,
                      int W, int C0, int dtype, mpn_stream_t stream);
/* The same + the batch-norm statistics of the (rounded) output, fused into the kernel's copy-out: stats_part
 * [mpn_stem_conv_fwd_num_parts()][2][C0] receives per-tile sum / sum of squares in the layout of mpn_bn_stats (finish with
 * mpn_bn_finalize; mobilenet_v1.py:56 applies batch-norm to Conv2d_0). num_parts == 0: not available for this C0 - run
 * mpn_bn_stats on the output instead. stats_part == NULL: plain forward. */
int mpn_stem_conv_fwd_num_parts(int N, int H, int W, int C0, int dtype);
int mpn_stem_conv_fwd_stats(const void* images, int images_u8, const float* w, void* y, int N, int H, int W, int C0,
                            int dtype, float* stats_part, mpn_stream_t stream);
int mpn_stem_conv_wgrad_num_parts(int N, int H, int W);
/* part [num_parts][27*C0] */
int mpn_stem_conv_bwd_weight(const void* images, int images_u8, const void* dy, float* part, int N,
                             int H, int W, int C0, int dtype, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K9/K10  legacy bilinear up-sampling by an integer factor into a channel slice of the concat
 * tensor (tf.image.resize_bilinear + tf.concat, detector/keypoint_subnet.py:37,86), its transpose,
 * and the gradient of the FPN's nearest-2x upsample (detector/fpn.py:58-76).
 */
int mpn_bilinear_up_fwd(const void* x, void* y, int N, int h, int w, int C, int upsample,
                        int y_channel_offset, int y_channels_total, int dtype,
                        const float* in_scale, const float* in_shift, int in_act,
                        mpn_stream_t stream);
int mpn_bilinear_up_bwd(const void* dy, void* dx, int N, int h, int w, int C, int upsample,
                        int y_channel_offset, int y_channels_total, int dtype, mpn_stream_t stream);
/* src [N,2h,2w,C] -> dst [N,h,w,C] (2x2 sums); accumulate != 0 adds into dst */
int mpn_sumpool2x2(const void* src, void* dst, int N, int h, int w, int C, int accumulate,
                   int dtype, mpn_stream_t stream);
/* dst += src over n elements: joins the two gradient paths that meet at c2..c4 */
int mpn_add_inplace(void* dst, const void* src, long long n, int dtype, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K11  `heatmaps` head: 1x1 conv Cin -> 18 + bias, f32 NHWC logits
 * (detector/keypoint_subnet.py:49-58); mode 1 = inference post-ops of create_pb.py:73-76.
 * w = `heatmaps/kernel` [1,1,Cin,18] f32, bias [18].
 */
int mpn_heatmap_head_fwd(const void* x, const float* w, const float* bias, long long M, int Cin,
                         int dtype, const float* in_scale, const float* in_shift, int in_act,
                         int mode, float* out, float* out_seg, mpn_stream_t stream);
int mpn_heatmap_head_bwd_num_parts(long long M);
/* dA [M][Cin]; part [num_parts][Cin*18 + 18] (dW then db) */
int mpn_heatmap_head_bwd(const void* x, const float* dlogits, const float* w, long long M, int Cin,
                         int dtype, const float* in_scale, const float* in_shift, int in_act,
                         void* dA, float* part, mpn_stream_t stream);
/* The same with the reduction pass of the batch-norm the head reads through (final_bn, keypoint_subnet.py:42-47) fused in:
 * dA comes out masked by that layer's activation and bn_part [mpn_heatmap_head_bwd_num_parts(M)][2][Cin] receives per-block
 * sums of g and g * x (raw x); finish with mpn_bn_bwd_finalize_raw + mpn_bn_bwd_apply. bf16, Cin = 16 / 32 / 64
 * (mpn_heatmap_head_bwd_bn_supported). */
int mpn_heatmap_head_bwd_bn_supported(int Cin, int dtype);
int mpn_heatmap_head_bwd_bn(const void* x, const float* dlogits, const float* w, long long M, int Cin, int dtype,
                            const float* in_scale, const float* in_shift, int in_act, void* dA, float* part,
                            float* bn_part, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K12  fused losses + gradients (keypoints_model.py:43-90,141-178).
 * losses_out[8] = focal, regression, seg@2, seg@3, seg@4, seg@5, total, per_pixel_reg_loss.
 * dlogits / daux* may be NULL (evaluation). part: [mpn_keypoint_loss_num_parts()][8].
 */
int mpn_keypoint_loss_num_parts(int B, int h, int w);
int mpn_keypoint_loss(const float* logits, const float* heatmaps, const float* loss_masks,
                      const float* segmentation_masks, const int* num_boxes, const void* p2,
                      const void* p3, const void* p4, const void* p5, int p_channels, int p_dtype,
                      float* dlogits, float* daux2, float* daux3, float* daux4, float* daux5,
                      float* part, float* losses_out, int B, int h, int w, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K13  optimizer step (keypoints_model.py:107-120): cosine-decayed learning rate,
 * tf.clip_by_value(g,-200,200), TF-1.15 Adam over a flat f32 arena. `step` (device int64 global
 * step, incremented by mpn_adam_prepare) and `hyper` (device f32[4]: lr_t, lr) stay on the
 * device so the whole step replays from a hipGraph.
 */
int mpn_adam_prepare(long long* step, float* hyper, double initial_learning_rate,
                     double decay_steps, double alpha, double beta1, double beta2,
                     mpn_stream_t stream);
int mpn_adam_step(float* params, const float* grads, float* m, float* v, long long n,
                  const float* hyper, float beta1, float beta2, float eps, float clip,
                  float grad_scale, mpn_stream_t stream);
/* mpn_adam_step that also writes 16-bit copies (fp16 / bf16 by cast_dtype) of up to 4 ranges of the UPDATED arena:
 * cast_dst[r][i] = (T) params[cast_begin[r] + i], i < cast_count[r] - the storage-dtype GEMM operand of a dense layer without a
 * second pass over its f32 master. begin / count multiples of 4, dst 8-byte aligned. */
int mpn_adam_step_cast(float* params, const float* grads, float* m, float* v, long long n, const float* hyper, float beta1,
                       float beta2, float eps, float clip, float grad_scale, int ncast, const long long* cast_begin,
                       const long long* cast_count, void* const* cast_dst, int cast_dtype, mpn_stream_t stream);
/* out[j] (+)= scale * sum_p part[p][j] in a fixed order (deterministic). `part` is scratch: large slabs are
 * reduced in two passes and the first pass folds range sums into the slab itself (its contents are clobbered). */
int mpn_reduce_partials(const float* part, int nparts, long long n, float* out, int accumulate,
                        float scale, mpn_stream_t stream);
/* All slab reductions of a training step in ONE launch (every weight-gradient kernel leaves a slab; 46 per step).
 * mpn_reduce_desc_fill writes one host-side job descriptor (mpn_reduce_desc_bytes() bytes; block_begin = running sum
 * of the returned block counts), the caller copies the table to the device once, mpn_reduce_partials_batched runs
 * out[j] = scale * sum_p part[p][j] for every job (fixed summation order; slabs are left intact). */
size_t mpn_reduce_desc_bytes(void);
int mpn_reduce_desc_fill(void* desc_host, const float* part, int nparts, long long n, float* out, float scale,
                         int block_begin);
int mpn_reduce_partials_batched(const void* descs_device, int ndesc, int total_blocks, mpn_stream_t stream);
int mpn_axpy(long long n, float a, const float* x, float* y, mpn_stream_t stream);
/* y[t][i] += a * x[t][i] over `count` tensors (host arrays of device pointers / element counts), one launch per 64 tensors:
 * the gradient of add_weight_decay's term for every regularised variable at once (keypoints_model.py:129-138). */
int mpn_axpy_batched(int count, const float* const* x, float* const* y, const long long* n, float a, mpn_stream_t stream);
/* acc[0] += scale * sum(w^2)/2 - `weight_decay * tf.nn.l2_loss(k)` of add_weight_decay (keypoints_model.py:129-138), the
 * term tf.losses.get_total_loss(add_regularization_losses=True) adds to the reported loss (keypoints_model.py:79).
 * One block, fixed summation order (f64): deterministic. */
int mpn_l2_loss_accumulate(long long n, const float* w, float scale, float* acc, mpn_stream_t stream);
/* The same over `count` tensors (host arrays of device pointers / element counts) in two launches: per-block f64 partial sums
 * into `workspace` (mpn_l2_loss_batched_workspace_bytes bytes), then one block adds them in a fixed order - the whole
 * regularisation term of a model (keypoints_model.py:129-138 sums every kernel) without one single-block launch per variable. */
size_t mpn_l2_loss_batched_workspace_bytes(int count, const long long* n);
int mpn_l2_loss_batched(int count, const float* const* w, const long long* n, float scale, float* acc, void* workspace,
                        size_t workspace_bytes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * L1  target-heatmap rendering (label producer of the keypoint path).
 * Replaces detector/input_pipeline/heatmap_creation.py:6-72 `get_heatmaps` (+ `get_kernel`
 * :75-86, `create_heatmap` :89-118), which the reference runs per image under the GIL via
 * tf.py_func (keypoints_detector_pipeline.py:86-90, prn_pipeline.py:91-95), for a whole
 * batch of equally sized images in one launch:
 *
 *   out[b,y,x,j] = max(0, max over visible persons p of image b of
 *                         float32(g_p[|y-cy_pj|] * g_p[|x-cx_pj|]),  |dy|,|dx| <= k_p)
 *   sigma_p = clip(0.007f * sqrtf(box area), 1, 4)            (float32, :33-37)
 *   k_p     = ceil(sqrt(-2 sigma^2 ln 0.01)), g_p[d] = exp(-d^2 / (2 sigma^2))  (float64, :78-84)
 *   cy, cx  = rint(float32(y / (height-1)) * (h-1)), likewise x  (:23-24,57,104-107)
 * Bit-identical to the reference (tests/golden/render_goldens.npz); peaks are exactly 1.0f.
 *
 *   keypoints    [P,17,3] int32 (y, x, visibility), persons of all images concatenated
 *   boxes        [P,4] f32 (ymin, xmin, ymax, xmax), absolute
 *   first_person [B+1] int32, device: persons of image b are first_person[b] .. first_person[b+1]-1
 *   width,height size of the (equally sized) images; h = ceil(height/downsample), w likewise
 *   out          [B,h,w,17] f32, every element written
 *   workspace    mpn_heatmap_render_workspace_bytes(P) bytes of scratch (no initialisation needed)
 * A blob whose centre lies outside the map is clipped (the numpy code raises or wraps there).
 */
size_t mpn_heatmap_render_workspace_bytes(int total_persons);
int mpn_heatmap_render(const int32_t* keypoints, const float* boxes, const int32_t* first_person,
                       int B, int total_persons, int width, int height, int downsample, float* out,
                       void* workspace, size_t workspace_bytes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * L2  keypoint input augmentation (the per-pixel half of the training / evaluation input pipeline).
 * Replaces the image and mask operations of detector/input_pipeline/keypoints_detector_pipeline.py
 * `augmentation` (:191-197: random_rotation.py:68-77, `randomly_crop_and_resize` :275-400,
 * color_augmentations.py:10-69, `random_flip_left_right` :403-450) and `resize_keeping_aspect_ratio`
 * (:200-272) for a batch of RAGGED uint8 sources in one launch. The host draws every random decision
 * and fills one descriptor per image (multiposenet_amd/detector/input_pipeline/keypoint_augment.py);
 * per output pixel (y, x), with p = flip ? W-1-x : x the position before the flip:
 *
 *   valid      p < valid_w and y < valid_h, else 0                        (pad_to_bounding_box, :243)
 *   resize     legacy bilinear over the crop: in = out * scale (f32 in/out), lo = floor(in),
 *              hi = min(lo+1, crop-1), top + (bottom-top)*y_lerp           (resize_images, :241, :363)
 *   tap        rotated image at (crop_y + row, crop_x + col): ImageProjectiveTransform BILINEAR of
 *              u8 * float32(1/255) with `transform`, corners floor / floor+1, 0 outside  (random_rotation.py:69)
 *   colour     clip(v + color[c], 0, 1)                                    (color_augmentations.py:19-33)
 *   grayscale  0.2989 r + 0.5870 g + 0.1140 b on all channels              (:35-38)
 *   scale      clip(v * (u * (1.1f - 0.9f) + 0.9f), 0, 1),
 *              u = (fmix32(seed ^ (idx * 0x9E3779B1)) >> 8) * 2^-24, idx = (y*W + p)*3 + c,
 *              fmix32 = murmur3's finaliser                                (color_augmentations.py:47-69)
 *   masks      training: crop_and_resize nearest of `window` over the rotated mask
 *              (in = y1*(mh-1) + y*(y2-y1)*(mh-1)/(H/4-1), roundf, 0 outside; the rotation is
 *              NEAREST with `mask_transform`, fill 0); evaluation (MPN_AUGMENT_EVAL): legacy
 *              resize_nearest_neighbor min(floor(out * mask_scale), in-1) inside valid_m*, 0 outside
 * Every float step is one IEEE round-to-nearest operation in that order (no contraction).
 *
 *   sources    concatenated uint8 RGB images [src_h, src_w, 3]; image b starts at byte src_offset
 *   masks      concatenated np.packbits of [ceil(src_h/4), ceil(src_w/4), 2] (0 loss, 1 segmentation)
 *   descs      [B] mpn_keypoint_augment_desc, DEVICE, 16-byte aligned
 *   images     [B,H,W,3] f32, 16-byte aligned; loss_masks, segmentation_masks [B,H/4,W/4] f32
 * B >= 1, H % 4 == 0, W % 4 == 0. Every output element is written. Descriptor fields are the caller's
 * to check (offsets and sizes inside the buffers); a source read outside an image's own rectangle
 * returns 0. mpn_keypoint_augment_desc_bytes() = sizeof(mpn_keypoint_augment_desc), for bindings.
 */
enum {
    MPN_AUGMENT_ROTATE = 1, MPN_AUGMENT_COLOR = 2, MPN_AUGMENT_GRAYSCALE = 4, MPN_AUGMENT_PIXEL_SCALE = 8,
    MPN_AUGMENT_FLIP = 16, MPN_AUGMENT_EVAL = 32
};
#define MPN_KEYPOINT_AUGMENT_DESC_BYTES 192
typedef struct mpn_keypoint_augment_desc {
    int64_t src_offset, mask_offset;            /* byte offsets into sources / masks */
    int32_t src_h, src_w, mask_h, mask_w;       /* mask_h = ceil(src_h/4), mask_w = ceil(src_w/4) */
    int32_t crop_y, crop_x, crop_h, crop_w;     /* integer crop of the rotated image (begin, size) */
    int32_t valid_h, valid_w, valid_mh, valid_mw; /* output region before the zero padding */
    float transform[8], mask_transform[8];      /* inverse projective transforms (MPN_AUGMENT_ROTATE) */
    float window[4];                            /* normalised crop window (ymin, xmin, ymax, xmax) for masks */
    float scale_y, scale_x;                     /* f32(crop_h)/f32(valid_h), f32(crop_w)/f32(valid_w) */
    float mask_scale_y, mask_scale_x;           /* f32(mask_h)/f32(valid_mh), likewise (MPN_AUGMENT_EVAL) */
    float color[3];                             /* per-channel offsets (MPN_AUGMENT_COLOR) */
    uint32_t seed;                              /* pixel-scale hash seed (MPN_AUGMENT_PIXEL_SCALE) */
    int32_t flags;                              /* MPN_AUGMENT_* */
    int32_t reserved[3];
} mpn_keypoint_augment_desc;
#ifdef __cplusplus
static_assert(sizeof(mpn_keypoint_augment_desc) == MPN_KEYPOINT_AUGMENT_DESC_BYTES, "descriptor size is fixed");
#endif
size_t mpn_keypoint_augment_desc_bytes(void);
int mpn_keypoint_augment(const uint8_t* sources, const uint8_t* masks, const void* descs, int B, int H, int W,
                         float* images, float* loss_masks, float* segmentation_masks, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * L2b person-detector input augmentation (the per-pixel half of the detector's input pipeline).
 * Replaces the image operations of detector/input_pipeline/person_detector_pipeline.py `augmentation`
 * (:109-116: `randomly_crop_and_resize` :119-138, `randomly_pad` :141-180, color_augmentations.py:10-69,
 * `random_flip_left_right` :245-257) and `resize_keeping_aspect_ratio` (:183-242) for a batch of RAGGED
 * uint8 sources in one launch. The host draws every random decision and fills one descriptor per image
 * (multiposenet_amd/detector/input_pipeline/detector_augment.py); per output pixel (y, x), with
 * p = flip ? W-1-x : x the position before the flip:
 *
 *   S2(sy,sx)  stage-2 canvas [H,W]: 0 unless sy < valid_h and sx < valid_w (pad_to_bounding_box, :225), else
 *              the legacy bilinear resize of the crop of u8 * float32(1/255): in = out * scale (f32 in/out),
 *              lo = floor(in), hi = min(lo+1, crop-1), top + (bottom-top)*y_lerp    (resize_images, :137, :221)
 *   pad        MPN_AUGMENT_PAD: 0 unless pad_y <= y < pad_y+pad_h and pad_x <= p < pad_x+pad_w, else the same
 *              legacy bilinear resize of S2 (in size H x W) sampled at (y-pad_y, p-pad_x) with pad_scale:
 *              4 taps of S2, each computed on the fly (S2 is never stored). Without the flag: S2(y, p).
 *   colour     clip(v + color[c], 0, 1), over the whole canvas, zero padding included   (:19-33)
 *   grayscale  0.2989 r + 0.5870 g + 0.1140 b on all channels                           (:35-38)
 *   scale      clip(v * (u * (maxval - minval) + minval), 0, 1),
 *              u = (fmix32(seed ^ (idx * 0x9E3779B1)) >> 8) * 2^-24, idx = (y*W + p)*3 + c  (:47-69)
 * Every float step is one IEEE round-to-nearest operation in that order (no contraction).
 * MPN_AUGMENT_EVAL marks a descriptor of the evaluation path (valid_h x valid_w smaller than H x W, no other
 * flag); the pixel arithmetic does not depend on it. The flag values are those of the keypoint kernel;
 * MPN_AUGMENT_ROTATE has no meaning here and is ignored.
 *
 *   sources    concatenated uint8 RGB images [src_h, src_w, 3]; image b starts at byte src_offset
 *   descs      [B] mpn_detector_augment_desc, DEVICE, 16-byte aligned
 *   images     [B,H,W,3] f32, 16-byte aligned
 * 1 <= B <= 65535, H % 4 == 0, W % 4 == 0, both <= 16384. Every output element is written. Descriptor fields are
 * the caller's to check (offsets and sizes inside the buffer); a source read outside an image's own rectangle
 * returns 0. mpn_detector_augment_desc_bytes() = sizeof(mpn_detector_augment_desc), for bindings.
 */
enum { MPN_AUGMENT_PAD = 64 };
#define MPN_DETECTOR_AUGMENT_DESC_BYTES 112
typedef struct mpn_detector_augment_desc {
    int64_t src_offset;                         /* byte offset into sources */
    int32_t src_h, src_w;
    int32_t crop_y, crop_x, crop_h, crop_w;     /* integer crop of the source (begin, size) */
    int32_t valid_h, valid_w;                   /* stage-2 size: H, W in training; new_h, new_w in evaluation */
    int32_t pad_y, pad_x, pad_h, pad_w;         /* placed rectangle (MPN_AUGMENT_PAD): offset and scaled size */
    float scale_y, scale_x;                     /* f32(crop_h)/f32(valid_h), f32(crop_w)/f32(valid_w) */
    float pad_scale_y, pad_scale_x;             /* f32(H)/f32(pad_h), f32(W)/f32(pad_w) (MPN_AUGMENT_PAD) */
    float color[3];                             /* per-channel offsets (MPN_AUGMENT_COLOR) */
    float minval, maxval;                       /* pixel-scale range (MPN_AUGMENT_PIXEL_SCALE) */
    uint32_t seed;                              /* pixel-scale hash seed (MPN_AUGMENT_PIXEL_SCALE) */
    int32_t flags;                              /* MPN_AUGMENT_* */
    int32_t reserved[3];
} mpn_detector_augment_desc;
#ifdef __cplusplus
static_assert(sizeof(mpn_detector_augment_desc) == MPN_DETECTOR_AUGMENT_DESC_BYTES, "descriptor size is fixed");
#endif
size_t mpn_detector_augment_desc_bytes(void);
int mpn_detector_augment(const uint8_t* sources, const void* descs, int B, int H, int W, float* images,
                         mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * L3  training examples of the pose residual network, from annotations alone (no image pixels).
 * Replaces the per-record work of detector/input_pipeline/prn_pipeline.py `parse_and_preprocess`
 * (:46-156: get_heatmaps through tf.py_func :91-95, tf.image.crop_and_resize :97-103, the label
 * maps :105-151) and `random_flip_left_right` (:159-203) for a batch of N examples drawn from R
 * source images of RAGGED sizes, in at most two launches (tables, examples) and without any host
 * synchronisation. For example n = (image r, person q, flip), output pixel (y, x), part c, with
 * xs = flip ? crop_w-1-x : x and cs = flip ? perm[c] : c, perm = [0,2,1,4,3,...,16,15]:
 *
 *   crops[n,y,x,c]  = crop_and_resize(M_r, boxes[q] / f32(H_r, W_r, H_r, W_r))[y, xs, cs]
 *                     bilinear, extrapolation value 0, arithmetic and order of mpn_prn_crop
 *                     (crop_and_resize_op.cc): in_y = y1*(h-1) + y*((y2-y1)*(h-1)/(crop_h-1)), 0 unless
 *                     0 <= in_y <= h-1 (x likewise), top + (bottom-top)*y_lerp of the taps at floor / ceil
 *   M_r             = get_heatmaps(persons of image r, W_r, H_r, downsample), [h, w, 17] with
 *                     h = ceil(H_r/downsample), w likewise: the values mpn_heatmap_render writes (same
 *                     f32 sigma / centre math, f64 window, f32 product, max over the image's visible
 *                     persons, peaks exactly 1.0f). M_r is never stored: each tap is evaluated from
 *                     the per-person tables, the candidate blobs culled per block in chunks of 60
 *                     persons (no limit on the persons of an image).
 *   labels[n,y,x,c] = 1 if keypoint cs of person q is visible (v > 0) and
 *                     y  == clip(rintf((f32(ky) - ymin) * (f32(crop_h) / (ymax - ymin))), 0, crop_h-1),
 *                     xs == clip(rintf((f32(kx) - xmin) * (f32(crop_w) / (xmax - xmin))), 0, crop_w-1),
 *                     else 0 (rintf: half to even, as tf.round)
 * Every float step is one IEEE round-to-nearest operation in that order (no contraction), so both
 * outputs are bit-identical to the reference's numpy / TensorFlow-CPU sequence.
 *
 *   keypoints    [Q,17,3] int32 (y, x, visibility), persons of all R images concatenated, DEVICE
 *   boxes        [Q,4] f32 (ymin, xmin, ymax, xmax), absolute, DEVICE
 *   first_person [R+1] int32, DEVICE: persons of image r are first_person[r] .. first_person[r+1]-1
 *   width,height [R] int32, DEVICE: size of image r (>= 2)
 *   examples     [N] mpn_prn_example_desc, DEVICE, 16-byte aligned
 *   crops,labels [N,crop_h,crop_w,17] f32, 16-byte aligned; EVERY element is written (no memset needed)
 *   workspace    mpn_prn_examples_workspace_bytes(Q) bytes of scratch, 16-byte aligned, uninitialised
 * Checked before any HIP call: N >= 0, crop_h, crop_w > 0, Q, R >= 0, downsample >= 1 (MPN_ERR_BAD_SHAPE);
 * N == 0 then returns MPN_OK without a launch; null pointers (MPN_ERR_BAD_ARG), alignment
 * (MPN_ERR_BAD_ALIGN), workspace size (MPN_ERR_WORKSPACE). The tables' contents are the caller's: an
 * example whose image or person index is out of range yields zeros; a box of zero height or width
 * divides by zero in the labels exactly as the reference does (the pipeline drops such persons).
 */
#define MPN_PRN_EXAMPLE_DESC_BYTES 16
typedef struct mpn_prn_example_desc {
    int32_t image;      /* r: index into first_person / width / height */
    int32_t person;     /* q: GLOBAL index into keypoints / boxes (first_person[r] <= q < first_person[r+1]) */
    int32_t flip;       /* nonzero: left-right flip with the left / right parts exchanged */
    int32_t reserved;
} mpn_prn_example_desc;
#ifdef __cplusplus
static_assert(sizeof(mpn_prn_example_desc) == MPN_PRN_EXAMPLE_DESC_BYTES, "descriptor size is fixed");
#endif
size_t mpn_prn_example_desc_bytes(void);
size_t mpn_prn_examples_workspace_bytes(int total_persons);
int mpn_prn_examples(const int32_t* keypoints, const float* boxes, int total_persons,
                     const int32_t* first_person, const int32_t* width, const int32_t* height,
                     int num_images, const void* examples, int N, int crop_h, int crop_w, int downsample,
                     float* crops, float* labels, void* workspace, size_t workspace_bytes, mpn_stream_t stream);

/* Skinny "NT" GEMM split over K: part[s][M][N] (f32, s < mpn_gemm_nt_num_parts(K)) = A[M][K] * B[N][K]^T over the s-th K range.
 * A, B 16-bit (MPN_BF16 / MPN_F16), row-major with K contiguous - the order the reference's variables already have for
 * dH = dPre2 * W2^T in the pose residual network (prn.py:11-33: fc2's data gradient), so no transposed copy of the weights is
 * made. K % 8 == 0, N % 4 == 0; finish with mpn_reduce_partials(part, parts, M * N, out, ...). */
int mpn_gemm_nt_num_parts(int K);
int mpn_gemm_nt(const void* a, const void* b, float* part, int M, int N, int K, int dtype, mpn_stream_t stream);
/* ------------------------------------------------------------------------------------
 * L2  PRN - pose residual network (BASELINE config 5).
 * Replaces detector/prn.py:5-25 (flatten -> fc1 34272->1024 + ReLU -> fc2 1024->34272 + ReLU -> x + y) and the loss of
 * prn_model.py:16-30 (softmax over h*w per keypoint channel, tf.losses.log_loss eps 1e-7, mean). The four GEMMs of a
 * training step run on mpn_conv_fwd / mpn_conv_bwd_weight (K = 34272 contractions as split-K "weight gradients" whose
 * pixel axis is K); these entry points are the glue: K-major operand copies, bias + ReLU, the loss and its gradient.
 */
int mpn_transpose_cast(const void* in, int in_dtype, void* out, int out_dtype, int R, int C, mpn_stream_t stream);
int mpn_cast(const void* in, int in_dtype, void* out, int out_dtype, long long n, mpn_stream_t stream);
int mpn_bias_relu_fwd(const void* pre, int pre_dtype, const float* bias, void* y, int out_dtype, int R, int C,
                      mpn_stream_t stream);
int mpn_bias_relu_bwd(const void* y, int y_dtype, const float* dy, void* dpre, int dpre_dtype, float* dbias, int R,
                      int C, mpn_stream_t stream);
/* grad_scale: dlogits = grad_scale * dloss/dlogits (static loss scale of the fp16 build, 1 otherwise; the caller passes
 * 1 / grad_scale to mpn_adam_step) */
int mpn_prn_loss(const float* x, const void* y2, int y2_dtype, const float* labels, int B, int P, int C,
                 float* logits, float* dlogits, float* loss_part, float grad_scale, mpn_stream_t stream);
/* logits[i] = x[i] + y2[i]: the residual connection of detector/prn.py:24 at inference (create_pb.py:112) */
int mpn_prn_residual(const float* x, const void* y2, int y2_dtype, long long n, float* logits, mpn_stream_t stream);

/* PRN inference glue (create_pb.py:86-142): what sits between the sigmoid heatmaps / the detector's boxes and the
 * network, and between its logits and the exported `keypoint_scores` / `keypoint_positions`.
 *   mpn_heatmap_minmax  per (image, channel) min and max over the map (create_pb.py:90-92: M, m). minmax_keys: B*C*2
 *                       32-bit words (opaque order-preserving keys, decoded by mpn_prn_crop). heatmaps f32 [B,h,w,C], C <= 17.
 *   mpn_prn_crop        (heatmaps - m) / (M - m) * (M > threshold), then tf.image.crop_and_resize (bilinear, extrapolation
 *                       value 0; create_pb.py:93-109) of box n of image box_ind[n]: boxes f32 [nb,4] normalised
 *                       (y1,x1,y2,x2) -> crops f32 [nb,crop_h,crop_w,C]. box_ind outside [0,B) gives a zero crop.
 *   mpn_prn_decode      logits f32 [nb,crop_h,crop_w,C] -> softmax over the crop_h*crop_w positions of each channel
 *                       (create_pb.py:114-117): scores f32 [nb,C] = its maximum, positions f32 [nb,C,2] =
 *                       (y / crop_h, x / crop_w) of the first maximum (argmax_2d + scaler, create_pb.py:119-138).
 */
int mpn_heatmap_minmax(const float* heatmaps, int B, int h, int w, int C, void* minmax_keys, mpn_stream_t stream);
int mpn_prn_crop(const float* heatmaps, const void* minmax_keys, const float* boxes, const int* box_ind, int nb, int B,
                 int h, int w, int C, int crop_h, int crop_w, float threshold, float* crops, mpn_stream_t stream);
/* mpn_prn_crop for `nb` consecutive slots slot0.. of a detector's padded output (boxes f32 [B,max_boxes,4], num_boxes i32
 * [B], retinanet.py:60-84): slot s = box s % max_boxes of image s / max_boxes; padding slots and slots past the array give
 * zero crops - the [:n] slices, box_ind vectors and concat of create_pb.py:96-104 without materialising them. */
int mpn_prn_crop_slots(const float* heatmaps, const void* minmax_keys, const float* boxes, const int* num_boxes, int slot0,
                       int nb, int max_boxes, int B, int h, int w, int C, int crop_h, int crop_w, float threshold,
                       float* crops, mpn_stream_t stream);
int mpn_prn_decode(const float* logits, int nb, int crop_h, int crop_w, int C, float* scores, float* positions,
                   mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * L3  RetinaNet person-detector head (BASELINE config 4): detector/retinanet.py:13-217,
 * detector/box_predictor.py:6-142, detector/fpn.py:42-46, detector/training_target_creation.py:5-159,
 * detector/utils/box_utils.py:14-139, detector/utils/nms.py:6-61. Its convolutions / batch-norms / optimizer are the entry
 * points above; these are the detector-specific pieces. Level arrays have 5 entries (p3..p7); anchors are ordered like
 * reshape_and_concatenate (box_predictor.py:55-90): level, then y, x, then the 6 anchors of a location.
 *
 *   mpn_patchify3x3s2     x [N,H,W,C] -> patches [N,ceil(H/2),ceil(W/2),9*C] for conv2d_same(k=3, stride=2) (pad 1, VALID):
 *                         the 3x3 stride-2 convolutions p6 / p7 (fpn.py:43,45) = this gather (producer's affine + act applied
 *                         on the way, zero padding after it) + a 1x1 convolution over 9*C channels with the HWIO kernel viewed
 *                         as [1,1,9*C,Cout]. mpn_unpatchify3x3s2 is its transpose: dpatches -> dx [N,H,W,C].
 *   mpn_retina_match      get_training_targets for a batch: anchors f32 [A,4] (normalised), gt_boxes f32 [B,max_boxes,4],
 *                         num_boxes int32 [B] -> matches int32 [B,A] (-2 ignore, -1 background, else the box index), targets
 *                         f32 [B,A,4] (encode(), zeros where unmatched), num_matched int32[1] = count of matches >= 0.
 *                         float32 arithmetic in the reference's operation order; arg-max ties: first index (tf.argmax).
 *   mpn_retina_loss       focal loss (gamma, alpha; weights = not ignored) + smooth L1 (matched anchors) over raw tower outputs
 *                         logits[l] [B,h,w,8] (6 used) / boxes[l] [B,h,w,24] + biases, both normalised by max(num_matched, 1);
 *                         dlogits / dboxes (same layouts, may be NULL arrays) receive d(loc_w*loc + cls_w*cls); part
 *                         [mpn_retina_loss_num_parts][32] = partial sums of {cls loss, loc loss, dbias_cls[6], dbias_box[24]}
 *                         (finish with mpn_reduce_partials; the two losses still need the 1/normaliser).
 *   mpn_retina_nms        get_predictions: sigmoid, score >= threshold, decode + clip to [0,1], greedy NMS, zero padding:
 *                         out_boxes f32 [B,max_det,4], out_scores f32 [B,max_det], out_num int32 [B].
 *                         The workspace holds one candidate list of A slots per image, a counter per image and ONE int32
 *                         OVERFLOW word at byte mpn_retina_nms_overflow_offset(B, A): 0 after a good call, 1 when a list would
 *                         have grown past its A slots (the appends past the list are refused, the selection never reads past
 *                         it). A caller reads it WITH the outputs (the library never synchronises; from a captured graph it is
 *                         the only report there is) and treats 1 as MPN_ERR_WORKSPACE.
 */
int mpn_patchify3x3s2(const void* x, void* patches, int N, int H, int W, int C, int dtype, const float* in_scale,
                      const float* in_shift, int in_act, mpn_stream_t stream);
int mpn_unpatchify3x3s2(const void* dpatches, void* dx, int N, int H, int W, int C, int dtype, mpn_stream_t stream);
size_t mpn_retina_match_workspace_bytes(int B, int max_boxes);
int mpn_retina_match(const float* anchors, const float* gt_boxes, const int* num_boxes, int B, int A, int max_boxes,
                     float positives_threshold, float negatives_threshold, int* matches, float* targets,
                     int* num_matched, void* workspace, size_t workspace_bytes, mpn_stream_t stream);
int mpn_retina_loss_num_parts(int B, int A);
int mpn_retina_loss(const void* const* logits, const void* const* boxes, void* const* dlogits, void* const* dboxes,
                    const int* h, const int* w, int dtype, const float* cls_bias, const float* box_bias,
                    const int* matches, const float* targets, const int* num_matched, int B, float gamma, float alpha,
                    float localization_loss_weight, float classification_loss_weight, float* part,
                    mpn_stream_t stream);
/* The scalar losses of a step from the reduced partial sums (retinanet.py:128-144, person_detector_model.py:33-45):
 * sums f32 [32] = {cls, loc, dbias_cls[6], dbias_box[24]} (mpn_reduce_partials of mpn_retina_loss's parts);
 * losses f32 [4] = {localization = sums[1] / max(num_matched, 1), classification = sums[0] / max(num_matched, 1),
 * regularization (left as the caller accumulated it), total = loc_w * localization + cls_w * classification + regularization};
 * dbias_cls f32 [6] / dbias_box f32 [24] (may be NULL) receive the output convolutions' bias gradients. */
int mpn_retina_loss_finalize(const float* sums, const int* num_matched, float localization_loss_weight,
                             float classification_loss_weight, float* losses, float* dbias_cls, float* dbias_box,
                             mpn_stream_t stream);
size_t mpn_retina_nms_workspace_bytes(int B, int A);
size_t mpn_retina_nms_overflow_offset(int B, int A);
int mpn_retina_nms(const void* const* logits, const void* const* boxes, const int* h, const int* w, int dtype,
                   const float* cls_bias, const float* box_bias, const float* anchors, int B, float score_threshold,
                   float iou_threshold, int max_detections, float* out_boxes, float* out_scores, int* out_num,
                   void* workspace, size_t workspace_bytes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Result packing of the batched joint inference graph (create_pb.py:53-61 for b images; the score filter of
 * inference/detector.py:54-59 and the live-slot gather of create_pb.py:96-104 without leaving the device).
 *
 *   mpn_pose_gather   boxes f32 [B,max_boxes,4] normalised (ymin,xmin,ymax,xmax), scores f32 [B,max_boxes], num_boxes int32 [B]
 *                     (mpn_retina_nms's outputs), keypoint_scores f32 [B*max_boxes,17], keypoint_positions f32
 *                     [B*max_boxes,17,2] = (y, x) normalised to the box (mpn_prn_decode's outputs; either may be NULL: its
 *                     fields and what derives from them are zero), overflow: the NMS overflow word (may be NULL: 0)
 *                     -> ONE record of mpn_pose_gather_record_bytes(B, max_boxes) bytes, in 32-bit words:
 *                       header  int32: total, counts[B], num_boxes[B] (copied through: the count BEFORE the filter),
 *                               overflow; zero words up to the next multiple of 16 bytes
 *                       rows    B*max_boxes of them, row r at byte mpn_pose_gather_row_offset(B, max_boxes, r); a row is
 *                               int32 image_index, f32 box[4], score, keypoint_scores[17], keypoint_positions[17][2],
 *                               keypoints[17][3] = (x, y, score) in image pixels:
 *                                 x = xmin*width + pos_x * (xmax*width - xmin*width), y likewise with height
 *                               (inference/predict.ipynb, draw_everything; plain IEEE f32 in that order, no contraction).
 *                     A slot is KEPT iff slot < num_boxes[image] and score > score_threshold (strict). Kept slots fill rows
 *                     0 .. total-1 in (image, slot) order; every other row is zero. Slots >= num_boxes are never read.
 *                     One block: B * max_boxes <= 4096 (MPN_ERR_BAD_SHAPE above; record_bytes then returns 0).
 *                     Checked before any HIP call: null boxes / scores / num_boxes / record (MPN_ERR_BAD_ARG), B, max_boxes,
 *                     height, width >= 1 and the row count (MPN_ERR_BAD_SHAPE), record 16-byte aligned (MPN_ERR_BAD_ALIGN),
 *                     record_bytes (MPN_ERR_WORKSPACE).
 *   mpn_pose_gather_row_offset   row in [0, B*max_boxes]; the last is the record's size; the difference of two neighbours is
 *                                the row stride. 0 for arguments out of range.
 */
size_t mpn_pose_gather_record_bytes(int B, int max_boxes);
size_t mpn_pose_gather_row_offset(int B, int max_boxes, int row);
int mpn_pose_gather(const float* boxes, const float* scores, const int* num_boxes, const float* keypoint_scores,
                    const float* keypoint_positions, const int* overflow, int B, int max_boxes, float score_threshold,
                    int height, int width, void* record, size_t record_bytes, mpn_stream_t stream);
/*   mpn_pose_gather_sized   mpn_pose_gather for images that were resized onto the network canvas: in place of the by-value
 *                     height, width it takes extent f32 [B,4] on the DEVICE, per image (box_scale_y, box_scale_x,
 *                     pixel_height, pixel_width). The record's box is box * (box_scale_y, box_scale_x, box_scale_y,
 *                     box_scale_x) (one f32 multiply each), its keypoints are computed from THAT box and (pixel_height,
 *                     pixel_width) with the arithmetic above in the same order. Same record layout, keep rule, one-block
 *                     limit and checks (extent: MPN_ERR_BAD_ARG when null). With extent (1, 1, height, width) the record
 *                     equals mpn_pose_gather's bit for bit. The values reach the kernel through device memory, so a
 *                     captured graph serves any later extents. */
int mpn_pose_gather_sized(const float* boxes, const float* scores, const int* num_boxes, const float* keypoint_scores,
                          const float* keypoint_positions, const int* overflow, int B, int max_boxes, float score_threshold,
                          const float* extent, void* record, size_t record_bytes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * COCO keypoint evaluation of the record's persons against ground truth: object keypoint similarity (OKS) and the greedy
 * matching of pycocotools' COCOeval for iouType='keypoints' (computeOks, evaluateImg), one block per image.
 *
 *   mpn_oks_match   record: what mpn_pose_gather[_sized] wrote for (B, max_boxes), DEVICE, read in place (the header's total
 *                     and counts; of a row its score, keypoint_scores and keypoints).
 *                   gt f64 [B, max_gt, 64] DEVICE: a row of mpn_oks_gt_row_bytes() = 512 bytes is keypoints[17][3] = (x, y, v),
 *                     bbox (x, y, w, h), area, ignore, iscrowd (non-zero = set), 6 doubles of padding; the pixels of the
 *                     record's keypoints. gt_counts int32 [B] DEVICE (a count above max_gt reads max_gt rows).
 *                   thresholds f64 [num_thresholds] DEVICE, 1 <= num_thresholds <= 10 (np.linspace(.5, .95, 10)).
 *                   score_mode 0: a detection's score is the box score; 1: box score * (sum of keypoint_scores in order / 17),
 *                     in f32. max_dets in 1..20: per image the first max_dets detections in descending score, equal scores
 *                     in record order, are evaluated.
 *                   Semantics, in float64 in this order without contraction: detection area (max x - min x) * (max y - min y)
 *                     of its 17 keypoints; vars = (2 sigma)^2 of COCO's 17 sigmas; k1 = ground-truth keypoints with v > 0;
 *                     k1 > 0: dx, dy = detection - ground truth over the v > 0 keypoints, else the distance to the doubled box
 *                     (x0 = bx - bw, x1 = bx + 2 bw: max(0, x0 - xd) + max(0, xd - x1)) over all 17;
 *                     e = (dx^2 + dy^2) / vars / (area + 2^-52) / 2; OKS = mean of exp(-e). Per area range (all [0, 1e10],
 *                     medium [32^2, 96^2], large [96^2, 1e10]) a ground truth is ignored iff its ignore is set or its area
 *                     lies outside; ground truth is walked not-ignored first (stable). Per range, threshold t and detection
 *                     in score order: iou = min(t, 1 - 1e-10), m = none; for each ground truth: skip it if matched and not
 *                     crowd; stop if m is set, not ignored, and this one is ignored; skip it if OKS < iou; else iou = OKS,
 *                     m = it. A matched detection takes the ignore flag of its ground truth; an unmatched one is ignored iff
 *                     its area lies outside the range.
 *                   out: mpn_oks_match_out_bytes(B, max_boxes) bytes DEVICE, one row of 152 bytes per record row, aligned
 *                     with the record's rows 0 .. total-1, every other row zero: int32 rank (>= max_dets: not evaluated,
 *                     matches -1), f32 score, f64 area, int32 match[3][10] (range, threshold): the ground truth's index in
 *                     the image's own order or -1 (also beyond num_thresholds), uint32 ignore[3]: bit t = ignored at
 *                     threshold t, 4 bytes of zero.
 *                   oks_out (may be NULL): f64 [B * max_boxes, max_gt], the OKS of each evaluated row against the image's
 *                     ground truth, zero elsewhere.
 *                   Checked before any HIP call: max_gt in 1..64 (MPN_ERR_BAD_SHAPE; a lane keeps its matched set in one
 *                     64-bit mask), null pointers and score_mode (MPN_ERR_BAD_ARG), B, max_boxes <= 256, B * max_boxes <=
 *                     4096, num_thresholds, max_dets (MPN_ERR_BAD_SHAPE), record 16-byte and the f64 buffers 8-byte aligned
 *                     (MPN_ERR_BAD_ALIGN). The grid depends on B alone: a captured launch serves any later ground truth.
 *   mpn_oks_match_out_bytes   0 for arguments out of range.
 */
size_t mpn_oks_gt_row_bytes(void);
size_t mpn_oks_match_out_bytes(int B, int max_boxes);
int mpn_oks_match(const void* record, int B, int max_boxes, const double* gt, const int* gt_counts, int max_gt,
                  const double* thresholds, int num_thresholds, int score_mode, int max_dets, void* out, double* oks_out,
                  mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Keypoint-similarity NMS of the record's persons: duplicate poses (two boxes on one person that box NMS kept apart) are
 * dropped by their OKS with a better pose. A pure function from one record to another of the same layout, one block per image
 * and one block that compacts; no atomics.
 *
 *   mpn_pose_nms   record_in: what mpn_pose_gather[_sized] wrote for (B, max_boxes), DEVICE, read in place: of the header
 *                     counts[B], each clamped to 0..max_boxes (the persons of image i are the rows behind the clamped counts
 *                     of the images before it, in record order p = 0..n-1; total is not read), num_boxes[B] and the overflow
 *                     word; of a row its score, keypoint_scores and keypoints.
 *                   Semantics, in float64 in this order without contraction unless f32 is named. Per image:
 *                     order score: score_mode 0 the row's box score; 1 box score * (sum of keypoint_scores in order / 17) in
 *                     f32 (mpn_oks_match's score_mode). Persons are visited in descending order score, equal scores in record
 *                     order; a NaN order score sorts behind every number, in record order.
 *                     a_p = (max x - min x) * (max y - min y) of the row's 17 keypoints (min / max in f32, the differences and
 *                     the product in f64). Similarity of p, q: the joints that count are those with keypoints[k][2] >=
 *                     min_keypoint_score (f32 compare) in BOTH rows, m of them; m == 0: 0; else denom = (a_p + a_q) / 2 +
 *                     2^-52, e_k = (dx^2 + dy^2) / vars[k] / denom / 2 with dx = (double)x_q - (double)x_p, dy likewise and
 *                     mpn_oks_match's vars; the similarity is (sum of exp(-e_k) over the counting joints in k order) / m.
 *                     It is symmetric; each unordered pair is computed once.
 *                     Suppression: in visit order a person that is not suppressed is KEPT and suppresses every person behind
 *                     it that is not yet suppressed and whose similarity with it is > (double)threshold (strict). A
 *                     suppressed person suppresses nothing.
 *                   record_out: record_bytes >= mpn_pose_gather_record_bytes(B, max_boxes) bytes DEVICE, the layout of
 *                     record_in: total and counts[B] are the kept numbers, num_boxes[B] and overflow are copied through, the
 *                     kept rows are byte copies of their input rows, dense, in record order (scores are not rewritten), every
 *                     other row and the header's padding are zero. It must not overlap record_in.
 *                   info: info_bytes >= mpn_pose_nms_info_bytes(B, max_boxes) bytes DEVICE: int32 suppressed[B] (the clamped
 *                     count minus the kept number), zero words up to a multiple of 16 bytes; then one 8-byte row per record
 *                     row, aligned with record_out's rows 0 .. total-1, every other row zero: int32 source (the person's index
 *                     p among its image's persons in record_in), int32 absorbed (the persons this one suppressed); then the
 *                     launch's workspace, 8 bytes per slot (image, p), p < max_boxes: int32 keep (1 / 0), int32 absorbed (0
 *                     unless kept), both 0 for p >= n.
 *                   sim_out (may be NULL): f64 [B, max_boxes, max_boxes] DEVICE, the similarity of persons p != q < n of each
 *                     image; the diagonal and everything else zero.
 *                   Checked before any HIP call, in this order: null record_in / record_out / info, score_mode not 0 / 1, a
 *                     NaN threshold or min_keypoint_score (MPN_ERR_BAD_ARG); B, max_boxes >= 1, max_boxes <= 64 (a person's
 *                     suppression set is one 64-bit mask), B * max_boxes <= 4096 (MPN_ERR_BAD_SHAPE); record_in == record_out
 *                     or overlapping ranges (MPN_ERR_BAD_ARG); the records 16-byte, info and sim_out 8-byte aligned
 *                     (MPN_ERR_BAD_ALIGN); record_bytes, info_bytes (MPN_ERR_WORKSPACE). The grids depend on B alone: a
 *                     captured launch serves any later record.
 *   mpn_pose_nms_info_bytes   0 for arguments out of range.
 */
size_t mpn_pose_nms_info_bytes(int B, int max_boxes);
int mpn_pose_nms(const void* record_in, int B, int max_boxes, float threshold, float min_keypoint_score, int score_mode,
                 void* record_out, size_t record_bytes, void* info, size_t info_bytes, double* sim_out, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Person identities across the frames of a video: the record's persons of every frame are matched against the tracks the
 * earlier frames left, one block per stream: greedily (mpn_pose_track) or by the optimal assignment (mpn_pose_track_optimal).
 *
 *   mpn_pose_track   record: what mpn_pose_gather[_sized] wrote for (B, max_boxes), DEVICE, read in place exactly as
 *                     mpn_oks_match reads it (the header's total and counts, clamped the same way; only rows 0 .. total-1;
 *                     of a row its box, score and keypoints).
 *                   Streams: B = streams * F. Stream s owns images s*F .. s*F+F-1 in time order: one camera with a batch of
 *                     consecutive frames is streams = 1, B cameras with one frame each is streams = B. Ids are per stream.
 *                   PURE: the launch reads prev and writes the COMPLETE new state to next and the rows to out; it never
 *                     writes prev, and running it twice in a row gives the same bytes. The caller advances the state by
 *                     copying next over prev behind the launch (a few KB). A capture / replay front end runs its device
 *                     side eagerly and then replays it on an entry's first call; an in-place update would count every track
 *                     twice there. prev == next is refused (MPN_ERR_BAD_ARG).
 *                   State, prev and next, mpn_pose_track_state_bytes(streams, max_tracks) bytes DEVICE, per stream in 32-bit
 *                     words: int32 next_id (a value < 1 reads as 1), int32 dropped (detections that found no free slot,
 *                     cumulative), two zero words; then max_tracks slots of 60 words: int32 id (0 = free), hits (frames
 *                     matched, the first included), age (frames since the first, that one included), misses (frames in a row
 *                     without a match), f32 box[4], score, keypoints[17][3], copied from the record row last matched. A free
 *                     slot is all zero in next. An all-zero state is the valid empty state.
 *                   Similarity of a live track (a) and a detection of the frame (b), without contraction:
 *                     similarity 0, IoU in f32 of the two record boxes (ymin, xmin, ymax, xmax): x0 = a.xmin > b.xmin ?
 *                       a.xmin : b.xmin, x1 = a.xmax < b.xmax ? a.xmax : b.xmax, iw = x1 - x0, iw = iw > 0 ? iw : 0, ih
 *                       likewise; inter = iw * ih; area = (xmax - xmin) * (ymax - ymin); union = area_a + area_b - inter;
 *                       inter / union if union > 0 else 0. Needs no keypoints.
 *                     similarity 1, OKS in f64 (mpn_oks_match's arithmetic): the track's stored keypoints are the ground
 *                       truth with all 17 visible, area = (max x - min x) * (max y - min y) of those keypoints (min / max in
 *                       f32), e = (dx^2 + dy^2) / vars / (area + 2^-52) / 2 with dx = detection - track, OKS = sum of
 *                       exp(-e) in keypoint order / 17.
 *                   Per frame, in this order:
 *                     1. among the pairs (live slot t, unmatched detection d) with similarity >= match_threshold (compared
 *                        in f64; a NaN never matches) the largest similarity is matched, ties to the smaller t, then the
 *                        smaller d; repeated until no pair is left.
 *                     2. a matched track takes the detection's box, score and keypoints; misses = 0, hits += 1, age += 1.
 *                     3. an unmatched live track: misses += 1, age += 1; freed (the slot zeroed) when misses > max_misses.
 *                     4. the unmatched detections with score >= new_track_score, in row order, take the lowest free slots
 *                        (those freed in step 3 included): id = next_id++, hits = 1, age = 1, misses = 0. With no free slot
 *                        left the detection stays untracked, its overflow flag is set and dropped += 1. Detections below
 *                        new_track_score stay untracked.
 *                     A frame without detections still ages the tracks.
 *                   out: mpn_pose_track_out_bytes(B, max_boxes) bytes DEVICE, one row of 24 bytes per record row, aligned
 *                     with the record's rows 0 .. total-1, every other row zero: int32 track_id (0 = untracked), int32 slot
 *                     (-1 = none), int32 hits, int32 flags (bit 0 = new this frame, bit 1 = overflow), f64 similarity to the
 *                     matched track (0 when new or untracked).
 *                   Checked before any HIP call: null pointers (MPN_ERR_BAD_ARG); streams >= 1, B % streams == 0,
 *                     1 <= max_tracks <= 64, 1 <= max_boxes <= 64, B * max_boxes <= 4096, similarity in {0, 1},
 *                     max_misses >= 0 (MPN_ERR_BAD_SHAPE); record 16-byte and prev / next / out 8-byte aligned
 *                     (MPN_ERR_BAD_ALIGN); prev == next (MPN_ERR_BAD_ARG). The grid depends on streams alone: a captured
 *                     launch serves any later record and state.
 *   mpn_pose_track_state_bytes, mpn_pose_track_out_bytes   0 for arguments out of range.
 *
 *   mpn_pose_track_optimal   mpn_pose_track with the frame's matching optimal (Hungarian) instead of greedy: the same
 *                     arguments, state layout, output rows, purity, grid and checks (in the same order; the messages begin
 *                     "pose_track_optimal:"). Of "Per frame" only step 1 differs; steps 2 - 4 are mpn_pose_track's word for
 *                     word. Step 1, for a frame with n detections and T = max_tracks slots:
 *                   Similarity: s(d, t) is the f64 value mpn_pose_track computes (IoU in f32, widened; OKS in f64).
 *                   Eligibility: the pair (d, t) is eligible when slot t is live and s >= (double)match_threshold; a NaN is
 *                     never eligible.
 *                   Weight: q = floor(s * 2^20) in f64, clamped to 0 .. 2^20 before the conversion to an integer; w = q + 1.
 *                     Integers make the optimum independent of the order of summation (a last-bit difference in exp changes
 *                     it only where s * 2^20 sits on an integer); the + 1 makes every eligible match worth taking.
 *                   Problem: rows i = 1..n are the detections. Columns j = 1..T are the slots, cost(i, j) = -w(i-1, j-1) where
 *                     eligible, absent otherwise. Columns j = T+1..T+n are dummies: cost(i, T+i) = 0, absent for every other
 *                     row. Every row is assigned to a distinct column at minimal total cost: the maximum-weight matching of the
 *                     eligible pairs, always feasible. A row on its dummy is an unmatched detection.
 *                   Algorithm (it fixes the result where several optima exist): shortest augmenting paths in exact integers,
 *                     potentials u[0..n] and v[0..m], p[0..m] (the row on column j, 0 = none), way[0..m], m = T + n, all 0
 *                     at the start of the frame; rows are inserted in row order:
 *                       for i in 1..n:
 *                         p[0] = i; j0 = 0; minv[1..m] = absent; used[0..m] = false
 *                         repeat:
 *                           used[j0] = true; i0 = p[j0]; delta = absent
 *                           for j in 1..m in increasing order, used[j] false:
 *                             if cost(i0, j) present: cur = cost(i0, j) - u[i0] - v[j];
 *                               if minv[j] absent or cur < minv[j]: minv[j] = cur; way[j] = j0
 *                             if minv[j] present and (delta absent or minv[j] < delta): delta = minv[j]; j1 = j
 *                               (ties: the smaller j)
 *                           for j in 0..m: used[j] ? (u[p[j]] += delta, v[j] -= delta)
 *                                                  : (minv[j] present ? minv[j] -= delta)
 *                           j0 = j1
 *                         until p[j0] == 0
 *                         repeat: j1 = way[j0]; p[j0] = p[j1]; j0 = j1 until j0 == 0
 *                     Detection p[j] - 1 is matched to slot j - 1 for every j <= T with p[j] != 0; the row's similarity is
 *                     the unquantised f64 s of its pair. The arithmetic is in 64-bit integers. The loops over rows, over
 *                     the repeat of a row and over its path are bounded (64, 129, 129 trips): should a bound be hit, the
 *                     frame's remaining detections stay unmatched.
 *
 *   mpn_pose_track_motion   either entry with a constant-velocity prediction in the track's role: a frame's detections are
 *                     compared with where each track is expected in that frame, not with the pose it was last seen with, and
 *                     the tracks that are live but not detected in a frame ("coasting") are reported at their predicted pose.
 *                     record, B, max_boxes, streams, max_tracks, similarity, match_threshold, new_track_score, max_misses,
 *                     prev, next, out: as for mpn_pose_track; the track state and the output rows keep their layout and
 *                     meaning. assignment: 0 = step 1 of mpn_pose_track (greedy), 1 = that of mpn_pose_track_optimal.
 *                     Every float operation below is one IEEE f32 operation in the order written, without contraction;
 *                     the division is correctly rounded.
 *                   Motion state, motion_prev and motion_next, mpn_pose_track_motion_state_bytes(streams, max_tracks) bytes
 *                     DEVICE, per stream in 32-bit words: four zero words; then max_tracks slots of 8 words: int32 id (the
 *                     track the velocities belong to, 0 = none), int32 seen (the matches the velocities have taken in),
 *                     f32 vel[6]: vel[0..3] the velocity per frame of the record box (ymin, xmin, ymax, xmax), vel[4..5] that
 *                     of the keypoint centroid (x, y) - two sets because a record's boxes are normalised to the image and
 *                     its keypoints are pixels. An all-zero state is the valid empty state. A slot of motion_prev whose id is
 *                     not the id of the same slot of prev (the track state was reset or replaced on its own) reads as
 *                     seen = 0, vel = 0. In motion_next a live slot holds its track's id, a free slot is all zero.
 *                   PURE, as mpn_pose_track: prev and motion_prev are only read, the COMPLETE new states go to next and
 *                     motion_next, two launches in a row write the same bytes. prev == next and motion_prev == motion_next
 *                     are refused.
 *                   The centroid of keypoints[17] is cx = (x_0 + x_1 + ... + x_16) / 17.0f, the sum taken in keypoint order
 *                     from x_0 on; cy likewise.
 *                   Per frame, in this order:
 *                     0. every live slot, with m = its misses and gap = f32(m + 1) (the frames since it was last observed,
 *                        this one included), is predicted: pbox[c] = box[c] + vel[c] * gap; pkp[k].x = kp[k].x + vel[4] * gap;
 *                        pkp[k].y = kp[k].y + vel[5] * gap. The score is unchanged. The anchor is the last OBSERVED pose:
 *                        the position is not filtered.
 *                     Similarity: mpn_pose_track's arithmetic with pbox / pkp in the track's role (a); for OKS the extent
 *                        area is that of pkp.
 *                     1 - 4. as mpn_pose_track (assignment 0) or mpn_pose_track_optimal (assignment 1), word for word; a
 *                        matched slot still takes the detection's own box, score and keypoints.
 *                     Velocities. A matched slot, with `last` the slot's pose before step 2 and z the detection, the six
 *                        components c being box[0..3] and the centroid (x, y) of the keypoints: vobs = (z[c] - last[c]) / gap;
 *                        g = (seen == 0 && velocity_gain > 0) ? 1.0f : velocity_gain; vel[c] = vel[c] + g * (vobs - vel[c]);
 *                        then seen += 1 (a track's second observation sets its velocity, later ones blend). An unmatched
 *                        live slot: vel[c] = vel[c] * damping. A freed slot: all zero. A born slot: its id, seen = 0, vel = 0.
 *                   coast_out: mpn_pose_track_coast_bytes(B, max_tracks) bytes DEVICE, max_tracks rows of 160 bytes per
 *                     image: the slots that are live after step 3 and were not matched in the frame (a slot born in the
 *                     frame is not among them), in slot order, packed at the front of the image's rows, the other rows
 *                     zero: int32 id, int32 misses (after step 3), f32 pbox[4], f32 pkp[17][2] - the prediction of this
 *                     frame's step 0.
 *                   With velocity_gain = 0 every velocity stays 0 (finite poses) and the prediction is the stored pose: the
 *                     output rows and the track state are byte for byte those of mpn_pose_track / mpn_pose_track_optimal.
 *                   Checked before any HIP call, the messages begin "pose_track_motion:": mpn_pose_track's checks in its
 *                     order, with motion_prev / motion_next / coast_out among the null pointers (MPN_ERR_BAD_ARG);
 *                     assignment in {0, 1} behind similarity (MPN_ERR_BAD_SHAPE); velocity_gain and damping finite and in
 *                     0..1 behind max_misses (MPN_ERR_BAD_ARG); motion_prev / motion_next / coast_out 8-byte aligned behind
 *                     the other alignments (MPN_ERR_BAD_ALIGN); motion_prev == motion_next behind prev == next
 *                     (MPN_ERR_BAD_ARG). The grid depends on streams alone.
 *   mpn_pose_track_motion_state_bytes   streams * (16 + 32 * max_tracks); 0 for arguments out of range.
 *   mpn_pose_track_coast_bytes          B * max_tracks * 160; 0 for arguments out of range (B outside 1..4096).
 */
size_t mpn_pose_track_state_bytes(int streams, int max_tracks);
size_t mpn_pose_track_out_bytes(int B, int max_boxes);
size_t mpn_pose_track_motion_state_bytes(int streams, int max_tracks);
size_t mpn_pose_track_coast_bytes(int B, int max_tracks);
int mpn_pose_track_motion(const void* record, int B, int max_boxes, int streams, int max_tracks, int similarity, int assignment,
                          float match_threshold, float new_track_score, int max_misses, float velocity_gain, float damping,
                          const void* prev, void* next, const void* motion_prev, void* motion_next, void* out, void* coast_out,
                          mpn_stream_t stream);
int mpn_pose_track(const void* record, int B, int max_boxes, int streams, int max_tracks, int similarity,
                   float match_threshold, float new_track_score, int max_misses, const void* prev, void* next, void* out,
                   mpn_stream_t stream);
int mpn_pose_track_optimal(const void* record, int B, int max_boxes, int streams, int max_tracks, int similarity,
                           float match_threshold, float new_track_score, int max_misses, const void* prev, void* next,
                           void* out, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * One-Euro smoothing (Casiez, Roussel, Vogel, CHI 2012) of the tracked persons' keypoints, and the per-joint velocities its
 * derivative estimate gives: one filter per (stream, track slot, joint), one block per stream.
 *
 *   mpn_pose_smooth   record: what mpn_pose_gather[_sized] wrote for (B, max_boxes), DEVICE, read in place exactly as
 *                     mpn_pose_track reads it (the header's total and counts, clamped the same way; only rows 0 .. total-1;
 *                     of a row only keypoints[17][3] = (x, y, score)).
 *                   track_rows: the `out` of mpn_pose_track for the same record, DEVICE; of a row int32 track_id and int32
 *                     slot are read.
 *                   Streams: B = streams * F, stream s owns images s*F .. s*F+F-1 in time order, as in mpn_pose_track.
 *                   PURE, as mpn_pose_track and for the same reason: the launch reads prev and writes the COMPLETE new state
 *                     to next and the rows to out; it never writes prev, and running it twice in a row gives the same bytes.
 *                     The caller advances the state by copying next over prev. prev == next is refused (MPN_ERR_BAD_ARG).
 *                   State, prev and next, mpn_pose_smooth_state_bytes(streams, max_tracks) bytes DEVICE, per stream in 32-bit
 *                     words: int32 frames (the frames this stream has seen), three zero words; then max_tracks slots of 88
 *                     words: int32 id (the track the filters belong to, 0 = none); 17 groups of {int32 last, f32 x_hat,
 *                     y_hat, dx_hat, dy_hat}, last = the stream's frame number at which the joint's filter last took a sample,
 *                     0 = no sample; two zero words. An all-zero state is the valid empty state. Frame numbers count from 1;
 *                     the counter is an int32 and is NOT guarded against wrap (2^31 frames are about 2 years at 30 Hz).
 *                   Every float operation below is one IEEE f32 operation in the order written, without contraction; the
 *                     division is correctly rounded. For frame j of the launch (0 <= j < F) n = prev.frames + j + 1. For
 *                     every record row r of that image:
 *                     untracked (track_id <= 0, or slot outside 0 .. max_tracks-1): out = the raw (x, y, score), velocity
 *                       (0, 0); no state is touched. A slot value of any kind never indexes anything.
 *                     tracked: if state[slot].id != track_id the slot becomes {id = track_id, every last = 0} (the slot was
 *                       given to another track; ids are never reused). Then per joint k with the raw (x, y, score):
 *                       rejected, not (score >= min_keypoint_score): last = 0; out = raw, velocity 0. The next good sample
 *                         starts the filter again.
 *                       first, last == 0: x_hat = x, y_hat = y, dx_hat = dy_hat = 0, last = n; out = raw, velocity 0.
 *                       filtered, otherwise, the same steps for y:
 *                         gap = n - last      (>= 1: frames without the person, or without any detection, count)
 *                         te = f32(gap) / rate
 *                         alpha(fc): r = (TWO_PI * fc) * te; alpha = r / (r + 1)        TWO_PI = 6.2831855f
 *                         dx = (x - x_hat) / te
 *                         dx_hat = dx_hat + alpha(d_cutoff) * (dx - dx_hat)
 *                         fc = min_cutoff + beta * fabs(dx_hat)
 *                         x_hat = x_hat + alpha(fc) * (x - x_hat)
 *                       then last = n; out = (x_hat, y_hat, score), velocity (dx_hat, dy_hat) in pixels per second. The
 *                       incremental form keeps a constant input exactly constant.
 *                     Slots that no row of the launch names are copied from prev to next unchanged; next.frames =
 *                     prev.frames + F. A frame without detections still counts. Two rows of one frame that name the same slot
 *                     cannot come out of mpn_pose_track; the result for that slot is then unspecified, memory safety is not.
 *                     The units are pixels: beta, which multiplies a speed, depends on the resolution.
 *                   out: mpn_pose_smooth_out_bytes(B, max_boxes) bytes DEVICE, one row of 340 bytes per record row, aligned
 *                     with the record's rows 0 .. total-1, every other row zero: f32 keypoints[17][3] (x, y, score), then f32
 *                     velocities[17][2].
 *                   Checked before any HIP call: null pointers, prev == next, rate / min_cutoff / d_cutoff not finite or not
 *                     > 0, beta not finite or < 0, min_keypoint_score not finite (MPN_ERR_BAD_ARG); streams >= 1,
 *                     B % streams == 0, 1 <= max_tracks <= 64, 1 <= max_boxes <= 64, B * max_boxes <= 4096
 *                     (MPN_ERR_BAD_SHAPE); record 16-byte and track_rows / prev / next / out 8-byte aligned
 *                     (MPN_ERR_BAD_ALIGN). The grid depends on streams alone: a captured launch serves any later record and
 *                     state.
 *   mpn_pose_smooth_state_bytes   streams * (16 + max_tracks * 352); 0 for arguments out of range.
 *   mpn_pose_smooth_out_bytes     B * max_boxes * 340; 0 for arguments out of range.
 */
size_t mpn_pose_smooth_state_bytes(int streams, int max_tracks);
size_t mpn_pose_smooth_out_bytes(int B, int max_boxes);
int mpn_pose_smooth(const void* record, const void* track_rows, int B, int max_boxes, int streams, int max_tracks,
                    float rate, float min_cutoff, float beta, float d_cutoff, float min_keypoint_score, const void* prev,
                    void* next, void* out, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Tracking accuracy: a frame's tracked persons against annotated persons that carry identities, by the CLEAR MOT mapping rule
 * (Bernardin & Stiefelhagen 2008) under keypoint OKS, one block per stream. What MOTA, MOTP and IDF1 are accumulated from.
 *
 *   mpn_track_eval   record: what mpn_pose_gather[_sized] wrote for (B, max_boxes), DEVICE, read in place exactly as
 *                     mpn_pose_track reads it (the header's total and counts, clamped the same way; only rows 0 .. total-1;
 *                     of a row only keypoints[17][3]).
 *                   track_rows: the `out` of mpn_pose_track for the same record, DEVICE; of a row only int32 track_id is read.
 *                     A row with id 0 is UNTRACKED: it takes no part below and is only counted.
 *                   gt f64 [B, max_gt, 64], gt_counts int32 [B] DEVICE: mpn_oks_match's rows, unchanged (a count above max_gt
 *                     reads max_gt rows); of a row the keypoints, bbox, area and the ignore flag are read.
 *                   gt_identity int32 [B, max_gt] DEVICE: the person's dense identity index within its stream. A value outside
 *                     0 .. max_identities-1 means the row has NO MEMORY: its stored id reads as 0 and nothing is stored.
 *                   Streams: B = streams * F, stream s owns images s*F .. s*F+F-1 in time order, as in mpn_pose_track.
 *                   PURE, as mpn_pose_track and for the same reason: the launch reads prev and writes the COMPLETE new state
 *                     to next and the rows to out; it never writes prev, and running it twice in a row gives the same bytes.
 *                     The caller advances the state by copying next over prev. prev == next is refused (MPN_ERR_BAD_ARG).
 *                   State, prev and next, mpn_track_eval_state_bytes(streams, max_identities) bytes DEVICE, per stream in
 *                     32-bit words: int32 frames (the frames evaluated), three zero words; then max_identities int32: the
 *                     track id the identity was last matched to, 0 = never. An all-zero state is the valid empty state.
 *                   Similarity s(g, h) of ground-truth row g and record row h: mpn_oks_match's f64 OKS (the v > 0 keypoints
 *                     of the ground truth, or the distance to its doubled box when it has none; the ground truth's own area),
 *                     without contraction. The pair is ELIGIBLE when h is tracked and s >= threshold; a NaN never is.
 *                   Per frame, in this order; `stored(g)` is the state's value for g's identity as the stream's earlier frames
 *                     left it (0 without memory):
 *                     1. kept correspondences: the ground truths that are not ignored, in row order: if stored(g) != 0 and a
 *                        tracked row h of the frame has track_id == stored(g), (g, h) is eligible and h is not yet taken, g
 *                        is matched to h (flag "kept"; of several such rows the lowest).
 *                     2. the ground truths that are neither ignored nor kept and the tracked rows that are not taken are
 *                        matched by the maximum-weight matching of their eligible pairs: weight w = q + 1 + 2^27 with q =
 *                        floor(s * 2^20) clamped to 0 .. 2^20 (mpn_pose_track_optimal's quantum). 64 quanta sum to less than
 *                        2^27, so a matching with more pairs outweighs any with fewer, and among those of equal size the
 *                        larger sum of quanta wins. The algorithm is the one stated under mpn_pose_track_optimal, word for
 *                        word, with rows i = 1..ng ALL the image's ground truths in row order (an ignored or kept one has
 *                        no eligible pair and lands on its dummy at delta 0, which moves no potential: leaving such rows
 *                        out, as the kernel does, changes nothing), columns j = 1..n the image's record rows,
 *                        j = n+1..n+ng the dummies, cost(i, j) = -w where eligible.
 *                     3. a tracked row that is unmatched and has an eligible pair with any ignored ground truth is IGNORED.
 *                     4. a matched ground truth whose stored id is non-zero and differs from the matched track_id is a
 *                        SWITCH; every matched ground truth with memory stores its track_id (in row order: of two rows with
 *                        one identity index the later); an unmatched ground truth that is not ignored is a MISS; a tracked
 *                        row that is neither matched nor ignored is a FALSE POSITIVE.
 *                   out: out_bytes >= mpn_track_eval_out_bytes(B, max_boxes, max_gt) DEVICE, three tables one behind the other:
 *                     B frame rows of 48 bytes: int32 num_gt (not ignored), num_hyp (tracked and not ignored), matches
 *                       (switches included), switches, misses, false_positives, ignored_hyp, untracked; f64 the sum of the
 *                       matched pairs' unquantised s, added in ground-truth row order from 0.0; 8 bytes of zero.
 *                     B * max_gt ground-truth rows of 32 bytes, row (image, g); rows g >= the image's count are zero: int32
 *                       the matched track_id (0 = none), int32 the matched row's index among the image's persons (-1 =
 *                       none), int32 flags (bit 0 matched, bit 1 switch, bit 2 kept, bit 3 ignored), int32 stored(g) before
 *                       the frame, f64 s of the match (0 = none), uint64 overlap mask: bit p set when person p of the image
 *                       is tracked and (g, p) is eligible (for ignored rows too).
 *                     B * max_boxes rows of 8 bytes aligned with the record's rows 0 .. total-1, every other row zero: int32
 *                       the matched ground truth's index in its image or -1; int32 flags (bit 0 false positive, bit 1
 *                       ignored, bit 2 untracked).
 *                   Checked before any HIP call, the messages begin "track_eval:": null pointers (MPN_ERR_BAD_ARG);
 *                     streams >= 1, B % streams == 0, 1 <= max_boxes <= 64, B * max_boxes <= 4096, 1 <= max_gt <= 64,
 *                     1 <= max_identities <= 1024 (MPN_ERR_BAD_SHAPE); a NaN threshold (MPN_ERR_BAD_ARG); record 16-byte,
 *                     track_rows / gt / prev / next / out 8-byte, gt_counts / gt_identity 4-byte aligned
 *                     (MPN_ERR_BAD_ALIGN); prev == next (MPN_ERR_BAD_ARG); state_bytes and out_bytes (MPN_ERR_WORKSPACE). The
 *                     grid depends on streams alone: a captured launch serves any later record, ground truth and state.
 *   mpn_track_eval_state_bytes   streams * (16 + 4 * max_identities); 0 for arguments out of range.
 *   mpn_track_eval_out_bytes     B * (48 + 32 * max_gt + 8 * max_boxes); 0 for arguments out of range.
 */
size_t mpn_track_eval_state_bytes(int streams, int max_identities);
size_t mpn_track_eval_out_bytes(int B, int max_boxes, int max_gt);
int mpn_track_eval(const void* record, const void* track_rows, int B, int max_boxes, int streams, const double* gt,
                   const int* gt_counts, const int* gt_identity, int max_gt, int max_identities, double threshold,
                   const void* prev, void* next, size_t state_bytes, void* out, size_t out_bytes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Zones and counting lines: which persons stand inside which polygon, who entered and who left (debounced), how long each stayed,
 * and who crossed a line in which direction, per tracked identity, with cumulative counters. One block per stream.
 * tests/zones_ref.py is this definition as plain loops.
 *
 *   mpn_zone_events   record: what mpn_pose_gather[_sized] or mpn_pose_nms wrote for (B, max_boxes), DEVICE, read in place
 *                     exactly as mpn_pose_smooth reads it (the header's total and counts, clamped the same way; only rows
 *                     0 .. total-1; of a row only its box (ymin, xmin, ymax, xmax, normalised), its score and
 *                     keypoints[17][3] = (x, y, score) in pixels).
 *                   track_rows: the `out` of mpn_pose_track* for the same record, DEVICE; of a row only int32 track_id is
 *                     read. The tracker's slot is NOT used: the stage keeps its own table keyed by id, so that ids from any
 *                     tracker serve.
 *                   Streams: B = streams * F, stream s owns images s*F .. s*F+F-1 in time order, as in mpn_pose_track.
 *                   PURE, as mpn_pose_smooth and for the same reason: the launch reads prev and writes the COMPLETE new state
 *                     to next and the rows to out; it never writes prev, and running it twice in a row gives the same bytes.
 *                     The caller advances the state by copying next over prev. prev == next is refused (MPN_ERR_BAD_ARG).
 *                   table: mpn_zone_table_bytes() = 4712 bytes DEVICE, built by the host once: int32 num_zones (0..16),
 *                     num_lines (0..16), min_frames (1..255), anchor (0 feet, 2 box_centre, anything else box_bottom); at byte
 *                     16 f64 height, width, min_keypoint_score; at byte 40 int32 vertex_count[16] (3..16); at byte 104 f64
 *                     vertices[16][16][2] as (x, y) in the pixels of the keypoints; at byte 4200 f64 lines[16][2][2], (P, Q) as
 *                     (x, y). The launcher cannot read device memory: the kernel CLAMPS every count into its range, so a bad
 *                     table gives wrong answers and indexes nothing out of range; range checks are the caller's.
 *                   Every operation below is one IEEE f64 operation in the order written, without contraction; f32 inputs are
 *                     widened first.
 *                   Anchor C of a row. feet: the ankles are joints 15 and 16; one PASSES when score >= min_keypoint_score (a
 *                     NaN never does). Both pass: ((x15 + x16) * 0.5, (y15 + y16) * 0.5); one passes: its (x, y); neither:
 *                     box_bottom. box_bottom: ((xmin + xmax) * 0.5 * width, ymax * height). box_centre: ((xmin + xmax) * 0.5 *
 *                     width, (ymin + ymax) * 0.5 * height). A row whose anchor has a non-finite coordinate HAS NO ANCHOR: its
 *                     output row is zero but for flag bit 2, it takes no slot and touches no state.
 *                   inside(z, C), the crossing number without a division: over the edges (x1, y1) -> (x2, y2) of zone z, the
 *                     one from its last vertex to its first included: an edge counts only if (y1 > Cy) != (y2 > Cy); then
 *                     t = (x2 - x1) * (Cy - y1) - (Cx - x1) * (y2 - y1), and the edge is crossed when y2 > y1 ? t > 0 : t < 0.
 *                     C is inside when the number of crossed edges is odd. (Of an axis-aligned rectangle the sides with the smaller x and the smaller y
 *                     belong to the zone, the other two do not: the rule decides, nothing is fuzzy.)
 *                   crossed(l, A, C), line l from P to Q, movement from A to C: d(X) = (Qx - Px) * (Xy - Py) - (Qy - Py) *
 *                     (Xx - Px), e(X) = (Cx - Ax) * (Xy - Ay) - (Cy - Ay) * (Xx - Ax). Crossed when (d(A) > 0) != (d(C) > 0)
 *                     and (e(P) > 0) != (e(Q) > 0); POSITIVE when d(C) > 0, else NEGATIVE.
 *                   State, prev and next, mpn_zone_state_bytes(streams) bytes DEVICE, per stream 1860 32-bit words: int32
 *                     frames, three zero words; cumulative uint32 zone_entries[16], zone_exits[16], line_positive[16],
 *                     line_negative[16]; then 64 slots (always 64: mpn_pose_track's largest table) of 28 words: int32 id (0 =
 *                     never used), uint32 inside (the confirmed membership mask), int32 last (the stream's frame number of the
 *                     last observation, 0 = none), one zero word, f64 ax, ay (the anchor of that observation), int32
 *                     entered_frame[16], uint8 run[16]. An all-zero state is the valid empty state. Frame numbers count from 1
 *                     and are NOT guarded against wrap, as in mpn_pose_smooth.
 *                   Per frame j of the launch (0 <= j < F), now = prev.frames + j + 1:
 *                     1. slots: the image's rows with track_id > 0 and an anchor, serially in row order (the one step whose
 *                        order matters). The row takes the lowest slot with id == track_id; if an earlier row of this frame
 *                        took that slot (two rows with one id), the row is handled as UNTRACKED. If no slot has the id, the row
 *                        takes, among the slots no earlier row of this frame took, the one with the smallest `last` (as int32),
 *                        the lowest index on a tie - a never-used slot has last = 0 and goes first - and resets it to {id =
 *                        track_id, every other word 0}. 64 slots and at most 64 rows per frame: there is always one.
 *                     2. zones, a row with a slot: for every zone z < num_zones, raw = inside(z, C). raw equal to the slot's
 *                        confirmed bit: run[z] = 0. Otherwise run[z] + 1 >= min_frames flips the bit with run[z] = 0 - to
 *                        inside: the row ENTERED, entered_frame[z] = now; to outside: the row EXITED, entered_frame[z] = 0 -
 *                        and else run[z] += 1. dwell[z] = now - entered_frame[z] + 1 while the bit is set, else 0. Frames in
 *                        which the person is not observed do not step run.
 *                     3. lines, a row whose slot had last != 0 before this frame: crossed(l, A, C) for every l < num_lines with
 *                        A the slot's stored anchor, however many frames ago. Lines are not debounced.
 *                     4. the slot's anchor becomes C, last = now.
 *                     5. every other row with an anchor (track_id <= 0, or the second of two rows with one id) is UNTRACKED:
 *                        inside is its raw mask, it has no events, dwell 0; no state is touched.
 *                     The counters take the frame's events as integer adds. Slots that no row names are copied from prev to next
 *                     unchanged; next.frames = prev.frames + F. A frame without detections still counts.
 *                   out: mpn_zone_out_bytes(B, max_boxes) bytes DEVICE. B * max_boxes person rows of 104 bytes aligned with the
 *                     record's rows 0 .. total-1, every row behind total zero: uint32 inside, entered, exited,
 *                     crossed_positive, crossed_negative (bit z or l), flags (bit 0 tracked: the row has a slot; bit 1 the
 *                     anchor came from the ankles; bit 2 no anchor), f64 anchor[2] = (x, y), int32 dwell[16]. Behind them B
 *                     image rows of uint32 [9][16]: occupancy (the image's rows whose inside bit is set, untracked ones
 *                     included), entries, exits, positive, negative (this frame's events), total_entries, total_exits,
 *                     total_positive, total_negative (cumulative, after this frame).
 *                   Checked before any HIP call, the messages begin "zone_events:": null pointers, prev == next
 *                     (MPN_ERR_BAD_ARG); streams >= 1, B % streams == 0, 1 <= max_boxes <= 64, B * max_boxes <= 4096
 *                     (MPN_ERR_BAD_SHAPE); record 16-byte, track_rows / table / prev / next / out 8-byte aligned
 *                     (MPN_ERR_BAD_ALIGN). The grid depends on streams alone: a captured launch serves any later record, table
 *                     contents and state.
 *   mpn_zone_table_bytes   4712.
 *   mpn_zone_state_bytes   streams * 7440; 0 for arguments out of range.
 *   mpn_zone_out_bytes     B * max_boxes * 104 + B * 576; 0 for arguments out of range.
 */
size_t mpn_zone_table_bytes(void);
size_t mpn_zone_state_bytes(int streams);
size_t mpn_zone_out_bytes(int B, int max_boxes);
int mpn_zone_events(const void* record, const void* track_rows, int B, int max_boxes, int streams, const void* table,
                    const void* prev, void* next, void* out, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Motion trails: where each tracked identity has been - a ring of its last K anchors in device state - returned per person as
 * a polyline, newest point first, and drawn into the annotated frames. tests/trails_ref.py is this definition as plain loops.
 *
 *   mpn_track_trails  record, track_rows, streams: as for mpn_zone_events (the header's total and counts, clamped the same way;
 *                     only rows 0 .. total-1; of a row its box and keypoints; of a track row only int32 track_id at byte 0 of a
 *                     24-byte row). B = streams * F, stream s owns images s*F .. s*F+F-1 in time order.
 *                   PURE, as mpn_zone_events: the launch reads prev and writes the COMPLETE new state to next and the rows to
 *                     out; it never writes prev, and running it twice in a row gives the same bytes. The caller advances the
 *                     state by copying next over prev. prev == next is refused (MPN_ERR_BAD_ARG).
 *                   By value: length K (1..64), the points a trail keeps; every (1..255), a point is kept once per `every`
 *                     frames; max_gap (0 = never restart, else 1..65535), an identity not observed for more than max_gap frames
 *                     starts a new trail; anchor (0 feet, 2 box_centre, anything else box_bottom); min_keypoint_score; height,
 *                     width of the frames in the pixels of the keypoints; with_keypoints (0: the record has no keypoints, feet
 *                     reads box_bottom).
 *                   Anchor C of a row: exactly mpn_zone_events' rule - every operation one IEEE f64 operation in the order
 *                     written there, without contraction, f32 inputs widened first; the ankles are joints 15 and 16 and one
 *                     PASSES when score >= min_keypoint_score (a NaN never does); both pass: ((x15 + x16) * 0.5, (y15 + y16) *
 *                     0.5); one passes: its (x, y); neither: box_bottom ((xmin + xmax) * 0.5 * width, ymax * height);
 *                     box_centre ((xmin + xmax) * 0.5 * width, (ymin + ymax) * 0.5 * height). Each coordinate is then rounded
 *                     ONCE to f32. A coordinate that is not finite before or after that rounding means NO ANCHOR: the output row
 *                     is zero but for flag bit 2, the row takes no slot and touches no state.
 *                   State, prev and next, mpn_track_trails_state_bytes(streams, K) bytes DEVICE, per stream 16 + 64 * (32 + 8*K)
 *                     bytes: int32 frames, three zero words; then 64 slots (always 64, as in mpn_zone_events), each int32 id (0 =
 *                     never used), last (the stream's frame number of the last observation, 0 = none), last_append (that of the
 *                     last point kept), count (points in the ring, 0..K), head (the index of the newest), three zero words, then
 *                     f32 ring[K][2] as (x, y). An all-zero state is the valid empty state. Frame numbers count from 1 and are
 *                     NOT guarded against wrap. count and head of a state this launch did not write are clamped into range.
 *                   Per frame j of the launch (0 <= j < F), now = prev.frames + j + 1:
 *                     1. slots: mpn_zone_events' rule word for word. The image's rows with track_id > 0 and an anchor, serially
 *                        in row order: the row takes the lowest slot with id == track_id; if an earlier row of this frame took
 *                        that slot (two rows with one id), the row is handled as UNTRACKED. If no slot has the id, the row takes,
 *                        among the slots no earlier row of this frame took, the one with the smallest `last` (as int32), the
 *                        lowest index on a tie, and resets it to {id = track_id, every other word 0, the ring included}.
 *                     2. restart: count > 0, max_gap > 0 and now - last > max_gap: every word of the slot but id becomes 0, the
 *                        ring included; the row is RESTARTED (flag bit 4).
 *                     3. append: count == 0 or now - last_append >= every: head = (count == 0) ? 0 : (head + 1) % K; ring[head] =
 *                        C; count = min(count + 1, K); last_append = now; the row is APPENDED (flag bit 3).
 *                     4. last = now.
 *                     5. the row's points, newest first. Appended: ring[(head - i + K) % K] for i < count, n = count.
 *                        Otherwise C, then those: n = count + 1 <= K + 1.
 *                     6. every other row with an anchor (track_id <= 0, or the second of two rows with one id) is UNTRACKED:
 *                        n = 1, points[0] = C, flag bit 0 clear; no state is touched.
 *                     Slots that no row names are copied from prev to next unchanged; next.frames = prev.frames + F. A frame
 *                     without detections still counts.
 *                   out: mpn_track_trails_out_bytes(B, max_boxes, K) bytes DEVICE: B * max_boxes rows of 8 * (K + 2) bytes
 *                     aligned with the record's rows 0 .. total-1, every row behind total zero: int32 n, uint32 flags (bit 0
 *                     tracked: the row has a slot; bit 1 the anchor came from the ankles; bit 2 no anchor; bit 3 appended; bit 4
 *                     restarted), f32 points[K + 1][2] as (x, y), zero behind n.
 *                   Checked before any HIP call, the messages begin "track_trails:": null pointers, prev == next, length, every,
 *                     max_gap outside their ranges, a non-finite height, width or min_keypoint_score (MPN_ERR_BAD_ARG);
 *                     streams >= 1, B % streams == 0, 1 <= max_boxes <= 64, B * max_boxes <= 4096 (MPN_ERR_BAD_SHAPE); record
 *                     16-byte, track_rows / prev / next / out 8-byte aligned (MPN_ERR_BAD_ALIGN). One block per stream: the
 *                     grid depends on streams alone.
 *   mpn_track_trails_state_bytes   streams * (16 + 64 * (32 + 8 * length)); 0 for arguments out of range.
 *   mpn_track_trails_out_bytes     B * max_boxes * 8 * (length + 2); 0 for arguments out of range.
 *
 *   mpn_draw_trails   the rows of mpn_track_trails as polylines over the RGBA frames mpn_draw_detections / mpn_draw_tracks
 *                     wrote, IN PLACE. descs: the same [B] mpn_draw_desc array; out_offset, h, w are read. record: the header's
 *                     total and counts say which rows belong to which image (clamped to the record's capacity). track_rows: as
 *                     above. trail_rows: mpn_track_trails' out for the same record and length; n is clamped to 0 .. length + 1.
 *                   Draw order: per image, in record row order, every row with flag bit 0, n >= 2 and track_id > 0 is a
 *                     polyline. Its segment s (0 <= s <= n-2) runs from points[s+1] to points[s]; segments are drawn OLDEST
 *                     first: s = n-2, ..., 0. End points: each f32 coordinate clamped to +-2^29 (a NaN becomes -2^29), then
 *                     truncated toward zero. The pixel set of a segment is exactly the `line` rule of mpn_draw_detections, from
 *                     the first (older) point: end point included, a zero-length segment is one pixel, clipped to the frame per
 *                     pixel.
 *                   Ink: palette[(track_id - 1) % P] with alpha a_s = 255 without the fade flag, else
 *                     a_s = 255 - (s * (255 - min_alpha)) / max(K - 1, 1) in integer division: the newest segment is opaque. A
 *                     pixel of a segment becomes, per colour channel, BLEND8(a_s, pixel, ink): t = a_s*ink + (255 - a_s)*pixel +
 *                     128; ((t >> 8) + t) >> 8; its alpha byte becomes 255. Segments are applied IN ORDER: a pixel that two
 *                     segments cover is blended twice - the joint pixel every two neighbours share included. That is what
 *                     Pillow draws with ImageDraw.Draw(rgb, 'RGBA').line([older, newer], fill=(r, g, b, a_s), width=1) once per
 *                     segment (tests/test_trails_host.py holds the restatement against Pillow).
 *                   tables: DEVICE, 4-byte aligned, tables_bytes >= MPN_DRAW_TRAILS_TABLE_HEADER_BYTES; int32 words: 0 flags
 *                     (bit 0 fade), 1 min_alpha (clamped to 0..255), 2 K of the fade formula (clamped to 1..64), 3 P, the
 *                     palette's size, 1..MPN_DRAW_TRACKS_MAX_PALETTE, 4 .. 3 + P the palette, one colour per word as
 *                     mpn_draw_tracks packs it (R | G<<8 | B<<16). mpn_draw_trails_tables_bytes(P): 16 + 4*P rounded up to 16; 0
 *                     out of range. The table is DATA: a palette that does not lie inside tables_bytes leaves every trail
 *                     undrawn.
 *                   In place: a pixel is read and written by exactly one thread, with 4-byte accesses - no scatter, no atomics on
 *                     global memory; pixels no segment covers are neither read nor written. The launch is therefore NOT
 *                     IDEMPOTENT with the fade flag (or wherever a_s < 255): run twice over the same frame it blends twice. In
 *                     the Detector's graph it always follows a draw launch that rewrote the whole frame, so replaying the graph's
 *                     device side is still harmless. An image whose descriptor reaches outside out_bytes, or has h, w outside
 *                     what mpn_draw_detections accepts, is left alone.
 *                   workspace: mpn_draw_trails_workspace_bytes(B, max_boxes, length) bytes (B * max_boxes * (48 * length + 32);
 *                     0 out of range), 16-byte aligned. Two launches whose grids depend on (B, max_boxes, length) alone: build
 *                     (a thread per row and segment: end points, bounding box, ink, alpha; and a bounding box per trail), then
 *                     the raster, which culls per wave by the trail's box, then by the segment's.
 *                   Checked before any HIP call, with mpn_draw_tracks' codes, the messages begin "draw_trails:": null pointers
 *                     (MPN_ERR_BAD_ARG); 1 <= B <= 65535, 1 <= max_boxes <= MPN_DRAW_MAX_BOXES, B * max_boxes <= 4096,
 *                     1 <= length <= 64 (MPN_ERR_BAD_SHAPE); descs, record, out_rgba, workspace 16-byte, track_rows, trail_rows,
 *                     tables 4-byte aligned (MPN_ERR_BAD_ALIGN); record_bytes, workspace_bytes, out_bytes >= 16, tables_bytes >=
 *                     the header (MPN_ERR_WORKSPACE).
 */
#define MPN_DRAW_TRAILS_TABLE_HEADER_BYTES 16
size_t mpn_track_trails_state_bytes(int streams, int length);
size_t mpn_track_trails_out_bytes(int B, int max_boxes, int length);
int mpn_track_trails(const void* record, const void* track_rows, int B, int max_boxes, int streams, int length, int every,
                     int max_gap, int anchor, double min_keypoint_score, double height, double width, int with_keypoints,
                     const void* prev, void* next, void* out, mpn_stream_t stream);
size_t mpn_draw_trails_tables_bytes(int palette_size);
size_t mpn_draw_trails_workspace_bytes(int B, int max_boxes, int length);
int mpn_draw_trails(const void* descs, const void* record, size_t record_bytes, const void* track_rows, const void* trail_rows,
                    const void* tables, size_t tables_bytes, int B, int max_boxes, int length, uint8_t* out_rgba, size_t out_bytes,
                    void* workspace, size_t workspace_bytes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Density maps: where in the picture persons stand, and how much - two planes of counters over a grid of square cells in device
 * state, dwell (person-frames per cell) and visits (arrivals of an identity in a cell) - returned per person as the cell it
 * stands in and laid over the annotated frames as a colour wash. tests/density_ref.py is this definition as plain loops.
 *
 *   mpn_density_map   record, streams: as for mpn_track_trails (the header's total and counts, clamped the same way; only rows
 *                     0 .. total-1; of a row its box and keypoints). track_rows: mpn_pose_track's rows for the record (of a row
 *                     only int32 track_id at byte 0 of a 24-byte row), or NULL: no identities - every row is untracked, step 2
 *                     is skipped and the visits plane only ages. B = streams * F, stream s owns images s*F .. s*F+F-1 in time
 *                     order.
 *                   PURE, as mpn_track_trails: the launch reads prev and writes the COMPLETE new state to next, the rows to out
 *                     and the snapshots; it never writes prev, and running it twice in a row gives the same bytes. The caller
 *                     advances the state by copying next over prev. prev == next is refused (MPN_ERR_BAD_ARG).
 *                   By value: height, width of the frames in pixels (1..8192 each); cell, the side of a cell in pixels (4..256):
 *                     the grid is gh = ceil(height / cell) rows of gw = ceil(width / cell) cells, G = gh * gw <= 16384, cell
 *                     (r, c) has index r * gw + c; the last row and column may be ragged. footprint (0 anchor, 1 box); anchor
 *                     (0 feet, 2 box_centre, anything else box_bottom); min_keypoint_score; with_keypoints (0: the record has
 *                     no keypoints, feet reads box_bottom); half_life (0 = never, else 1..65535 frames); show (0 dwell, 1
 *                     visits: the plane the snapshots copy; 1 needs track_rows).
 *                   Anchor C of a row: exactly mpn_zone_events' rule, in f64, NOT rounded to f32 (csrc/person_anchor.h holds
 *                     the rule for all three stages). A coordinate that is not finite means NO ANCHOR: the output row is
 *                     {-1, -1, flag bit 2, 0}, the row takes no slot and adds nothing.
 *                   The anchor's cell: the row is INSIDE when 0 <= Cx < width and 0 <= Cy < height (f64 comparisons); then
 *                     col = (int)Cx / cell, row = (int)Cy / cell - truncation, then integer division - and k = row * gw + col.
 *                     A row with an anchor that is not INSIDE is OUTSIDE (flag bit 3; row = col = -1).
 *                   State, prev and next, mpn_density_state_bytes(streams, gh, gw) bytes DEVICE, per stream 32 + 64 * 16 + 8 * G
 *                     bytes: int32 frames; uint32 max_dwell, max_visits; five zero words; then 64 slots (always 64, as in
 *                     mpn_zone_events), each int32 id (0 = never used), last (the stream's frame number of the last observation,
 *                     0 = none), cell1 (1 + the cell the identity was last seen INSIDE, 0 = none or OUTSIDE), one zero word; then
 *                     uint32 dwell[G], then uint32 visits[G]. An all-zero state is the valid empty state. Frame numbers count
 *                     from 1 and are NOT guarded against wrap.
 *                   Per frame j of the launch (0 <= j < F), now = prev.frames + j + 1, in this order:
 *                     1. halving: half_life > 0 and now % half_life == 0: every cell of both planes, max_dwell and max_visits
 *                        become v >> 1. Stepwise, not exponential: between two halvings nothing ages.
 *                     2. slots (not without track_rows): mpn_zone_events' rule word for word. The image's rows with
 *                        track_id > 0 and an anchor, serially in row order: the row takes the lowest slot with id == track_id;
 *                        if an earlier row of this frame took that slot (two rows with one id), the row is handled as
 *                        UNTRACKED. If no slot has the id, the row takes, among the slots no earlier row of this frame took, the
 *                        one with the smallest `last` (as int32), the lowest index on a tie, and resets it to {id = track_id,
 *                        every other word 0}.
 *                     3. a row with a slot (flag bit 0). INSIDE: when slot.cell1 != k + 1 the row is a VISIT (flag bit 4) and
 *                        visits[k] takes a saturating + 1; then cell1 = k + 1. OUTSIDE: cell1 = 0 - coming back to the old cell
 *                        is a visit again. In both cases last = now.
 *                     4. dwell: every row with an anchor, tracked or not, adds a saturating + 1 to the cells of its footprint.
 *                        anchor: INSIDE rows, cell k. box: every cell (r, c) with x0 <= (2*c + 1) * cell * 0.5 < x1 and
 *                        y0 <= (2*r + 1) * cell * 0.5 < y1 - the cells whose centre the box covers - where x0 = xmin * width,
 *                        x1 = xmax * width, y0 = ymin * height, y1 = ymax * height in f64 (f32 inputs widened first); a bound
 *                        that is not finite adds nothing. Saturation is at 2^32 - 1; saturating adds commute, so the order of
 *                        the rows does not matter.
 *                     5. maxima: max_dwell = max(max_dwell, the new value of every cell step 4 added to); max_visits likewise
 *                        over step 3. (For a state this launch wrote from the empty one they are the planes' maxima: max(v >> 1)
 *                        == max(v) >> 1.)
 *                     6. snapshot: with snapshots, the `show` plane as it now stands is copied to snapshots[image].
 *                     Slots that no row names are copied from prev to next unchanged; next.frames = prev.frames + F. A frame
 *                     without detections still counts.
 *                   out: mpn_density_out_bytes(B, max_boxes) = B * max_boxes * 16 + B * 16 bytes DEVICE, 16-byte aligned:
 *                     B * max_boxes person rows aligned with the record's rows 0 .. total-1, every row behind total zero: int32
 *                     row, col (the anchor's cell, -1, -1 when it has none); uint32 flags (bit 0 tracked: the row has a slot;
 *                     bit 1 the anchor came from the ankles; bit 2 no anchor; bit 3 outside; bit 4 visit); uint32 cells, the
 *                     cells step 4 added to for this row. Behind them, per image: uint32 max_dwell, max_visits (after the
 *                     frame), counted (the frame's rows with cells > 0), visits (the frame's VISIT rows).
 *                   snapshots: NULL or mpn_density_snapshot_bytes(B, gh, gw) = B * G * 4 bytes DEVICE: uint32 [B][G].
 *                   Checked before any HIP call, the messages begin "density_map:": null pointers other than track_rows and
 *                     snapshots, prev == next, cell outside 4..256, height or width outside 1..8192, G > 16384, footprint not 0
 *                     or 1, half_life outside 0..65535, show not 0 or 1, show == 1 without track_rows, a non-finite
 *                     min_keypoint_score (MPN_ERR_BAD_ARG); streams >= 1, B % streams == 0, 1 <= max_boxes <= 64, B * max_boxes
 *                     <= 4096 (MPN_ERR_BAD_SHAPE); record and out 16-byte, track_rows / prev / next / snapshots 8-byte aligned
 *                     (MPN_ERR_BAD_ALIGN). One block per stream: the grid depends on streams alone.
 *   mpn_density_state_bytes      streams * (32 + 64 * 16 + 8 * gh * gw); 0 for arguments out of range (gh * gw > 16384).
 *   mpn_density_out_bytes        B * max_boxes * 16 + B * 16; 0 for arguments out of range.
 *   mpn_density_snapshot_bytes   B * gh * gw * 4; 0 for arguments out of range.
 *
 *   mpn_draw_density  the snapshots as a colour wash over the RGBA frames mpn_draw_detections / mpn_draw_tracks (and
 *                     mpn_draw_trails) wrote, IN PLACE. descs: the same [B] mpn_draw_desc array; out_offset, h, w are read.
 *                     snapshots, rows: mpn_density_map's snapshots and out for the same B, max_boxes, height, width and cell; of
 *                     rows only the image rows are read.
 *                   An image is LEFT ALONE when its descriptor has (h, w) != (height, width), reaches outside out_bytes (or is
 *                     one mpn_draw_detections would not write), or when its M (below) is 0.
 *                   tables: DEVICE, 4-byte aligned, tables_bytes >= MPN_DRAW_DENSITY_TABLE_BYTES = 32 + 1024; 32-bit words:
 *                     0 int32 flags (bit 0 smooth; bit 1 the snapshots show visits: M is read from max_visits), 1 uint32
 *                     full_scale, 2..7 zero, 8..263 the colours of levels 0..255 as R | G<<8 | B<<16 | A<<24. The host fills
 *                     A[l] = (opacity * l + 127) / 255 and A[0] = 0. The table is DATA: the kernel clamps what it indexes with.
 *                   Cell level: M = full_scale, or with full_scale == 0 the image row's maximum of the shown plane;
 *                     L(cell) = min(255, (255 * v + M / 2) / M) in 64-bit integers.
 *                   Pixel level without smooth: L(y / cell, x / cell). With smooth, bilinear between the cells' centres in
 *                     integers, s = cell: u = 2*x + 1 - s; c0 = floor(u / (2*s)); fx = u - c0 * 2*s; c1 = c0 + 1; c0 and c1
 *                     clamped to 0..gw-1; rows likewise from y: r0, r1, fy;
 *                     level = (L00*(2s-fx)*(2s-fy) + L01*fx*(2s-fy) + L10*(2s-fx)*fy + L11*fx*fy + 2*s*s) / (4*s*s), Lrc the
 *                     level of cell (r, c) named by r0/r1 and c0/c1. (Below 2^31 in 32-bit integers.)
 *                   Blend: where A[level] > 0 every colour channel becomes BLEND8(A[level], pixel, ink[level]) as mpn_draw_trails
 *                     defines it and the alpha byte becomes 255; other pixels keep their bytes. That is Pillow's
 *                     frame.paste(colour_image, (0, 0), mask=alpha_image) on an RGB frame (tests/test_density_host.py holds the
 *                     restatement against Pillow).
 *                   In place: every pixel is read and written by exactly one thread, four pixels per 16-byte access; no scatter,
 *                     no atomics. NOT IDEMPOTENT: run twice over the same frame it blends twice. In the Detector's graph it
 *                     always follows a draw launch that rewrote the whole frame.
 *                   workspace: mpn_draw_density_workspace_bytes(B, gh, gw) bytes (B * G rounded up to 16; 0 out of range),
 *                     16-byte aligned: the levels as bytes [B][G]. Two launches whose grids depend on (B, height, width, gh, gw)
 *                     alone: the levels (a thread per image and cell), then the raster.
 *                   Checked before any HIP call, the messages begin "draw_density:": null pointers (MPN_ERR_BAD_ARG); 1 <= B <=
 *                     65535, 1 <= max_boxes <= 64, B * max_boxes <= 4096, height, width, cell and G as above
 *                     (MPN_ERR_BAD_SHAPE); descs, rows, out_rgba, workspace 16-byte, snapshots, tables 4-byte aligned
 *                     (MPN_ERR_BAD_ALIGN); workspace_bytes, out_bytes >= 16, tables_bytes (MPN_ERR_WORKSPACE).
 */
#define MPN_DRAW_DENSITY_TABLE_BYTES 1056
size_t mpn_density_state_bytes(int streams, int gh, int gw);
size_t mpn_density_out_bytes(int B, int max_boxes);
size_t mpn_density_snapshot_bytes(int B, int gh, int gw);
int mpn_density_map(const void* record, const void* track_rows, int B, int max_boxes, int streams, int height, int width, int cell,
                    int footprint, int anchor, double min_keypoint_score, int with_keypoints, int half_life, int show,
                    const void* prev, void* next, void* out, void* snapshots, mpn_stream_t stream);
size_t mpn_draw_density_tables_bytes(void);
size_t mpn_draw_density_workspace_bytes(int B, int gh, int gw);
int mpn_draw_density(const void* descs, const void* snapshots, const void* rows, const void* tables, size_t tables_bytes, int B,
                     int max_boxes, int height, int width, int cell, uint8_t* out_rgba, size_t out_bytes, void* workspace,
                     size_t workspace_bytes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The `masks` feature of a COCO keypoint record (the pixel work of the reference's data/create_tfrecords.py): the persons'
 * segmentations of a RAGGED batch of images -> per image the loss mask and the segmentation mask at full resolution ->
 * Lanczos4 to quarter size -> `> 0` -> packed bits. Three launches whatever the batch holds (zero, parts, finish); no
 * synchronisation. DESIGN.md section 21 has the semantics in full; tests/coco_mask_ref.py is their definition.
 *
 *   images   DEVICE [num_images]: sides h, w in 1..max_side; plane_offset: 32-bit words into `workspace`, where the image's
 *              mpn_coco_masks_plane_words(h, w) words lie; packed_offset: bytes into `packed`, where its
 *              mpn_coco_masks_packed_bytes(h, w) bytes go; full_offset: bytes into `full` (h * w * 2 of them; unused
 *              without `full`); tap_x, tap_y: first entry of its ceil(w/4) horizontal and ceil(h/4) vertical taps.
 *   parts    DEVICE [num_parts]: one polygon or one run-length code of a person of image `image`. flags:
 *              MPN_COCO_PART_DROPPED - the person is masked out of the loss (else it belongs to the segmentation mask);
 *              MPN_COCO_PART_RLE - `offset` / `count` are uint32 run lengths in `runs` (COCO's order: column-major,
 *              starting with a run of zeros), else `count` vertices = 2 * count float64 (x, y) from `xy[offset]`.
 *              Polygon -> mask is COCO maskApi's rleFrPoly; the masks of a person's parts are united (OR).
 *              seg = OR over the kept persons, loss = AND over the dropped persons of (mask == 0).
 *   taps     DEVICE [num_taps][5] int32: {floor of the source coordinate s, then int16 weight[8]} of OpenCV's
 *              resize(INTER_LANCZOS4) for uint8: taps at s-3 .. s+4, indices clamped to the image, weights with 11
 *              fractional bits; horizontal integer sum, vertical integer sum, (x + 2^21) >> 22 saturated to 0..255.
 *   workspace  DEVICE, 16-byte aligned, workspace_bytes a multiple of 16: the images' bitmaps (zeroed by the call).
 *   packed   DEVICE: per image numpy.packbits(stack([loss, seg], 2) > 0) of the [ceil(h/4), ceil(w/4), 2] array: MSB first,
 *              the bit stream running across row ends, the last byte zero-padded.
 *   full     DEVICE or NULL: per image uint8 [h, w, 2] of 0 / 1 (loss, seg).
 * The tables are read on the device: a part or an image whose offsets, counts or sides do not fit the totals given here
 * (num_xy in doubles, num_runs, num_taps, the three byte counts, max_side) is skipped, nothing is indexed out of range.
 * Checked before any HIP call: max_side in 1..MPN_COCO_MASKS_MAX_SIDE, num_images in 1..65535, counts >= 0, num_taps >= 1
 * (MPN_ERR_BAD_SHAPE); null pointers (MPN_ERR_BAD_ARG; parts / xy / runs may be null with a count of 0); alignment
 * (MPN_ERR_BAD_ALIGN); workspace_bytes, packed_bytes, full_bytes (MPN_ERR_WORKSPACE).
 *   mpn_coco_masks_plane_words, mpn_coco_masks_packed_bytes   0 for a side outside 1..MPN_COCO_MASKS_MAX_SIDE.
 */
#define MPN_COCO_MASKS_MAX_SIDE 1024
#define MPN_COCO_PART_DROPPED 1
#define MPN_COCO_PART_RLE 2
typedef struct mpn_coco_image_desc {
    long long plane_offset, packed_offset, full_offset;
    int h, w, tap_x, tap_y;
} mpn_coco_image_desc;                          /* 40 bytes */
typedef struct mpn_coco_part_desc {
    long long offset;
    int count, image, flags, reserved;
} mpn_coco_part_desc;                           /* 24 bytes */
size_t mpn_coco_masks_image_desc_bytes(void);
size_t mpn_coco_masks_part_desc_bytes(void);
size_t mpn_coco_masks_plane_words(int h, int w);
size_t mpn_coco_masks_packed_bytes(int h, int w);
int mpn_coco_masks(const mpn_coco_image_desc* images, int num_images, int max_side, const mpn_coco_part_desc* parts,
                   int num_parts, const double* xy, long long num_xy, const uint32_t* runs, long long num_runs,
                   const int32_t* taps, long long num_taps, void* workspace, size_t workspace_bytes, void* packed,
                   size_t packed_bytes, void* full, size_t full_bytes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Resize of a batch of RAGGED uint8 RGB sources onto the network canvas, equal byte for byte to Pillow's
 * `Image.resize` of an 8-bit RGB image with its default filter (antialiased bicubic), the host step of the reference's
 * inference/predict.ipynb (cell 6), with the top-left placement of `pad_to_bounding_box`
 * (person_detector_pipeline.py:229-233) when an image is resized to less than the canvas.
 *
 * Pillow's resize is two separable passes of integer arithmetic over coefficient tables. The HOST builds the tables
 * (multiposenet_amd/inference/resample.py: bicubic a = -0.5, support 2*max(in/out, 1), float64 weights normalised by
 * their sum, fixed point with 22 fractional bits); the device computes, per pass and per byte,
 *     clip8((sum_k pixel[first + k] * coeff[k] + 2^21) >> 22)         in int32
 * horizontal pass first, its result ROUNDED TO uint8 (the intermediate), then the vertical pass. A pass whose input
 * and output sizes are equal is a copy (Pillow skips it: the same bytes).
 *
 *   sources    concatenated uint8 images [src_h, src_w, 3]; image b starts at byte src_offset. A pixel is read as one
 *              (unaligned) dword: the buffer must be readable 1 byte past its last image.
 *   tables     int32 words; of an axis with `out` outputs: bounds [out,2] = (first tap, tap count) at word bounds_*,
 *              coeffs [out,ksize_*] at word coeffs_*. 16-byte aligned.
 *   descs      [B] mpn_image_resize_desc, DEVICE, 16-byte aligned
 *   out_u8     [B,H,W,3] uint8, 16-byte aligned. EVERY byte is written: zero outside new_h x new_w.
 *   workspace  the uint8 intermediates: image b's [src_h rows of tmp_stride bytes] at byte tmp_offset (a multiple of 16;
 *              tmp_stride = new_w*3 rounded up to 16). 16-byte aligned. An image whose intermediate does not fit
 *              workspace_bytes, or whose new_h x new_w exceeds H x W, or whose ksize exceeds the maximum, is written as
 *              zeros: no descriptor makes the kernels WRITE outside workspace or out_u8. What they READ (offsets and
 *              sizes inside sources and tables) is the caller's to check.
 * Two launches (horizontal, vertical). Grid and block sizes depend on (B, H, W) alone; source sizes, tap counts and
 * offsets reach the kernels through device memory, so a captured graph serves any later mix of sources that fits its
 * buffers. Tap loops are bounded by the descriptor, up to MPN_IMAGE_RESIZE_MAX_KSIZE taps (a 16x reduction).
 * mpn_image_resize_workspace_bytes(B, H, W, src_rows): bytes that hold the intermediates of B images whose src_h sum to
 * src_rows (0 for arguments out of range).
 * Checked before any HIP call: null pointers (MPN_ERR_BAD_ARG); 1 <= B <= 65535, H, W >= 1, W*3 a multiple of 16
 * (MPN_ERR_BAD_SHAPE); alignment (MPN_ERR_BAD_ALIGN); workspace_bytes >= 16 (MPN_ERR_WORKSPACE).
 */
#define MPN_IMAGE_RESIZE_MAX_KSIZE 65
#define MPN_IMAGE_RESIZE_DESC_BYTES 64
typedef struct mpn_image_resize_desc {
    int64_t src_offset;                         /* byte offset into sources */
    int64_t tmp_offset;                         /* byte offset of the intermediate in workspace, multiple of 16 */
    int32_t src_h, src_w, new_h, new_w;
    int32_t bounds_x, coeffs_x;                 /* word offsets into tables: src_w -> new_w */
    int32_t bounds_y, coeffs_y;                 /* src_h -> new_h */
    int32_t ksize_x, ksize_y;                   /* row lengths of coeffs_x / coeffs_y */
    int32_t tmp_stride;                         /* bytes of an intermediate row: new_w*3 rounded up to 16 */
    int32_t reserved;
} mpn_image_resize_desc;
#ifdef __cplusplus
static_assert(sizeof(mpn_image_resize_desc) == MPN_IMAGE_RESIZE_DESC_BYTES, "descriptor size is fixed");
#endif
size_t mpn_image_resize_desc_bytes(void);
size_t mpn_image_resize_workspace_bytes(int B, int H, int W, long long src_rows);
int mpn_image_resize(const uint8_t* sources, const int32_t* tables, const void* descs, int B, int H, int W,
                     uint8_t* out_u8, void* workspace, size_t workspace_bytes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Annotated frames: `draw_everything` of the reference's inference/predict.ipynb (cells 10 and 12) for a batch of RAGGED
 * uint8 RGB frames and the persons of mpn_pose_gather[_sized]'s record, equal byte for byte to what Pillow draws there.
 *
 * out = the frame as RGBA with alpha 255; then per KEPT person of the record, in record order: the box outline in red
 * (255,0,0,255), the 16 skeleton lines in white (255,255,255,255), one pixel wide, and the 17 keypoints as red dots, each an
 * opaque overwrite of what was drawn before, clipped to the frame per pixel. Coordinates are the notebook's numpy arithmetic,
 * recomputed from the record's box and keypoint_positions (NOT its float32 `keypoints`, which round differently):
 *     (ymin, xmin, ymax, xmax) = (h, w, h, w) * box                               float64
 *     x = f32(f64(f32(f64(pos_x) * (xmax - xmin))) + xmin), y likewise            float64 results rounded to float32
 *     dot corners  x - 2, x + 2 (float32)
 * each converted to int by truncation toward zero (Pillow). Integer rasterisation:
 *     rectangle  rows y0 and y1 over x0..x1, columns x0 and x1 between them; a box with y1 == y0 also sets (x0, y0+1) and
 *                (x1, y0+1), as Pillow does; a box with x1 < x0 or y1 < y0 (Pillow raises) is not drawn
 *     line       Bresenham from the first point, end point included: at step i of the major axis the minor axis has moved
 *                floor((2*m*i + n) / (2*n)) steps, n = max(|dx|, |dy|), m = min(|dx|, |dy|)
 *     dot        over corners (x0,y0)-(x1,y1), x1-x0 and y1-y0 in {3, 4}: row j = bits MPN_DRAW_DOT_STAMPS
 *                [(x1-x0-3)*2 + (y1-y0-3)][j], bit i = pixel x0+i (mpn_draw_dot_stamp; -1 outside the table). Other
 *                differences need |x| beyond 2^22 and are not drawn.
 * Coordinates are clamped to +-2^29 first.
 *
 *   sources     concatenated uint8 images [h, w, 3]; image b starts at byte src_offset (no alignment needed). A [B,h,w,3]
 *               batch is the same with src_offset = b*h*w*3.
 *   descs       [B] mpn_draw_desc, DEVICE, 16-byte aligned
 *   record      mpn_pose_gather's record for (B, max_boxes), DEVICE, 16-byte aligned: the header's total and counts and
 *               the rows' image_index, box and keypoint_positions are read (clamped to the record's capacity)
 *   with_keypoints  0: boxes only (a record made without keypoint positions)
 *   out_rgba    image b's uint8 [h, w, 4] at byte out_offset, a multiple of 16; written in 16-byte vectors: h*w*4 rounded
 *               up to 16 bytes are written. 16-byte aligned.
 *   workspace   mpn_draw_detections_workspace_bytes(B, max_boxes) bytes (0 for arguments out of range), 16-byte aligned
 * An image whose descriptor reaches outside sources_bytes / out_bytes, or has h, w outside [1, 65536] or h*w > 2^29, is left
 * unwritten: no descriptor makes the kernels read outside sources or write outside out_rgba.
 * Two launches: the primitives of every kept person (one thread each), then a gather - a pixel's colour is the last
 * primitive in draw order that covers it, else the source; nothing scatters, the output is deterministic. Grid and block
 * sizes depend on (B, max_boxes) alone, so a captured graph serves any later batch that fits its buffers.
 * Checked before any HIP call: null pointers (MPN_ERR_BAD_ARG); 1 <= B <= 65535, 1 <= max_boxes <= MPN_DRAW_MAX_BOXES,
 * B*max_boxes <= 4096 (MPN_ERR_BAD_SHAPE); alignment (MPN_ERR_BAD_ALIGN); record_bytes, workspace_bytes, sources_bytes >= 3,
 * out_bytes >= 16 (MPN_ERR_WORKSPACE).
 */
#define MPN_DRAW_MAX_BOXES 128
#define MPN_DRAW_DESC_BYTES 32
#define MPN_DRAW_DOT_STAMPS {{6, 15, 15, 6, 0}, {6, 15, 15, 15, 6}, {14, 31, 31, 14, 0}, {14, 31, 31, 31, 14}}
typedef struct mpn_draw_desc {
    int64_t src_offset;                         /* byte offset into sources */
    int64_t out_offset;                         /* byte offset into out_rgba, multiple of 16 */
    int32_t h, w;
    int32_t reserved[2];
} mpn_draw_desc;
#ifdef __cplusplus
static_assert(sizeof(mpn_draw_desc) == MPN_DRAW_DESC_BYTES, "descriptor size is fixed");
#endif
size_t mpn_draw_desc_bytes(void);
int mpn_draw_dot_stamp(int dw, int dh, int row);
size_t mpn_draw_detections_workspace_bytes(int B, int max_boxes);
int mpn_draw_detections(const uint8_t* sources, size_t sources_bytes, const void* descs, const void* record,
                        size_t record_bytes, int B, int max_boxes, int with_keypoints, uint8_t* out_rgba, size_t out_bytes,
                        void* workspace, size_t workspace_bytes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Annotated frames of TRACKED persons: the picture of mpn_draw_detections with a colour per identity and the id as a label,
 * equal byte for byte to what Pillow draws for it (tests/draw_tracks_ref.py restates it; tests/test_draw_tracks_host.py holds
 * the restatement against Pillow). sources, descs, record, with_keypoints, out_rgba, the geometry of box, lines and dots, the
 * clamping and the draw order (per KEPT person in record order: box, 16 lines, 17 dots, then the label; a pixel takes the
 * LAST primitive that covers it) are those of mpn_draw_detections. What differs, per person (record row r):
 *   colours      track_id = int32 at byte 0 of row r of track_rows (24-byte rows, mpn_pose_track's out for the same record).
 *                track_id <= 0, untracked: red box, white lines, red dots as mpn_draw_detections draws them - or, with the
 *                hide flag, nothing at all. track_id > 0: box and dots in palette[(track_id - 1) % P], lines in line_colour.
 *   keypoints    smooth_rows NULL: the notebook's f64 / f32 arithmetic from box and keypoint_positions, unchanged.
 *                Otherwise (x, y) = the f32 pair at floats 3k, 3k+1 of row r of smooth_rows (340-byte rows, mpn_pose_smooth's
 *                out): lines from (trunc x_a, trunc y_a) to (trunc x_b, trunc y_b), dot corners trunc(x - 2.0f) ..
 *                trunc(x + 2.0f) in f32. (For an untracked person those rows hold the record's own float32 keypoints.)
 *   label        only with the labels flag, for track_id > 0 and a box that is drawn (x1 >= x0 and y1 >= y0); also with
 *                with_keypoints = 0. The text is the decimal digits of track_id, n = 1..10 of them, one per cell. With
 *                pad = 1, lw = 2*pad + n*cell, lh = 2*pad + (bot - top) and the box's integer corner (x0, y0):
 *                    lx0 = x0;  ly0 = y0 - lh if that is >= 0, else y0     (above the box, or inside it at the frame's top)
 *                the FILLED rectangle [lx0, ly0, lx0+lw-1, ly0+lh-1] in the identity colour; digit k (from the left, value d)
 *                has its stamp's top left at (lx0 + pad + k*cell + ox_d, ly0 + pad - top + oy_d), and a pixel under stamp
 *                byte m is, per colour channel, BLEND8(m, identity, text): t = m*text + (255-m)*identity + 128;
 *                ((t >> 8) + t) >> 8; alpha 255. In Pillow's terms: draw.rectangle(fill=identity), then draw.text per digit
 *                at (lx0 + pad + k*cell, ly0 + pad - top) with a font whose getmask2(d, 'L') is (stamp_d, (ox_d, oy_d)),
 *                cell = max ceil(getlength(d)), top = min oy_d, bot = max (oy_d + h_d). Every stamp lies at most the padding
 *                outside its cell (-pad <= ox_d, ox_d + w_d <= cell + pad, top <= oy_d, oy_d + h_d <= bot), hence inside the
 *                rectangle. A glyph wider than its advance reaches into the neighbouring cell: a pixel under the stamps of two
 *                digits is blended twice, the left digit first, as Pillow draws them - BLEND8(m_right, BLEND8(m_left,
 *                identity, text), text). Either way a label pixel is a function of the style and the id alone.
 *   tables       DEVICE, 4-byte aligned, tables_bytes >= MPN_DRAW_TRACKS_TABLE_HEADER_BYTES; int32 words:
 *                    0 flags (bit 0 labels, bit 1 hide untracked)   1 line_colour   2 text_colour   (R | G<<8 | B<<16)
 *                    3 P, the palette's size, 1..MPN_DRAW_TRACKS_MAX_PALETTE   4 cell, 1..MPN_DRAW_TRACKS_MAX_CELL
 *                    5 top   6 bot (0 <= bot - top <= MPN_DRAW_TRACKS_MAX_STAMP_H, |top| <= that too)   7 zero
 *                    8 + 5*d .. 12 + 5*d, d = 0..9: the stamp of digit d: w, h, ox, oy, byte offset of its w*h L8 bytes
 *                                (rows of w) from the start of tables
 *                    58 .. 57 + P: the palette, one colour per word as above
 *                then the stamps' bytes. mpn_draw_tracks_tables_bytes(P, cell, bot - top): the bytes that hold any such
 *                table (header + 4*P + 10*(cell + 2*pad)*(bot-top), rounded up to 16); 0 for arguments out of range.
 *                The style is DATA: a captured graph serves any later table of at most tables_bytes. The kernels check every
 *                index they derive from the table against tables_bytes and the limits above; a palette that does not fit
 *                leaves a tracked person undrawn, a label whose cell, top / bot or digit stamps fail a check is not drawn.
 *   workspace    mpn_draw_tracks_workspace_bytes(B, max_boxes) bytes (0 out of range; more than mpn_draw_detections needs),
 *                16-byte aligned.
 * Two launches with the grids of mpn_draw_detections, no scatter, no atomics on global memory: the output is a function of
 * the inputs. Checked before any HIP call: null track_rows / tables (MPN_ERR_BAD_ARG; smooth_rows may be NULL); everything
 * mpn_draw_detections checks, with the same codes; track_rows / smooth_rows / tables not 4-byte aligned (MPN_ERR_BAD_ALIGN);
 * tables_bytes < MPN_DRAW_TRACKS_TABLE_HEADER_BYTES (MPN_ERR_WORKSPACE).
 */
#define MPN_DRAW_TRACKS_MAX_PALETTE 256
#define MPN_DRAW_TRACKS_MAX_CELL 32
#define MPN_DRAW_TRACKS_MAX_STAMP_H 48
#define MPN_DRAW_TRACKS_TABLE_HEADER_BYTES 232
size_t mpn_draw_tracks_tables_bytes(int palette_size, int cell_w, int stamp_h);
size_t mpn_draw_tracks_workspace_bytes(int B, int max_boxes);
int mpn_draw_tracks(const uint8_t* sources, size_t sources_bytes, const void* descs, const void* record, size_t record_bytes,
                    const void* track_rows, const void* smooth_rows, const void* tables, size_t tables_bytes, int B,
                    int max_boxes, int with_keypoints, uint8_t* out_rgba, size_t out_bytes, void* workspace,
                    size_t workspace_bytes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Persons made unrecognisable: per KEPT person of mpn_pose_gather[_sized]'s record a region of its frame - the head, from the
 * five face joints, or the box - is pixelated, blurred or filled. out_rgb = the packed RGB sources with those regions
 * replaced; a pixel no region covers is a copy of the source. The definition is this project's own (NOT Pillow's reduce or
 * GaussianBlur, which round differently); tests/anonymize_ref.py restates it as plain loops.
 *
 * All floating-point work is IEEE float64 on values widened from the record's float32, in the order written, no contraction;
 * h, w are the descriptor's.
 *   box      (by0, bx0, by1, bx1) = (box[0]*h, box[1]*w, box[2]*h, box[3]*w)
 *   bounds   region 1 (box):  (fx0, fy0, fx1, fy1) = (bx0, by0, bx1, by1)
 *            region 0 (head): F = the joints j in 0..4 (nose, eyes, ears) with with_keypoints != 0 and the row's
 *                             keypoints[j][2] >= min_keypoint_score (float32 compare; a NaN score is not in F).
 *                 F not empty: cx, cy = the sum of the x (y) of F in joint order, from 0.0, divided by |F|;
 *                              e = 0.0, then per joint of F in order: d = |x_j - cx|, if d > e: e = d; the same with |y_j - cy|;
 *                              s = e*scale; t = (by1 - by0)*min_size; if t > s: s = t;
 *                              bounds cx - s, cy - s, cx + s, cy + s
 *                 F empty:     bx0, by0, bx1, by0 + (by1 - by0)*fallback
 *            A person with a non-finite bound has no region.
 *   region   every bound clamped to +-2^20; x0 = floor(fx0), y0 = floor(fy0), x1 = ceil(fx1), y1 = ceil(fy1);
 *            [x0, x1) x [y0, y1) half-open; a = x1 - x0, b = y1 - y0; a <= 0 or b <= 0: no region.
 *   covered  frame pixel (x, y) lies in the rectangle and, for shape 0 (ellipse) with a, b <= 32768,
 *            u*u*b*b + v*v*a*a <= a*a*b*b in int64, u = 2x + 1 - (x0 + x1), v = 2y + 1 - (y0 + y1) (62 bits). A larger
 *            region is a rectangle.
 *   colour   of a covered pixel: that of the LAST person of its image, in record order, that covers it; that person reads the
 *            ORIGINAL sources, never another region's output.
 *              mode 2 (fill)      color
 *              mode 0 (pixelate)  c = ceil(max(a, b) / blocks); cell (i, j) = ((x - x0) / c, (y - y0) / c); per channel
 *                                 (2*S + n) / (2*n) (integer division), S and n the sum and the count of the source pixels of
 *                                 [x0 + i*c, x0 + (i+1)*c) x [y0 + j*c, y0 + (j+1)*c) inside the frame (clipped to the
 *                                 frame, not to the region or the ellipse; n >= 1)
 *              mode 1 (blur)      the frame after three passes, each a horizontal box mean then a vertical one of radius
 *                                 `radius`, n = 2*radius + 1 samples, sample indices clamped to the frame (every pass
 *                                 replicates its own edge), each 1-D mean (2*S + n) / (2*n) per channel, stored as uint8
 *                                 before the next
 *
 *   sources, descs   as for mpn_draw_detections: src_offset (no alignment needed), h, w are read; out_offset is not
 *   record      as for mpn_draw_detections (with mpn_pose_nms: the filtered one): the header's total and counts and the
 *               rows' image_index, box and keypoints are read; a row whose image_index is not the image the header's counts
 *               give it has no region
 *   params      HOST, read at call time
 *   out_rgb     out_bytes; image b's uint8 [h, w, 3] at byte src_offset, as in sources: every byte of every valid frame is
 *               written. mpn_draw_detections / mpn_draw_tracks take it as their `sources` with the same descriptors.
 *   workspace   mpn_anonymize_workspace_bytes(B, max_boxes) bytes (0 for arguments out of range), 16-byte aligned
 * An image whose descriptor reaches outside sources_bytes / out_bytes, or has h, w outside what mpn_draw_detections accepts,
 * is left unwritten: no descriptor makes a kernel read outside sources or write outside out_rgb.
 * Launches: the regions (a thread per row), a streaming copy of the frames, for pixelate the cell means (a wave per region
 * and cell), then a block per (row, tile of its region), which writes a covered pixel only where no later row of the image
 * covers it: one writer per pixel behind the copy, no scatter, no atomics on global memory - the output is a function of
 * (sources, descs, record, params), and launching twice gives the same bytes. Mosaic means and blur are computed only where a
 * region lies. Grid and block sizes depend on (B, max_boxes, params) alone.
 * Checked before any HIP call: null pointers (MPN_ERR_BAD_ARG); 1 <= B <= 65535, 1 <= max_boxes <= MPN_DRAW_MAX_BOXES,
 * B*max_boxes <= 4096 (MPN_ERR_BAD_SHAPE); descs, record, workspace 16-byte aligned (MPN_ERR_BAD_ALIGN); record_bytes,
 * workspace_bytes, sources_bytes >= 3, out_bytes >= 3 (MPN_ERR_WORKSPACE); every parameter's range (MPN_ERR_BAD_ARG).
 */
#define MPN_ANONYMIZE_MAX_BLOCKS 32
#define MPN_ANONYMIZE_MAX_RADIUS 12
typedef struct mpn_anonymize_params {
    int32_t region;                             /* 0 head, 1 box */
    int32_t mode;                               /* 0 pixelate, 1 blur, 2 fill */
    int32_t shape;                              /* 0 ellipse, 1 rectangle */
    int32_t blocks;                             /* 2..MPN_ANONYMIZE_MAX_BLOCKS */
    int32_t radius;                             /* 1..MPN_ANONYMIZE_MAX_RADIUS */
    int32_t color;                              /* R | G << 8 | B << 16 */
    float min_keypoint_score;                   /* finite */
    int32_t reserved;
    double scale;                               /* finite, > 0 */
    double min_size;                            /* finite, >= 0 */
    double fallback;                            /* in (0, 1] */
} mpn_anonymize_params;
size_t mpn_anonymize_params_bytes(void);
size_t mpn_anonymize_workspace_bytes(int B, int max_boxes);
int mpn_anonymize(const uint8_t* sources, size_t sources_bytes, const void* descs, const void* record, size_t record_bytes,
                  int B, int max_boxes, int with_keypoints, const mpn_anonymize_params* params, uint8_t* out_rgb,
                  size_t out_bytes, void* workspace, size_t workspace_bytes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Person crops: per row of mpn_pose_gather[_sized]'s record the picture of that person, cut from its frame and resized to
 * H x W, equal byte for byte to Pillow's `Image.resize((new_w, new_h), Image.BICUBIC, box=(x0, y0, x1, y1))` of the WHOLE
 * frame (so the taps at the rectangle's edge read the frame's pixels beside it, not a border). The boxes exist only on the
 * device: the tap tables of every crop are built there. tests/crops_ref.py restates everything below as plain loops;
 * tests/test_person_crops_host.py holds that restatement against Pillow.
 *
 * All floating-point work is IEEE float64 on values widened from the record's float32, one operation at a time in the order
 * written, no contraction (the file is compiled with contraction off); it relies on the device's float64 division being
 * correctly rounded, as the tracker's and the smoother's sections do. h, w are the descriptor's.
 *   rectangle  (ymin, xmin, ymax, xmax) = (h*box[0], w*box[1], h*box[2], w*box[3]), as mpn_draw_detections;
 *              bw = xmax - xmin; bh = ymax - ymin; px = pad*bw; py = pad*bh;
 *              x0 = xmin - px; x1 = xmax + px; y0 = ymin - py; y1 = ymax + py.
 *              One of the four not finite: EMPTY, rect = (0, 0, 0, 0), not clipped. Else the clamps, each setting CLIPPED
 *              when it moves a bound: if x0 < 0: x0 = 0;  if x1 > w: x1 = w;  if y0 < 0: y0 = 0;  if y1 > h: y1 = h.
 *              rw = x1 - x0; rh = y1 - y0; not (rw > 0) or not (rh > 0): EMPTY (rect is still reported).
 *   placement  fit 0 (stretch): (top, left, new_h, new_w) = (0, 0, H, W).
 *              fit 1 (pad): s = min(H / rh, W / rw); new_h = (int)min(H, max(1, rint(rh*s))), new_w likewise with rw and W
 *              (rint: half to even, what Python's `round` does in resample.resized_size); top = (H - new_h) / 2,
 *              left = (W - new_w) / 2 (integer division). Every pixel outside the placed part is `fill`.
 *   taps       per axis, (in0, in1, in_size, out) = (x0, x1, w, new_w) and (y0, y1, h, new_h): scale = (in1 - in0) / out;
 *              filterscale = max(scale, 1); support = 2*filterscale; ss = 1 / filterscale;
 *              ksize = (int)ceil(support)*2 + 1. ksize > MPN_IMAGE_RESIZE_MAX_KSIZE on either axis (a reduction beyond
 *              16x): TOO_LARGE. For output xx: center = in0 + (xx + 0.5)*scale;
 *              first = max((int)(center - support + 0.5), 0); last = min((int)(center + support + 0.5), in_size)
 *              (truncation toward zero); weight k = bicubic((k + first - center + 0.5)*ss), k = 0 .. last - first - 1, with
 *              bicubic(x), a = -0.5, on |x|: < 1: ((a + 2)*x - (a + 3))*x*x + 1;  < 2: (((x - 5)*x + 8)*x - 4)*a;  else 0.
 *              The weights are summed in tap order from 0.0; a sum that is not 0 divides each; the coefficient is
 *              (int)(w*2^22 + 0.5), for w < 0 (int)(w*2^22 - 0.5): 22 fractional bits, rounded half away from zero.
 *              (Pillow multiplies by ss where one might divide by filterscale; this follows Pillow.)
 *   passes     the integer arithmetic of mpn_image_resize: clip8((sum_k pixel[first + k]*coeff[k] + 2^21) >> 22) in int32, the
 *              horizontal pass first, rounded to uint8, then the vertical pass. Both always run: at scale 1 and an integer
 *              offset the taps are the identity, which is what Pillow's skipping the pass leaves.
 *   slots      slot s is row s of the record, s < total (the header's, clamped to B*max_boxes): the order of the result
 *              dicts' 'boxes'. An EMPTY or TOO_LARGE crop is all `fill`. A row whose image_index is not the image the
 *              header's counts give it, or whose frame's descriptor is refused (below), is EMPTY with a zero rect. Slots at
 *              and behind total are written as zeros, crops and info rows: both buffers are a function of the inputs.
 *
 *   sources, descs   as for mpn_draw_detections / mpn_anonymize: [B] mpn_draw_desc, DEVICE, 16-byte aligned; src_offset, h, w
 *               are read. A pixel is read as one unaligned dword except the last of its frame (as mpn_image_resize reads):
 *               nothing outside a frame's own bytes is touched. A frame that reaches outside sources_bytes, or has h, w
 *               outside [1, 65536] or h*w > 2^29, is refused on the device.
 *   record      as for mpn_draw_detections (with mpn_pose_nms: the filtered one): header and the rows' image_index and box
 *   H, W        the crop: multiples of 8, 8 <= H <= MPN_PERSON_CROPS_MAX_H, 8 <= W <= MPN_PERSON_CROPS_MAX_W
 *   pad         finite, 0 <= pad <= 4;  fit 0 or 1;  fill = R | G << 8 | B << 16
 *   crops_out   uint8 [B*max_boxes, H, W, 3], 16-byte aligned; every byte is written
 *   info_out    [B*max_boxes] mpn_person_crops_info, 16-byte aligned (mpn_person_crops_info_bytes(B, max_boxes))
 *   workspace   mpn_person_crops_workspace_bytes(B, max_boxes, H, W) bytes (0 for arguments out of range), 16-byte aligned:
 *               per slot and output coordinate (W columns, then H rows) a tap row of MPN_PERSON_CROPS_TAP_WORDS int32:
 *               first, count, 0, then the coefficients.
 * Two launches. (1) one thread per (slot, axis, output coordinate) writes its tap row - the weight sum sequential in tap
 * order - and thread 0 of the slot the info row. (2) one block per (slot, tile of output rows): the horizontal pass over
 * exactly the source rows the tile's vertical taps need, into LDS as uint8 (new_w*3 bytes a row), then the vertical pass
 * from LDS into crops_out; no intermediate goes to global memory. The tile height depends on (H, W) alone - the largest
 * whose tile*16 + 64 rows of W*3 bytes fit MPN_PERSON_CROPS_LDS_BYTES - and how many of those rows a slot uses is a
 * device value. Grid and block sizes depend on (B, max_boxes, H, W) alone; rectangles, tap counts and offsets travel through
 * device memory, so a captured graph serves every later record. The tap loops are bounded by the tap rows (count <=
 * MPN_IMAGE_RESIZE_MAX_KSIZE, first + count <= the frame) and every LDS row index is checked against the rows the block
 * holds: no descriptor or record makes a kernel write outside crops_out, info_out or the workspace, or read outside sources.
 * Checked before any HIP call, the messages begin "person_crops:": null pointers (MPN_ERR_BAD_ARG); 1 <= B <= 65535,
 * 1 <= max_boxes <= MPN_DRAW_MAX_BOXES, B*max_boxes <= 4096, H and W (MPN_ERR_BAD_SHAPE); pad, fit, fill
 * (MPN_ERR_BAD_ARG); descs, record, crops_out, info_out, workspace 16-byte aligned (MPN_ERR_BAD_ALIGN); record_bytes,
 * workspace_bytes, sources_bytes >= 3 (MPN_ERR_WORKSPACE).
 */
#define MPN_PERSON_CROPS_MAX_H 512
#define MPN_PERSON_CROPS_MAX_W 256
#define MPN_PERSON_CROPS_TAP_WORDS 68
#define MPN_PERSON_CROPS_LDS_BYTES 163840
#define MPN_PERSON_CROPS_EMPTY 1
#define MPN_PERSON_CROPS_TOO_LARGE 2
#define MPN_PERSON_CROPS_CLIPPED 4
#define MPN_PERSON_CROPS_USED 8
typedef struct mpn_person_crops_info {
    double rect[4];                             /* x0, y0, x1, y1 in the pixels of the frame */
    int32_t placed[4];                          /* top, left, new_h, new_w inside the crop (zeros for an EMPTY crop) */
    int32_t flags;                              /* MPN_PERSON_CROPS_*; 0: a slot at or behind the record's total */
    int32_t image;                              /* the row's image, -1 where a used row has none */
    int32_t ksize_x, ksize_y;                   /* tap row lengths (clamped to 2^20), 0 for an EMPTY crop */
} mpn_person_crops_info;
size_t mpn_person_crops_desc_bytes(void);
size_t mpn_person_crops_info_bytes(int B, int max_boxes);
size_t mpn_person_crops_workspace_bytes(int B, int max_boxes, int H, int W);
int mpn_person_crops(const uint8_t* sources, size_t sources_bytes, const void* descs, const void* record, size_t record_bytes,
                     int B, int max_boxes, int H, int W, double pad, int fit, int fill, uint8_t* crops_out, void* info_out,
                     void* workspace, size_t workspace_bytes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Heatmap and mask overlays: `plot_maps` of the reference's inference/predict.ipynb (the cells under "Show heatmaps") for
 * a batch of B frames of one size, equal byte for byte to what Pillow and matplotlib make there. With h = H / 2, w = W / 2
 * (integer division), panel j of frame b is rows j*h .. j*h + h - 1 of out_rgba[b]: the frame resized to (w, h) with
 * Pillow's Lanczos filter, alpha 255; over it panel j's overlay by `Image.alpha_composite`; then label j blended in red.
 *   overlay j < 17   heatmap channel j -> [minmax_keys != NULL: (x - m) / (M - m) per frame and channel, f32, correctly
 *                    rounded; M == m gives NaN] -> the colormap entry (matplotlib's rule for f32: NaN transparent (0,0,0,0),
 *                    x < 0 entry 0, x*256 >= 256 entry 255, else entry trunc(x*256)) -> Pillow's RGBA resize to (w, h):
 *                    premultiplied by alpha (MULDIV255; the table arrives premultiplied), horizontal then vertical Lanczos
 *                    pass through a uint8 intermediate, un-premultiplied (alpha 0 or 255: the pixel as it is, else
 *                    clip8(255 * c / alpha) in integers)
 *   overlay 17       trunc(255 * clip(mask, 0, 1)) as ONE band through the same two passes, that band as R, G, B and alpha
 *                    (mask == NULL: a transparent overlay). Inputs are finite.
 *   label j          stamp j of the tables (L8 pixels [sh, sw]) at (ox, j*h + oy): Pillow's BLEND8 of (255, 0, 0, 255) over
 *                    all four bands, weight = the stamp's pixel, clipped to the panel
 * Every pass is clip8((sum_k pixel[first + k] * coeff[k] + 2^21) >> 22) in int32 on the HOST's coefficient tables
 * (multiposenet_amd/inference/resample.py, filter 'lanczos'), as mpn_image_resize.
 *
 *   frames       [B,H,W,3] uint8            heatmaps  [B,hh,hw,17] f32            mask  [B,hh,hw] f32 or NULL
 *   minmax_keys  mpn_heatmap_minmax's keys of `heatmaps` (B*17*2 words), or NULL: the heatmaps as given
 *   tables       int32 words, DEVICE, 16-byte aligned: per axis bounds [out,2] = (first tap, tap count) and coeffs
 *                [out,ksize]; the colour table, 256 words (R in the low byte), premultiplied; 18 stamp descriptors of 8
 *                words (byte offset into the packed pixels, sw, sh, ox, oy, 3 reserved); the stamps' packed L8 pixels
 *   desc         ONE mpn_plot_maps_desc in HOST memory: where each part lies in tables (word offsets). Checked against
 *                table_words before any launch (MPN_ERR_BAD_ARG). What the tables HOLD is read on the device: a tap window is
 *                clamped to its source and a stamp that leaves stamp_bytes is not blended - no content of tables makes a
 *                kernel touch memory outside its buffers.
 *   out_rgba     [B, 18*h, w, 4] uint8, 16-byte aligned. EVERY byte is written.
 *   workspace    mpn_plot_maps_workspace_bytes(B, H, W, hh, hw) bytes (0 for arguments out of range), 16-byte aligned: the
 *                horizontally resampled rows [B,H,w4,4] of the frames and [B,hh,18,w4,4] of the overlays, w4 = w rounded up
 *                to 4
 * Three launches; grid and block sizes depend on (B, H, W, hh, hw) alone, so the call can be captured.
 * Checked before any HIP call: null pointers (MPN_ERR_BAD_ARG); 1 <= B <= 65535, 2 <= H <= 65535, 2 <= W <= 65536,
 * 1 <= hh <= 3640, 1 <= hw <= 65536 (MPN_ERR_BAD_SHAPE); alignment (MPN_ERR_BAD_ALIGN); workspace_bytes (MPN_ERR_WORKSPACE).
 */
#define MPN_PLOT_MAPS_PANELS 18
#define MPN_PLOT_MAPS_DESC_BYTES 64
typedef struct mpn_plot_maps_desc {
    int32_t bounds_fx, coeffs_fx, ksize_fx;     /* frame, horizontal: W -> w */
    int32_t bounds_fy, coeffs_fy, ksize_fy;     /* frame, vertical:   H -> h */
    int32_t bounds_mx, coeffs_mx, ksize_mx;     /* maps, horizontal:  hw -> w */
    int32_t bounds_my, coeffs_my, ksize_my;     /* maps, vertical:    hh -> h */
    int32_t lut;                                /* the premultiplied colour table, 256 words */
    int32_t stamps;                             /* 18 stamp descriptors of 8 words, a multiple of 4 */
    int32_t stamp_pixels;                       /* the stamps' packed L8 pixels */
    int32_t stamp_bytes;                        /* ... and how many bytes they are */
} mpn_plot_maps_desc;
#ifdef __cplusplus
static_assert(sizeof(mpn_plot_maps_desc) == MPN_PLOT_MAPS_DESC_BYTES, "descriptor size is fixed");
#endif
size_t mpn_plot_maps_desc_bytes(void);
size_t mpn_plot_maps_workspace_bytes(int B, int H, int W, int hh, int hw);
int mpn_plot_maps(const uint8_t* frames, const float* heatmaps, const float* mask, const void* minmax_keys,
                  const int32_t* tables, size_t table_words, const void* desc, int B, int H, int W, int hh, int hw,
                  uint8_t* out_rgba, void* workspace, size_t workspace_bytes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * JPEG decode, split in two: the serial part on the HOST, the parallel part on the device. The result equals what
 * libjpeg(-turbo) - and so Pillow's `Image.open(...).convert("RGB")` - returns for the same bytes, byte for byte.
 *
 * Supported (mpn_jpeg_info sets supported = 1): SOF0 / SOF1, 8-bit, Huffman coded, ONE interleaved scan; one component
 * (grayscale, R = G = B) or three components in YCbCr (JFIF, or what libjpeg guesses as YCbCr) with luma sampling 1x1, 2x1
 * or 2x2 and chroma 1x1; restart intervals; custom Huffman tables; any size from 1x1 to 65535 per side and 2^28 pixels.
 * Everything else is CLASSIFIED (supported = 0 and a reason) and left to a library: progressive, arithmetic, lossless /
 * hierarchical frames, 12-bit precision, 2 or 4 components (CMYK / YCCK), an Adobe marker with a transform other than 1
 * or 'R','G','B' component ids, other sampling (4:4:0, 4:1:1, ...), several scans, 16-bit quantisation tables.
 * (Progressive files and Adobe CMYK are read by the same host front end under its all-scans policy, mpn_jpeg_scans_decode
 * below; these three calls - its one-scan policy - still classify them as unsupported.)
 *
 * HOST (no HIP call, no global state: thread-safe and re-entrant; nothing is read past nbytes or written past coef_bytes):
 *   mpn_jpeg_info            scans the markers up to the first scan. MPN_OK for every stream it can classify (supported or
 *                            not); MPN_ERR_BAD_DATA (reason MPN_JPEG_MALFORMED) when the headers are damaged.
 *   mpn_jpeg_entropy_decode  Huffman-decodes the scan of a SUPPORTED stream into `coefs` (host): every 8x8 block of every
 *                            component as 64 RAW (not dequantised) int16 coefficients in natural (row-major) order, one
 *                            plane per component behind each other, blocks in raster order over the component's PADDED
 *                            block grid blocks_h x blocks_w (whole MCUs). Fills `desc` (host) except its three offsets.
 *                            MPN_ERR_WORKSPACE when coef_bytes < total_blocks * 128; MPN_ERR_BAD_DATA for an unsupported
 *                            stream, a truncated or damaged scan, a missing restart marker.
 *
 * DEVICE: mpn_jpeg_decode decodes one ragged batch per call, two launches:
 *   1. dequantise + inverse DCT, libjpeg's default "slow integer" method (jidctint.c: 13-bit constants, 2 extra bits kept
 *      after pass 1, columns first, then rows, descale (x + 2^(n-1)) >> n; +128 and the range limit through the low 10
 *      bits, as the library's table is indexed) -> uint8 component planes [blocks_h*8, blocks_w*8] in `work`;
 *   2. "fancy" chroma upsampling (jdsample.c: the triangle filter of h2v1 / h2v2 with its alternating rounding constants;
 *      edges at the component's true down-sampled size ceil(width / h_samp) x ceil(height / v_samp); a chroma component at
 *      most 2 samples wide is replicated instead, as the library does) and YCbCr -> RGB (jdcolor.c: 16-bit fixed point)
 *      -> packed uint8 [height, width, 3] at byte src_offset of sources_out. Only the image's bytes are written.
 *
 *   coefs        the coefficients of the batch, DEVICE, 16-byte aligned; image b's planes start at byte coef_offset
 *   descs        [B] mpn_jpeg_desc, DEVICE, 16-byte aligned
 *   sources_out  uint8, DEVICE, 16-byte aligned: the packed ragged source buffer mpn_keypoint_augment, mpn_detector_augment
 *                and mpn_image_resize read
 *   work         mpn_jpeg_decode_workspace_bytes(B, sum of total_blocks) bytes (64 per block; 0 for arguments out of range),
 *                16-byte aligned; image b's planes at byte work_offset
 * src_offset, coef_offset and work_offset are multiples of 16. The kernels recompute an image's geometry from (width,
 * height, components, h_samp, v_samp; components == 4: see "multi-scan and four-component files" below) and skip an image whose descriptor is out of range, misaligned, or reaches outside
 * coef_bytes / work_bytes / sources_bytes: no descriptor makes them read or write outside the four buffers.
 * Grid and block sizes depend on B alone. Checked before any HIP call: null pointers (MPN_ERR_BAD_ARG); 1 <= B <= 65535
 * (MPN_ERR_BAD_SHAPE); alignment (MPN_ERR_BAD_ALIGN); coef_bytes >= 128, work_bytes >= 64, sources_bytes >= 3
 * (MPN_ERR_WORKSPACE).
 */
enum {
    MPN_JPEG_SUPPORTED = 0,
    MPN_JPEG_MALFORMED = 1,     /* not a JPEG, or damaged / truncated headers */
    MPN_JPEG_PROGRESSIVE = 2,
    MPN_JPEG_ARITHMETIC = 3,
    MPN_JPEG_FRAME_TYPE = 4,    /* lossless or hierarchical */
    MPN_JPEG_PRECISION = 5,     /* not 8 bits */
    MPN_JPEG_COMPONENTS = 6,    /* neither 1 nor 3: CMYK / YCCK */
    MPN_JPEG_COLORSPACE = 7,    /* three components that libjpeg does not read as YCbCr */
    MPN_JPEG_SAMPLING = 8,
    MPN_JPEG_MULTISCAN = 9,
    MPN_JPEG_DQT16 = 10,
    MPN_JPEG_TOO_LARGE = 11     /* more than 2^28 pixels */
};
typedef struct mpn_jpeg_header {               /* what mpn_jpeg_info reports (host) */
    int32_t width, height, components;
    int32_t h_samp, v_samp;                     /* sampling of the first component (1, 1 for grayscale) */
    int32_t restart_interval;                   /* in MCUs; 0 = none */
    int32_t supported, reason;                  /* reason: MPN_JPEG_* */
    int32_t blocks_w[3], blocks_h[3];           /* padded block grid of each component (supported streams only) */
    int32_t total_blocks, reserved;             /* sum of blocks_w * blocks_h */
    int64_t coef_bytes;                         /* total_blocks * 128 */
} mpn_jpeg_header;
#define MPN_JPEG_DESC_BYTES 512
typedef struct mpn_jpeg_desc {
    int64_t src_offset;                         /* CALLER: byte offset of the image in sources_out, multiple of 16 */
    int64_t coef_offset;                        /* CALLER: byte offset of its coefficients in coefs, multiple of 16 */
    int64_t work_offset;                        /* CALLER: byte offset of its planes in work, multiple of 16 */
    int32_t width, height, components, h_samp, v_samp;
    int32_t total_blocks;
    int32_t blocks_w[3], blocks_h[3];
    int32_t blocks_w3, blocks_h3;               /* components == 4: the fourth component's grid (else 0) */
    int32_t quant3;                             /* components == 4: which of quant[0..2] the fourth component uses */
    int32_t reserved[11];
    uint16_t quant[3][64];                      /* per component, natural order (the 8-bit tables widened) */
} mpn_jpeg_desc;
#ifdef __cplusplus
static_assert(sizeof(mpn_jpeg_desc) == MPN_JPEG_DESC_BYTES, "descriptor size is fixed");
#endif
size_t mpn_jpeg_desc_bytes(void);
int mpn_jpeg_info(const uint8_t* data /* host */, size_t nbytes, mpn_jpeg_header* out /* host */);
int mpn_jpeg_entropy_decode(const uint8_t* data /* host */, size_t nbytes, int16_t* coefs /* host */, size_t coef_bytes,
                            mpn_jpeg_desc* desc /* host */);
size_t mpn_jpeg_decode_workspace_bytes(int B, long long total_blocks);
int mpn_jpeg_decode(const int16_t* coefs, size_t coef_bytes, const void* descs, int B, uint8_t* sources_out,
                    size_t sources_bytes, void* work, size_t work_bytes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * JPEG decode of multi-scan and four-component files: the all-scans policy of the HOST front end (one marker parser and one
 * scan decoder serve it and mpn_jpeg_entropy_decode alike), and a fourth plane in mpn_jpeg_decode. mpn_jpeg_info /
 * mpn_jpeg_entropy_decode / mpn_jpeg_scan_prepare keep the one-scan policy: they classify these files as
 * MPN_JPEG_PROGRESSIVE / MPN_JPEG_COMPONENTS, stop at the first verdict and never read behind the first scan, so on damaged
 * input the two policies may answer differently ("JPEG host front end").
 *
 * What it adds: 8-bit Huffman PROGRESSIVE files (SOF2) of one component, of three in YCbCr (the samplings above) or of four;
 * and BASELINE files of four. Four components means: every component sampled 1x1 and an Adobe APP14 marker with transform 0
 * (CMYK stored inverted: what Pillow writes for a "CMYK" image), the fourth component's quantisation table equal to one of
 * the first three's. YCCK (transform 2), four components without the Adobe marker, sampled CMYK, 4:4:0, arithmetic coding,
 * 12-bit precision, 16-bit quantisation tables and sequential files of several scans stay with a library (route LIBRARY).
 *
 * HOST (no HIP call, no global state, no allocation: thread-safe and re-entrant; nothing is read past nbytes or written
 * past coef_bytes, whatever the bytes are):
 *   mpn_jpeg_scans_info    the marker scan up to the first scan: geometry of up to four components, `route` - DEVICE (a
 *                          stream mpn_jpeg_info supports: its Huffman stage may run on the device), HOST_ENTROPY (a stream
 *                          only mpn_jpeg_scans_decode reads) or LIBRARY - and `reason` (MPN_JPEG_*; SUPPORTED unless the
 *                          route is LIBRARY). MPN_ERR_BAD_DATA when the headers are damaged.
 *   mpn_jpeg_scans_decode  decodes EVERY scan of a DEVICE or HOST_ENTROPY stream into the layout of
 *                          mpn_jpeg_entropy_decode: DC first / DC refinement scans (interleaved or one component), AC first
 *                          scans with end-of-band runs, AC refinement scans with their correction bits, any spectral band,
 *                          DHT / DQT / DRI redefined between scans (a component's quantisation table is the one in force
 *                          at its first scan), restart intervals; a scan of ONE component walks that component's own
 *                          ceil(w / 8) x ceil(h / 8) blocks, not the padded grid. Fills `desc` except its three offsets.
 *                          MPN_ERR_WORKSPACE when coef_bytes < total_blocks * 128; MPN_ERR_BAD_DATA for a LIBRARY stream, a
 *                          truncated file, an invalid code, a band past 63, a bit position above 13, a scan that does not
 *                          continue what the scans before it left (a refinement of a band never started, a band coded
 *                          twice), a file that ends before every coefficient has all its bits, more than 100 scans.
 *
 * DEVICE: a descriptor with components == 4 (h_samp = v_samp = 1; blocks_w3, blocks_h3, quant3 set) makes mpn_jpeg_decode
 * run the same inverse DCT over four planes and, in place of YCbCr -> RGB, what Pillow does with such a file: the four
 * samples s0..s3 pass through the library unchanged, Pillow inverts them on load (C = 255 - s0, ..., K = 255 - s3) and
 * `convert("RGB")` computes R = nk - MULDIV255(C, nk) with nk = 255 - K, MULDIV255(a, b) = (t + (t >> 8)) >> 8 for
 * t = a * b + 128 (likewise G from M, B from Y). Three bytes per pixel at src_offset, as for the other streams.
 */
enum { MPN_JPEG_ROUTE_DEVICE = 0, MPN_JPEG_ROUTE_HOST_ENTROPY = 1, MPN_JPEG_ROUTE_LIBRARY = 2 };
typedef struct mpn_jpeg_scans_header {          /* what mpn_jpeg_scans_info reports (host) */
    int32_t width, height, components;
    int32_t h_samp, v_samp;                     /* sampling of the first component (1, 1 for grayscale) */
    int32_t progressive;                        /* 1: SOF2 */
    int32_t route, reason;                      /* MPN_JPEG_ROUTE_*, MPN_JPEG_* */
    int32_t blocks_w[4], blocks_h[4];           /* padded block grid of each component (route DEVICE / HOST_ENTROPY only) */
    int32_t total_blocks, reserved;
    int64_t coef_bytes;                         /* total_blocks * 128 */
} mpn_jpeg_scans_header;
int mpn_jpeg_scans_info(const uint8_t* data /* host */, size_t nbytes, mpn_jpeg_scans_header* out /* host */);
int mpn_jpeg_scans_decode(const uint8_t* data /* host */, size_t nbytes, int16_t* coefs /* host */, size_t coef_bytes,
                          mpn_jpeg_desc* desc /* host */);

/* ------------------------------------------------------------------------------------
 * JPEG entropy decode on the device: the Huffman stage of a SUPPORTED stream (above) without the host decode. The host only
 * parses headers (mpn_jpeg_scan_prepare); the file's own bytes are staged, and mpn_jpeg_entropy_decode_device produces the
 * coefficients in the layout of mpn_jpeg_entropy_decode and the [B] mpn_jpeg_desc mpn_jpeg_decode reads.
 *
 * The scheme: an image's bytes are cut into subsequences of MPN_JPEG_SUBSEQ_BITS bits, the grid anchored at the image's
 * first byte (file_offset), NOT at the scan. A decoder state is (bit position over the RAW bytes, block index within the
 * MCU, zigzag index). f_i(entry) decodes whole symbols from `entry` until the position leaves subsequence i and returns the
 * exit state, the blocks completed and the restart markers passed. It works on raw bytes: the 00 behind an FF is skipped,
 * FF D0..D7 (behind any FF fill bytes) aligns to the byte behind the marker and resets the state to block 0, index 0, any
 * other marker or the end of the data ends the scan; nothing at or past nbytes is read. The first entry is known
 * (scan_offset * 8, 0, 0), every other starts as a guess (its subsequence's first bit, 0, 0); the true entries are the fixed
 * point of entry[i + 1] = f_i(entry[i]). A workgroup owns MPN_JPEG_GROUP_SUBSEQ consecutive subsequences (32 KB) and sweeps
 * them in LDS until nothing changes (at most that many sweeps); `max_passes` launches carry each group's exit into the next
 * group, a pass re-solving only what its changed entry changes. Then: an exclusive prefix sum of the block counts, a write
 * pass from the true entries (raw coefficients, de-zigzagged, DC as the difference, into the zeroed region), and a DC pass
 * (per-component running sum in decode order, reset every restart_interval MCUs). 5 + max_passes launches (the first gives every
 * image its own part of the workspace: a prefix sum over the descriptors); no workgroup waits on another; every loop is
 * bounded by nbytes, B or the group size; grids depend on B alone; no host synchronisation, no
 * allocation: capturable.
 *
 *   files        the staged bytes of the batch, DEVICE, 16-byte aligned; image b's file at byte file_offset (multiple of 16)
 *   scan_descs   [B] mpn_jpeg_scan_desc, DEVICE, 16-byte aligned (mpn_jpeg_scan_prepare + the caller's four offsets)
 *   coefs        as mpn_jpeg_decode reads them; image b's planes at byte coef_offset (zeroed by the call, then written)
 *   jpeg_descs_out [B] mpn_jpeg_desc, DEVICE, 16-byte aligned (a skipped image's is zeroed: mpn_jpeg_decode skips it too)
 *   records      [B] mpn_jpeg_entropy_record, DEVICE, 16-byte aligned:
 *     MPN_JPEG_ENT_OK             the coefficients equal mpn_jpeg_entropy_decode's
 *     MPN_JPEG_ENT_NOT_CONVERGED  max_passes did not reach the fixed point (a stream longer than max_passes groups that
 *                                 does not self-synchronise); the coefficients are not valid
 *     MPN_JPEG_ENT_BAD_DATA       judged from true entries only: an invalid code, a run past 63, a DC category above 11, a
 *                                 scan that ends without a marker or before the image does, a block or restart count that
 *                                 disagrees at a restart marker or at the end, a restart marker in a stream without an
 *                                 interval, a Huffman table that is not a prefix code. (Stricter than the host call in one
 *                                 place: the scan must END IN A MARKER; a file cut inside its EOI is BAD_DATA here.)
 *     MPN_JPEG_ENT_SKIPPED        the descriptor is out of range, misaligned, or reaches outside files_bytes / coef_bytes /
 *                                 work_bytes: nothing of the image is read or written
 *     passes = passes that changed anything (<= max_passes), blocks = blocks the fixed point holds.
 *   work         mpn_jpeg_entropy_decode_device_workspace_bytes(B, files_bytes) bytes (0 for arguments out of range),
 *                16-byte aligned; nothing in it needs initialising. The call divides it among the images in descriptor
 *                order by their nbytes: the files may lie in `files` in any order. The size covers every batch whose files
 *                do not overlap; descriptors that name the same bytes several times may exhaust it, and the images
 *                that no longer fit are SKIPPED - no two images ever share a part of it
 * Checked before any HIP call: null pointers (MPN_ERR_BAD_ARG); 1 <= B <= 65535, 1 <= max_passes <= MPN_JPEG_MAX_PASSES
 * (MPN_ERR_BAD_SHAPE); alignment (MPN_ERR_BAD_ALIGN); files_bytes in [16, 2^31), coef_bytes >= 128, work_bytes >= the
 * workspace size (MPN_ERR_WORKSPACE).
 *
 * mpn_jpeg_scan_prepare (HOST, no HIP call, thread-safe): the marker scan of mpn_jpeg_info into a fixed-size descriptor. It
 * never touches the scan's bytes. MPN_OK for every stream it can classify: `supported` / `reason` as mpn_jpeg_info reports
 * them, the other fields filled for a supported stream only; MPN_ERR_BAD_DATA for damaged headers.
 */
enum { MPN_JPEG_ENT_OK = 0, MPN_JPEG_ENT_NOT_CONVERGED = 1, MPN_JPEG_ENT_BAD_DATA = 2, MPN_JPEG_ENT_SKIPPED = 3 };
#define MPN_JPEG_SUBSEQ_BITS 1024
#define MPN_JPEG_GROUP_SUBSEQ 256
#define MPN_JPEG_MAX_PASSES 64
#define MPN_JPEG_MAX_FILE_BYTES (1 << 28)       /* keeps every bit position of a file in 32 bits */
#define MPN_JPEG_SCAN_DESC_BYTES 2704
typedef struct mpn_jpeg_scan_desc {
    int64_t file_offset;                        /* CALLER: byte offset of the file in files, multiple of 16 */
    int64_t coef_offset;                        /* CALLER: byte offset of its coefficients in coefs, multiple of 16 */
    int64_t src_offset, work_offset;            /* CALLER: copied into the mpn_jpeg_desc written for mpn_jpeg_decode */
    int64_t nbytes;                             /* size of the file */
    int64_t scan_offset;                        /* first entropy-coded byte */
    int32_t width, height, components, h_samp, v_samp;
    int32_t restart_interval;                   /* in MCUs; 0 = none */
    int32_t total_blocks;
    int32_t blocks_w[3], blocks_h[3];
    int32_t dc_table[3], ac_table[3];           /* per component: index into huff_bits / huff_vals */
    int32_t supported, reason;                  /* as mpn_jpeg_header */
    int32_t reserved[3];
    uint16_t quant[3][64];                      /* per component, natural order */
    uint8_t huff_bits[2][4][16];                /* [class: DC, AC][id]: codes of length 1..16 */
    uint8_t huff_vals[2][4][256];               /* their symbols */
} mpn_jpeg_scan_desc;
typedef struct mpn_jpeg_entropy_record {
    int32_t status, passes, blocks, reserved;
} mpn_jpeg_entropy_record;
#ifdef __cplusplus
static_assert(sizeof(mpn_jpeg_scan_desc) == MPN_JPEG_SCAN_DESC_BYTES, "descriptor size is fixed");
static_assert(sizeof(mpn_jpeg_entropy_record) == 16, "record size is fixed");
#endif
size_t mpn_jpeg_scan_desc_bytes(void);
int mpn_jpeg_scan_prepare(const uint8_t* data /* host */, size_t nbytes, mpn_jpeg_scan_desc* out /* host */);
size_t mpn_jpeg_entropy_decode_device_workspace_bytes(int B, long long total_file_bytes);
int mpn_jpeg_entropy_decode_device(const uint8_t* files, size_t files_bytes, const void* scan_descs, int B, int16_t* coefs,
                                   size_t coef_bytes, void* jpeg_descs_out, void* records, void* work, size_t work_bytes,
                                   int max_passes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * JPEG encode, all of it on the device: baseline, three components (YCbCr), luma sampling 1x1, 2x1 or 2x2 with chroma 1x1,
 * the standard (Annex K) Huffman tables, no restart intervals. The entropy-coded scan equals, byte for byte, the one
 * libjpeg(-turbo) - and so Pillow's `save(buf, "JPEG", quality=q, subsampling=s)` - writes for the same pixels and tables;
 * the headers in front of it are host bytes (multiposenet_amd.inference.jpeg.jpeg_headers). Two entry points, both over a
 * ragged batch described by [B] mpn_jpeg_enc_desc on the DEVICE, no host synchronisation, no allocation: capturable.
 *
 * mpn_jpeg_forward: pixels -> quantised coefficients in the layout mpn_jpeg_entropy_decode produces (int16, natural order,
 * one plane of blocks per component on the padded whole-MCU grid), image b's planes at byte coef_offset. One launch.
 *   sources   packed uint8 images; image b at byte src_offset as [height, width, channels], channels 3 (RGB) or 4 (RGBA,
 *             alpha ignored: the layout mpn_draw_detections writes)
 *   colour    RGB -> YCbCr in 16-bit fixed point (jccolor.c): constants (int)(x * 65536 + 0.5); Y adds 32768, Cb and Cr add
 *             (128 << 16) + 32767, then >> 16
 *   edges     columns: the source's right column is replicated (luma to the block grid, chroma - before downsampling - to
 *             the MCU width). Rows: the last source row is replicated up to a multiple of v_samp only; after downsampling
 *             the last DOWNSAMPLED row is replicated to the block grid
 *   chroma    h2v2: (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2, ... by output column; h2v1: (a + b + bias) >> 1, bias 0, 1, ...
 *   DCT       slow integer (jfdctint.c): samples - 128, 13-bit constants, rows first keeping 2 extra bits, then columns,
 *             descale (x + 2^(n-1)) >> n; the result is 8x the DCT
 *   quantise  q8 = 8 * quant: sign(c) * ((|c| + (q8 >> 1)) / q8)
 *   dummy blocks (luma blocks of the padded grid beyond ceil(width/8) x ceil(height/8)): 63 zero AC terms and the DC of the
 *             preceding block in MCU order (jccoefct.c)
 *
 * mpn_jpeg_entropy_encode: coefficients -> image b's scan at byte out_offset of `out`: MCU-interleaved Huffman coding, the
 * last byte padded with 1-bits, a 0x00 stuffed behind every 0xFF, then FF D9. `records` [B] mpn_jpeg_stream_record receives
 * (out_offset, size, status) per image:
 *   MPN_JPEG_ENC_OK           size bytes were written at out_offset
 *   MPN_JPEG_ENC_NO_FIT       size > capacity: nothing was written; size is the size the stream needs
 *   MPN_JPEG_ENC_NO_FIT_RAW   even the unstuffed stream exceeds capacity: nothing was written; size is a LOWER bound
 *   MPN_JPEG_ENC_SKIPPED      the descriptor is out of range (below); size 0
 * Seven launches: bit count per block (the DC predictor is the previous block of the component in scan order), a scan of
 * the counts (chunk sums; one workgroup per image scans the chunks), zeroing of the bit buffer, the emit pass (each block's
 * bits are ORed into the buffer with global atomics), the count of 0xFF bytes per chunk, its scan (which also writes the
 * record), and the scatter of the stuffed bytes and the trailer.
 *   work      image b's share at byte work_offset: mpn_jpeg_entropy_encode_workspace_bytes(total blocks of the image,
 *             capacity) bytes (0 for arguments out of range); nothing in it needs initialising
 * src_offset, coef_offset, out_offset and work_offset are multiples of 16. The kernels recompute an image's geometry from
 * (width, height, h_samp, v_samp) and skip an image whose descriptor is out of range (sides in [1, 65535], at most
 * MPN_JPEG_ENC_MAX_BLOCKS blocks, channels 3 or 4, one of the three samplings, capacity in [16, 2^30]), misaligned, or that
 * reaches outside sources_bytes / coef_bytes / out_bytes / work_bytes: no descriptor makes them read or write outside the
 * buffers, and nothing outside [out_offset, out_offset + capacity) is written for an image. A quantisation entry of 0 is
 * taken as 1. Grid and block sizes depend on B alone. Checked before any HIP call: null pointers (MPN_ERR_BAD_ARG); 1 <= B <=
 * 65535 (MPN_ERR_BAD_SHAPE); alignment (MPN_ERR_BAD_ALIGN); sources_bytes >= 3, coef_bytes >= 128, out_bytes >= 16,
 * work_bytes >= 16 (MPN_ERR_WORKSPACE).
 */
enum { MPN_JPEG_ENC_OK = 0, MPN_JPEG_ENC_NO_FIT = 1, MPN_JPEG_ENC_NO_FIT_RAW = 2, MPN_JPEG_ENC_SKIPPED = 3 };
#define MPN_JPEG_ENC_MAX_BLOCKS (1 << 21)       /* keeps every bit offset of a scan in 32 bits */
#define MPN_JPEG_ENC_DESC_BYTES 512
typedef struct mpn_jpeg_enc_desc {
    int64_t src_offset;                         /* byte offset of the pixels in sources */
    int64_t coef_offset;                        /* byte offset of the coefficients in coefs */
    int64_t out_offset;                         /* byte offset of the scan in out (entropy encode) */
    int64_t capacity;                           /* bytes the scan may take at out_offset */
    int64_t work_offset;                        /* byte offset of the image's share of work (entropy encode) */
    int32_t width, height, channels, h_samp, v_samp;
    int32_t reserved[17];
    uint16_t quant[3][64];                      /* per component, natural order */
} mpn_jpeg_enc_desc;
typedef struct mpn_jpeg_stream_record {
    int64_t offset, size;
    int32_t status, reserved[3];
} mpn_jpeg_stream_record;
#ifdef __cplusplus
static_assert(sizeof(mpn_jpeg_enc_desc) == MPN_JPEG_ENC_DESC_BYTES, "descriptor size is fixed");
static_assert(sizeof(mpn_jpeg_stream_record) == 32, "record size is fixed");
#endif
size_t mpn_jpeg_enc_desc_bytes(void);
int mpn_jpeg_forward(const uint8_t* sources, size_t sources_bytes, const void* descs, int B, int16_t* coefs, size_t coef_bytes,
                     mpn_stream_t stream);
size_t mpn_jpeg_entropy_encode_workspace_bytes(long long total_blocks, long long capacity);
int mpn_jpeg_entropy_encode(const int16_t* coefs, size_t coef_bytes, const void* descs, int B, uint8_t* out, size_t out_bytes,
                            void* records, void* work, size_t work_bytes, mpn_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Test-time augmentation of the joint inference graph: heatmaps averaged over the image, its mirror and further input sizes,
 * on the device (multiposenet_amd/inference/detector.py: flip=, scales=). tests/tta_ref.py restates both in numpy float32;
 * the kernels equal it bit for bit.
 *
 *   mpn_mirror_images   in, out uint8 [n,h,w,3], DIFFERENT buffers: out[i,y,x,:] = in[i,y,w-1-x,:]. Any n, h, w >= 1 with
 *                       n*h*w < 2^31 (MPN_ERR_BAD_SHAPE).
 *   mpn_tta_merge       sources: num_sources (1 .. MPN_TTA_MAX_SOURCES) mpn_tta_source in HOST memory, read before the
 *                       launch and passed to the kernel by value: heat f32 [B,h,w,17] (sigmoid heatmaps) and seg f32 [B,h,w]
 *                       (the raw mask channel), DEVICE, of the same B images at the source's own size h x w.
 *                       heat_out f32 [B,h0,w0,17], seg_out f32 [B,h0,w0], no source's buffer. Per output value, every
 *                       operation a separately rounded IEEE f32 operation, nothing contracted:
 *                         un-mirror  element (y, x, c) of a mirrored source's map is heat[y, w-1-x, FLIP_ORDER[c]] and
 *                                    seg[y, w-1-x]; FLIP_ORDER = 0, 2,1, 4,3, ..., 16,15 (keypoint_augment.FLIP_ORDER)
 *                         resize     of that un-mirrored map to h0 x w0, bilinear, half-pixel centres, clamped edges:
 *                                    sy = (y + 0.5f) * ((float)h / (float)h0) - 0.5f clamped to [0, h-1], y0 = floor(sy),
 *                                    y1 = min(y0+1, h-1), fy = sy - y0; the same along x; top = a00 + (a01 - a00) * fx,
 *                                    bot = a10 + (a11 - a10) * fx, v = top + (bot - top) * fy. A source with h == h0 and
 *                                    w == w0 is read directly.
 *                         average    sum = v_0, then sum = sum + v_k for k = 1, 2, ... in the order given;
 *                                    out = sum / (float)num_sources.
 *                       Checked before the launch: null pointers, num_sources, a source that is an output (MPN_ERR_BAD_ARG);
 *                       B, h0, w0, h, w >= 1, B*h0*w0*18 and every B*h*w*17 < 2^31 (MPN_ERR_BAD_SHAPE).
 * One launch each; grid and block sizes depend on the shapes alone, so the calls can be captured.
 */
#define MPN_TTA_MAX_SOURCES 8
typedef struct mpn_tta_source {
    const float* heat;
    const float* seg;
    int32_t h, w;
    int32_t mirrored;                           /* non-zero: the maps of the mirrored input */
    int32_t reserved;
} mpn_tta_source;
int mpn_mirror_images(const uint8_t* in, int n, int h, int w, uint8_t* out, mpn_stream_t stream);
int mpn_tta_merge(const mpn_tta_source* sources, int num_sources, int B, int h0, int w0, float* heat_out, float* seg_out,
                  mpn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPN_H_ */
