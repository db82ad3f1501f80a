/*
 * unetpp_hip.h -- C ABI of the MI355X (gfx950) UNet_Nested forward/backward path.
 *
 * The reference (unanan/UNet_Nested4Tiny_Objects_Keypoints) has no FFI of its own: its hot
 * path is reached through the torch.nn.Module API of models/unet.py and executes inside
 * torch.nn layers.  Each entry point below therefore cites the torch.nn call site in
 * /root/reference/models/unet.py that it replaces.  All functions
 *   - take plain device pointers, explicit sizes and a hipStream_t (passed as void*),
 *   - never allocate, never synchronise, never own memory,
 *   - return 0 on success or a negative UNETPP_E* code (nothing is thrown across the ABI),
 *   - are asynchronous on `stream` and re-entrant per (device, stream).
 * State.  No entry point passes data to another through the library: whatever a launch needs travels in its arguments
 * (the number of BatchNorm rows a convolution wrote reaches its finalize inside unetpp_gemm_fwd by value).  What the
 * library does keep, all of it configuration or diagnostics and none of it per call:
 *   - the CU count of each device (queried once) and, per kernel and device, the "large LDS" opt-in of the runtime;
 *   - unetpp_set_reserved_cus(): one process-wide integer;
 *   - unetpp_debug_set(): a process-wide table of dispatcher switches for A/B runs and tests, initialised ONCE from
 *     UNETPP_* environment variables at the first lookup -- no launch path reads the environment;
 *   - unetpp_last_kernel_name(): a thread-local pointer to a static string (profiling label).
 *
 * Tensor layout on the device is NHWC fp32 ("pixel-major": the channels of one pixel are
 * contiguous).  A `unetpp_view` names a channel slice of such a tensor, optionally sampled
 * on a strided pixel grid; the multi-view GEMM uses that to read a dense-skip concatenation
 * (models/unet.py:198-202) without materialising it, and to express the 2x2/stride-2
 * transposed convolution (models/unet.py:187) as a pointwise GEMM plus pixel shuffle.
 */
#ifndef UNETPP_HIP_H
#define UNETPP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNETPP_ABI_VERSION 14
#define UNETPP_MAX_VIEWS 8

#define UNETPP_OK 0
#define UNETPP_EINVAL (-1)   /* bad argument (null pointer, size <= 0, unsupported shape) */
#define UNETPP_ELAUNCH (-2)  /* hipLaunchKernel reported an error */

/* A channel slice [c_off, c_off + c_len) of an NHWC fp32 tensor [N, Hs, Ws, C], sampled at
 * tensor pixel (y*sy + oy, x*sx + ox) for logical pixel (y, x).  sy = sx = 1, oy = ox = 0
 * is the plain case. */
typedef struct unetpp_view {
  float* ptr;
  int32_t C, c_off, c_len;
  int32_t Hs, Ws;
  int32_t sy, sx, oy, ox;
  /* on load : v = v * scale[c] + shift[c] (c counted inside the slice) when scale != NULL
   * on store: unused */
  const float* scale;
  const float* shift;
  /* ReLU-backward gate: an NHWC tensor with the same geometry as `ptr`; the value is
   * multiplied by (gate > 0).  Applied on load for inputs, on store for outputs. */
  const float* gate;
  int32_t relu;        /* load: max(v, 0) after the affine; store: max(v, 0) after the bias */
  int32_t accumulate;  /* store only: dst += v instead of dst = v */
  int32_t gate_sum;    /* store only, with gate: 0 = gate this contribution before it is added,
                        * 1 = gate the accumulated sum (the last contribution applies the ReLU mask) */
  int32_t reserved;
} unetpp_view;

/* rows = N*H*W logical pixels;  out[p, n] = bias[n] + sum_{tap, k} in[p (+) tap, k] * weight[tap][k][n]
 * K = sum of in[].c_len (virtual channel concatenation in view order), Ncols = sum of out[].c_len.
 * taps = 9: 3x3 window, zero padding 1 (padding is applied AFTER the per-view load transform);
 * taps = 1: pointwise.  Replaces nn.Conv2d(.,.,3,1,1) (models/unet.py:132,140), its input
 * gradient, nn.ConvTranspose2d(.,.,2,2,0) (:187) forward and input gradient, nn.Conv2d(.,.,1) (:191). */
#define UNETPP_GEMM_DIRECT 1 /* flags: direct summation only.  Without it 3x3 launches on the fast path use the
                              * Winograd F(2x2,3x3) form: same fp32 result up to rounding (~1e-7 relative), 2.25x
                              * fewer multiplies.  The flag must be the same when the weight image is packed. */
#define UNETPP_GEMM_BF16 2   /* flags (GEMM and weight-gradient descriptors): bf16 STORAGE -- every activation pointer of
                              * the descriptor (view ptr and gate) addresses bf16 NHWC data although it is typed
                              * float*; C, c_off, c_len count bf16 channels and must be multiples of 8.  bias, scale,
                              * shift, stats_partial and slabs stay fp32; the arithmetic is v_mfma_f32_32x32x16_bf16
                              * with fp32 accumulation (BASELINE configs[3]/[4]).  There is no generic bf16 kernel:
                              * a descriptor the MFMA kernels cannot take returns UNETPP_EINVAL. */
/* BatchNorm2d training-mode finalize (models/unet.py:133) attached to the convolution call that takes the statistics:
 * the call leaves mean, invstd, scale = gamma * invstd, shift = beta - mean * scale ([Ncols] each) and the updated
 * running statistics behind, exactly as a unetpp_bn_finalize call of the caller would.  The persistent kernels then
 * write ONE row of sums per workgroup (all its units; <= 2048 rows instead of one per 256-pixel block) and the library
 * enqueues the finalize over those rows itself; kernels without that epilogue (generic shapes, more than 256
 * columns) keep per-block rows.  Same result up to the row partition of the fp32 sums.
 * scale == NULL: not attached (the caller finishes stats_partial with unetpp_bn_finalize). */
typedef struct unetpp_bn_fused {
  const float* gamma;
  const float* beta;
  float* running_mean; /* both NULL or both set */
  float* running_var;
  float* mean;
  float* invstd;
  float* scale;
  float* shift;
  int64_t count;     /* N*H*W */
  float eps, momentum;
} unetpp_bn_fused;

typedef struct unetpp_gemm_desc {
  int32_t N, H, W;
  int32_t taps;
  int32_t n_in;
  int32_t n_out;
  int32_t flags;    /* UNETPP_GEMM_* */
  int32_t reserved; /* 0 */
  unetpp_view in[UNETPP_MAX_VIEWS];
  unetpp_view out[UNETPP_MAX_VIEWS];
  const float* weight; /* packed [taps][K][Ncols] (see unetpp_pack_weight); may be NULL when weight_image is set */
  const float* bias;   /* [Ncols] or NULL */
  /* optional BatchNorm statistics epilogue: per pixel-block partial (sum, sum of squares) of the
   * stored values, [unetpp_gemm_pixel_blocks()][Ncols][2]; requires n_out == 1.  With `bn` set the buffer is
   * workspace of [unetpp_gemm_stats_rows()][Ncols][2] floats whose row structure is the kernel's own. */
  float* stats_partial;
  /* optional fast path: `weight` re-laid as the kernel's LDS image by unetpp_gemm_pack_weight_image
   * (unetpp_gemm_weight_image_floats() floats).  NULL selects the generic kernel. */
  const float* weight_image;
  unetpp_bn_fused bn; /* bn.scale != NULL: finish the statistics inside this call (needs stats_partial) */
} unetpp_gemm_desc;

/* weight gradient:  dW[tap][k][n] = sum_p x[p (+) tap, k] * dy[p, n]  (+ db[n] = sum_p dy[p, n]).
 * Replaces the weight/bias gradient of nn.Conv2d 3x3 / 1x1 and nn.ConvTranspose2d 2x2 s2
 * (autograd of models/unet.py:132,140,187,191).  Split over pixel blocks: each of the
 * `n_split` blocks per (k-tile, n-tile) writes one partial slab; unetpp_wgrad_finish sums them.
 * unetpp_wgrad_plan chooses n_split and tells how large the slabs are. */
typedef struct unetpp_wgrad_desc {
  int32_t N, H, W;
  int32_t taps;
  int32_t n_x;
  int32_t n_dy;
  unetpp_view x[UNETPP_MAX_VIEWS];  /* K = sum c_len */
  unetpp_view dy[UNETPP_MAX_VIEWS]; /* Ncols = sum c_len (several views: the 4 pixel phases of a 2x2 deconv) */
  int32_t n_split;                  /* partial slabs (unetpp_wgrad_plan) */
  int32_t flags;                    /* UNETPP_GEMM_DIRECT: direct summation only (no Winograd) */
  float* slabs;                    /* [n_split][planes*K + 1][Ncols] (unetpp_wgrad_plan: slab_floats); last row = db */
} unetpp_wgrad_desc;

int unetpp_abi_version(void);
const char* unetpp_build_arch(void); /* "gfx950" */

/* Name of the device kernel (and, where a launcher has several, of the form) that the calling thread's most recent
 * launching call chose: the GEMMs and weight gradients, the heads, the optimizer, the matcher and the streaming
 * launchers (BatchNorm finalize / apply / backward, pool passes, bilinear x2, layout converters).  unetpp_gemm_fwd keeps
 * its GEMM's label over an attached BatchNorm finalize; unetpp_sum_partials, the packers and the loss set none.  Read it
 * right after the call in question: any later labelled call replaces it.  Profiling labels (the rocprofv3 kernel name
 * up to template arguments, or name/form).  Static string, "" before the first call.  Diagnostic only (thread-local). */
const char* unetpp_last_kernel_name(void);

/* Dispatcher switches for A/B measurements and for tests that hold two kernels against each other inside one process
 * (v9; replaces per-launch getenv).  `name` is the switch without its UNETPP_ prefix: BF16_NO_DMA, BF16_DMA_ALL,
 * BF16_DMA_MIN8, BF16_DMA_FORM, BF16_DMA_SMALL, BF16_DMA_STATS, BF16_DMA_POINTWISE, BF16_DMA_SPLIT, BF16_WGRAD_QUAD,
 * WINO_NO_LEAN, WINO_ONE_PER_CU, MEMSET_NODES, BF16_PW_PLAIN, PW_DIRECT (0: fp32 pointwise launches back on the LDS-staged
 * kernels), PW_NT (fp32 pointwise GEMM: 1 / 0 = non-temporal / plain stores whatever the output size),
 * HEAD_WGS_PER_CU (bf16 head backward: at most this many workgroups per CU take tiles, default 4; 0 = the whole grid),
 * SMALL_WGRAD_BLOCKS (unetpp_wgrad_plan: slabs aimed at for a single x view on a 1..4-channel tensor, default 1024).  set != 0: the switch takes `value`; set == 0: back to the
 * dispatcher's built-in default.  The environment variable UNETPP_<name>, if present when the library first looks a
 * switch up, is the initial setting.  Process-wide; results never depend on a switch beyond the summation order of the
 * kernel it selects.  UNETPP_EINVAL for an unknown name. */
int unetpp_debug_set(const char* name, int64_t value, int32_t set);
/* The current state of a switch (v10): returns 1 and stores its value in *value when the switch is set (by
 * unetpp_debug_set or by its environment variable), 0 when it is unset (*value untouched), UNETPP_EINVAL for an unknown
 * name.  Lets a scoped override put back what it found. */
int unetpp_debug_get(const char* name, int64_t* value);

/* Data-parallel co-scheduling knob (v8).  Every hot kernel is a persistent launch sized to fill all CUs at 2-3 workgroups
 * per CU, so a collective kernel (RCCL all-reduce of a gradient bucket on a side stream, trainer/trainer.py:338's
 * replicas replaced by one process per GPU) only gets waves when a compute kernel ends.  n > 0 makes the persistent
 * grids leave n CUs' worth of workgroups unlaunched (unetpp_wgrad_plan scales n_split likewise); 0 (default,
 * or the UNETPP_RESERVED_CUS environment variable read at the first call) = use every CU.  Process-wide, takes effect
 * at the next launch; results do not depend on it.  Returns the value now in force (n clamped to [0, CUs - 8]);
 * unetpp_set_reserved_cus(-1) only reads it. */
int32_t unetpp_set_reserved_cus(int32_t n);
/* CUs of the current device a persistent grid may fill (physical - reserved, at least 8); *physical (may be NULL) gets
 * the device's CU count (v9). */
int32_t unetpp_usable_cus(int32_t* physical);

/* ---- multi-view pixel GEMM on MFMA (v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32) ------ */
int64_t unetpp_gemm_pixel_blocks(int32_t N, int32_t H, int32_t W);
/* rows of [Ncols][2] floats stats_partial must hold when the finalize is fused (d->bn.scale != NULL) */
int64_t unetpp_gemm_stats_rows(int32_t N, int32_t H, int32_t W);
/* What a forward / input-gradient GEMM launch needs settled before it runs (v13).  The library looks at the descriptor
 * once and decides which of its kernels takes it; the size of the weight image, the grid, the rows of an attached
 * BatchNorm finalize and the label all follow from that one decision, and unetpp_gemm_fwd launches the same kernel for the
 * same descriptor on a device with that many usable CUs. */
typedef struct unetpp_gemm_sizes {
  int64_t image_floats;   /* what d->weight_image must hold for this descriptor; 0: no image kernel applies */
  int64_t bn_rows;        /* rows the attached finalize reads; 0: one per 256-pixel block */
  int32_t workgroups, threads; /* grid and workgroup size of the (first) launch */
  const char* kernel;     /* label unetpp_last_kernel_name() reports after unetpp_gemm_fwd(d) (static string) */
} unetpp_gemm_sizes;
/* Everything in the descriptor, pointers included (their alignment selects kernels), must be what unetpp_gemm_fwd will
 * get, with ONE exception: only whether d->weight_image is NULL counts, not where it points -- NULL plans the kernels
 * that read d->weight (first layer, generic), anything else the image kernels, so a caller that has not allocated the
 * image yet passes any non-NULL value and allocates image_floats.  image_floats itself does not depend on
 * d->weight_image (it is unetpp_gemm_weight_image_floats(d)).  cus = usable CUs to plan for (the 8-wave LDS-DMA form
 * and every persistent grid depend on it), <= 0: those of the current device (unetpp_usable_cus).  Touches no device
 * memory and launches nothing.  UNETPP_EINVAL for a NULL argument or a descriptor unetpp_gemm_fwd would refuse (a bf16
 * descriptor without an image that is not a first layer; an image on a descriptor no image kernel can read; ...);
 * UNETPP_ELAUNCH when cus <= 0 and there is no device to ask. */
int unetpp_gemm_plan(const unetpp_gemm_desc* d, int32_t cus, unetpp_gemm_sizes* out);
int unetpp_gemm_fwd(const unetpp_gemm_desc* d, void* stream);
/* Fast path (register-prefetched LDS-image kernels; Winograd F(2x2,3x3) for taps = 9 unless UNETPP_GEMM_DIRECT):
 * applies when every input view is a 16-byte aligned slice without a ReLU gate on load (C, c_off and c_len
 * multiples of 4; an affine + ReLU load transform is allowed).  Returns the image size in floats, or 0 when the
 * descriptor must use the generic kernel. */
int64_t unetpp_gemm_weight_image_floats(const unetpp_gemm_desc* d);
/* The image of d, one launch of the packer on the job (taps, flags, channel counts of d's views; source; image) passed as
 * the kernel argument: stream-ordered, no allocation, copy or synchronisation (capturable).  UNETPP_EINVAL, and no launch,
 * for a NULL operand or a descriptor without an image (unetpp_gemm_weight_image_floats(d) == 0). */
int unetpp_gemm_pack_weight_image(const unetpp_gemm_desc* d, float* image, void* stream); /* from d->weight (packed) */
/* The same image built straight from a parameter in its torch layout (no unetpp_pack_weight pass; d->weight may be
 * NULL for a launch that carries a weight image).  Element W[tap][k][n] of the GEMM weight is read at
 *   src[tap' * s_t + (k % k_inner) * s_k + (k / k_inner) * s_ko + (n % n_inner) * s_n + (n / n_inner) * s_no],
 * tap' = flip ? taps-1-tap : tap; k_inner / n_inner = 0 mean "no split".  nn.Conv2d [co,ci,3,3] forward:
 * (s_t,s_k,s_n) = (1, 9, 9ci); its input gradient: flip, (1, 9ci, 9); nn.ConvTranspose2d [ci,co,2,2] forward
 * (N = phase*co + c): s_k = 4co, n_inner = co, s_n = 4, s_no = 1; its input gradient (K = phase*co + c): k_inner = co,
 * s_k = 4, s_ko = 1, s_n = 4co. */
typedef struct unetpp_weight_src {
  const float* src;
  int64_t s_t, s_k, s_ko, s_n, s_no;
  int32_t k_inner, n_inner, flip, reserved;
} unetpp_weight_src;
int unetpp_gemm_pack_weight_image_from(const unetpp_gemm_desc* d, const unetpp_weight_src* src, float* image, void* stream);
/* Many images in ONE launch (all launches of a forward or backward pass) of the same packer: a table of jobs in DEVICE
 * memory.  A job carries what the image layout depends on -- taps, flags and the channel counts of the launch's input / output views
 * (must describe a launch for which unetpp_gemm_weight_image_floats() > 0) -- plus source and destination.
 * max_image_floats = the largest image of the table (sizes the grid the jobs share, by the rule that sizes a single
 * image's). */
typedef struct unetpp_pack_job {
  unetpp_weight_src src;
  float* image;
  int32_t taps, flags, n_in, n_out;
  int32_t in_len[UNETPP_MAX_VIEWS], out_len[UNETPP_MAX_VIEWS];
} unetpp_pack_job;
int unetpp_gemm_pack_weight_images(const unetpp_pack_job* jobs_device, int32_t n_jobs, int64_t max_image_floats,
                                   void* stream);

/* What a weight-gradient launch needs settled before it runs (v12).  The library looks at the descriptor once and
 * decides which of its kernels takes it; n_split, the slab layout and the label all follow from that one decision, and
 * unetpp_wgrad launches the same kernel for the same descriptor. */
typedef struct unetpp_wgrad_sizes {
  int32_t n_split;             /* goes into unetpp_wgrad_desc.n_split */
  int32_t planes;              /* per slab: `taps` for direct summation, 16 for the Winograd F(2x2,3x3) kernel (it accumulates
                                  transform-domain products); the `taps` argument of unetpp_wgrad_finish */
  int32_t pairs_per_workgroup; /* (32-channel, 32-column) tile pairs a workgroup owns: 1, 4 (bf16, every view a multiple of
                                  64 channels wide) or 8 (fp32 pointwise blocks) */
  int32_t reserved;
  int64_t slab_floats;         /* n_split * (planes * K + 1) * Ncols: what d->slabs must hold */
  const char* kernel;          /* label unetpp_last_kernel_name() reports after unetpp_wgrad(d) (static string) */
} unetpp_wgrad_sizes;
/* d->n_split and d->slabs are ignored; everything else, pointers included (their alignment selects kernels), must be
 * what unetpp_wgrad will get.  target_blocks = workgroups to aim at, <= 0: the library's default (256).  The plan aims
 * at 1024 slabs for a single x view on a 1..4-channel tensor whatever target_blocks says, scales the target by usable /
 * physical CUs (unetpp_set_reserved_cus), and never plans more slabs than there are 256-pixel tiles, or 4096.  Touches
 * no device memory and launches nothing.  UNETPP_EINVAL for a NULL argument or a descriptor unetpp_wgrad would refuse.
 * Any n_split from 1 to the number of pixel tiles (at most 4096) is valid for unetpp_wgrad; planes and kernel do not
 * depend on it. */
int unetpp_wgrad_plan(const unetpp_wgrad_desc* d, int32_t target_blocks, unetpp_wgrad_sizes* out);
int unetpp_wgrad(const unetpp_wgrad_desc* d, void* stream);
/* `taps` = planes per slab.  column n = o*n_inner + i:  dw[t*d_t + k*d_k + i*d_n + o*d_o] = sum_s slabs[s][t*K + k][n];
 * db[i] = sum_o sum_s slabs[s][taps*K][o*n_inner + i]   (n_inner = Ncols for a plain convolution) */
int unetpp_wgrad_finish(const float* slabs, int32_t n_split, int32_t taps, int32_t K, int32_t Ncols, int32_t n_inner,
                        float* dw, int64_t d_t, int64_t d_k, int64_t d_n, int64_t d_o, float* db, void* stream);

/* dst[t*d_t + k*d_k + n*d_n] = src[tt*s_t + k*s_k + n*s_n], tt = flip ? T-1-t : t.
 * Re-lays a torch-layout weight ([co,ci,3,3] / [ci,co,2,2], the state-dict contract of
 * models/unet.py) into the packed [taps][K][Ncols] operand of the GEMM. */
int unetpp_pack_weight(float* dst, const float* src, int32_t T, int32_t K, int32_t Ncols,
                       int64_t d_t, int64_t d_k, int64_t d_n, int64_t s_t, int64_t s_k, int64_t s_n,
                       int32_t flip, void* stream);
/* Many strided copies in ONE launch: dst[o*dst_stride + i] = src[o*src_stride + i], o < n_outer, i < n_inner (floats;
 * n_outer*n_inner < 2^31 per job; 16-byte pieces when pointers, n_inner and strides allow).  The job table lives in
 * DEVICE memory; max_elems = the largest n_outer*n_inner of the table (sizes the grid).  Host-side re-layouts of a pass
 * that are not weight images: the bias of a 2x2 transposed convolution repeated for its four pixel phases (the GEMM
 * column is phase*co + c: src_stride 0, n_outer 4), the input-gradient weights of the dense skips grouped by producer
 * (channel slices of the consumers' conv1 weights, the torch.cat of models/unet.py:198-202, stacked along the output-channel axis). */
typedef struct unetpp_copy_job {
  const float* src;
  float* dst;
  int64_t n_outer, n_inner, src_stride, dst_stride;
} unetpp_copy_job;
int unetpp_copy_jobs(const unetpp_copy_job* jobs_device, int32_t n_jobs, int64_t max_elems, void* stream);

/* ---- BatchNorm2d, training mode (models/unet.py:133) -------------------------------------- */
/* partial [n_blocks][C][2] (sum, sumsq) -> mean, invstd, scale = gamma*invstd, shift = beta - mean*scale;
 * running_mean/var updated with `momentum` (unbiased variance), all [C]. count = N*H*W. */
int unetpp_bn_finalize(const float* partial, int64_t n_blocks, int32_t C, int64_t count,
                       const float* gamma, const float* beta, float eps, float momentum,
                       float* running_mean, float* running_var,
                       float* mean, float* invstd, float* scale, float* shift, void* stream);
/* eval mode: scale/shift from running statistics */
int unetpp_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                          const float* running_var, float eps, int32_t C, float* scale, float* shift,
                          void* stream);
/* the same coefficients (the same kernel: identical bits) plus what the backward of a frozen layer needs: invstd =
 * 1/sqrt(running_var + eps) and a snapshot of running_mean, both [C] (added within ABI 12) */
int unetpp_bn_eval_coeffs_stats(const float* gamma, const float* beta, const float* running_mean,
                                const float* running_var, float eps, int32_t C, float* scale, float* shift,
                                float* mean, float* invstd, void* stream);
/* act = relu?(y*scale + shift) (scale may be NULL = identity);  optional fused nn.MaxPool2d(2)
 * (models/unet.py:219): pooled [N,H/2,W/2,C] and pool_idx (uint8 window index 0..3, first max wins).
 * act may be NULL when only the pooled output is wanted; pool_idx may be NULL when the winners are not (forward-only
 * callers; backward needs them).  Odd H or W: the window grid is floor(H/2) x floor(W/2) as in
 * nn.MaxPool2d (the last row / column is in no window; act still covers every pixel). */
int unetpp_affine_relu_pool(const float* y, const float* scale, const float* shift, int32_t relu,
                            int32_t N, int32_t H, int32_t W, int32_t C,
                            float* act, float* pooled, uint8_t* pool_idx, void* stream);
/* d_act[window argmax] += d_pooled */
int unetpp_maxpool_bwd(const float* d_pooled, const uint8_t* pool_idx, int32_t N, int32_t H, int32_t W,
                       int32_t C, float* d_act, void* stream);
int64_t unetpp_bn_bwd_blocks(int64_t pixels, int32_t C);
/* g = d_act * (y*scale+shift > 0); partial [blocks][C][2] = (sum g, sum g*xhat) */
int unetpp_bn_bwd_reduce(const float* d_act, const float* y, const float* scale, const float* shift,
                         const float* mean, const float* invstd, int64_t pixels, int32_t C,
                         float* partial, void* stream);
/* sums the partials -> dgamma, dbeta; then dy = gamma*invstd*(g - dbeta/M - xhat*dgamma/M) (dy may alias d_act) */
int unetpp_bn_bwd_finalize(const float* partial, int64_t n_blocks, int32_t C, float* dgamma, float* dbeta,
                           void* stream);
int unetpp_bn_bwd_apply(const float* d_act, const float* y, const float* scale, const float* shift,
                        const float* mean, const float* invstd, const float* gamma,
                        const float* dgamma, const float* dbeta, int64_t pixels, int32_t C,
                        float* dy, void* stream);

/* BatchNorm backward of an encoder node whose output was also 2x2 max-pooled (models/unet.py:257-263): the pooled
 * consumer's gradient d_pooled [N, H/2, W/2, C] is routed to the argmax recorded by unetpp_affine_relu_pool WHILE
 * d_act is read, in both passes, instead of a separate unetpp_maxpool_bwd pass over d_act.  Needs
 * unetpp_bn_bwd_pool_ok(N, H, W, C) (4-aligned C with a power-of-two C/4 <= 256, even H and W, < 2^31 elements);
 * and every operand but `partial` 16-byte aligned (pool_idx: 4 bytes); otherwise call unetpp_maxpool_bwd and the plain
 * functions.  unetpp_bn_bwd_plan (below) answers both questions for a whole call.  partial:
 * unetpp_bn_bwd_blocks(N*H*W, C) rows, finished by unetpp_bn_bwd_finalize as usual. */
int unetpp_bn_bwd_pool_ok(int32_t N, int32_t H, int32_t W, int32_t C);
int unetpp_bn_bwd_reduce_pool(const float* d_act, const float* y, const float* scale, const float* shift,
                              const float* mean, const float* invstd, const float* d_pooled, const uint8_t* pool_idx,
                              int32_t N, int32_t H, int32_t W, int32_t C, float* partial, void* stream);
int unetpp_bn_bwd_apply_pool(const float* d_act, const float* y, const float* scale, const float* shift,
                             const float* mean, const float* invstd, const float* gamma, const float* dgamma,
                             const float* dbeta, const float* d_pooled, const uint8_t* pool_idx, int32_t N, int32_t H,
                             int32_t W, int32_t C, float* dy, void* stream);

/* BatchNorm + ReLU backward of a FROZEN layer -- one that normalised with its running statistics (eval mode, or
 * BatchNormParams.eval() inside a training model); added within ABI 12.  With fixed statistics dy does not depend on
 * the channel sums, so ONE streaming pass (two reads, one write) replaces reduce + finalize + apply:
 *     g  = d_act (+ d_pooled where this pixel won its 2x2 window; d_pooled / pool_idx both NULL = no pooled consumer)
 *     gg = (fma(y, scale, shift) > 0) ? g : 0          scale / shift: unetpp_bn_eval_coeffs[_stats], the forward's bits
 *     dy = gg * scale                                  dy may alias d_act
 * partial != NULL: also partial[block][c] = (sum gg, sum gg * (y - mean) * invstd) in a fixed order (no float atomics),
 * unetpp_bn_frozen_bwd_blocks(N*H*W, C) rows (unused ones zeroed), finished into dbeta / dgamma by
 * unetpp_bn_bwd_finalize; mean / invstd from unetpp_bn_eval_coeffs_stats.  partial == NULL (gamma and beta frozen too):
 * no sums, no LDS, mean / invstd may be NULL, and dy has the same bits.  Forms: 16-byte vectors (C % 4 == 0, aligned
 * d_act / y / dy), scalar, and with d_pooled the row-structured routing form, which needs unetpp_bn_bwd_pool_ok and
 * 16-byte aligned coefficients (otherwise: unetpp_maxpool_bwd into d_act first, then d_pooled = NULL).
 * UNETPP_EINVAL without touching the device for NULL operands, C < 1 or N*H*W < 1. */
int64_t unetpp_bn_frozen_bwd_blocks(int64_t pixels, int32_t C);
int unetpp_bn_frozen_bwd(const float* d_act, const float* y, const float* scale, const float* shift,
                         const float* mean, const float* invstd, const float* d_pooled, const uint8_t* pool_idx,
                         int32_t N, int32_t H, int32_t W, int32_t C, float* dy, float* partial, void* stream);

/* What one BatchNorm + ReLU backward needs settled before it runs (v14).  The library looks at the call once, with the
 * selection its launchers use, and says how the pool gradient travels and how large `partial` is:
 *   training: unetpp_bn_bwd_reduce[_pool|_bf16], unetpp_bn_bwd_finalize, unetpp_bn_bwd_apply[_pool|_bf16]
 *   frozen:   unetpp_bn_frozen_bwd[_bf16], and unetpp_bn_bwd_finalize when want_sums. */
typedef struct unetpp_bn_bwd_query {
  int32_t frozen;     /* != 0: running statistics (unetpp_bn_frozen_bwd), else training mode */
  int32_t bf16;       /* != 0: d_act / y / dy / d_pooled address bf16 */
  int32_t want_sums;  /* frozen only: the gamma / beta sums are wanted (training mode always takes them) */
  int32_t N, H, W, C;
  int32_t reserved;
  /* every pointer the launches will get: only the addresses are looked at (their alignment selects kernels).  d_pooled
   * and pool_idx both NULL: no pooled consumer.  gamma / dgamma / dbeta: training mode only.  mean / invstd may be NULL
   * for a frozen layer without sums. */
  const void *d_act, *y, *dy, *scale, *shift, *mean, *invstd, *gamma, *dgamma, *dbeta, *d_pooled, *pool_idx;
} unetpp_bn_bwd_query;
typedef struct unetpp_bn_bwd_sizes {
  int32_t route;          /* 0: no pool gradient.  1: pass d_pooled / pool_idx to the launches (unetpp_bn_bwd_reduce_pool and
                             unetpp_bn_bwd_apply_pool in fp32 training mode), which route it while they read d_act.
                             2: unetpp_maxpool_bwd[_bf16] into d_act first, then the launches without a pool gradient */
  int32_t reserved;
  int64_t partial_rows;   /* rows of `partial` and n_blocks of unetpp_bn_bwd_finalize: what the unetpp_bn_*_blocks[_bf16]
                             function of the mode and storage type returns; 0 for a shape none of the kernels takes */
  int64_t partial_floats; /* partial_rows * C * 2 */
} unetpp_bn_bwd_sizes;
/* route is 1 exactly when EVERY launch of the sequence accepts the routing form for these shapes and addresses (fp32:
 * unetpp_bn_bwd_pool_ok and 16-byte aligned operands, coefficients and parameter gradients, 4-byte aligned pool_idx),
 * otherwise 2 where unetpp_maxpool_bwd[_bf16] and the plain forms accept.  UNETPP_EINVAL for a NULL argument, half a
 * pool gradient, or a call some launch of every route would refuse (bf16 storage with C != 8 * 2^k, or with a pool
 * gradient on odd H or W); partial_rows and partial_floats are filled all the same.
 * Touches no device memory and launches nothing. */
int unetpp_bn_bwd_plan(const unetpp_bn_bwd_query* q, unetpp_bn_bwd_sizes* out);

/* ---- deep-supervision head: sigmoid(Conv1x1(Dropout(x))) (models/unet.py:242-244,254,283-286) ---- */
/* x NHWC [P, C]; weight [n_cls, C]; out NCHW [N, n_cls, H, W].  Dropout: keep mask regenerated from
 * (seed, element index) with keep probability 1-p_drop, or read from `mask` (uint8 NHWC) when not NULL;
 * p_drop = 0 disables it.  seed_dev (v8, may be NULL): one uint64 in device memory that is ADDED to `seed` when the
 * kernel runs -- a launch captured in a HIP graph bakes `seed` in, so a replayed training step keeps the varying part
 * of its seed there (forward and backward of a step must see the same value). */
int unetpp_head_fwd(const float* x, const float* weight, const float* bias, int32_t N, int32_t H, int32_t W,
                    int32_t C, int32_t n_cls, float p_drop, uint64_t seed, const uint8_t* mask, const uint64_t* seed_dev,
                    float* out_nchw, void* stream);
int64_t unetpp_head_bwd_blocks(int64_t pixels);
/* d_out, out: NCHW.  dx (NHWC) is written (accumulate = 0) or added to; partial [blocks][n_cls*C + n_cls]. */
int unetpp_head_bwd(const float* d_out_nchw, const float* out_nchw, const float* x, const float* weight,
                    int32_t N, int32_t H, int32_t W, int32_t C, int32_t n_cls, float p_drop, uint64_t seed,
                    const uint8_t* mask, const uint64_t* seed_dev, float* dx, int32_t accumulate, int32_t gate_x, float* partial,
                    void* stream); /* gate_x: after the (optional) accumulate, dx *= (x > 0) -- the ReLU mask of x */
/* ---- one head of a training step in one pass (added within v13: new entry points only, nothing existing changes) ----
 * What unetpp_head_fwd, the gradient of unetpp_focal_bce_heads for this head (the mean over n_heads of FocalLoss_BCE_2d
 * against target_nchw [N,n_cls,H,W], `rows` and `gamma` as there) and unetpp_head_bwd (accumulate = 0) compute in three
 * launches, with the same bits: out_nchw, dx and every row of partial (unetpp_head_bwd_blocks(N*H*W) rows of
 * [n_cls*C + n_cls], finished by unetpp_sum_partials).  x is read once, the map is written and not read back, the loss
 * gradient is never written; the loss VALUE is unetpp_focal_bce_heads over the maps without gradient pointers.
 * Accepts fp32 calls that unetpp_head_fwd takes with its streaming kernel AND unetpp_head_bwd with its power-of-two one
 * (C = 4 * 2^k, 16 <= C <= 128, n_cls padded to 4 or 8 at most C / 4, 16-byte aligned x, weight and dx, a 4-byte
 * aligned mask, fewer than 2^31 - 1 elements of x), rows >= 1 and 1 <= n_heads <= UNETPP_MAX_HEADS; anything else
 * returns UNETPP_EINVAL without touching the device, and the caller runs the three launches. */
int unetpp_head_train(const float* x, const float* weight, const float* bias, const float* target_nchw, int32_t N,
                      int32_t H, int32_t W, int32_t C, int32_t n_cls, float p_drop, uint64_t seed, const uint8_t* mask,
                      const uint64_t* seed_dev, int64_t rows, float gamma, int32_t n_heads, float* out_nchw, float* dx,
                      int32_t gate_x, float* partial, void* stream);
/* ---- Monte-Carlo dropout at one head (added within v13: a new entry point only, nothing existing changes) ----
 * `samples` = K draws of the head's dropout over ONE read of x; two maps leave, fp32 NCHW [N, n_cls, H, W]:
 *   seed_k = seed + 0xD6E8FEB86659FD93 * k (mod 2^64), k = 0 .. K-1; *seed_dev (may be NULL) is added to each, as in
 *            unetpp_head_fwd.
 *   s_k    = at every pixel and class, bit for bit what unetpp_head_fwd with p_drop, seed_k, mask = NULL and seed_dev
 *            writes through its streaming kernel: the same keep flags and keep scale, the same order of the dot
 *            product and of its sum over the lanes of a pixel, the same sigmoid expression.
 *   mean   = (((s_0 + s_1) + ...) + s_{K-1}) / (float)K                        a true division
 *   var    = (((d_0*d_0 + d_1*d_1) + ...) + d_{K-1}*d_{K-1}) / (float)(K-1),   d_k = s_k - mean
 *            every difference, product, sum and quotient rounded on its own: no fused multiply-add in the fold.
 * No square root here (the caller derives a standard deviation), no atomics: the result does not depend on the grid.
 * x is read once, 16 bytes per lane and pixel; the K samples never reach memory.
 * Accepts exactly the fp32 calls that unetpp_head_fwd takes with its streaming kernel under hashed dropout (C = 4 * 2^k,
 * 16 <= C <= 128, n_cls padded to 4 or 8 at most C / 4, 16-byte aligned x and weight, fewer than 2^31 - 1 elements of
 * x) with 0 < p_drop < 1 and 2 <= samples <= UNETPP_MC_MAX_SAMPLES; anything else, a NULL x / weight / bias / mean_nchw /
 * var_nchw included, returns UNETPP_EINVAL without touching the device (the caller then composes K unetpp_head_fwd
 * launches). */
#define UNETPP_MC_MAX_SAMPLES 32
int unetpp_head_mc(const float* x, const float* weight, const float* bias, int32_t N, int32_t H, int32_t W, int32_t C,
                   int32_t n_cls, float p_drop, uint64_t seed, const uint64_t* seed_dev, int32_t samples,
                   float* mean_nchw, float* var_nchw, void* stream);
/* out[i] = sum_b partial[b][i], i < len (used for head dW/db) */
int unetpp_sum_partials(const float* partial, int64_t n_blocks, int64_t len, float* out, void* stream);

/* ---- bilinear x2, align_corners=True (nn.UpsamplingBilinear2d, models/unet.py:190) ---------- */
int unetpp_bilinear2x_fwd(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, float* y, void* stream);
int unetpp_bilinear2x_bwd(const float* dy, int32_t N, int32_t H, int32_t W, int32_t C, float* dx, int32_t accumulate,
                          void* stream);

/* ---- caller side of the training step (trainer/trainer.py:114-136) -------------------------- */
/* FocalLoss_BCE_2d (tools/losses/focal_loss.py:255-301, size_average = False), value and gradient in one pass:
 * e = 1 - |pred - target| + 1e-20;  loss = sum(-(1 - e)^gamma log e) / rows;  rows = N*C of the [N,C,H,W] heads.
 * partial[unetpp_focal_bce_blocks(n)] is workspace (per-block sums, added in fixed order); loss[0] receives the
 * value, grad (may be NULL) dloss/dpred.  pred/target/grad 16-byte aligned, n elements. */
int64_t unetpp_focal_bce_blocks(int64_t n);
int unetpp_focal_bce(const float* pred, const float* target, int64_t n, int64_t rows, float gamma, float* grad,
                     float* partial, float* loss, void* stream);
/* The trainer's loop over the deep-supervision heads (trainer/trainer.py:122-135: criterion on every head, mean over
 * heads) in one pass over the target: loss[1 + h] = FocalLoss_BCE_2d(pred[h], target) exactly as unetpp_focal_bce
 * computes it, loss[0] = (0 + loss[1] + ... + loss[n_heads]) * (1 / n_heads) in that order (float32, what the loop body's
 * tensor arithmetic does), grad[h] = d loss[0] / d pred[h] = (d loss[1 + h] / d pred[h]) * (1 / n_heads) -- the product
 * autograd forms from the same two float32 factors.  1 <= n_heads <= UNETPP_MAX_HEADS; partial[n_heads *
 * unetpp_focal_bce_blocks(n)] is workspace; every pred[h] / grad[h] (grad[h] may be NULL) 16-byte aligned, n elements. */
#define UNETPP_MAX_HEADS 8
typedef struct unetpp_focal_heads {
  const float* pred[UNETPP_MAX_HEADS];
  float* grad[UNETPP_MAX_HEADS];
  int32_t n_heads, reserved;
} unetpp_focal_heads;
int unetpp_focal_bce_heads(const unetpp_focal_heads* heads, const float* target, int64_t n, int64_t rows, float gamma,
                           float* partial, float* loss, void* stream);
/* ---- top-k focal loss: hard-pixel mining per map (added within v12: new entry points only) ----
 * Heads and target are [rows, P] (rows = N*C maps of P = H*W pixels).  Per head and row only the k_eff = min(k, P)
 * elements with the largest |pred - target| (one float32 subtraction; ranked by the bits of its absolute value, so a
 * NaN ranks first) enter the loss; among elements equal to the k-th largest the lowest indices are taken.
 *   loss[1 + h] = sum over the selected elements of head h of the FocalLoss_BCE_2d term / denom,
 *   loss[0]     = (0 + loss[1] + ... + loss[n_heads]) * (1 / n_heads) as unetpp_focal_bce_heads forms it,
 *   grad[h]     = d loss[0] / d pred[h]: unetpp_focal_bce_heads' bits (same denom) on the selected elements, +0.0
 *                 on every other (and on a selected element with pred == target, where those write -0.0); grad[h]
 *                 may be NULL,
 *   kth[h * rows + r] = the k_eff-th largest |pred - target| of that head and row (exact).
 * denom: rows for the sum convention of FocalLoss_BCE_2d, rows * k_eff for the mean over the selected pixels.
 * k >= P is unetpp_focal_bce_heads itself (same bits).  workspace: unetpp_topk_focal_workspace_bytes(n_heads, rows, P)
 * bytes (0 for arguments the call would refuse).  target and every pred[h] / grad[h] 16-byte aligned (rows need not
 * be); 1 <= P < 2^31, 1 <= rows < 2^31, k >= 1, denom >= 1, 1 <= n_heads <= UNETPP_MAX_HEADS. */
int64_t unetpp_topk_focal_workspace_bytes(int32_t n_heads, int64_t rows, int64_t P);
int unetpp_topk_focal_heads(const unetpp_focal_heads* heads, const float* target, int64_t rows, int64_t P, int64_t k,
                            int64_t denom, float gamma, void* workspace, float* kth, float* loss, void* stream);
/* ---- penalty-reduced focal loss, normalised by positives (added within v13: new entry points only) ----
 * The heat-map loss of CornerNet / CenterNet for every head against one target, n float32 elements each.  Per element of
 * a head p (in [0, 1]) and the target t (domain [0, 1]); alpha >= 0, beta >= 0, eps in (0, 0.5), positive in (0, 1]:
 *   lo = float32(eps), hi = float32(1) - lo (one float32 subtraction);  q = min(max(p, lo), hi), a NaN stays a NaN;
 *   the gradient passes where lo <= p <= hi (torch.clamp's rule) and is exactly +0.0 elsewhere;
 *   t >= positive:  l = -(1 - q)^alpha log(q);   otherwise:  l = -(1 - t)^beta q^alpha log(1 - q), the logarithm
 *   evaluated as log1pf(-q);  0^0 = 1;
 *   n_pos[0] = the elements of the target with t >= positive (exact; per call, hence per replica under data parallel),
 *   denom = max(n_pos, 1);  loss[1 + h] = (sum of l over head h) * (1 / denom);
 *   loss[0]  = (0 + loss[1] + ... + loss[n_heads]) * (1 / n_heads) as unetpp_focal_bce_heads forms it;
 *   grad[h]  = d loss[0] / d pred[h] = ((dl / dq) * (1 / denom)) * (1 / n_heads), the float32 products in autograd's
 *              order; grad[h] may be NULL.
 * A NaN in pred makes the loss NaN; the gradient at that element is 0.  A label at a sub-pixel position never produces
 * a target of exactly 1: lower `positive` for such targets.  Three launches (an integer count pass over the target, the
 * main pass, a finish in fixed order), no host synchronisation, no atomics: two runs give the same bits, and the call
 * may be captured in a graph.  workspace: unetpp_pr_focal_workspace_bytes(n_heads, n) bytes (0 for arguments the call
 * would refuse), 8-byte aligned, as is n_pos; target and every pred[h] / grad[h] 16-byte aligned.  UNETPP_EINVAL, without
 * touching the device, for a NULL pointer, n < 1 (or n above 2^42), n_heads outside 1 .. UNETPP_MAX_HEADS, a negative or
 * NaN alpha / beta, eps outside (0, 0.5), positive outside (0, 1], a misaligned pointer. */
int64_t unetpp_pr_focal_workspace_bytes(int32_t n_heads, int64_t n);
int unetpp_pr_focal_heads(const unetpp_focal_heads* heads, const float* target, int64_t n, float alpha, float beta,
                          float eps, float positive, void* workspace, int64_t* n_pos, float* loss /* [1 + n_heads] */,
                          void* stream);
/* ---- ignore regions in the three fused losses (added within v13: new entry points only) ----
 * The signatures, workspaces, refusals and results of unetpp_focal_bce_heads, unetpp_topk_focal_heads and
 * unetpp_pr_focal_heads, with one more rule: an element of the target that is negative is IGNORED.  Ignored iff
 * t < 0.0f as an IEEE comparison: -0.0, +0.0 and a NaN are not, -inf and a negative denormal are.  For every head an
 * ignored element's loss term is +0.0 and its gradient exactly +0.0 (sign bit clear) whatever pred holds, a NaN
 * included; every other element runs the plain call's arithmetic, so on a target without a negative element every
 * output equals the plain call's bit for bit.
 *   top-k:  an ignored element's key is 0: it ranks last and is selected only when k_eff exceeds the number of non-zero
 *           keys of the row, and contributes +0.0 selected or not; k_eff, denom and kth are otherwise as defined above.
 *   penalty-reduced:  a negative target is never >= positive: n_pos is the plain call's.
 * unetpp_target_ignore writes such targets. */
int unetpp_focal_bce_heads_ignore(const unetpp_focal_heads* heads, const float* target, int64_t n, int64_t rows,
                                  float gamma, float* partial, float* loss, void* stream);
int unetpp_topk_focal_heads_ignore(const unetpp_focal_heads* heads, const float* target, int64_t rows, int64_t P,
                                   int64_t k, int64_t denom, float gamma, void* workspace, float* kth, float* loss,
                                   void* stream);
int unetpp_pr_focal_heads_ignore(const unetpp_focal_heads* heads, const float* target, int64_t n, float alpha, float beta,
                                 float eps, float positive, void* workspace, int64_t* n_pos,
                                 float* loss /* [1 + n_heads] */, void* stream);
/* ---- self-distillation across the heads (csrc/distill.hip; added within v13: new entry points only) ----
 * unetpp_focal_bce_heads (ignore = 0) or unetpp_focal_bce_heads_ignore (ignore = 1) with one more term: every head but the
 * deepest is also held, by the same element rule, against a deeper head's map -- its teacher, read as data (no gradient
 * reaches a head through its role as teacher).  Heads pred[0 .. n_heads - 1] are ordered shallow to deep.
 *   teacher:  UNETPP_DISTILL_LAST: the deepest head teaches every other;  UNETPP_DISTILL_NEXT: head h + 1 teaches head h.
 *   S_h = FocalLoss_BCE_2d(pred[h], target): unetpp_focal_bce_heads' loss[1 + h], bit for bit;
 *   D_h = the FocalLoss_BCE_2d sum of pred[h] against its teacher's map q over the ADMITTED elements, same divisor rows:
 *         without gate and ignore rule unetpp_focal_bce(pred[h], q)'s loss, bit for bit;  D of the deepest head = +0.0;
 *   L_h = S_h + w * D_h, one rounded float32 product and one rounded float32 sum, w = weight[0] read on the device;
 *   loss[0] = (0 + L_0 + ... ) * (1 / n_heads) as unetpp_focal_bce_heads forms it;  loss[1 + h] = L_h;
 *   loss[1 + n_heads + h] = S_h;  loss[1 + 2 * n_heads + h] = D_h;   loss holds 1 + 3 * n_heads floats;
 *   grad[h] = g_s + w * g_d on an admitted element (g_s: unetpp_focal_bce_heads' gradient element, g_d: the same rule
 *             against q, both with the factor 1 / n_heads; one rounded product, one rounded sum), g_s itself on an element
 *             that is not admitted and on every element of the deepest head; grad[h] may be NULL.
 * Admitted: gate = 0: every element.  gate = 1: where |q - t| < |p - t|, a float32 comparison of the absolute values of the
 * two float32 differences (false with a NaN on either side).  ignore = 1: an element with t < 0.0f has S term and g_s +0.0,
 * counts as having passed the gate, and is admitted iff distill_ignored = 1.
 * partial: workspace of 2 * n_heads * unetpp_focal_bce_blocks(n) floats.  weight: one float32 on the device, finite and
 * >= 0 (not checked: the call does not read it on the host).  Two launches, no host synchronisation, no atomics: two runs
 * give the same bits, and a captured call follows later changes of weight[0].  UNETPP_EINVAL, without touching the device,
 * for a NULL pointer (grad[h] excepted), n < 1, rows < 1, n_heads outside 1 .. UNETPP_MAX_HEADS, a negative or NaN gamma,
 * a flag outside its values, target or a pred[h] / grad[h] not 16-byte aligned, weight not 4-byte aligned. */
#define UNETPP_DISTILL_LAST 0
#define UNETPP_DISTILL_NEXT 1
int unetpp_distill_heads(const unetpp_focal_heads* heads, const float* target, int64_t n, int64_t rows, float gamma,
                         const float* weight, int32_t teacher, int32_t gate, int32_t ignore, int32_t distill_ignored,
                         float* partial, float* loss /* [1 + 3 * n_heads] */, void* stream);
/* ---- distillation from an external map (csrc/distill.hip; added within v13: new entry points only) ----
 * unetpp_distill_heads with the teacher taken from outside: EVERY head h in 0 .. n_heads - 1, the deepest included, is held
 * against the target and, by the same element rule, against one external map q = teacher -- fp32, n elements in the
 * target's order, read as data (another network's output, a stitched scene map).
 *   S_h, D_h, L_h = S_h + w * D_h, loss[0] and the layout of loss [1 + 3 * n_heads] are unetpp_distill_heads', formed by
 *   the same statements in the same order: S_h is unetpp_focal_bce_heads' (ignore = 1: _ignore's) loss[1 + h] bit for
 *   bit; where every element is admitted D_h is unetpp_focal_bce(pred[h], teacher)'s loss bit for bit; with the deepest
 *   head's own map as teacher, heads 0 .. n_heads - 2 have the bits of unetpp_distill_heads(UNETPP_DISTILL_LAST).
 *   grad[h] = g_s + w * g_d on an admitted element (one rounded product, one rounded sum), g_s itself, with its bits, on
 *             an element that is kept out and where the product w * g_d is a zero (the sum would only turn a g_s of -0.0,
 *             an exact hit of the target, into +0.0): with weight[0] = 0 on finite inputs loss and gradients are
 *             unetpp_focal_bce_heads' bit for bit; grad[h] may be NULL.
 * Admitted: the teacher exists there AND the gate AND the ignore rule.
 *   void:    an element with q < 0.0f has no teacher and is kept out (-0.0 and a NaN are not negative: a NaN teacher element
 *            is admitted and reaches D_h and loss[0]; nothing is hidden).  The -1 that fills a cut window outside its
 *            frame voids the teacher there.
 *   gate = 1: |q - t| < |p - t|, a float32 comparison of the absolute values of the two float32 differences (false with a
 *            NaN on either side).
 *   ignore = 1: an element with t < 0.0f has S term and g_s +0.0, counts as having passed the gate, and is admitted iff
 *            distill_ignored = 1 and the teacher exists there.
 * A thread reads its 8 targets and 8 teacher values once and walks the heads: 2 + 2 * n_heads map-sized streams.
 * partial: workspace of 2 * n_heads * unetpp_focal_bce_blocks(n) floats.  weight: one float32 on the device, finite and
 * >= 0 (not checked: the call does not read it on the host).  Two launches, no host synchronisation, no atomics: two runs
 * give the same bits, and a captured call follows later changes of weight[0] and of the teacher buffer's contents.
 * UNETPP_EINVAL, without touching the device, for every case unetpp_distill_heads refuses (a NULL pointer, grad[h]
 * excepted; n < 1; rows < 1; n_heads outside 1 .. UNETPP_MAX_HEADS; a negative or NaN gamma; a flag outside its values;
 * target or a pred[h] / grad[h] not 16-byte aligned; weight not 4-byte aligned), a NULL teacher and a teacher that is not
 * 16-byte aligned. */
int unetpp_teacher_heads(const unetpp_focal_heads* heads, const float* target, const float* teacher, int64_t n, int64_t rows,
                         float gamma, const float* weight, int32_t gate, int32_t ignore, int32_t distill_ignored,
                         float* partial, float* loss /* [1 + 3 * n_heads] */, void* stream);
/* ---- ensemble head of an eval forward (added within v12: new entry points only, nothing existing changes) ----
 * The output selection the UNet++ authors left as comments in models/unet.py:293-298: the mean of the first n_heads
 * deep-supervision heads, out = (((s_1 + s_2) + ...) + s_n) / (float)n with s_h = 1 / (1 + exp(-(bias_h + x_h . w_h)))
 * per pixel and class, in ONE pass: every feature tensor x_h (NHWC [N,H,W,C]; fp32, or bf16 for the _bf16 entry) is
 * read once, the fp32 NCHW [N,n_cls,H,W] mean is written once, the individual head maps never exist.  No dropout (eval
 * only), fp32 accumulation, fixed summation order.  weight_h [n_cls, C], bias_h [n_cls], fp32.  Returns UNETPP_EINVAL
 * without touching the device for a NULL descriptor / pointer, n_heads outside 1..UNETPP_MAX_HEADS, N/H/W/C < 1,
 * C > 128 or n_cls outside 1..8 (the limits of unetpp_head_fwd). */
typedef struct unetpp_head_src {
  const void* x;        /* NHWC features of this head's node X_0j */
  const float* weight;  /* [n_cls, C] */
  const float* bias;    /* [n_cls] */
} unetpp_head_src;
typedef struct unetpp_heads_mean {
  unetpp_head_src head[UNETPP_MAX_HEADS];
  int32_t n_heads, reserved;
} unetpp_heads_mean;
int unetpp_heads_mean_fwd(const unetpp_heads_mean* heads, int32_t N, int32_t H, int32_t W, int32_t C, int32_t n_cls,
                          float* out_nchw, void* stream);
int unetpp_heads_mean_fwd_bf16(const unetpp_heads_mean* heads, int32_t N, int32_t H, int32_t W, int32_t C,
                               int32_t n_cls, float* out_nchw, void* stream);
/* ---- backward of the ensemble head (added within v13: new entry points only, nothing existing changes) ----
 * `heads` is the descriptor of the forward, d_out_nchw the gradient of its fp32 NCHW [N,n_cls,H,W] mean.  Per pixel, class
 * and head h:  z = bias_h + x_h . w_h,  s = 1 / (1 + exp(-z)),  dl = (d_out * (1.0f / n_heads)) * (s * (1 - s)),
 *   dx_h = W_h^T dl,   dW_h += dl x_h^T,   db_h += dl.
 * The head maps s_h are recomputed from the feature tile the kernel stages for the weight gradient; they are never read
 * from or written to memory.  grads->head[h]: dx (NHWC, the features' storage type) is written, or added to when
 * accumulate != 0; gate_x: after the (optional) accumulate, dx *= (x_h > 0) (unetpp_head_bwd's semantics); partial:
 * unetpp_head_bwd_blocks(N*H*W) rows of [n_cls*C + n_cls], finished by unetpp_sum_partials (no floating-point atomics,
 * fixed order: two runs give the same bits).  Accepts every (C, n_cls, alignment, size) that unetpp_head_bwd (fp32) or
 * unetpp_head_bwd_bf16 (C = 8 * 2^k, 16-byte aligned x and dx, fewer than 2^31 - 1 pixels) accepts for one head, with
 * 1 <= n_heads <= UNETPP_MAX_HEADS and grads->n_heads == heads->n_heads; anything else, a NULL pointer included, returns
 * UNETPP_EINVAL without touching the device. */
typedef struct unetpp_head_grad {
  void* dx;        /* NHWC gradient of this head's features */
  float* partial;  /* unetpp_head_bwd_blocks(N*H*W) rows of [n_cls*C + n_cls] */
  int32_t accumulate, gate_x;
} unetpp_head_grad;
typedef struct unetpp_heads_mean_grad {
  unetpp_head_grad head[UNETPP_MAX_HEADS];
  int32_t n_heads, reserved;
} unetpp_heads_mean_grad;
int unetpp_heads_mean_bwd(const unetpp_heads_mean* heads, const unetpp_heads_mean_grad* grads, const float* d_out_nchw,
                          int32_t N, int32_t H, int32_t W, int32_t C, int32_t n_cls, void* stream);
int unetpp_heads_mean_bwd_bf16(const unetpp_heads_mean* heads, const unetpp_heads_mean_grad* grads,
                               const float* d_out_nchw, int32_t N, int32_t H, int32_t W, int32_t C, int32_t n_cls,
                               void* stream);
/* create_heatmap (tools/misc/helper.py:87-172): key points [N][P][2] as (x, y), P >= 6 -> float32 [N,4,H,W]:
 * ch0 = point 0, ch1 = points 1..3 summed / max, ch2 = point 4, ch3 = points 5..P-1 summed / max, each map
 * exp(-0.5 sqrt(dx^2 + dy^2) / radius) (the reference uses radius 3).  workspace: unetpp_heatmap_workspace_bytes(). */
int64_t unetpp_heatmap_workspace_bytes(int32_t N, int32_t H, int32_t W);
int unetpp_create_heatmap(const float* points, int32_t N, int32_t P, int32_t H, int32_t W, float radius,
                          float* out_nchw, void* workspace, void* stream);

/* ---- layout converters at the network edge ------------------------------------------------ */
int unetpp_nchw_to_nhwc(const float* src, int32_t N, int32_t C, int32_t H, int32_t W, float* dst, void* stream);
int unetpp_nhwc_to_nchw(const float* src, int32_t N, int32_t C, int32_t H, int32_t W, float* dst, void* stream);

/* ---- bf16-storage companions of the UNETPP_GEMM_BF16 launches (BASELINE configs[3]/[4]) -------------
 * Same operations as their fp32 namesakes above, on bf16 NHWC activations (void*: 16-byte aligned, C a multiple of
 * 8; the BatchNorm backward and head kernels want C/8 a power of two); coefficients, partial sums, parameter
 * gradients and the heads' NCHW probabilities / their gradients stay fp32.  The max-pool winner is the first maximum
 * in scan order of the STORED (bf16-rounded) activation.  d_pooled / pool_idx may be NULL (no pooled consumer):
 * otherwise the pooled gradient is routed to the window argmax while d_act is read, in both passes. */
int unetpp_affine_relu_pool_bf16(const void* y, const float* scale, const float* shift, int32_t relu,
                                 int32_t N, int32_t H, int32_t W, int32_t C,
                                 void* act, void* pooled, uint8_t* pool_idx, void* stream);
int64_t unetpp_bn_bwd_blocks_bf16(int64_t pixels, int32_t C);
int unetpp_bn_bwd_reduce_bf16(const void* d_act, const void* y, const float* scale, const float* shift,
                              const float* mean, const float* invstd, const void* d_pooled, const uint8_t* pool_idx,
                              int32_t N, int32_t H, int32_t W, int32_t C, float* partial, void* stream);
int unetpp_bn_bwd_apply_bf16(const void* d_act, const void* y, const float* scale, const float* shift,
                             const float* mean, const float* invstd, const float* gamma, const float* dgamma,
                             const float* dbeta, const void* d_pooled, const uint8_t* pool_idx,
                             int32_t N, int32_t H, int32_t W, int32_t C, void* dy, void* stream);
/* frozen-layer BatchNorm backward on bf16 octets (see unetpp_bn_frozen_bwd): fp32 arithmetic and sums, dy rounded to
 * bf16 once; routing of d_pooled (even H, W) inside the same kernel; C = 8 * 2^k <= 2048, 16-byte aligned tensors */
int64_t unetpp_bn_frozen_bwd_blocks_bf16(int64_t pixels, int32_t C);
int unetpp_bn_frozen_bwd_bf16(const void* d_act, const void* y, const float* scale, const float* shift,
                              const float* mean, const float* invstd, const void* d_pooled, const uint8_t* pool_idx,
                              int32_t N, int32_t H, int32_t W, int32_t C, void* dy, float* partial, void* stream);
int unetpp_head_fwd_bf16(const void* x, const float* weight, const float* bias, int32_t N, int32_t H, int32_t W,
                         int32_t C, int32_t n_cls, float p_drop, uint64_t seed, const uint8_t* mask, const uint64_t* seed_dev,
                         float* out_nchw, void* stream);
/* partial: unetpp_head_bwd_blocks(N*H*W) rows of [n_cls*C + n_cls], finished by unetpp_sum_partials */
int unetpp_head_bwd_bf16(const float* d_out_nchw, const float* out_nchw, const void* x, const float* weight,
                         int32_t N, int32_t H, int32_t W, int32_t C, int32_t n_cls, float p_drop, uint64_t seed,
                         const uint8_t* mask, const uint64_t* seed_dev, void* dx, int32_t accumulate, int32_t gate_x, float* partial,
                         void* stream);

/* is_batchnorm=False in bf16: d_act += d_pooled at the window argmax (unetpp_affine_relu_pool_bf16's pool_idx), then,
 * with gate != NULL, d_act *= (gate > 0) -- the ReLU mask of the node, applied by its last gradient contribution */
int unetpp_maxpool_bwd_bf16(const void* d_pooled, const uint8_t* pool_idx, int32_t N, int32_t H, int32_t W, int32_t C,
                            void* d_act, const void* gate, void* stream);
/* is_deconv=False in bf16 (nn.UpsamplingBilinear2d, models/unet.py:190): x [N,H,W,C] -> y [N,2H,2W,C]; backward in
 * gather form: dx = (accumulate ? dx : 0) + stencil^T(dy), then dx *= (gate > 0) when gate != NULL */
int unetpp_bilinear2x_fwd_bf16(const void* x, int32_t N, int32_t H, int32_t W, int32_t C, void* y, void* stream);
int unetpp_bilinear2x_bwd_bf16(const void* dy, int32_t N, int32_t H, int32_t W, int32_t C, void* dx, int32_t accumulate,
                               const void* gate, void* stream);

/* Input gradient of the network's first convolution (models/unet.py:220, 1..4 input channels) with bf16 activation
 * storage: dy bf16 [N,H,W,COUT] (COUT a multiple of 8, <= 128), weight fp32 in its torch layout [COUT][CIN][3][3],
 * dx fp32 [N,H,W,CIN].  (fp32 storage: unetpp_gemm_fwd with the rotated weights, as for every other layer.) */
int unetpp_first_layer_dgrad_bf16(const void* dy, const float* weight, int32_t N, int32_t H, int32_t W, int32_t CIN,
                                  int32_t COUT, float* dx, void* stream);

/* ---- heat-map side of validation (tools/misc/heatmap.py; SURVEY 8 row f3 -- parity unpinned: the reference needs
 * OpenCV, absent from the build image) ------------------------------------------------------------------------------
 * unetpp_heatmap_pattern: Heatmap.create_heatmap (heatmap.py:203-230).  points [N, P, 2] as (x, y); map m draws the
 * key points map_points[map_begin[m] .. map_begin[m+1]) (device int32 arrays, n_maps + 1 begins); out [N, n_maps, H, W]:
 * float32 sum of exp(-0.5 * distance / radius) in pattern order, divided by the map's maximum. */
int64_t unetpp_heatmap_pattern_workspace_bytes(int32_t N, int32_t n_maps, int32_t H, int32_t W);
int unetpp_heatmap_pattern(const float* points, int32_t N, int32_t P, const int32_t* map_points,
                           const int32_t* map_begin, int32_t n_maps, int32_t H, int32_t W, float radius,
                           float* out_nchw, void* workspace, void* stream);
/* unetpp_keypoints_extract: Heatmap.extract_points_ (heatmap.py:148-200).  heat [maps, H, W]; thr [maps] (device).
 * Stages on one workspace: 0 = mask (values < thr zeroed, 3x3 median > 0) and label initialisation; 1 = `sweeps` rounds
 * of label merging (8-connected components), *changed (device int32, zeroed by the caller) is set while labels still
 * move: repeat until it stays 0; 2 = per-region maximum and selection: points [maps, num, 2] = (x, y) of the first pixel
 * in raster order attaining the maximum of the num brightest regions (ties: raster order of the regions' first
 * pixels), -1 where there are fewer; counts [maps] = regions found (every count is ranked exactly; max_regions only
 * sizes the fast path's buffer).  0, 1.., 2 alone take a region to be a component of the mask.  The reference's own
 * region step (region_segment_, heatmap.py:100-144: distance-transform cores grown back by a watershed, so that blobs
 * which touch are split) goes between: 0; 3 = 3x3 chamfer distance initialised; 4 = `sweeps` relaxation sweeps, repeat
 * until *changed stays 0; 5 = cores (distance > 0.1 * the map's maximum) as labels; 1.. = components of the cores;
 * 6 = markers (core root / background beyond the two-pixel ring / unknown); 7 = `sweeps` pairs of level-0 flood rounds
 * (labels pass between pixels of the same mask value), repeat until *changed stays 0; 9 = one cross round (the
 * watershed's level 255: any labelled 4-neighbour passes its label on, which floods a hole enclosed by a region) and one
 * level-0 round, *changed set when either moved a pixel; alternate 7-until-stable and 9 until a stage 9 leaves *changed
 * at 0 (at most H*W times: each such stage 9 labels a pixel); 8 = region labels; 2.  Stages 7 and 9 leave the current
 * state in the marker buffer.  (Stage 9 was added within ABI version 13: a stage number that was an error before.)
 * Workspace layout (for callers that want the regions themselves, region_segment_'s return value): uint64 best
 * [maps*H*W], uint64 [maps*max_regions*2], then int32 label [maps*H*W] (after stage 8 / the last stage 1: raster index
 * of the region's first pixel, -1 outside), int32 distance [maps*H*W] (16-bit fixed point), int32 marker [maps*H*W]. */
int64_t unetpp_keypoints_workspace_bytes(int32_t maps, int32_t H, int32_t W, int32_t max_regions);
int unetpp_keypoints_extract(int32_t stage, const float* heat, int32_t maps, int32_t H, int32_t W,
                             const float* thr_per_map, int32_t num, int32_t max_regions, int32_t sweeps,
                             void* workspace, int32_t* changed, float* points, int32_t* counts, void* stream);

/* ---- Fused optimizer step (csrc/optim.hip): the reference trainer's AdamW / AdaBound / SGDW
 * (tools/optimizers/{adamw,adabound,sgdw}.py) as one multi-tensor launch per step.  These symbols, the struct and the
 * constants below were added at ABI version 11 without changing anything that was there before: the additions are
 * backward compatible, a caller of the earlier version-11 library sees no difference. ---- */
#define UNETPP_OPTIM_ADAMW 0
#define UNETPP_OPTIM_ADABOUND 1
#define UNETPP_OPTIM_SGDW 2
#define UNETPP_OPTIM_AMS 1          /* flags: amsgrad / amsbound (aux = max_exp_avg_sq) */
#define UNETPP_OPTIM_CAPTURABLE 2   /* flags: step counters live on the device (segment.step), advanced by the launch */
#define UNETPP_OPTIM_HYPER 8        /* doubles per parameter group in the hyper-parameter block: lr, beta1 (SGDW:
                                       momentum), beta2 (SGDW: dampening), eps, weight_decay, AdaBound's final_lr * lr /
                                       base_lr, gamma, and in slot 7 of ROW 0 only (unused in the other rows)
                                       max_norm of unetpp_optim_step_clip: <= 0 = no clipping */
#define UNETPP_OPTIM_H_MAX_NORM 7   /* index of max_norm in row 0 of the hyper-parameter block */
#define UNETPP_OPTIM_SKIP_NONFINITE 4   /* flags of unetpp_optim_step_clip (with _CAPTURABLE only): a non-finite sum of
                                           squared gradients leaves everything but skipped_steps unchanged */

/* One parameter tensor (fp32, contiguous) of the step.  Segments are in chunk order: segment i owns chunks
 * [chunk_begin, chunk_begin + ceil(numel / unetpp_optim_chunk_elems())). */
typedef struct unetpp_optim_segment {
  float* param;
  const float* grad;
  float* exp_avg;       /* AdamW / AdaBound; NULL for SGDW */
  float* exp_avg_sq;    /* AdamW / AdaBound; NULL for SGDW */
  float* aux;           /* max_exp_avg_sq (UNETPP_OPTIM_AMS), momentum_buffer (SGDW, momentum != 0), else NULL */
  float* step;          /* UNETPP_OPTIM_CAPTURABLE: the float32 count of updates before this one; else NULL */
  int64_t numel;
  int64_t chunk_begin;
  int32_t group;        /* row of the hyper-parameter block */
  int32_t vec;          /* 1 when param, grad, exp_avg, exp_avg_sq and aux are all 16-byte aligned */
} unetpp_optim_segment;

/* Elements per chunk of unetpp_optim_step (host only). */
int64_t unetpp_optim_chunk_elems(void);
/* unetpp_optim_step: one update of every segment (device table `segments`, n_segments rows; chunk_segment [n_chunks]:
 * the segment of each chunk).  kind = UNETPP_OPTIM_ADAMW / _ADABOUND / _SGDW; flags = UNETPP_OPTIM_AMS (not with SGDW)
 * | UNETPP_OPTIM_CAPTURABLE.  hyper [groups * UNETPP_OPTIM_HYPER] (device doubles).  Eager: steps [n_segments] (device
 * doubles) is the count of updates INCLUDING this one (SGDW: 1 on the momentum buffer's first update), done = NULL.
 * Capturable: steps = NULL, the count comes from segment.step + 1 and every segment.step is incremented once by the
 * launch; done is a device int32, zero before the first launch, that the launch leaves zero.
 * Negative status without touching the device for a null table, zero segments or chunks, a bad kind or bad flags. */
int unetpp_optim_step(int32_t kind, int32_t flags, const unetpp_optim_segment* segments, int32_t n_segments,
                      const int32_t* chunk_segment, int64_t n_chunks, const double* hyper, const double* steps,
                      int32_t* done, void* stream);
/* unetpp_optim_upload: hipMemcpyAsync host -> device on `stream` (the segment table of a step; with page-locked
 * `host_src` it is a memcpy node when the stream is being captured, and host_src must then outlive the graph). */
int unetpp_optim_upload(void* dst, const void* host_src, int64_t bytes, void* stream);

/* ---- Global gradient norm, clipping and non-finite skip over the optimizer's table (csrc/optim.hip).  Added within ABI
 * version 12 without changing anything that was there before. ---- */
/* What the consuming launch publishes (device memory owned by the caller, stable address; zero it once). */
typedef struct unetpp_clip_state {
  float total_norm;        /* float(sqrt(sum of squares)): the norm BEFORE clipping */
  float coef;              /* c = max_norm / (total_norm + 1e-6f); coef = c > 1 ? 1 : c (NaN norm: NaN; infinite: 0);
                              1 when there is no max_norm */
  int32_t skipped_steps;   /* advanced by one by every skipped unetpp_optim_step_clip */
  int32_t reserved;
} unetpp_clip_state;

/* unetpp_grad_norm: partials [n_chunks] (device doubles) = per chunk the sum of double(grad)^2 in a fixed order; reads
 * segment.grad, numel, chunk_begin and vec only.  The bits depend neither on the grid nor on segment.vec.  The table
 * is unetpp_optim_step's.  UNETPP_EINVAL without touching the device for a null pointer, zero segments or chunks. */
int unetpp_grad_norm(const unetpp_optim_segment* segments, int32_t n_segments, const int32_t* chunk_segment,
                     int64_t n_chunks, double* partials, void* stream);
/* unetpp_optim_step_clip: unetpp_optim_step with every gradient multiplied by coef as it is read (one rounded fp32
 * multiply; segment.grad is not written).  partials: what unetpp_grad_norm left for the SAME table on the same stream;
 * every workgroup sums it in one fixed order (double) before its first chunk and workgroup 0 writes *state.
 * max_norm = float(hyper[UNETPP_OPTIM_H_MAX_NORM]); <= 0: coef = 1.  flags as unetpp_optim_step, plus
 * UNETPP_OPTIM_SKIP_NONFINITE (UNETPP_EINVAL without _CAPTURABLE): when the sum of squares is not finite the launch
 * stores nothing -- parameters, moments, aux, segment.step and done unchanged -- but state->skipped_steps + 1 (and the
 * norm and coefficient).  Argument checks as unetpp_optim_step; partials and state must not be NULL. */
int unetpp_optim_step_clip(int32_t kind, int32_t flags, const unetpp_optim_segment* segments, int32_t n_segments,
                           const int32_t* chunk_segment, int64_t n_chunks, const double* hyper, const double* steps,
                           int32_t* done, const double* partials, unetpp_clip_state* state, void* stream);
/* unetpp_grad_scale: grad[i] = grad[i] * coef in place over the table (segment.grad is written, whatever its const
 * says; nothing is stored when coef == 1), coef from partials and max_norm (> 0, else UNETPP_EINVAL) as above;
 * state->total_norm and state->coef are written, skipped_steps is not touched.  Uses segment.grad, numel, chunk_begin
 * and vec (1: grad is 16-byte aligned) only. */
int unetpp_grad_scale(const unetpp_optim_segment* segments, int32_t n_segments, const int32_t* chunk_segment,
                      int64_t n_chunks, const double* partials, float max_norm, unetpp_clip_state* state, void* stream);

/* ---- Validation matcher (csrc/validate.hip): HeatmapPattern.match_distmin (tools/misc/heatmap.py:57-79, unfinished
 * there) and the landmark loss of the validation loop (trainer/trainer.py:220-221) for every head in one launch.  Added
 * at ABI version 11 without changing anything that was there before. ---- */
#define UNETPP_MATCH_MAX 64   /* most labels per map (pattern list) and most predictions per map */

/* unetpp_match_points: points [heads*N*C, K, 2] (x, y) in peak order, found [heads*N*C] (device int32: the first found[m]
 * points of map m are its predictions), labels [N, S, 2] (x, y), pattern as map_points / map_begin [C + 1] (device int32,
 * as unetpp_heatmap_pattern; every index in 0..S-1, at most UNETPP_MATCH_MAX per map, no index twice).  Per (head, image,
 * map) the labels of the map's list are matched to its predictions greedily by the global minimum of (d, label position,
 * prediction index), d = float64 squared distance of the float32 differences.  Out: matched [heads, N, S, 2] = the
 * prediction assigned to label s or (-1, -1); mask [heads, N, S] = 1 where label s is matched, else 0; loss [heads] =
 * float32(sum of d over the matched labels / (2 * count)) summed in float64 in a fixed order (csrc/validate.hip), NaN
 * when count is 0; count [heads] = matched labels.  One workgroup per head, deterministic.  Negative status without
 * touching the device for a null pointer, a size <= 0 or K > UNETPP_MATCH_MAX. */
int unetpp_match_points(const float* points, const int32_t* found, int32_t heads, int32_t N, int32_t C, int32_t K,
                        const float* labels, int32_t S, const int32_t* map_points, const int32_t* map_begin,
                        float* matched, uint8_t* mask, float* loss, int32_t* count, void* stream);

/* ---- Weight averaging (csrc/average.hip): the reference trainer's "average" save strategy (trainer/trainer.py:243-252,
 * not implemented there) as one multi-tensor launch per update.  Added within ABI version 12 without changing anything
 * that was there before. ---- */
#define UNETPP_AVG_MEAN 0         /* equal-weight running mean (SWA): w = 1 / (n + 1) */
#define UNETPP_AVG_EMA 1          /* exponential moving average: w = 1 - decay */
#define UNETPP_AVG_SWAP 2         /* exchange avg and src element by element */
#define UNETPP_AVG_CAPTURABLE 1   /* flags: the update count and the decay live on the device; the launch advances the count */

/* One tensor (fp32, contiguous) and its average.  avg and src do not overlap.  Segments are in chunk order: segment i
 * owns chunks [chunk_begin, chunk_begin + ceil(numel / unetpp_optim_chunk_elems())). */
typedef struct unetpp_avg_segment {
  float* avg;
  float* src;           /* written by UNETPP_AVG_SWAP only */
  int64_t numel;
  int64_t chunk_begin;
  int32_t vec;          /* 1 when avg and src are both 16-byte aligned */
  int32_t copy;         /* mean / ema: avg = src at every update (a buffer that is carried, not averaged) */
} unetpp_avg_segment;

/* unetpp_avg_update: one launch over every segment (device table `segments`, n_segments rows; chunk_segment [n_chunks]:
 * the segment of each chunk; build and upload them as for unetpp_optim_step).  With n = the number of updates made before
 * this one, UNETPP_AVG_MEAN / _EMA set avg = src bit for bit when n == 0 or segment.copy, else d = src - avg,
 * avg = avg + w * d (each operation rounded once; w formed in double, rounded to float once).  UNETPP_AVG_SWAP exchanges
 * avg and src, copy segments included.
 * Eager (flags 0): n = count (>= 0) and decay (in [0, 1), EMA only) are arguments; count_dev = hyper_dev = done = NULL.
 * UNETPP_AVG_CAPTURABLE (not with SWAP): n = *count_dev (device float32), decay = hyper_dev[0] (device double; may be
 * NULL for MEAN); the launch leaves *count_dev = n + 1; done is a device int32, zero before the first launch, that the
 * launch leaves zero.  count and decay are ignored.  SWAP takes flags 0 and NULL for all three device pointers.
 * UNETPP_EINVAL without touching the device for a null table, zero segments or chunks, an unknown kind or flag, or a
 * pointer combination that does not fit the mode. */
int unetpp_avg_update(int32_t kind, int32_t flags, const unetpp_avg_segment* segments, int32_t n_segments,
                      const int32_t* chunk_segment, int64_t n_chunks, int64_t count, double decay, float* count_dev,
                      const double* hyper_dev, int32_t* done, void* stream);

/* ---- Device-resident input pipeline (csrc/loader.hip): the part of the training loop the reference leaves on the host
 * (DatasetsBase.__getitem__ decodes an image and applies an empty transforms.Compose).  The decoded data set stays on the
 * device; one launch gathers a batch from it, warps it, normalises it and carries the key-point labels through the same
 * transform.  Added within ABI version 12 without changing anything that was there before. ---- */
#define UNETPP_WARP_PARAMS 16     /* floats per sample of the parameter table */
#define UNETPP_WARP_MAX_C 8
#define UNETPP_STORE_U8 0         /* store uint8 [M, Hs, Ws, C]: decoded images, channels last */
#define UNETPP_STORE_F32 1        /* store float32 [M, C, Hs, Ws] */

/* One sample's row of the parameter table, 16 floats.  Coordinates are pixel indices, a pixel centre is an integer
 * (align_corners = True):
 *   [0..5]   inverse map, output pixel -> source position:  xs = m0*xo + m1*yo + m2,  ys = m3*xo + m4*yo + m5
 *   [6..11]  forward map, source position -> output position, same form (labels)
 *   [12]     gain     [13] bias     [14..15] zero
 *
 * unetpp_warp_batch: out[n, c, yo, xo] = gain * (v * mul[c] + add[c]) + bias, out float32 [N, C, Ho, Wo] contiguous, v =
 * the bilinear sample of sample index[n] of the store at (xs, ys): the four neighbours of the position weighted
 * (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy, a neighbour outside the source frame contributing `fill` (source units) -- so v
 * is continuous in the position everywhere, and a map with whole entries copies pixels bit for bit.  Every operation is
 * rounded once (no contraction).  index int64 [N], params float32 [N][16], mul / add float32 [C], all on the device.
 * An index outside [0, M) gives an all-fill sample by the same arithmetic; nothing outside the store is read.
 * labels (may be NULL, then S = 0 and labels_out = inside = NULL): float32 [M, S, 2] as (x, y) -> labels_out [N, S, 2] by
 * the forward map and inside [N, S] uint8 = 1 iff 0 <= x <= Wo-1 and 0 <= y <= Ho-1.  A source label with a negative
 * coordinate (the "none" sentinel (-1, -1)) and every label of an out-of-range index come out (-1, -1) with inside = 0.
 * UNETPP_EINVAL without touching the device for a null pointer, a size <= 0, C > UNETPP_WARP_MAX_C, an image side above
 * 2^24 or an unknown store type. */
int unetpp_warp_batch(const void* store, int32_t store_type, int64_t M, int32_t Hs, int32_t Ws, int32_t C,
                      const int64_t* index, int32_t N, const float* params, const float* mul, const float* add,
                      float fill, float* out, int32_t Ho, int32_t Wo, const float* labels, int32_t S,
                      float* labels_out, uint8_t* inside, void* stream);

/* What unetpp_augment_draw draws from.  The defaults of the Python Augment are the blur-free family: flips, quarter
 * turns and whole-pixel shifts are pixel permutations under the bilinear kernel. */
typedef struct unetpp_augment {
  float p_flip_h, p_flip_v;   /* probability of a flip in x / in y */
  int32_t rot90;              /* non-zero: 0..3 quarter turns, applied as an exact integer matrix */
  float max_deg;              /* rotation in [-max_deg, max_deg] degrees */
  float scale_lo, scale_hi;   /* log-uniform scale, both > 0 */
  float max_tx, max_ty;       /* shift in [-max, max] source pixels, rounded to whole pixels */
  float gain_lo, gain_hi;     /* contrast */
  float max_bias;             /* brightness in [-max_bias, max_bias] */
  int32_t reserved;
} unetpp_augment;

/* unetpp_augment_draw: params [N][16] (device) for N samples, one thread per sample.  Uniform k of sample n is
 * u = (mix64(seed + 0x9E3779B97F4A7C15 * (16 n + k + 1)) >> 40) * 2^-24 (splitmix64's finaliser, as the heads' dropout):
 *   k = 0: flip x iff u < p_flip_h     1: flip y iff u < p_flip_v     2: q = floor(4 u) quarter turns (rot90)
 *   3: theta = (2u - 1) max_deg        4: s = exp(ln lo + u (ln hi - ln lo))
 *   5, 6: tx, ty = floor((2u - 1) max_t + 0.5)     7: gain = lo + u (hi - lo)     8: bias = (2u - 1) max_bias
 * forward  p_o = c_o + D R(theta) Q^q s (p_s - c_s - t),  inverse  p_s = c_s + t + (1/s) Q^-q R(-theta) D (p_o - c_o),
 * c = ((W - 1) / 2, (H - 1) / 2) of the source / output frame, D = diag(+-1, +-1), Q = [[0, -1], [1, 0]].  All in
 * float64, rounded to float32 once.  UNETPP_EINVAL for a null pointer, a size <= 0 or a scale bound <= 0. */
int unetpp_augment_draw(float* params, int32_t N, uint64_t seed, int32_t Hs, int32_t Ws, int32_t Ho, int32_t Wo,
                        const unetpp_augment* augment, void* stream);

/* ---- Scene inference (csrc/scene.hip): a frame far larger than the geometry the kernels are tuned for is cut into
 * overlapping tiles, the tiles run through the eval forward as a batch, and this launch puts each tile's owned interior
 * back into the frame maps -- averaging the dihedral variants of a tile (test-time augmentation) on the way.  The
 * reference has no counterpart (its validation loop feeds whole 256x256 images).  Added within ABI version 12 without
 * changing anything that was there before. ---- */
#define UNETPP_SCENE_MAX_VARIANTS 8
#define UNETPP_SCENE_FLIP_X 1     /* variant code bits: the variant is flip_y(flip_x(transpose(tile))), each step */
#define UNETPP_SCENE_FLIP_Y 2     /* taken only when its bit is set -- tile pixel (y, x) sits at variant pixel (a, b): */
#define UNETPP_SCENE_TRANSPOSE 4  /* (a, b) = (y, x), swapped by TRANSPOSE; then b = Tw-1-b (FLIP_X), a = Th-1-a (FLIP_Y) */

/* One tile of a chunk.  The tile covers frame pixels [oy, oy + Th) x [ox, ox + Tw) and OWNS the half-open rectangle
 * [y_lo, y_hi) x [x_lo, x_hi) (frame coordinates) inside it: only that part of its maps is read, and only that part of
 * the frame is written. */
typedef struct unetpp_scene_rect {
  int32_t frame;               /* index on out's leading axis; negative: a padding tile, skipped */
  int32_t oy, ox;
  int32_t y_lo, y_hi, x_lo, x_hi;
  int32_t reserved;
} unetpp_scene_rect;

/* unetpp_scene_stitch: tiles float32 [n_tiles, K, C, Th, Tw] (device): the head maps of K dihedral variants of every
 * tile, variant k made with code variants[k] (host array of K codes, bits above).  For every owned frame pixel (y, x)
 * of tile t and every class c:  out[frame, c, y, x] = (((v_0 + v_1) + ...) + v_{K-1}) / float(K), v_k = the value of
 * variant k at the pixel (y - oy, x - ox) lands on (the inverse of the variant's transform); K = 1 stores v_0.  The same
 * expression, with a true division, as unetpp_heads_mean_fwd; every operation rounded once.  out float32 [S, C, H, W]
 * (device), offsets into it are 64-bit.  rects / rects_dev: the same n_tiles rows on the host (checked here; they size
 * the grid) and on the device (read by the kernel).  Owned rectangles of one call must not overlap: every owned pixel is
 * written exactly once, by one thread; no atomics, no LDS.
 * UNETPP_EINVAL without touching the device for a null pointer, a size <= 0, K outside 1..8, an unknown variant bit, a
 * transposing variant with Th != Tw, n_tiles or C above 65535, or a live row whose frame is >= S, whose tile leaves the
 * frame, or whose owned rectangle is empty or leaves the tile. */
int unetpp_scene_stitch(const float* tiles, int32_t n_tiles, int32_t K, int32_t C, int32_t Th, int32_t Tw,
                        const int32_t* variants, const unetpp_scene_rect* rects, const unetpp_scene_rect* rects_dev,
                        float* out, int32_t S, int32_t H, int32_t W, void* stream);

/* unetpp_scene_screen (added within ABI version 13: new entry points only): the device-side decision of cascaded scene
 * inference -- which rectangles of a frame map hold anything.  maps float32 [S, C, H, W] (device).  Row t of the table
 * names the half-open rectangle [y_lo, y_hi) x [x_lo, x_hi) of frame `frame` (oy / ox are not used here; the caller has
 * grown and clipped the rectangle already).  Over all C classes and all pixels of the rectangle:
 *   active[t] = any(!(v < threshold))    a value equal to the threshold activates, and so does a NaN (fail safe)
 *   score[t]  = fmax of the values       a NaN is ignored; -inf when every value is NaN
 * A row with frame < 0 is padding: active = 0, score = -inf.  active int32 [n_rects] and score float32 [n_rects] are
 * device arrays.  One launch, one workgroup and one writer per rectangle, no atomics: the result is a pure function of
 * the rectangle's values, the same bits on every run.  Nothing outside a rectangle is read; offsets into maps are 64-bit.
 * rects / rects_dev: host and device copies of the table as for unetpp_scene_stitch -- the host copy is validated, a
 * device row that disagrees with the frame is never followed (it is reported as padding).  A table of nothing but
 * padding rows launches nothing and leaves active and score as they are (UNETPP_OK).
 * UNETPP_EINVAL without touching the device for a null pointer, a size <= 0, a NaN threshold, or a live row whose frame
 * is >= S or whose rectangle is empty or leaves the frame. */
int unetpp_scene_screen(const float* maps, int32_t S, int32_t C, int32_t H, int32_t W, const unetpp_scene_rect* rects,
                        const unetpp_scene_rect* rects_dev, int32_t n_rects, float threshold, int32_t* active,
                        float* score, void* stream);

/* ---- Detection (csrc/detect.hip): from the maps of a scene to a list of points per map, and from such lists to
 * true / false positives against labelled points.  The reference has no counterpart: its extraction returns a fixed
 * number of points per map (tools/misc/heatmap.py:148-200) and its matcher is unfinished.  Added within ABI version 12
 * without changing anything that was there before. ---- */

/* unetpp_peaks_detect: maps float32 [M, H, W] (device) -> the peaks of every map in raster order.  Pixel p is a peak
 * when v_p >= threshold and no other pixel q of the (2 radius + 1)^2 window around p, clipped to the map (there is no
 * padding value), beats it: q beats p when v_q > v_p, or v_q == v_p and q comes earlier in raster order.  Plain
 * comparisons, so a NaN is never a peak and never beats anything; a plateau gives one peak, its first pixel; equal
 * maxima more than `radius` apart (Chebyshev) are both peaks.
 * score [M, cap] = v_p.  xy [M, cap, 2] = (x, y), a pixel centre being an integer: the integer peak, plus -- with
 * refine != 0 -- a per-axis parabola offset computed in float64 from the float32 values a, b, c at x-1, x, x+1:
 * den = (a - 2*b) + c; den < 0: off = (0.5 * (a - c)) / den, limited to [-0.5, 0.5] by comparisons; else (den >= 0 or
 * NaN, or a neighbour beyond the map's edge) off = 0; x_out = float32(double(x) + off), rounded once.  Likewise y.
 * count [M] int32 = the number of peaks of the map, which may exceed cap: the first cap in raster order are kept.  Rows
 * k >= min(count, cap) are xy = -1, score = -inf.  Ranks come from per-workgroup counts and a prefix sum: the order is
 * the raster order on any grid, the same bits on every run, no atomics, no host read-back (three launches on `stream`).
 * workspace: unetpp_peaks_workspace_bytes(M, H, W) bytes on the device, 8-byte aligned (0 for sizes the call refuses).
 * Offsets into the maps and raster indices are 64-bit.
 * UNETPP_EINVAL without touching the device for a null pointer, a size <= 0, radius outside 1..8, cap <= 0, a NaN
 * threshold, H or W >= 2^24 (coordinates are carried in fp32), M > 65535, H * W above 2^42, or a misaligned workspace. */
int64_t unetpp_peaks_workspace_bytes(int32_t M, int32_t H, int32_t W);
int unetpp_peaks_detect(const float* maps, int32_t M, int32_t H, int32_t W, float threshold, int32_t radius,
                        int32_t refine, int32_t cap, float* xy, float* score, int32_t* count, void* workspace,
                        void* stream);

/* unetpp_detect_match: detections against labels, per group g = s * C + c (frame s, class c), G = S * C groups.
 * xy float32 [G, cap, 2]; n_pred int32 [G] (clipped to 0..cap here); order int32 [G, cap]: the first n_pred[g] entries
 * are the slots of group g's predictions in the order they are served (an entry outside 0..cap-1 is skipped).  labels
 * float32 [S, L, 2], label_class int32 [S, L]: label l of frame s belongs to group (s, label_class[s, l]); a class
 * outside 0..C-1 (-1 by convention) is padding.  Each prediction in turn takes the nearest label of its group that no
 * earlier prediction took, d = (double)dx*dx + (double)dy*dy of the float32 differences, provided
 * d <= (double)tolerance * tolerance; ties go to the lowest label index.
 * Out (all written here): pred_label int32 [G, cap] = the label index or -1; label_pred int32 [S, L] = the slot of the
 * matched prediction or -1; stats int32 [G, 3] = true positives, false positives (served and unmatched), false
 * negatives (labels of the group left over).  One workgroup per group, integer bookkeeping, deterministic.
 * UNETPP_EINVAL without touching the device for a null pointer, a size <= 0, S * C above 2^31 - 1, or a negative or NaN
 * tolerance. */
int unetpp_detect_match(const float* xy, const int32_t* n_pred, const int32_t* order, int32_t S, int32_t C, int32_t cap,
                        const float* labels, const int32_t* label_class, int32_t L, float tolerance, int32_t* pred_label,
                        int32_t* label_pred, int32_t* stats, void* stream);

/* ---- Training on scenes (csrc/crops.hip): windows drawn where the objects are, and the target maps of such windows from
 * label lists of any length.  The reference has no counterpart: its targets come from a fixed pattern of points per
 * image (tools/misc/heatmap.py:203-230).  Added within ABI version 12 without changing anything that was there
 * before. ---- */

/* unetpp_points_target: out float32 [N, C, Ho, Wo] (device) = the target maps of N warped windows.  labels float32
 * [M, L, 2] as (x, y), label_class int32 [M, L], index int64 [N], params float32 [N][16] (the rows of unetpp_warp_batch).
 * Label l of sample n is valid when index[n] lies in [0, M), its class lies in 0..C-1 and neither source coordinate is
 * negative (!(x < 0) && !(y < 0), the loader's sentinel test).  Its position in the window is the forward map in the
 * warp's own float32 expression, xo = (P[0]*x + P[1]*y) + P[2], yo = (P[3]*x + P[4]*y) + P[5], P = params[n] + 6 -- the
 * labels_out of unetpp_warp_batch.  Every valid label of the frame counts, inside the window or not.
 *   m = min over the valid labels of class c of dx*dx + dy*dy,  dx = (double)x - (double)xo,  dy likewise
 *   out[n, c, y, x] = (float)exp(-0.5 * sqrt(m) / (double)radius),  exactly 0 where class c has no valid label.
 * The search is exact: a workgroup keeps, per pixel tile and class, the labels whose least squared distance to the tile
 * does not exceed the least over the labels of the greatest one, and takes the minimum over those (csrc/crops.hip).
 * No atomics, no contraction, 64-bit offsets into out; the same bits on any grid and on every run.
 * UNETPP_EINVAL without touching the device for a null pointer, a size <= 0, C > 65535, a window side above 2^24, or a
 * radius that is not > 0 (a NaN included). */
int unetpp_points_target(const float* labels, const int32_t* label_class, int64_t M, int32_t L, const int64_t* index,
                         int32_t N, const float* params, int32_t C, int32_t Ho, int32_t Wo, float radius, float* out,
                         void* stream);

/* unetpp_target_ignore (added within v13): marks the ignored elements of target float32 [N, C, Ho, Wo] (device) with
 * exactly -1.0f, the sentinel of the *_ignore losses.  rects float32 [M, R, 4] as (x0, y0, x1, y1) in source-frame pixel
 * coordinates, both ends inclusive; rect_class int32 [M, R]: -1 applies to every class, c in 0..C-1 to class c, any other
 * value is padding, as is a row with x1 < x0, y1 < y0 or a NaN.  index, params: the rows of unetpp_warp_batch; Hs x Ws:
 * the frames' size.  The source position of window pixel (x, y) of sample n is the warp's own float32 expression,
 * xs = (P[0]*x + P[1]*y) + P[2], ys = (P[3]*x + P[4]*y) + P[5], P = params[n], no contraction.  target[n, c, y, x] is
 * set when
 *   index[n] lies in [0, M) and x0 <= xs && xs <= x1 && y0 <= ys && ys <= y1 (float32 comparisons: a NaN is never
 *   inside) for a rectangle of frame index[n] whose class is -1 or c, or
 *   outside != 0 and !(0 <= xs && xs <= Ws-1 && 0 <= ys && ys <= Hs-1): a bilinear neighbour of non-zero weight is
 *   the fill value, or the position is a NaN; every class, and every element of an all-fill sample (index[n] outside
 *   [0, M)).
 * Every other element is left untouched, not even read: ignoring wins over a label.  Stores of one constant: no atomics,
 * the same bits on any grid; 64-bit offsets into target.  R may be 0 (rects and rect_class then unread; with
 * outside == 0 the call does nothing).  UNETPP_EINVAL without touching the device for a null pointer, a size <= 0 (R < 0),
 * C > 65535 or a side above 2^24. */
int unetpp_target_ignore(const float* rects, const int32_t* rect_class, int64_t M, int32_t R, const int64_t* index,
                         int32_t N, const float* params, int32_t C, int32_t Ho, int32_t Wo, int32_t Hs, int32_t Ws,
                         int32_t outside, float* target, void* stream);

/* ---- Ignore masks (csrc/mask.hip; added within ABI version 13: new entry points only): a second producer of the same
 * -1 elements, for outlines that are not rectangles -- raster no-data masks and polygon rings.
 *
 * A mask is packed bit planes: bits int32 [S, P, H, Wd] (device), Wd = ceil(W / 32); bit (x & 31) of word (x >> 5) of
 * row y is pixel (x, y), the unused high bits of a row's last word are zero.  plane_class int32 [P]: -1 applies the
 * plane to every class, c in 0..C-1 to class c, any other value to none -- the meanings of rect_class.
 *
 * The lookup rule (unetpp_target_ignore_mask; IgnoreMask.contains restates it): a float32 position (xs, ys) is in the
 * frame iff 0 <= xs && xs <= W-1 && 0 <= ys && ys <= H-1 (a NaN is outside); its pixel is xi = clamp((int)floorf(xs +
 * 0.5f), 0, W-1), yi likewise; it is ignored for class c iff some plane of class -1 or c has that bit set.  Outside the
 * frame nothing is contained.
 *
 * The polygon rule (unetpp_mask_polygons): a pixel is its centre, the integer point (px, py).  For each used edge of a
 * ring, the closing edge included, the endpoints are ordered so that y0 <= y1; an edge with y0 == y1 is skipped.  The
 * edge straddles iff y0 <= py && py < y1, and then toggles the pixel iff d > 0,
 *   d = (x1 - x0) * (py - y0) - (px - x0) * (y1 - y0)      in float64, this order, every operation rounded on its own.
 * The pixel is inside the ring iff the number of toggles is odd.  Two rings that share an edge form the same d, so a
 * pixel on the shared edge belongs to exactly one of them.  The rings of a plane are walked in list order: an inside
 * pixel is set by a plain ring and cleared by a clearing ring. ---- */
#define UNETPP_MASK_U8 0    /* unetpp_mask_pack kinds: one byte per pixel (uint8 or bool) */
#define UNETPP_MASK_F32 1   /* float32 per pixel */

/* unetpp_mask_pack: bits of `rows` rows of W pixels from a raster of `kind`: mask [rows, W] (device, contiguous), bits
 * int32 [rows, ceil(W / 32)].  A pixel's bit is set iff !(v == 0): a NaN sets it, -0.0 does not.  A wave packs 64
 * consecutive x of a row by one ballot into two words stored separately (no alignment demanded of a row); tail bits
 * are zero; one writer per word, no atomics.  UNETPP_EINVAL without touching the device for a null pointer, a size
 * <= 0, W above 2^24, an unknown kind, or rows * W above 2^31 - 1. */
int unetpp_mask_pack(const void* mask, int32_t kind, int64_t rows, int32_t W, int32_t* bits, void* stream);

/* unetpp_mask_polygons: rasterises rings into bits int32 [S, P, H, ceil(W / 32)] by the polygon rule; EVERY word is
 * written (zero where no ring sets a bit).  vertices float32 [S, G, V, 2] as (x, y); counts int32 [S, G], the vertices
 * used per ring -- a ring with a count outside 3..V or with a NaN / infinity in a used vertex is padding; poly_plane
 * int32 [S, G], the plane a ring writes (outside 0..P-1: padding); poly_clear int32 [S, G], non-zero: a clearing ring.
 * G may be 0 (the lists are then unread).  A unit is (frame, plane, 16 rows x 64 pixels); the rings whose float
 * bounding box can matter to the tile are compacted in list order with wave ballots, their edges stream through LDS
 * 256 at a time; the culling drops a ring only where no pixel of the tile can be inside it, so it changes no bit.  No
 * atomics; the same bits on any grid and on every run.  UNETPP_EINVAL without touching the device for a null pointer, a
 * size <= 0 (G, V < 0), a side above 2^24, or a word or vertex count above 2^31 - 1. */
int unetpp_mask_polygons(const float* vertices, const int32_t* counts, const int32_t* poly_plane,
                         const int32_t* poly_clear, int32_t S, int32_t G, int32_t V, int32_t P, int32_t H, int32_t W,
                         int32_t* bits, void* stream);

/* unetpp_target_ignore_mask: unetpp_target_ignore with the frame's rectangles replaced by the P bit planes of frame
 * index[n] (bits int32 [M, P, Hs, ceil(Ws / 32)], plane_class int32 [P]): target[n, c, y, x] = -1.0f when the source
 * position of (x, y) -- the same float32 expression -- is ignored for class c by the lookup rule, or when outside != 0
 * and it lies outside the frame or index[n] outside [0, M).  Everything else is left untouched, not even read.  The
 * cost per pixel is one word load per plane, whatever the outline.  P may be 0 (bits and plane_class then unread: the
 * `outside` rule alone; with outside == 0 the call does nothing).  Stores of one constant, no atomics, the same bits on
 * any grid; 64-bit offsets.  UNETPP_EINVAL without touching the device for a null pointer, a size <= 0 (P < 0),
 * C > 65535, a side above 2^24, or a frame of more than 2^31 - 1 words. */
int unetpp_target_ignore_mask(const int32_t* bits, const int32_t* plane_class, int64_t M, int32_t P, int32_t Hs,
                              int32_t Ws, const int64_t* index, int32_t N, const float* params, int32_t C, int32_t Ho,
                              int32_t Wo, int32_t outside, float* target, void* stream);

/* unetpp_crops_draw: N windows of Ho x Wo pixels in M frames of Hs x Ws, one thread per sample: params [N][16], index
 * int64 [N] (the frame), origin int32 [N, 2] as (ox, oy), all on the device.  Uniforms u_k and the meaning of
 * k = 0, 1, 2, 3, 4, 7, 8 are unetpp_augment_draw's; k = 5, 6 are unused (max_tx and max_ty must be 0).  centre_frame
 * int32 [V], centre_xy float32 [V, 2] (device; V may be 0, the tables then unread):
 *   k = 9:   an object window iff V > 0 and u < p_object, a uniform window otherwise
 *   k = 10:  object: j = min(floor(u V), V - 1), frame = centre_frame[j], (cx, cy) = floor(centre_xy[j] + 0.5)
 *            uniform: frame = min(floor(u M), M - 1)
 *   k = 11:  object: cx += floor((2u - 1) jitter_x + 0.5)      uniform: cx = min(floor(u Ws), Ws - 1)
 *   k = 12:  object: cy += floor((2u - 1) jitter_y + 0.5)      uniform: cy = min(floor(u Hs), Hs - 1)
 * ox = cx - Wo / 2 limited to [0, Ws - Wo] when Ws >= Wo, else -((Wo - Ws) / 2), a centred pad (whole-number
 * divisions); oy likewise.  The row is unetpp_augment_draw's forward / inverse pair with c_s + t replaced by the
 * window's centre (ox + (Wo - 1) / 2, oy + (Ho - 1) / 2): with no rotation and unit scale every entry is a whole number.
 * A table row whose frame lies outside [0, M) gives index = -1, the all-fill sample of unetpp_warp_batch, for which
 * unetpp_points_target writes zeros.
 * UNETPP_EINVAL for a null pointer (the tables when V > 0), a size <= 0, V < 0, a side above 2^24, a scale bound <= 0,
 * a non-zero max_tx or max_ty, quarter turns with Ho != Wo, or a negative or NaN p_object or jitter. */
int unetpp_crops_draw(float* params, int64_t* index, int32_t* origin, int32_t N, uint64_t seed, int32_t M, int32_t Hs,
                      int32_t Ws, int32_t Ho, int32_t Wo, const int32_t* centre_frame, const float* centre_xy, int32_t V,
                      float p_object, float jitter_x, float jitter_y, const unetpp_augment* augment, void* stream);

/* ---- Copy-paste augmentation of tiny objects (csrc/paste.hip; added within v13): an object's few pixels are copied to
 * new places of a window, with their label.  Three launches between those above: unetpp_crops_draw, unetpp_warp_batch,
 * unetpp_paste_draw, unetpp_paste_apply, unetpp_points_target, unetpp_paste_target, unetpp_target_ignore.  The reference
 * has no counterpart.
 *
 * The source table: src_frame int32 [T], src_xy float32 [T, 2] as (x, y), src_class int32 [T] (device).  Row t can be
 * pasted when its frame lies in [0, M), its class in [0, C) and the patch of (2R+1) x (2R+1) whole pixels about its
 * rounded centre (cx, cy) = floor(src_xy + 0.5) lies inside the Hs x Ws frame: R <= cx <= Ws-1-R, R <= cy <= Hs-1-R,
 * compared as doubles, so a NaN or an infinity is not inside.  Both kernels that read the table test this themselves.
 *
 * A code 0..7 is one of the eight flips and quarter turns: q = code & 3 quarter turns, then a flip in x when code & 4,
 * T_code = D Q^q, Q^q = [[qc, -qs], [qs, qc]] with (qc, qs) = (1, 0), (0, 1), (-1, 0), (0, -1) as in unetpp_crops_draw,
 * D = diag(-1, 1) with the flip.  Source offset (i, j) from (cx, cy) lands at destination offset T_code (i, j):
 *   T_code (i, j) = (dx (qc i - qs j), qs i + qc j),   T_code^-1 (i, j) = (qc (dx i) + qs j, qc j - qs (dx i)). ---- */
#define UNETPP_PASTE_MAX_SLOTS 64    /* K, the paste slots of a window */
#define UNETPP_PASTE_MAX_RADIUS 16   /* R, the patch radius */

/* unetpp_paste_draw: what is pasted where, one workgroup per window, slots k = 0 .. K-1 in order.  Outputs (device):
 * src int32 [N, K] (the table row, or -1: the slot is void), dst int32 [N, K, 2] as (px, py), code int32 [N, K],
 * xy float32 [N, K, 2] (the pasted label; (-1, -1) when void), cls int32 [N, K] (the source class; -1 when void).
 * labels, label_class, M, L, index, params: as unetpp_points_target takes them; Hs x Ws: the frames, Ho x Wo: the window.
 * Uniform j of slot k of window n is 24 bits wide,
 *   u_j = float32(mix64(seed + 0x9E3779B97F4A7C15 * ((n * 64 + k) * 8 + j + 1)) >> 40) * 2^-24
 * (mix64: the splitmix64 finaliser of unetpp_augment_draw; 64 = UNETPP_PASTE_MAX_SLOTS whatever K is), and
 *   j = 0:  the slot attempts a paste iff (float)u < p
 *   j = 1:  t = min(floor(u T), T - 1), the source row
 *   j = 2:  code = floor(8 u), or 0 when dihedral == 0
 *   j = 3:  px = R + min(floor(u (Wo - 2R)), Wo - 2R - 1)        j = 4:  py likewise with Ho
 * so the patch is inside the window.  dst and code are written as drawn, void or not.  The slot is void when it does not
 * attempt, when index[n] lies outside [0, M), when row t cannot be pasted (above), when a label of frame index[n] with
 * class >= 0 and neither coordinate negative, at its window position (xo, yo) in the float32 expression of
 * unetpp_points_target, has dx*dx + dy*dy < clearance*clearance in float64 (dx = (double)xo - px), or when an earlier
 * slot k' < k of the window that was accepted has max(|px - px'|, |py - py'|) <= 2R: accepted patches are pairwise
 * disjoint.  The label of an accepted slot is xy = dst + T_code (src_xy[t] - floor(src_xy[t] + 0.5)), formed in float64
 * (the difference is exact) and rounded once.  No atomics; the same bits on any grid.
 * UNETPP_EINVAL without touching the device for a null pointer, a size <= 0, K > UNETPP_PASTE_MAX_SLOTS, C > 65535, a side
 * above 2^24, R outside 0..UNETPP_PASTE_MAX_RADIUS, a window side below 2R + 1, or a negative or NaN p or clearance. */
int unetpp_paste_draw(int32_t* src, int32_t* dst, int32_t* code, float* xy, int32_t* cls, int32_t N, int32_t K,
                      uint64_t seed, const int32_t* src_frame, const float* src_xy, const int32_t* src_class, int32_t T,
                      const float* labels, const int32_t* label_class, int64_t M, int32_t L, const int64_t* index,
                      const float* params, int32_t C, int32_t Hs, int32_t Ws, int32_t Ho, int32_t Wo, float p, int32_t R,
                      float clearance, int32_t dihedral, void* stream);

/* unetpp_paste_apply: the pixels, in place on inputs float32 [N, Cin, Ho, Wo] (device); a unit of work is (n, k).  src,
 * dst, code: rows as unetpp_paste_draw writes them, but any values are safe: a row is skipped unless src lies in [0, T),
 * the table row can be pasted (above), code lies in 0..7 and R <= px <= Wo-1-R, R <= py <= Ho-1-R; no address outside
 * the store or inputs is formed.  store, store_type, M, Hs, Ws, mul, add: as unetpp_warp_batch takes them (Cin channels);
 * params [N][16]: entries 12 and 13 of row n are the window's gain and bias; alpha float32 [2R+1][2R+1]: the blend
 * weights, indexed [j + R][i + R], symmetric under the eight codes.  For every offset (i, j) in [-R, R]^2 and channel c:
 *   v   = the store's pixel at (cx, cy) + T_code^-1 (i, j) of frame src_frame[t], channel c
 *   p   = gain * (v * mul[c] + add[c]) + bias                      (the expression of unetpp_warp_batch, float32)
 *   d   = inputs[n, c, py + j, px + i]
 *   out = alpha == 1 ? p : alpha == 0 ? d : d + alpha * (p - d)    (float32, no contraction)
 * The patches of a window must be pairwise disjoint (unetpp_paste_draw makes them so): units are then independent and
 * the result is the same in any order and on any grid.  No atomics; 64-bit offsets.
 * UNETPP_EINVAL without touching the device for a null pointer, a size <= 0, K > UNETPP_PASTE_MAX_SLOTS, Cin >
 * UNETPP_WARP_MAX_C, C > 65535, a side above 2^24, R outside 0..UNETPP_PASTE_MAX_RADIUS or an unknown store_type. */
int unetpp_paste_apply(float* inputs, int32_t N, int32_t K, int32_t Cin, int32_t Ho, int32_t Wo, const int32_t* src,
                       const int32_t* dst, const int32_t* code, const int32_t* src_frame, const float* src_xy,
                       const int32_t* src_class, int32_t T, const void* store, int32_t store_type, int64_t M, int32_t Hs,
                       int32_t Ws, int32_t C, const float* params, const float* mul, const float* add,
                       const float* alpha, int32_t R, void* stream);

/* unetpp_paste_target: folds the pasted labels into target float32 [N, C, Ho, Wo] (device), in place, after
 * unetpp_points_target: the target is a maximum over labels, so the result is what that call would have written had the
 * pasted labels been in the frame's list.  xy float32 [N, K, 2], cls int32 [N, K]: of unetpp_paste_draw; slot k of window
 * n is live when cls lies in [0, C).  A window without a live slot is skipped, nothing of it read or written.  Otherwise,
 * per class c that has a live slot and per pixel (x, y):
 *   m = min over the live slots of class c of dx*dx + dy*dy,  dx = (double)x - (double)xy[0],  dy likewise
 *   v = (float)exp(-0.5 * sqrt(m) / (double)radius)
 *   target[n, c, y, x] = v  where v > t and !(t < 0), t the value there: an ignored (negative) element stays.
 * The tiles of unetpp_target_ignore; the K rows of a window pass through LDS once per unit.  No atomics, no contraction,
 * 64-bit offsets; a pure function of target and the rows per element: the same bits on any grid.
 * UNETPP_EINVAL without touching the device for a null pointer, a size <= 0, K > UNETPP_PASTE_MAX_SLOTS, C > 65535, a
 * window side above 2^24, or a radius that is not > 0 (a NaN included). */
int unetpp_paste_target(float* target, int32_t N, int32_t K, int32_t C, int32_t Ho, int32_t Wo, const float* xy,
                        const int32_t* cls, float radius, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNETPP_HIP_H */
