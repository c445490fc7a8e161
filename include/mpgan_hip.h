/*
 * mpgan_hip.h -- C ABI of libmpgan_hip.so, the MI355X (gfx950) hot path of the
 * T1->T2 GAN training step.
 *
 * The reference (mbrzus/Cross-Modality-Minipig-Gan) has no FFI of its own: the
 * hot path is reached through torch.nn modules.  Each entry point below names
 * the reference call site whose ATen/cuDNN work it replaces
 * (paths relative to the reference repo; "MONAI" = monai==0.4.0, un-vendored,
 * called from code/GAN/GAN_final.py:106-114).
 *
 * Conventions
 *   - Activations are channels-last (N, D, H, W, C) fp32 with an explicit
 *     channel pitch `ld*` (elements between consecutive pixels), so a tensor
 *     may be a channel slice of a wider buffer (concat elision).  2-D tensors
 *     use D = 1 and kernel/stride/pad 1/1/0 in the depth dimension.
 *   - Conv weights are consumed in packed "OTI" order [Cout][tap][Cin]
 *     (tap = (kz*Ky+ky)*Kx+kx), produced by mpgan_pack_weights from the
 *     torch-layout parameters.
 *   - The caller (PyTorch) owns every buffer.  The library never allocates or
 *     frees device memory and keeps no pointer after return.  All calls are
 *     asynchronous on `stream` (a hipStream_t passed as void*).
 *   - Return value: 0 on success, negative on error; mpgan_last_error() returns
 *     a thread-local message.  Unsupported shapes are errors, never fallbacks.
 */
#ifndef MPGAN_HIP_H
#define MPGAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPGAN_OK 0
#define MPGAN_ERR_INVALID -1
#define MPGAN_ERR_UNSUPPORTED -2
#define MPGAN_ERR_HIP -3

#define MPGAN_ACT_NONE 0
#define MPGAN_ACT_LEAKY 1 /* x>0 ? x : slope*x ; PReLU (one shared alpha) and LeakyReLU(0.2) */

const char* mpgan_last_error(void);
int mpgan_abi_version(void);

/* Geometry of one convolution as the reference's nn.ConvNd / nn.ConvTransposeNd
 * describe it.  For a transposed conv, `in` is the (small) input and `out` the
 * up-sampled output: out = (in-1)*stride - 2*pad + k + out_pad. */
typedef struct {
  int32_t n;                 /* batch */
  int32_t in_dhw[3];         /* input  spatial (D,H,W) */
  int32_t out_dhw[3];        /* output spatial (D,H,W) */
  int32_t cin, cout;
  int32_t k[3];              /* kernel (kz,ky,kx) */
  int32_t stride[3];         /* per-dimension stride (1 in an unused depth dim) */
  int32_t pad[3];
  int32_t transposed;        /* 0: ConvNd, 1: ConvTransposeNd */
  int32_t flags;             /* MPGAN_CONV_* bits below; 0 = the reference's fp32 arithmetic */
  int32_t min_blocks;        /* launch size (in blocks) from which the big-tile forms serve this conv (the DMA-staged fp32
                              * form, the wide bf16 forms); 0 = the library's default (1024).  It travels WITH the
                              * geometry, so a sizing query (mpgan_conv_stats_rows*, mpgan_conv_variant*) and the launch
                              * it sizes cannot disagree; the library keeps no mutable dispatch state. */
} mpgan_conv_geom;

/* flags: matrix operands of this conv are rounded to bf16 on their way into LDS and contracted on the bf16 matrix
 * cores with fp32 accumulation (16x the fp32 matrix rate); tensors in HBM, the prologue's arithmetic, bias,
 * residual and statistics stay fp32.  Honoured by the MFMA kernels (K-stepped and 3-D patch forms, forward /
 * backward-data / backward-weight); the thin VALU kernels of 1-channel layers ignore it.  Statistics-row counts and
 * workspace sizes do not depend on it.  Config C5's generator (BASELINE.json: "3D 128^3 ... bf16"). */
#define MPGAN_CONV_MM_BF16 1

/* Optional "normalise + activate on load" prologue applied to the operand that
 * is a raw (pre-norm) conv output: a = act(z*scale[c] + shift[c]).
 * scale/shift may be per channel (n_stride = 0, BatchNorm) or per (n, c)
 * (n_stride = C, InstanceNorm).  slope_ptr (device, 1 float) overrides slope
 * when non-null (PReLU's learnable alpha). */
typedef struct {
  const float* scale;        /* null => no prologue */
  const float* shift;
  int32_t n_stride;
  int32_t act;
  float slope;
  const float* slope_ptr;
} mpgan_prologue;

/* ---- convolution blocks ------------------------------------------------- */

/* y = conv(prologue(x)) [+ bias] [+ resid] [tanh]   (forward of ConvNd, or of
 * ConvTransposeNd when g->transposed).
 * Replaces: conv3d/conv_transpose3d dispatched by MONAI Convolution /
 * ResidualUnit (GAN_final.py:106-114) and by Discriminator.model_conv
 * (GAN_final.py:167-189, test_runs/GAN.py:142-173).
 * stats_partials (nullable): fused BatchNorm statistics -- the kernel also leaves
 * per-tile partial sums [rows][2][Cout] of (y, y^2), rows = mpgan_conv_stats_rows(),
 * which mpgan_norm_finalize(n=1, chunks=rows, pixels=N*D*H*W, instance=0) consumes;
 * rows == 0 means this geometry has no fused statistics (use mpgan_channel_stats). */
int32_t mpgan_conv_stats_rows(const mpgan_conv_geom* g, int32_t has_prologue);
int mpgan_conv_forward(const mpgan_conv_geom* g, const float* x, int32_t ldx,
                       const float* w_packed, const float* bias,
                       const mpgan_prologue* pro,
                       const float* resid, int32_t ldr, int32_t tanh_out,
                       float* stats_partials,
                       float* y, int32_t ldy, void* stream);

/* The same forward with the K axis split over blocks, for output grids too small to fill
 * the chip (variant B's Linear(512*8^3 -> 64) expressed as a conv whose kernel spans the
 * 8^3 grid, test_runs/GAN.py:176-181).  workspace >= mpgan_conv_splitk_workspace() bytes
 * (0 = no split needed: plain forward is used). */
int64_t mpgan_conv_splitk_workspace(const mpgan_conv_geom* g);
int mpgan_conv_forward_splitk(const mpgan_conv_geom* g, const float* x, int32_t ldx,
                              const float* w_packed, const float* bias, const mpgan_prologue* pro,
                              void* workspace, int64_t workspace_bytes, float* y, int32_t ldy, void* stream);

/* dx = conv_backward_data(dy) [+ resid]: gradient w.r.t. the conv input
 * (for g->transposed: gradient w.r.t. the transposed conv's input).
 * `w_packed_bwd` is the packed weight for the backward direction
 * (mpgan_pack_weights with for_dgrad=1).
 * Replaces: the autograd conv backward-data kernels behind loss.backward()
 * (GAN_final.py:273,296 via Lightning's loop). */
int mpgan_conv_backward_data(const mpgan_conv_geom* g, const float* dy, int32_t lddy,
                             const float* w_packed_bwd,
                             const float* resid, int32_t ldr,
                             float* dx, int32_t lddx, void* stream);

/* Backward-data AND the reduce pass of the norm layer in front of the conv's input, in one launch: dx is the
 * gradient w.r.t. a = act(scale*z + shift); partials[rows][3][Cin] receive, per tile, the sums
 * mpgan_norm_bwd_reduce would form by re-reading dx and z (sum gy, sum gy*zhat, sum g*min(y,0)); feed them to
 * mpgan_norm_bwd_finalize with n = 1, chunks = rows.  BatchNorm only (scale/shift/mean/invstd: Cin values).
 * mpgan_conv_bwd_stats_rows: rows the launch leaves; 0 = this geometry is served by a thin or patch kernel
 * without fused sums.
 * Replaces: the autograd backward of `Conv -> BatchNorm -> LeakyReLU` chains of the discriminator
 * (GAN_final.py:167-189 under loss.backward(), :273,296). */
int32_t mpgan_conv_bwd_stats_rows(const mpgan_conv_geom* g);
int mpgan_conv_backward_data_stats(const mpgan_conv_geom* g, const float* dy, int32_t lddy,
                                   const float* w_packed_bwd, float* dx, int32_t lddx,
                                   const float* z, int32_t ldz, const float* scale, const float* shift,
                                   const float* mean, const float* invstd, int32_t act, float slope,
                                   float* partials, void* stream);

/* Which kernel serves this geometry (for profiling labels): 1 = thin Cin==1 VALU
 * stencil, 2 = thin Cout==1 VALU stencil, 16 = fp32-MFMA patch kernel (2-D, <= 32
 * output channels, input patch + weights staged once in LDS; 17 = its merged form, one block per
 * tile walking every phase of a strided backward-data / transposed conv), 18 = the 3-D patch kernel
 * (16 -> 16 channels, 3x3x3, stride 1: 2x8x8 output tiles, 16x16x4 MFMA), 32/64/128 = fp32-MFMA
 * K-stepped implicit GEMM with that output-channel tile.
 * 1128 = the 128 tile's mask-free instance (pad-free forward conv, Cout % 128 == 0, has_prologue 3).
 * 2032 / 2064 = the 32 / 64 tile with the K axis split over two 4-wave groups inside the block (output grids
 * of about one block per CU: the U-Net's 32 x 32 levels).
 * has_prologue: 0 none, 1 per-channel scale/shift, 2 per-(sample, channel), 3 per-channel +
 * LeakyReLU with a host-known slope in [0, 1]. */
int32_t mpgan_conv_variant(const mpgan_conv_geom* g, int32_t backward_data, int32_t has_prologue);
/* The profiling label of that launch: rocprofv3's name of the kernel instance it runs, without `void mpgan::` and the
 * argument list, written NUL-terminated into buf[len].  pro_code is has_prologue's encoding.  Formatted from the same
 * choice the launch makes (choose_gather, conv_igemm.hip); MPGAN_ERR_INVALID if the name needs more than len bytes. */
int mpgan_conv_kernel_name(const mpgan_conv_geom* g, int32_t backward_data, int32_t pro_code, char* buf, int32_t len);

/* Weight gradient: dW (torch layout, (Cout,Cin,k..) or (Cin,Cout,k..) for a
 * transposed conv) = beta*dW + sum over pixels.  x is the conv's input (with
 * optional prologue), dy the gradient of its raw output.  `workspace` holds
 * the split-K partial slabs (size from mpgan_conv_wgrad_workspace). */
int64_t mpgan_conv_wgrad_workspace(const mpgan_conv_geom* g);
int mpgan_conv_backward_weight(const mpgan_conv_geom* g, const float* x, int32_t ldx,
                               const mpgan_prologue* pro,
                               const float* dy, int32_t lddy,
                               float* dw, float* dbias /* nullable; ConvNd only: dbias = beta*dbias + colsum(dy), fused */,
                               float beta,
                               void* workspace, int64_t workspace_bytes, void* stream);
/* The profiling label of the weight-gradient launch (bf16_dy: of mpgan_conv_backward_weight_bf16dy), written like
 * mpgan_conv_kernel_name's; pro_code as there.  The launch, mpgan_conv_wgrad_workspace(_bf16dy) and this label read
 * one choice (choose_wgrad, conv_wgrad.hip). */
int mpgan_conv_wgrad_kernel_name(const mpgan_conv_geom* g, int32_t pro_code, int32_t bf16_dy, char* buf, int32_t len);
/* The same label for the operands actually passed: pitches, base alignment and prologue enter the choice as they do in
 * mpgan_conv_backward_weight (bf16_dy: mpgan_conv_backward_weight_bf16dy, which takes no prologue), after that entry's
 * own operand checks; a refusal returns the launch's status and message.  The pointers are read for alignment only:
 * nothing is dereferenced or launched. */
int mpgan_conv_wgrad_kernel_name_at(const mpgan_conv_geom* g, const float* x, int32_t ldx, const mpgan_prologue* pro,
                                    const void* dy, int32_t lddy, int32_t bf16_dy, char* buf, int32_t len);

/* Repack every conv / linear weight of a network in ONE launch.
 * table: device int64 [n_entries][8] = {src_off, dst_off, cout, cin, taps,
 * transposed, layout, 0}; offsets in floats into `flat_params` / `packed`;
 * layout 0 = [cout][tap][cin] (forward), 1 = [cin][tap][cout] (backward-data),
 * 2 = [tap][cin][cout] (backward-data of a Linear expressed as a whole-grid conv),
 * 3 = [tap][cout] of input channel 0 alone, cout*taps floats (ConvNd only; fp32 pack only): the backward-data pack of
 * the image plane of a two-plane conv, see mpgan_conv2p_forward. */
int mpgan_pack_weights(const float* flat_params, float* packed, const int64_t* table,
                       int32_t n_entries, int64_t max_elems, void* stream);

/* Perceptual-loss taps (variant B, test_runs/GAN.py:183-198,288-298): the discriminator
 * returns clones of every intermediate; the G loss adds sum_k mean|real_k - fake_k| / numel_k.
 * For a conv -> BatchNorm -> LeakyReLU layer the three taps (conv out z, norm out y,
 * activation a) are never materialised: their L1 terms and gradients are evaluated from the
 * two passes' raw conv outputs.  coef = device float[3]: d(loss)/d|tap| for (z, y, a). */
typedef struct {
  const float* z_peer;      /* the other pass's raw conv output, same shape */
  int32_t ld_peer;
  const float* scale_peer;  /* its norm scale / shift (per channel) */
  const float* shift_peer;
  const float* coef;        /* null => no peer */
} mpgan_peer_taps;

/* out3 = (mean|z_a-z_b|, mean|y_a-y_b|, mean|a_a-a_b|); partials >= mpgan_tap_l1_partials() floats */
int32_t mpgan_tap_l1_partials(void);
int mpgan_tap_l1(const float* za, int32_t lda, const mpgan_prologue* pa,
                 const float* zb, int32_t ldb, const mpgan_prologue* pb,
                 int64_t rows, int32_t c, float* partials, float* out3, void* stream);

/* ---- normalisation (BatchNorm training mode / InstanceNorm) -------------- */

/* Per-channel partial sums of z and z^2 over pixel chunks.
 * partials: [n][chunks][2][C]; returns chunks via mpgan_stats_chunks().
 * Replaces: the statistics half of batch_norm (every adn.N in MONAI UNet;
 * GAN_final.py:170,176,182,188). */
int32_t mpgan_stats_chunks(int64_t pixels_per_sample, int32_t c);
int mpgan_channel_stats(const float* z, int32_t ldz, int32_t n, int64_t pixels_per_sample,
                        int32_t c, float* partials, void* stream);

/* Finalise statistics: mean / biased var -> scale = gamma*invstd,
 * shift = beta - mean*scale; saves mean and invstd; updates running stats
 * (momentum, UNBIASED variance) when running_mean != null.
 * instance = 0: one set per channel (stats over n and pixels);
 * instance = 1: one set per (n, c).
 * With instance = 0 and more than 16384 partial rows (n*chunks > 16384) the rows are first folded to 32, into
 * scratch that must follow them in the same buffer: capacity >= (n*chunks + 32) * 2 * c floats
 * ((rows + 32) * 2 * cstride for mpgan_norm_finalize_strided). */
int mpgan_norm_finalize(const float* partials, int32_t n, int32_t chunks, int32_t c,
                        int64_t pixels_per_sample, int32_t instance,
                        const float* gamma, const float* beta, float eps, float momentum,
                        float* running_mean, float* running_var, int64_t* num_batches_tracked,
                        float* scale, float* shift, float* mean, float* invstd, void* stream);

/* The same over partial rows that are `cstride` >= c channels wide ([rows][2][cstride]): statistics of the FIRST c
 * channels of a conv that produced more (a ResidualUnit's first conv and its residual conv run as ONE conv
 * over their concatenated output channels -- same input, same geometry; only the first half feeds a norm). */
int mpgan_norm_finalize_strided(const float* partials, int32_t n, int32_t chunks, int32_t c, int32_t cstride,
                                int64_t pixels_per_sample, int32_t instance,
                                const float* gamma, const float* beta, float eps, float momentum,
                                float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                float* scale, float* shift, float* mean, float* invstd, void* stream);

/* Eval-mode BatchNorm (module.eval(), code/GAN/inferrence.py:97-110,169-170): scale/shift
 * from the running statistics; nothing is updated. */
int mpgan_norm_from_running(const float* gamma, const float* beta, const float* running_mean,
                            const float* running_var, float eps, int32_t c,
                            float* scale, float* shift, float* mean, float* invstd, void* stream);

/* The same for every norm layer of a network in one launch.  table: device int64[n_layers][10] =
 * {gamma, beta, running_mean, running_var, scale, shift, mean, invstd (device addresses; gamma/beta
 * may be 0), C, eps (the float's bit pattern in the low 32 bits)}. */
int mpgan_norm_from_running_multi(const int64_t* table, int32_t n_layers, void* stream);

/* Eval-mode inference (code/GAN/inferrence.py:97-110,169-170: generator.eval(); generator(x)): with running-statistics
 * BatchNorm a layer's affine is known before its conv runs, so the conv's epilogue applies it, the PReLU and the residual
 * add, and the ACTIVATED tensor is what reaches memory -- no norm_act_add launch, no prologue in the consumer:
 *     y = prelu(conv(x) * scale[c] + shift[c], slope[c]) (+ resid) (tanh)
 * The conv's own bias is folded into `shift` by the caller (mpgan_epi_vectors_multi does it); slope[c] = 1 leaves a
 * channel linear.  scale / shift / slope: [cout] floats, 16-byte aligned.  Not combinable with fused statistics. */
int mpgan_conv_forward_act(const mpgan_conv_geom* g, const float* x, int32_t ldx, const float* w_packed,
                           const float* scale, const float* shift, const float* slope, const float* resid,
                           int32_t ldr, int32_t tanh_out, float* y, int32_t ldy, void* stream);

/* The three vectors of every conv of an eval-mode plan in one launch.  table: device int64[n_layers][12] = {gamma, beta,
 * running_mean, running_var, conv bias, PReLU weight (one element) (device addresses; gamma / beta / bias / PReLU may be
 * 0), scale, shift, slope (outputs), c_norm, c_total, eps (the float's bit pattern in the low 32 bits)}: channels
 * < c_norm get scale = gamma / sqrt(var + eps), shift = beta + (bias - mean) * scale, slope = the PReLU weight (1 without
 * one); channels c_norm .. c_total - 1 (no norm layer: the residual half of a fused conv) get 1, bias, 1. */
int mpgan_epi_vectors_multi(const int64_t* table, int32_t n_layers, void* stream);

/* out = act(z*scale+shift) [+ r]   where r is either a plain tensor or itself
 * act(zr*scale_r+shift_r); optional tanh on the sum.  (ResidualUnit.forward's
 * "cx + res" and the generator's final Tanh, GAN_final.py:117.) */
int mpgan_norm_act_add(const float* z, int32_t ldz, const mpgan_prologue* pz,
                       const float* r, int32_t ldr, const mpgan_prologue* pr,
                       int32_t n, int64_t pixels_per_sample, int32_t c, int32_t tanh_out,
                       float* out, int32_t ldo, void* stream);

/* Backward of a = act(z*scale+shift), given g = dL/da:
 *   reduce  : partials [n][chunks][3][C] of (sum gy, sum gy*zhat, sum g*min(y,0)), followed by one float per
 *             row (n*chunks of them): that row's third sums added over the channels (the PReLU-slope gradient's
 *             terms) -- the buffer holds n*chunks*(3*C + 1) floats, chunks = mpgan_stats_chunks(P, C)
 *   finalize: dgamma += , dbeta += , dslope += (dslope != null needs the per-row scalars a reduce pass left;
 *             rows written by mpgan_conv_backward_data_stats carry none); coef c1 = sum gy / M, c2 = sum gy*zhat / M
 *   apply   : dz = scale*(gy - c1 - zhat*c2)
 * g may carry a fused pointwise factor: g_eff = g * (1 - t^2) (tanh backward)
 * when tanh_y != null. */
int mpgan_norm_bwd_reduce(const float* g, int32_t ldg, const float* z, int32_t ldz,
                          const mpgan_prologue* p, const float* mean, const float* invstd,
                          const mpgan_peer_taps* peer /* nullable */,
                          int32_t n, int64_t pixels_per_sample, int32_t c,
                          float* partials, void* stream);
int mpgan_norm_bwd_finalize(const float* partials, int32_t n, int32_t chunks, int32_t c,
                            int64_t pixels_per_sample, int32_t instance,
                            float* dgamma, float* dbeta, float* dslope,
                            float* c1, float* c2, void* stream);
int mpgan_norm_bwd_apply(const float* g, int32_t ldg, const float* z, int32_t ldz,
                         const mpgan_prologue* p, const float* mean, const float* invstd,
                         const float* c1, const float* c2,
                         const mpgan_peer_taps* peer /* nullable */,
                         int32_t n, int64_t pixels_per_sample, int32_t c,
                         float* dz, int32_t lddz, void* stream);

/* out[c] = beta*out[c] + sum_p partials[p][c]  (deterministic order). */
int mpgan_reduce_partials(const float* partials, int32_t rows, int32_t row_stride, int32_t c,
                          float* out, float beta, void* stream);

/* ---- pointwise helpers --------------------------------------------------- */
/* y = a + b (optionally y = tanh(a+b));  dx = g*(1-y^2). */
int mpgan_add_tanh(const float* a, const float* b, int64_t numel, int32_t apply_tanh,
                   float* y, void* stream);
int mpgan_tanh_backward(const float* g, const float* y, int64_t numel, float* dx, void* stream);
int mpgan_axpby(const float* a, float alpha, const float* b, float beta, int64_t numel,
                float* y, void* stream);
/* strided channel-slice copy: dst[p*ldd + c] = src[p*lds + c] (accumulate: +=) */
int mpgan_copy_slice(const float* src, int32_t lds, float* dst, int32_t ldd, int64_t pixels,
                     int32_t c, int32_t accumulate, void* stream);

/* ---- discriminator head: Flatten + Linear(F,1) + Sigmoid + BCE ------------ */
/* logit[n] = bias + sum_k act(z[n][k]*scale+shift) * w_perm[k]  where z is the
 * last conv's raw output in channels-last order and w_perm the Linear weight
 * permuted to that order by mpgan_pack_weights.  (GAN_final.py:198-204.) */
int32_t mpgan_linear1_partials(int32_t n); /* floats of `partials` scratch */
int mpgan_linear1_forward(const float* z, const mpgan_prologue* p, int32_t n,
                          int64_t pixels_per_sample, int32_t c, const float* w_perm,
                          const float* bias, float* partials, float* logit, float* prob /* sigmoid(logit), nullable */,
                          void* stream);
/* g_a[n][k] = dlogit[n]*w_perm[k];  dW (torch order, C-major) += sum_n dlogit[n]*a[n][k];
 * dbias += sum_n dlogit[n]. */
int mpgan_linear1_backward(const float* z, const mpgan_prologue* p, int32_t n,
                           int64_t pixels_per_sample, int32_t c, const float* w_perm,
                           const float* dlogit, float* g_a, float* dw, float* dbias,
                           float beta, void* stream);

/* ---- discriminator head, Markovian (PatchGAN): a last valid conv C -> 1 + Sigmoid ---- */
/* z: channels-last (n, in_dhw, c), depth 1 in 2-D; kernel k_dhw, stride 1, no padding: out = in - k + 1 per dimension.
 *   logit[n][p] = bias + sum_tap sum_c act(z[n][p+tap][c]*scale[c] + shift[c]) * w_perm[tap][c]
 *   prob = sigmoid(logit) (nullable)
 * p null: z is already activated; p->n_stride = c: per-sample scale / shift.  w_perm: what mpgan_pack_weights makes of
 * the (1, c, kd, kh, kw) weight, [tap][c].  fp32; no atomics, every sum in a fixed order (per lane its channel quads
 * and the taps in index order, then the lanes of the wave), so two runs give the same bits.
 * Refused before any launch: c % 4 != 0, z / w_perm / g_a / workspace not 16-byte aligned, in < k in any dimension,
 * taps*c*4 above the 64 KiB of LDS the kernels keep the weights in, a workspace that is too small. */
int mpgan_maphead_forward(const float* z, const mpgan_prologue* p, int32_t n, const int32_t in_dhw[3], int32_t c,
                          const int32_t k_dhw[3], const float* w_perm, const float* bias, float* logit,
                          float* prob /* nullable */, void* stream);
/* bytes of caller-supplied scratch mpgan_maphead_backward needs for dw (-1: geometry refused, see mpgan_last_error) */
int64_t mpgan_maphead_workspace(int32_t n, const int32_t in_dhw[3], int32_t c, const int32_t k_dhw[3]);
/* g_a[n][q][c] = sum_tap dlogit[n][q-tap] * w_perm[tap][c] over the taps that land inside the map (the gradient w.r.t.
 *   the ACTIVATED tensor, as mpgan_linear1_backward leaves it);
 * dw (torch order (1, c, kd, kh, kw)) = beta*dw + sum_{n,p} dlogit[n][p] * a[n][p+tap][c]: per-chunk partials in the
 *   workspace, then a finalize that adds the chunks in index order;
 * dbias = beta*dbias + sum dlogit.  g_a, dw, dbias: each nullable (workspace is needed for dw only). */
int mpgan_maphead_backward(const float* z, const mpgan_prologue* p, int32_t n, const int32_t in_dhw[3], int32_t c,
                           const int32_t k_dhw[3], const float* w_perm, const float* dlogit, float* g_a, float* dw,
                           float* dbias, float beta, void* workspace, int64_t workspace_bytes, void* stream);

/* prob = sigmoid(logit); loss = mean BCE(prob, target) with log clamped at
 * -100 (F.binary_cross_entropy, GAN_final.py:244-245); dlogit = loss_scale *
 * dL/dlogit computed THROUGH the clamped log and the sigmoid exactly as
 * autograd does (BCE backward: (p-t)/max((1-p)p, 1e-12)/n, then p(1-p)). */
int mpgan_sigmoid_bce(const float* logit, int32_t n, float target, float loss_scale,
                      float* prob, float* loss, float* dlogit, void* stream);

/* The same loss as separate autograd-shaped pieces (the module API returns the
 * probability, as the reference's Discriminator.forward does, and
 * GAN.adversarial_loss consumes it):
 *   bce_forward : loss = mean_i -(t_i*max(log p_i,-100) + (1-t_i)*max(log(1-p_i),-100))
 *   bce_backward: dprob_i = gout * (p_i - t_i) / max((1-p_i)*p_i, 1e-12) / n   (gout: device scalar)
 *   sigmoid_backward: dlogit_i = dprob_i * (1-p_i) * p_i */
int mpgan_bce_forward(const float* prob, const float* target, int32_t n, float* loss, void* stream);
int mpgan_bce_backward(const float* prob, const float* target, int32_t n, const float* gout,
                       float* dprob, void* stream);
int mpgan_sigmoid_forward(const float* logit, int32_t n, float* prob, void* stream);
int mpgan_sigmoid_backward(const float* dprob, const float* prob, int32_t n, float* dlogit, void* stream);
/* y = x * (*scalar)  (scalar on the device: an upstream autograd gradient) */
int mpgan_scale_by_device_scalar(const float* x, const float* scalar, int64_t numel, float* y, void* stream);
/* out[0] = sum_i v[i]*w[i], i = 0..n-1 in index order (n <= 4096 device scalars).  Replaces the running sum of
 * `F.l1_loss(...) / numel` over the 16 perceptual taps (test_runs/GAN.py:288-298): v holds the taps' L1 means, w
 * their 1/numel weights. */
int mpgan_weighted_sum(const float* v, const float* w, int32_t n, float* out, void* stream);

/* loss = mean |a-b| (F.l1_loss, GAN_final.py:247-248); grad_a = scale*sign(a-b)/numel
 * (written when grad_a != null).  partials: >= mpgan_l1_partials() floats. */
int32_t mpgan_l1_partials(void);
int mpgan_l1_loss(const float* a, const float* b, int64_t numel, float grad_scale,
                  float* partials, float* loss, float* grad_a, void* stream);

/* ---- adversarial objectives on the LOGITS (no Sigmoid in front) ----
 * MPGAN_ADV_BCE_LOGITS (F.binary_cross_entropy_with_logits; no log clamp, no 1e-12 guard; soft targets such as 0.9
 * are ordinary inputs):
 *   term_i = max(z_i,0) - z_i*t_i + log1p(exp(-|z_i|));  loss = mean_i term_i
 *   grad_i = (sigma(z_i) - t_i)/n,  sigma(z) = (z >= 0 ? 1 : e)/(1 + e) with e = exp(-|z|): neither branch overflows
 * MPGAN_ADV_LSGAN (F.mse_loss on the logits, CycleGAN's convention: no factor 1/2):
 *   term_i = (z_i - t_i)^2;  loss = mean_i term_i;  grad_i = 2*(z_i - t_i)/n
 * grad (nullable) is dL/dlogit for an upstream gradient of 1, written by the forward launch as mpgan_l1_loss writes its
 * own; an autograd backward is mpgan_scale_by_device_scalar on it.  Element terms in fp32, sums in fp64: per lane its
 * elements in index order, then the lanes of the wave, then the waves of the block, one plain store per block into
 * `partials`, the block partials added in index order (a second small launch; one block finishes alone).  No atomics
 * and a grid that depends on n alone: two runs give the same bits.  16-byte accesses when logit, target and grad are
 * 16-byte aligned (scalar tail), element-wise otherwise.  partials: >= mpgan_adv_loss_partials(n) doubles, 8-byte
 * aligned.  MPGAN_ERR_INVALID before any launch: n <= 0, an unknown kind, a null logit / target / partials / loss. */
enum { MPGAN_ADV_BCE_LOGITS = 0, MPGAN_ADV_LSGAN = 1 };
int32_t mpgan_adv_loss_partials(int32_t n); /* doubles of caller-supplied scratch (-1: n <= 0) */
int mpgan_adv_loss(const float* logit, const float* target, int32_t n, int32_t kind, double* partials, float* loss,
                   float* grad /* nullable */, void* stream);

/* ---- evaluation metrics (next-row N2: inferrence.py:188-204, metrics.py:213-223,
 *      psnr_ssim_metric.py:88-106) ---------------------------------------------------- */
/* y = clip(round((x-min)/(max-min)*(b_max-b_min)+b_min)): ScaleIntensityRangePercentiles(0,100,0,255)
 * + np.round as the inference script applies before writing / scoring; minmax2 receives (min,max).
 * partials >= mpgan_metric_partials() floats. */
int32_t mpgan_metric_partials(void);
int mpgan_rescale_minmax(const float* x, int64_t numel, float b_min, float b_max, int32_t do_round,
                         float* partials, float* minmax2, float* y, void* stream);
/* out3 = (MAE, MSE, PSNR = 10 log10(data_range^2 / MSE)) between two tensors. */
int mpgan_image_errors(const float* a, const float* b, int64_t numel, float data_range,
                       float* partials, float* out3, void* stream);

/* ---- pre-processing, array half of next-row N3 (GAN_final.py:386-394:
 *      ScaleIntensityRangePercentilesd(lower=1, upper=99, b_min=-1, b_max=1, clip=True)) ---------- */
/* out[j] = np.percentile(x, q[j]) (linear interpolation) for nq in {1, 2} percentiles: exact order
 * statistics by a 3-pass radix select; q_host is read on the host at call time.  Where q lands on an order
 * statistic (q = 0 and 100 among them) or between two equal ones the result is that statistic itself, so an
 * infinite minimum / maximum comes back infinite (numpy's interpolation forms inf - inf = NaN there); between an
 * infinity and another value the result is NaN or infinite as numpy's is.  NaN inputs are not supported.
 * numel < 2^32: the histogram counters are uint32 (a larger input is refused as unsupported).
 * workspace >= mpgan_percentile_workspace() bytes, 8-byte aligned. */
int64_t mpgan_percentile_workspace(void);
int mpgan_percentiles(const float* x, int64_t numel, const double* q_host, int32_t nq,
                      void* workspace, int64_t workspace_bytes, float* out, void* stream);
/* y = (x - a_min)/(a_max - a_min)*(b_max - b_min) + b_min, clipped to [b_min, b_max] when clip != 0
 * (MONAI ScaleIntensityRange; a_minmax = device float[2], e.g. the output of mpgan_percentiles). */
int mpgan_scale_intensity_range(const float* x, int64_t numel, const float* a_minmax, float b_min,
                                float b_max, int32_t clip, float* y, void* stream);

/* ResampleT1T2d (code/GAN/transforms.py:79-213) on arrays: linear-interpolation resampling of `vol` (contiguous
 * (D,H,W) fp32 with ITK geometry origin / spacing in (x,y,z) order and a row-major 3x3 direction matrix) onto
 * the identity-direction reference grid the transform builds: out_dhw voxels, origin = -size/2, spacing =
 * extent_mm / size (extent_mm = 256 in the reference), identity transform, default pixel 0.  Restates ITK 5's
 * ResampleImageFilter + LinearInterpolateImageFunction (ITK is not installable here: parity unpinned). */
int mpgan_resample_to_identity_grid(const float* vol, const int32_t* in_dhw, const double* origin_xyz,
                                    const double* spacing_xyz, const double* direction_3x3, const int32_t* out_dhw,
                                    double extent_mm, float* out, void* stream);

/* Mean structural similarity of two slices (dhw[0] == 1: 7x7 window) or volumes (dhw[0] >= 7: 7x7x7),
 * the algorithm skimage.metrics.structural_similarity runs with the arguments psnr_ssim_metric.py:91-92
 * passes (data_range only): uniform window, K1 = 0.01, K2 = 0.03, sample covariance, mean over the
 * interior that drops 3 border samples per windowed axis.  a, b: contiguous (D,H,W) fp32.
 * workspace >= mpgan_ssim_workspace(dhw) bytes (per-tile partial sums, double). */
int64_t mpgan_ssim_workspace(const int32_t* dhw);
int mpgan_ssim(const float* a, const float* b, const int32_t* dhw, float data_range,
               void* workspace, int64_t workspace_bytes, float* out1, void* stream);

/* ---- joint histogram and mutual information (the MUTINF figure stored in code/eval) ---- */
#define MPGAN_JH_MASK_NONE 0           /* every voxel inside both ranges */
#define MPGAN_JH_MASK_BOTH_NONZERO 1   /* ... whose two values are both non-zero */
#define MPGAN_JH_MASK_EITHER_NONZERO 2 /* ... of which at least one value is non-zero */
#define MPGAN_JH_MASK_EXPLICIT 3       /* ... whose byte in `mask` is non-zero */
/* hist[item][ia][ib] (int64, zeroed by the call) counts the voxels of item `item` of two contiguous fp32 arrays of
 * batch x numel_per_item elements whose a-value falls into bin ia and b-value into bin ib.  The bin of a value v over
 * [lo, hi] is min((int)floorf((v - lo) * s), bins - 1) with s = (float)bins / (hi - lo), evaluated in fp32 exactly as
 * written, so v == hi falls into the last bin; a voxel with a value below lo, above hi or NaN, or one the mask mode
 * refuses, is dropped.  Counts are exact and do not depend on execution order.  2 <= bins <= 256; `mask` (uint8,
 * same length) is read in mode 3 only and may be null otherwise; a and b may be null when numel_per_item == 0
 * (a zero histogram).  No workspace. */
int mpgan_joint_histogram(const float* a, const float* b, const uint8_t* mask, int32_t mask_mode,
                          int64_t numel_per_item, int32_t batch,
                          float lo_a, float hi_a, float lo_b, float hi_b, int32_t bins,
                          int64_t* hist, void* stream);
/* out6[item] = (mi, h_a, h_b, h_ab, nmi, count) in double from hist[item][bins][bins]: entropies in nats from the
 * integer counts, H = log N - (sum c log c) / N over the exact int64 marginals and the joint counts;
 * mi = h_a + h_b - h_ab; nmi = (h_a + h_b) / h_ab (Studholme); count = N.  N == 0: NaN for the five values and
 * count 0; every voxel in one bin (h_ab == 0): mi = 0, nmi = 1.  Fixed summation order: bitwise reproducible. */
int mpgan_mutual_information(const int64_t* hist, int32_t batch, int32_t bins, double* out6, void* stream);

/* ---- Parzen-window mutual information: a differentiable loss (MONAI 0.4.0 GlobalMutualInformationLoss, which
 * code/GAN/metrics.py:19 imports; MONAI is not in this image, the definition below is what is pinned) ----
 * a, b: contiguous fp32 arrays of batch x numel_per_item elements (channels fold into samples), N = numel_per_item.
 *   x'      = clamp((x - lo) / (hi - lo), 0, 1)            per image, NaN stays NaN
 *   c_i     = i / (K - 1), i = 0..K-1;  sigma = sigma_ratio / (K - 1);  p = 1 / (2 sigma^2)
 *   w_i(x)  = e_i / sum_k e_k,  e_i = exp(-p (x' - c_i)^2)
 *   pab_ij  = (1/N) sum_n wa_i(n) wb_j(n);  pa_i = sum_j pab_ij;  pb_j = sum_i pab_ij
 *   mi      = sum_ij pab_ij log((pab_ij + nr) / (pa_i pb_j + dr) + dr)
 * Gradient: R = (pab + nr) / (pa pb + dr);  A = log(R + dr) + pab / ((R + dr)(pa pb + dr));
 *   Dp = -pab (pab + nr) / ((R + dr)(pa pb + dr)^2);  G_ij = A_ij + sum_j Dp_ij pb_j;  G'_ij = A_ij + sum_i Dp_ij pa_i;
 *   h_i(n) = sum_j G_ij wb_j(n);  hbar(n) = sum_i wa_i(n) h_i(n);
 *   d mi / d a_n = (1/N) (1/(hi_a - lo_a)) m(n) sum_i wa_i(n) (h_i(n) - hbar(n)) (-2 p (a'_n - c_i)),
 *   m(n) = 1 when the mapped value lies in the CLOSED interval [0, 1] (torch.clamp's rule), else 0; for b the same
 *   with the roles swapped and G'.
 * 2 <= bins <= 32 (MPGAN_ERR_INVALID above, before any launch).  The weights and the joint accumulate in fp32 (each
 * wave an fmaf chain over at most 512 voxels), a block adds its 16 waves' tiles in wave order in fp64 into its own
 * workspace slot, the slots are summed in slot order and everything after the joint is fp64: results are bitwise
 * reproducible from call to call.  The calls allocate nothing, are asynchronous on `stream` and can be captured
 * into a graph. */
/* Bytes of workspace the forward needs (8-byte aligned): a function of (batch, numel_per_item) only; -1 on a bad
 * argument. */
int64_t mpgan_parzen_mi_workspace(int32_t batch, int64_t numel_per_item, int32_t bins);
/* mi[batch] (double).  Optional outputs, each may be null: joint[batch][bins][bins] (double, pab);
 * coef[batch][2][32][32] (float, 16-byte aligned: G and G' transposed, each less its pab-weighted mean -- a
 * constant that cancels in h_i - hbar --, what the backward reads);
 * loss (float): reduction 0: loss[0] = -mean_b mi; 1: loss[0] = -sum_b mi; 2: loss[b] = -mi[b]. */
int mpgan_parzen_mi_forward(const float* a, const float* b, int64_t numel_per_item, int32_t batch,
                            float lo_a, float hi_a, float lo_b, float hi_b, int32_t bins, double sigma_ratio,
                            double smooth_nr, double smooth_dr, void* workspace, int64_t workspace_bytes,
                            double* joint, double* mi, float* coef, int32_t reduction, float* loss, void* stream);
/* grad[batch][numel_per_item] = upstream[item * upstream_stride] * scale * d mi[item] / d (wrt == 0 ? a : b), with
 * the geometry and coef of the forward call.  upstream is a device array (stride 1) or one device scalar for every
 * item (stride 0); scale is the host factor of the reduction (-1, or -1/batch for the mean). */
int mpgan_parzen_mi_backward(const float* a, const float* b, int64_t numel_per_item, int32_t batch,
                             float lo_a, float hi_a, float lo_b, float hi_b, int32_t bins, double sigma_ratio,
                             const float* coef, const float* upstream, int32_t upstream_stride, float scale,
                             int32_t wrt, float* grad, void* stream);

/* ---- SSIM loss: the structural similarity of mpgan_ssim as a differentiable loss (the figure
 * code/GAN/psnr_ssim_metric.py:88-106 reports; the reference's trainer has no such term, the definition below is what
 * is pinned) ----
 * a, b: contiguous fp32 arrays of `items` images of dhw = (D, H, W) samples each; an item is one (batch, channel)
 * image, items = batch * channels.  D == 1: slices, 7x7 windows (d = 2); D >= 7: volumes, 7x7x7 windows (d = 3).
 * The samples enter shifted, a = x - lo (no clamp: the gradient passes through unchanged); L = hi - lo.
 *   n = 7^d;  cn = n / (n - 1);  C1 = (0.01 L)^2;  C2 = (0.03 L)^2
 *   per window lying wholly inside the image (M = prod(S_i - 6) of them):
 *     ux, uy = window means;  vx = cn (sum a^2 / n - ux^2), vy likewise;  vxy = cn (sum a b / n - ux uy)
 *     A1 = 2 ux uy + C1;  A2 = 2 vxy + C2;  B1 = ux^2 + uy^2 + C1;  B2 = vx + vy + C2;  S = A1 A2 / (B1 B2)
 *   ssim_item = mean of S over the M windows (what mpgan_ssim computes for one image);  loss_item = 1 - ssim_item
 *   reduction 0: loss[0] = mean over the items; 1: loss[0] = their sum; 2: loss[batch], entry b = mean over b's channels.
 * Gradient: per window  Q = -2 cn S / B2;  R = 2 cn A1 / (B1 B2);
 *     P = 2 uy A2 / (B1 B2) - 2 ux S / B1 - ux Q - uy R
 *   d ssim_item / d a_p = (1 / (n M)) (sum P + a_p sum Q + b_p sum R), the sums over the (up to 7^d) valid windows that
 *   contain sample p; for b the same with the roles swapped: P with ux <-> uy, Q and R shared.
 * Window sums, the maps and the box sums of the backward are fp64 and every sum has a fixed order (no atomics): the
 * loss and both gradients are bitwise reproducible from call to call.  The maps are stored as doubles because P holds
 * -ux Q: sum P + a_p sum Q cancels in flat regions, and an fp32 P would leave its rounding as the gradient's error.
 * The calls allocate nothing, are asynchronous on `stream` and can be captured into a graph.  Extents below the
 * window are MPGAN_ERR_INVALID, a depth in 2..6 is MPGAN_ERR_UNSUPPORTED, both before any launch. */
/* Bytes of workspace the forward needs (8-byte aligned); *coef_bytes (nullable) receives the bytes of the coefficient
 * buffer for grad_mask (bit 0: a gradient for a will be asked for, bit 1: for b; 0: none, no buffer).  -1 on a bad
 * argument. */
int64_t mpgan_ssim_loss_workspace(const int32_t* dhw, int32_t items, int32_t grad_mask, int64_t* coef_bytes);
/* loss as `reduction` says (fp32, written on the device: no host sync).  With grad_mask != 0 the same pass writes
 * coef = [Q][R][P of a, if bit 0][P of b, if bit 1], each [items][M] doubles over the window corners; coef may be
 * null when grad_mask == 0. */
int mpgan_ssim_loss_forward(const float* a, const float* b, const int32_t* dhw, int32_t items, int32_t channels,
                            double lo, double hi, int32_t grad_mask, void* workspace, int64_t workspace_bytes,
                            void* coef, int64_t coef_bytes, int32_t reduction, float* loss, void* stream);
/* grad[items][D][H][W] = upstream[(item / channels) * upstream_stride] * scale * d ssim_item / d (wrt == 0 ? a : b),
 * with the geometry, lo, grad_mask and coef of the forward call (coef is read, never written: a second call gives the
 * same bits).  upstream is a device array over the batch (stride 1) or one device scalar (stride 0); scale is the
 * host factor of the reduction (-1 for the sum, -1 / items for the mean, -1 / channels for reduction 2). */
int mpgan_ssim_loss_backward(const float* a, const float* b, const int32_t* dhw, int32_t items, int32_t channels,
                             double lo, int32_t grad_mask, const void* coef, int64_t coef_bytes,
                             const float* upstream, int32_t upstream_stride, double scale, int32_t wrt, float* grad,
                             void* stream);

/* ---- masked SSIM: the SSIM loss over a foreground, and the per-window map (ssim_loss.hip) ----
 * Everything is as in the "SSIM loss" block above: items, dhw, the 7-wide uniform window, n, cn, C1, C2, S, Q, R, P, lo
 * and hi.  One thing is added: every valid window k carries a weight w_k in {0, 1}, read at the window's CENTRE voxel:
 * corner + 3 on every windowed axis (for D == 1 the z index is unchanged).  That is "take the map of S, crop the
 * 3-sample border as skimage does, average it over the mask".  The weight has AT MOST ONE source:
 *   mask  uint8[items][D][H][W],  w_k = (mask[centre_k] != 0): any non-zero byte counts; or
 *   thr   device float[items],    w_k = (b[centre_k] > thr[item]) by mpgan_foreground_mask's rule: strict, in fp32, 0
 *                                 for a NaN on either side -- no mask array exists; or
 *   neither: w_k = 1.
 * Per item:
 *   n_item    = sum_k w_k, an exact count (mask voxels in the 3-wide border that the interior drops do not count)
 *   ssim_item = (sum_k w_k S_k) / n_item, and NaN where n_item == 0
 *   loss_item = 1 - ssim_item, and 0 where n_item == 0 (mpgan_masked_l1's convention for an empty item)
 *   reductions 0 / 1 / 2 as for the SSIM loss.
 *   d ssim_item / d a_p = (1 / (n n_item)) (sum w_k P_k + a_p sum w_k Q_k + b_p sum w_k R_k) over the valid windows that
 *   contain p; for b with the roles swapped; exactly 0 for an empty item.  Nothing flows into the mask or the threshold.
 * A block's sum of w S is fp64 in the SSIM loss's order, its count of w an integer; stats (device double[items][2])
 * receives (ssim_item, n_item), the item's partials added in slot order by the fixed tree of the other loss tails: no
 * atomics, bitwise reproducible.  The stored maps are w Q, w R, w P -- exact, zero or the value.  smap (nullable,
 * float[items][M] over the window corners, 4-byte aligned) receives S of EVERY valid window, whatever its weight,
 * rounded to fp32.  workspace >= mpgan_masked_ssim_loss_workspace(...) bytes and stats are 8-byte aligned; coef as for
 * the SSIM loss.  The backward reads its per-item factor scale / (n n_item) from stats on the device: nothing syncs.
 * MPGAN_ERR_INVALID before any launch: both mask sources, a null a / b / workspace / stats / loss (backward: a / b /
 * coef / stats / upstream / grad), a geometry, grad_mask or reduction the SSIM loss refuses, a workspace that is too
 * small or misaligned.  The calls allocate nothing, are asynchronous on `stream` and can be captured into a graph. */
int64_t mpgan_masked_ssim_loss_workspace(const int32_t* dhw, int32_t items, int32_t grad_mask, int64_t* coef_bytes);
int mpgan_masked_ssim_loss_forward(const float* a, const float* b, const int32_t* dhw, int32_t items, int32_t channels,
                                   double lo, double hi, const uint8_t* mask /* nullable */,
                                   const float* thr /* nullable */, int32_t grad_mask, void* workspace,
                                   int64_t workspace_bytes, void* coef, int64_t coef_bytes, double* stats,
                                   float* smap /* nullable */, int32_t reduction, float* loss, void* stream);
/* As mpgan_ssim_loss_backward, with the forward's stats; scale is the host factor of the reduction alone. */
int mpgan_masked_ssim_loss_backward(const float* a, const float* b, const int32_t* dhw, int32_t items,
                                    int32_t channels, double lo, int32_t grad_mask, const void* coef,
                                    int64_t coef_bytes, const double* stats, const float* upstream,
                                    int32_t upstream_stride, double scale, int32_t wrt, float* grad, void* stream);

/* ---- Sobel edge loss: the L1 distance of two 3-D Sobel edge-magnitude maps (the generator term of Ea-GAN, Yu et al.
 * 2019; the definition below is what is pinned; Ea-GAN's own filters are this operator times 8 in 2-D, times 32 in 3-D) ----
 * x, a, b: contiguous fp32 arrays of `items` images of dhw = (D, H, W) samples each; an item is one (batch, channel)
 * image, items = batch * channels.  Any extent >= 1 is legal.  d = 3 (a 2-D image has D = 1, see below).
 *   Dv = (-1, 0, 1);  Sv = (1, 2, 1);  clamp is per axis to [0, n - 1] (a replicate border: a constant image has no
 *   edges anywhere, where zero padding would plant a frame of them)
 *   G_k(x)_p = 1 / (2 4^(d-1)) sum over t in {-1,0,1}^d of Dv[t_k] prod_{j != k} Sv[t_j] x[clamp(p + t)]
 *              (a ramp of slope 1 per voxel along axis k answers 1)
 *   m(x)_p   = sqrt(sum_k G_k(x)_p^2 + eps),  eps > 0;  d m_p / d G_k = G_k / m, which is 0 in flat regions
 *   D == 1: the three z taps read one voxel, G_z = 0 and the z smoothing sums to 4 / 4: exactly the 2-D operator
 *   1 / (2 4) sum Dv Sv x.  Nothing is special-cased.
 *   loss_item = mean over the N = D H W voxels of |m(a)_p - m(b)_p|
 *   reduction 0: loss[0] = mean over the items; 1: loss[0] = their sum; 2: loss[batch], entry b = mean over b's channels.
 * Adjoint of m for an upstream map dy:  dx_p = sum_q dy_q sum_k (G_k / m)_q dG_k(x)_q / dx_p.  A tap of q that falls
 * outside the image lands on the border voxel it was clamped to, so along each axis the transposed taps of p are
 * (q = p - 1, p, p + 1) with weights (1, 2 + [p == 0] + [p == n - 1], 1) for Sv and (1, [p == n - 1] - [p == 0], -1)
 * for Dv, over the q inside the image.
 * Gradient of the loss: the adjoint with dy_q = s_q / N for a and -s_q / N for b (and b's G, m), where
 * s_q = sign(m(a)_q - m(b)_q), sign(0) = 0.
 * The tap sums are formed in fp64 (exact for fp32 samples) and rounded once, so G_k keeps its relative precision where
 * the image is nearly flat; m and G_k / m are fp32.  All four entry points take m from one device function: the loss
 * and a composition through the magnitude map see the same bits of m, hence the same signs.  Block partial sums of
 * the loss are fp64 and every sum has a fixed order (no atomics): results are bitwise reproducible from call to call.
 * Nothing but the inputs passes from forward to backward.  The calls allocate nothing, are asynchronous on `stream`
 * and can be captured into a graph.  A null pointer, eps <= 0, an extent < 1, items outside [1, 65535] or an unknown
 * reduction is MPGAN_ERR_INVALID before any launch. */
/* out[items][D][H][W] = m(x). */
int mpgan_sobel_magnitude_forward(const float* x, const int32_t* dhw, int32_t items, double eps, float* out,
                                  void* stream);
/* dx[items][D][H][W] = the adjoint above for the upstream map dy[items][D][H][W]; recomputed from x. */
int mpgan_sobel_magnitude_backward(const float* x, const int32_t* dhw, int32_t items, double eps, const float* dy,
                                   float* dx, void* stream);
/* Bytes of workspace mpgan_edge_loss_forward needs (8-byte aligned).  -1 on a bad argument. */
int64_t mpgan_edge_loss_workspace(const int32_t* dhw, int32_t items);
/* loss as `reduction` says (fp32, written on the device: no host sync).  No magnitude map is written: a block's
 * partial sum goes to `workspace`, a second stage adds an item's partials in slot order. */
int mpgan_edge_loss_forward(const float* a, const float* b, const int32_t* dhw, int32_t items, int32_t channels,
                            double eps, void* workspace, int64_t workspace_bytes, int32_t reduction, float* loss,
                            void* stream);
/* grad[items][D][H][W] = upstream[(item / channels) * upstream_stride] * scale * d loss_item / d (wrt == 0 ? a : b),
 * the signs formed on the fly from a and b.  upstream is a device array over the batch (stride 1) or one device scalar
 * (stride 0); scale is the host factor of the reduction (1 for the sum, 1 / items for the mean, 1 / channels for
 * reduction 2). */
int mpgan_edge_loss_backward(const float* a, const float* b, const int32_t* dhw, int32_t items, int32_t channels,
                             double eps, const float* upstream, int32_t upstream_stride, double scale, int32_t wrt,
                             float* grad, void* stream);

/* ---- foreground masks: Otsu threshold, mask / bounding box / count, mask-weighted L1, masked errors
 * (foreground.hip; DESIGN.md 7k.  The reference imports MONAI's CropForegroundd and ThresholdIntensityd in its scoring
 * scripts, code/GAN/minipig_inference.py:28,43, and never calls them; MONAI and skimage are not in this image: the
 * definitions below are what is pinned, against tests/foreground_ref.py) ----
 * An item is one (batch, channel) image of numel_per_item contiguous fp32 values; items = batch * channels.  All four
 * groups are one-pass streams: a block of 256 threads walks a contiguous chunk of one item, thread t taking the groups
 * of four consecutive values t, t + 256, ... of the chunk in that order -- 16 bytes wide when the item's first value is
 * 16-byte aligned (a mask: 4-byte aligned), value by value otherwise and in a last short group; the values a thread
 * sees, and their order, do not depend on the alignment.  The number of chunks depends on the sizes alone.
 * Floating-point sums are fp64: a thread adds its terms in that order, the block folds its threads by a fixed tree
 * and stores one partial, the partials of an item are added in slot order by a fixed tree.  No floating-point atomics
 * anywhere; integer atomics (counts, minima, maxima) do not depend on order.  Results are bitwise reproducible from
 * call to call.  The calls allocate nothing, are asynchronous on `stream` and can be captured into a graph. */

/* thr[item] (device float[items]) = Otsu's threshold of the item's histogram, as skimage.filters.threshold_otsu forms
 * it from bin counts and bin centres.
 *   n_j   = number of the item's values in bin j of `bins` equal-width bins over [lo, hi], by mpgan_joint_histogram's
 *           rule: j = min((int)floorf((v - lo) * s), bins - 1), s = (float)bins / (hi - lo), in fp32 exactly as written,
 *           so v == lo falls into bin 0 and v == hi into the last bin; v < lo, v > hi and NaN are dropped.  Exact integers.
 *   c_j   = lo + (j + 0.5) * (hi - lo) / bins          in double, evaluated left to right from the two floats
 *   N     = sum_j n_j
 *   for k = 0 .. bins - 2:
 *     w0 = sum_{j <= k} n_j;  w1 = N - w0                                        (integers)
 *     mu0 = (sum_{j <= k} n_j c_j, added for j = 0, 1, .. k) / w0                (double)
 *     mu1 = (sum_{j > k} n_j c_j, added for j = bins - 1, bins - 2, .. k + 1) / w1
 *     var_k = (w0 * w1) * ((mu0 - mu1) * (mu0 - mu1)), and 0 where w0 == 0 or w1 == 0
 *   k* = the FIRST k that attains max_k var_k;  thr = (float)c_{k*}
 * Degenerate items: N == 0 gives NaN; exactly one non-empty bin j gives (float)c_j (every var_k is 0 there, and the
 * centre of the occupied bin is the one value that describes the image).
 * 2 <= bins <= 256; items >= 1; numel_per_item >= 1; lo < hi, both finite and s finite; workspace >=
 * mpgan_otsu_workspace(items, bins) bytes, 8-byte aligned (the int64 histograms; the call zeroes them).  Anything
 * else, or a null x / workspace / thr, is MPGAN_ERR_INVALID before any launch. */
int64_t mpgan_otsu_workspace(int32_t items, int32_t bins); /* bytes; -1 on a bad argument */
int mpgan_otsu_threshold(const float* x, int64_t numel_per_item, int32_t items, float lo, float hi, int32_t bins,
                         void* workspace, float* thr, void* stream);

/* One pass over x[items][D][H][W] (dhw = (D, H, W), D == 1 for 2-D) against the per-item thresholds thr (device
 * float[items], e.g. mpgan_otsu_threshold's output: no host sync in between).  A voxel is foreground when
 * x > thr[item], strictly and in fp32: a value equal to the threshold is background, and a NaN value or a NaN
 * threshold gives background.  Each output may be null; at least one must be asked for.
 *   mask[items][D][H][W]  uint8, 1 for foreground and 0 otherwise
 *   count[items]          int64, the number of foreground voxels
 *   box[items][2][3]      int32, MONAI's generate_spatial_bounding_box per item over the axes (z, y, x):
 *                         box[item][0][d] = start_d = max(min_d - margin[d], 0),
 *                         box[item][1][d] = end_d   = min(max_d + 1 + margin[d], extent_d)   (exclusive),
 *                         min_d / max_d the smallest / largest index of a foreground voxel along axis d;
 *                         an item without foreground gives start = end = 0 on every axis.
 * margin: host int32[3] >= 0 over (z, y, x), read at call time; null means no margin.  The call initialises box and
 * count itself (a small launch in front, and one behind that turns the raw extremes into the box).
 * MPGAN_ERR_INVALID before any launch: a null x / dhw / thr, no output at all, items < 1, an extent < 1, a negative
 * margin. */
int mpgan_foreground_mask(const float* x, const int32_t* dhw, int32_t items, const float* thr, const int32_t* margin,
                          uint8_t* mask /* nullable */, int32_t* box /* nullable */, int64_t* count /* nullable */,
                          void* stream);

/* Mask-weighted L1 of two arrays a, b of items x numel_per_item values.  The mask has exactly ONE source:
 *   mask  uint8[items][numel_per_item], m_i = (mask_i != 0); or
 *   thr   device float[items],          m_i = (b_i > thr[item]) by mpgan_foreground_mask's rule -- no mask array exists.
 *   w_i = m_i ? w_fg : w_bg   (doubles, >= 0 and finite)
 *   num_item = sum_i w_i * |a_i - b_i|, every term in fp64 from the two floats (the difference is exact)
 *   den_item = w_fg * n_fg + w_bg * (numel_per_item - n_fg), n_fg the exact number of i with m_i  (= sum_i w_i)
 *   loss_item = num_item / den_item, and 0 where den_item == 0
 *   reduction 0: loss[0] = mean over the items; 1: loss[0] = their sum; 2: loss[batch], entry b = mean over b's channels
 *   (batch = items / channels), as the SSIM and edge losses define them.
 * den (device double[items]) receives den_item: the backward reads it.  workspace >=
 * mpgan_masked_l1_workspace(numel_per_item, items) bytes, 8-byte aligned.
 * MPGAN_ERR_INVALID before any launch: a null a / b / workspace / den / loss, both mask sources or neither,
 * items < 1, numel_per_item < 1, channels < 1 or no divisor of items, a negative or non-finite weight, an unknown
 * reduction, a workspace that is too small. */
int64_t mpgan_masked_l1_workspace(int64_t numel_per_item, int32_t items); /* bytes; -1 on a bad argument */
int mpgan_masked_l1_forward(const float* a, const float* b, int64_t numel_per_item, int32_t items, int32_t channels,
                            const uint8_t* mask, const float* thr, double w_fg, double w_bg, void* workspace,
                            int64_t workspace_bytes, double* den, int32_t reduction, float* loss, void* stream);
/* da_i = (float)(upstream[(item / channels) * upstream_stride] * scale * w_i / den_item) * sign(a_i - b_i), with
 * sign(0) = 0 (and 0 for a NaN difference), the factor formed in double and rounded to fp32 once per item and weight;
 * db_i = -da_i, bit for bit.  Either output may be null, not both.  An item with den_item == 0 gets zeros.  Nothing
 * flows into the mask or the threshold.  upstream is a device array over the batch (stride 1) or one device scalar
 * (stride 0); scale is the host factor of the reduction (1 for the sum, 1 / items for the mean, 1 / channels for
 * reduction 2).  The mask source, the weights and den are those of the forward call. */
int mpgan_masked_l1_backward(const float* a, const float* b, int64_t numel_per_item, int32_t items, int32_t channels,
                             const uint8_t* mask, const float* thr, double w_fg, double w_bg, const double* den,
                             const float* upstream, int32_t upstream_stride, double scale, float* da /* nullable */,
                             float* db /* nullable */, void* stream);

/* out4 (device double[4]) = (MAE, MSE, PSNR, count) of a against b over the n voxels whose mask byte is non-zero:
 *   MAE = sum |a - b| / n;  MSE = sum (a - b)^2 / n;  PSNR = 10 log10(data_range^2 / MSE);  count = n
 * with every term and every sum in fp64.  An empty mask gives NaN for the three and count 0.  MSE == 0 gives
 * PSNR = +infinity, as mpgan_image_errors gives.  partials: >= mpgan_masked_errors_partials(numel) doubles, 8-byte
 * aligned.  A null pointer or numel < 1 is MPGAN_ERR_INVALID before any launch. */
int64_t mpgan_masked_errors_partials(int64_t numel); /* doubles of caller-supplied scratch (-1: numel < 1) */
int mpgan_masked_image_errors(const float* a, const float* b, const uint8_t* mask, int64_t numel, float data_range,
                              double* partials, double* out4, void* stream);

/* ---- differentiable augmentation in front of the discriminator (DiffAugment, Zhao et al. 2020) ----
 * x: contiguous fp32 [n][D][H][W] (one channel; 2-D images have D = 1); N = D H W.  Per sample s, from two device tables
 * (nothing is read on the host):
 *   color: float [n][2] = (b, c), brightness offset and contrast factor
 *   geom:  int32 [n][9] = (t_d, t_h, t_w, lo_d, lo_h, lo_w, size_d, size_h, size_w)
 * `ops` selects what is applied; a disabled op ignores its table entries (and a table no enabled op reads may be null).
 * With m = the mean of x over the sample:
 *   u[q]    = c (x[q] - m) + m + b                 (b = 0 without BRIGHTNESS; c = 1 and no mean without CONTRAST)
 *   keep(p) = inside(p + t) and not (lo_k <= p_k < lo_k + size_k for every axis k)
 *   y[p]    = keep(p) ? u[p + t] : fill
 *   g_u[q]  = inside(q - t) and keep(q - t) ? g_y[q - t] : 0
 *   g_x[q]  = c g_u[q] + (1 - c) / N * sum_q' g_u[q']        (the sum only with CONTRAST)
 * Any t is legal (|t_k| >= S_k: all fill) and any box (negative lo, past the edge, size <= 0: nothing cut).  Without a
 * colour op y and g_x are copies, zeros and `fill`: exact.  m and (1 - c) / N * sum g_u are fp64 sums rounded to fp32
 * once; the element arithmetic is fp32.
 * Launches: one each way, two with CONTRAST (the block partials of the sample sums into `ws`, then the apply kernel, which
 * adds a sample's partials itself).  No atomics; the grid and every sum's order depend on (n, dhw) alone: two runs give
 * the same bits.  16-byte accesses when both pointers are 16-byte aligned and W % 4 == 0, element-wise otherwise.
 * ws: >= mpgan_diffaug_workspace(n, dhw) bytes, 8-byte aligned; read and written only with CONTRAST (may be null
 * otherwise).  The backward needs neither x nor y.  MPGAN_ERR_INVALID before any launch: a null x / y / dhw (or a table
 * an enabled op reads), n <= 0, an extent < 1, unknown ops bits, n * N >= 2^31, with CONTRAST a null, short or
 * misaligned ws. */
enum { MPGAN_DIFFAUG_BRIGHTNESS = 1, MPGAN_DIFFAUG_CONTRAST = 2, MPGAN_DIFFAUG_TRANSLATION = 4, MPGAN_DIFFAUG_CUTOUT = 8 };
int64_t mpgan_diffaug_workspace(int32_t n, const int32_t* dhw); /* bytes of fp64 block partials (-1: bad geometry) */
int mpgan_diffaug_forward(const float* x, int32_t n, const int32_t* dhw, int32_t ops, const float* color,
                          const int32_t* geom, float fill, void* ws, int64_t ws_bytes, float* y, void* stream);
int mpgan_diffaug_backward(const float* gy, int32_t n, const int32_t* dhw, int32_t ops, const float* color,
                           const int32_t* geom, void* ws, int64_t ws_bytes, float* gx, void* stream);

/* ---- paired affine augmentation of the training pair itself (pair_augment.hip) ----
 * x0, x1: contiguous fp32 [n][D][H][W] (one channel; 2-D images have D = 1), the two planes of a pair; x1 == y1 == null
 * warps one plane.  y0, y1: [n][oD][oH][oW]; in_dhw and out_dhw may differ.  Per sample s, from device tables (nothing is
 * read on the host):
 *   theta: double [n][12], a row-major 3 x 4 (A | t) in (d, h, w) voxel-index order
 *   sigma: float [n][2], the noise factor of plane 0 and plane 1
 * Output voxel p = (d, h, w) samples the input at the continuous index c = A p + t:
 *   y_k[p] = trilinear(x_k, c) + sigma[s][k] * noise_k[p]          (the second term only with a noise_k pointer)
 * over the 8 corners floor(c) + {0,1}^3 with the weights prod_axis (1 - f or f), f = c - floor(c):
 *   MPGAN_WARP_CONSTANT  a corner outside the input has the value fill_k (scipy's mode="grid-constant"; with fill 0
 *                        grid_sample(padding_mode="zeros", align_corners=True))
 *   MPGAN_WARP_BORDER    c is first clamped to [0, S - 1] per axis (scipy's mode="nearest"; grid_sample's "border")
 * Both are continuous in c; a corner whose weight is exactly 0 is not read.  c, the weights, the lerps and the noise
 * term are fp64, rounded to fp32 once; the coordinates and weights are computed once per voxel and used for both
 * planes.  An integer-valued (A | t) (identity, flips, quarter turns, integer shifts) copies bits.  A plane whose sigma
 * is 0, or that has no noise pointer, gets the bits of the call without noise.  Any theta is legal: a c beyond the
 * input (or NaN) is `fill` / the clamped edge.
 * Launch: one kernel for both planes, one thread per output voxel, a block per 4 x 8 x 32 (D = 1: 1 x 8 x 32) tile of
 * the output.  No atomics; the grid depends on (n, out_dhw) alone: two runs give the same bits.
 * MPGAN_ERR_INVALID before any launch: a null x0 / y0 / theta / in_dhw / out_dhw, x1 without y1 or the reverse, n <= 0,
 * an extent < 1, an unknown mode, a noise pointer without sigma (or sigma without one, or noise1 without x1),
 * n * N_in or n * N_out >= 2^31. */
enum { MPGAN_WARP_CONSTANT = 0, MPGAN_WARP_BORDER = 1 };
int mpgan_affine_warp(const float* x0, const float* x1, int32_t n, const int32_t* in_dhw, const int32_t* out_dhw,
                      const double* theta, int32_t mode, float fill0, float fill1, const float* noise0,
                      const float* noise1, const float* sigma, float* y0, float* y1, void* stream);

/* ---- the backward of mpgan_affine_warp in x, CONSTANT mode (pair_augment.hip) ----
 * gy: contiguous fp32 [n][oD][oH][oW], the gradient of the forward's output; gx: [n][D][H][W], the gradient of its
 * input, overwritten everywhere.  in_dhw, out_dhw, theta as for mpgan_affine_warp (in = the forward's input).  The
 * exact adjoint of the CONSTANT forward in x (`fill` is a constant and gets no gradient):
 *   c(p)    = A p + t, evaluated by the forward's own expression: A[k][0]*d + (A[k][1]*h + A[k][2]*w + A[k][3])
 *   tent(u) = 1 - |u| if |u| < 1, else 0 (also 0 for NaN)
 *   g_x[q]  = sum over output voxels p of g_y[p] * tent(c_d(p) - q_d) * tent(c_h(p) - q_h) * tent(c_w(p) - q_w)
 * Weights, products and the sum are fp64, rounded to fp32 once.  A term whose weight is exactly 0 is not read and not
 * added; the terms of one q are added in increasing linear order of p.  An integer-valued (A | t) therefore gives a
 * permuted copy of g_y, with zeros where no p lands.
 * Launch: one gather kernel, one thread per input voxel q on mpgan_affine_warp's tiles (of the input extent).  Per
 * sample the 3 x 3 inverse of A gives p* = A^-1 (q - t) and the half-extents r_k = sum_j |A^-1[k][j]|; a contributor has
 * |p_k - p*_k| < r_k, and along w the three conditions |c_k(p) - q_k| < 1 are intersected to one interval per (p_d, p_h).
 * No atomics and no order that depends on scheduling: two runs give the same bits, and a sample's gx does not depend
 * on the other samples of its batch.
 * Bounded work for any theta: a sample is supported when det A is finite and non-zero and every
 * r_k <= MPGAN_WARP_REACH_MAX (every theta of A = F R / s with s < 2 is: r_k <= 2 sqrt(3)).  An unsupported sample gets
 * NaN over its whole gx and no candidate loop; the other samples of the batch are unaffected.  So a voxel visits at
 * most 9 candidates per axis whatever theta holds.  (A supported A with a NaN or infinite t maps every p to a NaN c or
 * outside: zeros.)
 * MPGAN_ERR_INVALID before any launch: a null gy / gx / theta / in_dhw / out_dhw, n <= 0, an extent < 1, an unknown
 * mode, MPGAN_WARP_BORDER (a clamped coordinate sends gradient from arbitrarily far away to the faces: that adjoint is
 * not built), n * N_in or n * N_out >= 2^31. */
#define MPGAN_WARP_REACH_MAX 4.0
int mpgan_affine_warp_backward(const float* gy, int32_t n, const int32_t* in_dhw, const int32_t* out_dhw,
                               const double* theta, int32_t mode, float* gx, void* stream);

/* ---- the gradient of mpgan_affine_warp in theta, CONSTANT mode (pair_augment.hip) ----
 * x0, x1: the forward's inputs [n][D][H][W]; gy0, gy1: the gradients of its outputs [n][oD][oH][oW]; x1 and gy1 are both
 * given or both null (one plane).  gtheta: double [n][12], row-major [k][j] like theta, overwritten.  in_dhw, out_dhw,
 * theta, fill0, fill1 as for the forward.  Per sample and output voxel p = (d, h, w), with P = (d, h, w, 1):
 *   c        = A p + t by the forward's own expression, A[k][0]*d + (A[k][1]*h + A[k][2]*w + A[k][3]); c' = c clamped to
 *              [-1, S_k] per axis (the forward's CONSTANT clamp); b = floor(c'), f = c' - b
 *   v_ijl    = x[b + (i, j, l)] where that index lies inside the input, else fill.  ALL eight corners count, also those
 *              whose forward weight is exactly 0: the forward skips them, the derivative may not.  At an integer
 *              coordinate this makes the derivative the right-hand one, on the cell [b, b + 1].
 *   dy/dc_w  = lerp_d(lerp_h(v001 - v000, v011 - v010; f_h), lerp_h(v101 - v100, v111 - v110; f_h); f_d), and the d and h
 *              derivatives alike with the axes exchanged; lerp(a, b; f) = a + f (b - a)
 *   dead     a voxel with any c_k NaN or outside [-1, S_k]: all three derivatives are 0 (every corner around it is
 *              fill) and nothing is read for it
 *   g_theta[k][j] = sum_p (sum_planes gy_plane[p] * dy_plane/dc_k(p)) * P_j(p)
 * Everything is fp64 and nothing is rounded to fp32.  Any theta is legal; a NaN entry kills every voxel it reaches (a
 * sample with one gets zeros where its c is NaN).  A 2-D image (D = 1) is no special case: the j = 0 column is 0 because
 * d = 0, and the k = 0 row follows the rule above (its d corner pair is (x, fill)); the 2-D parametrisations never read
 * it.
 * Launches: two, no atomics.  (1) On the forward's tiles of the output (4 x 8 x 32, D = 1: 1 x 8 x 32), one thread per
 * (h, w) walking the tile's d steps: a thread adds its 12 products in increasing d, the block sums each entry in a
 * fixed order through LDS (16 threads per entry add 16 strided values each in index order, then fold by xor butterfly)
 * and stores 12 doubles to ws[sample][tile][12].  (2) One block per sample and entry: thread t adds tiles t, t + 256, ..
 * in order, then a fixed tree over the 256 threads.  Grid and orders depend on (n, out_dhw) alone: two runs give the
 * same bits, whatever ws held, and a sample's g_theta does not depend on the rest of its batch.  Coordinates, cell and
 * fractions are computed once per voxel for both planes.
 * mpgan_affine_warp_theta_workspace: the bytes of ws (n * tiles * 12 doubles), -1 for bad geometry.
 * MPGAN_ERR_INVALID before any launch: a null x0 / gy0 / theta / gtheta / in_dhw / out_dhw, x1 without gy1 or the
 * reverse, n <= 0, an extent < 1, an unknown mode, MPGAN_WARP_BORDER (the clamp of c makes it another function of theta:
 * that gradient is not built), a null, short or misaligned (8 bytes) ws, n * N_in or n * N_out >= 2^31. */
int64_t mpgan_affine_warp_theta_workspace(int32_t n, const int32_t* out_dhw);
int mpgan_affine_warp_backward_theta(const float* x0, const float* x1, const float* gy0, const float* gy1, int32_t n,
                                     const int32_t* in_dhw, const int32_t* out_dhw, const double* theta, int32_t mode,
                                     float fill0, float fill1, void* ws, int64_t ws_bytes, double* gtheta, void* stream);

/* ---- elastic deformation and MRI intensity augmentation of the same pair (pair_augment.hip) ----
 * mpgan_affine_warp with a smooth non-rigid displacement added to the map (both planes alike) and, per plane, a smooth
 * multiplicative bias field and a gamma change.  Every argument the two share means what it means above.  Per output
 * voxel p = (d, h, w) of sample s, in fp64 with one rounding to fp32 at the end:
 *   c      = (A p + t) + u(p)                    A p + t computed as mpgan_affine_warp computes it, u added afterwards;
 *                                                u: cubic B-spline free-form deformation, in input voxels, (d, h, w) order
 *   v_k    = trilinear(x_k, c)                   CONSTANT / BORDER and fill_k as above
 *   v_k   += (v_k - lo) * expm1(b(p))            planes of gain_planes only (bit 1 = plane 0, bit 2 = plane 1);
 *                                                b: cubic B-spline of a scalar log-gain lattice; skipped where expm1(b) == 0
 *   v_k    = lo + R * pow(max(v_k - lo, 0) / R, gamma[s][k])      R = hi - lo; skipped when gamma[s][k] == 1.0 exactly
 *   y_k[p] = v_k + sigma[s][k] * noise_k[p]      as above
 * Device tables (nothing is read on the host), each lattice with an int32 size triple of its own (read on the host):
 *   ctrl:  double [n][3][g_d][g_h][g_w], control displacements of the (d, h, w) coordinate; ctrl_dhw = (g_d, g_h, g_w)
 *   gain:  double [n][b_d][b_h][b_w], control values of the log-gain; gain_dhw = (b_d, b_h, b_w)
 *   gamma: double [n][2], the exponent of plane 0 and plane 1 (> 0)
 * Each of the three may be null: its term is then absent, not zero.
 * Lattice rule, the same for both lattices, over the OUTPUT extent S = out_dhw.  On an axis with S_k == 1 the lattice
 * extent must be 1: the axis has the single weight 1 and u_k = 0 there (2-D images: g_d = 1).  On every other axis
 * 4 <= g_k <= 64 and
 *   xi = 1 + p_k (g_k - 3) / (S_k - 1);   i = min(floor(xi), g_k - 3);   f = xi - i   (in [0, 1])
 *   value = sum over a = 0..3 (per axis) of B_a(f) * lattice[i + a - 1]
 *   B_0 = (1 - f)^3 / 6,  B_1 = (3 f^3 - 6 f^2 + 4) / 6,  B_2 = (-3 f^3 + 3 f^2 + 3 f + 1) / 6,  B_3 = f^3 / 6
 * so one control point lies beyond each face and the spacing is delta_k = (S_k - 1) / (g_k - 3) voxels.  The weights
 * are >= 0 and sum to 1; control displacements below about 0.4 delta_k cannot fold the map p + u(p).  The order of the
 * 64 terms is not part of the definition.
 * Consequences: all-zero ctrl, all-zero gain and gamma == 1 give the bits of mpgan_affine_warp on the same arguments;
 * a sampled value of exactly lo stays exactly lo under gain and gamma (background stays background; noise may then
 * move it); one plane and two planes give the same bits per plane; gain_planes leaves the other plane untouched.
 * Launch: one kernel on mpgan_affine_warp's tiles.  For each d step of its tile a block reduces the d and h sums of
 * both lattices once per (d, h) row into LDS (<= 16 KiB); a voxel then adds 4 terms per channel.  No atomics; the grid
 * depends on (n, out_dhw) alone and every sum has a fixed order: two runs give the same bits.
 * MPGAN_ERR_INVALID before any launch: everything mpgan_affine_warp refuses; a lattice pointer without its size
 * triple; a lattice extent that breaks the rule; gain with gain_planes == 0; gain_planes naming plane 1 without x1;
 * unknown gain_planes bits; hi <= lo when gain or gamma is given. */
int mpgan_deform_warp(const float* x0, const float* x1, int32_t n, const int32_t* in_dhw, const int32_t* out_dhw,
                      const double* theta, const double* ctrl, const int32_t* ctrl_dhw, const double* gain,
                      const int32_t* gain_dhw, int32_t gain_planes, const double* gamma, double lo, double hi,
                      int32_t mode, float fill0, float fill1, const float* noise0, const float* noise1,
                      const float* sigma, float* y0, float* y1, void* stream);

/* ---- optimiser ------------------------------------------------------------ */
/* torch.optim.Adam.step over one flat buffer (GAN_final.py:306-307):
 * m = b1*m+(1-b1)*g; v = b2*v+(1-b2)*g^2; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t)+eps).
 * grad_scale multiplies g first (1/world_size after a sum all-reduce).  Hyper-parameters are
 * doubles (python floats), rounded to fp32 where torch rounds them. */
int mpgan_adam_step(float* p, const float* g, float* m, float* v, int64_t numel,
                    double lr, double b1, double b2, double eps, int32_t step, float grad_scale,
                    void* stream);

/* The step's optional extras (optim_ops.hip); mpgan_adam_step above is the default step and unchanged.
 *
 * Global gradient norm and torch.nn.utils.clip_grad_norm_'s coefficient, both left on the device:
 *   out2[0] = (float)sqrt(sum_i (double)(fl32(g_i * grad_scale))^2)    the product in fp32, as Adam loads it; its
 *                                                                       square and every sum in fp64
 *   out2[1] = max_norm > 0 ? min(1, max_norm / (out2[0] + 1e-6f)) : 1   in fp32; a non-finite norm propagates as in torch
 * Two launches (block partials, then one finalising block), no atomics, a partial count that depends on numel alone:
 * two runs give the same bits.  16-byte loads when g is 16-byte aligned (scalar tail), element-wise otherwise.
 * ws: >= mpgan_grad_norm_workspace(numel) bytes, 8-byte aligned.  MPGAN_ERR_INVALID before any launch: numel <= 0, a
 * null g / ws / out2, a short or misaligned workspace. */
int64_t mpgan_grad_norm_workspace(int64_t numel);
int mpgan_grad_norm(const float* g, int64_t numel, float grad_scale, float max_norm, void* ws, int64_t ws_bytes,
                    float* out2, void* stream);
/* mpgan_adam_step with, when `coef` (one device float, e.g. out2 + 1 above) is given, the gradient also multiplied by
 * *coef: gi = g[i] * fl32(grad_scale * *coef), clipping without a host sync.  (The two factors are multiplied first:
 * a coefficient of exactly 1.0f then changes no bit, whatever grad_scale is.)  With coef == NULL and ema == NULL the
 * results equal mpgan_adam_step's bit for bit.  When `ema` is given, ema[i] = lerp(ema[i], p_new[i], ema_weight) in torch's form (w < 0.5: e + w*(p-e), else
 * p - (p-e)*(1-w)) while the new parameter is still in a register; ema_weight = 1 - decay, in [0, 1].
 * Any numel > 0 and any 4-byte alignment: 16-byte accesses when p, g, m, v (and ema) are all 16-byte aligned. */
int mpgan_adam_step_ex(float* p, const float* g, float* m, float* v, int64_t numel,
                       double lr, double b1, double b2, double eps, int32_t step, float grad_scale,
                       const float* coef /* device, may be NULL */, float* ema /* may be NULL */, float ema_weight,
                       void* stream);
/* EMA of a network's buffers into its twin's in one launch.  table: device int64 [n_entries][4] =
 * {src_ptr, dst_ptr, numel, kind}; kind 0: fp32, dst = lerp(dst, src, ema_weight) as above; kind 1: int64, dst = src
 * (BatchNorm's num_batches_tracked).  max_elems: the largest numel of the table.  n_entries == 0 returns 0 without a
 * launch. */
int mpgan_ema_buffers(const int64_t* table, int32_t n_entries, int64_t max_elems, float ema_weight, void* stream);

/* ---- patch gather / scatter (variant B, test_runs/GAN.py:263-272,313-337) -- */
/* patches[(b*S+s)][roi^dims] = vol[b][corner+...]; bit-exact copy.
 * corners: device int32 [B*S][3] (z,y,x). */
int mpgan_patch_gather(const float* vol, int32_t b, const int32_t dhw[3],
                       const int32_t* corners, int32_t samples, const int32_t roi[3],
                       float* patches, void* stream);
/* dvol[b][corner+...] += dpatches (atomic-free: one thread per volume voxel
 * walks the corners that cover it, in sample order => deterministic). */
int mpgan_patch_scatter_add(const float* dpatches, int32_t b, const int32_t dhw[3],
                            const int32_t* corners, int32_t samples, const int32_t roi[3],
                            float* dvol, void* stream);

/* ---- BatchNorm statistics without a finalize launch (the generator's forward chain) ----------------------
 * A conv leaves per-channel fixed-point sums (sum y, sum y^2) of its raw output in integer accumulators
 * `acc` = int64 [replicas][MPGAN_ACC_WORDS][cstride] (zeroed by the caller before the producing launch;
 * order-independent, hence reproducible); the FIRST consumer of those statistics folds them at block start
 * (mpgan_norm_fold), publishes scale / shift / mean / invstd and advances the running statistics -- what
 * mpgan_norm_finalize does, without its launch.  See csrc/norm_fold.h. */
#define MPGAN_ACC_WORDS 4
typedef struct {
  const int64_t* acc;        /* null => no fold: the prologue's own scale / shift are used */
  int32_t replicas;
  int32_t cstride;           /* channels per accumulator row (>= the c channels the norm covers) */
  int64_t count;             /* elements per channel (N*D*H*W) */
  const float* gamma;
  const float* beta;
  float eps, momentum;
  float* running_mean;       /* nullable */
  float* running_var;
  int64_t* num_batches_tracked;
  float* scale;              /* outputs, written by one block of the consuming launch */
  float* shift;
  float* mean;
  float* invstd;
} mpgan_norm_fold;

/* Zero `bytes` bytes at ptr on the stream (the accumulators of all norm layers of a plan: one call per forward). */
int mpgan_zero_bytes(void* ptr, int64_t bytes, void* stream);
/* 1 if the kernel serving this conv can leave accumulators (stats_acc) / can fold them on load (fold). */
int32_t mpgan_conv_acc_supported(const mpgan_conv_geom* g, int32_t has_prologue);
int32_t mpgan_conv_fold_supported(const mpgan_conv_geom* g);
/* mpgan_conv_forward with either form of statistics on either side: `fold` (nullable) replaces pro->scale/shift
 * (pro still carries act / slope / slope_ptr); stats_acc (nullable, exclusive with stats_partials) receives this
 * conv's sums with `acc_replicas` replicas of Cout-wide rows. */
int mpgan_conv_forward_fold(const mpgan_conv_geom* g, const float* x, int32_t ldx, const float* w_packed,
                            const float* bias, const mpgan_prologue* pro, const mpgan_norm_fold* fold,
                            const float* resid, int32_t ldr, int32_t tanh_out, float* stats_partials,
                            int64_t* stats_acc, int32_t acc_replicas, float* y, int32_t ldy, void* stream);
/* mpgan_norm_act_add whose z-side scale / shift come from accumulators (fold_z; pz carries act / slope). */
int mpgan_norm_act_add_fold(const float* z, int32_t ldz, const mpgan_prologue* pz, const mpgan_norm_fold* fold_z,
                            const float* r, int32_t ldr, const mpgan_prologue* pr, int32_t n,
                            int64_t pixels_per_sample, int32_t c, int32_t tanh_out, float* out, int32_t ldo,
                            void* stream);

/* ---- bf16 storage path (BASELINE config C5: the reference's own 3-D graph, GAN_final.py:106-114,167-189) ----
 * Activations, activation gradients and packed weights are bf16 in HBM (void* below); products accumulate in fp32
 * on v_mfma_f32_32x32x16_bf16; BatchNorm statistics, parameters, weight gradients and Adam stay fp32.
 * There is no normalise-on-load prologue in this path: a layer's BatchNorm + LeakyReLU output is materialised
 * once by mpgan_norm_act_bf16 (see conv_bf16.hip for why) and convolutions read plain activations. */

/* y (bf16) = conv(x (bf16)) + bias; gathered channels % 64 == 0, output channels % 8 == 0, <= 32 taps per phase.
 * stats_partials (nullable): per-tile partial sums [rows][2][Cout] of (y, y^2) in fp32 taken before rounding,
 * rows = mpgan_conv_stats_rows_bf16(); consumed by mpgan_norm_finalize(n=1, chunks=rows, pixels=N*D*H*W). */
int32_t mpgan_conv_stats_rows_bf16(const mpgan_conv_geom* g);
int mpgan_conv_forward_bf16(const mpgan_conv_geom* g, const void* x, int32_t ldx, const void* w_packed,
                            const float* bias, float* stats_partials, void* y, int32_t ldy, void* stream);
/* Which bf16 kernel serves this geometry (the forward: with statistics): 0 = the K-stepped gather kernel,
 * 1 = the patch form for stride-1 3x3x3 gathers (D.conv2 forward / backward-data at config C5),
 * 2 / 3 / 4 = the wide K-stepped form: 256 x 256 tiles, 512 x 128 tiles, 256 x 256 tiles over pairs of phases of a
 * strided backward-data gather (D.conv3 / D.conv4 at config C5), 5 = the big-patch form (8 x 8 x 8 tiles).
 * mpgan_conv_kernel_name_bf16 writes the profiling label of the same launch, like mpgan_conv_kernel_name.  Both, the
 * row queries and the launch read one choice (choose_bf16, conv_bf16.hip). */
int32_t mpgan_conv_variant_bf16(const mpgan_conv_geom* g, int32_t backward_data);
int mpgan_conv_kernel_name_bf16(const mpgan_conv_geom* g, int32_t backward_data, char* buf, int32_t len);

/* dx (bf16) = conv_backward_data(dy (bf16)); w_packed_bwd: bf16, layout 1 of mpgan_pack_weights_bf16. */
int mpgan_conv_backward_data_bf16(const mpgan_conv_geom* g, const void* dy, int32_t lddy, const void* w_packed_bwd,
                                  void* dx, int32_t lddx, void* stream);
/* Eval-mode forward in bf16 storage (Discriminator / PatchDiscriminator after .eval()): with running-statistics
 * BatchNorm the layer's affine is known before its conv runs, so the epilogue of the bf16 forward applies it and the
 * LeakyReLU to the fp32 MFMA accumulator of bf16 x and bf16 w,
 *     y = lrelu(acc * scale[c] + shift[c], slope[c]),
 * and the ACTIVATED tensor is stored once: rounded to bf16 (to nearest even), or unrounded as fp32 when y_f32 != 0
 * (the layer the fp32 Linear head reads; ldy % 4 == 0 then).  No raw z reaches memory and no mpgan_norm_act_bf16 pass
 * follows.  The conv's bias is folded into `shift` by the caller (mpgan_epi_vectors_multi does it; a LeakyReLU's constant
 * slope is passed to it as a one-element device tensor in the PReLU column).  scale / shift / slope: [cout] floats,
 * 16-byte aligned.  Runs on whichever form serves mpgan_conv_forward_bf16 for this geometry (mpgan_conv_variant_bf16,
 * mpgan_conv_kernel_name_bf16).  Fused statistics describe the raw conv output, which this launch never forms:
 * stats_partials must be NULL (MPGAN_ERR_INVALID otherwise). */
int mpgan_conv_forward_act_bf16(const mpgan_conv_geom* g, const void* x, int32_t ldx, const void* w_packed,
                                const float* scale, const float* shift, const float* slope, float* stats_partials,
                                void* y, int32_t ldy, int32_t y_f32, void* stream);
/* The same for the 1-input-channel first layer: fp32 image in, activated bf16 out (mpgan_conv_forward_f32_to_bf16's
 * kernels with the epilogue activation). */
int mpgan_conv_forward_act_f32_to_bf16(const mpgan_conv_geom* g, const float* x, int32_t ldx, const float* w_packed,
                                       const float* scale, const float* shift, const float* slope,
                                       float* stats_partials, void* y, int32_t ldy, void* stream);
/* kernel label of the bf16 weight gradient of this layer: 0 = 128 x 256 tiles, 1 = 256 x 256 (profiling only) */
int32_t mpgan_conv_wgrad_variant_bf16(const mpgan_conv_geom* g);
/* dW (fp32, torch layout) = beta*dW + sum over pixels of dy (bf16) x gathered x (bf16): pad-free ConvNd. */
int64_t mpgan_conv_wgrad_workspace_bf16(const mpgan_conv_geom* g);
int mpgan_conv_backward_weight_bf16(const mpgan_conv_geom* g, const void* x, int32_t ldx, const void* dy, int32_t lddy,
                                    float* dw, float beta, void* workspace, int64_t workspace_bytes, void* stream);
/* The 1-input-channel first layer (Discriminator.model_conv[0]): fp32 image in / bf16 raw output out, its
 * backward-data (bf16 dy -> fp32 dx) and its weight gradient with a bf16 dy (HBM-bound VALU kernels; packed
 * weights fp32 as in the fp32 path). */
int mpgan_conv_forward_f32_to_bf16(const mpgan_conv_geom* g, const float* x, int32_t ldx, const float* w_packed,
                                   const float* bias, float* stats_partials, void* y, int32_t ldy, void* stream);
int mpgan_conv_backward_data_bf16_to_f32(const mpgan_conv_geom* g, const void* dy, int32_t lddy,
                                         const float* w_packed_bwd, float* dx, int32_t lddx, void* stream);
int64_t mpgan_conv_wgrad_workspace_bf16dy(const mpgan_conv_geom* g);
int mpgan_conv_backward_weight_bf16dy(const mpgan_conv_geom* g, const float* x, int32_t ldx, const void* dy,
                                      int32_t lddy, float* dw, float* dbias, float beta, void* workspace,
                                      int64_t workspace_bytes, void* stream);
/* mpgan_pack_weights with a bf16 destination (same table; layouts 0 and 1; dst offsets in elements). */
int mpgan_pack_weights_bf16(const float* flat_params, void* packed, const int64_t* table, int32_t n_entries,
                            int64_t max_elems, void* stream);
/* out = LeakyReLU_slope(z*scale[c] + shift[c]) over [rows][C] bf16 z; out is bf16, or fp32 when out_f32 != 0
 * (the tensor the fp32 Linear head reads).  (nn.BatchNorm3d + nn.LeakyReLU(0.2), GAN_final.py:170-171.) */
int mpgan_norm_act_bf16(const void* z, int32_t ldz, const float* scale, const float* shift, float slope, int64_t rows,
                        int32_t c, void* out, int32_t ldo, int32_t out_f32, void* stream);
/* BatchNorm + LeakyReLU backward on bf16 z, given g = dL/da (bf16, or fp32 when g_f32 != 0):
 *   reduce: partial rows [mpgan_norm_bwd_rows_bf16()][3][C] for mpgan_norm_bwd_finalize(n=1, chunks=rows, P=rows_total);
 *   apply : dz (bf16) = scale*(gy - c1 - zhat*c2); bias_partials (nullable) receives per-block column sums
 *           [mpgan_norm_bwd_rows_bf16()][C] of the stored dz (the conv's bias gradient, reduce with mpgan_reduce_partials). */
/* Backward-data of the bf16 path + the reduce pass of the BatchNorm + LeakyReLU(slope) in front of the conv's input in one
 * launch (as mpgan_conv_backward_data_stats does for fp32): dx (bf16) is the gradient w.r.t. a = act(scale * z + shift);
 * partials[mpgan_conv_bwd_stats_rows_bf16(g)][3][cin] receive what mpgan_norm_bwd_reduce_bf16 would form from the STORED
 * dx and z.  rows == 0: this geometry runs on the narrow K-stepped kernel, which has no fused sums.
 * (nn.BatchNorm3d + nn.LeakyReLU(0.2) backward, GAN_final.py:170-171 under autograd.) */
int32_t mpgan_conv_bwd_stats_rows_bf16(const mpgan_conv_geom* g);
int mpgan_conv_backward_data_stats_bf16(const mpgan_conv_geom* g, const void* dy, int32_t lddy, const void* w_packed_bwd,
                                        void* dx, int32_t lddx, const void* z, int32_t ldz, const float* scale,
                                        const float* shift, const float* mean, const float* invstd, float slope,
                                        float* partials, void* stream);
int32_t mpgan_norm_bwd_rows_bf16(int64_t rows, int32_t c);
int mpgan_norm_bwd_reduce_bf16(const void* g, int32_t g_f32, int32_t ldg, const void* z, int32_t ldz, const float* scale,
                               const float* shift, const float* mean, const float* invstd, float slope, int64_t rows,
                               int32_t c, float* partials, void* stream);
int mpgan_norm_bwd_apply_bf16(const void* g, int32_t g_f32, int32_t ldg, const void* z, int32_t ldz, const float* scale,
                              const float* shift, const float* mean, const float* invstd, const float* c1,
                              const float* c2, float slope, int64_t rows, int32_t c, void* dz, int32_t lddz,
                              float* bias_partials, void* stream);

/* Variant B (the patch discriminator, test_runs/GAN.py:136-198,288-298) in bf16 storage: the perceptual taps of a
 * layer are defined on the STORED bf16 raw conv output z: y = z*scale + shift and a = LeakyReLU(y) in fp32. */
typedef struct {
  const void* z_peer;       /* the other pass's stored bf16 raw conv output, same shape */
  int32_t ld_peer;
  const float* scale_peer;  /* its norm scale / shift (per channel) */
  const float* shift_peer;
  const float* coef;        /* device float[3]: (z, y, a) gradient coefficients; required */
} mpgan_peer_taps_bf16;

/* mpgan_norm_bwd_reduce_bf16 / _apply_bf16 with the peer-tap terms of mpgan_norm_bwd_reduce / _apply:
 *   g_a = g - c_a*sign(a_peer - a);  gy = g_a*act'(y) - c_y*sign(y_peer - y);  dz += -c_z*sign(z_peer - z).
 * Same partial rows, bias partials and g_f32 switch as the entries without peer. */
int mpgan_norm_bwd_reduce_bf16_peer(const void* g, int32_t g_f32, int32_t ldg, const void* z, int32_t ldz,
                                    const float* scale, const float* shift, const float* mean, const float* invstd,
                                    const mpgan_peer_taps_bf16* peer, float slope, int64_t rows, int32_t c,
                                    float* partials, void* stream);
int mpgan_norm_bwd_apply_bf16_peer(const void* g, int32_t g_f32, int32_t ldg, const void* z, int32_t ldz,
                                   const float* scale, const float* shift, const float* mean, const float* invstd,
                                   const float* c1, const float* c2, const mpgan_peer_taps_bf16* peer, float slope,
                                   int64_t rows, int32_t c, void* dz, int32_t lddz, float* bias_partials, void* stream);
/* mpgan_tap_l1 over two passes' bf16 z (C % 8, pitches % 8, 16-byte aligned), each with its fp32 scale / shift:
 * out3 = (mean|z_a-z_b|, mean|y_a-y_b|, mean|a_a-a_b|), a = LeakyReLU_slope(y); partials >= mpgan_tap_l1_partials()
 * floats.  A fixed-order two-stage reduction without atomics: the result is reproducible. */
int mpgan_tap_l1_bf16(const void* za, int32_t lda, const float* scale_a, const float* shift_a, const void* zb,
                      int32_t ldb, const float* scale_b, const float* shift_b, float slope, int64_t rows, int32_t c,
                      float* partials, float* out3, void* stream);

/* ---- conditional (pix2pix) discriminator: the first conv over two input planes ----------------------------------
 * D(cat(image, condition)): model_conv[0] is Conv(2, 64, 3, stride 1, no padding), and its two input channels are two
 * SEPARATE dense 1-channel fp32 tensors (N, D, H, W), x_img (plane 0: the generated or real T2) and x_cond (plane 1:
 * the T1 it belongs to); no concatenated or interleaved tensor is materialised.  g describes the ConvNd itself
 * (cin == 2, cout == 64, 3x3 with depth 1 or 3x3x3, stride 1, pad 0, at least 4 output columns); every other geometry
 * is MPGAN_ERR_UNSUPPORTED with a message, before any launch.  w_packed: layout 0 of mpgan_pack_weights,
 * [64][tap][2], 8-byte aligned, so that weight[:, 0] of a conditional checkpoint is what an unconditional conv1 holds.
 * One row-walking VALU kernel, lane = output channel (thin_cin2_rows_kernel, conv_igemm.hip): each output pixel's 64
 * channels are stored once.
 * Replaces: Discriminator.model_conv[0] (GAN_final.py:167-169) applied to torch.cat([img, cond], 1), the conditional
 * discriminator of pix2pix (the paper GAN_final.py:125 cites); the reference itself has no such call.
 *
 * mpgan_conv2p_forward:  y (fp32) = conv + bias.  stats_partials must be NULL: as for the one-plane 1 -> 64 layer the
 *   fp32 launch leaves no fused statistics (mpgan_conv2p_stats_rows(g, 0) == 0; use mpgan_channel_stats).
 * mpgan_conv2p_forward_f32_to_bf16:  y (bf16) = conv + bias, rounded once; stats_partials (nullable) receives
 *   mpgan_conv2p_stats_rows(g, 1) rows [2][64] of (sum y, sum y^2) taken in fp32 before rounding, one per block of the
 *   launch, each pixel counted once; feed them to mpgan_norm_finalize(n = 1, chunks = rows).
 * mpgan_conv2p_forward_act / _act_f32_to_bf16:  eval mode, y = lrelu(conv * scale[c] + shift[c], slope[c]) stored once
 *   as fp32 / bf16 (mpgan_conv_forward_act's contract: the bias is folded into shift); stats_partials must be NULL.
 * mpgan_conv2p_kernel_name: the profiling label of those launches (out_bf16: of the _f32_to_bf16 ones), written like
 *   mpgan_conv_kernel_name's; rows, label and launch read one choice (choose_gather, conv_igemm.hip). */
int32_t mpgan_conv2p_stats_rows(const mpgan_conv_geom* g, int32_t out_bf16);
int mpgan_conv2p_kernel_name(const mpgan_conv_geom* g, int32_t out_bf16, char* buf, int32_t len);
int mpgan_conv2p_forward(const mpgan_conv_geom* g, const float* x_img, const float* x_cond, const float* w_packed,
                         const float* bias, float* stats_partials, float* y, int32_t ldy, void* stream);
int mpgan_conv2p_forward_act(const mpgan_conv_geom* g, const float* x_img, const float* x_cond, const float* w_packed,
                             const float* scale, const float* shift, const float* slope, float* y, int32_t ldy,
                             void* stream);
int mpgan_conv2p_forward_f32_to_bf16(const mpgan_conv_geom* g, const float* x_img, const float* x_cond,
                                     const float* w_packed, const float* bias, float* stats_partials, void* y,
                                     int32_t ldy, void* stream);
int mpgan_conv2p_forward_act_f32_to_bf16(const mpgan_conv_geom* g, const float* x_img, const float* x_cond,
                                         const float* w_packed, const float* scale, const float* shift,
                                         const float* slope, float* stats_partials, void* y, int32_t ldy, void* stream);
/* dW (fp32, torch layout (64, 2, k...)) = beta*dW + sum over pixels, both planes from ONE pass over dy; dbias
 * (nullable) = beta*dbias + colsum(dy), fused.  dy: fp32, or bf16 when dy_bf16 != 0 (converted on load).  Per-block
 * partial slabs in `workspace` (>= mpgan_conv2p_wgrad_workspace(g) bytes; -1: geometry refused), then the fixed-order
 * slab reducer of mpgan_conv_backward_weight: two runs give the same bits.  mpgan_conv2p_wgrad_kernel_name: the label,
 * from the same choice (choose_wgrad, conv_wgrad.hip).
 * Replaces: the autograd weight / bias gradient of that conv under loss.backward() (GAN_final.py:296).
 * There is no gradient for the condition (it is data), and the image plane's input gradient needs no entry of its
 * own: mpgan_conv_backward_data / mpgan_conv_backward_data_bf16_to_f32 with the geometry's cin set to 1 and the
 * layout-3 pack of mpgan_pack_weights ([tap][cout] of weight[:, 0]). */
int64_t mpgan_conv2p_wgrad_workspace(const mpgan_conv_geom* g);
int mpgan_conv2p_wgrad_kernel_name(const mpgan_conv_geom* g, int32_t bf16_dy, char* buf, int32_t len);
int mpgan_conv2p_backward_weight(const mpgan_conv_geom* g, const float* x_img, const float* x_cond, const void* dy,
                                 int32_t lddy, int32_t dy_bf16, float* dw, float* dbias, float beta, void* workspace,
                                 int64_t workspace_bytes, void* stream);

/* ---- sliding-window inference (MONAI 0.4.0 sliding_window_inference; code/GAN/minipig_inference.py:110-114) --
 * An image batch (B, C, D, H, W) contiguous fp32 (2-D: D = 1) is padded per dim by pad_lo before / the rest after
 * up to `padded` (never materialised: out-of-range reads give cval), covered by the windows start_z x start_y x
 * start_x (meshgrid "ij": z slowest) and each window batch goes through the caller's predictor.  Global window
 * index i = b * num_win + w (image-major).  The start table lives in device memory (`starts_dev`, the kernels read
 * it) and is mirrored on the host (`starts_host`, validated before any launch: 0 <= start <= padded - roi).
 * Element offsets are 64-bit.  Every thread owns its output elements: no atomics, deterministic results. */
typedef struct {
  int32_t batch;               /* B */
  int32_t dhw[3];              /* image extent */
  int32_t pad_lo[3];           /* padding before each dim */
  int32_t padded[3];           /* padded extent (>= dhw + pad_lo, >= roi) */
  int32_t roi[3];              /* window extent */
  int32_t num[3];              /* window starts per dim */
  const int32_t* starts_dev;   /* device int32[num[0] + num[1] + num[2]]: z starts, then y, then x (padded coords) */
  const int32_t* starts_host;  /* the same table on the host */
} mpgan_sw_geom;

/* win[k] (k < n, contiguous (n, cin, roi)) = padded image of global window first + k. */
int mpgan_sw_gather(const mpgan_sw_geom* g, const float* in, int32_t cin, int32_t first, int32_t n, float cval,
                    float* win, void* stream);
/* count[padded] (one spatial map for every image and channel) = sum of imp over the windows covering each voxel,
 * in window order.  imp: device (roi) fp32 importance map; null => constant 1. */
int mpgan_sw_count(const mpgan_sw_geom* g, const float* imp, float* count, void* stream);
/* acc (B, cout, padded), zeroed by the caller before the first call: for global windows first .. first+n-1 in order,
 * acc[b, :, win] = acc + imp * pred[k] (one rounded product, one rounded add).  pred: contiguous (n, cout, roi). */
int mpgan_sw_blend(const mpgan_sw_geom* g, const float* pred, int32_t cout, int32_t first, int32_t n, const float* imp,
                   float* acc, void* stream);
/* out (B, cout, dhw) = acc / count over the unpadded region (IEEE division). */
int mpgan_sw_finalize(const mpgan_sw_geom* g, const float* acc, int32_t cout, const float* count, float* out,
                      void* stream);
/* The profiler's name (without `void mpgan::` and the argument list, e.g. "sw_gather_kernel<true, false>") of the
 * kernel instance one of the four launches above runs, written to buf[len] from the same choice the launch makes.
 * Each launch has several forms (16-byte quads or scalars, constant or given importance map) and picks one from
 * the geometry (roi, padded extent, x starts, image width and x padding modulo 4) and from the 16-byte alignment of
 * its buffers; a buffer that is not 16-byte aligned sends its launch to the scalar form, except the gather's window
 * batch, which must be aligned when roi[2] % 4 == 0 (MPGAN_ERR_UNSUPPORTED otherwise, as from the launch).
 * p0..p2 are that launch's data pointers in its own argument order:
 *   MPGAN_SW_GATHER: in, win, (ignored)    MPGAN_SW_COUNT: imp (null => constant 1), count, (ignored)
 *   MPGAN_SW_BLEND: pred, imp, acc         MPGAN_SW_FINALIZE: acc, count, out
 * Nothing is launched and no data pointer is dereferenced (only starts_host is read); works without a GPU.  The
 * geometry and the required pointers are validated as by the launch, with the launch's status codes. */
enum { MPGAN_SW_GATHER = 0, MPGAN_SW_COUNT = 1, MPGAN_SW_BLEND = 2, MPGAN_SW_FINALIZE = 3 };
int mpgan_sw_kernel_name(int32_t launch, const mpgan_sw_geom* g, const void* p0, const void* p1, const void* p2,
                         char* buf, int32_t len);

/* ---- development aids (no counterpart in the reference) ----------------------------------------------------
 * In-kernel phase stamps: a library built with `make STAMPS=1` records, for each of the next `launches`
 * gather-conv launches, the 100 MHz device clock at every block's phase boundaries into
 * buf[launch][blocks_per_launch][12] (uint64; blocks beyond the cap do not stamp).  The product build returns
 * MPGAN_ERR_UNSUPPORTED.  mpgan_debug_stamps(NULL, 0, 0) switches stamping off. */
int mpgan_debug_stamps(void* buf, int64_t launches, int64_t blocks_per_launch);
int64_t mpgan_debug_stamps_used(void);
int32_t mpgan_debug_clock_khz(void);
/* (Rounds 2-3 had two process-wide setters here for the launch size from which the big-tile forms are used;
 *  since ABI version 2 that threshold is the geometry's own `min_blocks` field: no mutable dispatch state.) */

#ifdef __cplusplus
}
#endif
#endif /* MPGAN_HIP_H */
