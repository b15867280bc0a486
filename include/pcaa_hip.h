/*
 * pcaa_hip.h -- C ABI of the MI355X (gfx950) PCAA hot path.
 *
 * The reference (rmazzier/OpenSetGaitRecognition_PCAA) has no FFI: its operator
 * boundary is Python nn.Module.forward + autograd, below which sits PyTorch
 * ATen.  Each entry point here replaces the ATen work behind one reference call
 * site (cited per function as reference file:line).  The Python side
 * (opensetgaitrecognition_pcaa_amd/functional.py) binds them with ctypes and
 * wraps them in torch.autograd.Functions; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless named host_*; nothing is
 *     allocated, freed or synchronised inside a call (graph-capture safe);
 *   - `stream` is a hipStream_t passed as void*;
 *   - return value: PCAA_OK, or an error code with a message retrievable from
 *     pcaa_last_error() (thread-local);
 *   - activations are ROW-MAJOR [rows, channels] ("point-major": one row per
 *     point / per (batch,time) step, channels fastest);
 *   - dtype arguments: PCAA_F32 or PCAA_BF16 (storage type of an activation
 *     tensor); parameters, statistics, losses and optimizer state are fp32
 *     (BatchNorm statistics accumulate in fp64).
 */
#ifndef PCAA_HIP_H
#define PCAA_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCAA_ABI_VERSION 29 /* pcaa_abi_version() of a library built from this header */

#define PCAA_OK 0
#define PCAA_ERR_INVALID_ARG 1
#define PCAA_ERR_LAUNCH 2

#define PCAA_F32 0
#define PCAA_BF16 1
#define PCAA_SPLIT_F16 2 /* the [hi | lo] 16-bit image of an fp32 tensor (pcaa_gemm_split3): accepted where a call says so */
#define PCAA_FP8_E4M3 3 /* OCP e4m3fn bytes (not fnuz), no scale: pcaa_gemm_fp8_affine_elu and pcaa_pointnet_in_apply only */

/* operand storage order for pcaa_gemm */
#define PCAA_LAYOUT_KC 0 /* contraction index contiguous: A[m*ld + k], B[n*ld + k] */
#define PCAA_LAYOUT_RC 1 /* row index contiguous:         A[k*ld + m], B[k*ld + n] */

#define PCAA_ACT_NONE 0
#define PCAA_ACT_ELU 1

const char* pcaa_last_error(void);
int pcaa_abi_version(void);

/* ------------------------------------------------------------------ GEMM
 * C[M,N] (=|+=) A(M,K) . B(K,N) (+ bias[N]) on the MFMA pipe.
 *   math = PCAA_F32 : v_mfma_f32_32x32x2_f32 (exact fp32), any operand dtype/layout
 *   math = PCAA_BF16: v_mfma_f32_32x32x16_bf16, fp32 accumulate; operands KC
 * colstats != NULL: per-column sum and sum-of-squares of the bias-free
 *   accumulator over the M rows are added (fp64 atomics) into
 *   colstats[(tile_m % nrep)][2][N] -- the BatchNorm batch statistics of the
 *   layer this GEMM produces.
 * split_k > 1 or accumulate != 0: fp32 atomic accumulation into C (C must be
 *   fp32 and pre-initialised); bias is added by split 0 only.
 * Dispatch: every product entry point (pcaa_gemm, pcaa_gemm_slabs, pcaa_gemm_split3, pcaa_gemm_slabs_split3) first
 *   PLANS the call from its arguments alone -- every argument check and every decision, no device memory read, no HIP
 *   call -- and then launches the planned kernel, one of PCAA_GEMM_KERNEL_*.  The rule for the two 4-wave LDS-DMA loops
 *   is stated once (pcaa_gemm_4wave_kernel, csrc/gemm_bf16.hip); the *_supported predicates ask that same function.
 *   pcaa_gemm_route / pcaa_gemm_split3_route run the plan only and report the kernel (they work without a GPU);
 *   pcaa_gemm_last_kernel reports what the calling thread's most recent GEMM launch actually started.
 * Replaces: Conv2d(1x1) models.py:20-27, Conv1d via im2col models.py:59-68,
 *   Linear models.py:252-277, 346-371, 409-416, and their autograd backward.
 */
#define PCAA_GEMM_KERNEL_F32_TILE128 0 /* gemm_f32_kernel: 128 x 128 tiles, exact-fp32 MFMA, any dtype / layout */
#define PCAA_GEMM_KERNEL_BF16_SMALL 1  /* gemm_bf16_kernel: 128 x 128 tiles, bf16 MFMA, KC operands (csrc/gemm.hip) */
#define PCAA_GEMM_KERNEL_BF16_STAGED 2 /* gemm_bf16_big_kernel: 256 x 256 tiles, operands staged through registers */
#define PCAA_GEMM_KERNEL_V2_KC 3       /* v2::gemm_bf16_v2_kernel: the 4-wave LDS-DMA loop, KC x KC (also the fused entries) */
#define PCAA_GEMM_KERNEL_V2_RC 4       /* v2::gemm_bf16_v2rc_kernel: the 4-wave LDS-DMA loop, RC x RC -> fp32 */
int pcaa_gemm(int math,
              const void* A, int a_dtype, int a_layout, long lda,
              const void* B, int b_dtype, int b_layout, long ldb,
              void* C, int c_dtype, long ldc,
              int M, int N, int K,
              const float* bias, double* colstats, int nrep,
              int split_k, int accumulate, void* stream);

/* Split-K without atomics (the long-K weight-gradient products): split s writes its partial
 * M x N product to slabs + s * slab_stride (fp32), pcaa_splitk_reduce sums the slabs into
 * out (=|+=).  pcaa_gemm_num_splits tells how many splits pcaa_gemm / pcaa_gemm_slabs will
 * actually run for a requested split_k (K is cut into multiples of the kernel's K step). */
int pcaa_gemm_num_splits(int math, int K, int split_k);
/* ABI 21: the plan step alone.  pcaa_gemm_route: the arguments of pcaa_gemm plus slab_stride -- 0: the pcaa_gemm form;
 * non-zero: the pcaa_gemm_slabs form (C = slabs; c_dtype, ldc, bias, colstats, nrep and accumulate are then not looked at,
 * as pcaa_gemm_slabs has none).  pcaa_gemm_split3_route: pcaa_gemm_split3 (split_k = 1, c_split_stride = 0) or
 * pcaa_gemm_slabs_split3 (C = slabs, ldc = N, c_split_stride = slab_stride); out_scale decides nothing.  Both return the PCAA_GEMM_KERNEL_* the
 * launch would take, or -1 with pcaa_last_error() set exactly as the launch would set it.  Pointers are inspected for
 * NULL and alignment only; no HIP call is made.  The launched kernel differs from the planned one in a single case: a
 * 4-wave launcher whose hipFuncSetAttribute fails hands the launch to the register-staged kernel.
 * pcaa_gemm_last_kernel: the PCAA_GEMM_KERNEL_* that the calling thread's most recent GEMM launch (the fused entry
 * points included) started; -1 before any. */
int pcaa_gemm_route(int math,
                    const void* A, int a_dtype, int a_layout, long lda,
                    const void* B, int b_dtype, int b_layout, long ldb,
                    const void* C, int c_dtype, long ldc,
                    int M, int N, int K,
                    const float* bias, const double* colstats, int nrep,
                    int split_k, int accumulate, long slab_stride);
int pcaa_gemm_split3_route(const void* A, const void* B, int layout, long lda, long ldb, const void* C, long ldc, int M,
                           int N, int K, const double* colstats, int nrep, int split_k, long c_split_stride, float out_scale);
int pcaa_gemm_last_kernel(void);
/* ABI 14: n <= 8 small products C_i[M_i, N_i] += A_i^T . B_i in ONE launch (the temporal block's six weight gradients
 * dW_l = dy_l^T . col_l, reference models.py:108-160 through autograd): A_i [K_i, M_i], B_i [K_i, N_i], C_i [M_i, N_i], all
 * fp32 with contiguous rows, 16-B aligned, M_i and N_i multiples of 4; exact-fp32 MFMA; C_i is accumulated into (atomics
 * over split_k[i] ranges of the contraction): the caller zeroes it. */
int pcaa_gemm_group_rc_f32(int n, const void* const* A, const void* const* B, void* const* C, const int* M,
                           const int* N, const int* K, const int* split_k, void* stream);
/* ABI 17: the same products without atomics: slabs_i holds pcaa_gemm_num_splits(PCAA_F32, K_i, split_k[i]) slabs
 * [M_i, N_i], range s of the contraction overwrites slab s; pcaa_splitk_reduce then sums them in a fixed order (the same
 * result every run). */
int pcaa_gemm_group_rc_f32_slabs(int n, const void* const* A, const void* const* B, void* const* slabs, const int* M,
                                 const int* N, const int* K, const int* split_k, void* stream);
/* Lab switch of the 4-wave LDS-DMA loops (csrc/gemm_v2.h): 1 (default; environment PCAA_GEMM_V2=0 to start with 0) =
 * they take every launch pcaa_gemm_4wave_kernel admits; 0 = they decline every launch -- plain products then take the
 * register-staged 256 x 256 kernel, the fused entry points and the split products report their shapes unsupported.
 * Kept switchable for same-process A/B (tools/gemm_lab.py). */
int pcaa_gemm_v2_enable(int on);
int pcaa_gemm_slabs(int math,
                    const void* A, int a_dtype, int a_layout, long lda,
                    const void* B, int b_dtype, int b_layout, long ldb,
                    float* slabs, long slab_stride, int M, int N, int K, int split_k, void* stream);
/* dgrad of a PointNet layer fused with the BatchNorm+ELU backward of the layer BELOW it
 * (models.py:20-29 backward): da = dy[M,K] . Wt[N,K]^T never reaches memory; the epilogue reads that
 * layer's stored pre-activation y[M,N] and writes  dz = da * ELU'(y*scale+shift)  (bf16, same ld as y)
 * while adding {sum dz, sum dz*(y-mean)*rstd} per column into stats (as pcaa_bn_act_bwd_dz does in a
 * separate pass).  All operands bf16, N a multiple of 256, K of 64 and at least 320 (pcaa_gemm_dgrad_bn_supported);
 * M need not be a multiple of 256 (then ld % 8 == 0 and 16-B aligned y / dz).
 * x, xc, W1: must be NULL / 0 / NULL -- the variant of rounds 1-4 that rebuilt y of the first PointNet layer from the
 * points in the epilogue (never faster than the separate statistics pass) left with the 8-wave kernel in round 5; y is
 * required. */
/* Eval-mode PointNet layer in one launch (models.py:6-34 with BatchNorm2d in eval mode: a per-channel affine map
 * known before the product): out[M,N] bf16 = ELU(scale[n] * (A[M,K] . W[N,K]^T) + shift[n]), A and W bf16,
 * contraction contiguous; same shape rule as pcaa_gemm_dgrad_bn_supported.  pool_rows in {32, 64, 128}: the
 * activation is additionally averaged over groups of pool_rows consecutive rows (AvgPool2d((1,N)) over the
 * points of a frame, models.py:242-243) and out is fp32 [M/pool_rows, N] -- the [M,N] activation never
 * exists.  The inference path (inference_PCAA.py:196-231, BASELINE config[4]) uses both forms. */
int pcaa_gemm_affine_elu(const void* A, long lda, const void* W, long ldw, void* out, long ldo,
                         const float* scale, const float* shift, int M, int N, int K, int pool_rows,
                         void* stream);
/* ABI 29: the same eval-mode layer on the block-scaled fp8 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4, e4m3 x e4m3, every
 * e8m0 block scale 1.0, fp32 accumulate) -- a deployment precision of the scorers, never of training.
 * Contract:
 *   weights   pcaa_quantize_weight_fp8: fp32 W[R,C] (dense) -> W8[R,C] e4m3 and s[R] fp32.  Per row: absmax = f 2^E
 *             with f in [0.5, 1) gives s = 2^(E-8) (E is held at >= -118 so that s stays a normal fp32; a zero or
 *             non-finite absmax gives s = 1), W8 = e4m3fn_rne(W / s), |W / s| < 256.  The caller folds s into the
 *             layer's BatchNorm scale: scale8 = scale * s (exact, a power of two); shift is unchanged.
 *   values    e4m3fn_rne(clamp(v, -448, 448)), NaN stays NaN; the clamp is arithmetic, no mode bit of the convert.
 *   product   A8[M,K] . W8[N,K]^T, both contraction-contiguous e4m3 bytes.
 *   epilogue  ELU(scale8[n] * acc + shift[n]) as pcaa_gemm_affine_elu computes it, stored as
 *               pool_rows == 0: out_dtype PCAA_FP8_E4M3 (the next layer's operand) or PCAA_BF16, [M, ldo];
 *               pool_rows in {32, 64, 128}: out_dtype PCAA_F32, the mean over groups of pool_rows rows, [M / pool_rows, ldo]
 *               (M a multiple of pool_rows).
 * Shapes (pcaa_gemm_fp8_supported): N a multiple of 256, K a multiple of 128 and at least 128 (the four-stage ring is
 * filled stage by stage, so one 128-wide step is enough), M > 0: rows past M of a partial last row tile read as zeros
 * and are not stored.  lda, ldw multiples of 16 that cover K and stay below 2^23; A8, W8, out, scale8, shift 16-B
 * aligned (a pooled fp32 out: 4-B), ldo >= N and, unpooled, ldo * element size a multiple of 16.  Operands of any
 * total size: every tile addresses its own 256 rows. */
int pcaa_quantize_weight_fp8(const float* W, void* W8, float* s, int R, int C, void* stream);
int pcaa_gemm_fp8_supported(int M, int N, int K);
int pcaa_gemm_fp8_affine_elu(const void* A8, long lda, const void* W8, long ldw, void* out, int out_dtype, long ldo,
                             const float* scale8, const float* shift, int M, int N, int K, int pool_rows,
                             void* stream);
int pcaa_gemm_dgrad_bn_supported(int M, int N, int K);
int pcaa_gemm_dgrad_bn(const void* dy, long lddy, const void* Wt, long ldw, const void* y, void* dz, long ld,
                       const float* scale, const float* shift, const float* mean, const float* rstd,
                       double* stats, int nrep, int M, int N, int K,
                       const float* x, int xc, const float* W1, void* stream);
/* dy = coef0*dz + coef1*y + coef2 (fp32 dz, y) written as its [hi | lo] fp16 image [rows, 2 ch]: the second half of the
 * BatchNorm backward behind pcaa_gemm_dgrad_bn_split3 */
int pcaa_bn_bwd_dy_split(const float* dz, const float* y, void* dy_img, const float* coef, long rows, int ch,
                         float img_scale, void* stream);
/* pcaa_gemm_dgrad_bn for the split-fp16 parity mode: dy_img [M, 2K], Wt_img [N, 2K] are [hi | lo] fp16 images, y and dz
 * fp32 [M, ld]; out_scale = 1 / (image scales). */
int pcaa_gemm_dgrad_bn_split3(const void* dy_img, long lddy, const void* Wt_img, long ldw, const float* y, float* dz,
                              long ld, const float* scale, const float* shift, const float* mean, const float* rstd,
                              double* stats, int nrep, int M, int N, int K, float out_scale, void* stream);
/* Kernel-exact timing of one LDS-DMA GEMM launch (bench.py's roofline figure): events made by
 * pcaa_timing_events_create and armed with pcaa_time_next_gemm ride on the NEXT such launch of the
 * calling thread (hipExtLaunchKernelGGL start/stop events: the timestamps of the kernel's own dispatch
 * packet, what rocprofv3 reports).  pcaa_timing_pending: 1 while armed events have not been consumed
 * (the call did not reach that kernel); pcaa_time_next_gemm(NULL, NULL) disarms.  pcaa_timing_elapsed_ms
 * after the stream has been synchronised. */
int pcaa_timing_events_create(void** start, void** stop);
int pcaa_timing_events_destroy(void* start, void* stop);
int pcaa_time_next_gemm(void* start, void* stop);
int pcaa_timing_pending(void);
int pcaa_timing_elapsed_ms(void* start, void* stop, float* ms);
int pcaa_splitk_reduce(const float* slabs, int nsplit, long slab_stride, long n, float* out,
                       int accumulate, void* stream);
/* same, for out[rows, ch], plus the BatchNorm column statistics of out (stats as in pcaa_gemm) */
int pcaa_splitk_reduce_stats(const float* slabs, int nsplit, long slab_stride, float* out,
                             double* stats, int nrep, long rows, int ch, void* stream);

/* First PointNet layer, Conv2d(C -> cout, 1x1) on the raw points x[P,C] (models.py:87-89):
 * y[P,cout] = x . W[cout,C]^T + bias, with the same BatchNorm statistics as pcaa_gemm;
 * and its weight gradient dW[cout,C] += dy[P,cout]^T . x (dW must be pre-initialised).
 * C <= 8; the contraction is too narrow for MFMA, these stream y / dy at HBM rate. */
int pcaa_pointnet_in_fwd(const float* x, int C, const float* W, const float* bias, void* y, int y_dtype,
                         long P, int cout, double* stats, int nrep, void* stream);
int pcaa_pointnet_in_wgrad(const void* dy, int dy_dtype, const float* x, int C, float* dW, long P,
                           int cout, void* stream);
/* Recompute path of the same layer (+ its BatchNorm2d + ELU, models.py:20-29): y costs C FMAs per
 * element, so it is never stored.  Forward: pcaa_pointnet_in_fwd with y == NULL (statistics only),
 * pcaa_bn_finalize, then  a = ELU((x.W^T)*scale + shift).  Backward, two passes over the incoming
 * gradient da only: statistics {sum dz, sum dz*yhat} with dz = da*ELU'(z) (then
 * pcaa_bn_bwd_finalize), and  dW += dy^T.x  with dy = coef0*dz + coef1*y + coef2 formed in registers. */
/* a_dtype: PCAA_F32, PCAA_BF16, PCAA_SPLIT_F16 or (ABI 29) PCAA_FP8_E4M3 -- the same arithmetic, the activation stored
 * as e4m3fn_rne(clamp(a, -448, 448)) bytes [P, cout], the operand of pcaa_gemm_fp8_affine_elu. */
int pcaa_pointnet_in_apply(const float* x, int C, const float* W, const float* scale, const float* shift,
                           void* a, int a_dtype, long P, int cout, void* stream);
int pcaa_pointnet_in_bwd_stats(const void* da, int dtype, const float* x, int C, const float* W,
                               const float* scale, const float* shift, const float* mean, const float* rstd,
                               double* stats, int nrep, long P, int cout, void* stream);
/* One pass instead of the two (round 3): the weight gradient is linear in dy and y = x.W^T, so
 *   dW = c0 (.) (dz^T x) + c1 (.) (W . x^T x) + c2 (x) sum_p x.
 * pcaa_pointnet_in_bwd_onepass reduces the statistics AND G[nrep][cout,C] += dz^T.x (zero-initialised; workgroup b adds
 * into replica b % nrep: one shared image ran at the contended atomic rate) from one read of
 * da; pcaa_points_moments accumulates mom[pcaa_points_moments_size()] (zero-initialised fp64: x^T x at [k*8 + c], the
 * sums at [64 + c]); pcaa_pointnet_in_bwd_combine forms dW (=) from G, the moments and pcaa_bn_bwd_finalize's coef. */
int pcaa_pointnet_in_bwd_onepass(const void* da, int dtype, const float* x, int C, const float* W,
                                 const float* scale, const float* shift, const float* mean, const float* rstd,
                                 double* stats, int nrep, float* G, long P, int cout, const double* pivot_mom,
                                 double pivot_inv_count, void* stream);
/* ABI 17: the same pass without atomics on G: workgroup b STORES its partial to row b of
 * G[pcaa_pointnet_in_bwd_g_rows(P)][cout,C] (no zeroing needed); pass that row count as the combine's nrep, which sums
 * the rows in a fixed order -- dW is then the same every run. */
int pcaa_pointnet_in_bwd_onepass_rows(const void* da, int dtype, const float* x, int C, const float* W,
                                      const float* scale, const float* shift, const float* mean, const float* rstd,
                                      double* stats, int nrep, float* G, long P, int cout, const double* pivot_mom,
                                      double pivot_inv_count, void* stream);
int pcaa_pointnet_in_bwd_g_rows(long P);
int pcaa_points_moments_size(void);
int pcaa_points_moments(const float* x, int C, long P, double* mom, void* stream);
/* Round 4: G is accumulated against the points centred on a pivot, pivot[c] = (float)(pivot_mom[64 + c] *
 * pivot_inv_count) (pivot_mom NULL: no centring) -- normally the points' own moments and 1 / P; under SyncBN the
 * all-reduced moments and 1 / (global count), so that every rank uses the same pivot.  The combine takes the LOCAL
 * moments and point count P plus the same pivot source, and drops pivot (x) sum_p dy (zero per channel). */
int pcaa_pointnet_in_bwd_combine(const float* G, int nrep, const float* W, const double* mom, const float* coef,
                                 float* dW, int cout, int C, long P, const double* pivot_mom, double pivot_inv_count,
                                 void* stream);
/* The same moments give the layer's forward BatchNorm statistics without a pass over the points (sum y = W.sum x,
 * sum y^2 = W^T (x^T x) W per channel): arm the forward finalize on `mom` (pcaa_bn_tail_arm_fwd with stats = mom,
 * count = P, any non-null counter), then this call writes scale / shift / mean / rstd and the running statistics. */
int pcaa_pointnet_in_moment_stats(const double* mom, const float* W, int C, int cout, void* stream);
int pcaa_pointnet_in_bwd_wgrad(const void* da, int dtype, const float* x, int C, const float* W,
                               const float* scale, const float* shift, const float* coef, float* dW,
                               long P, int cout, int dz_is_pre /* da already is dz (pcaa_gemm_dgrad_bn) */,
                               void* stream);

/* bf16 shadow of an fp32 weight matrix src[R,C]: dst[R,C] and/or its transpose dst_t[C,R]
 * (either may be NULL).  Lets the bf16 GEMM stream both operands by LDS-DMA. */
int pcaa_cast_bf16(const float* src, void* dst, void* dst_t, int R, int C, void* stream);

/* ------------------------------------------------------------------ BatchNorm (+ELU) pieces
 * Training-mode BatchNorm2d/1d + ELU of PointNetModule (models.py:28-29) and
 * DilTempConv1d (models.py:71,77-78), split around the grid-wide statistics
 * dependency.  stats = [nrep][2][ch] fp64 (sum, sumsq of the bias-free linear
 * output); count = rows reduced over.
 */
int pcaa_bn_finalize(const double* stats, int nrep, long count, const float* lin_bias,
                     const float* gamma, const float* beta,
                     float* running_mean, float* running_var, long long* num_batches_tracked,
                     float momentum, float eps,
                     float* scale, float* shift, float* mean, float* rstd, int ch, void* stream);
/* eval mode: scale/shift from the running statistics.  NOTE: the pre-BN tensor y of these
 * layers is stored WITHOUT the linear layer's bias (it cancels in train-mode BatchNorm; here
 * it is folded into shift), hence lin_bias in both finalisers. */
int pcaa_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                        const float* running_var, const float* lin_bias, float eps, float* scale,
                        float* shift, int ch, void* stream);
/* a = ELU(y*scale + shift) */
int pcaa_bn_act_fwd(const void* y, void* a, int dtype, const float* scale, const float* shift,
                    long rows, int ch, void* stream);
/* pooled[g][c] = mean_{r in group g} ELU(y[g*group_rows + r][c]*scale[c] + shift[c])
 * (AvgPool2d over the N points, models.py:242-243,282; AvgPool1d over T, :249,284).
 * Training (e1, e2, mean, rstd non-NULL; all NULL in eval): also
 *   e1[g][c] = sum_r ELU'(z),  e2[g][c] = sum_r ELU'(z) * (y - mean[c]) * rstd[c]
 * from which pcaa_bn_pool_bwd_stats forms this layer's BatchNorm-backward statistics
 *   stats += { sum_g dpool*pool_scale*e1, sum_g dpool*pool_scale*e2 }
 * without re-reading y (the incoming gradient is constant over a group). */
int pcaa_bn_act_meanpool_fwd(const void* y, int dtype, const float* scale, const float* shift,
                             const float* mean, const float* rstd, float* pooled, float* e1, float* e2,
                             long groups, int group_rows, int ch, void* stream);
int pcaa_bn_pool_bwd_stats(const float* dpool, const float* e1, const float* e2, float pool_scale,
                           double* stats, int nrep, long groups, int ch, void* stream);
/* backward through ELU (+ the mean-pool broadcast when dpool != NULL):
 *   da = (dpool ? dpool[row / group_rows][c] * pool_scale : da[row][c])
 *   dz = da * ELU'(y*scale + shift);   stats += { sum dz, sum dz * yhat }  (fp64) */
int pcaa_bn_act_bwd_dz(const void* da, const float* dpool, int group_rows, float pool_scale,
                       const void* y, void* dz, int dtype,
                       const float* scale, const float* shift, const float* mean, const float* rstd,
                       double* stats, int nrep, long rows, int ch, void* stream);
/* coef[3][ch] such that dy = coef0*dz + coef1*y + coef2; dgamma, dbeta */
int pcaa_bn_bwd_finalize(const double* stats, int nrep, long count, const float* gamma,
                         const float* mean, const float* rstd,
                         float* coef, float* dgamma, float* dbeta, int ch, void* stream);
int pcaa_bn_bwd_dy(const void* dz, const void* y, void* dy, int dtype, const float* coef,
                   long rows, int ch, void* stream);
/* ABI 28: the streaming route of the element-wise passes (csrc/ew_stream.h: persistent grid, 16 bytes per lane, a ring
 * of row-loads per lane).  Every element it writes is bit-identical to the classic grid-stride kernel's.  A launcher
 * takes it when pcaa_ew_route answers "stream": the pass is one of those ported (PCAA_EW_ACT_FWD: pcaa_bn_act_fwd,
 * for ch >= 1024 only -- narrower rows measured inside the classic route's spread; PCAA_EW_BWD_DY: pcaa_bn_bwd_dy, in
 * place or not), dtype is PCAA_BF16, ch % 8 == 0 with ch / 8 dividing 256, the tensors are 16-byte aligned
 * (aligned != 0), and the switch is on.  Everything else -- fp32, the split images, a ragged ch, the other passes --
 * answers "classic".  A pure host function: no HIP call, works without a GPU.
 * The switch: the environment's PCAA_EW_STREAM=0 (read once, at the first decision) or pcaa_ew_stream_set(0) turn the
 * route off; pcaa_ew_stream_set returns the previous setting. */
#define PCAA_EW_ACT_FWD 0
#define PCAA_EW_BWD_DY 1
#define PCAA_EW_BWD_DY_FUSED 2
#define PCAA_EW_MEANPOOL 3
#define PCAA_EW_IN_BWD 4
#define PCAA_EW_IN_APPLY 5
const char* pcaa_ew_route(int pass, int dtype, long rows, int ch, int aligned);
/* the stream kernel's geometry for a pass (0 for a pass that has none): workgroups per CU of its persistent grid (the
 * grid is that times the CU count, at most one workgroup per trip of 256 / (ch/8) rows) and rows a lane keeps ahead */
int pcaa_ew_wgs_per_cu(int pass);
int pcaa_ew_ring_depth(int pass);
int pcaa_ew_stream_set(int on);
/* ABI 23: backward through EVAL-mode BatchNorm + ELU (BatchNorm is the fixed map z = scale*y + shift, scale = gamma*r,
 * r = 1/sqrt(running_var + eps); y is stored bias-free, so the mean it is centred on is m' = running_mean - bias).
 * pcaa_bn_eval_moments writes (m', r) as fp32 vectors.  pcaa_bn_eval_act_bwd makes ONE pass over y[rows, ch]:
 *   g  = (dpool ? dpool[row / group_rows][c] * pool_scale : da[row][c])
 *   dz = g * ELU'(y*scale + shift);   dy = scale * dz  (y's dtype; dy may alias da);
 *   stats += { sum dz, sum dz * (y - mean)*rstd }  (fp32 inside a workgroup of 128 rows, fp64 across: [nrep][2][ch],
 *   zero-initialised);  ch as for pcaa_bn_act_bwd_dz.
 * pcaa_bn_eval_bwd_finalize: dbeta = sum dz, dgamma = sum dz*xhat, dbias = scale*dbeta -- the bias in front of an
 * eval-mode BatchNorm has a real gradient -- in fp64 with one rounding; each destination may be NULL. */
int pcaa_bn_eval_moments(const float* running_mean, const float* running_var, const float* lin_bias,
                         float eps, float* mean, float* rstd, int ch, void* stream);
int pcaa_bn_eval_act_bwd(const void* da, const float* dpool, int group_rows, float pool_scale,
                         const void* y, void* dy, int dtype,
                         const float* scale, const float* shift, const float* mean, const float* rstd,
                         double* stats, int nrep, long rows, int ch, void* stream);
int pcaa_bn_eval_bwd_finalize(const double* stats, int nrep, const float* scale,
                              float* dgamma, float* dbeta, float* dbias, int ch, void* stream);
/* The finalize CARRIED BY THE PRODUCER of the statistics (round 3; csrc/bn_tail.h).  pcaa_bn_tail_arm_fwd / _bwd
 * note the arguments of pcaa_bn_finalize / pcaa_bn_bwd_finalize on the calling thread; the NEXT launch on that thread
 * that accumulates into exactly this `stats` buffer and can carry a tail (pcaa_gemm on the LDS-DMA path with colstats,
 * pcaa_gemm_dgrad_bn, pcaa_pointnet_in_fwd (statistics only), pcaa_pointnet_in_bwd_stats / _onepass, pcaa_bn_pool_bwd_stats,
 * pcaa_dtc_conv_fwd / _dgrad without K split) takes it: its last workgroup to finish (agent-scope arrival counter,
 * `counter`: one zero-initialised word, left at zero) writes the coefficients, and the separate finalize launch
 * -- 5-8 us on the critical path, 20 per train step -- is gone.  pcaa_bn_tail_pending() == 1 after the producer's
 * call means it did not take the tail: call pcaa_bn_tail_disarm() and the stand-alone finalize. */
int pcaa_bn_tail_arm_fwd(const double* stats, int nrep, long count, const float* lin_bias,
                         const float* gamma, const float* beta,
                         float* running_mean, float* running_var, long long* num_batches_tracked,
                         float momentum, float eps,
                         float* scale, float* shift, float* mean, float* rstd, int ch, unsigned* counter);
int pcaa_bn_tail_arm_bwd(const double* stats, int nrep, long count, const float* gamma,
                         const float* mean, const float* rstd,
                         float* coef, float* dgamma, float* dbeta, int ch, unsigned* counter);
int pcaa_bn_tail_pending(void);
int pcaa_bn_tail_disarm(void);
/* Two-pass form that never materialises dz: first pcaa_bn_act_bwd_dz with dz == NULL
 * (statistics only), then dy = coef0 * (da * ELU'(y*scale+shift)) + coef1 * y + coef2 here
 * (da / dpool as in pcaa_bn_act_bwd_dz; dy may alias da). */
int pcaa_bn_bwd_dy_fused(const void* da, const float* dpool, int group_rows, float pool_scale,
                         const void* y, void* dy, int dtype, const float* scale, const float* shift,
                         const float* coef, long rows, int ch, void* stream);

/* ------------------------------------------------------------------ small fp32 helpers */
/* y = act(y + bias[col])  (Linear bias + ELU of the decoder / MLP heads, models.py:373-382) */
int pcaa_bias_act(float* y, const float* bias, int act, long rows, int cols, void* stream);
/* dz = da * ELU'(z) computed from the saved output a = ELU(z) */
int pcaa_elu_bwd_from_out(const float* da, const float* a, float* dz, long n, void* stream);
/* out[c] = sum_r x[r][c]   (bias gradients) */
int pcaa_colsum(const float* x, float* out, long rows, int cols, void* stream);
/* out[0] = scale * sum(x[0..n)) -- deterministic single-block reduction */
int pcaa_sum(const float* x, long n, float scale, float* out, void* stream);
/* out[r] = scale * sum_c x[r][c] */
int pcaa_rowsum(const float* x, float* out, long rows, int cols, float scale, void* stream);
/* out[i] = x[i] * s[0]   (s is a DEVICE scalar: chain-rule scaling without a host sync) */
int pcaa_scale_by_device_scalar(const float* x, const float* s, float* out, long n, void* stream);
/* out[r][c] = x[r][c] * s[r] */
int pcaa_scale_rows(const float* x, const float* s, float* out, long rows, int cols, void* stream);
/* Prior sampling of the D-step (PCAA_ablation.py:904-931): onehot[b][k] = (k == gt[b]),
 * z[b] = z0[b] + means[gt[b]] */
int pcaa_prior_sample(const float* z0, const float* means, const long long* gt, int B, int K, int D,
                      float* z, float* onehot, void* stream);
/* dst[b,t,n,c] (contiguous) = src[b,c,t,n] (given element strides) */
int pcaa_pack_points(const float* src, long sb, long sc, long st, long sn,
                     float* dst, int B, int C, int T, int N, void* stream);

/* Batch assembly from a packed crop store resident in HBM (replaces the per-sample np.load + default collate
 * of MSRadarDataset.__getitem__ / DataLoader, datasets.py:466-479, PCAA_ablation.py:794-800):
 * dst[r] = src[idx[r]], rows of row_bytes bytes (multiple of 16).  An index outside [0, n_src_rows)
 * zero-fills its row and sets *err_flag (device int, may be NULL) to 1. */
int pcaa_gather_rows(const void* src, long n_src_rows, long row_bytes, const long long* idx, void* dst,
                     long n_rows, int* err_flag, void* stream);

/* causal dilated Conv1d (k=3) as a GEMM: col[(b,t)][ci*3+tap] = a[b][t-(2-tap)*d][ci] or 0
 * (models.py:59-68,75-76) and its adjoint */
int pcaa_dtc_im2col(const float* a, float* col, int B, int T, int Cin, int dilation, void* stream);
int pcaa_dtc_col2im(const float* dcol, float* da, int B, int T, int Cin, int dilation, void* stream);

/* ------------------------------------------------------------------ losses
 * SeqChamferLoss (utils.py:88-132) forward + analytic backward w.r.t. preds.
 * preds/gts/dpreds are logical [B,C,T,N] tensors with element strides.
 * frame_loss[b*T+t] = sum_j min_i P + sum_i min_j P;
 * dpreds (nullable) = d/dpreds of sum_{b,t} w_b * frame_loss, w_b = grad_scale
 *   * (grad_per_b ? grad_per_b[b] : 1). */
int pcaa_chamfer_fwd_bwd(const float* preds, long p_sb, long p_sc, long p_st, long p_sn,
                         const float* gts, long g_sb, long g_sc, long g_st, long g_sn,
                         int B, int T, int N, int C, float* frame_loss,
                         float* dpreds, long d_sb, long d_sc, long d_st, long d_sn,
                         float grad_scale, const float* grad_per_b, void* stream);
/* CrossEntropyLoss(mean) (PCAA_ablation.py:1008) + argmax(softmax) (:891-893).
 * loss, dlogits, preds are each nullable. dlogits = grad_scale*(softmax - onehot)/B.
 * err_flag (nullable, device int32[1]): set to 1 if a target is outside [0,K) -- torch raises there; the
 * row is then scored against class 0 so that nothing is read out of bounds. */
int pcaa_cross_entropy(const float* logits, const long long* target, int B, int K,
                       float* loss, float* dlogits, float grad_scale, long long* preds,
                       int* err_flag, void* stream);

/* ------------------------------------------------------------------ CGDiscriminator (models.py:405-421)
 * u = [x(32) ; label(K)] -> 64 ELU -> 32 ELU -> 1.  Parameters in PyTorch layout. */
int pcaa_disc_forward(const float* x, const float* label, int B, int K,
                      const float* W1, const float* b1, const float* W2, const float* b2,
                      const float* W3, const float* b3, float* out, void* stream);
/* first-order backward: gout[B] -> dx[B,32], dlabel[B,K], parameter grads (each nullable;
 * parameter grads are OVERWRITTEN) */
int pcaa_disc_backward(const float* x, const float* label, int B, int K,
                       const float* W1, const float* b1, const float* W2, const float* b2,
                       const float* W3, const float* b3, const float* gout,
                       float* dx, float* dlabel,
                       float* dW1, float* db1, float* dW2, float* db2, float* dW3, float* db3,
                       float* workspace, size_t workspace_bytes, void* stream);
/* backward OF that input gradient (what torch.autograd.grad(D(interp), interp, create_graph=True) followed by
 * .backward() needs, PCAA_ablation.py:955-976): with g[B,32] = the dx of pcaa_disc_backward for the same
 * (x, label, gout) and gbar[B,32] the incoming gradient w.r.t. g, the gradients of sum_b <gbar_b, g_b> w.r.t.
 * x (dx2), label (dlabel2), gout (dgout [B]) and the parameters (db3 = 0).  Outputs nullable, OVERWRITTEN;
 * workspace as pcaa_disc_workspace_bytes. */
int pcaa_disc_backward_backward(const float* x, const float* label, int B, int K,
                                const float* W1, const float* b1, const float* W2, const float* b2,
                                const float* W3, const float* b3, const float* gout, const float* gbar,
                                float* dx2, float* dlabel2, float* dgout,
                                float* dW1, float* db1, float* dW2, float* db2, float* dW3, float* db3,
                                float* workspace, size_t workspace_bytes, void* stream);
/* WGAN-GP critic step (PCAA_ablation.py:939-976): d_loss = mean D(fv) - mean D(z)
 * + gp_weight * mean (|dD/dx(z + alpha (fv - z))| - 1)^2 with the closed-form
 * second-order gradient.  losses[0]=d_loss, losses[1]=gp.
 * Parameter grads are OVERWRITTEN.  dz (or NULL): d(d_loss)/dz [B,32] -- ablation variant 1
 * (PCAA_ablation.py:28-378) learns the prior centroids, z = z0 + GaussianMeanLearner(onehot) (:170-186),
 * so the critic loss is differentiated w.r.t. z too (real pass + the penalty through the interpolates). */
size_t pcaa_disc_workspace_bytes(int B, int K);
int pcaa_disc_wgan_gp(const float* z, const float* fv, const float* label, const float* alphas,
                      int B, int K,
                      const float* W1, const float* b1, const float* W2, const float* b2,
                      const float* W3, const float* b3, float gp_weight, float* losses,
                      float* dW1, float* db1, float* dW2, float* db2, float* dW3, float* db3,
                      float* dz, float* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ open-set scoring
 * joint_likelihood (inference_PCAA.py:129-136): lik[b] = (1/K) sum_k N(x_b; mu_k, I_D), float64,
 * evaluated as exp(log-pdf) like scipy.stats.multivariate_normal.pdf.
 * k-window vote (inference_PCAA.py:263-271): window w covers crops [w*k,(w+1)*k); known iff
 * #(lik > threshold) > k/2 -> most frequent predicted label over the encoder's n_classes outputs
 * (np.argmax(np.bincount(preds)): lowest label on ties), else n_labels (the "unknown" id = number of
 * distinct labels of the known test split, which may be smaller than n_classes). */
int pcaa_joint_likelihood(const float* x, const float* means, int B, int K, int D, double* lik,
                          void* stream);
int pcaa_kvote(const double* lik, const long long* preds, double threshold, int k, int n_labels,
               int n_classes, int n_windows, long long* out, void* stream);

/* ------------------------------------------------------------------ batch-skinny Linear layers
 * The CGDecoder's Linear stack (models.py CGDecoder: nn.Linear(32+K, S/16) ... nn.Linear(S/2, S),
 * called from PCAA_ablation.py train_variant4) with M = batch <= 64 rows: each product is one
 * pass over the fp32 weight matrix W[N][K] (N = out_features, K = in_features, ldw elements
 * between rows), streamed from HBM straight into bf16 MFMA fragments (fp32 accumulate).
 *   fwd  : y[M][N]  = act(x[M][K] . W^T + bias)
 *   dgrad: dx[M][K] (=|+=) (dz[M][N] . W) * ELU'(a_prev)   (a_prev = ELU output of the layer
 *          below, NULL: no factor) -- i.e. the gradient w.r.t. that layer's pre-activation
 *   wgrad: dW[N][K] = dz^T . x
 * fwd/dgrad split the contraction into `nsplit` slabs in `ws` (>= nsplit*M*N resp. nsplit*M*K
 * floats) and reduce them deterministically; nsplit must come from pcaa_skinny_splits (kind 0
 * fwd, 1 dgrad; 2 / 3: the _exact forms) -- the deepest split whose grid still fits the chip's resident workgroups of
 * that kernel in ONE round.  pcaa_skinny_supported: 1 <= M <= 64, N and K multiples of 64, N >= 128, K >= 64, N K < 2^31 - 2^20. */
int pcaa_skinny_supported(int M, int N, int K);
int pcaa_skinny_splits(int kind, int M, int N, int K);
int pcaa_skinny_linear_fwd(const float* x, long ldx, const float* W, long ldw, const float* bias, int act,
                           float* y, float* ws, long ws_floats, int M, int N, int K, int nsplit,
                           void* stream);
int pcaa_skinny_linear_dgrad(const float* dz, long lddz, const float* W, long ldw, float* dx,
                             const float* a_prev, int accumulate, float* ws, long ws_floats, int M, int N,
                             int K, int nsplit, void* stream);
int pcaa_skinny_linear_wgrad(const float* dz, long lddz, const float* x, long ldx, float* dW, long lddw,
                             int M, int N, int K, void* stream);
/* The same three passes with fp32 products (v_mfma_f32_32x32x2_f32 on the unrounded operands): the decoder of the parity
 * modes ("fp32", "fp16x3"), which rounds 1-2 ran on the 128x128-tile fp32 GEMM.  Same arguments; the dgrad needs W 8-B
 * aligned with an even leading dimension. */
int pcaa_skinny_linear_fwd_exact(const float* x, long ldx, const float* W, long ldw, const float* bias, int act,
                                 float* y, float* ws, long ws_floats, int M, int N, int K, int nsplit, void* stream);
int pcaa_skinny_linear_dgrad_exact(const float* dz, long lddz, const float* W, long ldw, float* dx,
                                   const float* a_prev, int accumulate, float* ws, long ws_floats, int M, int N,
                                   int K, int nsplit, void* stream);
int pcaa_skinny_linear_wgrad_exact(const float* dz, long lddz, const float* x, long ldx, float* dW, long lddw,
                                   int M, int N, int K, void* stream);
int pcaa_skinny_linear_wgrad_adam_exact(const float* dz, long lddz, const float* x, long ldx, float* W,
                                        float* exp_avg, float* exp_avg_sq, long ldw, int M, int N, int K,
                                        float beta1, float beta2, float eps, float grad_scale,
                                        const float* coef_dev, void* stream);   /* = pcaa_skinny_linear_wgrad_adam, fp32 products */
/* The same product written as bf16 (dW_bf16 [N, lddw] bf16, lddw even): the data-parallel step with bf16 gradient
 * buckets produces the gradient in the form it crosses the wire in (no fp32 copy, no cast pass). */
int pcaa_skinny_linear_wgrad_bf16(const float* dz, long lddz, const float* x, long ldx, void* dW_bf16, long lddw,
                                  int M, int N, int K, void* stream);
/* The same product fused with optimizer_G's Adam update of that weight (PCAA_ablation.py:1018-1021: backward,
 * then optimizer_G.step()): dW[N,K] = dz^T x stays in registers, W / exp_avg / exp_avg_sq [N,ldw] are read and
 * written in place -- torch.optim.Adam's update with the step-dependent scalars from coef_dev (pcaa_adam_advance),
 * bit-identical to pcaa_skinny_linear_wgrad followed by pcaa_adam_step_dev on the same buffers.  W must not be
 * read by anything still in flight (the layer's dgrad).  Single-process training only. */
int pcaa_skinny_linear_wgrad_adam(const float* dz, long lddz, const float* x, long ldx, float* W,
                                  float* exp_avg, float* exp_avg_sq, long ldw, int M, int N, int K,
                                  float beta1, float beta2, float eps, float grad_scale,
                                  const float* coef_dev, void* stream);
/* ABI 15 (round 5): the same fused update from GATHERED rows -- the data-parallel step's exchange for the batch-skinny
 * decoder layers.  dz [M, lddz], x [M, ldx] hold the rows of ALL ranks stacked (M = world * B <= 512, all-gathered: 4 M
 * (N + K) bytes instead of the gradient's 4 N K); every rank forms the global gradient dz^T x in registers and applies
 * the identical Adam update (grad_scale = 1 / world: the reference's mean over the global batch, PCAA_ablation.py:1008-
 * 1021 at BATCH_SIZE = world * B).  bf16 products, fp32 accumulation over the rows in ascending order; M <= 64 gives the
 * bits of pcaa_skinny_linear_wgrad_adam. */
int pcaa_skinny_linear_wgrad_adam_rows(const float* dz, long lddz, const float* x, long ldx, float* W,
                                       float* exp_avg, float* exp_avg_sq, long ldw, int M, int N, int K,
                                       float beta1, float beta2, float eps, float grad_scale,
                                       const float* coef_dev, int rows_alloc, void* stream);
/* (x is read in whole 64-row chunks: rows_alloc = the rows x is allocated for, >= the next of 64 / 128 / 256 / 512 above
 * M; the rows past M must hold finite values -- they meet zeros) */
/* ABI 16 (round 6): the gathered update from PACKED operands -- what the data-parallel step exchanges since round 6.
 * The reference has no multi-GPU path; this stands where a torch DDP port of PCAA_ablation.py:1018-1021 would all-reduce
 * the decoder's gradient.  Every rank packs the two weight-gradient operands of a batch-skinny layer -- dz [rows, N] and
 * x [rows, K], rows <= 64 -- into ONE chunk P[(N + K)][64] bf16: transposed (one 128-B row per column of dz, then per
 * column of x), rounded to nearest even (the rounding the weight-gradient kernels apply in registers), zero behind `rows`.
 * The ranks' chunks concatenate (one all-gather per layer, 2 (N + K) 64 bytes per rank); pcaa_skinny_linear_wgrad_adam_t16
 * contracts over `chunks` <= 8 of them (chunk c at packed + c * chunk_stride elements, chunk_stride >=
 * pcaa_packed_chunk_elems(N, K)) and applies Adam in place: W <- Adam(W, grad_scale * sum_c dz_c^T x_c), 24 B per
 * parameter, bf16 products, fp32 accumulation.  Supersedes pcaa_skinny_linear_wgrad_adam_rows in the trainer (that entry
 * takes fp32 row-major operands and needs no pack; it stays for callers that hold such operands). */
long pcaa_packed_chunk_elems(int N, int K);
int pcaa_pack_rows_t16(const float* dz, long lddz, int N, const float* x, long ldx, int K, int rows, void* chunk_bf16,
                       void* stream);
int pcaa_skinny_linear_wgrad_adam_t16(const void* packed_bf16, long chunk_stride, int chunks, float* W, float* exp_avg,
                                      float* exp_avg_sq, long ldw, int N, int K, float beta1, float beta2, float eps,
                                      float grad_scale, const float* coef_dev, void* stream);
/* ABI 14: the bf16 IMAGE of a decoder weight (W16 [N, ldw] bf16: every element = the weight rounded to nearest even, the
 * conversion pcaa_skinny_linear_fwd / _dgrad apply in registers -- results are bit-identical).  _fwd_w16 / _dgrad_w16
 * stream the image instead of the fp32 matrix: half the bytes of the two passes that sit on the step's critical path.
 * The caller owns the image: train.PCAATrainer rebuilds it with pcaa_cast_bf16 behind each fused update (side stream) and
 * whenever the weight's version counter moved.  (Writing the image from inside pcaa_skinny_linear_wgrad_adam was
 * measured and dropped: 64-B partial lines from different CUs doubled that kernel's time.) */
int pcaa_skinny_linear_fwd_w16(const float* x, long ldx, const void* W16, long ldw, const float* bias, int act,
                               float* y, float* ws, long ws_floats, int M, int N, int K, int nsplit, void* stream);
int pcaa_skinny_linear_dgrad_w16(const float* dz, long lddz, const void* W16, long ldw, float* dx,
                                 const float* a_prev, int accumulate, float* ws, long ws_floats, int M, int N,
                                 int K, int nsplit, void* stream);

/* ------------------------------------------------------------------ temporal block, fused forward
 * One DilTempConv1d layer (models.py:37-79) in one launch: implicit im2col of the causal dilated
 * convolution, the previous layer's BatchNorm+ELU applied while its bias-free output `src` is staged
 * (scale/shift null: src is the block input, used as is), y[B*T,cout] = bias-free pre-BN output,
 * BatchNorm statistics of y (fp64 sums into stats[nrep][2][cout], as pcaa_gemm's colstats) and,
 * if col != null, the im2col matrix col[B*T, cin*3] (layout of pcaa_dtc_im2col) that the weight
 * gradient contracts with.  W = conv1d.weight viewed [cout, cin*3].  Exact-fp32 MFMA.
 * ksplit > 1 cuts the input channels over workgroups: split z writes its partial product to
 * y + z*slab_stride (y then holds ksplit slabs, stats must be null) and pcaa_splitk_reduce_stats
 * finishes the sum and the statistics.
 * pcaa_dtc_conv_supported: T <= 32, cin % 4 == 0, cout % 16 == 0. */
int pcaa_dtc_conv_supported(int T, int cin, int cout);
int pcaa_dtc_conv_ksplit(int B, int cin, int cout);   /* the ksplit to pass: >= cin/256, 8 for few long tiles */
/* ABI 24: the kernel a temporal-conv call takes, from its shape alone (a host function: no HIP call, works without a GPU).
 * adjoint: 0 = pcaa_dtc_conv_fwd*, 1 = pcaa_dtc_conv_dgrad*; bf16: the _bf16 entry point; windowed: the _win / _seg forms.
 * The entry points dispatch on this value.  One workgroup = one sequence (32 output columns fp32, 128 bf16), or two
 * sequences x 32 or 64 columns (contraction >= 128 channels in whole 32-chunks, >= 64 output channels, ksplit == 1, not
 * windowed; 64 columns when (B + 1) / 2 * (columns / 64) >= 192 workgroups remain).  PCAA_DTC_PAIR (0, fwd, adj) switches
 * the two-sequence kernels off per direction.  The limit of 256 (forward) / 512 (adjoint) contraction channels per
 * workgroup is the one-sequence kernels': a call this function sends to a two-sequence kernel stages its channels in
 * passes of 256 and is accepted with ksplit == 1 at any width (through ABI 23 the entry points refused those calls before
 * they looked at the route, so the forward's further passes could not be reached). */
#define PCAA_DTC_ROUTE_ONE_F32 0
#define PCAA_DTC_ROUTE_ONE_BF16 1
#define PCAA_DTC_ROUTE_PAIR32_F32 2
#define PCAA_DTC_ROUTE_PAIR32_BF16 3
#define PCAA_DTC_ROUTE_PAIR64_F32 4
#define PCAA_DTC_ROUTE_PAIR64_BF16 5
int pcaa_dtc_conv_route(int adjoint, int bf16, int B, int cin, int cout, int ksplit, int windowed);
int pcaa_dtc_conv_fwd(const float* src, const float* scale, const float* shift, const float* W, float* y,
                      float* col, double* stats, int nrep, int B, int T, int cin, int cout, int dilation,
                      int ksplit, long slab_stride, void* stream);
/* the bf16 throughput mode's variant (round 4): same arguments, same results up to bf16 rounding of the operands -- the
 * contraction on v_mfma_f32_32x32x16_bf16 (fp32 accumulate), 128 output channels per workgroup; y, col, statistics fp32 */
int pcaa_dtc_conv_fwd_bf16(const float* src, const float* scale, const float* shift, const float* W, float* y,
                      float* col, double* stats, int nrep, int B, int T, int cin, int cout, int dilation,
                      int ksplit, long slab_stride, void* stream);

/* ABI 18: the same layer in eval form (col and stats must be NULL) on a WINDOWED source.  `table` is a frame-feature table
 * [table_rows, cin]: the eval-mode PointNet block plus the mean over a frame's points is a function of one frame
 * (models.py:6-34, 82-105, 242-243, 279-282), and consecutive crops of a track share T - hop of their T frames
 * (datasets.py:16-25, 297-302), so each frame is encoded once and a crop is a window of T rows of the table.  Sequence b,
 * step t reads table row win_row[b] + t (win_row: [B] device ints), or row (win_row[b] + t) % ring_rows with ring_rows > 0
 * (a ring of the last ring_rows frames of a live stream; T <= ring_rows <= table_rows) -- only the staging address of
 * pcaa_dtc_conv_fwd changes (one kernel body serves both), so the [B*T, cin] input of overlapping windows is never
 * written out.  ksplit / slab_stride as above.  The caller checks the range of win_row (0 <= win_row[b],
 * win_row[b] + T <= table_rows, or win_row[b] < ring_rows) on the host copy of the plan that produced it: the kernel
 * does not.  Same values staged, same instruction sequence: y equals what pcaa_dtc_conv_fwd gives on the materialised
 * windows bit for bit where that call takes the one-sequence kernel (always for cout < 64 or cin < 128; a windowed source
 * never takes the two-sequence kernels). */
int pcaa_dtc_conv_fwd_win(const float* table, const float* scale, const float* shift, const float* W, float* y,
                          float* col, double* stats, int nrep, int B, int T, int cin, int cout, int dilation,
                          int ksplit, long slab_stride, const int* win_row, long table_rows, long ring_rows,
                          void* stream);
int pcaa_dtc_conv_fwd_win_bf16(const float* table, const float* scale, const float* shift, const float* W, float* y,
                          float* col, double* stats, int nrep, int B, int T, int cin, int cout, int dilation,
                          int ksplit, long slab_stride, const int* win_row, long table_rows, long ring_rows,
                          void* stream);

/* ABI 19: the windowed eval form on SEGMENTED rings (the rings of many live streams in one table).  `table` is n_seg
 * rings of ring_rows rows back to back ([n_seg * ring_rows, cin]); win_row[b] is an ABSOLUTE table row and the window wraps
 * inside the ring it starts in: with base = (win_row[b] / ring_rows) * ring_rows, step t reads row
 * base + (win_row[b] - base + t) % ring_rows.  Needs ring_rows >= T, n_seg >= 1; the range of win_row (0 <= win_row[b] <
 * n_seg * ring_rows) is the caller's to check on the host plan, as for pcaa_dtc_conv_fwd_win.  Eval only (no col, no
 * statistics); only the staging address differs from pcaa_dtc_conv_fwd_win, whose result it equals bit for bit when
 * n_seg == 1. */
int pcaa_dtc_conv_fwd_seg(const float* table, const float* scale, const float* shift, const float* W, float* y,
                          int B, int T, int cin, int cout, int dilation, int ksplit, long slab_stride,
                          const int* win_row, long n_seg, long ring_rows, void* stream);
int pcaa_dtc_conv_fwd_seg_bf16(const float* table, const float* scale, const float* shift, const float* W, float* y,
                          int B, int T, int cin, int cout, int dilation, int ksplit, long slab_stride,
                          const int* win_row, long n_seg, long ring_rows, void* stream);

/* ------------------------------------------------------------------ frame-deduplicated inference (track_infer.hip)
 * Which consecutive crops of a sequentially ordered split share frames.  Crops are cut with a hop of CROP_STEP out of
 * tracks whose frames were standardised one by one before the cut (datasets.py:16-25, 143-146, 297-302), so a shared
 * frame has the same bits in every crop that holds it.  crops: M crops of crop_elems floats, each T frames of
 * frame_elems floats (point-major [M, T, N, C]: frame_elems = N * C).  same[i] = 1 iff the first T - hop frames of crop
 * i + 1 equal the last T - hop frames of crop i compared as 32-bit WORDS (-0.0 != +0.0, equal NaN payloads are equal),
 * else 0; every same[i] is written (no pre-set needed).  One workgroup per pair; 16-byte loads when frame_elems % 4 == 0
 * and crops is 16-B aligned, 4-byte loads otherwise (pcaa_crop_overlap_vec_bytes tells which: 16 or 4).  M == 1: no
 * launch.  Frames merged on this mask have equal bits, hence equal features, whatever the reason for the equality. */
int pcaa_crop_overlap_vec_bytes(const float* crops, long crop_elems, long frame_elems);
int pcaa_crop_overlap(const float* crops, long crop_elems, long frame_elems, int M, int T, int hop, int* same,
                      void* stream);
/* pcaa_gather_rows for rows that are a multiple of 4 but not of 16 bytes (a frame of N = 150 points x C = 5 features is
 * 3 000 bytes): dst[r] = src[idx[r]], rows of row_words 32-bit words; an index outside [0, n_src_rows) zero-fills its
 * row and sets *err_flag (may be NULL). */
int pcaa_gather_rows_w4(const void* src, long n_src_rows, long row_words, const long long* idx, void* dst,
                        long n_rows, int* err_flag, void* stream);

/* ABI 19: the inverse of the row gather: dst[dst_row[r]] = src[r] for n_rows rows of row_words 32-bit words (dst_row:
 * [n_rows] device ints).  dst_row[r] < 0 skips the row (padding); dst_row[r] >= n_dst_rows skips it and sets *err_flag
 * (may be NULL).  Duplicate destinations are the caller's error.  16-byte copies when row_words % 4 == 0 and src and dst
 * are 16-B aligned, 4-byte copies otherwise. */
int pcaa_scatter_rows(const void* src, const int* dst_row, long n_rows, long row_words, void* dst, long n_dst_rows,
                      int* err_flag, void* stream);
/* ABI 27: the adjoint of the row gather (dst[r] = src[idx[r]]), the overlap-add of window gradients into a frame-feature
 * table: dst[u] = sum_{k = csr_off[u]}^{csr_off[u + 1] - 1} src[csr_idx[k]] for n_dst_rows rows of row_words fp32 words
 * (csr_off [n_dst_rows + 1], csr_idx [nnz]: device ints; the CSR of idx by destination row).  The sum starts from +0 and
 * adds the contributors in ascending k in fp32 with plain adds (no contraction, no atomics): the result is a function of
 * the CSR alone and is reproduced bit for bit by the same loop on the host.  A row without contributors is zero.  An
 * index outside [0, n_src_rows) is skipped and sets *err_flag (may be NULL); a row whose offsets leave [0, nnz] is
 * written as zeros and sets it too.  16-byte accesses when row_words % 4 == 0 and src and dst are 16-B aligned, 4-byte
 * accesses otherwise.  dst may not alias src. */
int pcaa_gather_sum_rows(const float* src, long n_src_rows, long row_words, const int* csr_off, const int* csr_idx,
                         long nnz, float* dst, long n_dst_rows, int* err_flag, void* stream);
/* ABI 19: one tick of a multi-stream scorer in one launch: for the tick's nw windows preds[i] (first maximal softmax
 * probability: the want_preds rule of pcaa_cross_entropy) and lik[i] (the expression of pcaa_joint_likelihood, same bits),
 * and for every window with win_j[i] % k == k - 1 the vote of group win_j[i] / k by the rule of pcaa_kvote, written to
 * votes[vote_pos[i]] (vote_pos[i] < 0: none).  The windows of one stream are a contiguous run of the arrays with ascending
 * win_j: run r is [run_start[r], run_start[r + 1]) (run_start: [n_runs + 1], run_start[0] = 0, run_start[n_runs] = nw),
 * win_stream[i] in [0, max_streams) its stream, a stream has at most one run per call.  hist_lik / hist_pred
 * [max_streams, k] keep a stream's current, incomplete vote group between calls (slot j % k = window j): a vote reads
 * the predecessors that are not in this call from them, and the last k windows of a run are written back.  One
 * workgroup per run, so the number of launches does not depend on the number of streams. */
int pcaa_stream_score(const float* logits, const float* sup_fv, const float* means, const int* run_start, int n_runs,
                      const int* win_stream, const int* win_j, const int* vote_pos, int nw, int K, int D, int Kc,
                      double threshold, int k, int n_labels, int n_classes, double* hist_lik, long long* hist_pred,
                      int max_streams, long long* preds, double* lik, long long* votes, int n_votes, void* stream);

/* ------------------------------------------------------------------ run-time enrolment (gallery.hip)
 * Added after ABI 29 like pcaa_crops_from_raw (the version is unchanged: a library without these entry points fails to
 * load by name).  A gallery holds modes that did not come from training, beside the K prior means, in three device
 * buffers: sums fp64 [E_max, D], counts int32 [E_max], centroids fp32 [E_max, D].  Slot e with counts[e] > 0 is a live
 * mode N(centroids[e], I) and is identity e; a slot with count 0 contributes nothing anywhere.  E is the host's
 * high-water mark of slots ever used: the kernels scan slots 0 .. E - 1.
 *
 * pcaa_gallery_accumulate: sums[slot] += (double)fv[rows[i]] for i = 0 .. m - 1 in that order, plain fp64 adds (rows:
 * int32 [m] on the device, or NULL for rows 0 .. m - 1 of fv [n_rows, D]); then counts[slot] += the number added and
 * centroids[slot] = (float)(sums[slot] / counts[slot]).  A row index outside [0, n_rows) is skipped and sets *err_flag
 * (may be NULL).  Repeated calls continue the running sum.  One launch; on the host the centroid is
 * np.float32(cumsum_in_float64[-1] / count), bit for bit. */
int pcaa_gallery_accumulate(const float* fv, int n_rows, int D, const int* rows, int m, int slot, int E_max,
                            double* sums, int* counts, float* centroids, int* err_flag, void* stream);
/* B windows sup_fv [B, D] with the classifier's preds [B] against means [Kc, D] and the gallery:
 *   lik[b]    = (acc_prior + acc_gallery) / Kc: acc_prior the sum pcaa_joint_likelihood forms (same operations, same
 *               order, before its division), acc_gallery the sum of exp(-0.5 (D log 2pi + |x - c_e|^2)) over the live
 *               slots in fp64 (every lane of a wavefront adds its slots e = lane, lane + 64, ... in ascending order, the
 *               64 partials meet in a fixed butterfly).  The divisor stays Kc: with an empty gallery (acc_gallery = +0.0)
 *               lik is bit-equal to pcaa_joint_likelihood's.
 *   near[b]   = the index in 0 .. Kc + E - 1 (prior modes first) of the mode with the smallest fp64 squared distance,
 *               the lowest index on exact ties;
 *   labels[b] = preds[b] when near < Kc, else n_labels + 1 + (near - Kc); n_labels stays "unknown".
 * One wavefront per window: a window's outputs do not depend on B, its position or the grid.  E = 0: centroids and
 * counts may be NULL. */
int pcaa_gallery_score(const float* sup_fv, const long long* preds, const float* means, int B, int Kc, int D,
                       const float* centroids, const int* counts, int E, int n_labels, double* lik, long long* labels,
                       int* near, void* stream);
/* The rule of pcaa_kvote over arbitrary non-negative labels: a group is known iff #(lik > threshold) > k/2 and then
 * takes the most frequent label of its k windows (the lowest on ties: argmax(bincount)), else n_labels.  On labels
 * below n_classes it equals pcaa_kvote. */
int pcaa_gallery_kvote(const double* lik, const long long* labels, double threshold, int k, int n_labels, int n_windows,
                       long long* out, void* stream);
/* pcaa_stream_score with the score of pcaa_gallery_score (same bits) and the vote of pcaa_gallery_kvote: same runs,
 * history and barriers, one launch whatever the number of streams and slots.  hist_label [max_streams, k] holds the
 * extended labels as they were stored: a label is never recomputed when the gallery changes between ticks.  H > 0:
 * window j's sup_fv is also written to fv_hist[stream * H + j % H] (fv_hist fp32 [max_streams * H, D]); H = 0: fv_hist
 * may be NULL. */
int pcaa_stream_score_gallery(const float* logits, const float* sup_fv, const float* means, const int* run_start,
                              int n_runs, const int* win_stream, const int* win_j, const int* vote_pos, int nw, int K,
                              int D, int Kc, double threshold, int k, int n_labels, const float* centroids,
                              const int* counts, int E, double* hist_lik, long long* hist_label, int max_streams,
                              float* fv_hist, int H, long long* labels, double* lik, int* near, long long* votes,
                              int n_votes, void* stream);

/* ------------------------------------------------------------------ raw radar detections -> frames (raw_frames.hip)
 * ABI 20: what datasets.process_track does per frame on the host (reference datasets.py:79-161), for the n frames of a
 * tick in one launch.  points [P, 5] (x, y, z, doppler, linear power; fp32, or fp64 when points_f64: the reference's
 * on-disk type), offsets [n + 1]: frame f owns rows offsets[f] .. offsets[f + 1] - 1 (card = the difference).
 * out [n_out, N, C] fp32, n_out >= n: out[f, p] = the first C columns of the frame's point pick[f, p], the power as
 * 10 log10(p + 1e-8) (C == 5 only), minus the per-column mean over the frame's N output points when standardize, divided
 * by (population std + 1e-8) when also divide_by_std; gather, dB, mean and std in fp64 in a fixed order, one rounding to
 * fp32.  Rows n .. n_out - 1 are written as zeros (whole-tile padding for the bf16 eval GEMM).
 * pick [n, N] given: used as is (the host-drawn picks of the reference's generator: the parity path).  pick NULL: drawn
 * on the device from frame_key [n, 2] and seed with the counter-based hash documented in raw_frames.hip (card < N: identity
 * then (uint64(h(card + d)) * card) >> 32; card >= N: the N smallest of the keys (h(i), i), in key order);
 * datasets.device_picks_host restates it integer for integer.  pick_out [n, N] (may be NULL): the picks used.
 * A frame depends on its own detections and picks / key only: not on n, its position in the launch, or the grid.
 * A frame with card < 1 or card > PCAA_RAW_MAX_CARD, with offsets outside [0, P], or with a supplied pick outside
 * [0, card) is written as zeros (pick_out: -1) and *err_flag (may be NULL) is set; nothing faults, nothing is checked on
 * the host.  One workgroup per output frame; 1 <= N <= PCAA_RAW_MAX_POINTS, 1 <= C <= 5. */
#define PCAA_RAW_MAX_CARD 1024   /* detections of one raw frame */
#define PCAA_RAW_MAX_POINTS 1024 /* N: points of one processed frame */
int pcaa_frames_from_raw(const void* points, int points_f64, long P, const int* offsets, int n, const int* pick,
                         const int* frame_key, long seed, int N, int C, int standardize, int divide_by_std,
                         float* out, int n_out, int* pick_out, int* err_flag, void* stream);
/* ABI 29, added after it (the version is unchanged: a library without this entry point fails to load by name):
 * a training batch straight from the detections of a whole split.  points / offsets [F + 1] / pick [F, N] (may be
 * NULL) / frame_key [F, 2] are the tables of ALL F frames of a store; start [B] int32 is the store index of each crop's
 * first frame; out [B, T, N, C] fp32, out[b, t] = the frame pcaa_frames_from_raw writes for store frame start[b] + t
 * under the same pick row / key and seed, bit for bit (the same per-frame code, one workgroup per output frame): a
 * frame's bits depend on its detections, its key / pick row and the seed, not on where it stands in the batch.  Crops may
 * overlap and repeat.  The bad-frame rule of pcaa_frames_from_raw holds per frame (zeros, *err_flag set).  A crop with
 * start[b] < 0 or start[b] + T > F is written as zeros and sets *err_flag: nothing is read outside the tables, nothing is
 * checked on the host.  Vector stores when N * C % 4 == 0; no atomics on out.  B * T < 2^31, F < 2^31. */
int pcaa_crops_from_raw(const void* points, int points_f64, long P, const int* offsets, long F, const int* start, int B,
                        int T, const int* pick, const int* frame_key, long seed, int N, int C, int standardize,
                        int divide_by_std, float* out, int* err_flag, void* stream);
/* ABI 25: the same frames without their padding.  A padded frame repeats detections, and in eval mode the per-point
 * network f is a pure function of the point, so mean over the N padded rows of f(row) = (1/N) sum_i m_i f(p_i) over the
 * frame's DISTINCT picked detections p_i with multiplicities m_i (pcaa_segment_weighted_mean below pools that way).
 * Arguments as pcaa_frames_from_raw up to divide_by_std.  Two launches, nothing read back:
 *  1. u_off [n + 1] int32 = exclusive scan of u_cnt[f] = min(card_f, N), 1 for a frame whose offsets are bad (card < 1,
 *     card > PCAA_RAW_MAX_CARD, offsets outside [0, P]): a function of offsets alone;
 *  2. rows [M, C] fp32 and weight [M] fp32: rows u_off[f] .. of frame f are its distinct picked detections in order of
 *     first occurrence in its pick row, each exactly the value pcaa_frames_from_raw writes for that pick (the same code:
 *     the mean and std are those of the N padded rows), weight = the multiplicity (integer-valued).  The rows of a frame's
 *     allotment that its picks leave unused (supplied picks only) and the rows u_off[n] .. M - 1 are zero with weight 0.
 * A bad frame (the rule of pcaa_frames_from_raw, a supplied pick out of range included) is ONE zero row of weight N, the
 * rest of its allotment unused, pick_out -1, *err_flag set: pooled, it gives f(0), the padded path's all-zero frame.
 * For ascending offsets inside [0, P], u_off[n] <= min(P + n, n N); a frame whose rows would pass M (inconsistent
 * offsets) is not written and sets *err_flag, and pcaa_segment_weighted_mean returns zeros for it.  A frame's rows and
 * weights depend on its own detections and picks / key only.  1 <= M < 2^31, n * 1024 < 2^31. */
int pcaa_frames_from_raw_unique(const void* points, int points_f64, long P, const int* offsets, int n, const int* pick,
                                const int* frame_key, long seed, int N, int C, int standardize, int divide_by_std,
                                float* rows, float* weight, int* u_off, long M, int* pick_out, int* err_flag,
                                void* stream);
/* ABI 29, added after it like pcaa_crops_from_raw (the version is unchanged: a library without these entry points fails to
 * load by name): the three entry points above with a thinning stage in front of the draw -- a frame keeps at most k_f of its
 * detections before it is padded or subsampled to N: what a sparser radar would deliver, the reference's
 * force_pc_subsampling sweep, and point dropout for training, all from the same resident detections.  Arguments as the
 * neighbour of the same name, then keep (K), keep_min (Kmin) and keep_rule (PCAA_RAW_KEEP_FIRST / _RANDOM);
 * 1 <= keep_min <= keep <= PCAA_RAW_MAX_CARD.  With s the frame's chain state after seed_lo, seed_hi, key[0], key[1] and
 * t = absorb(s, 0x6b656570) (raw_frames.hip: absorb(s, w) = mix((s ^ w) + 0x9e3779b9)):
 *   k_f = keep_min + ((uint64)absorb(t, 0xffffffff) * (keep - keep_min + 1) >> 32), drawn only when keep_min < keep;
 *   k_f >= card: the frame's picks and output bits are exactly those of the entry point without _thin;
 *   FIRST: the kept raw indices are 0 .. k_f - 1;  RANDOM: the k_f detections with the smallest (absorb(t, i), i), in
 *   rank order;  then the draw of pcaa_frames_from_raw, unchanged, over the k_f kept points (repeat-pad if k_f < N, a rank
 *   subset otherwise), mapped back through the keep list: pick_out holds RAW indices.
 * datasets.device_picks_host(..., keep, keep_min, keep_rule) restates it integer for integer.  The picks are drawn on the
 * device only: pick must be NULL (supplied picks decide by themselves) and frame_key non-NULL when there are frames; these,
 * the range of keep / keep_min and keep_rule outside {0, 1} are argument errors, refused before any launch.  A frame has
 * the same bits in all three; the bad-frame rule, the zero padding rows and the launches per call are those of the
 * neighbours.  pcaa_frames_from_raw_unique_thin: u_cnt[f] = min(card_f, k_f, N) (a bad frame: 1), so u_off depends on keep
 * and, when keep_min < keep, on seed and frame_key as well; u_off[n] <= min(P + n, n min(N, keep)). */
#define PCAA_RAW_KEEP_FIRST 0
#define PCAA_RAW_KEEP_RANDOM 1
int pcaa_frames_from_raw_thin(const void* points, int points_f64, long P, const int* offsets, int n, const int* pick,
                              const int* frame_key, long seed, int N, int C, int standardize, int divide_by_std,
                              float* out, int n_out, int* pick_out, int* err_flag, void* stream, int keep, int keep_min,
                              int keep_rule);
int pcaa_crops_from_raw_thin(const void* points, int points_f64, long P, const int* offsets, long F, const int* start,
                             int B, int T, const int* pick, const int* frame_key, long seed, int N, int C,
                             int standardize, int divide_by_std, float* out, int* err_flag, void* stream, int keep,
                             int keep_min, int keep_rule);
int pcaa_frames_from_raw_unique_thin(const void* points, int points_f64, long P, const int* offsets, int n,
                                     const int* pick, const int* frame_key, long seed, int N, int C, int standardize,
                                     int divide_by_std, float* rows, float* weight, int* u_off, long M, int* pick_out,
                                     int* err_flag, void* stream, int keep, int keep_min, int keep_rule);
/* ABI 29, added after them in the same way (the version is unchanged: a library without these entry points fails to load
 * by name): the same three with an AUGMENTATION stage between the gather and the statistics -- the picked detections are
 * moved in fp64, after the power column has become dB and BEFORE the frame is centred, then mean, std, the one rounding
 * and the stores follow unchanged.  Arguments as the _thin neighbour, then aug: PCAA_RAW_AUG_PARAMS doubles on the HOST
 * (read by the launcher, handed to the kernel by value), indexed by the macros below.
 *   per TRACK (every frame of a track shares them: overlapping windows agree, the dynamics between frames survive):
 *     u = absorb(absorb(absorb(absorb(0x9e3779b9, seed_lo), seed_hi), key[0]), 0x6175676d "augm"); key[1] is not absorbed;
 *     w_j = absorb(u, j), r_j = (w_j + 0.5) 2^-32 in fp64, j = 0 .. 3;
 *     theta = yaw (2 r_0 - 1);  m = w_1 >> 31 (used when mirror != 0);  a = scale_lo + (scale_hi - scale_lo) r_2;
 *     v = speed_lo + (speed_hi - speed_lo) r_3;
 *   per DETECTION, keyed by its RAW index i in its frame (not by the padded row: every copy of a detection carries the
 *   same noise, so padded duplicates stay bit-equal rows and the compact-row route stays exact):
 *     n = absorb(s, 0x6e6f6973 "nois"), s the frame's chain state after seed_lo, seed_hi, key[0], key[1]; q = absorb(n, i);
 *     r1 = (absorb(q, 2c) + 0.5) 2^-32, r2 = (absorb(q, 2c + 1) + 0.5) 2^-32;  g(i, c) = sqrt(-2 ln r1) cos(2 pi r2);
 *   per picked point, in this order, fp64, no contraction:
 *     1. val[c] += sigma[c] g(i, c) for c < C with sigma[c] != 0 (metres, m/s, dB for the power column);
 *     2. x, y, z *= a; doppler *= v;   3. x = -x when m;   4. (x, y) <- (x cos theta - y sin theta, x sin theta + y cos theta).
 *   A step whose parameters are neutral (sigma[c] == 0, lo == hi == 1, mirror == 0, yaw == 0) is skipped.  Rotation about
 *   the radar's vertical axis and the mirror across boresight leave range and radial velocity alone: after centring they
 *   are what a person at another azimuth delivers, which is why they act before centring and never touch the Doppler.
 * datasets.frames_from_picks(..., augment, seed, keys) restates the stage in numpy.  keep == 0 is allowed here and means
 * no thinning (keep_min, keep_rule are then ignored); pick may be supplied, then keep must be 0; frame_key must be non-NULL
 * when there are frames (with supplied picks too).  Argument errors, refused before any launch: aug NULL, yaw outside
 * [0, pi] or not finite, yaw != 0 with C < 2, scale_lo <= 0, speed_lo <= 0, lo > hi, a range or sigma that is not finite,
 * a negative sigma.  A frame has the same bits in all three; the bad-frame rule, the zero padding rows, the launches per
 * call and u_off are those of the neighbours: u_off does not depend on aug.  The kernels of the entry points above are the
 * instantiations they were before these existed. */
#define PCAA_RAW_AUG_PARAMS 11
#define PCAA_RAW_AUG_YAW 0      /* radians, 0 .. pi: theta uniform in (-yaw, yaw) */
#define PCAA_RAW_AUG_MIRROR 1   /* != 0: x -> -x for the tracks whose bit m is set */
#define PCAA_RAW_AUG_SCALE_LO 2 /* x, y, z times a factor uniform in [lo, hi] */
#define PCAA_RAW_AUG_SCALE_HI 3
#define PCAA_RAW_AUG_SPEED_LO 4 /* doppler times a factor uniform in [lo, hi] */
#define PCAA_RAW_AUG_SPEED_HI 5
#define PCAA_RAW_AUG_SIGMA 6    /* sigma[5]: x, y, z, doppler, power (dB) */
int pcaa_frames_from_raw_aug(const void* points, int points_f64, long P, const int* offsets, int n, const int* pick,
                             const int* frame_key, long seed, int N, int C, int standardize, int divide_by_std,
                             float* out, int n_out, int* pick_out, int* err_flag, void* stream, int keep, int keep_min,
                             int keep_rule, const double* aug);
int pcaa_crops_from_raw_aug(const void* points, int points_f64, long P, const int* offsets, long F, const int* start,
                            int B, int T, const int* pick, const int* frame_key, long seed, int N, int C,
                            int standardize, int divide_by_std, float* out, int* err_flag, void* stream, int keep,
                            int keep_min, int keep_rule, const double* aug);
int pcaa_frames_from_raw_unique_aug(const void* points, int points_f64, long P, const int* offsets, int n,
                                    const int* pick, const int* frame_key, long seed, int N, int C, int standardize,
                                    int divide_by_std, float* rows, float* weight, int* u_off, long M, int* pick_out,
                                    int* err_flag, void* stream, int keep, int keep_min, int keep_rule, const double* aug);
/* ------------------------------------------------------------------ scene frames -> people (scene.hip)
 * Added after ABI 29 like pcaa_crops_from_raw (the version is unchanged: a library without these entry points fails to
 * load by name).  A scene frame is one radar frame with everybody in view plus clutter, in the layout of
 * pcaa_frames_from_raw: points [P, 5] fp32 / fp64 (x, y, z, doppler, linear power), offsets [n + 1].
 * pcaa_scene_cluster clusters every frame by density, one workgroup per frame, one launch:
 *   d2(i, j) = dx*dx + dy*dy + wz2*dz*dz + wv2*dv*dv in fp64 from the stored values, in that order, no contraction;
 *   i, j neighbours iff d2 <= eps2 (self included); i core iff it has >= min_points neighbours; clusters = connected
 *   components of the core points; a non-core point with a core neighbour joins the cluster of its nearest one (smallest
 *   d2, lowest index on exact ties) and links nothing; the rest is noise (-1); ids 0 .. c - 1 by ascending lowest core
 *   index; clusters with id >= Cmax become noise and set bit 1 of *err.  scene.cluster_host restates it bit for bit.
 * Outputs: label int32 [P]; n_clusters int32 [n] (= min(c, Cmax)); cluster_count int32 [n, Cmax]; centroid fp32
 * [n, Cmax, 4] = (float)(sum64 / count) of x, y, z, doppler, the fp64 sum in ascending detection order, unused entries
 * zero; grouped [P, 5] in the input type: frame f's rows as cluster 0, cluster 1, ..., then noise, each group in ascending
 * detection order and bit-equal to the input rows; seg_off int32 [n, Cmax + 1], absolute rows: cluster c of frame f owns
 * grouped[seg_off[f, c] : seg_off[f, c + 1]], the noise grouped[seg_off[f, Cmax] : offsets[f + 1]].
 * A frame without detections is legal (zero clusters, seg_off = offsets[f]).  A frame with more than PCAA_RAW_MAX_CARD
 * detections sets bit 0 of *err and is all noise (grouped = its rows, seg_off = offsets[f]); a frame whose offsets leave
 * [0, P] or run backwards sets bit 0, has zero clusters, seg_off = 0, and none of its rows is read or written.  Rows of
 * label / grouped that no frame owns are not written.  Frames are checked one by one, not against each other: offsets that
 * are not monotone (0, 10, 5, 15) give two valid frames that share rows, and those rows of label / grouped then hold
 * either frame's values -- in bounds, *err not set; the per-frame tables stay exact.  The centroid's fp64 sum starts from the
 * cluster's first member (np.cumsum(...)[-1] / count on the host, bit for bit).  Every loop of the kernel is bounded by the frame's cardinality:
 * no input can hang it; *err (required) is its only report.  1 <= Cmax <= PCAA_SCENE_MAX_CLUSTERS, min_points >= 1,
 * eps2 / wz2 / wv2 finite and >= 0, P < 2^31; grouped may not alias points. */
#define PCAA_SCENE_MAX_CLUSTERS 64
int pcaa_scene_cluster(const void* points, int points_f64, long P, const int* offsets, int n, double eps2, double wz2,
                       double wv2, int min_points, int Cmax, int* label, int* n_clusters, int* cluster_count,
                       float* centroid, void* grouped, int* seg_off, int* err, void* stream);
/* out rows out_off[o] .. out_off[o + 1] - 1 = the rows of src [P, 5] from seg_start[o] on, o < M, one launch: the
 * (points, offsets = out_off) that pcaa_frames_from_raw takes, from the segments the host chose.  out [R, 5] in src's
 * type.  A segment that leaves [0, P], or whose out rows leave [0, R] or run backwards, is skipped and sets *err (may be
 * NULL). */
int pcaa_gather_segments(const void* src, int src_f64, long P, const int* seg_start, const int* out_off, int M, void* out,
                         long R, int* err, void* stream);
/* ABI 25 (segment_pool.hip): out[f, c] = (1 / N) sum_{r = u_off[f]}^{u_off[f + 1] - 1} weight[r] * v(a[r * lda + c]) for
 * n frames, a [M, ch] fp32 or bf16 (dtype) with leading dimension lda, out [n, ch] fp32.  v = identity; with scale / shift
 * [ch] (both or neither) a is a pre-BatchNorm y and v = ELU(a * scale[c] + shift[c]) (fused multiply-add, expm1f).  fp32
 * accumulation in a fixed order that is a function of the segment alone (four row lanes, each ascending, added in lane
 * order, one division by N): the result does not depend on n or the grid.  16-byte loads: ch % 8 == 0, lda % 8 == 0,
 * a / out / scale / shift 16-B aligned.  Segments of any length (0 rows: zeros).  A segment with u_off[f] < 0,
 * u_off[f + 1] < u_off[f] or u_off[f + 1] > M is written as zeros and sets *err_flag (may be NULL): no fault. */
int pcaa_segment_weighted_mean(const void* a, int dtype, long lda, const float* weight, const int* u_off, int n, long M,
                               int ch, int N, const float* scale, const float* shift, float* out, int* err_flag,
                               void* stream);
/* ABI 27 (segment_pool.hip): the adjoint of pcaa_segment_weighted_mean in its (scale, shift) form, and the ragged form of
 * pcaa_bn_eval_act_bwd's (dpool, y) mode.  For row r of segment f (u_off[f] <= r < u_off[f + 1]) and channel c:
 *   g = dpool[f, c] * (weight[r] / N),  dz = g * ELU'(y[r, c] * scale[c] + shift[c]),  dy[r, c] = scale[c] * dz
 * (dy in y's dtype, fp32 or bf16; y and dy [M, ch] with the same leading dimension lda; dpool [n, ch] fp32), and
 *   stats += { sum_r dz, sum_r dz * (y - mean) * rstd }   ([nrep][2][ch] fp64, ZEROED by the caller)
 * with (mean, rstd) of pcaa_bn_eval_moments; pcaa_bn_eval_bwd_finalize turns them into dgamma, dbeta and dbias.  The
 * statistics are summed in fp32 over at most 128 consecutive rows of a segment, then in fp64 (one fp64 atomic per
 * workgroup, statistic and channel), so their error does not grow with the cardinality.  dy is zero-filled by the call
 * before its kernel runs: every row that no valid segment owns (the rows from u_off[n] on, the rows of a bad segment)
 * is zero.  A segment with u_off[f] < 0, u_off[f + 1] < u_off[f] or u_off[f + 1] > M contributes nothing and sets
 * *err_flag (may be NULL): no fault.  Valid segments must be DISJOINT: validity is checked segment by segment.  With
 * non-decreasing offsets they are; two valid segments can only share rows behind a segment that runs backwards, which
 * sets *err_flag -- in such a call the shared rows of dy hold the value of either segment and the statistics count them
 * once per segment (nothing faults, every other row is as stated); a caller that finds the flag set discards the result.
 * One workgroup per (segment, 512 channels), 16-byte accesses: ch % 8 == 0, lda % 8 == 0, dpool / y / dy / scale / shift /
 * mean / rstd 16-B aligned.  dy may not alias y. */
int pcaa_segment_weighted_mean_bwd(const float* dpool, const void* y, void* dy, int dtype, long lda, const float* weight,
                                   const int* u_off, int n, long M, int ch, int N, const float* scale,
                                   const float* shift, const float* mean, const float* rstd, double* stats, int nrep,
                                   int* err_flag, void* stream);
/* ABI 26 (frame_unique.hip): the same compact table from frames whose padding is already WRITTEN OUT (stored crops,
 * processed tracks): frames [n, N, C] fp32, contiguous, point-major; 1 <= N <= PCAA_RAW_MAX_POINTS, 1 <= C <= 5,
 * n * N < 2^31.  Two rows of a frame are the same point iff all their C 32-bit words are equal as BITS (-0.0 != +0.0, two
 * NaNs are equal iff their payloads are).  u_off [n + 1] int32 = exclusive scan of the number of distinct rows per frame:
 * two launches whatever n is (a count per frame, one workgroup's scan with a carry), nothing read back.  One workgroup per
 * frame, the frame in LDS, integer compares only; 16-byte loads for C == 4 on a 16-B aligned base, 4-byte loads else. */
int pcaa_frames_unique_offsets(const float* frames, int n, int N, int C, int* u_off, void* stream);
/* ABI 26: the rows of frames a .. b - 1 (0 <= a <= b <= n) of the same frames and u_off, one launch.  With
 * base = u_off[a], frame f owns rows u_off[f] - base .. u_off[f + 1] - base - 1 of rows [M, C] fp32 / weight [M] fp32: its
 * distinct rows in order of first occurrence, each bit-equal to the source row, weight = the multiplicity (a frame's
 * weights add up to N).  Rows u_off[b] - base .. M - 1 are zero with weight 0.  seg_off [b - a + 1] int32 receives the
 * rebased offsets pcaa_segment_weighted_mean takes (an offset outside [0, M]: -1, a bad segment there).  A frame whose
 * given segment is not exactly its number of distinct rows inside [0, M] (a u_off from other frames, an M too small)
 * writes nothing and sets *err_flag (may be NULL); the call still returns 0.  The search runs again here: no scratch is
 * kept from pcaa_frames_unique_offsets.  1 <= M < 2^31. */
int pcaa_frames_unique(const float* frames, int n, int N, int C, const int* u_off, int a, int b, float* rows,
                       float* weight, long M, int* seg_off, int* err_flag, void* stream);
/* The adjoint w.r.t. the layer input in one launch (replaces dcol = dy . W on the im2col layout followed by
 * pcaa_dtc_col2im): da[(b,t)][ci] = sum_{co,tap} dy[b][t+(2-tap)*d][co] * W[co][ci][tap].
 *  - dy given, or formed on load from this layer's dz, y and the coefficients of pcaa_bn_bwd_finalize
 *    (dy = coef0*dz + coef1*y + coef2: the second half of the BatchNorm backward, no separate pass); dy_out
 *    (optional) receives the staged dy for the weight gradient;
 *  - ep_stats given: `out` is dz of the layer BELOW, da * ELU'(ep_y*ep_scale + ep_shift), and its BatchNorm-
 *    backward statistics {sum dz, sum dz*(ep_y-ep_mean)*ep_rstd} are accumulated into ep_stats[nrep][2][cin]
 *    (the first half of that layer's backward, no separate pass); needs ksplit == 1.
 * ksplit > 1 (cout > 512) writes slabs for pcaa_splitk_reduce, as the forward. */
int pcaa_dtc_conv_dgrad_ksplit(int B, int cin, int cout);
int pcaa_dtc_conv_dgrad(const float* dy, const float* dz, const float* y, const float* coef, float* dy_out,
                        const float* W, float* out, const float* ep_y, const float* ep_scale,
                        const float* ep_shift, const float* ep_mean, const float* ep_rstd, double* ep_stats,
                        int nrep, int B, int T, int cin, int cout, int dilation, int ksplit, long slab_stride,
                        void* stream);
int pcaa_dtc_conv_dgrad_bf16(const float* dy, const float* dz, const float* y, const float* coef, float* dy_out,
                        const float* W, float* out, const float* ep_y, const float* ep_scale,
                        const float* ep_shift, const float* ep_mean, const float* ep_rstd, double* ep_stats,
                        int nrep, int B, int T, int cin, int cout, int dilation, int ksplit, long slab_stride,
                        void* stream);      /* likewise, the adjoint */

/* ------------------------------------------------------------------ MLP heads, fused
 * CGEncoder's MLP_sup1 / MLP_head / MLP_sup2 (models.py:252-277, applied at :285-292) and the
 * decoder projection head Sequential(Linear(32,64), ELU) (PCAA_ablation.py:778-781) as one forward
 * and one backward launch (fp32 FMAs, exact in both precision modes):
 *   sup_fv = ELU(W1 x4 + b1)  [B,32];   h = ELU(Wh sup_fv + bh)  [B,16]   (Wh null: no projection head)
 *   logits = ELU(W2 (h | sup_fv) + b2)  [B,K];   hproj = ELU(Wg sup_fv + bg)  [B,64]   (Wg null: skipped)
 * Backward: d_logits / d_hproj are gradients w.r.t. those (post-ELU) outputs, d_sup is whatever else
 * arrives at sup_fv (critic, decoder without head); any of the three may be null.  All weight / bias
 * gradients and dx4 [B,512] are WRITTEN (not accumulated).  pcaa_heads_supported: widths
 * 512/32/(16|0)/(64|0); the backward keeps all rows in LDS: B <= 64, K <= 8. */
int pcaa_heads_supported(int B, int K, int d_in, int d_sup, int d_head, int d_proj, int backward);
int pcaa_heads_fwd(const float* x4, const float* W1, const float* b1, const float* Wh, const float* bh,
                   const float* W2, const float* b2, const float* Wg, const float* bg, float* sup_fv,
                   float* h, float* logits, float* hproj, int B, int K, void* stream);
int pcaa_heads_bwd(const float* x4, const float* sup_fv, const float* h, const float* logits,
                   const float* hproj, const float* W1, const float* Wh, const float* W2,
                   const float* Wg, const float* d_logits, const float* d_sup, const float* d_hproj,
                   float* dW1, float* db1, float* dWh, float* dbh, float* dW2, float* db2, float* dWg,
                   float* dbg, float* dx4, int B, int K, void* stream);

/* ------------------------------------------------------------------ split-operand parity mode (round 3, "fp16x3")
 * A parity-grade product without the 1/16-rate fp32 MFMA: an fp32 operand e is kept as hi = fp16(s e),
 * lo = fp16(s e - hi) -- its "[hi | lo] image": for a row-major [rows, ch] tensor a 16-bit [rows, 2 ch] with lo at
 * column ch + c (the same bytes as the fp32 tensor); s (img_scale) is a power of two that keeps the tensor in fp16's
 * normal range (activations 1, weights 2^8, gradients 2^16) -- and the product is hi.hi + lo.hi + hi.lo on the f16
 * MFMA pipe (the bf16 rate), fp32 accumulate, times out_scale = 1 / (s_A s_B): 22 mantissa bits per operand.
 * pcaa_gemm_split3: C[M,N] fp32 = A.B^T from images; layout KC: A [M, 2K], B [N, 2K]; RC: A [K, 2M], B [K, 2N]
 * (contraction over the rows: the weight gradient); colstats as pcaa_gemm.  pcaa_gemm_slabs_split3: slab split-K
 * (pcaa_gemm_split3_num_splits slabs, reduce with pcaa_splitk_reduce).  Whole 256x256 tiles, K % 64 == 0.
 * Producers of images: pcaa_split_f16 (any fp32 matrix, optionally transposed), pcaa_bn_act_fwd_split,
 * pcaa_bn_bwd_dy_fused_split, pcaa_pointnet_in_apply with a_dtype = PCAA_SPLIT_F16 (img_scale 1). */
int pcaa_gemm_split3_supported(int M, int N, int K);
int pcaa_gemm_split3(const void* A, const void* B, int layout, long lda, long ldb, float* C, long ldc, int M,
                     int N, int K, double* colstats, int nrep, float out_scale, void* stream);
int pcaa_gemm_split3_num_splits(int K, int split_k);
int pcaa_gemm_slabs_split3(const void* A, const void* B, int layout, long lda, long ldb, float* slabs,
                           long slab_stride, int M, int N, int K, int split_k, float out_scale, void* stream);
int pcaa_split_f16(const float* src, void* dst_img, long rows, int ch, int transpose, float img_scale, void* stream);
/* Range guard of the images (round 4): fp16 holds |x| <= 65504 while the fp32 tensors of the reference have no limit.
 * Every image producer saturates a scaled value that leaves that range (finite hi, lo = 0) and sets *dev_flag
 * (device int32, registered per calling thread; NULL = no flag) to 1; NaN inputs set it too and stay NaN in the image.  The caller reads the
 * flag when it next synchronises (PCAATrainer.check()) and must not trust that step's products. */
int pcaa_set_range_flag(int* dev_flag);
int pcaa_bn_act_fwd_split(const float* y, void* a_img, const float* scale, const float* shift, long rows,
                          int ch, float img_scale, void* stream);
int pcaa_bn_bwd_dy_fused_split(const float* da, const float* dpool, int group_rows, float pool_scale,
                               const float* y, void* dy_img, const float* scale, const float* shift,
                               const float* coef, long rows, int ch, float img_scale, void* stream);

/* ------------------------------------------------------------------ OR-CED baseline heads (round 3)
 * ORCEDEncoder's three Linear heads and the reparametrisation (reference models.py:489-505):
 *   mu = x4.Wmu^T + bmu, logvar = x4.Wlv^T + blv, sup_fv = mu + eps*exp(0.5*logvar), logits = sup_fv.Wc^T + bc
 * (x4 [B,d_in], eps [B,d_lat]: the caller's randn draw), their backward (any of d_logits / d_sup / d_mu / d_logvar may
 * be NULL = zero; ws: 2*B*d_lat floats of scratch; dx4 may be NULL), and CG_kl_divergence (utils.py:72-85):
 *   loss = mean_b( -0.5 sum_j (1 + logvar - (mu - mu_k)^2 - exp(logvar)) ),  gradients scaled by gscale / B. */
int pcaa_orced_heads_supported(int B, int K, int d_in, int d_lat);
int pcaa_orced_heads_fwd(const float* x4, const float* Wmu, const float* bmu, const float* Wlv, const float* blv,
                         const float* eps, const float* Wc, const float* bc, float* mu, float* logvar, float* sup_fv,
                         float* logits, int B, int K, int d_in, int d_lat, void* stream);
int pcaa_orced_heads_bwd(const float* x4, const float* eps, const float* logvar, const float* sup_fv,
                         const float* Wmu, const float* Wlv, const float* Wc, const float* d_logits,
                         const float* d_sup, const float* d_mu, const float* d_logvar, float* ws, float* dWmu,
                         float* dbmu, float* dWlv, float* dblv, float* dWc, float* dbc, float* dx4, int B, int K,
                         int d_in, int d_lat, void* stream);
int pcaa_orced_kl(const float* mu, const float* logvar, const float* mu_k, float* loss, float* d_mu,
                  float* d_logvar, float* d_muk, float gscale, int B, int d_lat, void* stream);
/* ABI 22: OR-CED's triplet term (reference train_ORCED.py:9,30,34: miners.MultiSimilarityMiner(epsilon) feeding
 * losses.TripletMarginLoss(margin) of pytorch_metric_learning 1.6.0, as restated by orced.multi_similarity_miner /
 * orced.triplet_margin_loss) in dense form, with e = x / max(|x|, 1e-12), S = e e^T, D[a,j] = |e_a - e_j|:
 *   P[a,p] = same label, p != a, S[a,p] - epsilon < max over a's negatives of S[a,.]   (no negative: P empty)
 *   N[a,n] = other label,        S[a,n] + epsilon > min over a's positives of S[a,.]   (no positive: N empty)
 *   h = D[a,p] - D[a,n] + margin over all (a, p, n) with P[a,p] and N[a,n]
 *   *loss = sum_{h>0} h / #{h>0}, 0 with a zero gradient where nothing is mined or no hinge is positive
 *   dx [B,d_lat] (may be NULL) = gscale * dloss/dx, through the normalisation; a pair at D == 0 contributes nothing
 *   (torch.cdist's backward rule).
 * x [B,d_lat] fp32 with non-zero rows, labels [B] int64.  Three launches on `stream`, no atomics, no host read: the
 * same inputs give the same bits.  ws: (B*B + B*d_lat + 4*B) floats of scratch, 8-byte aligned. */
int pcaa_orced_triplet_supported(int B, int d_lat);
int pcaa_orced_triplet(const float* x, const long long* labels, float epsilon, float margin, float gscale, float* ws,
                       float* loss, float* dx, int B, int d_lat, void* stream);
/* ABI 22: the ensemble open-set rule of inference_ORCED.py:18-132 after its training-set statistics, one wave per
 * sample.  Per sample: z [n,d_lat] fp32, re [n] fp32, pred [n] int64; per class, fp64: mean_z, sd_z [K,d_lat] (sd_z is the
 * SQUARE ROOT of the class's std: the reference hands the std to scipy as a variance, :107) and thr_re [K].
 *   p_k = prod_d Phi(dev/sd) - prod_d Phi(-dev/sd), dev = |z - mean_k|, in fp64 (Phi(t) = erfc(-t / sqrt 2) / 2)
 *   out [n] = K where p_k > thresholds_g for EVERY k, or (double)re > thr_re[pred] (or pred outside [0, K)); else pred.
 * p [K,n] fp64 may be NULL. */
int pcaa_orced_ood(const float* z, const float* re, const long long* pred, const double* mean_z, const double* sd_z,
                   const double* thr_re, double thresholds_g, long long* out, double* p, int n, int K, int d_lat,
                   void* stream);

/* ------------------------------------------------------------------ optimizer
 * torch.optim.Adam (no weight decay, no amsgrad; PCAA_ablation.py:820-833) on a
 * flat fp32 buffer. `step` is the 1-based step count after this update.  max_blocks (0 =
 * default, fill the device) caps the grid: <= 1024 selects the 4-quads-per-thread kernel that
 * saturates HBM from 1-2 workgroups per CU, for updates that run beside other kernels. */
int pcaa_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n,
                   float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                   int max_blocks, void* stream);
/* The same update with the step count kept ON THE DEVICE, so that a captured hipGraph of the
 * train step replays without per-step host arguments: pcaa_adam_advance does
 * `*step_dev += 1; coef_dev[0] = lr / (1 - beta1^step); coef_dev[1] = 1 / sqrt(1 - beta2^step)`
 * (fp64, the arithmetic of pcaa_adam_step) once per optimizer step; pcaa_adam_step_dev applies the
 * update to any sub-range of the flat buffer with those two scalars read from coef_dev. */
int pcaa_adam_advance(int* step_dev, float* coef_dev, float lr, float beta1, float beta2, void* stream);
int pcaa_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n,
                       float beta1, float beta2, float eps, const float* coef_dev, float grad_scale,
                       int max_blocks, void* stream);
/* pcaa_adam_step_dev with the gradient given as bf16 (n elements, 8-B aligned): the data-parallel step with bf16
 * gradient buckets hands the reduced bucket to the optimizer as it came off the wire, without widening it into the
 * fp32 gradient buffer first (one pass over the decoder's 157 M gradients less, and half the bytes of Adam's read). */
int pcaa_adam_step_dev_g16(float* param, const void* grad_bf16, float* exp_avg, float* exp_avg_sq, long n,
                           float beta1, float beta2, float eps, const float* coef_dev, float grad_scale,
                           int max_blocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PCAA_HIP_H */
