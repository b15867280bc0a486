// Segmented weighted mean over the rows of a compact table (pcaa_segment_weighted_mean): the pooling step of the eval
// PointNet when a frame's duplicated points were computed once (pcaa_frames_from_raw_unique, raw_frames.hip):
//   out[f, c] = (1 / N) * sum_{r = u_off[f]}^{u_off[f + 1] - 1} weight[r] * v(a[r, c])
// v = identity, or ELU(a * scale[c] + shift[c]) when (scale, shift) are given (a is then a pre-BatchNorm y).
//
// One workgroup of 256 threads per (frame, 512 channels): thread (g, l) = (tid % 64, tid / 64) owns the 8 channels
// 8 g .. 8 g + 7 of the block's channel range and the rows u0 + l, u0 + l + 4, ...; a wave reads 1 KiB (bf16) or two
// times 1 KiB (fp32) of one row per step with 16-byte loads.  fp32 accumulation in a FIXED order: each row lane adds its
// rows in ascending order with one fused multiply-add per element, the four row lanes are added in lane order through
// LDS, one division by N.  The order is a function of the segment alone, so a frame's result does not depend on n, on its
// position in the launch or on the grid.  A segment that leaves [0, M] (or runs backwards) is written as zeros and sets
// *err_flag: no fault.
#include "common.h"

namespace {

constexpr int POOL_THREADS = 256;
constexpr int POOL_GROUPS = 64;                   // 8-channel groups per block: 512 channels
constexpr int POOL_LANES = POOL_THREADS / POOL_GROUPS;
constexpr int SEG_STAT_ROWS = 128;               // consecutive rows of a segment whose statistics are summed in fp32

__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
  const f32x4 a = load4(p), b = load4(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void load8(const bf16_t* p, float (&v)[8]) {
  const uint4 raw = *reinterpret_cast<const uint4*>(p);
  v[0] = __uint_as_float(raw.x << 16); v[1] = __uint_as_float(raw.x & 0xffff0000u);
  v[2] = __uint_as_float(raw.y << 16); v[3] = __uint_as_float(raw.y & 0xffff0000u);
  v[4] = __uint_as_float(raw.z << 16); v[5] = __uint_as_float(raw.z & 0xffff0000u);
  v[6] = __uint_as_float(raw.w << 16); v[7] = __uint_as_float(raw.w & 0xffff0000u);
}

template <typename T, bool AFFINE>
__global__ __launch_bounds__(POOL_THREADS) void segment_weighted_mean_kernel(
    const T* __restrict__ a, long lda, const float* __restrict__ weight, const int* __restrict__ u_off, long M, int ch,
    int N, const float* __restrict__ scale, const float* __restrict__ shift, float* __restrict__ out,
    int* __restrict__ err) {
#pragma clang fp contract(off)
  __shared__ float s_part[POOL_LANES][POOL_GROUPS * 8];
  const int g = threadIdx.x % POOL_GROUPS, l = threadIdx.x / POOL_GROUPS;
  const long f = blockIdx.x;
  const int c0 = ((int)blockIdx.y * POOL_GROUPS + g) * 8;
  const bool live = c0 < ch;                      // ch % 8 == 0: a group is whole or absent
  long u0 = u_off[f], u1 = u_off[f + 1];
  if (u0 < 0 || u1 < u0 || u1 > M) {              // uniform over the workgroup
    if (err != nullptr && threadIdx.x == 0 && blockIdx.y == 0) atomicOr(err, 1);
    u0 = u1 = 0;                                  // an empty sum: zeros
  }
  float acc[8], sc[8], sh[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  if (live) {
    if (AFFINE) {
      load8(scale + c0, sc);
      load8(shift + c0, sh);
    }
    for (long r = u0 + l; r < u1; r += POOL_LANES) {
      const float w = weight[r];
      float v[8];
      load8(a + r * lda + c0, v);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float x = AFFINE ? elu_f(__builtin_fmaf(v[k], sc[k], sh[k])) : v[k];
        acc[k] = __builtin_fmaf(w, x, acc[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s_part[l][g * 8 + k] = acc[k];
  }
  __syncthreads();
  if (live && l == 0) {
    float o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float s = s_part[0][g * 8 + k];
#pragma unroll
      for (int j = 1; j < POOL_LANES; ++j) s += s_part[j][g * 8 + k];
      o[k] = s / (float)N;
    }
    float* dst = out + f * (long)ch + c0;
    const f32x4 lo = {o[0], o[1], o[2], o[3]}, hi = {o[4], o[5], o[6], o[7]};
    store4(dst, lo);
    store4(dst + 4, hi);
  }
}

__device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
  const f32x4 lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
  store4(p, lo);
  store4(p + 4, hi);
}
__device__ __forceinline__ void store8(bf16_t* p, const float (&v)[8]) {
  bf16x8 b;
#pragma unroll
  for (int k = 0; k < 8; ++k) b[k] = (bf16_t)v[k];
  *reinterpret_cast<bf16x8*>(p) = b;
}

// The adjoint of the (scale, shift) form above, and the ragged form of bn_eval_act_bwd_kernel's pooled mode
// (elementwise.hip): for row r of segment f
//   g = dpool[f, c] * (weight[r] / N),  dz = g * ELU'(y[r, c] * scale[c] + shift[c]),  dy[r, c] = scale[c] * dz
// and the BatchNorm statistics {sum dz, sum dz * (y - mean) * rstd}.  The same grid and thread map as the forward kernel:
// a workgroup knows its segment, so no row searches for its owner, and dpool[f, 8 channels] stays in registers.  A row
// lane sums its rows of at most 128 consecutive rows of the segment in fp32 (32 rows), then adds them to fp64 registers;
// the four lanes meet in LDS in fp64 and lane 0 issues one fp64 atomic per (workgroup, statistic, channel) into replica
// blockIdx.x % nrep -- the layout pcaa_bn_eval_bwd_finalize reads.  The launcher zero-fills dy first: this kernel writes
// the rows of valid segments only, so rows behind u_off[n] and rows of a bad segment are zeros, never stale memory.
template <typename T>
__global__ __launch_bounds__(POOL_THREADS) void segment_weighted_mean_bwd_kernel(
    const float* __restrict__ dpool, const T* __restrict__ y, long lda, const float* __restrict__ weight,
    const int* __restrict__ u_off, long M, int ch, int N, const float* __restrict__ scale,
    const float* __restrict__ shift, const float* __restrict__ mean, const float* __restrict__ rstd,
    T* __restrict__ dy, double* __restrict__ stats, int nrep, int* __restrict__ err) {
  __shared__ double s_red[POOL_LANES - 1][2][POOL_GROUPS * 8];
  const int g = threadIdx.x % POOL_GROUPS, l = threadIdx.x / POOL_GROUPS;
  const long f = blockIdx.x;
  const int c0 = ((int)blockIdx.y * POOL_GROUPS + g) * 8;
  const bool live = c0 < ch;                      // ch % 8 == 0: a group is whole or absent
  const long u0 = u_off[f], u1 = u_off[f + 1];
  if (u0 < 0 || u1 < u0 || u1 > M) {              // uniform over the workgroup
    if (err != nullptr && threadIdx.x == 0 && blockIdx.y == 0) atomicOr(err, 1);
    return;
  }
  if (u0 == u1) return;                           // (uniform) an empty segment owns no row and adds nothing
  double d1[8], d2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) d1[k] = d2[k] = 0.0;
  if (live) {
    float dp[8], sc[8], sh[8], mu[8], rs[8];
    load8(dpool + f * (long)ch + c0, dp);
    load8(scale + c0, sc);
    load8(shift + c0, sh);
    load8(mean + c0, mu);
    load8(rstd + c0, rs);
    for (long base = u0; base < u1; base += SEG_STAT_ROWS) {
      const long end = base + SEG_STAT_ROWS < u1 ? base + SEG_STAT_ROWS : u1;
      float s1[8], s2[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) s1[k] = s2[k] = 0.f;
      for (long r = base + l; r < end; r += POOL_LANES) {
        const float wn = weight[r] / (float)N;
        float v[8], o[8];
        load8(y + r * lda + c0, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float dz = (dp[k] * wn) * elu_grad_from_pre_t<T>(v[k] * sc[k] + sh[k]);
          o[k] = sc[k] * dz;
          s1[k] += dz;
          s2[k] += dz * ((v[k] - mu[k]) * rs[k]);
        }
        store8(dy + r * lda + c0, o);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        d1[k] += (double)s1[k];
        d2[k] += (double)s2[k];
      }
    }
    if (l > 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        s_red[l - 1][0][g * 8 + k] = d1[k];
        s_red[l - 1][1][g * 8 + k] = d2[k];
      }
    }
  }
  __syncthreads();
  if (live && l == 0) {
    double* dst = stats + (long)(blockIdx.x % (unsigned)nrep) * 2 * ch + c0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      double a1 = d1[k], a2 = d2[k];
#pragma unroll
      for (int j = 0; j < POOL_LANES - 1; ++j) {
        a1 += s_red[j][0][g * 8 + k];
        a2 += s_red[j][1][g * 8 + k];
      }
      unsafeAtomicAdd(dst + k, a1);
      unsafeAtomicAdd(dst + ch + k, a2);
    }
  }
}

}  // namespace

extern "C" int pcaa_segment_weighted_mean(const void* a, int dtype, long lda, const float* weight, const int* u_off, int n,
                                          long M, int ch, int N, const float* scale, const float* shift, float* out,
                                          int* err_flag, void* stream) {
  PCAA_CHECK_ARG(a && weight && u_off && out, "pcaa_segment_weighted_mean: null pointer");
  PCAA_CHECK_ARG(dtype == PCAA_F32 || dtype == PCAA_BF16, "pcaa_segment_weighted_mean: bad dtype %d", dtype);
  PCAA_CHECK_ARG(n >= 1 && M >= 0 && N >= 1, "pcaa_segment_weighted_mean: needs n >= 1, M >= 0, N >= 1");
  PCAA_CHECK_ARG(ch >= 8 && ch % 8 == 0 && lda >= ch && lda % 8 == 0,
                 "pcaa_segment_weighted_mean: needs ch %% 8 == 0 and a leading dimension lda >= ch with lda %% 8 == 0 "
                 "(ch=%d lda=%ld)", ch, lda);
  PCAA_CHECK_ARG((scale != nullptr) == (shift != nullptr), "pcaa_segment_weighted_mean: scale and shift come together");
  PCAA_CHECK_ARG(((uintptr_t)a % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)weight % 4) == 0 &&
                     ((uintptr_t)u_off % 4) == 0 && ((uintptr_t)scale % 16) == 0 && ((uintptr_t)shift % 16) == 0,
                 "pcaa_segment_weighted_mean: a / out / scale / shift must be 16-B aligned, weight / u_off 4-B aligned");
  const dim3 grid((unsigned)n, (unsigned)cdiv(ch / 8, POOL_GROUPS));
  hipStream_t s = as_stream(stream);
#define LAUNCH_SP(T, AFF)                                                                                              \
  hipLaunchKernelGGL((segment_weighted_mean_kernel<T, AFF>), grid, dim3(POOL_THREADS), 0, s, (const T*)a, lda, weight,  \
                     u_off, M, ch, N, scale, shift, out, err_flag)
  if (dtype == PCAA_F32) { if (scale) LAUNCH_SP(float, true); else LAUNCH_SP(float, false); }
  else { if (scale) LAUNCH_SP(bf16_t, true); else LAUNCH_SP(bf16_t, false); }
#undef LAUNCH_SP
  PCAA_RETURN_LAUNCH_STATUS("pcaa_segment_weighted_mean");
}

extern "C" int pcaa_segment_weighted_mean_bwd(const float* dpool, const void* y, void* dy, int dtype, long lda,
                                              const float* weight, const int* u_off, int n, long M, int ch, int N,
                                              const float* scale, const float* shift, const float* mean,
                                              const float* rstd, double* stats, int nrep, int* err_flag, void* stream) {
  PCAA_CHECK_ARG(dpool && y && dy && weight && u_off && scale && shift && mean && rstd && stats,
                 "pcaa_segment_weighted_mean_bwd: null pointer");
  PCAA_CHECK_ARG(dtype == PCAA_F32 || dtype == PCAA_BF16, "pcaa_segment_weighted_mean_bwd: bad dtype %d", dtype);
  PCAA_CHECK_ARG(n >= 1 && M >= 0 && N >= 1 && nrep >= 1,
                 "pcaa_segment_weighted_mean_bwd: needs n >= 1, M >= 0, N >= 1, nrep >= 1");
  PCAA_CHECK_ARG(ch >= 8 && ch % 8 == 0 && lda >= ch && lda % 8 == 0,
                 "pcaa_segment_weighted_mean_bwd: needs ch %% 8 == 0 and a leading dimension lda >= ch with lda %% 8 == 0 "
                 "(ch=%d lda=%ld)", ch, lda);
  PCAA_CHECK_ARG(dy != y, "pcaa_segment_weighted_mean_bwd: dy may not alias y");
  PCAA_CHECK_ARG(((uintptr_t)dpool % 16) == 0 && ((uintptr_t)y % 16) == 0 && ((uintptr_t)dy % 16) == 0 &&
                     ((uintptr_t)scale % 16) == 0 && ((uintptr_t)shift % 16) == 0 && ((uintptr_t)mean % 16) == 0 &&
                     ((uintptr_t)rstd % 16) == 0 && ((uintptr_t)weight % 4) == 0 && ((uintptr_t)u_off % 4) == 0 &&
                     ((uintptr_t)stats % 8) == 0,
                 "pcaa_segment_weighted_mean_bwd: dpool / y / dy / scale / shift / mean / rstd must be 16-B aligned, "
                 "weight / u_off 4-B, stats 8-B aligned");
  hipStream_t s = as_stream(stream);
  const size_t es = dtype == PCAA_F32 ? 4 : 2;
  if (M > 0) {
    // rows no valid segment owns are zeros: they feed the weight-gradient product
    const hipError_t e = lda == ch ? hipMemsetAsync(dy, 0, (size_t)M * ch * es, s)
                                   : hipMemset2DAsync(dy, (size_t)lda * es, 0, (size_t)ch * es, (size_t)M, s);
    if (e != hipSuccess) {
      pcaa_set_error("pcaa_segment_weighted_mean_bwd: zero-fill failed: %s", hipGetErrorString(e));
      return PCAA_ERR_LAUNCH;
    }
  }
  const dim3 grid((unsigned)n, (unsigned)cdiv(ch / 8, POOL_GROUPS));
#define LAUNCH_SPB(T)                                                                                                  \
  hipLaunchKernelGGL((segment_weighted_mean_bwd_kernel<T>), grid, dim3(POOL_THREADS), 0, s, dpool, (const T*)y, lda,    \
                     weight, u_off, M, ch, N, scale, shift, mean, rstd, (T*)dy, stats, nrep, err_flag)
  if (dtype == PCAA_F32) LAUNCH_SPB(float); else LAUNCH_SPB(bf16_t);
#undef LAUNCH_SPB
  PCAA_RETURN_LAUNCH_STATUS("pcaa_segment_weighted_mean_bwd");
}
