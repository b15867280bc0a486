// Raw radar detections -> processed frames, on the device: what datasets.process_track does per frame on the host
// (reference datasets.py:79-161), one launch for all the frames of a tick.
//
// A radar frame is a ragged list of detections (x, y, z, doppler, linear power); the encoder wants N points per frame,
// centred (optionally divided by std + 1e-8) per frame and column.  pcaa_frames_from_raw takes the detections of n frames
// packed back to back (`points` [P, 5], `offsets` [n + 1]) and writes [n_out, N, C] fp32, rows n .. n_out - 1 zero.
// One workgroup of 256 threads per OUTPUT frame; everything a frame needs lives in its workgroup, so a frame's bits
// depend on its own detections, picks / key and nothing else (not on n, its position in the launch, or the grid):
//   1. picks -> LDS.  Supplied (`pick` [n, N], range-checked), or drawn here from a counter-based hash (below);
//   2. gather in fp64 -> LDS, point-major like the output; the power column becomes 10 log10(p + 1e-8) on the way;
//   3. per-column mean (and population std: second pass over (x - mean)^2, as numpy's std) in fp64 in a FIXED order:
//      thread t adds points t, t + 256, ... in sequence, a xor-butterfly over the wave's 64 lanes, then the four wave
//      partials in wave order -- every thread ends with the same bits;
//   4. (x - mean) [/ (std + 1e-8)] in fp64, rounded ONCE to fp32, stored with 16-byte vector stores where a frame is a
//      whole number of them (N * C % 4 == 0), 4-byte ones otherwise.
// A frame whose cardinality is < 1 or > PCAA_RAW_MAX_CARD, whose offsets leave [0, P], or with a supplied pick outside
// [0, card) is written as zeros (its pick_out row as -1) and *err_flag is set: no fault, no host check.
//
// Device-drawn picks.  h(seed, key, i) is a chain of the 32-bit mixer "lowbias32" (C. Wellons, hash-prospector:
//   x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16) over the words
//   seed_lo, seed_hi, key[0], key[1], i:  s = 0x9e3779b9;  for w in words: s = mix((s ^ w) + 0x9e3779b9);  h = s
// (32-bit wrap-around arithmetic; the added constant keeps 0 from being a fixed point).  Integer-exact, so
// datasets.device_picks_host restates it in numpy.
//   card <  N (the reference's repeat-pad): picks 0 .. card - 1 are the identity, pick card + d is
//              (uint64(h(seed, key, card + d)) * card) >> 32;
//   card >= N (its subsample without replacement): point i has the sort key (h(seed, key, i), i); its rank among the
//              frame's card keys is counted against the keys in LDS (all lanes read the same word: a broadcast); rank
//              r < N gives pick[r] = i: a uniform random N-subset in uniform random order, with no sequential shuffle.
#include "common.h"

namespace {

constexpr int RAW_THREADS = 256;
constexpr int RAW_WAVES = RAW_THREADS / 64;
constexpr int RAW_COLS = 5;                      // x, y, z, doppler, power

__host__ __device__ __forceinline__ uint32_t raw_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t raw_absorb(uint32_t s, uint32_t w) { return raw_mix((s ^ w) + 0x9e3779b9u); }

// the sum of v[c] over the workgroup, c < C, in the fixed order of the header comment; every thread gets the result
template <int C>
__device__ __forceinline__ void block_sum_cols(double (&v)[C], double* red /* [RAW_WAVES][RAW_COLS] */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = wave_sum_d(v[c]);
  __syncthreads();                                // the previous use of red is over
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) red[wave * RAW_COLS + c] = v[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < C; ++c) {
    double s = red[c];
#pragma unroll
    for (int w = 1; w < RAW_WAVES; ++w) s += red[w * RAW_COLS + c];
    v[c] = s;
  }
}

__device__ __forceinline__ void zero_frame(float* dst, int NC, bool vec) {
  if (vec) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int e = threadIdx.x * 4; e < NC; e += RAW_THREADS * 4) store4(dst + e, z);
  } else {
    for (int e = threadIdx.x; e < NC; e += RAW_THREADS) dst[e] = 0.f;
  }
}

template <typename T, int C>
__global__ __launch_bounds__(RAW_THREADS) void frames_from_raw_kernel(
    const T* __restrict__ points, long P, const int* __restrict__ offsets, int n, const int* __restrict__ pick,
    const int* __restrict__ frame_key, uint32_t seed_lo, uint32_t seed_hi, int N, int standardize, int divide_by_std,
    float* __restrict__ out, int* __restrict__ pick_out, int* __restrict__ err) {
#pragma clang fp contract(off)
  __shared__ double s_val[PCAA_RAW_MAX_POINTS * RAW_COLS];
  __shared__ int s_pick[PCAA_RAW_MAX_POINTS];
  __shared__ uint32_t s_key[PCAA_RAW_MAX_CARD];
  __shared__ double s_red[RAW_WAVES * RAW_COLS];
  __shared__ int s_bad;

  const int tid = threadIdx.x;
  const long f = blockIdx.x;
  const int NC = N * C;
  float* dst = out + f * (long)NC;
  const bool vec = (NC % 4 == 0) && ((uintptr_t)out % 16 == 0);
  if (f >= n) {                                   // whole-tile padding: rows n .. n_out - 1
    zero_frame(dst, NC, vec);
    return;
  }
  const long off0 = offsets[f], off1 = offsets[f + 1];
  const long card_l = off1 - off0;
  bool bad = off0 < 0 || off1 > P || card_l < 1 || card_l > PCAA_RAW_MAX_CARD;     // uniform over the workgroup
  const int card = bad ? 1 : (int)card_l;
  if (tid == 0) s_bad = 0;
  __syncthreads();

  if (!bad) {
    if (pick != nullptr) {
      bool mine = false;
      for (int p = tid; p < N; p += RAW_THREADS) {
        const int i = pick[f * N + p];
        mine |= i < 0 || i >= card;
        s_pick[p] = i;
      }
      if (mine) s_bad = 1;
    } else {
      uint32_t s = raw_absorb(raw_absorb(0x9e3779b9u, seed_lo), seed_hi);
      s = raw_absorb(raw_absorb(s, (uint32_t)frame_key[2 * f]), (uint32_t)frame_key[2 * f + 1]);
      if (card < N) {
        for (int p = tid; p < N; p += RAW_THREADS)
          s_pick[p] = p < card ? p : (int)(((uint64_t)raw_absorb(s, (uint32_t)p) * (uint64_t)card) >> 32);
      } else {
        for (int i = tid; i < card; i += RAW_THREADS) s_key[i] = raw_absorb(s, (uint32_t)i);
        __syncthreads();
        for (int i = tid; i < card; i += RAW_THREADS) {
          const uint32_t k = s_key[i];
          int rank = 0;
          for (int j = 0; j < card; ++j) {
            const uint32_t kj = s_key[j];
            rank += (kj < k) || (kj == k && j < i);
          }
          if (rank < N) s_pick[rank] = i;
        }
      }
    }
    __syncthreads();
    bad = s_bad != 0;
  }
  if (bad) {
    zero_frame(dst, NC, vec);
    if (pick_out != nullptr)
      for (int p = tid; p < N; p += RAW_THREADS) pick_out[f * N + p] = -1;
    if (err != nullptr && tid == 0) atomicOr(err, 1);
    return;
  }
  if (pick_out != nullptr)
    for (int p = tid; p < N; p += RAW_THREADS) pick_out[f * N + p] = s_pick[p];

  // gather, point-major; the power column to dB
  const T* src = points + off0 * RAW_COLS;
  for (int e = tid; e < NC; e += RAW_THREADS) {
    const int p = e / C, c = e - p * C;
    double v = (double)src[(long)s_pick[p] * RAW_COLS + c];
    if (C == RAW_COLS && c == RAW_COLS - 1) v = 10.0 * log10(v + 1e-8);
    s_val[e] = v;
  }
  __syncthreads();

  double mean[C], denom[C];
#pragma unroll
  for (int c = 0; c < C; ++c) { mean[c] = 0.0; denom[c] = 1.0; }
  if (standardize) {
    double acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    for (int p = tid; p < N; p += RAW_THREADS) {
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += s_val[p * C + c];
    }
    block_sum_cols<C>(acc, s_red);
#pragma unroll
    for (int c = 0; c < C; ++c) mean[c] = acc[c] / (double)N;
    if (divide_by_std) {
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = 0.0;
      for (int p = tid; p < N; p += RAW_THREADS) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const double d = s_val[p * C + c] - mean[c];
          acc[c] += d * d;
        }
      }
      block_sum_cols<C>(acc, s_red);
#pragma unroll
      for (int c = 0; c < C; ++c) denom[c] = sqrt(acc[c] / (double)N) + 1e-8;
    }
  }

  // centre, scale, round once, store
  auto finish = [&](int e) -> float {
    const int c = e % C;
    double m = mean[0], d = denom[0];
#pragma unroll
    for (int k = 1; k < C; ++k) {                 // a select chain: mean / denom stay in registers
      m = c == k ? mean[k] : m;
      d = c == k ? denom[k] : d;
    }
    double v = s_val[e] - m;
    if (divide_by_std) v = v / d;
    return (float)v;
  };
  if (vec) {
    for (int e = tid * 4; e < NC; e += RAW_THREADS * 4) {
      f32x4 o;
      o.x = finish(e); o.y = finish(e + 1); o.z = finish(e + 2); o.w = finish(e + 3);
      store4(dst + e, o);
    }
  } else {
    for (int e = tid; e < NC; e += RAW_THREADS) dst[e] = finish(e);
  }
}

template <typename T>
void launch_frames_from_raw(int C, dim3 grid, hipStream_t st, const T* points, long P, const int* offsets, int n,
                            const int* pick, const int* frame_key, long seed, int N, int standardize, int divide_by_std,
                            float* out, int* pick_out, int* err) {
  const uint32_t lo = (uint32_t)((uint64_t)seed & 0xffffffffu), hi = (uint32_t)((uint64_t)seed >> 32);
#define PCAA_RAW_CASE(CC)                                                                                              \
  case CC:                                                                                                             \
    hipLaunchKernelGGL((frames_from_raw_kernel<T, CC>), grid, dim3(RAW_THREADS), 0, st, points, P, offsets, n, pick,   \
                       frame_key, lo, hi, N, standardize, divide_by_std, out, pick_out, err);                          \
    break;
  switch (C) {
    PCAA_RAW_CASE(1) PCAA_RAW_CASE(2) PCAA_RAW_CASE(3) PCAA_RAW_CASE(4) PCAA_RAW_CASE(5)
  }
#undef PCAA_RAW_CASE
}

}  // namespace

extern "C" int pcaa_frames_from_raw(const void* points, int points_f64, long P, const int* offsets, int n, const int* pick,
                                    const int* frame_key, long seed, int N, int C, int standardize, int divide_by_std,
                                    float* out, int n_out, int* pick_out, int* err_flag, void* stream) {
  PCAA_CHECK_ARG(n >= 0 && n_out >= n && n_out >= 1 && P >= 0, "pcaa_frames_from_raw: needs 0 <= n <= n_out, n_out >= 1, P >= 0");
  PCAA_CHECK_ARG(N >= 1 && N <= PCAA_RAW_MAX_POINTS && C >= 1 && C <= RAW_COLS,
                 "pcaa_frames_from_raw: needs 1 <= N <= PCAA_RAW_MAX_POINTS and 1 <= C <= 5");
  PCAA_CHECK_ARG(out != nullptr && ((uintptr_t)out % 4) == 0, "pcaa_frames_from_raw: out is null or not 4-B aligned");
  PCAA_CHECK_ARG(n == 0 || (offsets != nullptr && (points != nullptr || P == 0)),
                 "pcaa_frames_from_raw: points / offsets are null");
  PCAA_CHECK_ARG(n == 0 || pick != nullptr || frame_key != nullptr,
                 "pcaa_frames_from_raw: without picks the frames need their keys (frame_key)");
  PCAA_CHECK_ARG(((uintptr_t)points % (points_f64 ? 8 : 4)) == 0, "pcaa_frames_from_raw: points are misaligned");
  const dim3 grid((unsigned)n_out);
  if (points_f64)
    launch_frames_from_raw<double>(C, grid, as_stream(stream), static_cast<const double*>(points), P, offsets, n, pick,
                                   frame_key, seed, N, standardize, divide_by_std, out, pick_out, err_flag);
  else
    launch_frames_from_raw<float>(C, grid, as_stream(stream), static_cast<const float*>(points), P, offsets, n, pick,
                                  frame_key, seed, N, standardize, divide_by_std, out, pick_out, err_flag);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_frames_from_raw");
}
