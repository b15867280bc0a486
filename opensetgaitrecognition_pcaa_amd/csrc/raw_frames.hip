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
// pcaa_crops_from_raw writes the same frames as training batches [B, T, N, C] from the tables of a whole store (below).
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
//
// Thinning (the _thin entry points): a first stage that keeps at most k_f of a frame's detections before the draw above
// pads or subsamples them to N -- what a sparser radar would deliver, and the reference's force_pc_subsampling sweep.
// Parameters keep (K >= 1; 0 = off: the instantiations without the stage), keep_min (1 <= Kmin <= K) and keep_rule
// (FIRST = 0, RANDOM = 1).  With s the chain state after seed_lo, seed_hi, key[0], key[1] and t = absorb(s, 0x6b656570)
// ("keep"; absorb(s, w) = mix((s ^ w) + 0x9e3779b9)):
//   count    k_f = Kmin + ((uint64)absorb(t, 0xffffffff) * (K - Kmin + 1) >> 32); the hash is drawn only when Kmin < K;
//   k_f >= card: the frame is untouched -- its picks and output bits are those of the entry points without thinning;
//   FIRST    the kept raw indices are 0 .. k_f - 1 (the support of the reference's quirk: datasets.process_track
//            overwrites the cardinality before it chooses);
//   RANDOM   the k_f detections with the smallest (absorb(t, i), i), in rank order, ranks counted against keys in LDS
//            exactly like the card >= N branch above (the key array is reused: it is dead before stage 2 writes it);
//   stage 2  the draw above, unchanged, over a virtual frame of k_f points (repeat-pad if k_f < N, a rank subset
//            otherwise), still on absorb(s, i) with i < 1024, which can never meet the tagged chain t; the result is
//            mapped through the keep list (16-bit, in LDS), so pick_out holds RAW indices.
// datasets.device_picks_host(..., keep, keep_min, keep_rule) restates it.  A supplied pick decides by itself: together
// with keep > 0 it is an argument error.
//
// Augmentation (the _aug entry points): a stage between steps 2 and 3 that moves the picked detections in fp64 in LDS,
// after the power column has become dB and before the frame is centred; steps 3 and 4 follow unchanged, so the compact-row
// route and the bit-equality of a frame across the three kernels hold as without it.  Parameters (RawAug; pcaa_hip.h):
// yaw, mirror, scale_lo / _hi, speed_lo / _hi, sigma[5].
//   per track   u = absorb(absorb(absorb(absorb(0x9e3779b9, seed_lo), seed_hi), key[0]), 0x6175676d) ("augm"; key[1] is
//               NOT absorbed: every frame of a track shares the draws, so overlapping windows agree and the gait dynamics
//               between frames survive);  w_j = absorb(u, j), r_j = (w_j + 0.5) 2^-32, j = 0 .. 3;
//               theta = yaw (2 r_0 - 1);  m = w_1 >> 31 (when mirror);  a = scale_lo + (scale_hi - scale_lo) r_2;
//               v = speed_lo + (speed_hi - speed_lo) r_3;
//   per detection, keyed by its RAW index i (every copy of a detection carries the same noise: padded duplicates stay
//               bit-equal rows):  n = absorb(s, 0x6e6f6973) ("nois"), q = absorb(n, i), r1 = (absorb(q, 2c) + 0.5) 2^-32,
//               r2 = (absorb(q, 2c + 1) + 0.5) 2^-32, g(i, c) = sqrt(-2 ln r1) cos(2 pi r2).  Both tags exceed 1024 and
//               differ from "keep": these chains never meet the pick draws;
//   per picked point, in order:  val[c] += sigma[c] g(i, c);  x, y, z *= a, doppler *= v;  x = -x when m;
//               (x, y) <- (x cos theta - y sin theta, x sin theta + y cos theta).  Neutral steps are skipped.
// Steps 1 - 3 of the list are element-wise and ride on the gather; the rotation is one pass over the points in place: no
// further LDS array.  A rotation about the radar's vertical axis and a mirror across boresight leave range and radial
// velocity alone; after centring they are what a person at another azimuth delivers -- hence before centring, and the
// Doppler untouched.  The stage is a template flag beside KEEP: the kernels without it are the code they were.
// datasets.frames_from_picks(..., augment=, seed=, keys=) restates it in numpy.
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

// the chain state of frame f after the words seed_lo, seed_hi, key[0], key[1]
__device__ __forceinline__ uint32_t raw_chain(uint32_t seed_lo, uint32_t seed_hi, const int* __restrict__ frame_key, long f) {
  const uint32_t s = raw_absorb(raw_absorb(0x9e3779b9u, seed_lo), seed_hi);
  return raw_absorb(raw_absorb(s, (uint32_t)frame_key[2 * f]), (uint32_t)frame_key[2 * f + 1]);
}

constexpr uint32_t RAW_KEEP_WORD = 0x6b656570u;  // "keep": the tag of the thinning stage's chain
constexpr int RAW_KEEP_FIRST = 0, RAW_KEEP_RANDOM = 1;
struct RawKeep {                                 // the thinning parameters: the kernels' last argument, read under KEEP only
  int keep, keep_min, rule;
};

// k_f of the header comment from t = absorb(s, RAW_KEEP_WORD): the one place it is computed (the frames' kernels and
// the scan of u_off must agree on it)
__device__ __forceinline__ int raw_keep_count(uint32_t t, int keep, int keep_min) {
  if (keep_min >= keep) return keep;
  return keep_min + (int)(((uint64_t)raw_absorb(t, 0xffffffffu) * (uint64_t)(keep - keep_min + 1)) >> 32);
}

// The augmentation stage's parameters (the _aug entry points; PCAA_RAW_AUG_* of pcaa_hip.h), by value behind the thinning
// ones: the kernels without the stage take RawKeep alone, as before it existed.
constexpr uint32_t RAW_AUG_WORD = 0x6175676du;   // "augm": the tag of a track's draws
constexpr uint32_t RAW_NOISE_WORD = 0x6e6f6973u; // "nois": the tag of a frame's noise chain
struct RawAug {
  double yaw, scale_lo, scale_hi, speed_lo, speed_hi, sigma[5];
  int mirror;
};
struct RawKeepAug : RawKeep {
  RawAug aug;
};
template <bool AUG>
using RawParams = typename std::conditional<AUG, RawKeepAug, RawKeep>::type;

// a hash word as a number in (0, 1): exact in fp64
__device__ __forceinline__ double raw_unit(uint32_t w) { return ((double)w + 0.5) * 0x1p-32; }

// what a track's frames share (the header comment's per-track draws), the same in every thread of every frame of it
struct RawAugDraw {
  double cos_t, sin_t, scale, speed;
  bool rotate, flip, do_scale, do_speed;
};
__device__ __forceinline__ RawAugDraw raw_aug_draw(const RawAug& ag, uint32_t seed_lo, uint32_t seed_hi, uint32_t key0) {
#pragma clang fp contract(off)
  const uint32_t u =
      raw_absorb(raw_absorb(raw_absorb(raw_absorb(0x9e3779b9u, seed_lo), seed_hi), key0), RAW_AUG_WORD);
  RawAugDraw d;
  d.rotate = ag.yaw != 0.0;
  d.cos_t = 1.0;
  d.sin_t = 0.0;
  if (d.rotate) {
    const double theta = ag.yaw * (2.0 * raw_unit(raw_absorb(u, 0u)) - 1.0);
    d.cos_t = cos(theta);
    d.sin_t = sin(theta);
  }
  d.flip = ag.mirror != 0 && (raw_absorb(u, 1u) >> 31) != 0;
  d.do_scale = !(ag.scale_lo == 1.0 && ag.scale_hi == 1.0);
  d.scale = d.do_scale ? ag.scale_lo + (ag.scale_hi - ag.scale_lo) * raw_unit(raw_absorb(u, 2u)) : 1.0;
  d.do_speed = !(ag.speed_lo == 1.0 && ag.speed_hi == 1.0);
  d.speed = d.do_speed ? ag.speed_lo + (ag.speed_hi - ag.speed_lo) * raw_unit(raw_absorb(u, 3u)) : 1.0;
  return d;
}

// steps 1 - 3 of the stage for column c of the detection whose noise chain is q = absorb(n, raw index): noise, scale /
// speed, mirror; a neutral step is skipped
template <int C>
__device__ __forceinline__ double raw_aug_element(double v, int c, uint32_t q, const RawAug& ag, const RawAugDraw& d) {
#pragma clang fp contract(off)
  double sg = 0.0;
#pragma unroll
  for (int k = 0; k < C; ++k) sg = c == k ? ag.sigma[k] : sg;   // a select chain: no indexed copy of the parameters
  if (sg != 0.0) {
    const double r1 = raw_unit(raw_absorb(q, 2u * (uint32_t)c)), r2 = raw_unit(raw_absorb(q, 2u * (uint32_t)c + 1u));
    v += sg * (sqrt(-2.0 * log(r1)) * cos(6.283185307179586 * r2));
  }
  if (c < 3) {
    if (d.do_scale) v *= d.scale;
  } else if (c == 3) {
    if (d.do_speed) v *= d.speed;
  }
  if (c == 0 && d.flip) v = -v;
  return v;
}

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

// a frame's offsets are unusable: the first half of the bad-frame rule (the second: a supplied pick outside [0, card))
__host__ __device__ __forceinline__ bool raw_offsets_bad(long off0, long off1, long P) {
  const long card = off1 - off0;
  return off0 < 0 || off1 > P || card < 1 || card > PCAA_RAW_MAX_CARD;
}

// the LDS of one frame's workgroup
struct RawShared {
  double val[PCAA_RAW_MAX_POINTS * RAW_COLS];     // the gathered points, point-major like the output
  int pick[PCAA_RAW_MAX_POINTS];
  uint32_t key[PCAA_RAW_MAX_CARD];
  double red[RAW_WAVES * RAW_COLS];
  int bad;
};
// ... with the thinning stage: the kept raw indices by rank (a frame holds at most 1024: 16 bits each)
struct RawSharedKeep : RawShared {
  uint16_t keep[PCAA_RAW_MAX_CARD];
};
template <bool KEEP>
using RawSharedOf = typename std::conditional<KEEP, RawSharedKeep, RawShared>::type;

// Steps 1 - 3 of the header comment for frame f, shared by every kernel of this file so that they produce the same
// bits: picks -> sh.pick (and pick_out), gather -> sh.val, mean / denom in every thread's registers.  Returns false
// for a bad frame: pick_out is -1, *err set, sh.val / mean / denom undefined; the caller writes its zeros.
// KEEP: with the thinning stage of the header comment (kp is read only then).  AUG: with the augmentation stage between
// the gather and the statistics (kp.aug); those kernels are instantiated with KEEP and take kp.keep == 0 as "no thinning".
template <typename T, int C, bool KEEP, bool AUG>
__device__ __forceinline__ bool raw_frame_prepare(
    RawSharedOf<KEEP>& sh, const T* __restrict__ points, long P, const int* __restrict__ offsets, long f,
    const int* __restrict__ pick, const int* __restrict__ frame_key, uint32_t seed_lo, uint32_t seed_hi, int N,
    int standardize, int divide_by_std, const RawParams<AUG>& kp, int* __restrict__ pick_out, int* __restrict__ err,
    int& card_out, double (&mean)[C], double (&denom)[C]) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const int NC = N * C;
  const long off0 = offsets[f], off1 = offsets[f + 1];
  bool bad = raw_offsets_bad(off0, off1, P);      // uniform over the workgroup
  const int card = bad ? 1 : (int)(off1 - off0);
  card_out = card;
  if (tid == 0) sh.bad = 0;
  __syncthreads();

  if (!bad) {
    if (pick != nullptr) {
      bool mine = false;
      for (int p = tid; p < N; p += RAW_THREADS) {
        const int i = pick[f * N + p];
        mine |= i < 0 || i >= card;
        sh.pick[p] = i;
      }
      if (mine) sh.bad = 1;
    } else {
      const uint32_t s = raw_chain(seed_lo, seed_hi, frame_key, f);
      int vcard = card;                             // the frame stage 2 draws over
      bool mapped = false;
      if constexpr (KEEP) {
        // stage 1: k_f, and under RANDOM the keep list (everything here is uniform over the workgroup); the _aug
        // kernels take keep == 0 as k_f = card: the frame is untouched
        const uint32_t t = raw_absorb(s, RAW_KEEP_WORD);
        const int kf = (AUG && kp.keep == 0) ? card : raw_keep_count(t, kp.keep, kp.keep_min);
        vcard = kf < card ? kf : card;
        mapped = kf < card && kp.rule == RAW_KEEP_RANDOM;
        if (mapped) {
          for (int i = tid; i < card; i += RAW_THREADS) sh.key[i] = raw_absorb(t, (uint32_t)i);
          __syncthreads();
          for (int i = tid; i < card; i += RAW_THREADS) {
            const uint32_t k = sh.key[i];
            int rank = 0;
            for (int j = 0; j < card; ++j) {
              const uint32_t kj = sh.key[j];
              rank += (kj < k) || (kj == k && j < i);
            }
            if (rank < vcard) sh.keep[rank] = (uint16_t)i;   // the ranks are a permutation: every slot < k_f is written
          }
          __syncthreads();                          // the list is complete, and sh.key is free for stage 2
        }
      }
      if (vcard < N) {
        for (int p = tid; p < N; p += RAW_THREADS)
          sh.pick[p] = p < vcard ? p : (int)(((uint64_t)raw_absorb(s, (uint32_t)p) * (uint64_t)vcard) >> 32);
      } else {
        for (int i = tid; i < vcard; i += RAW_THREADS) sh.key[i] = raw_absorb(s, (uint32_t)i);
        __syncthreads();
        for (int i = tid; i < vcard; i += RAW_THREADS) {
          const uint32_t k = sh.key[i];
          int rank = 0;
          for (int j = 0; j < vcard; ++j) {
            const uint32_t kj = sh.key[j];
            rank += (kj < k) || (kj == k && j < i);
          }
          if (rank < N) sh.pick[rank] = i;
        }
      }
      if constexpr (KEEP) {
        if (mapped) {                               // virtual -> raw indices (FIRST: the list is the identity)
          __syncthreads();
          for (int p = tid; p < N; p += RAW_THREADS) sh.pick[p] = (int)sh.keep[sh.pick[p]];
        }
      }
    }
    __syncthreads();
    bad = sh.bad != 0;
  }
  if (bad) {
    if (pick_out != nullptr)
      for (int p = tid; p < N; p += RAW_THREADS) pick_out[f * N + p] = -1;
    if (err != nullptr && tid == 0) atomicOr(err, 1);
    return false;
  }
  if (pick_out != nullptr)
    for (int p = tid; p < N; p += RAW_THREADS) pick_out[f * N + p] = sh.pick[p];

  // gather, point-major; the power column to dB
  const T* src = points + off0 * RAW_COLS;
  if constexpr (AUG) {
    // the stage's element-wise steps ride on the gather, keyed by the RAW index: every copy of a detection gets the same
    // noise; then the rotation, point by point, in place
    const RawAugDraw d = raw_aug_draw(kp.aug, seed_lo, seed_hi, (uint32_t)frame_key[2 * f]);
    const uint32_t nz = raw_absorb(raw_chain(seed_lo, seed_hi, frame_key, f), RAW_NOISE_WORD);
    for (int e = tid; e < NC; e += RAW_THREADS) {
      const int p = e / C, c = e - p * C, i = sh.pick[p];
      double v = (double)src[(long)i * RAW_COLS + c];
      if (C == RAW_COLS && c == RAW_COLS - 1) v = 10.0 * log10(v + 1e-8);
      sh.val[e] = raw_aug_element<C>(v, c, raw_absorb(nz, (uint32_t)i), kp.aug, d);
    }
    __syncthreads();
    if constexpr (C >= 2) {
      if (d.rotate) {                               // uniform over the workgroup
        for (int p = tid; p < N; p += RAW_THREADS) {
          const double x = sh.val[p * C], y = sh.val[p * C + 1];
          sh.val[p * C] = x * d.cos_t - y * d.sin_t;
          sh.val[p * C + 1] = x * d.sin_t + y * d.cos_t;
        }
        __syncthreads();
      }
    }
  } else {
    for (int e = tid; e < NC; e += RAW_THREADS) {
      const int p = e / C, c = e - p * C;
      double v = (double)src[(long)sh.pick[p] * RAW_COLS + c];
      if (C == RAW_COLS && c == RAW_COLS - 1) v = 10.0 * log10(v + 1e-8);
      sh.val[e] = v;
    }
    __syncthreads();
  }

#pragma unroll
  for (int c = 0; c < C; ++c) { mean[c] = 0.0; denom[c] = 1.0; }
  if (standardize) {
    double acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    for (int p = tid; p < N; p += RAW_THREADS) {
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += sh.val[p * C + c];
    }
    block_sum_cols<C>(acc, sh.red);
#pragma unroll
    for (int c = 0; c < C; ++c) mean[c] = acc[c] / (double)N;
    if (divide_by_std) {
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = 0.0;
      for (int p = tid; p < N; p += RAW_THREADS) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const double d = sh.val[p * C + c] - mean[c];
          acc[c] += d * d;
        }
      }
      block_sum_cols<C>(acc, sh.red);
#pragma unroll
      for (int c = 0; c < C; ++c) denom[c] = sqrt(acc[c] / (double)N) + 1e-8;
    }
  }
  return true;
}

// step 4 for element e = p * C + c of the frame: centre, scale, round once
template <int C>
__device__ __forceinline__ float raw_frame_finish(const RawShared& sh, int e, const double (&mean)[C],
                                                  const double (&denom)[C], int divide_by_std) {
#pragma clang fp contract(off)
  const int c = e % C;
  double m = mean[0], d = denom[0];
#pragma unroll
  for (int k = 1; k < C; ++k) {                   // a select chain: mean / denom stay in registers
    m = c == k ? mean[k] : m;
    d = c == k ? denom[k] : d;
  }
  double v = sh.val[e] - m;
  if (divide_by_std) v = v / d;
  return (float)v;
}

// Steps 1 - 4 for store frame f into the padded frame at dst ([N, C] fp32): the one body of the kernels that write padded
// frames (frames_from_raw_kernel, crops_from_raw_kernel), so that a frame has the same bits wherever it is written.
template <typename T, int C, bool KEEP, bool AUG>
__device__ __forceinline__ void raw_frame_write(
    RawSharedOf<KEEP>& sh, const T* __restrict__ points, long P, const int* __restrict__ offsets, long f,
    const int* __restrict__ pick, const int* __restrict__ frame_key, uint32_t seed_lo, uint32_t seed_hi, int N,
    int standardize, int divide_by_std, const RawParams<AUG>& kp, float* __restrict__ dst, bool vec,
    int* __restrict__ pick_out, int* __restrict__ err) {
  const int tid = threadIdx.x;
  const int NC = N * C;
  double mean[C], denom[C];
  int card;
  if (!raw_frame_prepare<T, C, KEEP, AUG>(sh, points, P, offsets, f, pick, frame_key, seed_lo, seed_hi, N, standardize,
                                          divide_by_std, kp, pick_out, err, card, mean, denom)) {
    zero_frame(dst, NC, vec);
    return;
  }
  if (vec) {
    for (int e = tid * 4; e < NC; e += RAW_THREADS * 4) {
      f32x4 o;
      o.x = raw_frame_finish<C>(sh, e, mean, denom, divide_by_std);
      o.y = raw_frame_finish<C>(sh, e + 1, mean, denom, divide_by_std);
      o.z = raw_frame_finish<C>(sh, e + 2, mean, denom, divide_by_std);
      o.w = raw_frame_finish<C>(sh, e + 3, mean, denom, divide_by_std);
      store4(dst + e, o);
    }
  } else {
    for (int e = tid; e < NC; e += RAW_THREADS) dst[e] = raw_frame_finish<C>(sh, e, mean, denom, divide_by_std);
  }
}

template <typename T, int C, bool KEEP, bool AUG>
__global__ __launch_bounds__(RAW_THREADS) void frames_from_raw_kernel(
    const T* __restrict__ points, long P, const int* __restrict__ offsets, int n, const int* __restrict__ pick,
    const int* __restrict__ frame_key, uint32_t seed_lo, uint32_t seed_hi, int N, int standardize, int divide_by_std,
    float* __restrict__ out, int* __restrict__ pick_out, int* __restrict__ err, RawParams<AUG> kp) {
  __shared__ RawSharedOf<KEEP> sh;
  const long f = blockIdx.x;
  const int NC = N * C;
  float* dst = out + f * (long)NC;
  const bool vec = (NC % 4 == 0) && ((uintptr_t)out % 16 == 0);
  if (f >= n) {                                   // whole-tile padding: rows n .. n_out - 1
    zero_frame(dst, NC, vec);
    return;
  }
  raw_frame_write<T, C, KEEP, AUG>(sh, points, P, offsets, f, pick, frame_key, seed_lo, seed_hi, N, standardize,
                                   divide_by_std, kp, dst, vec, pick_out, err);
}

// ---------------------------------------------------------------------------------------------------------------------
// A training batch straight from the detections of a whole split (pcaa_crops_from_raw): `points` / `offsets` / `pick` /
// `frame_key` are the tables of ALL F frames of the store, crop b is store frames start[b] .. start[b] + T - 1, out is
// [B, T, N, C].  Workgroup b * T + t writes frame (b, t) through raw_frame_write: the frame that pcaa_frames_from_raw
// writes for store frame start[b] + t, bit for bit, wherever it stands in the batch and however often it is asked for
// (overlapping and repeated crops each get their own copy: no workgroup reads what another wrote).  A crop that leaves
// the store (start[b] < 0 or start[b] + T > F; compared in 64 bits) is zeros and sets *err before any table is read.
// The flag is raised as everywhere in this file (atomicOr); the output has no atomics.
template <typename T, int C, bool KEEP, bool AUG>
__global__ __launch_bounds__(RAW_THREADS) void crops_from_raw_kernel(
    const T* __restrict__ points, long P, const int* __restrict__ offsets, long F, const int* __restrict__ start, int Tc,
    const int* __restrict__ pick, const int* __restrict__ frame_key, uint32_t seed_lo, uint32_t seed_hi, int N,
    int standardize, int divide_by_std, float* __restrict__ out, int* __restrict__ err, RawParams<AUG> kp) {
  __shared__ RawSharedOf<KEEP> sh;
  const int NC = N * C;
  const long slot = blockIdx.x;                   // b * T + t < B * T: the grid is exactly the batch's frames
  const int b = (int)(slot / Tc), t = (int)(slot - (long)b * Tc);
  float* dst = out + slot * (long)NC;
  const bool vec = (NC % 4 == 0) && ((uintptr_t)out % 16 == 0);
  const long s = start[b];                        // uniform over the workgroup
  if (s < 0 || s + (long)Tc > F) {
    zero_frame(dst, NC, vec);
    if (err != nullptr && threadIdx.x == 0) atomicOr(err, 1);
    return;
  }
  raw_frame_write<T, C, KEEP, AUG>(sh, points, P, offsets, s + t, pick, frame_key, seed_lo, seed_hi, N, standardize,
                                   divide_by_std, kp, dst, vec, nullptr, err);
}

// ---------------------------------------------------------------------------------------------------------------------
// The same frames without their padding (pcaa_frames_from_raw_unique): a padded frame repeats detections, and in eval mode
// the per-point network is a pure function of the point, so mean over the N rows of f(row) = (1/N) sum_i m_i f(p_i) over
// the DISTINCT picked detections p_i with multiplicities m_i.  Frame f owns u_cnt[f] = min(card, N) rows of a compact
// [M, C] table from u_off[f] on (a frame whose offsets are bad: one row); thinned, min(card, k_f, N).  u_off depends on the
// offsets alone, with thinning also on keep, and under a count range (keep_min < keep) on the seed and the frames' keys.

// u_off[0 .. n] = exclusive scan of u_cnt: one workgroup walks the frames in chunks of its size with a running carry
constexpr int SCAN_THREADS = 1024;
template <bool KEEP>
__global__ __launch_bounds__(SCAN_THREADS) void raw_unique_offsets_kernel(
    const int* __restrict__ offsets, int n, long P, int N, int* __restrict__ u_off, const int* __restrict__ frame_key,
    uint32_t seed_lo, uint32_t seed_hi, RawKeep kp) {
  __shared__ int s_wave[SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;                                  // the same in every thread
  if (tid == 0) u_off[0] = 0;
  for (int base = 0; base < n; base += SCAN_THREADS) {
    const int f = base + tid;
    int cnt = 0;
    if (f < n) {
      const long off0 = offsets[f], off1 = offsets[f + 1];
      cnt = raw_offsets_bad(off0, off1, P) ? 1 : (int)((off1 - off0) < (long)N ? (off1 - off0) : (long)N);
      if constexpr (KEEP) {                       // k_f as raw_frame_prepare computes it; the keys are read for a range only
        const int kf = kp.keep_min >= kp.keep
                           ? kp.keep
                           : raw_keep_count(raw_absorb(raw_chain(seed_lo, seed_hi, frame_key, f), RAW_KEEP_WORD), kp.keep,
                                            kp.keep_min);
        cnt = cnt < kf ? cnt : kf;                // a bad frame's one row stays: k_f >= 1
      }
    }
    int incl = cnt;                               // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    __syncthreads();                              // the previous chunk's reads of s_wave are over
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SCAN_THREADS / 64; ++w) {
      const int t = s_wave[w];
      before += w < wave ? t : 0;
      total += t;
    }
    if (f < n) u_off[f + 1] = carry + before + incl;
    carry += total;
  }
}

constexpr int RAW_PER_THREAD = PCAA_RAW_MAX_POINTS / RAW_THREADS;      // pick positions one thread ranks

template <typename T, int C, bool KEEP, bool AUG>
__global__ __launch_bounds__(RAW_THREADS) void frames_from_raw_unique_kernel(
    const T* __restrict__ points, long P, const int* __restrict__ offsets, int n, const int* __restrict__ pick,
    const int* __restrict__ frame_key, uint32_t seed_lo, uint32_t seed_hi, int N, int standardize, int divide_by_std,
    float* __restrict__ rows, float* __restrict__ weight, const int* __restrict__ u_off, long M,
    int* __restrict__ pick_out, int* __restrict__ err, RawParams<AUG> kp) {
  __shared__ RawSharedOf<KEEP> sh;
  __shared__ int s_cnt[PCAA_RAW_MAX_CARD];        // by raw index: how often it was picked
  __shared__ int s_first[PCAA_RAW_MAX_CARD];      // by raw index: the first pick position that holds it
  __shared__ int s_rank[PCAA_RAW_MAX_POINTS];     // by pick position: distinct detections first seen before it
  __shared__ int s_wave[RAW_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool vec = (C == 4) && ((uintptr_t)rows % 16 == 0);

  auto zero_rows = [&](long r0, long r1) {        // rows r0 .. r1 - 1: the zero point, weight 0
    for (long r = r0 + tid; r < r1; r += RAW_THREADS) weight[r] = 0.f;
    for (long e = r0 * C + tid; e < r1 * C; e += RAW_THREADS) rows[e] = 0.f;
  };

  if ((long)blockIdx.x >= (long)n) {              // the rows no frame owns: u_off[n] .. M - 1, shared by the tail blocks
    long r0 = u_off[n];
    r0 = r0 < 0 ? 0 : (r0 > M ? M : r0);
    const long nb = (long)gridDim.x - n, b = (long)blockIdx.x - n;
    const long per = (M - r0 + nb - 1) / nb;
    const long a = r0 + b * per, z = a + per < M ? a + per : M;
    if (a < z) zero_rows(a, z);
    return;
  }
  const long f = blockIdx.x;
  const long u0 = u_off[f], u1 = u_off[f + 1];
  if (u0 < 0 || u1 <= u0 || u1 > M) {             // the table is too small for this frame (inconsistent offsets)
    if (err != nullptr && tid == 0) atomicOr(err, 1);
    return;
  }
  double mean[C], denom[C];
  int card;
  if (!raw_frame_prepare<T, C, KEEP, AUG>(sh, points, P, offsets, f, pick, frame_key, seed_lo, seed_hi, N, standardize,
                                          divide_by_std, kp, pick_out, err, card, mean, denom)) {
    zero_rows(u0, u1);                            // one row, the zero point N times: the padded path's all-zero frame
    __syncthreads();                              // (the weight below is written after the zeros, by the thread that wrote them)
    if (tid == 0) weight[u0] = (float)N;
    return;
  }

  // multiplicities and first occurrences: integer LDS atomics, so the result does not depend on their order
  for (int i = tid; i < card; i += RAW_THREADS) { s_cnt[i] = 0; s_first[i] = N; }
  __syncthreads();
  for (int p = tid; p < N; p += RAW_THREADS) {
    const int i = sh.pick[p];
    atomicAdd(&s_cnt[i], 1);
    atomicMin(&s_first[i], p);
  }
  __syncthreads();
  // rank of every first occurrence: thread t owns positions t * RAW_PER_THREAD .. + RAW_PER_THREAD - 1
  int mine = 0;
#pragma unroll
  for (int k = 0; k < RAW_PER_THREAD; ++k) {
    const int p = tid * RAW_PER_THREAD + k;
    mine += (p < N && s_first[sh.pick[p]] == p) ? 1 : 0;
  }
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int before = incl - mine, distinct = 0;
#pragma unroll
  for (int w = 0; w < RAW_WAVES; ++w) {
    const int t = s_wave[w];
    before += w < wave ? t : 0;
    distinct += t;
  }
#pragma unroll
  for (int k = 0; k < RAW_PER_THREAD; ++k) {
    const int p = tid * RAW_PER_THREAD + k;
    if (p < N) {
      const bool first = s_first[sh.pick[p]] == p;
      s_rank[p] = first ? before : -1;
      before += first ? 1 : 0;
    }
  }
  __syncthreads();

  // distinct <= min(card, k_f, N) = u1 - u0: the rows the picks leave unused are zero with weight 0
  if (vec) {
    for (int p = tid; p < N; p += RAW_THREADS) {
      const int r = s_rank[p];
      if (r < 0) continue;
      f32x4 o;
      o.x = raw_frame_finish<C>(sh, p * C, mean, denom, divide_by_std);
      o.y = raw_frame_finish<C>(sh, p * C + 1, mean, denom, divide_by_std);
      o.z = raw_frame_finish<C>(sh, p * C + 2, mean, denom, divide_by_std);
      o.w = raw_frame_finish<C>(sh, p * C + 3, mean, denom, divide_by_std);
      store4(rows + (u0 + r) * C, o);
    }
  } else {
    for (int e = tid; e < N * C; e += RAW_THREADS) {
      const int p = e / C, r = s_rank[p];
      if (r >= 0) rows[(u0 + r) * C + (e - p * C)] = raw_frame_finish<C>(sh, e, mean, denom, divide_by_std);
    }
  }
  for (int p = tid; p < N; p += RAW_THREADS) {
    const int r = s_rank[p];
    if (r >= 0) weight[u0 + r] = (float)s_cnt[sh.pick[p]];
  }
  zero_rows(u0 + distinct, u1);
}

// every launcher: KEEP = kp.keep > 0 picks the instantiation; without thinning the kernels are those of ABI 29.  KP is
// RawKeep, or RawKeepAug for the kernels with the augmentation stage (one instantiation per C: KEEP, keep == 0 allowed).
#define PCAA_RAW_CASE(LAUNCH, CC)                                                                                      \
  case CC:                                                                                                             \
    if constexpr (AUG) { LAUNCH(CC, true) } else if (kp.keep > 0) { LAUNCH(CC, true) } else { LAUNCH(CC, false) }      \
    break;
#define PCAA_RAW_CASES(LAUNCH)                                                                                         \
  constexpr bool AUG = std::is_same<KP, RawKeepAug>::value;                                                            \
  switch (C) {                                                                                                         \
    PCAA_RAW_CASE(LAUNCH, 1) PCAA_RAW_CASE(LAUNCH, 2) PCAA_RAW_CASE(LAUNCH, 3) PCAA_RAW_CASE(LAUNCH, 4)                \
    PCAA_RAW_CASE(LAUNCH, 5)                                                                                           \
  }

template <typename T, typename KP>
void launch_frames_from_raw(int C, dim3 grid, hipStream_t st, const T* points, long P, const int* offsets, int n,
                            const int* pick, const int* frame_key, long seed, int N, int standardize, int divide_by_std,
                            KP kp, float* out, int* pick_out, int* err) {
  const uint32_t lo = (uint32_t)((uint64_t)seed & 0xffffffffu), hi = (uint32_t)((uint64_t)seed >> 32);
#define PCAA_RAW_LAUNCH(CC, KEEP)                                                                                      \
  hipLaunchKernelGGL((frames_from_raw_kernel<T, CC, KEEP, AUG>), grid, dim3(RAW_THREADS), 0, st, points, P, offsets,   \
                     n, pick, frame_key, lo, hi, N, standardize, divide_by_std, out, pick_out, err, kp);
  PCAA_RAW_CASES(PCAA_RAW_LAUNCH)
#undef PCAA_RAW_LAUNCH
}

template <typename T, typename KP>
void launch_crops_from_raw(int C, dim3 grid, hipStream_t st, const T* points, long P, const int* offsets, long F,
                           const int* start, int Tc, const int* pick, const int* frame_key, long seed, int N,
                           int standardize, int divide_by_std, KP kp, float* out, int* err) {
  const uint32_t lo = (uint32_t)((uint64_t)seed & 0xffffffffu), hi = (uint32_t)((uint64_t)seed >> 32);
#define PCAA_RAW_LAUNCH(CC, KEEP)                                                                                      \
  hipLaunchKernelGGL((crops_from_raw_kernel<T, CC, KEEP, AUG>), grid, dim3(RAW_THREADS), 0, st, points, P, offsets, F, \
                     start, Tc, pick, frame_key, lo, hi, N, standardize, divide_by_std, out, err, kp);
  PCAA_RAW_CASES(PCAA_RAW_LAUNCH)
#undef PCAA_RAW_LAUNCH
}

template <typename T, typename KP>
void launch_frames_from_raw_unique(int C, dim3 grid, hipStream_t st, const T* points, long P, const int* offsets, int n,
                                   const int* pick, const int* frame_key, long seed, int N, int standardize,
                                   int divide_by_std, KP kp, float* rows, float* weight, const int* u_off, long M,
                                   int* pick_out, int* err) {
  const uint32_t lo = (uint32_t)((uint64_t)seed & 0xffffffffu), hi = (uint32_t)((uint64_t)seed >> 32);
#define PCAA_RAW_LAUNCH(CC, KEEP)                                                                                      \
  hipLaunchKernelGGL((frames_from_raw_unique_kernel<T, CC, KEEP, AUG>), grid, dim3(RAW_THREADS), 0, st, points, P,    \
                     offsets, n, pick, frame_key, lo, hi, N, standardize, divide_by_std, rows, weight, u_off, M,       \
                     pick_out, err, kp);
  PCAA_RAW_CASES(PCAA_RAW_LAUNCH)
#undef PCAA_RAW_LAUNCH
}
#undef PCAA_RAW_CASES
#undef PCAA_RAW_CASE

// what the _thin entry points check on top of their neighbours' arguments: no launch follows a refusal
int check_keep(const char* who, int keep, int keep_min, int keep_rule, const void* pick, const void* frame_key, long n) {
  PCAA_CHECK_ARG(keep >= 1 && keep_min >= 1 && keep_min <= keep && keep <= PCAA_RAW_MAX_CARD,
                 "%s: needs 1 <= keep_min <= keep <= PCAA_RAW_MAX_CARD", who);
  PCAA_CHECK_ARG(keep_rule == RAW_KEEP_FIRST || keep_rule == RAW_KEEP_RANDOM, "%s: keep_rule is 0 (first) or 1 (random)", who);
  PCAA_CHECK_ARG(pick == nullptr, "%s: supplied picks decide by themselves; pick must be NULL", who);
  PCAA_CHECK_ARG(n == 0 || frame_key != nullptr, "%s: the frames need their keys (frame_key)", who);
  return PCAA_OK;
}

// what the _aug entry points check on top of their neighbours' arguments (thinning is optional there, picks allowed
// without it), and the parameters as the kernels take them: no launch follows a refusal
int check_aug(const char* who, const double* aug, int C, int keep, int keep_min, int keep_rule, const void* pick,
              const void* frame_key, long n, RawKeepAug& kp) {
  PCAA_CHECK_ARG(aug != nullptr, "%s: aug is null (PCAA_RAW_AUG_PARAMS doubles)", who);
  PCAA_CHECK_ARG(n == 0 || frame_key != nullptr, "%s: the frames need their keys (frame_key), with supplied picks too", who);
  if (keep != 0) {
    if (int rc = check_keep(who, keep, keep_min, keep_rule, pick, frame_key, n)) return rc;
  } else {
    keep_min = keep_rule = 0;
  }
  const double yaw = aug[PCAA_RAW_AUG_YAW], s0 = aug[PCAA_RAW_AUG_SCALE_LO], s1 = aug[PCAA_RAW_AUG_SCALE_HI];
  const double v0 = aug[PCAA_RAW_AUG_SPEED_LO], v1 = aug[PCAA_RAW_AUG_SPEED_HI];
  PCAA_CHECK_ARG(yaw >= 0.0 && yaw <= 3.14159265358979323846, "%s: yaw must lie in [0, pi]", who);   // a NaN fails too
  PCAA_CHECK_ARG(yaw == 0.0 || C >= 2, "%s: a rotation needs the x and y columns (C >= 2)", who);
  PCAA_CHECK_ARG(std::isfinite(aug[PCAA_RAW_AUG_MIRROR]), "%s: mirror is 0 or 1", who);
  PCAA_CHECK_ARG(s0 > 0.0 && s0 <= s1 && std::isfinite(s1), "%s: needs 0 < scale_lo <= scale_hi, finite", who);
  PCAA_CHECK_ARG(v0 > 0.0 && v0 <= v1 && std::isfinite(v1), "%s: needs 0 < speed_lo <= speed_hi, finite", who);
  kp.keep = keep, kp.keep_min = keep_min, kp.rule = keep_rule;
  kp.aug.yaw = yaw, kp.aug.scale_lo = s0, kp.aug.scale_hi = s1, kp.aug.speed_lo = v0, kp.aug.speed_hi = v1;
  kp.aug.mirror = aug[PCAA_RAW_AUG_MIRROR] != 0.0;
  for (int c = 0; c < RAW_COLS; ++c) {
    const double sg = aug[PCAA_RAW_AUG_SIGMA + c];
    PCAA_CHECK_ARG(sg >= 0.0 && std::isfinite(sg), "%s: a sigma is negative or not finite", who);
    kp.aug.sigma[c] = sg;
  }
  return PCAA_OK;
}

// The bodies of the entry points, `who` the name in their messages; kp.keep == 0: without thinning.  KP = RawKeepAug:
// with the augmentation stage.
template <typename KP>
int frames_from_raw_impl(const char* who, const void* points, int points_f64, long P, const int* offsets, int n,
                         const int* pick, const int* frame_key, long seed, int N, int C, int standardize,
                         int divide_by_std, KP kp, float* out, int n_out, int* pick_out, int* err_flag, void* stream) {
  PCAA_CHECK_ARG(n >= 0 && n_out >= n && n_out >= 1 && P >= 0, "%s: needs 0 <= n <= n_out, n_out >= 1, P >= 0", who);
  PCAA_CHECK_ARG(N >= 1 && N <= PCAA_RAW_MAX_POINTS && C >= 1 && C <= RAW_COLS,
                 "%s: needs 1 <= N <= PCAA_RAW_MAX_POINTS and 1 <= C <= 5", who);
  PCAA_CHECK_ARG(out != nullptr && ((uintptr_t)out % 4) == 0, "%s: out is null or not 4-B aligned", who);
  PCAA_CHECK_ARG(n == 0 || (offsets != nullptr && (points != nullptr || P == 0)), "%s: points / offsets are null", who);
  PCAA_CHECK_ARG(n == 0 || pick != nullptr || frame_key != nullptr,
                 "%s: without picks the frames need their keys (frame_key)", who);
  PCAA_CHECK_ARG(((uintptr_t)points % (points_f64 ? 8 : 4)) == 0, "%s: points are misaligned", who);
  const dim3 grid((unsigned)n_out);
  if (points_f64)
    launch_frames_from_raw<double>(C, grid, as_stream(stream), static_cast<const double*>(points), P, offsets, n, pick,
                                   frame_key, seed, N, standardize, divide_by_std, kp, out, pick_out, err_flag);
  else
    launch_frames_from_raw<float>(C, grid, as_stream(stream), static_cast<const float*>(points), P, offsets, n, pick,
                                  frame_key, seed, N, standardize, divide_by_std, kp, out, pick_out, err_flag);
  PCAA_RETURN_LAUNCH_STATUS(who);
}

template <typename KP>
int crops_from_raw_impl(const char* who, const void* points, int points_f64, long P, const int* offsets, long F,
                        const int* start, int B, int T, const int* pick, const int* frame_key, long seed, int N, int C,
                        int standardize, int divide_by_std, KP kp, float* out, int* err_flag, void* stream) {
  PCAA_CHECK_ARG(B >= 1 && T >= 1 && F >= 0 && P >= 0 && (long)B * T < (1L << 31) && F < (1L << 31),
                 "%s: needs B >= 1, T >= 1, B * T < 2^31, 0 <= F < 2^31, P >= 0", who);
  PCAA_CHECK_ARG(N >= 1 && N <= PCAA_RAW_MAX_POINTS && C >= 1 && C <= RAW_COLS,
                 "%s: needs 1 <= N <= PCAA_RAW_MAX_POINTS and 1 <= C <= 5", who);
  PCAA_CHECK_ARG(out != nullptr && ((uintptr_t)out % 4) == 0, "%s: out is null or not 4-B aligned", who);
  PCAA_CHECK_ARG(start != nullptr && offsets != nullptr && (points != nullptr || P == 0),
                 "%s: points / offsets / start are null", who);
  PCAA_CHECK_ARG(F == 0 || pick != nullptr || frame_key != nullptr,
                 "%s: without picks the frames need their keys (frame_key)", who);
  PCAA_CHECK_ARG(((uintptr_t)points % (points_f64 ? 8 : 4)) == 0, "%s: points are misaligned", who);
  const dim3 grid((unsigned)((long)B * T));
  if (points_f64)
    launch_crops_from_raw<double>(C, grid, as_stream(stream), static_cast<const double*>(points), P, offsets, F, start,
                                  T, pick, frame_key, seed, N, standardize, divide_by_std, kp, out, err_flag);
  else
    launch_crops_from_raw<float>(C, grid, as_stream(stream), static_cast<const float*>(points), P, offsets, F, start, T,
                                 pick, frame_key, seed, N, standardize, divide_by_std, kp, out, err_flag);
  PCAA_RETURN_LAUNCH_STATUS(who);
}

template <typename KP>
int frames_from_raw_unique_impl(const char* who, const void* points, int points_f64, long P, const int* offsets, int n,
                                const int* pick, const int* frame_key, long seed, int N, int C, int standardize,
                                int divide_by_std, KP kp, float* rows, float* weight, int* u_off, long M,
                                int* pick_out, int* err_flag, void* stream) {
  PCAA_CHECK_ARG(n >= 0 && M >= 1 && P >= 0 && (long)n * PCAA_RAW_MAX_POINTS < (1L << 31) && M < (1L << 31),
                 "%s: needs n >= 0, 1 <= M < 2^31, P >= 0, n * 1024 < 2^31", who);
  PCAA_CHECK_ARG(N >= 1 && N <= PCAA_RAW_MAX_POINTS && C >= 1 && C <= RAW_COLS,
                 "%s: needs 1 <= N <= PCAA_RAW_MAX_POINTS and 1 <= C <= 5", who);
  PCAA_CHECK_ARG(rows != nullptr && weight != nullptr && u_off != nullptr && ((uintptr_t)rows % 4) == 0 &&
                     ((uintptr_t)weight % 4) == 0 && ((uintptr_t)u_off % 4) == 0,
                 "%s: rows / weight / u_off are null or not 4-B aligned", who);
  PCAA_CHECK_ARG(n == 0 || (offsets != nullptr && (points != nullptr || P == 0)), "%s: points / offsets are null", who);
  PCAA_CHECK_ARG(n == 0 || pick != nullptr || frame_key != nullptr,
                 "%s: without picks the frames need their keys (frame_key)", who);
  PCAA_CHECK_ARG(((uintptr_t)points % (points_f64 ? 8 : 4)) == 0, "%s: points are misaligned", who);
  const uint32_t lo = (uint32_t)((uint64_t)seed & 0xffffffffu), hi = (uint32_t)((uint64_t)seed >> 32);
  const RawKeep& thin = kp;                       // u_off does not depend on the augmentation
  if (kp.keep > 0)
    hipLaunchKernelGGL(raw_unique_offsets_kernel<true>, dim3(1), dim3(SCAN_THREADS), 0, as_stream(stream), offsets, n, P,
                       N, u_off, frame_key, lo, hi, thin);
  else
    hipLaunchKernelGGL(raw_unique_offsets_kernel<false>, dim3(1), dim3(SCAN_THREADS), 0, as_stream(stream), offsets, n,
                       P, N, u_off, frame_key, lo, hi, thin);
  long tail = cdiv(M, 4096);                      // blocks that zero the rows no frame owns
  tail = tail < 1 ? 1 : (tail > 64 ? 64 : tail);
  const dim3 grid((unsigned)(n + tail));
  if (points_f64)
    launch_frames_from_raw_unique<double>(C, grid, as_stream(stream), static_cast<const double*>(points), P, offsets, n,
                                          pick, frame_key, seed, N, standardize, divide_by_std, kp, rows, weight, u_off,
                                          M, pick_out, err_flag);
  else
    launch_frames_from_raw_unique<float>(C, grid, as_stream(stream), static_cast<const float*>(points), P, offsets, n,
                                         pick, frame_key, seed, N, standardize, divide_by_std, kp, rows, weight, u_off,
                                         M, pick_out, err_flag);
  PCAA_RETURN_LAUNCH_STATUS(who);
}

}  // namespace

extern "C" int pcaa_frames_from_raw(const void* points, int points_f64, long P, const int* offsets, int n, const int* pick,
                                    const int* frame_key, long seed, int N, int C, int standardize, int divide_by_std,
                                    float* out, int n_out, int* pick_out, int* err_flag, void* stream) {
  return frames_from_raw_impl("pcaa_frames_from_raw", points, points_f64, P, offsets, n, pick, frame_key, seed, N, C,
                              standardize, divide_by_std, RawKeep{0, 0, 0}, out, n_out, pick_out, err_flag, stream);
}

extern "C" int pcaa_frames_from_raw_thin(const void* points, int points_f64, long P, const int* offsets, int n,
                                         const int* pick, const int* frame_key, long seed, int N, int C, int standardize,
                                         int divide_by_std, float* out, int n_out, int* pick_out, int* err_flag,
                                         void* stream, int keep, int keep_min, int keep_rule) {
  const char* who = "pcaa_frames_from_raw_thin";
  if (int rc = check_keep(who, keep, keep_min, keep_rule, pick, frame_key, n)) return rc;
  return frames_from_raw_impl(who, points, points_f64, P, offsets, n, pick, frame_key, seed, N, C, standardize,
                              divide_by_std, RawKeep{keep, keep_min, keep_rule}, out, n_out, pick_out, err_flag, stream);
}

extern "C" int pcaa_crops_from_raw(const void* points, int points_f64, long P, const int* offsets, long F,
                                   const int* start, int B, int T, const int* pick, const int* frame_key, long seed,
                                   int N, int C, int standardize, int divide_by_std, float* out, int* err_flag,
                                   void* stream) {
  return crops_from_raw_impl("pcaa_crops_from_raw", points, points_f64, P, offsets, F, start, B, T, pick, frame_key, seed,
                             N, C, standardize, divide_by_std, RawKeep{0, 0, 0}, out, err_flag, stream);
}

extern "C" int pcaa_crops_from_raw_thin(const void* points, int points_f64, long P, const int* offsets, long F,
                                        const int* start, int B, int T, const int* pick, const int* frame_key, long seed,
                                        int N, int C, int standardize, int divide_by_std, float* out, int* err_flag,
                                        void* stream, int keep, int keep_min, int keep_rule) {
  const char* who = "pcaa_crops_from_raw_thin";
  if (int rc = check_keep(who, keep, keep_min, keep_rule, pick, frame_key, F)) return rc;
  return crops_from_raw_impl(who, points, points_f64, P, offsets, F, start, B, T, pick, frame_key, seed, N, C,
                             standardize, divide_by_std, RawKeep{keep, keep_min, keep_rule}, out, err_flag, stream);
}

extern "C" int pcaa_frames_from_raw_unique(const void* points, int points_f64, long P, const int* offsets, int n,
                                           const int* pick, const int* frame_key, long seed, int N, int C,
                                           int standardize, int divide_by_std, float* rows, float* weight, int* u_off,
                                           long M, int* pick_out, int* err_flag, void* stream) {
  return frames_from_raw_unique_impl("pcaa_frames_from_raw_unique", points, points_f64, P, offsets, n, pick, frame_key,
                                     seed, N, C, standardize, divide_by_std, RawKeep{0, 0, 0}, rows, weight, u_off, M,
                                     pick_out, err_flag, stream);
}

extern "C" int pcaa_frames_from_raw_unique_thin(const void* points, int points_f64, long P, const int* offsets, int n,
                                                const int* pick, const int* frame_key, long seed, int N, int C,
                                                int standardize, int divide_by_std, float* rows, float* weight,
                                                int* u_off, long M, int* pick_out, int* err_flag, void* stream, int keep,
                                                int keep_min, int keep_rule) {
  const char* who = "pcaa_frames_from_raw_unique_thin";
  if (int rc = check_keep(who, keep, keep_min, keep_rule, pick, frame_key, n)) return rc;
  return frames_from_raw_unique_impl(who, points, points_f64, P, offsets, n, pick, frame_key, seed, N, C, standardize,
                                     divide_by_std, RawKeep{keep, keep_min, keep_rule}, rows, weight, u_off, M, pick_out,
                                     err_flag, stream);
}

extern "C" int pcaa_frames_from_raw_aug(const void* points, int points_f64, long P, const int* offsets, int n,
                                        const int* pick, const int* frame_key, long seed, int N, int C, int standardize,
                                        int divide_by_std, float* out, int n_out, int* pick_out, int* err_flag,
                                        void* stream, int keep, int keep_min, int keep_rule, const double* aug) {
  const char* who = "pcaa_frames_from_raw_aug";
  RawKeepAug kp;
  if (int rc = check_aug(who, aug, C, keep, keep_min, keep_rule, pick, frame_key, n, kp)) return rc;
  return frames_from_raw_impl(who, points, points_f64, P, offsets, n, pick, frame_key, seed, N, C, standardize,
                              divide_by_std, kp, out, n_out, pick_out, err_flag, stream);
}

extern "C" int pcaa_crops_from_raw_aug(const void* points, int points_f64, long P, const int* offsets, long F,
                                       const int* start, int B, int T, const int* pick, const int* frame_key, long seed,
                                       int N, int C, int standardize, int divide_by_std, float* out, int* err_flag,
                                       void* stream, int keep, int keep_min, int keep_rule, const double* aug) {
  const char* who = "pcaa_crops_from_raw_aug";
  RawKeepAug kp;
  if (int rc = check_aug(who, aug, C, keep, keep_min, keep_rule, pick, frame_key, F, kp)) return rc;
  return crops_from_raw_impl(who, points, points_f64, P, offsets, F, start, B, T, pick, frame_key, seed, N, C,
                             standardize, divide_by_std, kp, out, err_flag, stream);
}

extern "C" int pcaa_frames_from_raw_unique_aug(const void* points, int points_f64, long P, const int* offsets, int n,
                                               const int* pick, const int* frame_key, long seed, int N, int C,
                                               int standardize, int divide_by_std, float* rows, float* weight,
                                               int* u_off, long M, int* pick_out, int* err_flag, void* stream, int keep,
                                               int keep_min, int keep_rule, const double* aug) {
  const char* who = "pcaa_frames_from_raw_unique_aug";
  RawKeepAug kp;
  if (int rc = check_aug(who, aug, C, keep, keep_min, keep_rule, pick, frame_key, n, kp)) return rc;
  return frames_from_raw_unique_impl(who, points, points_f64, P, offsets, n, pick, frame_key, seed, N, C, standardize,
                                     divide_by_std, kp, rows, weight, u_off, M, pick_out, err_flag, stream);
}
