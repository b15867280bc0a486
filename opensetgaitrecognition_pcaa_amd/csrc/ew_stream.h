// One streaming skeleton for the element-wise passes over a bf16 [rows, ch] tensor (tools/microbench/ew_stream.hip is
// the lab it comes from, profiles/ew_stream_lab.txt its table): a persistent grid of K workgroups per CU, 16 bytes
// (8 channels) per lane, and per lane an explicit ring of R row-loads ahead of the arithmetic, so that what a CU keeps
// in flight is a chosen amount (K * R * 4 KB per input) and not whatever the occupancy happens to give.
//
// The skeleton owns
//   - the row walk: a trip is the 256 / (ch/8) rows one workgroup covers at once; workgroup b takes trips b, b + G, ...
//   - the lane-to-channel mapping: a lane keeps ONE channel octet for its whole life -- the functor loads its
//     coefficients into registers once, no index division anywhere;
//   - the load ring: R stages, each refilled as soon as it is consumed; loads are never branched around -- a row past
//     the end is clamped to the last row and what it returns is not used;
//   - the tail: the main loop runs whole batches of R full trips with UNCONDITIONAL stores (so every s_waitcnt in it
//     is counted), the at most R stages the ring still holds after it are stored under a row predicate;
//   - the store policy (plain or non-temporal, per pass: the lab's table).
// The arithmetic is the functor's: it carries the pass's pointers; F::init(k, c, ch) loads the lane's coefficients
// (F::Coef k, c = first channel of the octet) once, then F::quad(k, h, v0, v1) -> f32x4 forms the low (h = 0) and high
// (h = 1) four channels of a row.
//
// Aliasing: `out` may be `in1` (bn_bwd_dy in place over dz).  A lane reads an element before it writes it -- the ring
// only runs ahead over the lane's OWN later rows -- and no other lane writes that element; the only foreign reads are the
// clamped loads of the last row, whose values are discarded.  The aliased pair is therefore not __restrict__.
#pragma once
#include "common.h"

namespace ew {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int OCT = 8;             // channels per lane (16 bytes of bf16)

// row bytes a multiple of 16 and ch/8 lanes per row tiling a 256-thread workgroup
inline bool ch_ok(int ch) { return ch >= OCT && (ch % OCT) == 0 && ch / OCT <= 256 && (256 % (ch / OCT)) == 0; }
inline int rows_per_trip(int ch) { return 256 / (ch / OCT); }

__device__ __forceinline__ f32x4 unpack(unsigned lo, unsigned hi) {
  return f32x4{__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u), __uint_as_float(hi << 16),
               __uint_as_float(hi & 0xffff0000u)};
}
// the rounding of store4(bf16_t*, f32x4)
__device__ __forceinline__ u32x2 pack(f32x4 v) {
  bf16x4 b;
  b.x = (bf16_t)v.x; b.y = (bf16_t)v.y; b.z = (bf16_t)v.z; b.w = (bf16_t)v.w;
  return __builtin_bit_cast(u32x2, b);
}
template <bool NT>
__device__ __forceinline__ u32x4 load16(const bf16_t* p) {
  if (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
  return *reinterpret_cast<const u32x4*>(p);
}
template <bool NT>
__device__ __forceinline__ void store16(bf16_t* p, u32x4 v) {
  if (NT) __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
  else *reinterpret_cast<u32x4*>(p) = v;
}

// NIN: 1 (out = f(in0)) or 2 (out = f(in0, in1)); NTL / NTS: non-temporal loads / stores
template <int NIN, int R, bool NTL, bool NTS, typename F>
__global__ __launch_bounds__(256) void stream_kernel(const bf16_t* __restrict__ in0, const bf16_t* in1, bf16_t* out, F f,
                                                     unsigned rows, unsigned ch) {
  const unsigned L = ch / OCT, rpt = 256u / L;               // lanes per row, rows per trip
  const unsigned c = (threadIdx.x % L) * OCT, rl = threadIdx.x / L;
  const unsigned G = gridDim.x, full = rows / rpt;           // trips whose rows all exist
  typename F::Coef k;
  f.init(k, c, ch);
  u32x4 b0[R], b1[R];
  auto issue = [&](int s, unsigned t) {
    const unsigned row = min(t * rpt + rl, rows - 1);        // clamped, never branched around
    const size_t o = (size_t)row * ch + c;
    b0[s] = load16<NTL>(in0 + o);
    if (NIN == 2) b1[s] = load16<NTL>(in1 + o);
  };
  auto consume = [&](int s, unsigned t, bool refill, bool all_rows) {
    const unsigned row = t * rpt + rl;
    const u32x4 w0 = b0[s], w1 = NIN == 2 ? b1[s] : b0[s];
    const u32x2 lo = pack(f.quad(k, 0, unpack(w0.x, w0.y), unpack(w1.x, w1.y)));
    const u32x2 hi = pack(f.quad(k, 1, unpack(w0.z, w0.w), unpack(w1.z, w1.w)));
    if (refill) issue(s, t + R * G);
    if (all_rows || row < rows) store16<NTS>(out + (size_t)row * ch + c, u32x4{lo.x, lo.y, hi.x, hi.y});
  };
  unsigned t = blockIdx.x;
#pragma unroll
  for (int s = 0; s < R; ++s) issue(s, t + s * G);
  for (; t + (R - 1) * G < full; t += R * G) {
#pragma unroll
    for (int s = 0; s < R; ++s) consume(s, t + s * G, true, true);
  }
  // the ring holds trips t + s*G: full ones, the partial last one, or (clamped) ones past the end
#pragma unroll
  for (int s = 0; s < R; ++s) consume(s, t + s * G, false, false);
}

// ---------------------------------------------------------------- the passes' arithmetic
// a = ELU(y*scale + shift): bn_act_fwd_kernel<bf16_t>'s expressions (its v*sc + sh contracts to this fused multiply-add)
struct ActFwd {
  const float *scale, *shift;
  struct Coef { f32x4 sc[2], sh[2]; };
  __device__ __forceinline__ void init(Coef& k, unsigned c, unsigned) const {
    k.sc[0] = load4(scale + c); k.sc[1] = load4(scale + c + 4);
    k.sh[0] = load4(shift + c); k.sh[1] = load4(shift + c + 4);
  }
  __device__ __forceinline__ f32x4 quad(const Coef& k, int h, f32x4 v, f32x4) const {
    f32x4 o;
    o.x = elu_t<bf16_t>(__builtin_fmaf(v.x, k.sc[h].x, k.sh[h].x));
    o.y = elu_t<bf16_t>(__builtin_fmaf(v.y, k.sc[h].y, k.sh[h].y));
    o.z = elu_t<bf16_t>(__builtin_fmaf(v.z, k.sc[h].z, k.sh[h].z));
    o.w = elu_t<bf16_t>(__builtin_fmaf(v.w, k.sc[h].w, k.sh[h].w));
    return o;
  }
};

// dy = c0*dz + c1*y + c2 (in0 = y, in1 = dz): bn_bwd_dy_kernel<bf16_t> compiles its k0*d + k1*yv + k2 to
// fma(k0, d, k1*yv) + k2; written out here so that no other contraction can be chosen
struct BwdDy {
  const float* coef;
  struct Coef { f32x4 k0[2], k1[2], k2[2]; };
  __device__ __forceinline__ void init(Coef& k, unsigned c, unsigned ch) const {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      k.k0[h] = load4(coef + c + 4 * h);
      k.k1[h] = load4(coef + ch + c + 4 * h);
      k.k2[h] = load4(coef + 2 * ch + c + 4 * h);
    }
  }
  __device__ __forceinline__ f32x4 quad(const Coef& k, int h, f32x4 yv, f32x4 d) const {
#pragma clang fp contract(off)
    const f32x4 t = k.k1[h] * yv;
    return __builtin_elementwise_fma(k.k0[h], d, t) + k.k2[h];
  }
};

// ---------------------------------------------------------------- launch
// What the lab chose per pass (profiles/ew_stream_lab.txt): K workgroups per CU, R rows ahead, the cache policy.
//   ActFwd: 2 x 2, plain loads and stores -- `a` feeds the next product and must stay in the L2; non-temporal stores
//           without non-temporal loads lost 10-30 % in the lab.
//   BwdDy:  1 x 4, non-temporal both ways -- dz and y are read for the last time, dy is far larger than the L2.
struct ActFwdPolicy { static constexpr int K = 2, R = 2; static constexpr bool NTL = false, NTS = false; };
struct BwdDyPolicy { static constexpr int K = 1, R = 4; static constexpr bool NTL = true, NTS = true; };

int cu_count();      // the device's compute units, asked once (elementwise.hip)

template <int NIN, typename P, typename F>
inline void launch(const bf16_t* in0, const bf16_t* in1, bf16_t* out, const F& f, long rows, int ch, hipStream_t stream) {
  const long trips = cdiv(rows, rows_per_trip(ch));
  long grid = (long)P::K * cu_count();
  if (grid > trips) grid = trips;
  hipLaunchKernelGGL((stream_kernel<NIN, P::R, P::NTL, P::NTS, F>), dim3((unsigned)grid), dim3(256), 0, stream, in0, in1,
                     out, f, (unsigned)rows, (unsigned)ch);
}

}  // namespace ew
