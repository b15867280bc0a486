// How fast can the element-wise passes of the PointNet block stream on gfx950?  Three skeletons over random bf16
// operands [245760, 512] and [245760, 1024]:
//   rd   read only, per-column sum and sum of squares into 2*ch fp64 values (replicated, atomics)
//   rw   read + write            a  = ELU(y*s + t)
//   rrw  two reads + one write   dy = c0*dz + c1*y + c2, in place over dz
// and for each of them
//   ctl        today's loop: flat 8-byte quads, column-invariant grid-stride, up to 2048 workgroups
//   w16        the same loop with 16 bytes (8 channels) per lane
//   ring k R   persistent grid of k workgroups per CU, each lane keeps R row-loads ahead of its arithmetic
//              (rows past the end are clamped, loads are never branched around, stores are predicated)
//   dma k R    the same ring filled by buffer_load ... lds into a per-wave LDS ring, ds_read by the owning lane
//   +nl / +ns  non-temporal loads / non-temporal stores
// 9 interleaved rounds; per variant the median and min-max in us and the rate of the bytes the skeleton must move.
// Every variant's output is compared with the control's before it is timed.
//   hipcc --offload-arch=gfx950 -O3 -o ew_stream ew_stream.hip && ./ew_stream
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <type_traits>
#include <utility>
#include <string>
#include <vector>

typedef __bf16 bf16_t;
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;

enum { RD = 0, RW = 1, RRW = 2 };
constexpr int NREP = 32;   // replicas of the rd skeleton's statistics

__device__ __forceinline__ f32x4 unpack(u32x2 raw) {
  f32x4 r;
  r.x = __uint_as_float(raw.x << 16); r.y = __uint_as_float(raw.x & 0xffff0000u);
  r.z = __uint_as_float(raw.y << 16); r.w = __uint_as_float(raw.y & 0xffff0000u);
  return r;
}
__device__ __forceinline__ u32x2 pack(f32x4 v) {
  bf16x4 b;
  b.x = (bf16_t)v.x; b.y = (bf16_t)v.y; b.z = (bf16_t)v.z; b.w = (bf16_t)v.w;
  return __builtin_bit_cast(u32x2, b);
}
__device__ __forceinline__ float elu(float z) { return z > 0.f ? z : __expf(z) - 1.f; }
__device__ __forceinline__ f32x4 load4f(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// per-quad arithmetic of the three skeletons; k[0..2] are the quad's coefficient vectors.  The fused multiply-adds are
// written out: left to the compiler, k0*d + k1*y + k2 was contracted one way in one kernel and the other way in the
// next (even in one of the 2R unrolled copies of a ring's body and not the others), and the comparison with the control
// reported a few thousand last-bit differences that were no variant's fault.
template <int SK>
__device__ __forceinline__ u32x2 quad_op(u32x2 ry, u32x2 rd, const f32x4* k) {
#pragma clang fp contract(off)
  const f32x4 v = unpack(ry);
  if (SK == RW) {
    f32x4 o;
    o.x = elu(__builtin_fmaf(v.x, k[0].x, k[1].x)); o.y = elu(__builtin_fmaf(v.y, k[0].y, k[1].y));
    o.z = elu(__builtin_fmaf(v.z, k[0].z, k[1].z)); o.w = elu(__builtin_fmaf(v.w, k[0].w, k[1].w));
    return pack(o);
  }
  const f32x4 t = k[1] * v;
  return pack(__builtin_elementwise_fma(k[0], unpack(rd), t) + k[2]);
}

template <int NT, typename V>
__device__ __forceinline__ V ld(const void* p) {
  if (NT & 1) return __builtin_nontemporal_load(reinterpret_cast<const V*>(p));
  return *reinterpret_cast<const V*>(p);
}
template <int NT, typename V>
__device__ __forceinline__ void st(void* p, V v) {
  if (NT & 2) __builtin_nontemporal_store(v, reinterpret_cast<V*>(p));
  else *reinterpret_cast<V*>(p) = v;
}

// column sums of the rd skeleton: the workgroup's row lanes are folded in LDS, then one fp64 atomic per column
template <int W>
__device__ __forceinline__ void flush_stats(float (&s1)[W], float (&s2)[W], double* stats, unsigned ch, unsigned lanes_per_row,
                                            unsigned c) {
  __shared__ float red[2][256 * W];
#pragma unroll
  for (int e = 0; e < W; ++e) { red[0][threadIdx.x * W + e] = s1[e]; red[1][threadIdx.x * W + e] = s2[e]; }
  __syncthreads();
  if (threadIdx.x < lanes_per_row) {
    double* dst = stats + (size_t)(blockIdx.x % NREP) * 2 * ch;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      double a = 0.0, b = 0.0;
      for (unsigned l = 0; l < 256 / lanes_per_row; ++l) {
        a += red[0][(l * lanes_per_row + threadIdx.x) * W + e];
        b += red[1][(l * lanes_per_row + threadIdx.x) * W + e];
      }
      atomicAdd(dst + c + e, a);
      atomicAdd(dst + ch + c + e, b);
    }
  }
}

// ---------------------------------------------------------------- ctl / w16: flat grid-stride, W = 4 or 8 channels per lane
template <int SK, int W, int NT>
__global__ __launch_bounds__(256) void flat_kernel(const bf16_t* __restrict__ y, bf16_t* io, const float* __restrict__ coef,
                                                   double* stats, unsigned nvec, unsigned vpr, unsigned ch) {
  typedef typename std::conditional<W == 8, u32x4, u32x2>::type V;
  const unsigned q0 = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;
  const unsigned c = (q0 % vpr) * W;
  f32x4 k[W / 4][3];
#pragma unroll
  for (int h = 0; h < W / 4; ++h)
#pragma unroll
    for (int j = 0; j < 3; ++j) k[h][j] = load4f(coef + j * ch + c + 4 * h);
  float s1[W] = {}, s2[W] = {};
  for (unsigned q = q0; q < nvec; q += stride) {
    const size_t o = (size_t)q * W;
    const V vy = ld<NT, V>(y + o);
    V vd = vy;
    if (SK == RRW) vd = ld<NT, V>(io + o);
    if (SK == RD) {
#pragma unroll
      for (int h = 0; h < W / 4; ++h) {
        const f32x4 v = unpack(u32x2{vy[2 * h], vy[2 * h + 1]});
#pragma unroll
        for (int e = 0; e < 4; ++e) { s1[4 * h + e] += v[e]; s2[4 * h + e] += v[e] * v[e]; }
      }
    } else {
      V out;
#pragma unroll
      for (int h = 0; h < W / 4; ++h) {
        const u32x2 r = quad_op<SK>(u32x2{vy[2 * h], vy[2 * h + 1]}, u32x2{vd[2 * h], vd[2 * h + 1]}, k[h]);
        out[2 * h] = r.x; out[2 * h + 1] = r.y;
      }
      st<NT, V>(io + o, out);
    }
  }
  if (SK == RD) flush_stats<W>(s1, s2, stats, ch, vpr, c);
}

// ---------------------------------------------------------------- ring: persistent grid, R row-loads ahead per lane
template <int SK, int R, int NT>
__global__ __launch_bounds__(256) void ring_kernel(const bf16_t* __restrict__ y, bf16_t* io, const float* __restrict__ coef,
                                                   double* stats, unsigned rows, unsigned ch) {
  const unsigned L = ch >> 3, rpt = 256u / L;             // lanes per row, rows per trip
  const unsigned c = (threadIdx.x % L) << 3, rl = threadIdx.x / L;
  const unsigned trips = (rows + rpt - 1) / rpt, G = gridDim.x;
  f32x4 k[2][3];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < 3; ++j) k[h][j] = load4f(coef + j * ch + c + 4 * h);
  float s1[8] = {}, s2[8] = {};
  u32x4 by[R], bd[R];
  auto issue = [&](int s, unsigned t) {
    const unsigned row = min(t * rpt + rl, rows - 1);      // clamped, never branched around
    const size_t o = (size_t)row * ch + c;
    by[s] = ld<NT, u32x4>(y + o);
    if (SK == RRW) bd[s] = ld<NT, u32x4>(io + o);
  };
  // one stage: consume the landed row, refill the slot (when more is coming), store
  auto consume = [&](int s, unsigned tt, bool refill, bool all_valid) {
    const unsigned row = tt * rpt + rl;
    const bool ok = all_valid || row < rows;
    if (SK == RD) {
      const float m = ok ? 1.f : 0.f;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x4 v = unpack(u32x2{by[s][2 * h], by[s][2 * h + 1]}) * m;
#pragma unroll
        for (int e = 0; e < 4; ++e) { s1[4 * h + e] += v[e]; s2[4 * h + e] += v[e] * v[e]; }
      }
      if (refill) issue(s, tt + R * G);
    } else {
      u32x4 out;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const u32x2 r = quad_op<SK>(u32x2{by[s][2 * h], by[s][2 * h + 1]}, u32x2{bd[s][2 * h], bd[s][2 * h + 1]}, k[h]);
        out[2 * h] = r.x; out[2 * h + 1] = r.y;
      }
      if (refill) issue(s, tt + R * G);
      if (ok) st<NT, u32x4>(io + (size_t)row * ch + c, out);
    }
  };
  unsigned t = blockIdx.x;
#pragma unroll
  for (int s = 0; s < R; ++s) issue(s, t + s * G);
  // full batches: all R stages are whole trips, stores are unconditional (the waits stay counted)
  const unsigned full = rows / rpt;
  for (; t + (R - 1) * G < full; t += R * G) {
#pragma unroll
    for (int s = 0; s < R; ++s) consume(s, t + s * G, true, true);
  }
  // what the ring still holds: trips t + s*G, the last of them partial or past the end
#pragma unroll
  for (int s = 0; s < R; ++s) consume(s, t + s * G, false, false);
  if (SK == RD) flush_stats<8>(s1, s2, stats, ch, L, c);
}

// ---------------------------------------------------------------- dma: the ring lives in LDS, filled by buffer_load ... lds
// ch >= 512 and rows % (256 / (ch/8)) == 0 only (a wave = 1 KB of one row): lab shapes.  The waits are counted: at
// the wait for step i the operations issued behind its loads are the other R-1 stages' loads and the stores of the
// last min(i, R) steps; the main loop runs whole batches of R valid trips, so every one of them was issued.  The
// stages the ring still holds after it are finished behind a vmcnt(0).
template <int SK, int R, int NT>
__global__ __launch_bounds__(256) void dma_kernel(const bf16_t* __restrict__ y, bf16_t* io, const float* __restrict__ coef,
                                                  double* stats, unsigned rows, unsigned ch) {
  constexpr int NIN = SK == RRW ? 2 : 1, NST = SK == RD ? 0 : 1;
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * R * NIN * 1024];
  const unsigned L = ch >> 3, rpt = 256u / L;
  const unsigned c = (threadIdx.x % L) << 3, rl = threadIdx.x / L;
  const unsigned trips = rows / rpt, G = gridDim.x;
  const unsigned lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned wave_off = __builtin_amdgcn_readfirstlane((rl * ch + (c & ~511u)) * 2u);   // bytes, wave-uniform
  const unsigned trip_bytes = rpt * ch * 2u;
  unsigned char* slot = lds + wave * (R * NIN * 1024);
  const unsigned total = rows * ch * 2u;
  rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(y), 0, (int)total, 0x00020000);
  rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(io, 0, (int)total, 0x00020000);
  f32x4 k[2][3];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < 3; ++j) k[h][j] = load4f(coef + j * ch + c + 4 * h);
  float s1[8] = {}, s2[8] = {};
  auto issue = [&](int s, unsigned t) {
    const unsigned tc = min(t, trips - 1);
    const unsigned soff = tc * trip_bytes + wave_off;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(ry, (__attribute__((address_space(3))) void*)(slot + (s * NIN) * 1024), 16,
                                             lane * 16, soff, 0, (NT & 1) ? 2 : 0);
    if (SK == RRW)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (__attribute__((address_space(3))) void*)(slot + (s * NIN + 1) * 1024),
                                               16, lane * 16, soff, 0, (NT & 1) ? 2 : 0);
  };
  auto finish = [&](int s, unsigned tt, bool ok, bool refill) {
    const unsigned row = tt * rpt + rl;
    const u32x4 vy = *(const u32x4*)(slot + (s * NIN) * 1024 + lane * 16);
    u32x4 vd = vy;
    if (SK == RRW) vd = *(const u32x4*)(slot + (s * NIN + 1) * 1024 + lane * 16);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (refill) issue(s, tt + R * G);
    if (SK == RD) {
      const float m = ok ? 1.f : 0.f;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x4 v = unpack(u32x2{vy[2 * h], vy[2 * h + 1]}) * m;
#pragma unroll
        for (int e = 0; e < 4; ++e) { s1[4 * h + e] += v[e]; s2[4 * h + e] += v[e] * v[e]; }
      }
    } else {
      u32x4 out;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const u32x2 r = quad_op<SK>(u32x2{vy[2 * h], vy[2 * h + 1]}, u32x2{vd[2 * h], vd[2 * h + 1]}, k[h]);
        out[2 * h] = r.x; out[2 * h + 1] = r.y;
      }
      if (ok) st<NT, u32x4>(io + (size_t)row * ch + c, out);
    }
  };
  unsigned t = blockIdx.x;
#pragma unroll
  for (int s = 0; s < R; ++s) issue(s, t + s * G);
  bool first = true;
  auto step = [&](auto S) {
    constexpr int s = decltype(S)::value;
    if (first) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((R - 1) * NIN + s * NST) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((R - 1) * NIN + R * NST) : "memory");
    finish(s, t + s * G, true, true);
  };
  for (; t + (R - 1) * G < trips; t += R * G) {
    step(std::integral_constant<int, 0>{});
    if constexpr (R > 1) step(std::integral_constant<int, 1>{});
    if constexpr (R > 2) { step(std::integral_constant<int, 2>{}); step(std::integral_constant<int, 3>{}); }
    first = false;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int s = 0; s < R; ++s) finish(s, t + s * G, t + s * G < trips, false);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (SK == RD) flush_stats<8>(s1, s2, stats, ch, L, c);
}

// ---------------------------------------------------------------- host
struct Bufs { bf16_t *y, *io, *src, *ref; float* coef; double *stats, *stats_ref; unsigned* diff; };

static int col_invariant_grid(long nvec, int vpr) {
  int a = vpr, b = 256;
  while (b) { const int t = a % b; a = b; b = t; }
  const int unit = vpr / a;
  long g = (nvec + 255) / 256;
  if (g > 2048) g = 2048;
  return (int)((g + unit - 1) / unit * unit);
}

struct Variant {
  std::string name;
  int sk;
  void (*launch)(const Bufs&, unsigned rows, unsigned ch, int k);
  int k;
  std::vector<float> us;
};

template <int SK, int W, int NT>
static void launch_flat(const Bufs& b, unsigned rows, unsigned ch, int) {
  const long nvec = (long)rows * (ch / W);
  hipLaunchKernelGGL((flat_kernel<SK, W, NT>), dim3(col_invariant_grid(nvec, ch / W)), dim3(256), 0, 0, b.y, b.io, b.coef,
                     b.stats, (unsigned)nvec, ch / W, ch);
}
template <int SK, int R, int NT>
static void launch_ring(const Bufs& b, unsigned rows, unsigned ch, int k) {
  hipLaunchKernelGGL((ring_kernel<SK, R, NT>), dim3(256 * k), dim3(256), 0, 0, b.y, b.io, b.coef, b.stats, rows, ch);
}
template <int SK, int R, int NT>
static void launch_dma(const Bufs& b, unsigned rows, unsigned ch, int k) {
  hipLaunchKernelGGL((dma_kernel<SK, R, NT>), dim3(256 * k), dim3(256), 0, 0, b.y, b.io, b.coef, b.stats, rows, ch);
}

__global__ void fill_kernel(bf16_t* p, size_t n, unsigned seed, float amp) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned h = (unsigned)i * 2654435761u + seed;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
    p[i] = (bf16_t)(((float)(h & 0xffff) / 32768.f - 1.f) * amp);
  }
}
__global__ void diff_kernel(const unsigned* a, const unsigned* b, size_t n, unsigned* out) {
  unsigned d = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) d += a[i] != b[i];
  if (d) atomicAdd(out, d);
}

static const char* nt_name(int nt) { return nt == 0 ? "" : nt == 1 ? "+nl" : nt == 2 ? "+ns" : "+nl+ns"; }

template <int SK>
static void add_variants(std::vector<Variant>& v) {
  const char* sk = SK == RD ? "rd " : SK == RW ? "rw " : "rrw";
  auto nm = [&](const char* base, int k, int r, int nt) {
    char buf[64];
    if (k) snprintf(buf, sizeof(buf), "%s %s k=%d R=%d%s", sk, base, k, r, nt_name(nt));
    else snprintf(buf, sizeof(buf), "%s %s%s", sk, base, nt_name(nt));
    return std::string(buf);
  };
  v.push_back({nm("ctl", 0, 0, 0), SK, launch_flat<SK, 4, 0>, 0, {}});
  v.push_back({nm("w16", 0, 0, 0), SK, launch_flat<SK, 8, 0>, 0, {}});
  v.push_back({nm("w16", 0, 0, 1), SK, launch_flat<SK, 8, 1>, 0, {}});
  if (SK != RD) {
    v.push_back({nm("ctl", 0, 0, 2), SK, launch_flat<SK, 4, 2>, 0, {}});
    v.push_back({nm("w16", 0, 0, 2), SK, launch_flat<SK, 8, 2>, 0, {}});
    v.push_back({nm("w16", 0, 0, 3), SK, launch_flat<SK, 8, 3>, 0, {}});
  }
#define RING(K, R)                                                                     \
  v.push_back({nm("ring", K, R, 0), SK, launch_ring<SK, R, 0>, K, {}});                \
  v.push_back({nm("ring", K, R, 1), SK, launch_ring<SK, R, 1>, K, {}});                \
  if (SK != RD) {                                                                      \
    v.push_back({nm("ring", K, R, 2), SK, launch_ring<SK, R, 2>, K, {}});              \
    v.push_back({nm("ring", K, R, 3), SK, launch_ring<SK, R, 3>, K, {}});              \
  }
  RING(1, 4) RING(1, 8) RING(2, 2) RING(2, 4) RING(4, 1) RING(4, 2) RING(4, 4) RING(8, 1) RING(8, 2)
#undef RING
#define DMA(K, R)                                                                      \
  v.push_back({nm("dma", K, R, 0), SK, launch_dma<SK, R, 0>, K, {}});                  \
  v.push_back({nm("dma", K, R, 1), SK, launch_dma<SK, R, 1>, K, {}});                  \
  if (SK != RD) v.push_back({nm("dma", K, R, 3), SK, launch_dma<SK, R, 3>, K, {}});
  DMA(2, 2) DMA(2, 4) DMA(4, 2)
#undef DMA
}

#define CK(x)                                                                    \
  do {                                                                           \
    hipError_t e_ = (x);                                                         \
    if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } \
  } while (0)

int main(int argc, char** argv) {
  const unsigned rows = argc > 1 ? (unsigned)atoi(argv[1]) : 245760u;
  const int rounds = 9;
  const size_t maxn = (size_t)rows * 1024;
  Bufs b;
  CK(hipMalloc(&b.y, maxn * 2)); CK(hipMalloc(&b.io, maxn * 2)); CK(hipMalloc(&b.src, maxn * 2)); CK(hipMalloc(&b.ref, maxn * 2));
  CK(hipMalloc(&b.coef, 3 * 1024 * 4)); CK(hipMalloc(&b.stats, NREP * 2 * 1024 * 8)); CK(hipMalloc(&b.stats_ref, NREP * 2 * 1024 * 8));
  CK(hipMalloc(&b.diff, 4));
  hipLaunchKernelGGL(fill_kernel, dim3(2048), dim3(256), 0, 0, b.y, maxn, 1u, 1.5f);
  hipLaunchKernelGGL(fill_kernel, dim3(2048), dim3(256), 0, 0, b.src, maxn, 77u, 0.2f);
  std::vector<float> hc(3 * 1024);
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (unsigned ch : {512u, 1024u}) {
    // rw reads k0 = scale, k1 = shift; rrw reads c0, c1, c2 (|c0| < 1 keeps the in-place iteration bounded)
    for (unsigned c = 0; c < ch; ++c) {
      hc[c] = 0.5f + 0.4f * sinf(0.37f * c); hc[ch + c] = 0.3f * cosf(0.11f * c); hc[2 * ch + c] = 0.01f * sinf(0.05f * c);
    }
    CK(hipMemcpy(b.coef, hc.data(), 3 * ch * 4, hipMemcpyHostToDevice));
    const size_t n = (size_t)rows * ch;
    std::vector<Variant> vars;
    add_variants<RD>(vars); add_variants<RW>(vars); add_variants<RRW>(vars);
    // correctness against the control of the same skeleton, once
    std::vector<double> sref(2 * ch), sgot(NREP * 2 * ch);
    for (auto& v : vars) {
      const bool is_ctl = v.name.find("ctl") != std::string::npos && v.name.find('+') == std::string::npos;
      CK(hipMemcpy(b.io, b.src, n * 2, hipMemcpyDeviceToDevice));
      CK(hipMemset(b.stats, 0, NREP * 2 * ch * 8));
      v.launch(b, rows, ch, v.k);
      CK(hipDeviceSynchronize());
      if (v.sk == RD) {
        CK(hipMemcpy(sgot.data(), b.stats, NREP * 2 * ch * 8, hipMemcpyDeviceToHost));
        std::vector<double> s(2 * ch, 0.0);
        for (int r = 0; r < NREP; ++r) for (unsigned i = 0; i < 2 * ch; ++i) s[i] += sgot[(size_t)r * 2 * ch + i];
        if (is_ctl) sref = s;
        else {
          double worst = 0.0;
          for (unsigned i = 0; i < 2 * ch; ++i) worst = std::max(worst, fabs(s[i] - sref[i]) / (fabs(sref[i]) + 1.0 + (i >= ch ? 1e3 : 1e2)));
          if (worst > 1e-2) printf("MISMATCH [%u] %s: stats differ by %.3g\n", ch, v.name.c_str(), worst);
        }
      } else if (is_ctl) {
        CK(hipMemcpy(b.ref, b.io, n * 2, hipMemcpyDeviceToDevice));
      } else {
        CK(hipMemset(b.diff, 0, 4));
        hipLaunchKernelGGL(diff_kernel, dim3(2048), dim3(256), 0, 0, (const unsigned*)b.io, (const unsigned*)b.ref, n / 2, b.diff);
        unsigned d = 0;
        CK(hipMemcpy(&d, b.diff, 4, hipMemcpyDeviceToHost));
        if (d) printf("MISMATCH [%u] %s: %u words differ from the control\n", ch, v.name.c_str(), d);
      }
    }
    CK(hipMemcpy(b.io, b.src, n * 2, hipMemcpyDeviceToDevice));
    for (int round = -1; round < rounds; ++round) {       // round -1 warms up
      for (auto& v : vars) {
        CK(hipEventRecord(e0));
        v.launch(b, rows, ch, v.k);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (round >= 0) v.us.push_back(ms * 1e3f);
      }
    }
    float ctl_med[3] = {}, ctl_lo[3] = {}, ctl_hi[3] = {};
    for (auto& v : vars) {
      std::sort(v.us.begin(), v.us.end());
      const float med = v.us[v.us.size() / 2], lo = v.us.front(), hi = v.us.back();
      const bool is_ctl = v.name.find("ctl") != std::string::npos && v.name.find('+') == std::string::npos;
      if (is_ctl) { ctl_med[v.sk] = med; ctl_lo[v.sk] = lo; ctl_hi[v.sk] = hi; }
      const double bytes = (double)n * 2 * (v.sk + 1);
      printf("[%4u] %-24s %7.1f us (%6.1f-%6.1f) %5.2f TB/s | ctl %7.1f (%6.1f-%6.1f) %s\n", ch, v.name.c_str(), med, lo, hi,
             bytes / med / 1e6, ctl_med[v.sk], ctl_lo[v.sk], ctl_hi[v.sk],
             is_ctl ? "" : (ctl_med[v.sk] - med > ctl_hi[v.sk] - ctl_lo[v.sk] ? "WINS" : (med > ctl_med[v.sk] ? "loses" : "inside spread")));
    }
    fflush(stdout);
  }
  CK(hipDeviceSynchronize());
  printf("%s\n", hipGetErrorString(hipGetLastError()));
  return 0;
}
