// TemporalConvolutionBlock forward (reference models.py:37-79, 108-160), one launch per layer:
//
//   y_l[(b,t)][co] = sum_{ci,tap} W_l[co][ci][tap] * a_{l-1}[b][t-(2-tap)*d][ci]      (causal, zero for t<0)
//   a_{l-1} = ELU(scale_{l-1} * y_{l-1} + shift_{l-1})   applied once, while the sequence is staged (layer 1: the input as is)
//
// The block holds 0.08 % of the step's FLOPs (2.2 GFLOP forward at B=64) in six layers that each need
// the BatchNorm statistics of ALL B*T rows of the layer before: the unfused path spent 310 us here in 29
// launches (im2col, 128x128-tile MFMA GEMM, split-K reduction, finalize, BN+ELU pass per layer).  This
// kernel does BN/ELU-on-load + implicit im2col + the contraction + the BatchNorm statistics of its own
// output in one launch on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: an fmaf chain, so fp32 mode keeps
// its parity and bf16 mode shares the path).  One workgroup = one sequence (T <= 32 rows) x 32 output
// channels:
//   * the activated sequence tile a[T][channels] is staged in LDS ONCE (coalesced 16-B loads, one ELU per
//     element); the causal shifts of the three taps are row offsets of the MFMA's A-fragment reads into
//     that tile (a dedicated zero row serves t < 0), so im2col never exists as data on the forward path;
//   * the contraction runs tap-major inside 32-channel chunks (k' = tap*32 + ci: any order is valid as
//     long as both operands share it), so a lane's four consecutive k' are four consecutive channels:
//     one 16-B LDS read per operand feeds four MFMAs;
//   * per chunk only the weights move: 32 x 96 floats, contiguous in HBM, scattered tap-major into LDS;
//   * the four waves split each chunk's contraction on the same 32x32 tile and are combined through
//     LDS at the end, where the tile is stored and its column sums go to the fp64 statistics.
// Earlier forms, measured at B=64 (us for the 256->512 layer): gathering im2col elements one by one
// with BN+ELU per gathered element 50-80 (24 scalar loads per thread and chunk: load-issue bound, not
// the expm1f), plain-FMA register tiles 80 (the non-packed fp32 VALU peaks at half the fp32-MFMA rate).
// The first column tile also writes the im2col matrix the BACKWARD's weight gradient contracts with.
#include "common.h"
#include "bn_tail.h"

// LAB builds only (PCAA_HIPCC_EXTRA=-DPCAA_DTC_TRACE, tools/dtc_lab.py --trace): wave 0 of every workgroup adds the clock
// ticks it spent in each phase of the kernel to a device array
#ifdef PCAA_DTC_TRACE
__device__ unsigned long long g_dtc_trace[16];
#define DTC_T0() unsigned long long t_prev = __builtin_readcyclecounter()
#define DTC_MARK(i)                                                              \
  do {                                                                           \
    const unsigned long long t_now = __builtin_readcyclecounter();               \
    if (threadIdx.x == 0) atomicAdd(&g_dtc_trace[i], t_now - t_prev);            \
    t_prev = t_now;                                                              \
  } while (0)
extern "C" int pcaa_lab_dtc_trace(unsigned long long* out16, int reset) {
  if (out16 != nullptr && hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_dtc_trace), sizeof(g_dtc_trace)) != hipSuccess) return 1;
  if (reset) {
    unsigned long long z[16] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_dtc_trace), z, sizeof(z)) != hipSuccess) return 1;
  }
  return 0;
}
#else
#define DTC_T0()
#define DTC_MARK(i)
#endif

namespace {

constexpr int ROWS = 32;   // rows (time steps) per workgroup, T <= ROWS

struct DtcFwdParams {
  const float* src;     // [B*T, cin]: block input (layer 1) or the previous layer's bias-free pre-BN output
  const float* scale;   // [cin] BatchNorm+ELU of the previous layer applied on load; null: src used as is
  const float* shift;
  const float* W;       // [cout, cin*3], k = ci*3 + tap
  float* y;             // [B*T, cout]
  float* col;           // [B*T, cin*3] (im2col of the activated input) or null
  double* stats;        // [nrep][2][cout] fp64 sums (sum, sum of squares) or null
  int B, T, cin, cout, dil, nrep;
  long slab_stride;     // gridDim.z > 1: split z writes its partial product to y + z*slab_stride
  BnTail tail;          // the BatchNorm finalize of ``stats``, run by the last workgroup (bn_tail.h); kind 0: none
  // windowed source (pcaa_dtc_conv_fwd_win): sequence b, step t reads row win_row[b] + t of a frame-feature table (modulo
  // ring_rows if > 0) instead of row b*T + t; null = the addressing above
  const int* win_row;
  long ring_rows;
  // segmented rings (pcaa_dtc_conv_fwd_seg): the table is rings of ring_rows rows back to back, win_row[b] is an absolute
  // row and the window wraps inside the ring it starts in; 0 = one ring from row 0
  int seg;
};

// the source rows of one sequence: step r reads row base + (row0 + r), wrapped inside the ring
struct DtcSrc {
  long base, row0;
};

// first source row of sequence b and the row of step r from it (ring: T <= ring_rows, so one conditional subtraction wraps)
__device__ __forceinline__ DtcSrc dtc_src_row0(const DtcFwdParams& p, int b) {
  if (p.win_row == nullptr) return DtcSrc{0, (long)b * p.T};
  const long r0 = p.win_row[b];
  if (p.seg) {
    const long base = (r0 / p.ring_rows) * p.ring_rows;
    return DtcSrc{base, r0 - base};
  }
  return DtcSrc{0, p.ring_rows > 0 ? r0 % p.ring_rows : r0};
}
__device__ __forceinline__ long dtc_src_row(const DtcFwdParams& p, const DtcSrc& s, int r) {
  const long row = s.row0 + r;
  return s.base + ((p.ring_rows > 0 && row >= p.ring_rows) ? row - p.ring_rows : row);
}

constexpr int CC = 32;              // input channels per chunk: 3*CC = 96-deep contraction per trip
constexpr int WP = 3 * CC + 4;      // weight tile pitch: 36*row mod 64 walks all 16 four-bank groups
constexpr int MAX_CR = 256;         // channels of the activated sequence tile one workgroup keeps in LDS
constexpr int ZROW = ROWS;          // index of the all-zero row of that tile

// ELU for the staging path.  Relative error <= 3e-7 over the whole range: a degree-6 Taylor polynomial
// where exp(z)-1 would cancel (|z| < 0.25, truncation z^7/5040), v_exp_f32 elsewhere (|result| >= 0.22).
__device__ __forceinline__ float elu_stage(float z) {
  if (z > 0.f) return z;
  const float poly = z * (1.f + z * (0.5f + z * (1.f / 6 + z * (1.f / 24 + z * (1.f / 120 + z * (1.f / 720))))));
  return z > -0.25f ? poly : __expf(z) - 1.f;
}

// im2col of the activated input for the backward's weight gradient: col[(b,t)][ci*3+tap] = a[t-(2-tap)*d][ci], from the
// sequence tile in the LDS.  Round 4: the column tiles of a sequence SHARE the write (each takes a slice of the 16-B quads;
// it used to be the first tile's job alone, one 4-B store per element: 5-16 us of the launch on one workgroup in 16), 16 B
// per lane.  (cr is a multiple of 4, so a row's 3*cr floats are whole quads; K*4 and cz0*12 bytes keep them 16-B aligned.)
__device__ __forceinline__ void write_col(float* col, int K, const float* a_lds, int AP, int T, int cr, int d, int tid) {
  const int run4 = (cr * 3) >> 2, total = T * run4;
  const int per = (total + (int)gridDim.y - 1) / (int)gridDim.y;
  const int q_end = min(total, ((int)blockIdx.y + 1) * per);
  int q = (int)blockIdx.y * per + tid;
  const int dr = 256 / run4, dc = 256 - dr * run4;
  int r = q / run4, c = q - r * run4;                     // (row, quad in row), advanced by increments
  for (; q < q_end; q += 256) {
    const int k4 = c << 2;
    f32x4 v;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int kk = k4 + m, ci = kk / 3, tap = kk - ci * 3;
      const int ts = r - (2 - tap) * d;
      v[m] = ts >= 0 ? a_lds[ts * AP + ci] : 0.f;
    }
    store4(col + (long)r * K + k4, v);
    r += dr;
    c += dc;
    if (c >= run4) { c -= run4; ++r; }
  }
}

// ------------------------------------------------------------------ the pieces every kernel of this file is built from
// A workgroup stages its sequence tile once, then walks the contraction in 96-deep chunks (CC channels x 3 taps): the
// chunk's weights go from HBM to registers (chunk_load), from there tap-major into an LDS tile of NT output columns
// (chunk_store), and meet the sequence tile on the matrix pipe (contract_chunk); the results leave through Emit and one
// of the statistics commits.  ADJ: the adjoint (rows offset forwards in time, weights read along their rows and scattered
// transposed).  BF: the bf16 throughput mode, v_mfma_f32_32x32x16_bf16 on operands rounded as the fragments are built
// (the sequence tile stays fp32 in the LDS, so the im2col matrix for the weight gradient is unchanged; the weight chunk is
// stored as bf16): a 96-deep chunk is 6 MFMAs of 32 cycles instead of 12 of 64.
constexpr int NCT = 128;            // output channels of a one-sequence bf16 workgroup
constexpr int WPH = 3 * CC + 8;     // bf16 pitch of a weight-tile row (208 B)

__device__ __forceinline__ bf16x8 cvt8(const float* p) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
  bf16x8 r;
  r[0] = (bf16_t)a.x; r[1] = (bf16_t)a.y; r[2] = (bf16_t)a.z; r[3] = (bf16_t)a.w;
  r[4] = (bf16_t)b.x; r[5] = (bf16_t)b.y; r[6] = (bf16_t)b.z; r[7] = (bf16_t)b.w;
  return r;
}

// BatchNorm + ELU of the layer before on one staged quad
__device__ __forceinline__ f32x4 activate4(f32x4 v, const f32x4& sc, const f32x4& sh) {
  v.x = elu_stage(fmaf(sc.x, v.x, sh.x));
  v.y = elu_stage(fmaf(sc.y, v.y, sh.y));
  v.z = elu_stage(fmaf(sc.z, v.z, sh.z));
  v.w = elu_stage(fmaf(sc.w, v.w, sh.w));
  return v;
}

// (dy = coef0*dz + coef1*y + coef2 stays spelled out in both adjoint staging loops: as a function of the quad the compiler
// contracts the other of its two products into the fused multiply-add in the pair kernel, and dy changes in the last bit)

// One chunk of weights into registers, NT * 24 / 256 quads per thread.  c0g: the chunk's first contraction channel, kend:
// the end of the workgroup's contraction range, wrow: floats per row of W, nc: output columns.
//   forward: NT columns x 96 contiguous floats W[n0 + c][c0g * 3 ...]: quad q -> (column c = q / 24, run offset f)
//   adjoint: 32 contraction rows x (NT * 3) contiguous floats W[c0g + co_l][n0 * 3 ...]
template <bool ADJ, int NT>
__device__ __forceinline__ void chunk_load(f32x4 (&rw)[NT * 24 / 256], const float* W, long wrow, int n0, int nc, int c0g,
                                           int kend, int tid) {
#pragma unroll
  for (int j = 0; j < NT * 24 / 256; ++j) {
    const int q = tid + j * 256;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!ADJ) {
      const int c = q / 24, f = (q - c * 24) << 2;
      if (n0 + c < nc && c0g * 3 + f < kend * 3) v = load4(W + (long)(n0 + c) * wrow + (long)(c0g * 3 + f));
    } else {
      constexpr int RUN4 = NT * 3 / 4;
      const int co_l = q / RUN4, f = (q - co_l * RUN4) << 2;
      if (c0g + co_l < kend && (long)n0 * 3 + f < wrow) v = load4(W + (long)(c0g + co_l) * wrow + (long)n0 * 3 + f);
    }
    rw[j] = v;
  }
}

// ... and from the registers tap-major into the weight tile: run element kk = channel * 3 + tap goes to
// row = output column, k' = tap * CC + contraction channel (fp32 rows of WP floats, bf16 rows of WPH halves)
template <bool ADJ, bool BF, int NT>
__device__ __forceinline__ void chunk_store(const f32x4 (&rw)[NT * 24 / 256], float* wtile, int tid) {
  bf16_t* wh = reinterpret_cast<bf16_t*>(wtile);
#pragma unroll
  for (int j = 0; j < NT * 24 / 256; ++j) {
    const int q = tid + j * 256;
    int row0, f;          // forward: row0 = the column, k' from f;  adjoint: row0 = contraction channel, column from f
    if (!ADJ) { row0 = q / 24; f = (q - row0 * 24) << 2; }
    else { constexpr int RUN4 = NT * 3 / 4; row0 = q / RUN4; f = (q - row0 * RUN4) << 2; }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int kk = f + m, a = kk / 3, tap = kk - a * 3;
      const int col = ADJ ? a : row0, kl = ADJ ? row0 : a;
      if (BF) wh[col * WPH + tap * CC + kl] = (bf16_t)rw[j][m];
      else wtile[col * WP + tap * CC + kl] = rw[j][m];
    }
  }
}

// The MFMAs of one chunk on a wave's 32 x 32 block: tile-local channels cl .. cl + 31 of the kr staged ones against column
// wcol of the weight tile, k-groups g0 .. g0 + NG - 1.  fp32: 12 groups of 8 per chunk (tap = g / 4), a lane's four
// consecutive k' feed four 32x32x2 MFMAs;  bf16: 6 steps of 16 (tap = g / 2), a lane's eight feed one 32x32x16.  The taps
// are row offsets of the A-fragment reads; a row outside the sequence, or a channel outside the range, reads the zero row.
template <bool ADJ, bool BF, int NG>
__device__ __forceinline__ void contract_chunk(f32x16& acc, const float* tile, int AP, const float* wtile, int wcol, int g0,
                                               int cl, int kr, int T, int d, int l31, int half) {
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int gg = g0 + g;
    const int tap = BF ? gg >> 1 : gg >> 2;
    const int kl = BF ? ((gg & 1) << 4) + (half << 3) : ((gg & 3) << 3) + (half << 2);
    const int rs = ADJ ? l31 + (2 - tap) * d : l31 - (2 - tap) * d;
    const bool ok = (ADJ ? rs < T : rs >= 0) && cl + kl < kr;
    const float* ap = ok ? &tile[rs * AP + cl + kl] : &tile[ZROW * AP];
    if (BF) {
      const bf16x8 av = cvt8(ap);
      const bf16x8 wv = *reinterpret_cast<const bf16x8*>(&reinterpret_cast<const bf16_t*>(wtile)[wcol * WPH + tap * CC + kl]);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, wv, acc, 0, 0, 0);
    } else {
      const f32x4 av = *reinterpret_cast<const f32x4*>(ap);
      const f32x4 wv = *reinterpret_cast<const f32x4*>(&wtile[wcol * WP + tap * CC + kl]);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, wv.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, wv.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, wv.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, wv.w, acc, 0, 0, 0);
    }
  }
}

// accumulator i of lane (l31, half) is row acc_row(i, half), column l31 of the wave's block
__device__ __forceinline__ constexpr int acc_row(int i, int half) { return (i & 3) + 8 * (i >> 2) + 4 * half; }

// Waves that split a chunk's k-groups combine their partial tiles through part[.][ROWS][33], which aliases the sequence
// tile: a barrier before the stores (the tile's readers are done) and one after
__device__ __forceinline__ void part_store(float* part, int w, const f32x16& acc, int l31, int half) {
#pragma unroll
  for (int i = 0; i < 16; ++i) part[(w * ROWS + acc_row(i, half)) * 33 + l31] = acc[i];
}
__device__ __forceinline__ float part_at(const float* part, int w, int r, int c) { return part[(w * ROWS + r) * 33 + c]; }

// One result leaves: the store and its two statistic terms (a thread calls it in ascending row order).
//   forward: y and {sum y, sum y^2}
//   adjoint: da, or with ``ep`` the first half of the BatchNorm+ELU backward of the layer below: dz = da * ELU'(z) and
//            {sum dz, sum dz * yhat}
template <bool ADJ>
struct Emit {
  float* out;           // [B*T, nc]
  int T, nc;
  bool ep;
  const float* ep_y;
  float esc = 0.f, esh = 0.f, emu = 0.f, ers = 0.f;
  float s1 = 0.f, s2 = 0.f;
  // the epilogue's per-column constants, for the one column gn this thread emits
  template <class P>
  __device__ __forceinline__ void column(const P& p, int gn) {
    if (ep && gn < nc) { esc = p.ep_scale[gn]; esh = p.ep_shift[gn]; emu = p.ep_mean[gn]; ers = p.ep_rstd[gn]; }
  }
  __device__ __forceinline__ void operator()(float v, int b, int r, int gn) {
    const long g = ((long)b * T + r) * nc + gn;
    if (!ADJ) {
      out[g] = v;
      s1 += v;
      s2 += v * v;
    } else {
      if (ep) {
        const float yb = ep_y[g];
        v *= elu_grad_from_pre(fmaf(yb, esc, esh));
        s1 += v;
        s2 += v * ((yb - emu) * ers);
      }
      out[g] = v;
    }
  }
};

// Statistics of a 32-column tile whose thread (row group tid >> 5, column tid & 31) holds the sums of its rows: the 8 row
// groups meet in red[2][8][32], 64 threads add them in fp64, ascending, and issue one atomic each into replica ``rep``
__device__ __forceinline__ void commit_stats_rows(float* red, float s1, float s2, int tid, double* stats, int rep, int nc, int n0) {
  red[(0 * 8 + (tid >> 5)) * 32 + (tid & 31)] = s1;
  red[(1 * 8 + (tid >> 5)) * 32 + (tid & 31)] = s2;
  __syncthreads();
  if (tid < 64) {
    const int stat = tid >> 5, c = tid & 31;
    if (n0 + c < nc) {
      double v = 0.0;
#pragma unroll
      for (int g = 0; g < 8; ++g) v += (double)red[(stat * 8 + g) * 32 + c];
      unsafeAtomicAdd(&stats[((long)rep * 2 + stat) * nc + n0 + c], v);
    }
  }
}

// Statistics of a wave that holds all rows of its 32 columns in registers: the two half-waves' sums meet by a shuffle and
// half 0 adds (``own``: this lane is in half 0 and its column gn exists)
__device__ __forceinline__ void commit_stats_wave(float s1, float s2, bool own, double* stats, int rep, int nc, int gn) {
  s1 += __shfl_xor(s1, 32, 64);
  s2 += __shfl_xor(s2, 32, 64);
  if (own) {
    unsafeAtomicAdd(&stats[((long)rep * 2 + 0) * nc + gn], (double)s1);
    unsafeAtomicAdd(&stats[((long)rep * 2 + 1) * nc + gn], (double)s2);
  }
}

// ------------------------------------------------------------------ one sequence per workgroup
// gridDim.z > 1 splits the contraction channels over workgroups in whole chunks (the 1024->16 layer: 64 workgroups walking
// K = 3072 was one long chain of load latencies): split z writes its partial product to its slab and
// pcaa_splitk_reduce_stats finishes the sum and the statistics.  This workgroup's range is [cz0, cz0 + cr).
struct ZRange { int cz0, cr; };
__device__ __forceinline__ ZRange split_range(int kc) {
  const int per_z = ((kc + CC - 1) / CC + (int)gridDim.z - 1) / (int)gridDim.z * CC;
  const int cz0 = blockIdx.z * per_z;
  return ZRange{cz0, max(0, min(kc, cz0 + per_z) - cz0)};
}

// what both staging loops leave behind the T staged rows of the tile (pitch AP = cr + 4)
template <bool BF>
__device__ __forceinline__ void stage_zero_rest(float* a_lds, int T, int cr, int AP, int tid) {
  if (BF) {
    // cvt8 reads 8 floats from a column that is a multiple of 8: with cr % 8 == 4 a row's last fragment takes in the
    // row's four pad floats, which meet zero weights -- and 0 x NaN is NaN on the matrix pipe: the pad is zeros
    for (int r = tid; r < T; r += 256) *reinterpret_cast<f32x4*>(&a_lds[r * AP + cr]) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int q = tid; q < (ROWS + 1 - T) * AP; q += 256) a_lds[T * AP + q] = 0.f;     // rows T..31 and the zero row
}

// the activated sequence tile of sequence b, once (coalesced 16-B loads, one ELU per element)
template <bool BF>
__device__ __forceinline__ void stage_one_fwd(const DtcFwdParams& p, float* a_lds, int b, int cz0, int cr, int AP, int tid) {
  const int T = p.T, q4 = cr >> 2;
  const bool act = p.scale != nullptr;
  const DtcSrc row0 = dtc_src_row0(p, b);
  for (int q = tid; q < T * q4; q += 256) {
    const int r = q / q4, c4 = (q - r * q4) << 2;
    f32x4 v = load4(p.src + dtc_src_row(p, row0, r) * p.cin + cz0 + c4);
    if (act) v = activate4(v, load4(p.scale + cz0 + c4), load4(p.shift + cz0 + c4));
    *reinterpret_cast<f32x4*>(&a_lds[r * AP + c4]) = v;
  }
  stage_zero_rest<BF>(a_lds, T, cr, AP, tid);
}

template <bool BF>
__global__ __launch_bounds__(256) void dtc_fwd_one_kernel(DtcFwdParams p) {
  // fp32: 32 output channels, the four waves split each chunk's k-groups on the same 32x32 tile and are combined through
  // the LDS.  bf16: 128 output channels, one 32-column block per wave, the whole contraction in that wave, no cross-wave
  // reduction -- a sequence's tile is staged and activated by 4 workgroups instead of 16 (256 -> 512 layer)
  constexpr int NT = BF ? NCT : 32;
  constexpr int TILE_FLOATS = (ROWS + 1) * (MAX_CR + 4), W_FLOATS = BF ? NCT * WPH / 2 : 32 * WP, RED_FLOATS = BF ? 0 : 2 * 8 * 32;
  __shared__ __attribute__((aligned(16))) float smem[TILE_FLOATS + W_FLOATS + RED_FLOATS + 1];
  static_assert(BF || 4 * ROWS * 33 <= TILE_FLOATS, "partial tiles alias the sequence tile");
  static_assert(TILE_FLOATS % 4 == 0, "the weight tile is 16-B aligned");
  float* a_lds = smem;                                 // [ROWS + 1][cr + 4]; fp32: later the 4 partial tiles
  float* Ws = smem + TILE_FLOATS;                      // fp32 [32][WP], bf16 [NCT][WPH]
  float* red = Ws + W_FLOATS;                          // fp32 only: [2][8][32]
  int* tail_flag = reinterpret_cast<int*>(red + RED_FLOATS);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  const int b = blockIdx.x, n0 = blockIdx.y * NT;
  const int T = p.T, cin = p.cin, K = cin * 3, d = p.dil;
  const bool split = gridDim.z > 1;
  const ZRange z = split_range(cin);
  const int cz0 = z.cz0, cr = z.cr, AP = cr + 4;

  DTC_T0();
  stage_one_fwd<BF>(p, a_lds, b, cz0, cr, AP, tid);
  const float* Wz = p.W + (long)cz0 * 3;               // this split's weights: W[.][cz0 * 3 ...]
  f32x4 rw[NT * 24 / 256];
  if (cr > 0) chunk_load<false, NT>(rw, Wz, K, n0, p.cout, 0, cr, tid);
  __syncthreads();
  DTC_MARK(0);      // staging
  if (p.col != nullptr) write_col(p.col + (long)b * T * K + (long)cz0 * 3, K, a_lds, AP, T, cr, d, tid);
  DTC_MARK(1);      // im2col
  const bool active = !BF || n0 + wave * 32 < p.cout;   // (wave-uniform) bf16: this wave's 32 columns exist
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int c0 = 0; c0 < cr; c0 += CC) {
    if (c0 > 0) __syncthreads();          // previous trip's readers are done with the weight tile
    chunk_store<false, BF, NT>(rw, Ws, tid);
    __syncthreads();
    if (c0 + CC < cr) chunk_load<false, NT>(rw, Wz, K, n0, p.cout, c0 + CC, cr, tid);    // in flight while this chunk is consumed
    if (active) contract_chunk<false, BF, BF ? 6 : 3>(acc, a_lds, AP, Ws, (BF ? wave * 32 : 0) + l31, BF ? 0 : wave * 3, c0, cr, T, d, l31, half);
  }
  DTC_MARK(2);      // contraction
  Emit<false> emit{p.y + (long)blockIdx.z * p.slab_stride, T, p.cout, false, nullptr};
  const bool want_stats = p.stats != nullptr && !split;
  if (!BF) {
    __syncthreads();                      // the sequence tile is dead by now
    part_store(a_lds, wave, acc, l31, half);
    __syncthreads();
    const int colx = tid & 31, rg = tid >> 5, gn = n0 + colx;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = rg + 8 * i;
      const float v = (part_at(a_lds, 0, r, colx) + part_at(a_lds, 1, r, colx)) + (part_at(a_lds, 2, r, colx) + part_at(a_lds, 3, r, colx));
      if (r < T && gn < p.cout) emit(v, b, r, gn);
    }
    DTC_MARK(3);    // combine + store
    if (want_stats) commit_stats_rows(red, emit.s1, emit.s2, tid, p.stats, b % p.nrep, p.cout, n0);
  } else {
    const int gn = n0 + wave * 32 + l31;
    if (active && gn < p.cout) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int r = acc_row(i, half);
        if (r < T) emit(acc[i], b, r, gn);
      }
    }
    DTC_MARK(3);    // store
    if (want_stats) commit_stats_wave(emit.s1, emit.s2, active && half == 0 && gn < p.cout, p.stats, b % p.nrep, p.cout, gn);
  }
  DTC_MARK(4);      // statistics
  bn_tail_run(p.tail, tid, 256, gridDim.x * gridDim.y * gridDim.z, tail_flag);
  DTC_MARK(5);      // tail
}

// ------------------------------------------------------------------ backward w.r.t. the layer input
//   da[(b,t)][ci] = sum_{co,tap} dy[b][t+(2-tap)*d][co] * W[co][ci][tap]        (rows past the sequence end: zero)
// The adjoint of the forward as the same kernel shape: the gradient sequence tile dy[T][cout range] is staged in
// LDS once, the taps are row offsets (now forwards in time) of the A-fragment reads, the contraction runs over
// (tap, co) in 32-channel chunks and the weight tile of a chunk is the same 96-float run per co as in the
// forward, scattered TRANSPOSED (row = input channel ci, k' = tap*32 + co).  Replaces a 128x128-tile GEMM on a
// handful of workgroups (dcol = dy . W) plus the col2im pass that summed its three taps.
struct DtcDgradParams {
  const float* dy;      // [B*T, cout], or null: dy = coef0*dz + coef1*y + coef2 is formed while the tile is staged
  const float* dz;      // [B*T, cout]  d(loss)/d(pre-activation z) of THIS layer      (dy == null)
  const float* y;       // [B*T, cout]  this layer's bias-free pre-BN output             (dy == null)
  const float* coef;    // [3][cout]    pcaa_bn_bwd_finalize's coefficients             (dy == null)
  float* dy_out;        // [B*T, cout] or null: the staged dy, written by the first column tile (for the wgrad)
  const float* W;       // [cout, cin*3]
  float* out;           // [B*T, cin]: da, or with the epilogue dz of the layer BELOW (gridDim.z > 1: slabs)
  // epilogue (layer below): out = da * ELU'(ep_y*ep_scale + ep_shift), statistics {sum dz, sum dz*yhat}
  const float* ep_y; const float* ep_scale; const float* ep_shift; const float* ep_mean; const float* ep_rstd;
  double* ep_stats; int nrep;
  int B, T, cin, cout, dil;
  long slab_stride;
  BnTail tail;          // the BatchNorm-backward finalize of ``ep_stats`` (bn_tail.h); kind 0: none
};

constexpr int DG_MAX_CR = 512;                       // contraction channels per workgroup (dynamic LDS)
constexpr int DG_PART_FLOATS = 4 * ROWS * 33;        // the four waves' partial tiles alias the sequence tile
static inline int dg_tile_floats(int cr) { const int a = (ROWS + 1) * (cr + 4); return a > DG_PART_FLOATS ? a : DG_PART_FLOATS; }

// the gradient sequence tile of sequence b, once: dy as given or formed on load; the first column tile keeps it for the wgrad
template <bool BF>
__device__ __forceinline__ void stage_one_adj(const DtcDgradParams& p, float* a_lds, int b, int cz0, int cr, int AP, int tid) {
  const int T = p.T, cout = p.cout, q4 = cr >> 2;
  const bool form = p.dy == nullptr;
  const bool keep = p.dy_out != nullptr && blockIdx.y == 0;
  for (int q = tid; q < T * q4; q += 256) {
    const int r = q / q4, c4 = (q - r * q4) << 2;
    const long g = ((long)b * T + r) * cout + cz0 + c4;
    f32x4 v;
    if (form) {
      const f32x4 k0 = load4(p.coef + cz0 + c4), k1 = load4(p.coef + cout + cz0 + c4),
                  k2 = load4(p.coef + 2 * cout + cz0 + c4);
      v = k0 * load4(p.dz + g) + k1 * load4(p.y + g) + k2;
    } else {
      v = load4(p.dy + g);
    }
    *reinterpret_cast<f32x4*>(&a_lds[r * AP + c4]) = v;
    if (keep) store4(p.dy_out + g, v);
  }
  stage_zero_rest<BF>(a_lds, T, cr, AP, tid);
}

// fp32: 32 input channels per workgroup, k-groups split over the waves;  bf16: 128, one 32-column block per wave
template <bool BF>
__global__ __launch_bounds__(256) void dtc_dgrad_one_kernel(DtcDgradParams p, int tile_floats) {
  extern __shared__ __attribute__((aligned(16))) float dg_smem[];
  constexpr int NT = BF ? NCT : 32;
  constexpr int W_FLOATS = BF ? NCT * WPH / 2 : 32 * WP, RED_FLOATS = BF ? 0 : 2 * 8 * 32;
  float* a_lds = dg_smem;                              // [ROWS + 1][cr + 4]; fp32: later the 4 partial tiles
  float* Ws = dg_smem + tile_floats;                   // fp32 [32][WP], bf16 [NCT][WPH]
  float* red = Ws + W_FLOATS;                          // fp32 only: [2][8][32]
  int* tail_flag = reinterpret_cast<int*>(red + RED_FLOATS);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  const int b = blockIdx.x, n0 = blockIdx.y * NT;      // n0: first input channel (output column)
  const int T = p.T, cin = p.cin, d = p.dil;
  const long wrow = (long)cin * 3;
  const ZRange z = split_range(p.cout);
  const int cz0 = z.cz0, cr = z.cr, AP = cr + 4;

  DTC_T0();
  stage_one_adj<BF>(p, a_lds, b, cz0, cr, AP, tid);
  const float* Wz = p.W + (long)cz0 * wrow;            // this split's weights: W[cz0 ...][.]
  f32x4 rw[NT * 24 / 256];
  if (cr > 0) chunk_load<true, NT>(rw, Wz, wrow, n0, cin, 0, cr, tid);
  __syncthreads();
  DTC_MARK(8);      // staging
  const bool active = !BF || n0 + wave * 32 < cin;      // (wave-uniform) bf16: this wave's 32 columns exist
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int c0 = 0; c0 < cr; c0 += CC) {
    if (c0 > 0) __syncthreads();
    chunk_store<true, BF, NT>(rw, Ws, tid);
    __syncthreads();
    if (c0 + CC < cr) chunk_load<true, NT>(rw, Wz, wrow, n0, cin, c0 + CC, cr, tid);
    if (active) contract_chunk<true, BF, BF ? 6 : 3>(acc, a_lds, AP, Ws, (BF ? wave * 32 : 0) + l31, BF ? 0 : wave * 3, c0, cr, T, d, l31, half);
  }
  DTC_MARK(9);      // contraction
  Emit<true> emit{p.out + (long)blockIdx.z * p.slab_stride, T, cin, p.ep_stats != nullptr, p.ep_y};
  if (!BF) {
    __syncthreads();
    part_store(a_lds, wave, acc, l31, half);
    __syncthreads();
    const int colx = tid & 31, rg = tid >> 5, gn = n0 + colx;
    emit.column(p, gn);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = rg + 8 * i;
      if (r < T && gn < cin)
        emit((part_at(a_lds, 0, r, colx) + part_at(a_lds, 1, r, colx)) + (part_at(a_lds, 2, r, colx) + part_at(a_lds, 3, r, colx)), b, r, gn);
    }
    DTC_MARK(10);   // combine + epilogue + store
    if (emit.ep) commit_stats_rows(red, emit.s1, emit.s2, tid, p.ep_stats, b % p.nrep, cin, n0);
  } else {
    const int gn = n0 + wave * 32 + l31;
    emit.column(p, gn);
    if (active && gn < cin) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int r = acc_row(i, half);
        if (r < T) emit(acc[i], b, r, gn);
      }
    }
    DTC_MARK(10);   // epilogue + store
    if (emit.ep) commit_stats_wave(emit.s1, emit.s2, active && half == 0 && gn < cin, p.ep_stats, b % p.nrep, cin, gn);
  }
  DTC_MARK(11);     // statistics
  bn_tail_run(p.tail, tid, 256, gridDim.x * gridDim.y * gridDim.z, tail_flag);
  DTC_MARK(12);     // tail
}

// ------------------------------------------------------------------ round 4: two sequences per workgroup (layers 5, 6)
// The per-phase trace of the kernels above (tools/dtc_lab.py --trace, profiles/r04_dtc_trace.txt) put 72 % of the
// 256 -> 512 layer's 42 us into the chunk loop -- 3.3 us per 96-deep chunk for 0.35 us of MFMA: every one of the
// 1 024 (sequence, 32-column) workgroups streams its own 96 KB weight slice through a CU that holds three or four of
// them, and stages the same 30 KB sequence tile as its 15 siblings.  Here a workgroup owns TWO sequences (64 rows) and
// NT output channels; a weight chunk is fetched once per pair (half the weight traffic, and with NT = 64 half the
// staging), requested TWO chunks ahead into registers and published through a double-buffered LDS tile (one barrier per
// chunk).  One body serves the forward and its adjoint (ADJ: anti-causal row offsets, dy formed on load, the
// BatchNorm+ELU backward's first half in the epilogue, weights read along their rows) and both matrix pipes
// (BF: v_mfma_f32_32x32x16_bf16 on operands rounded as the fragments are built, the throughput mode).
//   NT = 64: wave = (sequence, 32-column block), whole contraction in the wave, results leave from the registers;
//   NT = 32: wave = (sequence, half of each chunk's k-groups), two partial tiles combined through the LDS.
// Contraction channels beyond PAIR_KC are staged in further passes over the same LDS tile (the adjoint of layer 6).
struct DtcPairParams {
  const float* src;      // forward: [B*T, kc] block input / previous pre-BN output;  adjoint: dy or null
  const float* scale;    // forward: BatchNorm+ELU of the previous layer on load (null: as is)
  const float* shift;
  const float* dz; const float* y; const float* coef;   // adjoint with src == null: tile = coef0*dz + coef1*y + coef2
  float* keep;           // adjoint: the formed dy written out (by the first column tile) or null
  const float* W;        // [cout, cin*3], k = ci*3 + tap
  float* out;            // [B*T, nc]
  float* col;            // forward: im2col of the activated input or null
  double* stats; int nrep;
  const float* ep_y; const float* ep_scale; const float* ep_shift; const float* ep_mean; const float* ep_rstd;
  int B, T, kc, nc, dil; // kc: contraction channels, nc: output channels
  BnTail tail;
};

constexpr int PAIR_KC = 256;

template <bool ADJ, bool BF, int NT>
__global__ __launch_bounds__(256) void dtc_pair_kernel(DtcPairParams p, int tile_floats) {
  extern __shared__ __attribute__((aligned(16))) float pr_smem[];
  constexpr int WROW = BF ? WPH / 2 : WP;              // floats per weight-tile row (bf16 rows: 104 halves = 52 floats)
  constexpr int NJ = NT * 24 / 256;                    // float4 per thread and chunk: NT columns x 96 floats
  float* tile = pr_smem;                               // [2][ROWS + 1][AP]; NT = 32: later part[2][2][ROWS][33]
  float* Wsf = pr_smem + tile_floats;                  // [2][NT][WROW]
  float* red = Wsf + 2 * NT * WROW;                    // [2][8][32]
  int* flag = reinterpret_cast<int*>(red + 2 * 8 * 32);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  const int sq = wave >> 1, wsub = wave & 1;           // sequence of the pair; column block (NT = 64) or k-half (NT = 32)
  const int b0 = 2 * blockIdx.x, n0 = blockIdx.y * NT;
  const int T = p.T, kc = p.kc, nc = p.nc, d = p.dil;
  const int AP = min(kc, PAIR_KC) + 4;
  const long wrow = (long)(ADJ ? nc : kc) * 3;         // floats per row of W
  const int nch = (kc + CC - 1) / CC;
  float* tile_s = tile + sq * (ROWS + 1) * AP;
  DTC_T0();

  f32x4 rw0[NJ], rw1[NJ];
  auto load_w = [&](f32x4 (&rw)[NJ], int c0g) { chunk_load<ADJ, NT>(rw, p.W, wrow, n0, nc, c0g, kc, tid); };
  auto store_w = [&](const f32x4 (&rw)[NJ], int buf) { chunk_store<ADJ, BF, NT>(rw, Wsf + buf * NT * WROW, tid); };
  load_w(rw0, 0);
  if (nch > 1) load_w(rw1, CC);

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  auto contract = [&](int buf, int cl, int kr) {
    // NT = 64: the wave's column block, all of the chunk's k-groups;  NT = 32: half of them on the one block
    constexpr int NG = (BF ? 6 : 12) / (NT == 64 ? 1 : 2);
    contract_chunk<ADJ, BF, NG>(acc, tile_s, AP, Wsf + buf * NT * WROW, (NT == 64 ? wsub * 32 : 0) + l31,
                                NT == 64 ? 0 : wsub * NG, cl, kr, T, d, l31, half);
  };

  int c = 0;                                             // chunk index over the whole contraction
  for (int k0 = 0; k0 < kc; k0 += PAIR_KC) {
    const int kr = min(kc - k0, PAIR_KC);                // channels staged in this pass
    if (k0 > 0) __syncthreads();                         // the previous pass's readers are done with the tiles
    // ---- the two sequence tiles.  One workgroup per CU: nothing hides a load's latency but the loads themselves, so a
    // thread requests NB quads (adjoint: of dz and of y) before it transforms the first one
    {
      constexpr int NB = ADJ ? 8 : 16;                  // 16 loads in flight per thread either way: the whole pair in one round at 256 channels
      const int q4 = kr >> 2, R2 = 2 * T;
      // quad q = tid + 256 i of the pair's 2 T rows x q4 quads: (row, quad-in-row) advanced by increments -- the two
      // integer divisions per quad were a third of this phase (tools/dtc_lab.py --trace)
      const int dr = 256 / q4, dc = 256 - dr * q4;
      int R = tid / q4, cq = tid - R * q4;
      // the per-channel vectors of this thread's first quad: with q4 | 256 (every layer of the block) they serve all its
      // quads -- loaded per quad they sat, as dependent L2 round trips, in the middle of the transform loop (4 us of 11)
      const int cq0 = cq;
      f32x4 h0 = {1.f, 1.f, 1.f, 1.f}, h1 = {0.f, 0.f, 0.f, 0.f}, h2 = {0.f, 0.f, 0.f, 0.f};
      if (R < R2) {
        if (!ADJ) {
          if (p.scale != nullptr) { h0 = load4(p.scale + k0 + (cq0 << 2)); h1 = load4(p.shift + k0 + (cq0 << 2)); }
        } else if (p.src == nullptr) {
          h0 = load4(p.coef + k0 + (cq0 << 2));
          h1 = load4(p.coef + kc + k0 + (cq0 << 2));
          h2 = load4(p.coef + 2 * kc + k0 + (cq0 << 2));
        }
      }
      while (R < R2) {
        f32x4 v[NB], w[NB];
        int Rj[NB], cj[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          Rj[j] = R;
          cj[j] = cq;
          const int s = R >= T ? 1 : 0, r = R - s * T, c4 = cq << 2;
          v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
          w[j] = v[j];
          if (R < R2 && b0 + s < p.B) {
            const long g = ((long)(b0 + s) * T + r) * kc + k0 + c4;
            if (ADJ && p.src == nullptr) {
              v[j] = load4(p.dz + g);
              w[j] = load4(p.y + g);
            } else {
              v[j] = load4(p.src + g);
            }
          }
          R += dr;
          cq += dc;
          if (cq >= q4) { cq -= q4; ++R; }
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const int s = Rj[j] >= T ? 1 : 0, r = Rj[j] - s * T, c4 = cj[j] << 2;
          if (Rj[j] < R2) {
            f32x4 x = v[j];
            if (b0 + s < p.B) {
              const long g = ((long)(b0 + s) * T + r) * kc + k0 + c4;
              if (!ADJ) {
                if (p.scale != nullptr) {
                  f32x4 sc = h0, sh = h1;
                  if (cj[j] != cq0) { sc = load4(p.scale + k0 + c4); sh = load4(p.shift + k0 + c4); }
                  x = activate4(x, sc, sh);
                }
              } else {
                if (p.src == nullptr) {
                  f32x4 c0v = h0, c1v = h1, c2v = h2;
                  if (cj[j] != cq0) { c0v = load4(p.coef + k0 + c4); c1v = load4(p.coef + kc + k0 + c4); c2v = load4(p.coef + 2 * kc + k0 + c4); }
                  x = c0v * x + c1v * w[j] + c2v;
                }
                if (p.keep != nullptr && blockIdx.y == 0) store4(p.keep + g, x);
              }
            }
            *reinterpret_cast<f32x4*>(&tile[s * (ROWS + 1) * AP + r * AP + c4]) = x;      // B odd: the missing sequence is zeros
          }
        }
      }
      for (int q = tid; q < 2 * (ROWS + 1 - T) * AP; q += 256) {                           // rows T..31 and the zero row, both tiles
        const int s = q >= (ROWS + 1 - T) * AP ? 1 : 0;
        tile[s * (ROWS + 1) * AP + T * AP + (q - s * (ROWS + 1 - T) * AP)] = 0.f;
      }
    }
    __syncthreads();
    DTC_MARK(0);      // staging
    if (!ADJ && p.col != nullptr) {
      for (int s = 0; s < 2; ++s)
        if (b0 + s < p.B)
          write_col(p.col + (long)(b0 + s) * T * (kc * 3) + (long)k0 * 3, kc * 3, tile + s * (ROWS + 1) * AP, AP, T, kr, d, tid);
    }
    DTC_MARK(1);      // im2col
    for (int cl = 0; cl < kr; cl += 2 * CC) {
      store_w(rw0, 0);
      __syncthreads();
      if (c + 2 < nch) load_w(rw0, (c + 2) * CC);
      contract(0, cl, kr);
      ++c;
      if (cl + CC < kr) {
        store_w(rw1, 1);
        __syncthreads();
        if (c + 2 < nch) load_w(rw1, (c + 2) * CC);
        contract(1, cl + CC, kr);
        ++c;
      }
    }
    DTC_MARK(2);      // contraction
  }

  // ---- results.  accumulator i of lane (l31, half) is row (i & 3) + 8 (i >> 2) + 4 half, column l31 of the wave's block
  Emit<ADJ> emit{p.out, T, nc, ADJ && p.stats != nullptr, p.ep_y};
  const bool want_stats = p.stats != nullptr;
  if (NT == 64) {
    const int gn = n0 + wsub * 32 + l31, b = b0 + sq;
    emit.column(p, gn);
    if (gn < nc && b < p.B) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int r = acc_row(i, half);
        if (r < T) emit(acc[i], b, r, gn);
      }
    }
    DTC_MARK(3);      // store
    if (want_stats) {
      // the two sequences of a column block meet in ``red`` before the one atomic
      const float s1 = emit.s1 + __shfl_xor(emit.s1, 32, 64);
      const float s2 = emit.s2 + __shfl_xor(emit.s2, 32, 64);
      if (half == 0) {
        red[(0 * 8 + wave) * 32 + l31] = s1;
        red[(1 * 8 + wave) * 32 + l31] = s2;
      }
      __syncthreads();
      if (tid < 128) {
        const int stat = tid >> 6, cc = tid & 63, cb = cc >> 5;
        if (n0 + cc < nc) {
          const double v = (double)red[(stat * 8 + cb) * 32 + (cc & 31)] + (double)red[(stat * 8 + 2 + cb) * 32 + (cc & 31)];
          unsafeAtomicAdd(&p.stats[((long)(blockIdx.x % p.nrep) * 2 + stat) * nc + n0 + cc], v);
        }
      }
    }
  } else {
    __syncthreads();                                     // the sequence tiles are dead
    float* part = tile;                                  // [2][2][ROWS][33]
    part_store(part, sq * 2 + wsub, acc, l31, half);
    __syncthreads();
    const int colx = tid & 31, rg = tid >> 5, gn = n0 + colx;
    emit.column(p, gn);
    if (gn < nc) {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = rg + 8 * i;
          if (r < T && b0 + s < p.B) emit(part_at(part, s * 2 + 0, r, colx) + part_at(part, s * 2 + 1, r, colx), b0 + s, r, gn);
        }
    }
    DTC_MARK(3);      // combine + store
    if (want_stats) commit_stats_rows(red, emit.s1, emit.s2, tid, p.stats, blockIdx.x % p.nrep, nc, n0);
  }
  DTC_MARK(4);        // statistics
  bn_tail_run(p.tail, tid, 256, gridDim.x * gridDim.y, flag);
  DTC_MARK(5);
}

static inline int pair_tile_floats(int kc) {
  const int a = 2 * (ROWS + 1) * ((kc < PAIR_KC ? kc : PAIR_KC) + 4), part = 2 * 2 * ROWS * 33;
  return a > part ? a : part;
}

// the pair kernels take the wide layers: at least four chunks of contraction, whole chunks, at least 64 output channels
static inline bool pair_takes(int kc, int nc, int ksplit, bool adj) {
  // PCAA_DTC_PAIR: 0 = off, fwd / adj = that direction only (lab), anything else = both
  static const int which = [] {
    const char* e = getenv("PCAA_DTC_PAIR");
    if (e == nullptr) return 3;
    if (e[0] == '0') return 0;
    if (e[0] == 'f') return 1;
    if (e[0] == 'a') return 2;
    return 3;
  }();
  return (which & (adj ? 2 : 1)) != 0 && ksplit == 1 && kc >= 128 && kc % CC == 0 && nc >= 64 && nc % 4 == 0;
}

// Launch KERN(p, tile) with ``lds`` bytes of dynamic LDS, more than the default limit allows: the limit is raised once per
// kernel, to ``cap`` (the most any launch of it asks for).  If that fails the launch did not happen: the BatchNorm tail
// taken for it is re-armed and the error is ``who``'s.
template <auto KERN, class Params>
static int launch_dyn_lds(size_t cap, dim3 grid, size_t lds, hipStream_t s, const Params& p, int tile, const char* who) {
  static bool configured = false;
  if (!configured) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)cap) != hipSuccess) {
      pcaa_rearm_bn_tail(p.tail);
      pcaa_set_error("%s: cannot raise the dynamic LDS limit", who);
      return PCAA_ERR_LAUNCH;
    }
    configured = true;
  }
  hipLaunchKernelGGL(KERN, grid, dim3(256), lds, s, p, tile);
  PCAA_RETURN_LAUNCH_STATUS(who);
}

template <bool ADJ, bool BF, int NT>
static int launch_pair(const DtcPairParams& p, hipStream_t s, const char* who) {
  constexpr int REST = 2 * NT * (BF ? WPH / 2 : WP) + 2 * 8 * 32 + 4;      // two weight tiles, red, the finalize flag
  const int tile = pair_tile_floats(p.kc);
  return launch_dyn_lds<dtc_pair_kernel<ADJ, BF, NT>>((size_t)(pair_tile_floats(PAIR_KC) + REST) * sizeof(float),
                                                      dim3((p.B + 1) / 2, (p.nc + NT - 1) / NT),
                                                      (size_t)(tile + REST) * sizeof(float), s, p, tile, who);
}

// 64-column workgroups when they still fill the chip (the 256 -> 512 layer's forward: 32 pairs x 8), else 32
static inline bool pair_wide(int B, int nc) { return (long)((B + 1) / 2) * (nc / 64) >= 192 && nc % 64 == 0; }

// the kernel a call takes (PCAA_DTC_ROUTE_*): the one decision both entry points launch by and pcaa_dtc_conv_route reports.
// A windowed source always takes the one-sequence kernels (the block's first layer, 1024 -> 16, is theirs anyway)
static inline int dtc_route(bool adj, bool bf16, int B, int cin, int cout, int ksplit, bool windowed) {
  const int kc = adj ? cout : cin, nc = adj ? cin : cout;
  int family = 0;
  if (!windowed && pair_takes(kc, nc, ksplit, adj)) family = pair_wide(B, nc) ? 2 : 1;
  return family * 2 + (bf16 ? 1 : 0);
}

template <bool ADJ>
static int launch_pair_route(const DtcPairParams& p, int route, hipStream_t s, const char* who) {
  switch (route) {
    case PCAA_DTC_ROUTE_PAIR64_BF16: return launch_pair<ADJ, true, 64>(p, s, who);
    case PCAA_DTC_ROUTE_PAIR64_F32: return launch_pair<ADJ, false, 64>(p, s, who);
    case PCAA_DTC_ROUTE_PAIR32_BF16: return launch_pair<ADJ, true, 32>(p, s, who);
    default: return launch_pair<ADJ, false, 32>(p, s, who);
  }
}

}  // namespace

extern "C" int pcaa_dtc_conv_route(int adjoint, int bf16, int B, int cin, int cout, int ksplit, int windowed) {
  return dtc_route(adjoint != 0, bf16 != 0, B, cin, cout, ksplit, windowed != 0);
}

extern "C" int pcaa_dtc_conv_supported(int T, int cin, int cout) {
  return (T >= 1 && T <= ROWS && cin >= 4 && cin % 4 == 0 && cout >= 16 && cout % 16 == 0) ? 1 : 0;
}

/* smallest / recommended split of the input channels over workgroups: a workgroup keeps at most MAX_CR
 * channels of its sequence in LDS; few workgroups with a long contraction are cut further */
extern "C" int pcaa_dtc_conv_ksplit(int B, int cin, int cout) {
  const int chunks = (cin + CC - 1) / CC;
  int ks = (cin + MAX_CR - 1) / MAX_CR;
  if ((long)B * ((cout + 31) / 32) <= 128 && chunks >= 16) ks = ks > 8 ? ks : 8;
  return ks < chunks ? ks : chunks;
}

static int dtc_conv_fwd_impl(bool bf16, const float* src, const float* scale, const float* shift, const float* W, float* y,
                             float* col, double* stats, int nrep, int B, int T, int cin, int cout, int dilation,
                             int ksplit, long slab_stride, void* stream, const int* win_row = nullptr,
                             long ring_rows = 0, int seg = 0) {
  PCAA_CHECK_ARG(src && W && y && B >= 1 && dilation >= 1 && ksplit >= 1, "pcaa_dtc_conv_fwd: bad args");
  PCAA_CHECK_ARG(pcaa_dtc_conv_supported(T, cin, cout), "pcaa_dtc_conv_fwd: needs T <= %d, cin %% 4 == 0, cout %% 16 == 0",
                 ROWS);
  PCAA_CHECK_ARG((scale == nullptr) == (shift == nullptr), "pcaa_dtc_conv_fwd: scale and shift go together");
  PCAA_CHECK_ARG(stats == nullptr || nrep >= 1, "pcaa_dtc_conv_fwd: nrep");
  PCAA_CHECK_ARG(((uintptr_t)W % 16) == 0 && ((uintptr_t)src % 16) == 0 && (scale == nullptr || (((uintptr_t)scale % 16) == 0 &&
                 ((uintptr_t)shift % 16) == 0)), "pcaa_dtc_conv_fwd: src, W, scale, shift must be 16-B aligned");
  const int chunks = (cin + CC - 1) / CC;
  const int per_z = (chunks + ksplit - 1) / ksplit * CC;
  // (the two-sequence kernels stage their contraction channels in passes of PAIR_KC: the limit is the one-sequence kernels')
  const int route = dtc_route(false, bf16, B, cin, cout, ksplit, win_row != nullptr);
  PCAA_CHECK_ARG(ksplit <= chunks && (route >= PCAA_DTC_ROUTE_PAIR32_F32 || per_z <= MAX_CR),
                 "pcaa_dtc_conv_fwd: ksplit must keep <= %d channels per workgroup (pcaa_dtc_conv_ksplit)", MAX_CR);
  PCAA_CHECK_ARG(ksplit == 1 || (stats == nullptr && slab_stride >= (long)B * T * cout),
                 "pcaa_dtc_conv_fwd: ksplit > 1 writes slabs (no statistics): slab_stride >= B*T*cout");
  if (route >= PCAA_DTC_ROUTE_PAIR32_F32) {
    DtcPairParams pp{src, scale, shift, nullptr, nullptr, nullptr, nullptr, W, y, col, stats, nrep,
                     nullptr, nullptr, nullptr, nullptr, nullptr, B, T, cin, cout, dilation,
                     stats != nullptr ? pcaa_take_bn_tail(stats) : BnTail{}};
    return launch_pair_route<false>(pp, route, as_stream(stream), "pcaa_dtc_conv_fwd");
  }
  DtcFwdParams p{src, scale, shift, W, y, col, stats, B, T, cin, cout, dilation, nrep, ksplit > 1 ? slab_stride : 0,
                 (stats != nullptr && ksplit == 1) ? pcaa_take_bn_tail(stats) : BnTail{}, win_row, ring_rows, seg};
  if (route == PCAA_DTC_ROUTE_ONE_BF16) hipLaunchKernelGGL(dtc_fwd_one_kernel<true>, dim3(B, (cout + NCT - 1) / NCT, ksplit), dim3(256), 0, as_stream(stream), p);
  else hipLaunchKernelGGL(dtc_fwd_one_kernel<false>, dim3(B, (cout + 31) / 32, ksplit), dim3(256), 0, as_stream(stream), p);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_dtc_conv_fwd");
}
extern "C" int pcaa_dtc_conv_fwd(const float* src, const float* scale, const float* shift, const float* W, float* y,
                                 float* col, double* stats, int nrep, int B, int T, int cin, int cout, int dilation,
                                 int ksplit, long slab_stride, void* stream) {
  return dtc_conv_fwd_impl(false, src, scale, shift, W, y, col, stats, nrep, B, T, cin, cout, dilation, ksplit, slab_stride, stream);
}
extern "C" int pcaa_dtc_conv_fwd_bf16(const float* src, const float* scale, const float* shift, const float* W, float* y,
                                      float* col, double* stats, int nrep, int B, int T, int cin, int cout, int dilation,
                                      int ksplit, long slab_stride, void* stream) {
  return dtc_conv_fwd_impl(true, src, scale, shift, W, y, col, stats, nrep, B, T, cin, cout, dilation, ksplit, slab_stride, stream);
}


// The eval form (col and stats null) on a windowed source: see include/pcaa_hip.h.  The range of win_row is the caller's to
// check (on the host copy of the plan it came from); here only what the host can see.
static int dtc_conv_fwd_win_impl(bool bf16, const float* table, const float* scale, const float* shift, const float* W,
                                 float* y, float* col, double* stats, int nrep, int B, int T, int cin, int cout,
                                 int dilation, int ksplit, long slab_stride, const int* win_row, long table_rows,
                                 long ring_rows, void* stream) {
  PCAA_CHECK_ARG(col == nullptr && stats == nullptr, "pcaa_dtc_conv_fwd_win: eval form only (col and stats null)");
  PCAA_CHECK_ARG(win_row != nullptr && table_rows >= T && ring_rows >= 0 && ring_rows <= table_rows &&
                 (ring_rows == 0 || ring_rows >= T),
                 "pcaa_dtc_conv_fwd_win: needs win_row, T <= table_rows, ring_rows 0 or in [T, table_rows]");
  return dtc_conv_fwd_impl(bf16, table, scale, shift, W, y, nullptr, nullptr, nrep, B, T, cin, cout, dilation, ksplit,
                           slab_stride, stream, win_row, ring_rows);
}
extern "C" int pcaa_dtc_conv_fwd_win(const float* table, const float* scale, const float* shift, const float* W, float* y,
                                     float* col, double* stats, int nrep, int B, int T, int cin, int cout, int dilation,
                                     int ksplit, long slab_stride, const int* win_row, long table_rows, long ring_rows,
                                     void* stream) {
  return dtc_conv_fwd_win_impl(false, table, scale, shift, W, y, col, stats, nrep, B, T, cin, cout, dilation, ksplit,
                               slab_stride, win_row, table_rows, ring_rows, stream);
}
extern "C" int pcaa_dtc_conv_fwd_win_bf16(const float* table, const float* scale, const float* shift, const float* W,
                                          float* y, float* col, double* stats, int nrep, int B, int T, int cin, int cout,
                                          int dilation, int ksplit, long slab_stride, const int* win_row,
                                          long table_rows, long ring_rows, void* stream) {
  return dtc_conv_fwd_win_impl(true, table, scale, shift, W, y, col, stats, nrep, B, T, cin, cout, dilation, ksplit,
                               slab_stride, win_row, table_rows, ring_rows, stream);
}

// Segmented rings: n_seg rings of ring_rows rows back to back, win_row[b] an absolute table row (include/pcaa_hip.h).
static int dtc_conv_fwd_seg_impl(bool bf16, const float* table, const float* scale, const float* shift, const float* W,
                                 float* y, int B, int T, int cin, int cout, int dilation, int ksplit, long slab_stride,
                                 const int* win_row, long n_seg, long ring_rows, void* stream) {
  PCAA_CHECK_ARG(win_row != nullptr && n_seg >= 1 && ring_rows >= T && T >= 1,
                 "pcaa_dtc_conv_fwd_seg: needs win_row, n_seg >= 1, ring_rows >= T");
  return dtc_conv_fwd_impl(bf16, table, scale, shift, W, y, nullptr, nullptr, 1, B, T, cin, cout, dilation, ksplit,
                           slab_stride, stream, win_row, ring_rows, 1);
}
extern "C" int pcaa_dtc_conv_fwd_seg(const float* table, const float* scale, const float* shift, const float* W, float* y,
                                     int B, int T, int cin, int cout, int dilation, int ksplit, long slab_stride,
                                     const int* win_row, long n_seg, long ring_rows, void* stream) {
  return dtc_conv_fwd_seg_impl(false, table, scale, shift, W, y, B, T, cin, cout, dilation, ksplit, slab_stride, win_row,
                               n_seg, ring_rows, stream);
}
extern "C" int pcaa_dtc_conv_fwd_seg_bf16(const float* table, const float* scale, const float* shift, const float* W,
                                          float* y, int B, int T, int cin, int cout, int dilation, int ksplit,
                                          long slab_stride, const int* win_row, long n_seg, long ring_rows, void* stream) {
  return dtc_conv_fwd_seg_impl(true, table, scale, shift, W, y, B, T, cin, cout, dilation, ksplit, slab_stride, win_row,
                               n_seg, ring_rows, stream);
}

/* channel split for the dgrad (its contraction runs over the OUTPUT channels of the convolution; a workgroup
 * keeps up to 512 of them in LDS) */
extern "C" int pcaa_dtc_conv_dgrad_ksplit(int B, int cin, int cout) {
  (void)B; (void)cin;
  const int ks = (cout + DG_MAX_CR - 1) / DG_MAX_CR;
  return ks < 1 ? 1 : ks;
}

static int dtc_conv_dgrad_impl(bool bf16, const float* dy, const float* dz, const float* y, const float* coef, float* dy_out,
                               const float* W, float* out, const float* ep_y, const float* ep_scale,
                               const float* ep_shift, const float* ep_mean, const float* ep_rstd,
                               double* ep_stats, int nrep, int B, int T, int cin, int cout, int dilation,
                               int ksplit, long slab_stride, void* stream) {
  PCAA_CHECK_ARG(W && out && B >= 1 && dilation >= 1 && ksplit >= 1, "pcaa_dtc_conv_dgrad: bad args");
  PCAA_CHECK_ARG((dy != nullptr) != (dz != nullptr && y != nullptr && coef != nullptr),
                 "pcaa_dtc_conv_dgrad: either dy, or dz + y + coef");
  PCAA_CHECK_ARG(T >= 1 && T <= ROWS && cin >= 4 && cin % 4 == 0 && cout >= 4 && cout % 4 == 0,
                 "pcaa_dtc_conv_dgrad: needs T <= %d, cin %% 4 == 0, cout %% 4 == 0", ROWS);
  PCAA_CHECK_ARG(((uintptr_t)W % 16) == 0 && (!dy || ((uintptr_t)dy % 16) == 0) && (!dz || (((uintptr_t)dz % 16) == 0 &&
                 ((uintptr_t)y % 16) == 0 && ((uintptr_t)coef % 16) == 0)) && (!dy_out || ((uintptr_t)dy_out % 16) == 0),
                 "pcaa_dtc_conv_dgrad: 16-B alignment");
  const int chunks = (cout + CC - 1) / CC;
  const int per_z = (chunks + ksplit - 1) / ksplit * CC;
  const int route = dtc_route(true, bf16, B, cin, cout, ksplit, false);
  PCAA_CHECK_ARG(ksplit <= chunks && (route >= PCAA_DTC_ROUTE_PAIR32_F32 || per_z <= DG_MAX_CR),
                 "pcaa_dtc_conv_dgrad: ksplit must keep <= %d channels per workgroup (pcaa_dtc_conv_dgrad_ksplit)", DG_MAX_CR);
  PCAA_CHECK_ARG(ksplit == 1 || slab_stride >= (long)B * T * cin, "pcaa_dtc_conv_dgrad: slab_stride >= B*T*cin");
  const bool ep = ep_stats != nullptr;
  PCAA_CHECK_ARG(!ep || (ksplit == 1 && ep_y && ep_scale && ep_shift && ep_mean && ep_rstd && nrep >= 1),
                 "pcaa_dtc_conv_dgrad: the epilogue needs ksplit == 1 and ep_y, ep_scale, ep_shift, ep_mean, ep_rstd");
  if (route >= PCAA_DTC_ROUTE_PAIR32_F32) {
    DtcPairParams pp{dy, nullptr, nullptr, dz, y, coef, dy_out, W, out, nullptr, ep_stats, nrep,
                     ep_y, ep_scale, ep_shift, ep_mean, ep_rstd, B, T, cout, cin, dilation,
                     ep ? pcaa_take_bn_tail(ep_stats) : BnTail{}};
    return launch_pair_route<true>(pp, route, as_stream(stream), "pcaa_dtc_conv_dgrad");
  }
  const int tile = dg_tile_floats(per_z);
  DtcDgradParams p{dy, dz, y, coef, dy_out, W, out, ep_y, ep_scale, ep_shift, ep_mean, ep_rstd, ep_stats, nrep,
                   B, T, cin, cout, dilation, ksplit > 1 ? slab_stride : 0,
                   ep ? pcaa_take_bn_tail(ep_stats) : BnTail{}};
  // behind the sequence tile: the weight tile, (fp32) red, the finalize flag
  const int rest = (route == PCAA_DTC_ROUTE_ONE_BF16 ? NCT * WPH / 2 : 32 * WP + 2 * 8 * 32) + 4;
  const size_t lds = (size_t)(tile + rest) * sizeof(float), cap = (size_t)(dg_tile_floats(DG_MAX_CR) + rest) * sizeof(float);
  if (route == PCAA_DTC_ROUTE_ONE_BF16)
    return launch_dyn_lds<dtc_dgrad_one_kernel<true>>(cap, dim3(B, (cin + NCT - 1) / NCT, ksplit), lds, as_stream(stream), p, tile,
                                                      "pcaa_dtc_conv_dgrad_bf16");
  return launch_dyn_lds<dtc_dgrad_one_kernel<false>>(cap, dim3(B, (cin + 31) / 32, ksplit), lds, as_stream(stream), p, tile,
                                                     "pcaa_dtc_conv_dgrad");
}
extern "C" int pcaa_dtc_conv_dgrad(const float* dy, const float* dz, const float* y, const float* coef, float* dy_out,
                                   const float* W, float* out, const float* ep_y, const float* ep_scale,
                                   const float* ep_shift, const float* ep_mean, const float* ep_rstd,
                                   double* ep_stats, int nrep, int B, int T, int cin, int cout, int dilation,
                                   int ksplit, long slab_stride, void* stream) {
  return dtc_conv_dgrad_impl(false, dy, dz, y, coef, dy_out, W, out, ep_y, ep_scale, ep_shift, ep_mean, ep_rstd, ep_stats, nrep,
                             B, T, cin, cout, dilation, ksplit, slab_stride, stream);
}
extern "C" int pcaa_dtc_conv_dgrad_bf16(const float* dy, const float* dz, const float* y, const float* coef, float* dy_out,
                                        const float* W, float* out, const float* ep_y, const float* ep_scale,
                                        const float* ep_shift, const float* ep_mean, const float* ep_rstd,
                                        double* ep_stats, int nrep, int B, int T, int cin, int cout, int dilation,
                                        int ksplit, long slab_stride, void* stream) {
  return dtc_conv_dgrad_impl(true, dy, dz, y, coef, dy_out, W, out, ep_y, ep_scale, ep_shift, ep_mean, ep_rstd, ep_stats, nrep,
                             B, T, cin, cout, dilation, ksplit, slab_stride, stream);
}
