// The distinct rows of PADDED frames, on the device (pcaa_frames_unique_offsets, pcaa_frames_unique): the front of the
// padding-free eval PointNet for frames whose padding is already written out -- the stored crops of the test / unseen
// splits and processed tracks [F, N, C].  process_track appends arr[choice(card, N - card)] and centres and casts every
// copy identically, so the repeated points are bit-equal rows of the same frame.  raw_frames.hip builds the same compact
// table from the picks; here there are no picks, only the rows.
//
// Two rows are the same point iff all their C 32-bit words are equal AS BITS (-0.0 != +0.0, NaNs are equal iff their
// payloads are): the per-point network is a function of the bits, so merging on bits is always safe.
//
// One workgroup of 256 threads per frame, the frame's N * C <= 5 120 words staged in LDS (16-byte loads for C == 4 on a
// 16-byte-aligned base, 4-byte loads otherwise).  Thread t owns rows t, t + 256, ... (one row for N <= 256, the sizes the
// project's configurations use; up to four above) in registers and walks ALL rows q = 0 .. N - 1 of the frame: every lane
// reads the same LDS words (a broadcast), compares them with its own rows as integers, and keeps "no equal row before
// mine" (first occurrence) and "equal rows" (multiplicity).  N C broadcast reads per thread, N^2 C / 256 compares: integer
// only, no atomics, no order to depend on.  The ranks of the first occurrences come from a wave-shuffle scan plus the wave
// totals in LDS, block of 256 rows after block with a carry, so the distinct rows leave in order of first occurrence.
//
// The search runs TWICE: pcaa_frames_unique_offsets counts (then one workgroup scans the counts in place with a running
// carry, as raw_unique_offsets_kernel does), pcaa_frames_unique searches again and writes.  The alternative, an int32
// [n, N] rank scratch left by the count pass, trades the second search for n N words written and read back; DESIGN.md has
// the measurement behind the choice.
#include "common.h"

namespace {

constexpr int FU_THREADS = 256;
constexpr int FU_WAVES = FU_THREADS / 64;
constexpr int FU_MAX_COLS = 5;
constexpr int FU_SCAN_THREADS = 1024;

// the frame's words -> LDS; NC = N * C <= PCAA_RAW_MAX_POINTS * FU_MAX_COLS (checked by the entry points)
template <int C>
__device__ __forceinline__ void stage_frame(uint32_t* s_w, const float* __restrict__ frame, int NC, bool vec) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(frame);
  if (C == 4 && vec) {
    for (int e = threadIdx.x * 4; e < NC; e += FU_THREADS * 4)
      *reinterpret_cast<uint4*>(s_w + e) = *reinterpret_cast<const uint4*>(src + e);
  } else {
    for (int e = threadIdx.x; e < NC; e += FU_THREADS) s_w[e] = src[e];
  }
  __syncthreads();
}

// For the rows p_k = tid + 256 k, k < PER, of the staged frame: first[k] = p_k < N and no row before p_k has its bits;
// mult[k] = rows of the frame with its bits (COUNT only).  Every lane reads row q: one LDS address per word.
template <int C, int PER, bool COUNT>
__device__ __forceinline__ void search_rows(const uint32_t* s_w, int N, bool (&first)[PER], int (&mult)[PER]) {
  uint32_t mine[PER][C], dup[PER];                // dup: an equal row stands before mine (flags as integers: no branch)
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int p = threadIdx.x + k * FU_THREADS;
    const int pc = p < N ? p : 0;                 // a thread without a row compares row 0 and reports nothing
#pragma unroll
    for (int c = 0; c < C; ++c) mine[k][c] = s_w[pc * C + c];
    first[k] = false;
    dup[k] = 0;
    mult[k] = 0;
  }
  if ((int)(threadIdx.x & ~63u) >= N) return;     // a wave without rows (N <= 192) has nothing to search: wave-uniform
#pragma unroll 8                                  // eight rows' LDS reads in flight: the loop is bound by their latency
  for (int q = 0; q < N; ++q) {
    uint32_t w[C];
#pragma unroll
    for (int c = 0; c < C; ++c) w[c] = s_w[q * C + c];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      uint32_t diff = 0;
#pragma unroll
      for (int c = 0; c < C; ++c) diff |= mine[k][c] ^ w[c];
      const uint32_t eq = diff == 0 ? 1u : 0u;
      dup[k] |= eq & (q < (int)threadIdx.x + k * FU_THREADS ? 1u : 0u);
      if (COUNT) mult[k] += (int)eq;
    }
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) first[k] = (int)threadIdx.x + k * FU_THREADS < N && dup[k] == 0;
}

// rank[k] = first occurrences before row p_k (in row order); returns the frame's number of distinct rows in every thread
template <int PER>
__device__ __forceinline__ int rank_first(const bool (&first)[PER], int (&rank)[PER], int* s_wave /* [FU_WAVES] */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int flag = first[k] ? 1 : 0;
    int incl = flag;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    __syncthreads();                              // the previous block's reads of s_wave are over
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < FU_WAVES; ++w) {
      const int t = s_wave[w];
      before += w < wave ? t : 0;
      total += t;
    }
    rank[k] = carry + before + incl - flag;
    carry += total;
  }
  return carry;
}

// u_off[f + 1] = the number of distinct rows of frame f (scanned in place by the kernel below)
template <int C, int PER>
__global__ __launch_bounds__(FU_THREADS) void frames_unique_count_kernel(const float* __restrict__ frames, int N,
                                                                         int* __restrict__ u_off) {
  __shared__ __attribute__((aligned(16))) uint32_t s_w[PER * FU_THREADS * C];
  __shared__ int s_wave[FU_WAVES];
  const long f = blockIdx.x;
  const int NC = N * C;
  stage_frame<C>(s_w, frames + f * (long)NC, NC, (uintptr_t)frames % 16 == 0);
  bool first[PER];
  int mult[PER], rank[PER];
  search_rows<C, PER, false>(s_w, N, first, mult);
  const int distinct = rank_first<PER>(first, rank, s_wave);
  if (threadIdx.x == 0) u_off[f + 1] = distinct;
}

// u_off[0] = 0, u_off[f + 1] = cnt[0] + .. + cnt[f] where cnt[f] arrives in u_off[f + 1]: one workgroup walks the frames in
// chunks of its size with a running carry; a thread reads and writes its own entry only
__global__ __launch_bounds__(FU_SCAN_THREADS) void frames_unique_scan_kernel(int n, int* __restrict__ u_off) {
  __shared__ int s_wave[FU_SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;                                  // the same in every thread
  if (tid == 0) u_off[0] = 0;
  for (int base = 0; base < n; base += FU_SCAN_THREADS) {
    const int f = base + tid;
    int incl = f < n ? u_off[f + 1] : 0;
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
    for (int w = 0; w < FU_SCAN_THREADS / 64; ++w) {
      const int t = s_wave[w];
      before += w < wave ? t : 0;
      total += t;
    }
    if (f < n) u_off[f + 1] = carry + before + incl;
    carry += total;
  }
}

// an offset rebased to the call's first frame, as pcaa_segment_weighted_mean takes it; -1 (a bad segment there) when it
// leaves [0, M]
__device__ __forceinline__ int seg_value(long v, long M) { return (v < 0 || v > M) ? -1 : (int)v; }

// Frames a .. a + nf - 1 (u_off already points at entry a): blocks 0 .. nf - 1 write a frame each, the blocks behind them
// share the rows no frame owns
template <int C, int PER>
__global__ __launch_bounds__(FU_THREADS) void frames_unique_kernel(
    const float* __restrict__ frames, int nf, int N, const int* __restrict__ u_off, float* __restrict__ rows,
    float* __restrict__ weight, long M, int* __restrict__ seg_off, int* __restrict__ err) {
  __shared__ __attribute__((aligned(16))) uint32_t s_w[PER * FU_THREADS * C];
  __shared__ int s_wave[FU_WAVES];
  const int tid = threadIdx.x;
  const long base = u_off[0];

  if ((long)blockIdx.x >= (long)nf) {             // rows u_off[nf] - base .. M - 1: zero, weight 0
    long r0 = (long)u_off[nf] - base;
    r0 = r0 < 0 ? 0 : (r0 > M ? M : r0);
    const long nb = (long)gridDim.x - nf, b = (long)blockIdx.x - nf;
    const long per = (M - r0 + nb - 1) / nb;
    const long lo = r0 + b * per, hi = lo + per < M ? lo + per : M;
    for (long r = lo + tid; r < hi; r += FU_THREADS) weight[r] = 0.f;
    for (long e = lo * C + tid; e < hi * C; e += FU_THREADS) rows[e] = 0.f;
    if (b == 0 && tid == 0) seg_off[0] = 0;
    return;
  }
  const long f = blockIdx.x;
  const long u0 = (long)u_off[f] - base, u1 = (long)u_off[f + 1] - base;
  if (tid == 0) seg_off[f + 1] = seg_value(u1, M);
  const int NC = N * C;
  stage_frame<C>(s_w, frames + f * (long)NC, NC, (uintptr_t)frames % 16 == 0);
  bool first[PER];
  int mult[PER], rank[PER];
  search_rows<C, PER, true>(s_w, N, first, mult);
  const int distinct = rank_first<PER>(first, rank, s_wave);
  if (u0 < 0 || u1 > M || u1 - u0 != (long)distinct) {       // the segment is not this frame's (inconsistent offsets):
    if (err != nullptr && tid == 0) atomicOr(err, 1);        // nothing is written, uniform over the workgroup
    return;
  }
  const bool vec = (C == 4) && ((uintptr_t)rows % 16 == 0);
  uint32_t* out = reinterpret_cast<uint32_t*>(rows);
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (!first[k]) continue;
    const int p = tid + k * FU_THREADS;           // < N: first[k] says so
    const long r = u0 + rank[k];                  // rank[k] < distinct = u1 - u0, 0 <= u0, u1 <= M
    if (C == 4 && vec) {
      *reinterpret_cast<uint4*>(out + r * C) = *reinterpret_cast<const uint4*>(s_w + p * C);
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) out[r * C + c] = s_w[p * C + c];
    }
    weight[r] = (float)mult[k];
  }
}

struct FuArgs {
  const float* frames;
  int nf, N;
  int* u_off;
  float *rows, *weight;
  long M;
  int *seg_off, *err;
};

template <int C, int PER>
void launch_fu(bool count, dim3 grid, hipStream_t st, const FuArgs& a) {
  if (count)
    hipLaunchKernelGGL((frames_unique_count_kernel<C, PER>), grid, dim3(FU_THREADS), 0, st, a.frames, a.N, a.u_off);
  else
    hipLaunchKernelGGL((frames_unique_kernel<C, PER>), grid, dim3(FU_THREADS), 0, st, a.frames, a.nf, a.N, a.u_off, a.rows,
                       a.weight, a.M, a.seg_off, a.err);
}

// one row per thread up to N = 256, four above (N <= PCAA_RAW_MAX_POINTS = 4 * 256)
void dispatch_fu(bool count, int C, dim3 grid, hipStream_t st, const FuArgs& a) {
  static_assert(PCAA_RAW_MAX_POINTS == 4 * FU_THREADS, "a thread owns at most four rows");
#define PCAA_FU_CASE(CC)                                                                                               \
  case CC:                                                                                                             \
    if (a.N <= FU_THREADS) launch_fu<CC, 1>(count, grid, st, a); else launch_fu<CC, 4>(count, grid, st, a);            \
    break;
  switch (C) {
    PCAA_FU_CASE(1) PCAA_FU_CASE(2) PCAA_FU_CASE(3) PCAA_FU_CASE(4) PCAA_FU_CASE(5)
  }
#undef PCAA_FU_CASE
}

}  // namespace

extern "C" int pcaa_frames_unique_offsets(const float* frames, int n, int N, int C, int* u_off, void* stream) {
  PCAA_CHECK_ARG(N >= 1 && N <= PCAA_RAW_MAX_POINTS && C >= 1 && C <= FU_MAX_COLS,
                 "pcaa_frames_unique_offsets: needs 1 <= N <= PCAA_RAW_MAX_POINTS and 1 <= C <= 5");
  PCAA_CHECK_ARG(n >= 0 && (long)n * N < (1L << 31), "pcaa_frames_unique_offsets: needs n >= 0 and n * N < 2^31");
  PCAA_CHECK_ARG(u_off != nullptr && ((uintptr_t)u_off % 4) == 0, "pcaa_frames_unique_offsets: u_off is null or not 4-B aligned");
  PCAA_CHECK_ARG(n == 0 || (frames != nullptr && ((uintptr_t)frames % 4) == 0),
                 "pcaa_frames_unique_offsets: frames are null or not 4-B aligned");
  hipStream_t st = as_stream(stream);
  if (n > 0) {
    const FuArgs a{frames, n, N, u_off, nullptr, nullptr, 0, nullptr, nullptr};
    dispatch_fu(true, C, dim3((unsigned)n), st, a);
  }
  hipLaunchKernelGGL(frames_unique_scan_kernel, dim3(1), dim3(FU_SCAN_THREADS), 0, st, n, u_off);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_frames_unique_offsets");
}

extern "C" int pcaa_frames_unique(const float* frames, int n, int N, int C, const int* u_off, int a, int b, float* rows,
                                  float* weight, long M, int* seg_off, int* err_flag, void* stream) {
  PCAA_CHECK_ARG(N >= 1 && N <= PCAA_RAW_MAX_POINTS && C >= 1 && C <= FU_MAX_COLS,
                 "pcaa_frames_unique: needs 1 <= N <= PCAA_RAW_MAX_POINTS and 1 <= C <= 5");
  PCAA_CHECK_ARG(n >= 0 && (long)n * N < (1L << 31) && a >= 0 && a <= b && b <= n,
                 "pcaa_frames_unique: needs n >= 0, n * N < 2^31 and 0 <= a <= b <= n");
  PCAA_CHECK_ARG(M >= 1 && M < (1L << 31), "pcaa_frames_unique: needs 1 <= M < 2^31");
  PCAA_CHECK_ARG(rows != nullptr && weight != nullptr && u_off != nullptr && seg_off != nullptr &&
                     ((uintptr_t)rows % 4) == 0 && ((uintptr_t)weight % 4) == 0 && ((uintptr_t)u_off % 4) == 0 &&
                     ((uintptr_t)seg_off % 4) == 0,
                 "pcaa_frames_unique: rows / weight / u_off / seg_off are null or not 4-B aligned");
  PCAA_CHECK_ARG(a == b || (frames != nullptr && ((uintptr_t)frames % 4) == 0),
                 "pcaa_frames_unique: frames are null or not 4-B aligned");
  long tail = cdiv(M, 4096);                      // blocks that zero the rows no frame owns
  tail = tail < 1 ? 1 : (tail > 64 ? 64 : tail);
  const int nf = b - a;
  const FuArgs args{frames == nullptr ? nullptr : frames + (long)a * N * C, nf, N, const_cast<int*>(u_off) + a, rows,
                    weight, M, seg_off, err_flag};
  dispatch_fu(false, C, dim3((unsigned)(nf + tail)), as_stream(stream), args);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_frames_unique");
}
