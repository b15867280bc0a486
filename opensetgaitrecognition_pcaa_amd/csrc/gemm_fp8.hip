// Eval-mode PointNet layers 2-4 on the block-scaled fp8 MFMA (pcaa_gemm_fp8_affine_elu, pcaa_quantize_weight_fp8): the
// deployment precision of the scorers (the numerics contract is in include/pcaa_hip.h).
//
// v_mfma_scale_f32_32x32x64_f8f6f4 with e4m3 operands and every e8m0 block scale 1.0 (0x7f) runs at twice the bf16 rate
// per clock; the plain _fp8_fp8 forms run at the bf16 rate.  256 x 256 tile, four waves (2 x 2) of 128 x 128 = 4 x 4
// accumulator blocks of 32 x 32 (256 accumulator registers, as the bf16 loop of gemm_v2.h), one workgroup per tile.
//
// Staging: a ring of FOUR 32-KB stages, each 64 bytes of K of both operands (256 rows x 64 B each), filled by LDS-DMA
// (buffer_load ... lds, 16 B per lane, 1 KB per instruction).  An operand's image is row-major with 64-B rows, the four
// 16-B granules of row r stored at position g ^ ((r >> 2) & 3): a request fetches the whole 64 bytes of 16 rows, and the
// 16 lanes of a fragment read (two ds_read_b128 per lane: granules h and 2 + h of row lane & 31, h = lane >> 5) hit 16
// distinct bank groups.  (The first layout, no longer built: the image in fragment order, a
// fragment read 1 KB contiguous -- and every request 32 bytes from each of 32 rows: twice the cache-line touches per
// byte, and slower: DESIGN.md section 4.)  Both operands use the same lane -> k map, so whatever order the
// instruction gives the 64 k of a step, it pairs a[k] with w[k]; only the row / column lane map (lane & 31) and the C/D
// layout (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) matter.
// Pipeline: the fragments of step t + 1 are read into a second register set under the MFMAs of step t; the stage a step
// has just read is refilled for step t + 4 behind the step's one barrier: three steps of prefetch distance.  The
// fragment reads are inline asm: the compiler does not see that they read what the DMA writes and so keeps its own
// s_waitcnt vmcnt(0) out of the loop; every use of a fragment sits behind an explicit s_waitcnt lgkmcnt(0).
//
// Which operand is the MFMA's A decides what a lane holds at the end:
//   * unpooled (e4m3 / bf16 rows): A = weights, B = activations -- a lane holds ONE output row and 16 channels per block;
//     the weight rows are permuted on their way into the LDS (slot rho of a 32-row block holds channel
//     16 ((rho >> 2) & 1) + (rho & 3) + 4 (rho >> 3)) so that these are 16 ADJACENT channels: one 16-B store of e4m3;
//   * pooled (fp32 means): A = activations, B = weights -- a lane holds one channel and 16 rows of a 32-row block: the
//     mean over a group is 15 adds per block and ONE cross-lane exchange.
// Rows past M of a partial last row tile lie outside the activation's buffer range and read as zeros; their stores are
// guarded.  Each tile's resources are based on its own 256 rows: operands of any total size.
// Registers / LDS / rates: DESIGN.md section 4.
#include "gemm_common.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;

constexpr int TILE = 256;                  // rows and columns of a tile
constexpr int KSTAGE = 64;                 // bytes (= e4m3 elements) of K per ring stage: one 32x32x64 MFMA per block
constexpr int NSTAGE = 4;
constexpr int OP_BYTES = TILE * KSTAGE;    // one operand's stage image (16 KB)
constexpr int STAGE_BYTES = 2 * OP_BYTES;  // activations, then weights
constexpr int LDS_BYTES = NSTAGE * STAGE_BYTES;      // 128 KB: one workgroup per CU
constexpr int K_MIN = 128, K_STEP = 128;   // two stages per loop trip (the register sets alternate)

enum { OUT_E4M3 = 0, OUT_BF16 = 1, OUT_POOL = 2 };

struct Fp8Params {
  const unsigned char* A; const unsigned char* W; void* out;
  long lda, ldw, ldo;
  const float* scale; const float* shift;
  int M, N, K;
};

__device__ __forceinline__ rsrc_t make_rsrc(const void* base, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)(unsigned)bytes, 0x00020000);
}

// as gemm_v2.h: ELU of z given z2 = z log2(e) -- and a NaN stays a NaN (the min / max of that form drop one: a NaN
// accumulator would leave as -1, and the route's contract is that a NaN operand row shows in its output row)
__device__ __forceinline__ float elu_from_z2(float z2) {
  const float e = __builtin_fminf(__builtin_fmaxf(__builtin_amdgcn_exp2f(z2), 0.f), 1.f);
  const float r = fmaf(__builtin_fmaxf(z2, 0.f), 0.6931471805599453f, e - 1.f);
  return z2 != z2 ? z2 : r;
}

__device__ __forceinline__ f32x16 mfma_e4m3(const i32x8& a, const i32x8& b, const f32x16& c) {
  // cbsz = blgp = 0: both operands e4m3; scales: byte 0 of 0x7f7f7f7f = 2^0 for every 32-element block
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
}

__device__ __forceinline__ unsigned pack2_bf16(float a, float b) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  const bf16x2 v = {(bf16_t)a, (bf16_t)b};
  return __builtin_bit_cast(unsigned, v);
}

// OUT_E4M3 / OUT_BF16: out [M, ldo]; OUT_POOL with IPG = pool_rows / 32 blocks per group: out fp32 [M / pool_rows, ldo]
template <int OUT, int IPG>
__global__ __launch_bounds__(256) void gemm_fp8_kernel(Fp8Params p) {
  extern __shared__ __attribute__((aligned(64))) unsigned char smem[];
  constexpr bool POOL = OUT == OUT_POOL;
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int nbm = (p.M + TILE - 1) / TILE, nbn = p.N / TILE;
  int tm, tn;
  xcd_tile_coords(nbm, nbn, (int)blockIdx.x, tm, tn);
  const int nt = p.K / KSTAGE;             // ring stages of this tile (even: K % 128 == 0)

  const rsrc_t rA = make_rsrc(p.A + (long)tm * TILE * p.lda, (long)min(TILE, p.M - tm * TILE) * p.lda);   // rows past M: zeros
  const rsrc_t rW = make_rsrc(p.W + (long)tn * TILE * p.ldw, (long)TILE * p.ldw);
  // this wave's four pieces of each operand: piece w * 4 + j = rows 16 (4 w + j) .. + 15 of the image; lane l: row l >> 2
  // of them, stored granule l & 3.  The row offset rides in the VECTOR offset: the buffer range check does not cover the
  // scalar one.
  unsigned voA[4], voW[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = 16 * (4 * wave + j) + (lane >> 2), g = (lane & 3) ^ ((row >> 2) & 3);
    const int rho = row & 31;
    const int rw = POOL ? row : (row & ~31) + 16 * ((rho >> 2) & 1) + (rho & 3) + 4 * (rho >> 3);
    voA[j] = (unsigned)((long)row * p.lda + 16 * g);
    voW[j] = (unsigned)((long)rw * p.ldw + 16 * g);
  }
  typedef __attribute__((address_space(3))) void* lds_ptr;
#define FP8_REQUEST(t)                                                                                              \
  do {                                                                                                              \
    unsigned char* st_ = smem + ((t) & (NSTAGE - 1)) * STAGE_BYTES + wave * 4096;                                   \
    const unsigned so_ = (unsigned)__builtin_amdgcn_readfirstlane((t) * KSTAGE);                                    \
    _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_)                                                                \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_ptr)(st_ + j_ * 1024), 16, voA[j_], so_, 0, 0);             \
    _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_)                                                                \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (lds_ptr)(st_ + OP_BYTES + j_ * 1024), 16, voW[j_], so_, 0, 0);  \
  } while (0)
  // eight requests per wave and stage; loads retire in order, so "at most 8 n outstanding" means every stage but the
  // newest n has landed
#define FP8_WAIT_STAGE(newer)                                                             \
  do {                                                                                    \
    if ((newer) >= 2) asm volatile("s_waitcnt vmcnt(16)\n\ts_barrier" ::: "memory");      \
    else if ((newer) == 1) asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");  \
    else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");                    \
  } while (0)

  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  // a lane's two 16-B reads (q = 0, 1) of block b of its wave's four: + 2048 b from these
  unsigned fA, fW;
  {
    const int r = lane & 31, h = lane >> 5, sw = (r >> 2) & 3;
    const unsigned l0 = (unsigned)(r * 64 + ((h ^ sw) * 16));
    fA = lds0 + (unsigned)(wm * 8 * 1024) + l0;
    fW = lds0 + (unsigned)(OP_BYTES + wn * 8 * 1024) + l0;
  }
  // The 16 fragments (two sets of 4 weight + 4 activation blocks, 8 registers each) live in v[128:255] BY NAME: a fragment
  // is two ds_read_b128 into the halves of one 8-register operand, and inline asm cannot name half of an operand the
  // register allocator chose (left to it, every fragment was copied once per step: 64 v_mov_b64 per loop trip).
  i32x8 fr[16];        // [8 set + b]: weight block b; [8 set + 4 + b]: activation block b
  // (the second granule sits at the first one's address with bit 5 flipped -- the stage images start on 64-B
  // boundaries -- formed in the destination's own first register: no second address register per operand)
#define FP8_RD(n, r0, r3, r4, r7, addr, off)                                                                              \
  asm volatile("ds_read_b128 v[" #r0 ":" #r3 "], %1 offset:%2\n\tv_xor_b32 v" #r4 ", 32, %1\n\t"                          \
               "ds_read_b128 v[" #r4 ":" #r7 "], v" #r4 " offset:%2"                                                      \
               : "=&{v[" #r0 ":" #r7 "]}"(fr[n]) : "v"(addr), "n"(off))
  // fragment k (0..7) of a set: k < 4 weight block k, else activation block k - 4
#define FP8_READ_ONE(set, k, aw, aa)                                                      \
  do {                                                                                    \
    if ((set) == 0) {                                                                     \
      if (k == 0) FP8_RD(0, 128, 131, 132, 135, aw, 0);                                   \
      if (k == 1) FP8_RD(1, 136, 139, 140, 143, aw, 2048);                                \
      if (k == 2) FP8_RD(2, 144, 147, 148, 151, aw, 4096);                                \
      if (k == 3) FP8_RD(3, 152, 155, 156, 159, aw, 6144);                                \
      if (k == 4) FP8_RD(4, 160, 163, 164, 167, aa, 0);                                   \
      if (k == 5) FP8_RD(5, 168, 171, 172, 175, aa, 2048);                                \
      if (k == 6) FP8_RD(6, 176, 179, 180, 183, aa, 4096);                                \
      if (k == 7) FP8_RD(7, 184, 187, 188, 191, aa, 6144);                                \
    } else {                                                                              \
      if (k == 0) FP8_RD(8, 192, 195, 196, 199, aw, 0);                                   \
      if (k == 1) FP8_RD(9, 200, 203, 204, 207, aw, 2048);                                \
      if (k == 2) FP8_RD(10, 208, 211, 212, 215, aw, 4096);                               \
      if (k == 3) FP8_RD(11, 216, 219, 220, 223, aw, 6144);                               \
      if (k == 4) FP8_RD(12, 224, 227, 228, 231, aa, 0);                                  \
      if (k == 5) FP8_RD(13, 232, 235, 236, 239, aa, 2048);                               \
      if (k == 6) FP8_RD(14, 240, 243, 244, 247, aa, 4096);                               \
      if (k == 7) FP8_RD(15, 248, 251, 252, 255, aa, 6144);                               \
    }                                                                                     \
  } while (0)

  f32x16 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // prologue: stages 0 .. 3 (as far as the tile has them); the fragments of stage 0
  FP8_REQUEST(0);
  FP8_REQUEST(1);
  if (nt > 2) { FP8_REQUEST(2); FP8_REQUEST(3); }
  FP8_WAIT_STAGE(nt - 1);
#pragma unroll
  for (int k = 0; k < 8; ++k) FP8_READ_ONE(0, k, fW, fA);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // step t on register set ``set``: stage t + 1 has landed and every wave holds its fragments of stage t (barrier), so
  // stage t is dead: refill it for t + 4; the fragments of t + 1 go into the other set under the first MFMAs of stage t
  // (sched_barrier: the order written here is the order issued).  The reads are unconditional -- behind the tile's last
  // stage they fetch a stale stage into registers nobody uses: a branch around inline asm costs a copy of every fragment.
#define FP8_STEP(set, t)                                                                                          \
  do {                                                                                                            \
    const bool more_ = (t) + 1 < nt;                                                                              \
    if (more_) {                                                                                                  \
      FP8_WAIT_STAGE(nt - 2 - (t));                                                                               \
      if ((t) + NSTAGE < nt) FP8_REQUEST((t) + NSTAGE);                                                           \
    }                                                                                                             \
    const unsigned so_ = (unsigned)((((t) + 1) & (NSTAGE - 1)) * STAGE_BYTES);                                     \
    const unsigned aw_ = fW + so_, aa_ = fA + so_;                                                                \
    _Pragma("unroll") for (int m_ = 0; m_ < 16; ++m_) {                                                           \
      const int i_ = m_ >> 2, j_ = m_ & 3;                                                                        \
      if (m_ < 8) FP8_READ_ONE((set) ^ 1, m_, aw_, aa_);                                                          \
      acc[i_][j_] = POOL ? mfma_e4m3(fr[8 * (set) + 4 + i_], fr[8 * (set) + j_], acc[i_][j_])                     \
                         : mfma_e4m3(fr[8 * (set) + j_], fr[8 * (set) + 4 + i_], acc[i_][j_]);                    \
      __builtin_amdgcn_sched_barrier(0);                                                                          \
    }                                                                                                             \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                            \
  } while (0)
  for (int t = 0; t < nt; t += 2) {
    FP8_STEP(0, t);
    FP8_STEP(1, t + 1);
  }
#undef FP8_STEP
#undef FP8_READ_ONE
#undef FP8_RD
#undef FP8_WAIT_STAGE
#undef FP8_REQUEST

  // ------------------------------------------------------------------------------------------------ epilogues
  constexpr float LOG2E = 1.4426950408889634f;
  // the lane id re-read from the hardware (volatile: not hoisted): derived from the kernel's first lane id, the epilogue's
  // row pointers were formed in front of the tile loop and spilled across it (36 B of scratch in the bf16 instantiations)
  int le;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(le));
  const int c = le & 31, h = le >> 5;
  if constexpr (!POOL) {
    // lane (c, h): row 32 i + c of the wave's 128, channels 32 j + 16 h .. + 15 (register r: channel 16 h + r)
    // (bf16 rows four channels at a time: with more in flight that instantiation's temporaries went to scratch)
    constexpr int NCH = OUT == OUT_E4M3 ? 16 : 4;
#pragma unroll
    for (int jj = 0; jj < 4 * (16 / NCH); ++jj) {
      const int j = jj / (16 / NCH), r0 = (jj % (16 / NCH)) * NCH;
      const int n0 = tn * TILE + wn * 128 + 32 * j + 16 * h + r0;
      float esc[NCH], esh[NCH];
#pragma unroll
      for (int v = 0; v < NCH / 4; ++v) {
        const f32x4 s4 = load4(p.scale + n0 + 4 * v), h4 = load4(p.shift + n0 + 4 * v);
#pragma unroll
        for (int e = 0; e < 4; ++e) { esc[4 * v + e] = s4[e] * LOG2E; esh[4 * v + e] = h4[e] * LOG2E; }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long m = (long)tm * TILE + wm * 128 + 32 * i + c;
        float o[NCH];
#pragma unroll
        for (int r = 0; r < NCH; ++r) o[r] = elu_from_z2(fmaf(acc[i][j][r0 + r], esc[r], esh[r]));
        if (m < p.M) {
          if constexpr (OUT == OUT_E4M3) {
            unsigned char* d = reinterpret_cast<unsigned char*>(p.out) + m * p.ldo + n0;
            *reinterpret_cast<u32x4*>(d) = u32x4{pack4_e4m3(o[0], o[1], o[2], o[3]), pack4_e4m3(o[4], o[5], o[6], o[7]),
                                                 pack4_e4m3(o[8], o[9], o[10], o[11]), pack4_e4m3(o[12], o[13], o[14], o[15])};
          } else {
            bf16_t* d = reinterpret_cast<bf16_t*>(p.out) + m * p.ldo + n0;
            *reinterpret_cast<uint2*>(d) = uint2{pack2_bf16(o[0], o[1]), pack2_bf16(o[2], o[3])};
          }
        }
      }
    }
  } else {
    // lane (c, h): channel 32 j + c, rows (r & 3) + 8 (r >> 2) + 4 h of block i; a group is IPG whole blocks
    float* out = reinterpret_cast<float*>(p.out);
    constexpr float inv_n = 1.f / (32 * IPG);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = tn * TILE + wn * 128 + 32 * j + c;
      const float esc = p.scale[n] * LOG2E, esh = p.shift[n] * LOG2E;
#pragma unroll
      for (int g0 = 0; g0 < 4; g0 += IPG) {
        float s = 0.f;
#pragma unroll
        for (int i = g0; i < g0 + IPG; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) s += elu_from_z2(fmaf(acc[i][j][r], esc, esh));
        s += __shfl_xor(s, 32, 64);
        const long row0 = (long)tm * TILE + wm * 128 + 32 * g0;      // (M is a whole number of groups)
        if (h == 0 && row0 < p.M) out[row0 / (32 * IPG) * p.ldo + n] = s * inv_n;
      }
    }
  }
}

template <int OUT, int IPG>
bool launch_fp8(const Fp8Params& p, unsigned ntiles, hipStream_t s) {
  static bool configured = false;
  auto kern = gemm_fp8_kernel<OUT, IPG>;
  if (!configured) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess)
      return false;
    configured = true;
  }
  hipLaunchKernelGGL(kern, dim3(ntiles), dim3(256), LDS_BYTES, s, p);
  return true;
}

// one row per wave: absmax, then W / s (an exact scaling by a power of two) rounded to e4m3
__global__ __launch_bounds__(256) void quantize_weight_fp8_kernel(const float* __restrict__ W, unsigned char* __restrict__ W8,
                                                                   float* __restrict__ s, int R, int C) {
  const int row = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
  if (row >= R) return;
  const float* w = W + (long)row * C;
  float m = 0.f;
  bool finite = true;
  for (int k = lane; k < C; k += 64) {
    const float v = fabsf(w[k]);
    finite = finite && v <= 3.4028234663852886e38f;      // false for an infinity and for a NaN
    m = fmaxf(m, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  finite = __all(finite);
  int e = 8;                                             // s = 2^(e - 8): 1 for a zero or non-finite row
  if (finite && m > 0.f) {
    (void)frexpf(m, &e);
    e = max(e, -118);                                    // s stays a normal fp32
  }
  if (lane == 0) s[row] = ldexpf(1.f, e - 8);
  unsigned char* d = W8 + (long)row * C;
  if ((C & 3) == 0) {
    for (int k = 4 * lane; k < C; k += 256) {
      const f32x4 v = load4(w + k);
      *reinterpret_cast<unsigned*>(d + k) = pack4_e4m3(ldexpf(v.x, 8 - e), ldexpf(v.y, 8 - e), ldexpf(v.z, 8 - e), ldexpf(v.w, 8 - e));
    }
  } else {
    for (int k = lane; k < C; k += 64) d[k] = (unsigned char)(pack4_e4m3(ldexpf(w[k], 8 - e), 0.f, 0.f, 0.f) & 0xffu);
  }
}

}  // namespace

extern "C" int pcaa_quantize_weight_fp8(const float* W, void* W8, float* s, int R, int C, void* stream) {
  PCAA_CHECK_ARG(W && W8 && s, "pcaa_quantize_weight_fp8: null pointer");
  PCAA_CHECK_ARG(R >= 1 && C >= 1, "pcaa_quantize_weight_fp8: bad shape (R=%d C=%d)", R, C);
  PCAA_CHECK_ARG(((uintptr_t)W % 16) == 0 && ((uintptr_t)W8 % 4) == 0, "pcaa_quantize_weight_fp8: W needs 16-B, W8 4-B alignment");
  hipLaunchKernelGGL(quantize_weight_fp8_kernel, dim3((unsigned)cdiv(R, 4)), dim3(256), 0, as_stream(stream), W,
                     reinterpret_cast<unsigned char*>(W8), s, R, C);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_quantize_weight_fp8");
}

extern "C" int pcaa_gemm_fp8_supported(int M, int N, int K) {
  return M > 0 && N > 0 && (N % TILE) == 0 && K >= K_MIN && (K % K_STEP) == 0 && (long)cdiv(M, TILE) * (long)(N / TILE) < (1L << 31);
}

extern "C" int pcaa_gemm_fp8_affine_elu(const void* A8, long lda, const void* W8, long ldw, void* out, int out_dtype, long ldo,
                                        const float* scale8, const float* shift, int M, int N, int K, int pool_rows,
                                        void* stream) {
  PCAA_CHECK_ARG(A8 && W8 && out && scale8 && shift, "pcaa_gemm_fp8_affine_elu: null pointer");
  PCAA_CHECK_ARG(pool_rows == 0 || pool_rows == 32 || pool_rows == 64 || pool_rows == 128,
                 "pcaa_gemm_fp8_affine_elu: pool_rows must be 0, 32, 64 or 128");
  PCAA_CHECK_ARG(pool_rows ? out_dtype == PCAA_F32 : (out_dtype == PCAA_FP8_E4M3 || out_dtype == PCAA_BF16),
                 "pcaa_gemm_fp8_affine_elu: bad out_dtype %d (pool_rows 0: PCAA_FP8_E4M3 or PCAA_BF16; pooled: PCAA_F32)", out_dtype);
  PCAA_CHECK_ARG(pcaa_gemm_fp8_supported(M, N, K), "pcaa_gemm_fp8_affine_elu: N must be a multiple of 256, K of 128 and at least "
                 "128 (M: any; a partial last row tile is served) (M=%d N=%d K=%d)", M, N, K);
  PCAA_CHECK_ARG(pool_rows == 0 || (M % pool_rows) == 0, "pcaa_gemm_fp8_affine_elu: M must be a multiple of pool_rows (M=%d)", M);
  const int esz = out_dtype == PCAA_FP8_E4M3 ? 1 : (out_dtype == PCAA_BF16 ? 2 : 4);
  PCAA_CHECK_ARG(lda >= K && ldw >= K && ldo >= N && (lda % 16) == 0 && (ldw % 16) == 0 && lda < (1L << 23) && ldw < (1L << 23) &&
                 (pool_rows != 0 || (ldo * esz) % 16 == 0), "pcaa_gemm_fp8_affine_elu: bad leading dimension");
  PCAA_CHECK_ARG(((uintptr_t)A8 % 16) == 0 && ((uintptr_t)W8 % 16) == 0 && ((uintptr_t)out % (pool_rows ? 4 : 16)) == 0 &&
                 ((uintptr_t)scale8 % 16) == 0 && ((uintptr_t)shift % 16) == 0, "pcaa_gemm_fp8_affine_elu: 16-B alignment");
  Fp8Params p;
  p.A = reinterpret_cast<const unsigned char*>(A8); p.W = reinterpret_cast<const unsigned char*>(W8); p.out = out;
  p.lda = lda; p.ldw = ldw; p.ldo = ldo;
  p.scale = scale8; p.shift = shift;
  p.M = M; p.N = N; p.K = K;
  const unsigned ntiles = (unsigned)(cdiv(M, TILE) * (N / TILE));
  const hipStream_t s = as_stream(stream);
  bool ok;
  switch (pool_rows) {
    case 0: ok = out_dtype == PCAA_FP8_E4M3 ? launch_fp8<OUT_E4M3, 1>(p, ntiles, s) : launch_fp8<OUT_BF16, 1>(p, ntiles, s); break;
    case 32: ok = launch_fp8<OUT_POOL, 1>(p, ntiles, s); break;
    case 64: ok = launch_fp8<OUT_POOL, 2>(p, ntiles, s); break;
    default: ok = launch_fp8<OUT_POOL, 4>(p, ntiles, s); break;
  }
  if (!ok) {
    pcaa_set_error("pcaa_gemm_fp8_affine_elu: launch configuration failed");
    return PCAA_ERR_LAUNCH;
  }
  PCAA_RETURN_LAUNCH_STATUS("pcaa_gemm_fp8_affine_elu");
}
