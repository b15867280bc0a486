// Frame-deduplicated open-set inference: the byte-level helpers around the existing eval path.
//
// Crops are cut out of a processed track with a hop of CROP_STEP = 6 frames out of NSTEPS = 30 (reference
// datasets.py:16-25, 297-302), after the frames were standardised one by one (datasets.py:143-146): consecutive crops of a
// track share 24 frames, with the same bits.  In eval mode the PointNet block and the mean over a frame's points see one
// frame at a time (models.py:82-105, 242-243), so a shared frame needs encoding once.  Here:
//   * pcaa_crop_overlap    -- which consecutive crops share their overlap bit for bit (the mask the plan is built from);
//   * pcaa_gather_rows_w4  -- the row gather for frames that are not a multiple of 16 bytes (N = 150, C = 5: 3 000 B);
//   * pcaa_scatter_rows    -- the inverse of the row gather: a tick's frame features into the rings of many live streams;
//   * pcaa_gather_sum_rows -- the adjoint of the row gather: window gradients added up into the frame-feature table.
// The windowed read of the frame-feature table is an addressing mode of the temporal block's kernels (dtc_fused.hip).
#include "common.h"

namespace {

// One workgroup per pair (i, i + 1): words [hop * frame, T * frame) of crop i against words [0, (T - hop) * frame) of crop
// i + 1.  Memory bound: 2 x 48 KB per pair at N = 128, C = 4, every lane keeps UNROLL independent 16-B (or 4-B) loads of
// each side in flight.  The verdict of the 256 threads meets in one LDS word (every writer stores the same value), so
// same[i] is written exactly once per launch and needs no pre-set.
template <typename V>
__device__ __forceinline__ bool words_differ(const V& a, const V& b);
template <>
__device__ __forceinline__ bool words_differ<uint4>(const uint4& a, const uint4& b) {
  return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) != 0u;
}
template <>
__device__ __forceinline__ bool words_differ<uint32_t>(const uint32_t& a, const uint32_t& b) {
  return a != b;
}

template <typename V>
__global__ __launch_bounds__(256) void crop_overlap_kernel(const V* __restrict__ crops, long crop_vec, long lead_vec,
                                                           long n_vec, int* __restrict__ same) {
  __shared__ int differs;
  const int tid = threadIdx.x;
  if (tid == 0) differs = 0;
  __syncthreads();
  const V* a = crops + (long)blockIdx.x * crop_vec + lead_vec;        // last T - hop frames of crop i
  const V* b = crops + ((long)blockIdx.x + 1) * crop_vec;             // first T - hop frames of crop i + 1
  constexpr int UNROLL = 4;
  bool diff = false;
  long v = tid;
  for (; v + (UNROLL - 1) * 256 < n_vec; v += UNROLL * 256) {
    V va[UNROLL], vb[UNROLL];
#pragma unroll
    for (int j = 0; j < UNROLL; ++j) {
      va[j] = a[v + j * 256];
      vb[j] = b[v + j * 256];
    }
#pragma unroll
    for (int j = 0; j < UNROLL; ++j) diff |= words_differ<V>(va[j], vb[j]);
  }
  for (; v < n_vec; v += 256) diff |= words_differ<V>(a[v], b[v]);
  if (diff) differs = 1;
  __syncthreads();
  if (tid == 0) same[blockIdx.x] = differs ? 0 : 1;
}

__global__ __launch_bounds__(256) void gather_rows_w4_kernel(const uint32_t* __restrict__ src, const long long* __restrict__ idx,
                                                             long n_src, uint32_t* __restrict__ dst, long n_rows,
                                                             long row_words, int* __restrict__ err) {
  const long total = n_rows * row_words;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < total; v += (long)gridDim.x * 256) {
    const long r = v / row_words, off = v - r * row_words;
    const long long i = idx[r];
    uint32_t val = 0u;
    if (i >= 0 && i < n_src) val = src[i * row_words + off];
    else if (err != nullptr && off == 0) atomicOr(err, 1);
    dst[v] = val;
  }
}

// dst[dst_row[r]] = src[r], rows of row_vec vectors: a 4-KB feature row is 256 16-B vectors, one per lane of a workgroup.
// dst_row[r] < 0: the row is dropped (padding); >= n_dst: dropped and flagged.  Plain vector loads and stores.
template <typename V>
__global__ __launch_bounds__(256) void scatter_rows_kernel(const V* __restrict__ src, const int* __restrict__ dst_row,
                                                           long n_dst, V* __restrict__ dst, long n_rows, long row_vec,
                                                           int* __restrict__ err) {
  const long total = n_rows * row_vec;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < total; v += (long)gridDim.x * 256) {
    const long r = v / row_vec, off = v - r * row_vec;
    const long d = dst_row[r];
    if (d < 0) continue;
    if (d >= n_dst) {
      if (err != nullptr && off == 0) atomicOr(err, 1);
      continue;
    }
    dst[d * row_vec + off] = src[v];
  }
}

// dst[u] = sum_{k = csr_off[u]}^{csr_off[u + 1] - 1} src[csr_idx[k]]: the adjoint of the row gather, the overlap-add of the
// window gradients into the frame-feature table.  One thread per (table row, vector) walks the row's contributors in
// ascending k and adds them to +0 in fp32: plain adds, no atomics, so the result is a function of the CSR alone.  A row
// without contributors is zero; an index outside the source is skipped and flagged, and so is a row whose offsets leave
// [0, nnz] (it is written as zeros).
template <typename V>
__global__ __launch_bounds__(256) void gather_sum_rows_kernel(const V* __restrict__ src, long n_src,
                                                              const int* __restrict__ csr_off,
                                                              const int* __restrict__ csr_idx, long nnz,
                                                              V* __restrict__ dst, long n_dst, long row_vec,
                                                              int* __restrict__ err) {
#pragma clang fp contract(off)
  const long total = n_dst * row_vec;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < total; v += (long)gridDim.x * 256) {
    const long u = v / row_vec, off = v - u * row_vec;
    long k0 = csr_off[u], k1 = csr_off[u + 1];
    if (k0 < 0 || k1 < k0 || k1 > nnz) {
      if (err != nullptr && off == 0) atomicOr(err, 1);
      k0 = k1 = 0;
    }
    V acc = {};
    for (long k = k0; k < k1; ++k) {
      const long i = csr_idx[k];
      if (i < 0 || i >= n_src) {
        if (err != nullptr && off == 0) atomicOr(err, 1);
        continue;
      }
      acc += src[i * row_vec + off];
    }
    dst[v] = acc;
  }
}

}  // namespace

extern "C" int pcaa_crop_overlap_vec_bytes(const float* crops, long crop_elems, long frame_elems) {
  // crop_elems = T * frame_elems and every offset is a whole number of frames: frames of whole 16-B vectors keep all of them aligned
  return (((uintptr_t)crops % 16) == 0 && frame_elems % 4 == 0 && crop_elems % 4 == 0) ? 16 : 4;
}

extern "C" int pcaa_crop_overlap(const float* crops, long crop_elems, long frame_elems, int M, int T, int hop, int* same,
                                 void* stream) {
  PCAA_CHECK_ARG(crops && M >= 1 && T >= 1 && hop >= 1 && hop <= T && frame_elems >= 1 && crop_elems >= (long)T * frame_elems,
                 "pcaa_crop_overlap: bad args (1 <= hop <= T, crop_elems >= T * frame_elems)");
  PCAA_CHECK_ARG(((uintptr_t)crops % 4) == 0, "pcaa_crop_overlap: crops must be 4-B aligned");
  if (M == 1) return PCAA_OK;
  PCAA_CHECK_ARG(same != nullptr, "pcaa_crop_overlap: same is null");
  const long n = (long)(T - hop) * frame_elems, lead = (long)hop * frame_elems;     // hop == T: nothing shared, all equal
  if (pcaa_crop_overlap_vec_bytes(crops, crop_elems, frame_elems) == 16)
    hipLaunchKernelGGL(crop_overlap_kernel<uint4>, dim3(M - 1), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const uint4*>(crops), crop_elems / 4, lead / 4, n / 4, same);
  else
    hipLaunchKernelGGL(crop_overlap_kernel<uint32_t>, dim3(M - 1), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const uint32_t*>(crops), crop_elems, lead, n, same);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_crop_overlap");
}

extern "C" int pcaa_gather_rows_w4(const void* src, long n_src_rows, long row_words, const long long* idx, void* dst,
                                   long n_rows, int* err_flag, void* stream) {
  PCAA_CHECK_ARG(src && idx && dst && n_src_rows >= 1 && n_rows >= 1 && row_words >= 1, "pcaa_gather_rows_w4: bad args");
  PCAA_CHECK_ARG(((uintptr_t)src % 4) == 0 && ((uintptr_t)dst % 4) == 0, "pcaa_gather_rows_w4: 4-B alignment");
  const long total = n_rows * row_words;
  const long blocks = cdiv(total, 256 * 4);
  hipLaunchKernelGGL(gather_rows_w4_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks))), dim3(256), 0,
                     as_stream(stream), reinterpret_cast<const uint32_t*>(src), idx, n_src_rows,
                     reinterpret_cast<uint32_t*>(dst), n_rows, row_words, err_flag);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_gather_rows_w4");
}

extern "C" int pcaa_scatter_rows(const void* src, const int* dst_row, long n_rows, long row_words, void* dst,
                                 long n_dst_rows, int* err_flag, void* stream) {
  PCAA_CHECK_ARG(src && dst_row && dst && n_rows >= 1 && row_words >= 1 && n_dst_rows >= 1, "pcaa_scatter_rows: bad args");
  PCAA_CHECK_ARG(((uintptr_t)src % 4) == 0 && ((uintptr_t)dst % 4) == 0, "pcaa_scatter_rows: 4-B alignment");
  const bool v16 = row_words % 4 == 0 && ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0;
  const long row_vec = v16 ? row_words / 4 : row_words;
  const long want = cdiv(n_rows * row_vec, 256);
  const dim3 grid((unsigned)(want > 4096 ? 4096 : want));
  if (v16)
    hipLaunchKernelGGL(scatter_rows_kernel<uint4>, grid, dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const uint4*>(src), dst_row, n_dst_rows, reinterpret_cast<uint4*>(dst), n_rows,
                       row_vec, err_flag);
  else
    hipLaunchKernelGGL(scatter_rows_kernel<uint32_t>, grid, dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const uint32_t*>(src), dst_row, n_dst_rows, reinterpret_cast<uint32_t*>(dst), n_rows,
                       row_vec, err_flag);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_scatter_rows");
}

extern "C" int pcaa_gather_sum_rows(const float* src, long n_src_rows, long row_words, const int* csr_off,
                                    const int* csr_idx, long nnz, float* dst, long n_dst_rows, int* err_flag,
                                    void* stream) {
  PCAA_CHECK_ARG(src && csr_off && dst && (csr_idx || nnz == 0), "pcaa_gather_sum_rows: null pointer");
  PCAA_CHECK_ARG(n_src_rows >= 1 && n_dst_rows >= 1 && row_words >= 1 && nnz >= 0 && nnz < (1L << 31),
                 "pcaa_gather_sum_rows: needs n_src_rows, n_dst_rows, row_words >= 1 and 0 <= nnz < 2^31");
  PCAA_CHECK_ARG(((uintptr_t)src % 4) == 0 && ((uintptr_t)dst % 4) == 0 && ((uintptr_t)csr_off % 4) == 0 &&
                     ((uintptr_t)csr_idx % 4) == 0, "pcaa_gather_sum_rows: 4-B alignment");
  PCAA_CHECK_ARG(src != dst, "pcaa_gather_sum_rows: dst may not alias src");
  const bool v16 = row_words % 4 == 0 && ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0;
  const long row_vec = v16 ? row_words / 4 : row_words;
  const long want = cdiv(n_dst_rows * row_vec, 256);
  const dim3 grid((unsigned)(want > 4096 ? 4096 : want));
  if (v16)
    hipLaunchKernelGGL(gather_sum_rows_kernel<f32x4>, grid, dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const f32x4*>(src), n_src_rows, csr_off, csr_idx, nnz,
                       reinterpret_cast<f32x4*>(dst), n_dst_rows, row_vec, err_flag);
  else
    hipLaunchKernelGGL(gather_sum_rows_kernel<float>, grid, dim3(256), 0, as_stream(stream), src, n_src_rows, csr_off,
                       csr_idx, nnz, dst, n_dst_rows, row_vec, err_flag);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_gather_sum_rows");
}
