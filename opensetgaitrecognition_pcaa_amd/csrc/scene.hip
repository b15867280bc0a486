// Scene frames -> people, on the device: the first link of the raw chain.  A radar delivers one point
// cloud per frame with everybody in view plus clutter; pcaa_scene_cluster splits every frame of a tick into density
// clusters and regroups its detections cluster by cluster, pcaa_gather_segments then lays the segments the host's
// association step chose out as the (points, offsets) that push_raw takes.
//
// THE RULE (scene.cluster_host restates it in numpy, bit for bit).  A frame of m detections, columns x, y, z, doppler:
//   d2(i, j) = dx*dx + dy*dy + wz2*dz*dz + wv2*dv*dv        in fp64 from the stored values, evaluated in that order
//              (((dx*dx + dy*dy) + (wz2*dz)*dz) + (wv2*dv)*dv), every product and sum rounded (contraction is off);
//   i and j are NEIGHBOURS iff d2 <= eps2; a point is its own neighbour (a NaN coordinate has none: not even itself);
//   i is CORE iff it has >= min_points neighbours;
//   CLUSTERS are the connected components of the core points under the neighbour relation;
//   a non-core point with at least one core neighbour is a BORDER point and joins the cluster of its NEAREST core
//     neighbour: smallest d2, lowest index on exact ties.  A border point never links two clusters;
//   everything else is NOISE, label -1;
//   cluster ids are 0 .. c - 1 in ascending order of each cluster's lowest core index; clusters with id >= Cmax become
//     noise and set bit 1 of *err.
// Outputs per frame f (rows off0 = offsets[f] .. offsets[f + 1] - 1): label per detection; n_clusters = min(c, Cmax);
// cluster_count [Cmax]; centroid [Cmax, 4] = float32(sum64 / count) per column, the fp64 sum in ascending detection order
// starting from the first member (np.cumsum(...)[-1], bit for bit; unused entries zero); grouped: the frame's rows
// rewritten as cluster 0, cluster 1, ..., then noise, each group in ascending detection order, every row a bit copy; seg_off [Cmax + 1] ABSOLUTE rows: cluster c owns
// grouped[seg_off[c] : seg_off[c + 1]], the noise grouped[seg_off[Cmax] : offsets[f + 1]].
// m == 0 is legal: nobody in view, zero clusters, seg_off = off0.  BAD frames set bit 0 of *err and have zero clusters:
// m > PCAA_RAW_MAX_CARD with offsets inside [0, P] is all noise (labels -1, grouped = the input rows, seg_off = off0);
// offsets outside [0, P] or running backwards touch no row at all (seg_off = 0).  A frame is checked against [0, P] only,
// not against its neighbours: offsets that are not monotone ([0, 10, 5, 15]) make two valid frames share rows, whose
// label / grouped then hold either frame's values (in bounds, no hang, *err not set); the per-frame tables stay exact.
//
// One workgroup of 256 threads per frame; the four used columns (fp64), labels, core flags and ranks live in LDS
// (about 44 KB).  Components: lab[i] = i for a core point, then rounds of "take the smallest label among my core
// neighbours, follow it to its root (pointer jumping)" until a workgroup-wide vote says nothing changed.  Labels only
// decrease and always name a core point of the same component, so concurrent in-place updates are safe and the fixed
// point (every core point holds its component's lowest core index) is unique.  EVERY loop has a trip count bounded by m
// (or Cmax): no spin wait, no communication between workgroups, no device-side assert or printf -- *err is the only
// report, and a wrong input cannot hang the launch.  Distances are recomputed in every round (a neighbour matrix of
// 1024 x 1024 bits would not fit beside the columns), but only against points whose label could still lower mine.
#include "common.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_MAX = PCAA_RAW_MAX_CARD;
constexpr int SC_PER_THREAD = SC_MAX / SC_THREADS;     // consecutive points one thread ranks
constexpr int SC_COLS = 5;                             // a row: x, y, z, doppler, power
constexpr int SC_MAX_CLUSTERS = PCAA_SCENE_MAX_CLUSTERS;
constexpr int SC_NONE = 0x7fffffff;                    // the label of a point that is in no cluster (yet)

struct SceneMetric {
  double eps2, wz2, wv2;
};

struct SceneShared {
  double col[4][SC_MAX];            // x, y, z, doppler of the frame's detections
  int lab[SC_MAX];                  // a core point's current label; SC_NONE for the others until the border pass
  int cid[SC_MAX];                  // by root index: the cluster id; later by point: the final label
  uint16_t rank[SC_MAX];            // a point's position inside its group
  uint8_t core[SC_MAX];
  int cnt[SC_MAX_CLUSTERS + 1];     // detections per cluster; [Cmax]: noise
  int start[SC_MAX_CLUSTERS + 2];   // exclusive scan of cnt
  int wave[SC_WAVES];
};

__device__ __forceinline__ double scene_d2(const SceneShared& sh, double xi, double yi, double zi, double vi, int j,
                                           const SceneMetric& mt) {
#pragma clang fp contract(off)
  const double dx = xi - sh.col[0][j], dy = yi - sh.col[1][j], dz = zi - sh.col[2][j], dv = vi - sh.col[3][j];
  return dx * dx + dy * dy + mt.wz2 * dz * dz + mt.wv2 * dv * dv;
}

template <typename T>
__global__ __launch_bounds__(SC_THREADS) void scene_cluster_kernel(
    const T* __restrict__ points, long P, const int* __restrict__ offsets, int n, SceneMetric mt, int min_points, int Cmax,
    int* __restrict__ label, int* __restrict__ n_clusters, int* __restrict__ cluster_count, float* __restrict__ centroid,
    T* __restrict__ grouped, int* __restrict__ seg_off, int* __restrict__ err) {
#pragma clang fp contract(off)
  __shared__ SceneShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long f = blockIdx.x;                       // < n: the grid is exactly the frames
  const long off0 = offsets[f], off1 = offsets[f + 1];
  int* const my_cnt = cluster_count + f * Cmax;
  float* const my_cen = centroid + f * Cmax * 4;
  int* const my_seg = seg_off + f * (Cmax + 1);

  // the per-frame tables of a frame without clusters; seg_off all `row`
  auto no_clusters = [&](int row) {
    for (int e = tid; e < Cmax; e += SC_THREADS) my_cnt[e] = 0;
    for (int e = tid; e < Cmax * 4; e += SC_THREADS) my_cen[e] = 0.f;
    for (int e = tid; e <= Cmax; e += SC_THREADS) my_seg[e] = row;
    if (tid == 0) n_clusters[f] = 0;
  };
  if (off0 < 0 || off1 > P || off1 < off0) {       // uniform over the workgroup: no row of this frame is touched
    no_clusters(0);
    if (tid == 0) atomicOr(err, 1);
    return;
  }
  const T* src = points + off0 * SC_COLS;
  T* dst = grouped + off0 * SC_COLS;
  if (off1 - off0 > SC_MAX) {                      // too many detections: all noise, the rows copied as they are
    no_clusters((int)off0);
    if (tid == 0) atomicOr(err, 1);
    for (long i = off0 + tid; i < off1; i += SC_THREADS) label[i] = -1;
    for (long e = tid; e < (off1 - off0) * SC_COLS; e += SC_THREADS) dst[e] = src[e];
    return;
  }
  const int m = (int)(off1 - off0);
  if (m == 0) {                                    // nobody in view
    no_clusters((int)off0);
    return;
  }

  // stage the four used columns
  for (int e = tid; e < m * 4; e += SC_THREADS) {
    const int i = e >> 2, c = e & 3;
    sh.col[c][i] = (double)src[(long)i * SC_COLS + c];
  }
  __syncthreads();

  // core points: >= min_points neighbours, self included
  for (int i = tid; i < m; i += SC_THREADS) {
    const double xi = sh.col[0][i], yi = sh.col[1][i], zi = sh.col[2][i], vi = sh.col[3][i];
    int cnt = 0;
    for (int j = 0; j < m; ++j) cnt += scene_d2(sh, xi, yi, zi, vi, j, mt) <= mt.eps2 ? 1 : 0;
    const bool core = cnt >= min_points;
    sh.core[i] = core ? 1 : 0;
    sh.lab[i] = core ? i : SC_NONE;
  }
  __syncthreads();

  // components of the core points: at most m rounds (a round that changes something moves a label at least one hop)
  for (int round = 0; round < m; ++round) {
    int changed = 0;
    for (int i = tid; i < m; i += SC_THREADS) {
      if (!sh.core[i]) continue;
      const double xi = sh.col[0][i], yi = sh.col[1][i], zi = sh.col[2][i], vi = sh.col[3][i];
      const int mine = sh.lab[i];
      int best = mine;
      for (int j = 0; j < m; ++j) {
        const int lj = sh.lab[j];                  // SC_NONE for a point that is not core: never below best
        if (lj < best && scene_d2(sh, xi, yi, zi, vi, j, mt) <= mt.eps2) best = lj;
      }
      for (int hop = 0; hop < m; ++hop) {          // pointer jumping: a label names a core point whose label is <= it
        const int up = sh.lab[best];
        if (up >= best) break;
        best = up;
      }
      if (best < mine) {
        sh.lab[i] = best;                          // only this thread writes lab[i]
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) break;         // the workgroup-wide vote (and the barrier between rounds)
  }

  // border points: the cluster of the nearest core neighbour, the lowest index on exact ties (ascending j, strict <)
  for (int i = tid; i < m; i += SC_THREADS) {
    if (sh.core[i]) continue;
    const double xi = sh.col[0][i], yi = sh.col[1][i], zi = sh.col[2][i], vi = sh.col[3][i];
    double bd = 0.0;
    int bj = -1;
    for (int j = 0; j < m; ++j) {
      if (!sh.core[j]) continue;
      const double d2 = scene_d2(sh, xi, yi, zi, vi, j, mt);
      if (d2 <= mt.eps2 && (bj < 0 || d2 < bd)) { bd = d2; bj = j; }
    }
    if (bj >= 0) sh.lab[i] = sh.lab[bj];           // lab of a core point: final since the vote (nobody writes it here)
  }
  __syncthreads();

  // cluster ids: the rank of every root (a core point that is its own label) among the roots, ascending.  Thread t owns
  // points t * SC_PER_THREAD .. + SC_PER_THREAD - 1.
  int roots = 0;
#pragma unroll
  for (int k = 0; k < SC_PER_THREAD; ++k) {
    const int i = tid * SC_PER_THREAD + k;
    roots += (i < m && sh.core[i] && sh.lab[i] == i) ? 1 : 0;
  }
  int incl = roots;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) sh.wave[wv] = incl;
  __syncthreads();
  int before = incl - roots, total = 0;
#pragma unroll
  for (int w = 0; w < SC_WAVES; ++w) {
    const int t = sh.wave[w];
    before += w < wv ? t : 0;
    total += t;
  }
#pragma unroll
  for (int k = 0; k < SC_PER_THREAD; ++k) {
    const int i = tid * SC_PER_THREAD + k;
    if (i < m && sh.core[i] && sh.lab[i] == i) sh.cid[i] = before++;
  }
  __syncthreads();
  const int nc = total < Cmax ? total : Cmax;
  if (total > Cmax && tid == 0) atomicOr(err, 2);
  // the final label of every point: read through the root, then written over cid (a barrier between the two)
  int fin[SC_PER_THREAD];
#pragma unroll
  for (int k = 0; k < SC_PER_THREAD; ++k) {
    const int i = tid * SC_PER_THREAD + k;
    fin[k] = -1;
    if (i < m) {
      const int r = sh.lab[i];
      if (r != SC_NONE) {
        const int c = sh.cid[r];
        fin[k] = c < Cmax ? c : -1;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SC_PER_THREAD; ++k) {
    const int i = tid * SC_PER_THREAD + k;
    if (i < m) sh.cid[i] = fin[k];
  }
  __syncthreads();

  // one thread per (group, column) walks the frame in ascending order: the group's count, its fp64 column sum, and (the
  // thread of column 0) every member's rank inside the group.  Group Cmax is the noise.
  for (int e = tid; e < (Cmax + 1) * 4; e += SC_THREADS) {
    const int g = e >> 2, c = e & 3;
    const int want = g < Cmax ? g : -1;
    int cnt = 0;
    double s = 0.0;
    if (g < nc || g == Cmax) {
      for (int i = 0; i < m; ++i) {
        if (sh.cid[i] != want) continue;
        if (c == 0) sh.rank[i] = (uint16_t)cnt;
        s = cnt == 0 ? sh.col[c][i] : s + sh.col[c][i];      // np.cumsum starts from the first member: a column of -0.0 sums to -0.0
        ++cnt;
      }
    }
    if (c == 0) sh.cnt[g] = cnt;
    if (g < Cmax) {
      my_cen[g * 4 + c] = cnt > 0 ? (float)(s / (double)cnt) : 0.f;
      if (c == 0) my_cnt[g] = cnt;
    }
  }
  __syncthreads();
  if (tid == 0) {                                  // Cmax + 1 <= 65 entries: a serial scan
    int run = 0;
    for (int g = 0; g <= Cmax; ++g) {
      sh.start[g] = run;
      my_seg[g] = (int)off0 + run;
      run += sh.cnt[g];
    }
    n_clusters[f] = nc;
  }
  __syncthreads();

  for (int i = tid; i < m; i += SC_THREADS) label[off0 + i] = sh.cid[i];
  for (int e = tid; e < m * SC_COLS; e += SC_THREADS) {
    const int i = e / SC_COLS, c = e - i * SC_COLS;
    const int g = sh.cid[i] < 0 ? Cmax : sh.cid[i];
    const int row = sh.start[g] + (int)sh.rank[i];     // < m: the groups partition the frame
    if (row < m) dst[(long)row * SC_COLS + c] = src[e];
  }
}

// out rows out_off[o] .. out_off[o + 1] - 1 = src rows seg_start[o] ..: one workgroup per output frame
template <typename T>
__global__ __launch_bounds__(SC_THREADS) void gather_segments_kernel(
    const T* __restrict__ src, long P, const int* __restrict__ seg_start, const int* __restrict__ out_off, int M, long R,
    T* __restrict__ out, int* __restrict__ err) {
  const int o = blockIdx.x;                        // < M
  const long a = out_off[o], b = out_off[o + 1], s = seg_start[o];
  if (a < 0 || b < a || b > R || s < 0 || s + (b - a) > P) {      // uniform over the workgroup
    if (threadIdx.x == 0 && err != nullptr) atomicOr(err, 1);
    return;
  }
  const T* from = src + s * SC_COLS;
  T* to = out + a * SC_COLS;
  for (long e = threadIdx.x; e < (b - a) * SC_COLS; e += SC_THREADS) to[e] = from[e];
}

template <typename T>
void launch_scene_cluster(hipStream_t st, const void* points, long P, const int* offsets, int n, SceneMetric mt,
                          int min_points, int Cmax, int* label, int* n_clusters, int* cluster_count, float* centroid,
                          void* grouped, int* seg_off, int* err) {
  hipLaunchKernelGGL(scene_cluster_kernel<T>, dim3((unsigned)n), dim3(SC_THREADS), 0, st, static_cast<const T*>(points), P,
                     offsets, n, mt, min_points, Cmax, label, n_clusters, cluster_count, centroid, static_cast<T*>(grouped),
                     seg_off, err);
}

}  // namespace

extern "C" int pcaa_scene_cluster(const void* points, int points_f64, long P, const int* offsets, int n, double eps2,
                                  double wz2, double wv2, int min_points, int Cmax, int* label, int* n_clusters,
                                  int* cluster_count, float* centroid, void* grouped, int* seg_off, int* err,
                                  void* stream) {
  const char* who = "pcaa_scene_cluster";
  PCAA_CHECK_ARG(n >= 0 && P >= 0 && P < (1L << 31), "%s: needs n >= 0 and 0 <= P < 2^31", who);
  PCAA_CHECK_ARG(Cmax >= 1 && Cmax <= SC_MAX_CLUSTERS && min_points >= 1,
                 "%s: needs 1 <= Cmax <= PCAA_SCENE_MAX_CLUSTERS and min_points >= 1", who);
  PCAA_CHECK_ARG(eps2 >= 0.0 && wz2 >= 0.0 && wv2 >= 0.0 && std::isfinite(eps2) && std::isfinite(wz2) && std::isfinite(wv2),
                 "%s: eps2, wz2 and wv2 must be finite and >= 0", who);      // (a NaN fails too)
  PCAA_CHECK_ARG(err != nullptr, "%s: err is null (the kernel's only report)", who);
  if (n == 0) return PCAA_OK;
  PCAA_CHECK_ARG(offsets && n_clusters && cluster_count && centroid && seg_off, "%s: null pointer", who);
  PCAA_CHECK_ARG(P == 0 || (points && label && grouped), "%s: points / label / grouped are null", who);
  PCAA_CHECK_ARG(((uintptr_t)points % (points_f64 ? 8 : 4)) == 0 && ((uintptr_t)grouped % (points_f64 ? 8 : 4)) == 0,
                 "%s: points / grouped are misaligned", who);
  PCAA_CHECK_ARG(points != grouped || P == 0, "%s: grouped may not alias points", who);
  const SceneMetric mt{eps2, wz2, wv2};
  if (points_f64)
    launch_scene_cluster<double>(as_stream(stream), points, P, offsets, n, mt, min_points, Cmax, label, n_clusters,
                                 cluster_count, centroid, grouped, seg_off, err);
  else
    launch_scene_cluster<float>(as_stream(stream), points, P, offsets, n, mt, min_points, Cmax, label, n_clusters,
                                cluster_count, centroid, grouped, seg_off, err);
  PCAA_RETURN_LAUNCH_STATUS(who);
}

extern "C" int pcaa_gather_segments(const void* src, int src_f64, long P, const int* seg_start, const int* out_off, int M,
                                    void* out, long R, int* err, void* stream) {
  const char* who = "pcaa_gather_segments";
  PCAA_CHECK_ARG(M >= 0 && P >= 0 && R >= 0, "%s: needs M >= 0, P >= 0, R >= 0", who);
  if (M == 0) return PCAA_OK;
  PCAA_CHECK_ARG(seg_start && out_off, "%s: seg_start / out_off are null", who);
  PCAA_CHECK_ARG((R == 0 || out) && (P == 0 || src), "%s: src / out are null", who);
  PCAA_CHECK_ARG(((uintptr_t)src % (src_f64 ? 8 : 4)) == 0 && ((uintptr_t)out % (src_f64 ? 8 : 4)) == 0,
                 "%s: src / out are misaligned", who);
  if (src_f64)
    hipLaunchKernelGGL(gather_segments_kernel<double>, dim3((unsigned)M), dim3(SC_THREADS), 0, as_stream(stream),
                       static_cast<const double*>(src), P, seg_start, out_off, M, R, static_cast<double*>(out), err);
  else
    hipLaunchKernelGGL(gather_segments_kernel<float>, dim3((unsigned)M), dim3(SC_THREADS), 0, as_stream(stream),
                       static_cast<const float*>(src), P, seg_start, out_off, M, R, static_cast<float*>(out), err);
  PCAA_RETURN_LAUNCH_STATUS(who);
}
