// Run-time enrolment: a gallery of modes beside the prior's.  A person seen for a few windows gets
// a mode of their own -- the centroid of their embeddings under the same unit covariance -- and the open-set rule of
// scoring.hip recognises them from then on:
//   lik   = (acc_prior + acc_gallery) / Kc       acc_prior: the sum pcaa_joint_likelihood forms, same order, same bits;
//                                                acc_gallery: the same term over the live slots (counts[e] > 0)
//   near  = the mode of smallest fp64 squared distance among 0 .. Kc + E - 1 (lowest index on exact ties)
//   label = preds                 when near < Kc   (a trained class: the classifier names it)
//           n_labels + 1 + slot   otherwise        (n_labels itself stays "unknown")
// One wavefront scores one window: lanes stride the modes, every lane forms one mode's term with the maha_of / term_of
// that mixture_likelihood is written in (score_tick.h), and the partials meet in a fixed order -- a window's outputs are a
// function of the window and the gallery alone, whatever the batch, its position or the grid.  The live tick is the
// shared body stream_tick_kernel (score_tick.h) under the GalleryTick policy below.
#include "score_tick.h"

namespace {

constexpr int WAVE = 64;
constexpr int SCORE_WAVES = 4;        // windows per workgroup of gallery_score_kernel / waves of a stream run

struct GalleryView {
  const float* centroids;   // [E_max, D]
  const int* counts;        // [E_max]
  int E;                    // slots 0 .. E - 1 are scanned
};

struct Nearest {
  double d2;
  int idx;
};
__device__ __forceinline__ bool closer(double d2, int idx, const Nearest& n) {
  return d2 < n.d2 || (d2 == n.d2 && idx < n.idx);
}

// One window by one wavefront (all 64 lanes call it) -> lik and near, valid in every lane.
__device__ __forceinline__ void wave_score(const float* __restrict__ x, const float* __restrict__ means, int Kc, int D,
                                           const GalleryView& g, double& lik, int& near) {
  const int lane = threadIdx.x & (WAVE - 1);
  Nearest best{__builtin_inf(), 0x7fffffff};
  // prior modes: 64 terms at a time, then added one by one in ascending k from +0.0, as mixture_likelihood adds them
  double acc_prior = 0.0;
  for (int k0 = 0; k0 < Kc; k0 += WAVE) {
    const int k = k0 + lane;
    double t = 0.0;
    if (k < Kc) {
      const double maha = maha_of(x, means + (long)k * D, D);
      t = term_of(maha, D);
      if (closer(maha, k, best)) best = Nearest{maha, k};
    }
    const int n = min(WAVE, Kc - k0);
    for (int i = 0; i < n; ++i) acc_prior += __shfl(t, i, WAVE);
  }
  // gallery slots: every lane adds its own live slots in ascending order from +0.0, the 64 partials meet in the fixed
  // butterfly of wave_sum_d
  double acc_g = 0.0;
  for (int e = lane; e < g.E; e += WAVE) {
    if (g.counts[e] <= 0) continue;
    const double maha = maha_of(x, g.centroids + (long)e * D, D);
    acc_g += term_of(maha, D);
    if (closer(maha, Kc + e, best)) best = Nearest{maha, Kc + e};
  }
  acc_g = wave_sum_d(acc_g);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double od = __shfl_xor(best.d2, o, WAVE);
    const int oi = __shfl_xor(best.idx, o, WAVE);
    if (closer(od, oi, best)) best = Nearest{od, oi};
  }
  lik = (acc_prior + acc_g) / (double)Kc;
  near = best.idx == 0x7fffffff ? 0 : best.idx;       // (every distance NaN: mode 0)
}

__device__ __forceinline__ long long label_of(long long pred, int near, int Kc, int n_labels) {
  return near < Kc ? pred : (long long)n_labels + 1 + (near - Kc);
}

__global__ __launch_bounds__(WAVE* SCORE_WAVES) void gallery_score_kernel(
    const float* __restrict__ sup_fv, const long long* __restrict__ preds, const float* __restrict__ means, int B, int Kc,
    int D, GalleryView g, int n_labels, double* __restrict__ lik, long long* __restrict__ labels, int* __restrict__ near) {
  const int b = blockIdx.x * SCORE_WAVES + (threadIdx.x / WAVE);      // (uniform per wavefront)
  if (b >= B) return;
  double l;
  int nr;
  wave_score(sup_fv + (long)b * D, means, Kc, D, g, l, nr);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    lik[b] = l;
    near[b] = nr;
    labels[b] = label_of(preds[b], nr, Kc, n_labels);
  }
}

// the rule of vote_of (scoring.hip) over arbitrary labels: known iff #(lik > thr) > k/2, then the most frequent label of
// the k windows, the lowest on ties (argmax(bincount)), else n_labels
template <typename Get>
__device__ __forceinline__ long long gallery_vote_of(Get get, double thr, int k, int n_labels) {
  int above = 0;
  for (int i = 0; i < k; ++i) above += get(i).lik > thr ? 1 : 0;
  if (2 * above <= k) return n_labels;
  long long best = 0;
  int best_count = 0;
  for (int i = 0; i < k; ++i) {
    const long long li = get(i).label;
    int cnt = 0;
    for (int m = 0; m < k; ++m) cnt += get(m).label == li ? 1 : 0;
    if (cnt > best_count || (cnt == best_count && li < best)) { best_count = cnt; best = li; }
  }
  return best;
}

__global__ void gallery_kvote_kernel(const double* __restrict__ lik, const long long* __restrict__ labels, double thr,
                                     int k, int n_labels, int nwin, long long* __restrict__ out) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nwin) return;
  out[w] = gallery_vote_of([&](int i) { return Scored{lik[(long)w * k + i], labels[(long)w * k + i]}; }, thr, k, n_labels);
}

// sums[slot] += fv[rows[i]] for i = 0 .. m - 1 in that order (thread d owns column d: plain fp64 adds, no atomics), then
// the count and the centroid.  One workgroup.
__global__ __launch_bounds__(256) void gallery_accumulate_kernel(
    const float* __restrict__ fv, int n_rows, int D, const int* __restrict__ rows, int m, int slot,
    double* __restrict__ sums, int* __restrict__ counts, float* __restrict__ centroids, int* __restrict__ err_flag) {
  const int before = counts[slot];
  int added = 0;
  for (int i = 0; i < m; ++i) {
    const int r = rows ? rows[i] : i;
    if (r >= 0 && r < n_rows) ++added;
  }
  if (added != m && threadIdx.x == 0 && err_flag) *err_flag = 1;
  const int total = (before > 0 ? before : 0) + added;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    double s = before > 0 ? sums[(long)slot * D + d] : 0.0;       // (a free slot starts from +0.0 whatever it held)
    for (int i = 0; i < m; ++i) {
      const int r = rows ? rows[i] : i;
      if (r < 0 || r >= n_rows) continue;
      s += (double)fv[(long)r * D + d];
    }
    sums[(long)slot * D + d] = s;
    if (total > 0) centroids[(long)slot * D + d] = (float)(s / (double)total);
  }
  __syncthreads();                                               // every thread has read counts[slot]
  if (threadIdx.x == 0) counts[slot] = total;
}

// the tick (score_tick.h) with this score and this vote: one workgroup of SCORE_WAVES wavefronts per run.  Phase 1 gives
// every window to one wavefront (wave_score); after phase 3 the run's last H embeddings also stay in the stream's ring
// fv_hist (slot j % H).
struct GalleryTick {
  static constexpr int THREADS = WAVE * SCORE_WAVES;
  struct Params : TickParams {
    float* fv_hist;               // [max_streams * H, D] (H > 0)
    int* near;                    // [nw]
    GalleryView g;
    int H;
  };
  static __device__ __forceinline__ void score(const Params& p, int i0, int i1) {
    const int tid = threadIdx.x;
    for (int i = i0 + tid / WAVE; i < i1; i += SCORE_WAVES) {      // (uniform per wavefront)
      const int am = softmax_argmax(p.logits + (long)i * p.K, p.K);
      double l;
      int nr;
      wave_score(p.sup_fv + (long)i * p.D, p.means, p.Kc, p.D, p.g, l, nr);
      if ((tid & (WAVE - 1)) == 0) {
        p.lik[i] = l;
        p.near[i] = nr;
        p.labels[i] = label_of(am, nr, p.Kc, p.n_labels);
      }
    }
  }
  template <typename Get>
  static __device__ __forceinline__ long long vote(const Params& p, Get get) {
    return gallery_vote_of(get, p.thr, p.k, p.n_labels);
  }
  static __device__ __forceinline__ void keep(const Params& p, int s, int i0, int i1) {
    if (p.H <= 0) return;
    const int a = max(i0, i1 - p.H);                                // two windows H apart share a slot: the later one only
    for (long e = threadIdx.x; e < (long)(i1 - a) * p.D; e += THREADS) {
      const int i = a + (int)(e / p.D), d = (int)(e % p.D), j = p.win_j[i];
      if (j < 0) continue;
      p.fv_hist[((long)s * p.H + j % p.H) * p.D + d] = p.sup_fv[(long)i * p.D + d];
    }
  }
};

}  // namespace

extern "C" int pcaa_gallery_accumulate(const float* fv, int n_rows, int D, const int* rows, int m, int slot, int E_max,
                                       double* sums, int* counts, float* centroids, int* err_flag, void* stream) {
  PCAA_CHECK_ARG(fv && sums && counts && centroids, "pcaa_gallery_accumulate: null pointer");
  PCAA_CHECK_ARG(n_rows >= 1 && D >= 1 && m >= 1 && E_max >= 1 && slot >= 0 && slot < E_max && (rows || m <= n_rows),
                 "pcaa_gallery_accumulate: bad args");
  hipLaunchKernelGGL(gallery_accumulate_kernel, dim3(1), dim3(256), 0, as_stream(stream), fv, n_rows, D, rows, m, slot,
                     sums, counts, centroids, err_flag);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_gallery_accumulate");
}

extern "C" int pcaa_gallery_score(const float* sup_fv, const long long* preds, const float* means, int B, int Kc, int D,
                                  const float* centroids, const int* counts, int E, int n_labels, double* lik,
                                  long long* labels, int* near, void* stream) {
  PCAA_CHECK_ARG(sup_fv && preds && means && lik && labels && near, "pcaa_gallery_score: null pointer");
  PCAA_CHECK_ARG(B >= 1 && Kc >= 1 && D >= 1 && n_labels >= 1 && E >= 0 && (E == 0 || (centroids && counts)) &&
                 (long)Kc + E < 0x7fffffffL, "pcaa_gallery_score: bad args");
  hipLaunchKernelGGL(gallery_score_kernel, dim3((unsigned)cdiv(B, SCORE_WAVES)), dim3(WAVE * SCORE_WAVES), 0,
                     as_stream(stream), sup_fv, preds, means, B, Kc, D, GalleryView{centroids, counts, E}, n_labels, lik,
                     labels, near);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_gallery_score");
}

extern "C" int pcaa_gallery_kvote(const double* lik, const long long* labels, double threshold, int k, int n_labels,
                                  int n_windows, long long* out, void* stream) {
  PCAA_CHECK_ARG(lik && labels && out && k >= 1 && n_labels >= 1 && n_windows >= 1, "pcaa_gallery_kvote: bad args");
  hipLaunchKernelGGL(gallery_kvote_kernel, dim3((unsigned)cdiv(n_windows, 128)), dim3(128), 0, as_stream(stream), lik,
                     labels, threshold, k, n_labels, n_windows, out);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_gallery_kvote");
}

extern "C" int pcaa_stream_score_gallery(const float* logits, const float* sup_fv, const float* means,
                                         const int* run_start, int n_runs, const int* win_stream, const int* win_j,
                                         const int* vote_pos, int nw, int K, int D, int Kc, double threshold, int k,
                                         int n_labels, const float* centroids, const int* counts, int E,
                                         double* hist_lik, long long* hist_label, int max_streams, float* fv_hist, int H,
                                         long long* labels, double* lik, int* near, long long* votes, int n_votes,
                                         void* stream) {
  PCAA_CHECK_ARG(logits && sup_fv && means && run_start && win_stream && win_j && vote_pos && hist_lik && hist_label &&
                 labels && lik && near, "pcaa_stream_score_gallery: null pointer");
  PCAA_CHECK_ARG(nw >= 1 && n_runs >= 1 && n_runs <= nw && K >= 1 && D >= 1 && Kc >= 1 && k >= 1 && n_labels >= 1 &&
                 max_streams >= 1 && n_votes >= 0 && (votes != nullptr || n_votes == 0) && E >= 0 &&
                 (E == 0 || (centroids && counts)) && (long)Kc + E < 0x7fffffffL && H >= 0 && (H == 0 || fv_hist),
                 "pcaa_stream_score_gallery: bad args");
  GalleryTick::Params p{{logits, sup_fv, means, run_start, win_stream, win_j, vote_pos, hist_lik, hist_label, labels, lik,
                         votes, threshold, nw, K, D, Kc, k, n_labels, max_streams, n_votes},
                        fv_hist, near, GalleryView{centroids, counts, E}, H};
  hipLaunchKernelGGL(stream_tick_kernel<GalleryTick>, dim3((unsigned)n_runs), dim3(GalleryTick::THREADS), 0,
                     as_stream(stream), p);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_stream_score_gallery");
}
