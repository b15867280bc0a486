// Open-set scoring of the PCAA inference path (reference inference_PCAA.py:129-136,
// 251-271): mixture likelihood of an embedding under K unit-covariance Gaussians in
// float64, and the k-window majority vote.
#include "score_tick.h"

namespace {

__global__ void joint_likelihood_kernel(const float* __restrict__ x, const float* __restrict__ means,
                                        int B, int K, int D, double* __restrict__ lik) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  lik[b] = mixture_likelihood(x + (long)b * D, means, K, D);
}

// window w = crops [w*k, (w+1)*k): known iff #(lik > thr) > k/2, then the most frequent
// predicted label over ALL n_classes encoder outputs (lowest label on ties, like argmax(bincount)), else
// n_labels (= unknown; the number of labels present in the known test split)
// the vote of one group of k windows; get(i) -> (lik, pred) of its i-th window
template <typename Get>
__device__ __forceinline__ long long vote_of(Get get, double thr, int k, int n_labels, int n_classes) {
  int above = 0;
  for (int i = 0; i < k; ++i) above += get(i).lik > thr ? 1 : 0;
  if (2 * above <= k) return n_labels;
  int best = 0, best_count = -1;
  for (int c = 0; c < n_classes; ++c) {
    int cnt = 0;
    for (int i = 0; i < k; ++i) cnt += get(i).label == c ? 1 : 0;
    if (cnt > best_count) { best_count = cnt; best = c; }
  }
  return best;
}

__global__ void kvote_kernel(const double* __restrict__ lik, const long long* __restrict__ preds, double thr,
                             int k, int n_labels, int n_classes, int nwin, long long* __restrict__ out) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nwin) return;
  out[w] = vote_of([&](int i) { return Scored{lik[(long)w * k + i], preds[(long)w * k + i]}; }, thr, k, n_labels,
                   n_classes);
}

// the tick (score_tick.h) under the prior alone: one thread scores one window, the vote counts over the classifier's
// n_classes outputs
struct PriorTick {
  static constexpr int THREADS = 64;
  struct Params : TickParams {
    int n_classes;
  };
  static __device__ __forceinline__ void score(const Params& p, int i0, int i1) {
    for (int i = i0 + threadIdx.x; i < i1; i += THREADS) {
      p.labels[i] = softmax_argmax(p.logits + (long)i * p.K, p.K);
      p.lik[i] = mixture_likelihood(p.sup_fv + (long)i * p.D, p.means, p.Kc, p.D);
    }
  }
  template <typename Get>
  static __device__ __forceinline__ long long vote(const Params& p, Get get) {
    return vote_of(get, p.thr, p.k, p.n_labels, p.n_classes);
  }
  static __device__ __forceinline__ void keep(const Params&, int, int, int) {}
};

}  // namespace

extern "C" int pcaa_joint_likelihood(const float* x, const float* means, int B, int K, int D, double* lik,
                                     void* stream) {
  PCAA_CHECK_ARG(x && means && lik && B >= 1 && K >= 1 && D >= 1, "pcaa_joint_likelihood: bad args");
  hipLaunchKernelGGL(joint_likelihood_kernel, dim3((unsigned)cdiv(B, 128)), dim3(128), 0, as_stream(stream), x,
                     means, B, K, D, lik);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_joint_likelihood");
}

extern "C" int pcaa_kvote(const double* lik, const long long* preds, double threshold, int k, int n_labels,
                          int n_classes, int n_windows, long long* out, void* stream) {
  PCAA_CHECK_ARG(lik && preds && out && k >= 1 && n_labels >= 1 && n_classes >= 1 && n_windows >= 1,
                 "pcaa_kvote: bad args");
  hipLaunchKernelGGL(kvote_kernel, dim3((unsigned)cdiv(n_windows, 128)), dim3(128), 0, as_stream(stream), lik, preds,
                     threshold, k, n_labels, n_classes, n_windows, out);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_kvote");
}

extern "C" int pcaa_stream_score(const float* logits, const float* sup_fv, const float* means, const int* run_start,
                                 int n_runs, const int* win_stream, const int* win_j, const int* vote_pos, int nw, int K,
                                 int D, int Kc, double threshold, int k, int n_labels, int n_classes, double* hist_lik,
                                 long long* hist_pred, int max_streams, long long* preds, double* lik, long long* votes,
                                 int n_votes, void* stream) {
  PCAA_CHECK_ARG(logits && sup_fv && means && run_start && win_stream && win_j && vote_pos && hist_lik && hist_pred &&
                 preds && lik, "pcaa_stream_score: null pointer");
  PCAA_CHECK_ARG(nw >= 1 && n_runs >= 1 && n_runs <= nw && K >= 1 && D >= 1 && Kc >= 1 && k >= 1 && n_labels >= 1 &&
                 n_classes >= 1 && max_streams >= 1 && n_votes >= 0 && (votes != nullptr || n_votes == 0),
                 "pcaa_stream_score: bad args");
  PriorTick::Params p{{logits, sup_fv, means, run_start, win_stream, win_j, vote_pos, hist_lik, hist_pred, preds, lik, votes,
                       threshold, nw, K, D, Kc, k, n_labels, max_streams, n_votes}, n_classes};
  hipLaunchKernelGGL(stream_tick_kernel<PriorTick>, dim3((unsigned)n_runs), dim3(PriorTick::THREADS), 0, as_stream(stream),
                     p);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_stream_score");
}
