// Open-set scoring of the PCAA inference path (reference inference_PCAA.py:129-136,
// 251-271): mixture likelihood of an embedding under K unit-covariance Gaussians in
// float64, and the k-window majority vote.
#include "common.h"

namespace {

// lik = (1/K) sum_k exp(-0.5 * (D*log(2*pi) + |x - mu_k|^2))   -- the way scipy's
// multivariate_normal(mean, eye).pdf evaluates it (exp of the log-pdf), in fp64.  One expression for every kernel that
// scores an embedding (joint_likelihood_kernel, stream_score_kernel): same operations in the same order, same bits.
__device__ __forceinline__ double mixture_likelihood(const float* __restrict__ x, const float* __restrict__ means, int K,
                                                     int D) {
  const double log2pi = 1.8378770664093453;
  double acc = 0.0;
  for (int k = 0; k < K; ++k) {
    double maha = 0.0;
    for (int d = 0; d < D; ++d) {
      const double diff = (double)x[d] - (double)means[(long)k * D + d];
      maha += diff * diff;
    }
    acc += exp(-0.5 * ((double)D * log2pi + maha));
  }
  return acc / (double)K;
}

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
    for (int i = 0; i < k; ++i) cnt += get(i).pred == c ? 1 : 0;
    if (cnt > best_count) { best_count = cnt; best = c; }
  }
  return best;
}

struct Scored {
  double lik;
  long long pred;
};

__global__ void kvote_kernel(const double* __restrict__ lik, const long long* __restrict__ preds, double thr,
                             int k, int n_labels, int n_classes, int nwin, long long* __restrict__ out) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nwin) return;
  out[w] = vote_of([&](int i) { return Scored{lik[(long)w * k + i], preds[(long)w * k + i]}; }, thr, k, n_labels,
                   n_classes);
}

// One tick of a multi-stream scorer: argmax, likelihood, vote state and votes of its nw windows.  The windows of one
// stream are a contiguous, ascending run of the tick's arrays; one workgroup takes one run (run_start[r] .. run_start[r +
// 1]), so everything a vote needs from this tick was written by the same workgroup and the per-stream history (the
// stream's current, incomplete vote group: slot j % k holds window j) has one reader and one writer per launch:
//   1. every window: preds (first maximal softmax probability, the rule of cross_entropy_kernel) and lik;
//   2. every window with j % k == k - 1: the vote of group j / k from its k - 1 predecessors -- those of this run from the
//      arrays phase 1 wrote, older ones from the history -- to votes[vote_pos];
//   3. the run's last k windows: their history slot (two windows k apart share a slot; only the later one is among them).
// The barriers order the phases: a slot phase 2 reads for an old window may be the one phase 3 overwrites.
struct StreamScoreParams {
  const float* logits;          // [nw, K]
  const float* sup_fv;          // [nw, D]
  const float* means;           // [Kc, D]
  const int* run_start;         // [n_runs + 1]
  const int* win_stream;        // [nw]
  const int* win_j;             // [nw]
  const int* vote_pos;          // [nw], < 0: the window completes no group
  double* hist_lik;             // [max_streams, k]
  long long* hist_pred;         // [max_streams, k]
  long long* preds;             // [nw]
  double* lik;                  // [nw]
  long long* votes;             // [n_votes]
  double thr;
  int nw, K, D, Kc, k, n_labels, n_classes, max_streams, n_votes;
};

__global__ __launch_bounds__(64) void stream_score_kernel(StreamScoreParams p) {
  const int i0 = p.run_start[blockIdx.x], i1 = p.run_start[blockIdx.x + 1];
  if (i0 < 0 || i1 > p.nw || i0 >= i1) return;                  // (uniform: the whole workgroup leaves)
  const int s = p.win_stream[i0];
  if (s < 0 || s >= p.max_streams) return;
  const int k = p.k;
  double* hl = p.hist_lik + (long)s * k;
  long long* hp = p.hist_pred + (long)s * k;
  for (int i = i0 + threadIdx.x; i < i1; i += 64) {
    const float* x = p.logits + (long)i * p.K;
    float mx = x[0];
    for (int c = 1; c < p.K; ++c) mx = fmaxf(mx, x[c]);
    float se = 0.f;
    for (int c = 0; c < p.K; ++c) se += expf(x[c] - mx);
    int am = 0;
    float pbest = -1.f;
    for (int c = 0; c < p.K; ++c) {
      const float pk = expf(x[c] - mx) / se;   // softmax exactly as exp / sum
      if (pk > pbest) { pbest = pk; am = c; }  // first index on ties
    }
    p.preds[i] = am;
    p.lik[i] = mixture_likelihood(p.sup_fv + (long)i * p.D, p.means, p.Kc, p.D);
  }
  __syncthreads();
  for (int i = i0 + threadIdx.x; i < i1; i += 64) {
    const int j = p.win_j[i], pos = p.vote_pos[i];
    if (j < 0 || j % k != k - 1 || pos < 0 || pos >= p.n_votes) continue;
    p.votes[pos] = vote_of(
        [&](int m) {
          const int im = i - (k - 1) + m;                         // window j - (k - 1) + m
          if (im >= i0) return Scored{p.lik[im], p.preds[im]};
          return Scored{hl[m], hp[m]};                            // (j - (k - 1) + m) % k == m
        },
        p.thr, k, p.n_labels, p.n_classes);
  }
  __syncthreads();
  for (int i = max(i0, i1 - k) + threadIdx.x; i < i1; i += 64) {
    const int j = p.win_j[i];
    if (j < 0) continue;
    hl[j % k] = p.lik[i];
    hp[j % k] = p.preds[i];
  }
}

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
  StreamScoreParams p{logits, sup_fv, means, run_start, win_stream, win_j, vote_pos, hist_lik, hist_pred, preds, lik, votes,
                      threshold, nw, K, D, Kc, k, n_labels, n_classes, max_streams, n_votes};
  hipLaunchKernelGGL(stream_score_kernel, dim3((unsigned)n_runs), dim3(64), 0, as_stream(stream), p);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_stream_score");
}
