// The open-set scoring rule, written once: the per-window arithmetic every scoring kernel shares and the tick of a
// multi-stream scorer, with the prior-only (scoring.hip: PriorTick) and prior-plus-gallery (gallery.hip: GalleryTick)
// variants as two policies of one body.
#pragma once
#include "common.h"

namespace {

// |x - c|^2 in fp64
__device__ __forceinline__ double maha_of(const float* __restrict__ x, const float* __restrict__ c, int D) {
  double maha = 0.0;
  for (int d = 0; d < D; ++d) {
    const double diff = (double)x[d] - (double)c[d];
    maha += diff * diff;
  }
  return maha;
}

// its term exp(-0.5 * (D*log(2*pi) + maha)) -- the way scipy's multivariate_normal(mean, eye).pdf evaluates it (exp of
// the log-pdf)
__device__ __forceinline__ double term_of(double maha, int D) {
  const double log2pi = 1.8378770664093453;
  return exp(-0.5 * ((double)D * log2pi + maha));
}

// lik = (1/K) sum_k term_k, added in ascending k from +0.0, in fp64.  One expression for every kernel that scores an
// embedding against the prior alone (joint_likelihood_kernel, PriorTick): same operations in the same order, same
// bits; wave_score (gallery.hip) adds the same terms in the same order.
__device__ __forceinline__ double mixture_likelihood(const float* __restrict__ x, const float* __restrict__ means, int K,
                                                     int D) {
  double acc = 0.0;
  for (int k = 0; k < K; ++k) acc += term_of(maha_of(x, means + (long)k * D, D), D);
  return acc / (double)K;
}

// the first maximal softmax probability of K logits (the rule of cross_entropy_kernel)
__device__ __forceinline__ int softmax_argmax(const float* x, int K) {
  float mx = x[0];
  for (int c = 1; c < K; ++c) mx = fmaxf(mx, x[c]);
  float se = 0.f;
  for (int c = 0; c < K; ++c) se += expf(x[c] - mx);
  int am = 0;
  float pbest = -1.f;
  for (int c = 0; c < K; ++c) {
    const float pk = expf(x[c] - mx) / se;   // softmax exactly as exp / sum
    if (pk > pbest) { pbest = pk; am = c; }  // first index on ties
  }
  return am;
}

// what a vote reads of one window
struct Scored {
  double lik;
  long long label;
};

struct TickParams {
  const float* logits;          // [nw, K]
  const float* sup_fv;          // [nw, D]
  const float* means;           // [Kc, D]
  const int* run_start;         // [n_runs + 1]
  const int* win_stream;        // [nw]
  const int* win_j;             // [nw]
  const int* vote_pos;          // [nw], < 0: the window completes no group
  double* hist_lik;             // [max_streams, k]
  long long* hist_label;        // [max_streams, k]
  long long* labels;            // [nw]
  double* lik;                  // [nw]
  long long* votes;             // [n_votes]
  double thr;
  int nw, K, D, Kc, k, n_labels, max_streams, n_votes;
};

// One tick of a multi-stream scorer: label, likelihood, vote state and votes of its nw windows.  The windows of one
// stream are a contiguous, ascending run of the tick's arrays; one workgroup takes one run (run_start[r] .. run_start[r +
// 1]), so everything a vote needs from this tick was written by the same workgroup and the per-stream history (the
// stream's current, incomplete vote group: slot j % k holds window j) has one reader and one writer per launch:
//   1. P::score -- every window of the run: labels and lik;
//   2. every window with j % k == k - 1: P::vote, the vote of group j / k from its k - 1 predecessors -- those of this
//      run from the arrays phase 1 wrote, older ones from the history -- to votes[vote_pos];
//   3. the run's last k windows: their history slot (two windows k apart share a slot; only the later one is among them);
//      then P::keep, whatever else the policy keeps of the run.
// The barriers order the phases: a slot phase 2 reads for an old window may be the one phase 3 overwrites.
// A policy P: THREADS (the workgroup), Params (TickParams and its own), score(p, i0, i1), vote(p, get) with get(m) ->
// Scored of the group's m-th window, keep(p, s, i0, i1).
template <class P>
__global__ __launch_bounds__(P::THREADS) void stream_tick_kernel(typename P::Params p) {
  const int i0 = p.run_start[blockIdx.x], i1 = p.run_start[blockIdx.x + 1];
  if (i0 < 0 || i1 > p.nw || i0 >= i1) return;                  // (uniform: the whole workgroup leaves)
  const int s = p.win_stream[i0];
  if (s < 0 || s >= p.max_streams) return;
  const int k = p.k, nt = P::THREADS, tid = threadIdx.x;
  double* hl = p.hist_lik + (long)s * k;
  long long* hp = p.hist_label + (long)s * k;
  P::score(p, i0, i1);
  __syncthreads();
  for (int i = i0 + tid; i < i1; i += nt) {
    const int j = p.win_j[i], pos = p.vote_pos[i];
    if (j < 0 || j % k != k - 1 || pos < 0 || pos >= p.n_votes) continue;
    p.votes[pos] = P::vote(p, [&](int m) {
      const int im = i - (k - 1) + m;                             // window j - (k - 1) + m
      if (im >= i0) return Scored{p.lik[im], p.labels[im]};
      return Scored{hl[m], hp[m]};                                // (j - (k - 1) + m) % k == m
    });
  }
  __syncthreads();
  for (int i = max(i0, i1 - k) + tid; i < i1; i += nt) {
    const int j = p.win_j[i];
    if (j < 0) continue;
    hl[j % k] = p.lik[i];
    hp[j % k] = p.labels[i];
  }
  P::keep(p, s, i0, i1);
}

}  // namespace
