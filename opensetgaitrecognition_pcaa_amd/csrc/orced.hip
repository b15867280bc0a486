// OR-CED baseline heads (reference models.py:446-505, train_ORCED.py:143-176, utils.py:72-85) on the device:
//
//   vae_mu     = MLP_mu(x4)      = x4 . Wmu^T + bmu            [B, L]     (L = SUP_LATENT_DIM = 32, x4 [B, 512])
//   vae_logvar = MLP_logvar(x4)  = x4 . Wlv^T + blv            [B, L]
//   sup_fv     = vae_mu + eps * exp(0.5 * vae_logvar)           (eps: the caller's randn draw, [B, L])
//   logits     = MLP_classification(sup_fv) = sup_fv . Wc^T + bc   [B, K]   (no activation anywhere)
//
// and  KL( N(mu, exp(logvar)) || N(mu_k, I) )  averaged over the batch.  Everything here is [B, 32]-sized: one
// workgroup per batch row, fp32 FMAs, the row of x4 staged in LDS.  Round 2 ran these as stock torch ops.
// Further down: the triplet term (pcaa_orced_triplet) and the open-set rule (pcaa_orced_ood), the same sizes.
#include "common.h"

namespace {

constexpr int MAX_IN = 1024, MAX_LAT = 128, MAX_K = 64;

// one wave: dot(w[0..n), x[0..n)) with x in LDS
__device__ __forceinline__ float wave_dot(const float* __restrict__ w, const float* xs, int n, int lane) {
  float a = 0.f;
  for (int k = lane; k < n; k += 64) a = fmaf(w[k], xs[k], a);
  return wave_sum(a);
}

__global__ __launch_bounds__(256) void orced_heads_fwd_kernel(const float* __restrict__ x4, const float* __restrict__ Wmu,
                                                              const float* __restrict__ bmu, const float* __restrict__ Wlv,
                                                              const float* __restrict__ blv, const float* __restrict__ eps,
                                                              const float* __restrict__ Wc, const float* __restrict__ bc,
                                                              float* mu, float* logvar, float* sup_fv, float* logits,
                                                              int K, int d_in, int L) {
  __shared__ float xs[MAX_IN];
  __shared__ float ml[2 * MAX_LAT];
  __shared__ float ss[MAX_LAT];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int k = tid; k < d_in; k += 256) xs[k] = x4[(long)b * d_in + k];
  __syncthreads();
  for (int o = wave; o < 2 * L; o += 4) {
    const bool is_mu = o < L;
    const int j = is_mu ? o : o - L;
    const float v = wave_dot((is_mu ? Wmu : Wlv) + (long)j * d_in, xs, d_in, lane) + (is_mu ? bmu[j] : blv[j]);
    if (lane == 0) ml[o] = v;
  }
  __syncthreads();
  if (tid < L) {
    const float m = ml[tid], lv = ml[L + tid];
    const float s = m + eps[(long)b * L + tid] * expf(0.5f * lv);
    mu[(long)b * L + tid] = m;
    logvar[(long)b * L + tid] = lv;
    sup_fv[(long)b * L + tid] = s;
    ss[tid] = s;
  }
  __syncthreads();
  if (tid < K) {
    float a = bc[tid];
    for (int j = 0; j < L; ++j) a = fmaf(Wc[tid * L + j], ss[j], a);
    logits[(long)b * K + tid] = a;
  }
}

// per row: the gradients that reach mu and logvar (into ws[0][B][L], ws[1][B][L]) and dx4
__global__ __launch_bounds__(256) void orced_heads_bwd_rows_kernel(const float* __restrict__ eps,
                                                                   const float* __restrict__ logvar,
                                                                   const float* __restrict__ Wmu,
                                                                   const float* __restrict__ Wlv,
                                                                   const float* __restrict__ Wc,
                                                                   const float* __restrict__ d_logits,
                                                                   const float* __restrict__ d_sup,
                                                                   const float* __restrict__ d_mu,
                                                                   const float* __restrict__ d_logvar, float* ws,
                                                                   float* dx4, int B, int K, int d_in, int L) {
  __shared__ float dm[MAX_LAT], dl[MAX_LAT];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < L) {
    float ds = d_sup ? d_sup[(long)b * L + tid] : 0.f;
    if (d_logits)
      for (int k = 0; k < K; ++k) ds = fmaf(Wc[k * L + tid], d_logits[(long)b * K + k], ds);
    const float lv = logvar[(long)b * L + tid];
    const float gm = (d_mu ? d_mu[(long)b * L + tid] : 0.f) + ds;
    const float gl = (d_logvar ? d_logvar[(long)b * L + tid] : 0.f) + ds * eps[(long)b * L + tid] * 0.5f * expf(0.5f * lv);
    dm[tid] = gm;
    dl[tid] = gl;
    ws[(long)b * L + tid] = gm;
    ws[(long)(B + b) * L + tid] = gl;
  }
  __syncthreads();
  if (dx4 != nullptr) {
    for (int k = tid; k < d_in; k += 256) {
      float a = 0.f;
      for (int j = 0; j < L; ++j) a = fmaf(Wmu[(long)j * d_in + k], dm[j], fmaf(Wlv[(long)j * d_in + k], dl[j], a));
      dx4[(long)b * d_in + k] = a;
    }
  }
}

// weight / bias gradients: block o < 2L: row o of dWmu (o < L) or dWlv; block 2L: dWc and dbc
__global__ __launch_bounds__(256) void orced_heads_bwd_params_kernel(const float* __restrict__ x4,
                                                                     const float* __restrict__ sup_fv,
                                                                     const float* __restrict__ d_logits,
                                                                     const float* __restrict__ ws, float* dWmu, float* dbmu,
                                                                     float* dWlv, float* dblv, float* dWc, float* dbc, int B,
                                                                     int K, int d_in, int L) {
  const int o = blockIdx.x, tid = threadIdx.x;
  if (o < 2 * L) {
    const bool is_mu = o < L;
    const int j = is_mu ? o : o - L;
    const float* g = ws + (is_mu ? 0 : (long)B * L) + j;      // g[b * L]
    float* dW = (is_mu ? dWmu : dWlv) + (long)j * d_in;
    for (int k = tid; k < d_in; k += 256) {
      float a = 0.f;
      for (int b = 0; b < B; ++b) a = fmaf(g[(long)b * L], x4[(long)b * d_in + k], a);
      dW[k] = a;
    }
    if (tid == 0) {
      float a = 0.f;
      for (int b = 0; b < B; ++b) a += g[(long)b * L];
      (is_mu ? dbmu : dblv)[j] = a;
    }
  } else {
    for (int i = tid; i < K * L; i += 256) {
      const int k = i / L, j = i - k * L;
      float a = 0.f;
      if (d_logits)
        for (int b = 0; b < B; ++b) a = fmaf(d_logits[(long)b * K + k], sup_fv[(long)b * L + j], a);
      dWc[i] = a;
    }
    if (tid < K) {
      float a = 0.f;
      if (d_logits)
        for (int b = 0; b < B; ++b) a += d_logits[(long)b * K + tid];
      dbc[tid] = a;
    }
  }
}

// loss = mean_b( -0.5 sum_j (1 + lv - (mu - mk)^2 - exp(lv)) ); gradients scaled by gscale / B
__global__ __launch_bounds__(256) void orced_kl_kernel(const float* __restrict__ mu, const float* __restrict__ logvar,
                                                       const float* __restrict__ mu_k, float* loss, float* d_mu,
                                                       float* d_logvar, float* d_muk, float gscale, int B, int L) {
  __shared__ double red[4];
  const int tid = threadIdx.x, n = B * L;
  double acc = 0.0;
  const float gs = gscale / (float)B;
  for (int i = tid; i < n; i += 256) {
    const float m = mu[i], lv = logvar[i], d = m - mu_k[i], e = expf(lv);
    acc += (double)(1.f + lv - d * d - e);
    if (d_mu) d_mu[i] = gs * d;
    if (d_muk) d_muk[i] = -gs * d;
    if (d_logvar) d_logvar[i] = gs * (-0.5f) * (1.f - e);
  }
  acc = wave_sum_d(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0 && loss) *loss = (float)(-0.5 * ((red[0] + red[1]) + (red[2] + red[3])) / (double)B);
}

// ---------------------------------------------------------------------------------------------------------------------
// Triplet term (train_ORCED.py:9,30,34: MultiSimilarityMiner(epsilon) feeding TripletMarginLoss(margin), restated in
// orced.py) in dense form, three launches, no atomics, no host read:
//   e = x / max(|x|, 1e-12), S = e e^T, D[a,j] = |e_a - e_j|
//   P[a,p] = same label, p != a, S[a,p] - eps < max_neg S[a,.]     N[a,n] = other label, S[a,n] + eps > min_pos S[a,.]
//   h = D[a,p] - D[a,n] + margin over P[a,.] x N[a,.];  loss = sum_{h>0} h / #{h>0}  (0 where nothing is mined)
// Workspace (floats; the base 8-byte aligned): psum [B] fp64 | pcnt [B] int32 | invn [B] | e [B,L] | c [B,B].
constexpr int TRIP_MAX_B = 1024;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// S[a,j] and D[a,j] from the normalised rows; the one expression both launches evaluate (same bits for (a,j) and (j,a):
// a product commutes, a difference only changes sign)
__device__ __forceinline__ void trip_pair(const float* ea, const float* __restrict__ ej, int L, float& S, float& D) {
  float s = 0.f, d2 = 0.f;
  for (int k = 0; k < L; ++k) {
    const float u = ea[k], v = ej[k], d = u - v;
    s = fmaf(u, v, s);
    d2 = fmaf(d, d, d2);
  }
  S = s;
  D = sqrtf(d2);
}

// one wave per row: e = x / max(|x|, 1e-12) (torch.nn.functional.normalize) and 1 / max(|x|, 1e-12)
__global__ __launch_bounds__(256) void orced_triplet_norm_kernel(const float* __restrict__ x, float* e, float* invn, int B,
                                                                 int L) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;                                    // (wave-uniform: no barrier below)
  float a = 0.f;
  for (int k = lane; k < L; k += 64) {
    const float v = x[(long)row * L + k];
    a = fmaf(v, v, a);
  }
  const float n = fmaxf(sqrtf(wave_sum(a)), 1e-12f);
  for (int k = lane; k < L; k += 64) e[(long)row * L + k] = x[(long)row * L + k] / n;
  if (lane == 0) invn[row] = 1.f / n;
}

// one workgroup per anchor a: row a of S and D in LDS, the two extrema, the masks, the |P_a| x |N_a| hinge loop.
// Writes psum[a] (fp64 sum of the positive hinges), pcnt[a] (their number) and c[a,j] = #(active triplets with j as the
// positive) - #(active triplets with j as the negative).
__global__ __launch_bounds__(256) void orced_triplet_rows_kernel(const float* __restrict__ e,
                                                                 const long long* __restrict__ labels, double* psum,
                                                                 int* pcnt, float* c, float epsilon, float margin, int B,
                                                                 int L) {
  __shared__ float es[MAX_LAT];
  __shared__ float Ds[TRIP_MAX_B];
  __shared__ unsigned char flag[TRIP_MAX_B];               // 1: mined positive, 2: mined negative
  __shared__ float redf[8];
  __shared__ double redd[4];
  __shared__ int redi[4];
  const int a = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int k = tid; k < L; k += 256) es[k] = e[(long)a * L + k];
  __syncthreads();
  const long long la = labels[a];
  // (B <= 1024: at most 4 columns per thread, kept in registers between the two passes)
  float Sj[TRIP_MAX_B / 256];
  float mx = -INFINITY, mn = INFINITY;
#pragma unroll
  for (int q = 0; q < TRIP_MAX_B / 256; ++q) {
    const int j = q * 256 + tid;
    Sj[q] = 0.f;
    if (j < B) {
      float S, D;
      trip_pair(es, e + (long)j * L, L, S, D);
      Sj[q] = S;
      Ds[j] = D;
      if (labels[j] != la) mx = fmaxf(mx, S);
      else if (j != a) mn = fminf(mn, S);
    }
  }
  mx = wave_max(mx);
  mn = wave_min(mn);
  if (lane == 0) { redf[wave] = mx; redf[4 + wave] = mn; }
  __syncthreads();
  const float maxneg = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
  const float minpos = fminf(fminf(redf[4], redf[5]), fminf(redf[6], redf[7]));
#pragma unroll
  for (int q = 0; q < TRIP_MAX_B / 256; ++q) {
    const int j = q * 256 + tid;
    if (j < B) {
      unsigned char f = 0;
      if (labels[j] != la) f = (Sj[q] + epsilon > minpos) ? 2 : 0;
      else if (j != a) f = (Sj[q] - epsilon < maxneg) ? 1 : 0;
      flag[j] = f;
    }
  }
  __syncthreads();
  double acc = 0.0;
  int cnt = 0;
  for (int j = tid; j < B; j += 256) {
    const unsigned char f = flag[j];
    const float Dj = Ds[j];
    int cj = 0;
    if (f == 1) {                                          // j a mined positive: every mined negative
      for (int n = 0; n < B; ++n) {
        const float h = (Dj - Ds[n]) + margin;
        if (flag[n] == 2 && h > 0.f) { acc += (double)h; ++cj; }
      }
      cnt += cj;
    } else if (f == 2) {                                   // j a mined negative: every mined positive (the same h, bit for bit)
      for (int p = 0; p < B; ++p) {
        const float h = (Ds[p] - Dj) + margin;
        if (flag[p] == 1 && h > 0.f) --cj;
      }
    }
    c[(long)a * B + j] = (float)cj;
  }
  acc = wave_sum_d(acc);
  cnt = wave_sum_i(cnt);
  if (lane == 0) { redd[wave] = acc; redi[wave] = cnt; }
  __syncthreads();
  if (tid == 0) {
    psum[a] = (redd[0] + redd[1]) + (redd[2] + redd[3]);
    pcnt[a] = (redi[0] + redi[1]) + (redi[2] + redi[3]);
  }
}

// one workgroup per row i: the totals (every workgroup adds them in the same order; workgroup 0 writes the loss), then
//   g_i = gscale / count * sum_j (c[i,j] + c[j,i]) (e_i - e_j) / D[i,j]      (a pair with D == 0 contributes nothing:
//   torch.cdist's backward rule),   dx_i = (g_i - e_i (e_i . g_i)) / max(|x_i|, 1e-12)   (normalize's backward)
__global__ __launch_bounds__(256) void orced_triplet_grad_kernel(const float* __restrict__ e, const float* __restrict__ invn,
                                                                 const double* __restrict__ psum,
                                                                 const int* __restrict__ pcnt, const float* __restrict__ c,
                                                                 float* loss, float* dx, float gscale, int B, int L) {
  __shared__ float es[MAX_LAT];
  __shared__ float w[TRIP_MAX_B];                          // (c[i,j] + c[j,i]) / D[i,j]
  __shared__ double gpart[4][MAX_LAT];
  __shared__ float gs[MAX_LAT];
  __shared__ double redd[4];
  __shared__ int redi[4];
  __shared__ float dotv;
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double acc = 0.0;
  int cnt = 0;
  for (int a = tid; a < B; a += 256) { acc += psum[a]; cnt += pcnt[a]; }
  acc = wave_sum_d(acc);
  cnt = wave_sum_i(cnt);
  if (lane == 0) { redd[wave] = acc; redi[wave] = cnt; }
  for (int k = tid; k < L; k += 256) es[k] = e[(long)i * L + k];
  __syncthreads();
  const int count = (redi[0] + redi[1]) + (redi[2] + redi[3]);
  if (i == 0 && tid == 0)
    *loss = count > 0 ? (float)(((redd[0] + redd[1]) + (redd[2] + redd[3])) / (double)count) : 0.f;
  if (dx == nullptr) return;
  if (count == 0) {                                        // (uniform over the grid)
    for (int k = tid; k < L; k += 256) dx[(long)i * L + k] = 0.f;
    return;
  }
  for (int j = tid; j < B; j += 256) {
    const float cij = c[(long)i * B + j] + c[(long)j * B + i];
    float wj = 0.f;
    if (cij != 0.f) {
      float S, D;
      trip_pair(es, e + (long)j * L, L, S, D);
      if (D > 0.f) wj = cij / D;
    }
    w[j] = wj;
  }
  __syncthreads();
  // wave v takes the columns j = v mod 4, its lanes the components k; the four partial sums meet in a fixed order
  for (int k = lane; k < L; k += 64) {
    const float ek = es[k];
    double g = 0.0;
    for (int j = wave; j < B; j += 4) {
      const float wj = w[j];
      if (wj != 0.f) g += (double)(wj * (ek - e[(long)j * L + k]));
    }
    gpart[wave][k] = g;
  }
  __syncthreads();
  const float sc = gscale / (float)count;
  float part = 0.f;
  for (int k = tid; k < L; k += 256) {
    const float g = sc * (float)((gpart[0][k] + gpart[1][k]) + (gpart[2][k] + gpart[3][k]));
    gs[k] = g;
    part = fmaf(es[k], g, part);
  }
  part = wave_sum(part);                                   // L <= 128: waves 0 and 1 hold the two halves
  if (lane == 0) redd[wave] = (double)part;
  __syncthreads();
  if (tid == 0) dotv = (float)(redd[0] + redd[1]);
  __syncthreads();
  const float dot = dotv, inv = invn[i];
  for (int k = tid; k < L; k += 256) dx[(long)i * L + k] = (gs[k] - es[k] * dot) * inv;
}

// ---------------------------------------------------------------------------------------------------------------------
// Open-set rule of inference_ORCED.py:18-132 after its statistics, one wave per sample:
//   p_k = prod_d Phi(dev / sd) - prod_d Phi(-dev / sd),  dev = |z - mean_k|   (fp64; Phi(t) = erfc(-t / sqrt 2) / 2)
//   latent test: p_k > thresholds_g for EVERY k;  reconstruction test: re > thr_re[pred];  either -> K (unknown)
__device__ __forceinline__ double wave_prod_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v *= __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void orced_ood_kernel(const float* __restrict__ z, const float* __restrict__ re,
                                                        const long long* __restrict__ pred,
                                                        const double* __restrict__ mean_z, const double* __restrict__ sd_z,
                                                        const double* __restrict__ thr_re, double thresholds_g,
                                                        long long* out, double* p, int n, int K, int L) {
  const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= n) return;                                      // (wave-uniform: no barrier below)
  bool every = true;
  for (int k = 0; k < K; ++k) {
    double hi = 1.0, lo = 1.0;
    for (int d = lane; d < L; d += 64) {
      const double t = fabs((double)z[(long)s * L + d] - mean_z[(long)k * L + d]) / sd_z[(long)k * L + d] * M_SQRT1_2;
      hi *= 0.5 * erfc(-t);
      lo *= 0.5 * erfc(t);
    }
    const double pk = wave_prod_d(hi) - wave_prod_d(lo);
    if (p != nullptr && lane == 0) p[(long)k * n + s] = pk;
    every = every && (pk > thresholds_g);
  }
  if (lane == 0) {
    const long long pr = pred[s];
    // (a prediction outside [0, K) has no threshold to be tested against: unknown)
    const bool rec = (pr >= 0 && pr < K) ? ((double)re[s] > thr_re[pr]) : true;
    out[s] = (every || rec) ? (long long)K : pr;
  }
}

}  // namespace

extern "C" int pcaa_orced_heads_supported(int B, int K, int d_in, int d_lat) {
  return (B >= 1 && K >= 1 && K <= MAX_K && d_in >= 1 && d_in <= MAX_IN && d_lat >= 1 && d_lat <= MAX_LAT) ? 1 : 0;
}

extern "C" int pcaa_orced_heads_fwd(const float* x4, const float* Wmu, const float* bmu, const float* Wlv,
                                    const float* blv, const float* eps, const float* Wc, const float* bc, float* mu,
                                    float* logvar, float* sup_fv, float* logits, int B, int K, int d_in, int d_lat,
                                    void* stream) {
  PCAA_CHECK_ARG(x4 && Wmu && bmu && Wlv && blv && eps && Wc && bc && mu && logvar && sup_fv && logits,
                 "pcaa_orced_heads_fwd: null pointer");
  PCAA_CHECK_ARG(pcaa_orced_heads_supported(B, K, d_in, d_lat), "pcaa_orced_heads_fwd: need K <= %d, d_in <= %d, d_lat <= %d",
                 MAX_K, MAX_IN, MAX_LAT);
  hipLaunchKernelGGL(orced_heads_fwd_kernel, dim3(B), dim3(256), 0, as_stream(stream), x4, Wmu, bmu, Wlv, blv, eps, Wc, bc,
                     mu, logvar, sup_fv, logits, K, d_in, d_lat);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_orced_heads_fwd");
}

extern "C" int pcaa_orced_heads_bwd(const float* x4, const float* eps, const float* logvar, const float* sup_fv,
                                    const float* Wmu, const float* Wlv, const float* Wc, const float* d_logits,
                                    const float* d_sup, const float* d_mu, const float* d_logvar, float* ws, float* dWmu,
                                    float* dbmu, float* dWlv, float* dblv, float* dWc, float* dbc, float* dx4, int B, int K,
                                    int d_in, int d_lat, void* stream) {
  PCAA_CHECK_ARG(x4 && eps && logvar && sup_fv && Wmu && Wlv && Wc && ws && dWmu && dbmu && dWlv && dblv && dWc && dbc,
                 "pcaa_orced_heads_bwd: null pointer");
  PCAA_CHECK_ARG(pcaa_orced_heads_supported(B, K, d_in, d_lat), "pcaa_orced_heads_bwd: need K <= %d, d_in <= %d, d_lat <= %d",
                 MAX_K, MAX_IN, MAX_LAT);
  hipLaunchKernelGGL(orced_heads_bwd_rows_kernel, dim3(B), dim3(256), 0, as_stream(stream), eps, logvar, Wmu, Wlv, Wc,
                     d_logits, d_sup, d_mu, d_logvar, ws, dx4, B, K, d_in, d_lat);
  hipLaunchKernelGGL(orced_heads_bwd_params_kernel, dim3(2 * d_lat + 1), dim3(256), 0, as_stream(stream), x4, sup_fv,
                     d_logits, ws, dWmu, dbmu, dWlv, dblv, dWc, dbc, B, K, d_in, d_lat);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_orced_heads_bwd");
}

extern "C" int pcaa_orced_kl(const float* mu, const float* logvar, const float* mu_k, float* loss, float* d_mu,
                             float* d_logvar, float* d_muk, float gscale, int B, int d_lat, void* stream) {
  PCAA_CHECK_ARG(mu && logvar && mu_k && B >= 1 && d_lat >= 1, "pcaa_orced_kl: bad args");
  hipLaunchKernelGGL(orced_kl_kernel, dim3(1), dim3(256), 0, as_stream(stream), mu, logvar, mu_k, loss, d_mu, d_logvar, d_muk,
                     gscale, B, d_lat);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_orced_kl");
}

extern "C" int pcaa_orced_triplet_supported(int B, int d_lat) {
  return (B >= 1 && B <= TRIP_MAX_B && d_lat >= 1 && d_lat <= MAX_LAT) ? 1 : 0;
}

extern "C" int pcaa_orced_triplet(const float* x, const long long* labels, float epsilon, float margin, float gscale,
                                  float* ws, float* loss, float* dx, int B, int d_lat, void* stream) {
  PCAA_CHECK_ARG(x && labels && ws && loss, "pcaa_orced_triplet: null pointer");
  PCAA_CHECK_ARG(pcaa_orced_triplet_supported(B, d_lat), "pcaa_orced_triplet: need 1 <= B <= %d, 1 <= d_lat <= %d",
                 TRIP_MAX_B, MAX_LAT);
  PCAA_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "pcaa_orced_triplet: ws must be 8-byte aligned");
  double* psum = reinterpret_cast<double*>(ws);
  int* pcnt = reinterpret_cast<int*>(ws + 2 * (long)B);
  float* invn = ws + 3 * (long)B;
  float* e = ws + 4 * (long)B;
  float* c = e + (long)B * d_lat;
  hipLaunchKernelGGL(orced_triplet_norm_kernel, dim3((unsigned)cdiv(B, 4)), dim3(256), 0, as_stream(stream), x, e, invn, B,
                     d_lat);
  hipLaunchKernelGGL(orced_triplet_rows_kernel, dim3(B), dim3(256), 0, as_stream(stream), e, labels, psum, pcnt, c, epsilon,
                     margin, B, d_lat);
  hipLaunchKernelGGL(orced_triplet_grad_kernel, dim3(dx ? B : 1), dim3(256), 0, as_stream(stream), e, invn, psum, pcnt, c,
                     loss, dx, gscale, B, d_lat);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_orced_triplet");
}

extern "C" int pcaa_orced_ood(const float* z, const float* re, const long long* pred, const double* mean_z,
                              const double* sd_z, const double* thr_re, double thresholds_g, long long* out, double* p,
                              int n, int K, int d_lat, void* stream) {
  PCAA_CHECK_ARG(z && re && pred && mean_z && sd_z && thr_re && out, "pcaa_orced_ood: null pointer");
  PCAA_CHECK_ARG(n >= 1 && K >= 1 && d_lat >= 1, "pcaa_orced_ood: need n, K, d_lat >= 1");
  hipLaunchKernelGGL(orced_ood_kernel, dim3((unsigned)cdiv(n, 4)), dim3(256), 0, as_stream(stream), z, re, pred, mean_z, sd_z,
                     thr_re, thresholds_g, out, p, n, K, d_lat);
  PCAA_RETURN_LAUNCH_STATUS("pcaa_orced_ood");
}
