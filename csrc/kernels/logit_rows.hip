// Per-request logit penalties of the continuous decode batch: repetition penalty, presence and
// frequency penalties and logit bias, applied in place to a logits row before the sampler reads it
// (docs/DESIGN.md "Per-request logit penalties").
#include "rt_common.h"

using namespace rt;

#define LOGIT_ROWS_MAX_SEQ 4096  // history positions staged per row: 16 KB of LDS
#define LOGIT_ROWS_MAX_BIAS 16

namespace {

// the arithmetic type: fp32 for bf16 logits; fp64 for fp32 logits, so that the stored value is one
// rounding of the exact result there too
template <typename T> struct LogitAcc;
template <> struct LogitAcc<bf16_t> {
  typedef float type;
  static __device__ __forceinline__ float load(bf16_t x) { return bf2f(x); }
  static __device__ __forceinline__ bf16_t store(float x) { return f2bf(x); }
};
template <> struct LogitAcc<float> {
  typedef double type;
  static __device__ __forceinline__ double load(float x) { return (double)x; }
  static __device__ __forceinline__ float store(double x) { return (float)x; }
};

}  // namespace

// Row b = blockIdx.x. History = hist[b, kv_start .. kv_len] (L = kv_len + 1 - kv_start tokens), its
// last gen_len tokens generated, the ones before them the prompt. `tok_in` != null: the step's input
// token is first appended at hist[b, kv_len] (it is the newest generated token; the staged copy takes
// it from tok_in, so nothing is read back from memory). For every distinct token v of the history,
// with c = its count among the generated tokens, the thread that owns v's FIRST position applies
//   l = l > 0 ? l * inv_rho : l * rho;   l -= pi * [c > 0] + phi * c;   l += bias (if v has one)
// and stores l rounded once. Bias tokens that are not in the history belong to thread j < nbias of
// their entry j (entries are distinct tokens, checked on the host): every touched element has exactly
// one reader and writer, so there is no atomic and no ordering between threads beyond the staging
// barrier. Inactive rows and neutral rows (rho = 1, pi = phi = 0, no bias) leave on a
// workgroup-uniform branch before any store. Tokens outside [0, V) are skipped.
template <typename T>
__global__ __launch_bounds__(256) void logit_rows_penalty_kernel(
    T* __restrict__ logits, long ld, int V, long* __restrict__ hist, int Smax, const long* __restrict__ tok_in,
    const int* __restrict__ kv_len, const int* __restrict__ kv_start, const int* __restrict__ gen_len,
    const uint8_t* __restrict__ active, const float* __restrict__ rho, const float* __restrict__ inv_rho,
    const float* __restrict__ pi, const float* __restrict__ phi, const int* __restrict__ nbias,
    const int* __restrict__ bias_tok, const float* __restrict__ bias_val) {
  typedef typename LogitAcc<T>::type acc_t;
  __shared__ __attribute__((aligned(16))) int toks[LOGIT_ROWS_MAX_SEQ];
  __shared__ int btok[LOGIT_ROWS_MAX_BIAS];
  __shared__ float bval[LOGIT_ROWS_MAX_BIAS];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (active && active[b] == 0) return;
  const float r = rho[b], ir = inv_rho[b], p = pi[b], f = phi[b];
  const int nb = min(max(nbias[b], 0), LOGIT_ROWS_MAX_BIAS);
  if (r == 1.f && ir == 1.f && p == 0.f && f == 0.f && nb == 0) return;
  const int kl = kv_len[b];
  if (kl < 0 || kl >= Smax) return;
  const int ks = min(max(kv_start ? kv_start[b] : 0, 0), kl);
  const int L = kl + 1 - ks;
  if (L > LOGIT_ROWS_MAX_SEQ) return;  // refused on the host (the batcher's max_seq check)
  const int n_gen = min(max(gen_len[b], 0), L);
  const int P = L - n_gen;  // staged positions [0, P): prompt, [P, L): generated
  long* h = hist + (long)b * Smax;
  T* row = logits + (long)b * ld;

  const bool append = tok_in != nullptr;
  const long newest = append ? tok_in[b] : 0;
  if (append && tid == 0) h[kl] = newest;
  for (int i = tid; i < L; i += blockDim.x) {
    const long t = (append && i == L - 1) ? newest : h[ks + i];
    toks[i] = (t >= 0 && t < V) ? (int)t : -1;
  }
  // a tail of "no token" up to a multiple of 4: the scan below reads 16 B at a time
  const int L4 = (L + 3) & ~3;
  if (tid < L4 - L) toks[L + tid] = -1;
  if (tid < LOGIT_ROWS_MAX_BIAS) {
    const int t = tid < nb ? bias_tok[b * LOGIT_ROWS_MAX_BIAS + tid] : -1;
    btok[tid] = (t >= 0 && t < V) ? t : -1;
    bval[tid] = tid < nb ? bias_val[b * LOGIT_ROWS_MAX_BIAS + tid] : 0.f;
  }
  __syncthreads();

  const int4* toks4 = (const int4*)toks;
  for (int i = tid; i < L; i += blockDim.x) {
    const int v = toks[i];
    if (v < 0) continue;
    // one pass over the staged history (every lane reads the same 16 B: a broadcast): the first
    // position of v and its count among the generated tokens
    int first = L, c = 0;
    for (int q = 0; q < L4 / 4; ++q) {
      const int4 w = toks4[q];
      const int j = 4 * q;
      const bool e0 = w.x == v, e1 = w.y == v, e2 = w.z == v, e3 = w.w == v;
      if (e3) first = min(first, j + 3);
      if (e2) first = min(first, j + 2);
      if (e1) first = min(first, j + 1);
      if (e0) first = min(first, j);
      c += (int)(e0 && j >= P) + (int)(e1 && j + 1 >= P) + (int)(e2 && j + 2 >= P) + (int)(e3 && j + 3 >= P);
    }
    if (first != i) continue;  // an earlier position owns this token
    acc_t l = LogitAcc<T>::load(row[v]);
    l = l > (acc_t)0 ? l * (acc_t)ir : l * (acc_t)r;
    l -= (acc_t)p * (acc_t)(c > 0 ? 1 : 0) + (acc_t)f * (acc_t)c;
#pragma unroll
    for (int j = 0; j < LOGIT_ROWS_MAX_BIAS; ++j)
      if (btok[j] == v) l += (acc_t)bval[j];
    row[v] = LogitAcc<T>::store(l);
  }
  // bias entries whose token the history does not hold: rule 3 alone
  if (tid < nb) {
    const int v = btok[tid];
    bool seen = v < 0;
    for (int q = 0; q < L4 / 4 && !seen; ++q) {
      const int4 w = toks4[q];
      seen = w.x == v || w.y == v || w.z == v || w.w == v;
    }
    if (!seen) row[v] = LogitAcc<T>::store(LogitAcc<T>::load(row[v]) + (acc_t)bval[tid]);
  }
}

extern "C" int rt_logit_rows_max_seq() { return LOGIT_ROWS_MAX_SEQ; }

extern "C" int rt_logit_rows_penalty(void* logits, int is_f32, long ld, long B, int V, long* hist, int Smax,
                                     const long* tok_in, const int* kv_len, const int* kv_start, const int* gen_len,
                                     const uint8_t* active, const float* rho, const float* inv_rho, const float* pi,
                                     const float* phi, const int* nbias, const int* bias_tok, const float* bias_val,
                                     hipStream_t stream) {
  if (V < 1 || ld < V || Smax < 1 || Smax > LOGIT_ROWS_MAX_SEQ) return -1;
  if (B == 0) return 0;
  if (is_f32)
    hipLaunchKernelGGL(logit_rows_penalty_kernel<float>, dim3((unsigned)B), dim3(256), 0, stream, (float*)logits, ld, V,
                       hist, Smax, tok_in, kv_len, kv_start, gen_len, active, rho, inv_rho, pi, phi, nbias, bias_tok,
                       bias_val);
  else
    hipLaunchKernelGGL(logit_rows_penalty_kernel<bf16_t>, dim3((unsigned)B), dim3(256), 0, stream, (bf16_t*)logits, ld,
                       V, hist, Smax, tok_in, kv_len, kv_start, gen_len, active, rho, inv_rho, pi, phi, nbias, bias_tok,
                       bias_val);
  RT_LAUNCH_CHECK();
  return 0;
}
