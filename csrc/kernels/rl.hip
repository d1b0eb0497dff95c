// RL kernels: token-level GAE reverse scan, and the decode-step bookkeeping kernel
// that keeps a hipGraph-captured generation loop free of host round trips.
//
// GAE follows reinforcement_learning_optimization_after_rag.py:176-191 (delta = r + g*V' - V,
// A = delta + g*lam*A') but over the tokens of each response instead of across batch samples, with
// lam a parameter (reference hard-codes 0.95) and padding tokens masked out.
#include "rt_common.h"

namespace rt {

__global__ void gae_kernel(const float* __restrict__ rewards, const float* __restrict__ values,
                           const float* __restrict__ mask, int B, int T, float gamma, float lam,
                           float* __restrict__ adv, float* __restrict__ ret) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float nextv = 0.f, last = 0.f;
  for (int t = T - 1; t >= 0; --t) {
    const long i = (long)b * T + t;
    if (mask[i] == 0.f) {
      adv[i] = 0.f;
      ret[i] = 0.f;
      continue;
    }
    const float v = values[i];
    const float delta = rewards[i] + gamma * nextv - v;
    last = delta + gamma * lam * last;
    adv[i] = last;
    ret[i] = last + v;
    nextv = v;
  }
}

// PPO advantages in one launch (one workgroup; a thread per sequence, then block reductions):
//   kl[b,t]   = old_logp - ref_logp                      (t < len[b])
//   r[b,t]    = -kl_coef kl + (t == len[b] - 1) score[b]  (reward at the last response token)
//   GAE over r with V = old values (the reverse scan of gae_kernel)
//   whiten: adv = (adv - mean) / sqrt(var + eps) over the valid tokens (masked_whiten)
//   kl_seq[b] = sum_t kl                                  (the KL-to-reference statistic)
// Replaces ~15 small ATen launches between the reference forward and the update
// (reinforcement_learning_optimization_after_rag.py:176-191 GAE, with the SURVEY B3 KL term).
__global__ __launch_bounds__(256) void ppo_advantages_kernel(const float* __restrict__ old_lp, const float* __restrict__ ref_lp,
                                                             const float* __restrict__ values, const float* __restrict__ score,
                                                             const int* __restrict__ len, int B, int T, float kl_coef,
                                                             float gamma, float lam, int whiten, float eps,
                                                             float* __restrict__ adv, float* __restrict__ ret,
                                                             float* __restrict__ rew, float* __restrict__ kl_seq) {
  __shared__ float sb[4];
  float s1 = 0.f, n = 0.f;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const int L = min(max(len[b], 0), T);
    float nextv = 0.f, last = 0.f, klsum = 0.f;
    for (int t = T - 1; t >= 0; --t) {
      const long i = (long)b * T + t;
      if (t >= L) {
        adv[i] = 0.f; ret[i] = 0.f; rew[i] = 0.f;
        continue;
      }
      const float kl = old_lp[i] - ref_lp[i];
      klsum += kl;
      const float r = -kl_coef * kl + (t == L - 1 ? score[b] : 0.f);
      rew[i] = r;
      const float v = values[i];
      const float delta = r + gamma * nextv - v;
      last = delta + gamma * lam * last;
      adv[i] = last;
      ret[i] = last + v;
      nextv = v;
      s1 += last;
    }
    n += (float)L;
    kl_seq[b] = klsum;
  }
  if (!whiten) return;
  const float tot = block_sum(s1, sb);
  const float cnt = block_sum(n, sb);
  const float mean = tot / fmaxf(cnt, 1.f);
  float s2 = 0.f;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const int L = min(max(len[b], 0), T);
    for (int t = 0; t < L; ++t) {
      const float d = adv[(long)b * T + t] - mean;
      s2 += d * d;
    }
  }
  const float var = block_sum(s2, sb) / fmaxf(cnt, 1.f);
  const float inv = rsqrtf(var + eps);
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const int L = min(max(len[b], 0), T);
    for (int t = 0; t < L; ++t) {
      const long i = (long)b * T + t;
      adv[i] = (adv[i] - mean) * inv;
    }
  }
}

// After sampling token `tok[b]` at decode step `step`: record it, update finished flags (eos or
// length budget), advance per-row cache length/position, bump the RNG offset and step counter.
// Rows that are finished keep emitting pad and stop advancing. `row_max_new` (optional, [B]): the
// row's own answer length; a row finishes at min(row_max_new[b], max_new).
__global__ void decode_update_kernel(const long* __restrict__ tok, long* __restrict__ out_tokens, int max_new,
                                     float* __restrict__ out_logp, const float* __restrict__ logp,
                                     float* __restrict__ out_values, const float* __restrict__ values,
                                     uint8_t* __restrict__ active, int* __restrict__ kv_len, int* __restrict__ pos,
                                     long* __restrict__ next_input, int* __restrict__ gen_len,
                                     int64_t* __restrict__ step, int64_t* __restrict__ rng_offset, int B,
                                     const long* __restrict__ eos_ids, int n_eos, long pad_id,
                                     int* __restrict__ attn_len, const int* __restrict__ kv_start,
                                     const int* __restrict__ row_max_new) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t s = *step;
  if (b < B) {
    const bool act = active[b] != 0;
    long t = tok[b];
    // the row's own output position: equal to the step counter for every active row of a static
    // batch (rows start together and never reactivate); rows admitted mid-flight by continuous
    // batching start at 0
    const int sr = gen_len[b];
    if (act && sr < max_new) {
      out_tokens[(long)b * max_new + sr] = t;
      if (out_logp) out_logp[(long)b * max_new + sr] = logp[b];
      if (out_values && values) out_values[(long)b * max_new + sr] = values[b];
      gen_len[b] = sr + 1;
      bool fin = (sr + 1 >= (row_max_new ? min(row_max_new[b], max_new) : max_new));
      for (int e = 0; e < n_eos; ++e) fin = fin || (t == eos_ids[e]);
      if (fin) active[b] = 0;
      kv_len[b] += 1;
      pos[b] += 1;
      next_input[b] = t;
    } else {
      next_input[b] = pad_id;
    }
    // the next step's attention length and rotary position (kept here, not as two extra
    // elementwise launches at the head of every decode step)
    if (attn_len) {
      const int kl = kv_len[b];
      attn_len[b] = kl + 1;
      pos[b] = kl - (kv_start ? kv_start[b] : 0);
    }
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *step = s + 1;
    *rng_offset = *rng_offset + 1;
  }
}

// Prompt-lookup speculative decoding, bookkeeping of a verify step (G = K + 1 positions per row).
// `inp` [B, G] held the step's inputs (last emitted token | K draft tokens, n_draft[b] of them real),
// `sampled` / `logp` [B, G] what the sampler drew after each of them. An active row accepts the
// longest prefix a of its draft that the sampler reproduced and emits sampled[0..a], cut after the
// first EOS and at the output width; tokens and log-probs go to the row's own output position, the
// tokens also into the history `hist` [B, Smax] (indexed like cache slots: the last emitted token
// sits at hist[kv_len], the slot the next step appends it at). Lengths advance by the emitted count.
// counters: {row-steps, drafted tokens, accepted tokens that were emitted} (integer atomics: the sum
// does not depend on thread order). One thread per row, one workgroup.
// `row_max_new` (optional, [B]): the row's own answer length; it finishes at min(row_max_new[b],
// max_new), as in decode_update_kernel. `row_stats` (optional, [B, 2] int32): per row {verify steps
// it was active in, accepted tokens emitted}, added by the row's own thread (plain load / add /
// store; zeroed by the host when a request is admitted into the row).
__global__ void lookup_accept_kernel(const long* __restrict__ sampled, const float* __restrict__ logp,
                                     const long* __restrict__ inp, const int* __restrict__ n_draft, int G,
                                     long* __restrict__ out_tokens, float* __restrict__ out_logp, int max_new,
                                     long* __restrict__ hist, int Smax, uint8_t* __restrict__ active,
                                     int* __restrict__ kv_len, int* __restrict__ pos, int* __restrict__ attn_len,
                                     const int* __restrict__ kv_start, int* __restrict__ gen_len,
                                     int64_t* __restrict__ step, int64_t* __restrict__ rng_offset,
                                     unsigned long long* __restrict__ counters, int B,
                                     const long* __restrict__ eos_ids, int n_eos,
                                     const int* __restrict__ row_max_new, int* __restrict__ row_stats) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t s = *step;
  if (b < B) {
    const int gl = gen_len[b], kl = kv_len[b];
    if (active[b] != 0 && gl < max_new) {
      const int lim = row_max_new ? min(row_max_new[b], max_new) : max_new;
      const int nd = min(max(n_draft[b], 0), G - 1);
      int a = 0;
      while (a < nd && sampled[(long)b * G + a] == inp[(long)b * G + a + 1]) ++a;
      int e = 0;
      bool fin = false;
      for (int i = 0; i <= a && !fin; ++i) {
        const long t = sampled[(long)b * G + i];
        out_tokens[(long)b * max_new + gl + i] = t;
        out_logp[(long)b * max_new + gl + i] = logp[(long)b * G + i];
        if (kl + 1 + i < Smax) hist[(long)b * Smax + kl + 1 + i] = t;
        e = i + 1;
        fin = gl + e >= lim;
        for (int q = 0; q < n_eos; ++q) fin = fin || (t == eos_ids[q]);
      }
      gen_len[b] = gl + e;
      kv_len[b] = kl + e;
      if (fin) active[b] = 0;
      atomicAdd(counters + 0, 1ull);
      atomicAdd(counters + 1, (unsigned long long)nd);
      atomicAdd(counters + 2, (unsigned long long)(e - 1));
      if (row_stats) {
        row_stats[2 * b] += 1;
        row_stats[2 * b + 1] += e - 1;
      }
    }
    const int kn = kv_len[b];
    attn_len[b] = kn + 1;
    pos[b] = kn - (kv_start ? kv_start[b] : 0);
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *step = s + 1;
    *rng_offset = *rng_offset + 1;
  }
}

// The next verify step's inputs of row b = blockIdx.x: inp[b, 0] = the last emitted token
// hist[b, kv_len]; inp[b, 1..K] = the draft. With end = kv_len + 1 tokens of history, for n = ngram
// .. 1 the latest start i in [kv_start, end - n) with hist[i .. i + n) == hist[end - n .. end) wins
// (so at least one token follows it) and the up-to-K tokens after the match are proposed; n_draft =
// how many exist (0: nothing matched), the rest is pad. The latest start is a max-reduction over
// the candidates (block_max over per-thread maxima: independent of thread order). row_active
// [B, G] = the row's active flag per position (the sampler's row mask). Inactive rows get pad.
// `row_draft` (optional, [B]): the row's own draft length, capping the proposal at
// min(row_draft[b], G - 1) tokens; 0: an empty draft, the verify step emits one token for the row.
__global__ __launch_bounds__(256) void lookup_draft_kernel(const long* __restrict__ hist, int Smax,
                                                           const int* __restrict__ kv_len,
                                                           const int* __restrict__ kv_start,
                                                           const uint8_t* __restrict__ active, int G, int ngram,
                                                           long pad_id, long* __restrict__ inp,
                                                           int* __restrict__ n_draft,
                                                           uint8_t* __restrict__ row_active,
                                                           const int* __restrict__ row_draft) {
  __shared__ int red[4];
  __shared__ int best_sh;
  const int b = blockIdx.x, tid = threadIdx.x;
  const bool act = active[b] != 0;
  const long* h = hist + (long)b * Smax;
  long* in = inp + (long)b * G;
  if (tid < G) row_active[(long)b * G + tid] = act ? 1 : 0;
  const int kl = kv_len[b];
  if (!act || kl < 0 || kl >= Smax) {  // uniform over the workgroup
    if (tid < G) in[tid] = pad_id;
    if (tid == 0) n_draft[b] = 0;
    return;
  }
  const int end = kl + 1, ks = max(kv_start ? kv_start[b] : 0, 0);
  int best = -1, bn = 0;
  for (int n = ngram; n >= 1 && best < 0; --n) {
    int loc = -1;
    if (end - n > ks) {
      for (int i = ks + tid; i < end - n; i += blockDim.x) {
        bool eq = true;
        for (int k = 0; k < n; ++k) eq = eq && (h[i + k] == h[end - n + k]);
        if (eq) loc = i;  // ascending i: the thread's latest
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) loc = max(loc, __shfl_xor(loc, off, 64));
    if ((tid & 63) == 0) red[tid >> 6] = loc;
    __syncthreads();
    if (tid == 0) best_sh = max(max(red[0], red[1]), max(red[2], red[3]));
    __syncthreads();
    best = best_sh;
    bn = n;
    __syncthreads();  // red / best_sh are rewritten by the next n
  }
  const int cont = best + bn;  // first proposed token
  const int cap = row_draft ? min(max(row_draft[b], 0), G - 1) : G - 1;
  const int avail = best >= 0 ? min(cap, end - cont) : 0;
  if (tid == 0) {
    in[0] = h[kl];
    n_draft[b] = avail;
  }
  if (tid >= 1 && tid < G) in[tid] = tid - 1 < avail ? h[cont + tid - 1] : pad_id;
}

extern "C" int rt_lookup_accept(const long* sampled, const float* logp, const long* inp, const int* n_draft, int G,
                                long* out_tokens, float* out_logp, int max_new, long* hist, int Smax,
                                uint8_t* active, int* kv_len, int* pos, int* attn_len, const int* kv_start,
                                int* gen_len, int64_t* step, int64_t* rng_offset, unsigned long long* counters, int B,
                                const long* eos_ids, int n_eos, const int* row_max_new, int* row_stats,
                                hipStream_t stream) {
  if (B > 1024 || G < 1 || G > 8) return -1;
  if (B == 0) return 0;
  hipLaunchKernelGGL(lookup_accept_kernel, dim3(1), dim3(((B + 63) / 64) * 64), 0, stream, sampled, logp, inp,
                     n_draft, G, out_tokens, out_logp, max_new, hist, Smax, active, kv_len, pos, attn_len, kv_start,
                     gen_len, step, rng_offset, counters, B, eos_ids, n_eos, row_max_new, row_stats);
  RT_LAUNCH_CHECK();
  return 0;
}

extern "C" int rt_lookup_draft(const long* hist, int Smax, const int* kv_len, const int* kv_start,
                               const uint8_t* active, int G, int ngram, long pad_id, long* inp, int* n_draft,
                               uint8_t* row_active, int B, const int* row_draft, hipStream_t stream) {
  if (G < 1 || G > 8 || ngram < 1) return -1;
  if (B == 0) return 0;
  hipLaunchKernelGGL(lookup_draft_kernel, dim3((unsigned)B), dim3(256), 0, stream, hist, Smax, kv_len, kv_start,
                     active, G, ngram, pad_id, inp, n_draft, row_active, row_draft);
  RT_LAUNCH_CHECK();
  return 0;
}

// Token-level PPO objective over [B, T] (masked mean over the n response tokens), forward AND its
// closed-form gradient in one single-workgroup launch (a minibatch holds a few thousand tokens):
//   pg   = mean(-min(r A, clip(r, 1 +- eps) A)),  r = exp(lp - old)
//   vl   = 0.5 mean((v - R)^2)   [value_clip > 0: 0.5 mean(max((v - R)^2, (vc - R)^2)),
//                                 vc = v_old + clamp(v - v_old, +-value_clip)]
//   ent  = mean(entropy);  loss = pg + c_v vl - c_e ent
//   stats[0..5] = loss, pg, vl, ent, approx_kl = mean(old - lp), clipfrac = mean(|r - 1| > eps)
//   ref != null (KL to the frozen reference in the loss, PPOConfig.kl_in_loss): with d = ref - lp,
//   loss += kl_coef mean(k3), k3 = e^d - d - 1 (the non-negative, unbiased-in-expectation
//   estimator of KL(pi || ref) on tokens drawn from pi); stats[6] = mean(k3), stats[7] =
//   mean(lp - ref) (k1); stats[8] = n (masked tokens); d k3 / d lp = 1 - e^d
//   dlp = d loss / d lp, dv = d loss / d v, dent = d loss / d entropy (per token, 0 off the mask)
// Formulas: reference PPOTrainer.ppo_update (reinforcement_learning_optimization_after_rag.py:212-225)
// at token level, with the SURVEY B5 true-entropy fix. Replaces ~25 tiny elementwise/reduction
// launches (and as many in the backward) per minibatch with one.
__global__ __launch_bounds__(1024) void ppo_loss_kernel(
    const float* __restrict__ lp, const float* __restrict__ old, const float* __restrict__ adv,
    const float* __restrict__ v, const float* __restrict__ ret, const float* __restrict__ vold,
    const float* __restrict__ ent, const float* __restrict__ mask, long n_el, float eps, float c_v, float c_e,
    float vclip, const float* __restrict__ ref, float kl_coef, float* __restrict__ stats, float* __restrict__ dlp,
    float* __restrict__ dv, float* __restrict__ dent) {
  constexpr int NA = 8;
  __shared__ float red[16][NA];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  float acc[NA] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // n, pg, vl, ent, kl, clipfrac, k3, k1 (sums)
  for (long i = tid; i < n_el; i += 1024) {
    const float m = mask[i];
    if (m == 0.f) continue;
    const float r = __expf(lp[i] - old[i]);
    const float A = adv[i];
    const float rc = fminf(fmaxf(r, 1.f - eps), 1.f + eps);
    acc[0] += m;
    acc[1] += m * fmaxf(-r * A, -rc * A);
    const float dvv = v[i] - ret[i];
    float vterm = dvv * dvv;
    if (vclip > 0.f) {
      const float vc = vold[i] + fminf(fmaxf(v[i] - vold[i], -vclip), vclip);
      vterm = fmaxf(vterm, (vc - ret[i]) * (vc - ret[i]));
    }
    acc[2] += m * vterm;
    acc[3] += m * ent[i];
    acc[4] += m * (old[i] - lp[i]);
    acc[5] += m * (fabsf(r - 1.f) > eps ? 1.f : 0.f);
    if (ref) {
      const float d = ref[i] - lp[i];
      acc[6] += m * (__expf(d) - d - 1.f);
      acc[7] -= m * d;
    }
  }
#pragma unroll
  for (int k = 0; k < NA; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < NA; ++k) red[wid][k] = acc[k];
  __syncthreads();
  float tot[NA];
#pragma unroll
  for (int k = 0; k < NA; ++k) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += red[w][k];
    tot[k] = t;
  }
  const float inv_n = 1.f / fmaxf(tot[0], 1.f);
  if (tid == 0) {
    const float pg = tot[1] * inv_n, vl = 0.5f * tot[2] * inv_n, em = tot[3] * inv_n;
    const float k3 = tot[6] * inv_n;
    stats[0] = pg + c_v * vl - c_e * em + (ref && kl_coef != 0.f ? kl_coef * k3 : 0.f);
    stats[1] = pg;
    stats[2] = vl;
    stats[3] = em;
    stats[4] = tot[4] * inv_n;
    stats[5] = tot[5] * inv_n;
    stats[6] = k3;
    stats[7] = tot[7] * inv_n;
    stats[8] = tot[0];
  }
  for (long i = tid; i < n_el; i += 1024) {
    const float m = mask[i];
    float g_lp = 0.f, g_v = 0.f, g_e = 0.f;
    if (m != 0.f) {
      const float r = __expf(lp[i] - old[i]);
      const float A = adv[i];
      const float rc = fminf(fmaxf(r, 1.f - eps), 1.f + eps);
      // -min(rA, rc A): the unclipped branch is active (or tied) -> d/dlp = -A r; the clipped branch
      // only differs when r is outside the range, where clamp has no gradient
      g_lp = (r * A <= rc * A) ? -A * r : 0.f;
      if (ref && kl_coef != 0.f) g_lp += kl_coef * (1.f - __expf(ref[i] - lp[i]));
      const float dvv = v[i] - ret[i];
      float gv = dvv;
      if (vclip > 0.f) {
        const float d0 = v[i] - vold[i];
        const float vc = vold[i] + fminf(fmaxf(d0, -vclip), vclip);
        if ((vc - ret[i]) * (vc - ret[i]) > dvv * dvv) gv = (fabsf(d0) < vclip) ? (vc - ret[i]) : 0.f;
      }
      g_v = c_v * gv;  // d(0.5 x^2)/dx = x
      g_e = -c_e;
      g_lp *= m * inv_n;
      g_v *= m * inv_n;
      g_e *= m * inv_n;
    }
    dlp[i] = g_lp;
    dv[i] = g_v;
    dent[i] = g_e;
  }
}

}  // namespace rt

using namespace rt;

extern "C" int rt_ppo_loss(const float* lp, const float* old, const float* adv, const float* v, const float* ret,
                           const float* vold, const float* ent, const float* mask, long n_el, float eps, float c_v,
                           float c_e, float vclip, const float* ref, float kl_coef, float* stats, float* dlp,
                           float* dv, float* dent, hipStream_t stream) {
  hipLaunchKernelGGL(ppo_loss_kernel, dim3(1), dim3(1024), 0, stream, lp, old, adv, v, ret, vold, ent, mask, n_el,
                     eps, c_v, c_e, vclip, ref, kl_coef, stats, dlp, dv, dent);
  RT_LAUNCH_CHECK();
  return 0;
}

extern "C" int rt_gae(const float* rewards, const float* values, const float* mask, int B, int T, float gamma, float lam,
                      float* adv, float* ret, hipStream_t stream) {
  if (B == 0) return 0;
  hipLaunchKernelGGL(gae_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, rewards, values, mask, B, T, gamma, lam, adv,
                     ret);
  RT_LAUNCH_CHECK();
  return 0;
}

extern "C" int rt_ppo_advantages(const float* old_lp, const float* ref_lp, const float* values, const float* score,
                                 const int* len, int B, int T, float kl_coef, float gamma, float lam, int whiten,
                                 float eps, float* adv, float* ret, float* rew, float* kl_seq, hipStream_t stream) {
  if (B == 0) return 0;
  hipLaunchKernelGGL(ppo_advantages_kernel, dim3(1), dim3(256), 0, stream, old_lp, ref_lp, values, score, len, B, T,
                     kl_coef, gamma, lam, whiten, eps, adv, ret, rew, kl_seq);
  RT_LAUNCH_CHECK();
  return 0;
}

extern "C" int rt_decode_update(const long* tok, long* out_tokens, int max_new, float* out_logp, const float* logp,
                                float* out_values, const float* values, uint8_t* active, int* kv_len, int* pos,
                                long* next_input, int* gen_len, int64_t* step, int64_t* rng_offset, int B,
                                const long* eos_ids, int n_eos, long pad_id, int* attn_len, const int* kv_start,
                                hipStream_t stream) {
  if (B > 1024) return -1;
  hipLaunchKernelGGL(decode_update_kernel, dim3(1), dim3(((B + 63) / 64) * 64), 0, stream, tok, out_tokens, max_new,
                     out_logp, logp, out_values, values, active, kv_len, pos, next_input, gen_len, step, rng_offset, B,
                     eos_ids, n_eos, pad_id, attn_len, kv_start, (const int*)nullptr);
  RT_LAUNCH_CHECK();
  return 0;
}

// The same bookkeeping with a per-row answer length (continuous batching with per-request sampling).
extern "C" int rt_decode_update_rows(const long* tok, long* out_tokens, int max_new, float* out_logp,
                                     const float* logp, float* out_values, const float* values, uint8_t* active,
                                     int* kv_len, int* pos, long* next_input, int* gen_len, int64_t* step,
                                     int64_t* rng_offset, int B, const long* eos_ids, int n_eos, long pad_id,
                                     int* attn_len, const int* kv_start, const int* row_max_new, hipStream_t stream) {
  if (B > 1024 || !row_max_new) return -1;
  hipLaunchKernelGGL(decode_update_kernel, dim3(1), dim3(((B + 63) / 64) * 64), 0, stream, tok, out_tokens, max_new,
                     out_logp, logp, out_values, values, active, kv_len, pos, next_input, gen_len, step, rng_offset, B,
                     eos_ids, n_eos, pad_id, attn_len, kv_start, row_max_new);
  RT_LAUNCH_CHECK();
  return 0;
}
