// Per-request stop strings and stop token ids of the continuous decode batch: after the bookkeeping
// kernel of a decode (or verify) step, each row's newly emitted tokens are turned into bytes through
// the vocabulary byte table and searched for the row's stop strings (docs/DESIGN.md "Per-request stop
// strings").
#include "rt_common.h"

using namespace rt;

#define STOP_MAX_STR 4         // stop strings per row
#define STOP_MAX_LEN 32        // bytes per stop string
#define STOP_MAX_TOK 8         // stop token ids per row
#define STOP_MAX_ENTRY 256     // bytes of the longest vocabulary entry
#define STOP_CHUNK 8           // new tokens staged at a time (a verify step emits at most 8)
#define STOP_CTX (STOP_MAX_LEN - 1)

namespace {

// inclusive prefix sum over the wave's lanes
__device__ __forceinline__ int wave_scan(int v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int u = __shfl_up(v, off, 64);
    if (lane >= off) v += u;
  }
  return v;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long k) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)k, off, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(k >> 32), off, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    k = o < k ? o : k;
  }
  return k;
}

// (offset, length) of token t's entry in the byte table; nothing for an id outside the vocabulary
// or an entry that does not lie inside the blob
__device__ __forceinline__ void entry(long t, const int* __restrict__ offs, int V, int blob_n, int& o, int& l) {
  o = 0;
  l = 0;
  if (t < 0 || t >= V) return;
  const int a = offs[t], e = offs[t + 1];
  if (a < 0 || e < a || e > blob_n) return;
  o = a;
  l = min(e - a, STOP_MAX_ENTRY);
}

}  // namespace

// Row b = blockIdx.x, one wave. The row's generated tokens are out_tokens[b, 0 .. gen_len[b]); their
// table entries, concatenated, are the raw stream; the stream text drops one leading space when
// `strip` is set and the raw stream starts with one (skip = 1). seen[b] tokens and nbytes[b] raw
// bytes are already scanned. The new tokens are taken STOP_CHUNK at a time: buf holds the last
// STOP_CTX raw bytes before the chunk (fewer at the stream start: positions below `lo` are stale and
// never read) followed by the chunk's bytes. A candidate is (stop string i, end position inside the
// chunk's bytes); it matches when the bytes ending there equal the string and it begins at raw
// offset >= skip. A stop token id among the chunk's tokens is a zero-length match where that token
// begins. The winner is the smallest (token that completed the match, match start, kind) with a stop
// token before a string: a wave min over a packed key, no atomics. A hit writes stop_hit, stop_at,
// active = 0 and gen_len = that token's index + 1; no hit writes seen and nbytes.
__global__ __launch_bounds__(64) void stop_rows_kernel(
    const long* __restrict__ out_tokens, long ldt, int T, int* __restrict__ gen_len, uint8_t* __restrict__ active,
    const int* __restrict__ offs, const uint8_t* __restrict__ blob, int V, int blob_n, int strip,
    const int* __restrict__ n_stop, const int* __restrict__ stop_len, const uint8_t* __restrict__ stop_bytes,
    const int* __restrict__ n_stop_tok, const int* __restrict__ stop_tok, int* __restrict__ seen,
    int* __restrict__ nbytes, int* __restrict__ stop_hit, int* __restrict__ stop_at) {
  __shared__ uint8_t buf[STOP_CTX + STOP_CHUNK * STOP_MAX_ENTRY + 1];
  __shared__ uint8_t sstr[STOP_MAX_STR * STOP_MAX_LEN];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int ns = min(max(n_stop[b], 0), STOP_MAX_STR), nt = min(max(n_stop_tok[b], 0), STOP_MAX_TOK);
  const int gl = min(gen_len[b], T);
  int c0 = max(seen[b], 0);
  // workgroup-uniform: nothing new, no stops, or already stopped
  if (c0 >= gl || (ns == 0 && nt == 0) || stop_hit[b] >= 0) return;
  const long* row = out_tokens + (long)b * ldt;

  for (int i = lane; i < STOP_MAX_STR * STOP_MAX_LEN; i += 64) sstr[i] = stop_bytes[(long)b * STOP_MAX_STR * STOP_MAX_LEN + i];
  int slen[STOP_MAX_STR];
#pragma unroll
  for (int i = 0; i < STOP_MAX_STR; ++i)
    slen[i] = i < ns ? min(max(stop_len[b * STOP_MAX_STR + i], 0), STOP_MAX_LEN) : 0;
  int my_stop = -1;  // lane q < nt holds stop token q
  if (lane < nt) my_stop = stop_tok[b * STOP_MAX_TOK + lane];

  // the stripped leading space: the first non-empty entry of the row decides (same address in every lane)
  int skip = 0;
  if (strip) {
    for (int i = 0; i < gl; ++i) {
      int o, l;
      entry(row[i], offs, V, blob_n, o, l);
      if (l > 0) {
        skip = blob[o] == ' ' ? 1 : 0;
        break;
      }
    }
  }

  int base = max(nbytes[b], 0);  // raw offset of the chunk's first byte
  const unsigned long long NONE = ~0ull;
  unsigned long long win = NONE;
  while (c0 < gl) {
    const int n = min(gl - c0, STOP_CHUNK);
    __syncthreads();  // the previous chunk's reads of buf are done
    // ---- context: walk back through the tokens before c0, 64 at a time
    const int want = min(base, STOP_CTX);
    int have = 0;
    for (int tb = c0 - 1; tb >= 0 && have < want; tb -= 64) {
      const int idx = tb - lane;
      int o = 0, l = 0;
      if (idx >= 0) entry(row[idx], offs, V, blob_n, o, l);
      const int cum = wave_scan(l, lane);
      const int d_start = have + cum;  // distance of the entry's first byte from the chunk start
      if (l > 0 && d_start - l < want)
        for (int k = max(0, d_start - want); k < l; ++k) buf[STOP_CTX - d_start + k] = blob[o + k];
      have += __shfl(cum, 63, 64);
    }
    const int lo = STOP_CTX - min(have, want);  // first valid position of buf
    // ---- the chunk's bytes
    int o = 0, l = 0;
    long t = -1;
    if (lane < n) {
      t = row[c0 + lane];
      entry(t, offs, V, blob_n, o, l);
    }
    const int cend = wave_scan(l, lane);  // lane j < n: end of token j inside the chunk's bytes
    const int nb = __shfl(cend, 63, 64);
    for (int j = 0; j < n; ++j) {
      const int oj = __shfl(o, j, 64), lj = __shfl(l, j, 64), sj = __shfl(cend, j, 64) - lj;
      for (int k = lane; k < lj; k += 64) buf[STOP_CTX + sj + k] = blob[oj + k];
    }
    __syncthreads();
    // ---- candidates
    unsigned long long key = NONE;
    // stop token ids: lane j < n checks its token against the ids held by lanes q < nt
    for (int q = 0; q < nt; ++q) {
      const int st = __shfl(my_stop, q, 64);
      if (lane < n && t == (long)st) {
        const unsigned long long k = ((unsigned long long)lane << 40) | ((unsigned long long)(base + cend - l) << 8) | (unsigned)q;
        key = k < key ? k : key;
      }
    }
    int ends[STOP_CHUNK];
#pragma unroll
    for (int j = 0; j < STOP_CHUNK; ++j) ends[j] = __shfl(cend, j, 64);
#pragma unroll
    for (int i = 0; i < STOP_MAX_STR; ++i) {
      const int L = slen[i];
      if (L == 0) continue;
      for (int e = lane; e < nb; e += 64) {
        const int st = STOP_CTX + e + 1 - L;  // match start in buf
        if (st < lo || base - STOP_CTX + st < skip) continue;
        bool eq = true;
        for (int k = L - 1; k >= 0 && eq; --k) eq = buf[st + k] == sstr[i * STOP_MAX_LEN + k];
        if (!eq) continue;
        int j = 0;
#pragma unroll
        for (int q = 0; q < STOP_CHUNK - 1; ++q) j += (e >= ends[q]) ? 1 : 0;  // the token byte e lies in
        const unsigned long long k = ((unsigned long long)j << 40) | ((unsigned long long)(base - STOP_CTX + st) << 8) |
                                     (unsigned)(STOP_MAX_TOK + i);
        key = k < key ? k : key;
      }
    }
    win = wave_min_u64(key);
    if (win != NONE) break;
    c0 += n;
    base += nb;
  }
  if (lane == 0) {
    if (win != NONE) {
      const int j = (int)(win >> 40), start = (int)((win >> 8) & 0xffffffffu), kind = (int)(win & 0xff);
      stop_hit[b] = kind < STOP_MAX_TOK ? STOP_MAX_STR + kind : kind - STOP_MAX_TOK;
      stop_at[b] = max(start - skip, 0);
      active[b] = 0;
      gen_len[b] = c0 + j + 1;
    } else {
      seen[b] = gl;
      nbytes[b] = base;
    }
  }
}

extern "C" int rt_stop_rows(const long* out_tokens, long ldt, int T, int* gen_len, uint8_t* active, const int* offs,
                            const uint8_t* blob, int V, int blob_n, int strip, const int* n_stop, const int* stop_len,
                            const uint8_t* stop_bytes, const int* n_stop_tok, const int* stop_tok, int* seen,
                            int* nbytes, int* stop_hit, int* stop_at, long B, hipStream_t stream) {
  if (V < 1 || T < 1 || ldt < T || blob_n < 0) return -1;
  if (B == 0) return 0;
  hipLaunchKernelGGL(stop_rows_kernel, dim3((unsigned)B), dim3(64), 0, stream, out_tokens, ldt, T, gen_len, active,
                     offs, blob, V, blob_n, strip, n_stop, stop_len, stop_bytes, n_stop_tok, stop_tok, seen, nbytes,
                     stop_hit, stop_at);
  RT_LAUNCH_CHECK();
  return 0;
}
