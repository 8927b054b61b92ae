// RecNet gfx950 kernels: device-side greedy / beam / sampling search, scoring of given captions.
// Included through kernels.hpp.
#pragma once
// =============================================================================================
// inference search on the device (eval.py:19-120): the per-sample Python loops of the reference become kernels
// =============================================================================================
// out[row] = argmax_v x[row, v]  (lowest index among equal maxima), one workgroup per row
__global__ __launch_bounds__(256) void argmax_rows_kernel(const float* __restrict__ x, int ld, int cols, int64_t* __restrict__ out) {
  __shared__ float sv[256]; __shared__ int si[256];
  const int row = blockIdx.x, tid = threadIdx.x;
  float best = -3.0e38f; int bi = 0x7fffffff;
  for (int v = tid; v < cols; v += 256) {
    const float y = x[(size_t)row * ld + v];
    if (y > best || (y == best && v < bi)) { best = y; bi = v; }
  }
  sv[tid] = best; si[tid] = bi;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      const float y = sv[tid + w]; const int j = si[tid + w];
      if (y > sv[tid] || (y == sv[tid] && j < si[tid])) { sv[tid] = y; si[tid] = j; }
    }
    __syncthreads();
  }
  if (tid == 0) out[row] = si[0];
}
// ---- sampling: one token per row drawn from softmax(x / temperature) restricted to the top_k largest logits, by Gumbel-max
// on the project's counter-based hash (the reference has no counterpart; DESIGN.md "Sampling search" states the definition,
// tests/sample_ref.py restates it for the CPU).
#define SR_ROW_LDS_MAX 12288      // floats of a row that are kept in LDS (48 KB); longer rows are re-read from global memory
// order-preserving key of a float: a < b <=> key(a) < key(b); -0 and +0 share a key, like they compare equal
__device__ __forceinline__ uint32_t sr_key(float x) {
  const uint32_t u = __float_as_uint(x == 0.f ? 0.f : x);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
// inclusive prefix sum over the 256 threads of a block, in thread order; sm: 4 ints of LDS scratch
__device__ __forceinline__ int block_scan256(int c, int* sm) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int s = c;
  for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(s, o); if (lane >= o) s += y; }
  __syncthreads();
  if (lane == 63) sm[w] = s;
  __syncthreads();
  for (int j = 0; j < w; ++j) s += sm[j];
  return s;
}
struct SampleArgs {
  const float* x; int V, k, B, t;      // logits [rows][V]; k = 0: every entry allowed, else 0 < k < V; B, t: the (t * B + row) of the draw
  float temp; uint32_t key;            // key = rn_site_key(seed, RN_SITE_SAMPLE)
  int64_t* tok; float* lp;             // [rows]
};
// One workgroup per row.  (1) k > 0: the k-th largest key by a radix select, 8 bits per pass from the top — an LDS histogram of the
// entries that share the prefix found so far, a scan from the top bin down, one thread owns the bin the k-th entry falls in; entries
// equal to the cut value are admitted lowest index first (the order of topk_rows_kernel), by a count over contiguous index chunks
// where they are more than the cut leaves room for.  (2) max of s = x / temp and arg-max of s + g over the allowed entries, lowest
// index among equals.  (3) sum exp(s - max).  Reads the logits only.
template <bool RES> __global__ __launch_bounds__(256) void sample_rows_kernel(const SampleArgs p) {
  extern __shared__ float sr_row[];
  __shared__ int hist[256]; __shared__ float sv[256]; __shared__ int si[256]; __shared__ int sw[4]; __shared__ float sf[4];
  __shared__ uint32_t sel[3];
  const int row = blockIdx.x, tid = threadIdx.x, V = p.V;
  const float* xg = p.x + (size_t)row * V;
  if (RES) {
    for (int v = tid; v < V; v += 256) sr_row[v] = xg[v];
    __syncthreads();
  }
  const float* x = RES ? sr_row : xg;
  // allowed: key > thr, or key == thr and v < cut
  uint32_t thr = 0; int cut = V;
  if (p.k > 0) {
    uint32_t prefix = 0; int krem = p.k, ceq = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
      hist[tid] = 0;
      __syncthreads();
      const uint32_t hi = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
      for (int v = tid; v < V; v += 256) {
        const uint32_t key = sr_key(x[v]);
        if (((key ^ prefix) & hi) == 0) atomicAdd(&hist[(key >> shift) & 255], 1);
      }
      __syncthreads();
      const int c = hist[255 - tid];                                   // thread order = bins from the top down
      const int incl = block_scan256(c, sw), excl = incl - c;
      if (excl < krem && krem <= incl) { sel[0] = 255 - tid; sel[1] = krem - excl; sel[2] = c; }
      __syncthreads();
      prefix |= sel[0] << shift; krem = (int)sel[1]; ceq = (int)sel[2];
    }
    thr = prefix;
    if (krem < ceq) {            // more entries equal to the cut value than the cut admits: the krem lowest indices
      const int C = (V + 255) / 256, v0 = tid * C, v1 = v0 + C < V ? v0 + C : V;
      int c = 0;
      for (int v = v0; v < v1; ++v) c += sr_key(x[v]) == thr;
      const int incl = block_scan256(c, sw), excl = incl - c;
      if (excl < krem && krem <= incl) {
        int need = krem - excl;
        for (int v = v0; v < v1; ++v)
          if (sr_key(x[v]) == thr && --need == 0) { sel[0] = v + 1; break; }
      }
      __syncthreads();
      cut = (int)sel[0];
    }
  }
  const uint32_t base = ((uint32_t)p.t * (uint32_t)p.B + (uint32_t)row) * (uint32_t)V;
  float mx = -INFINITY, best = -INFINITY; int bi = 0x7fffffff;
  for (int v = tid; v < V; v += 256) {
    const float xv = x[v]; const uint32_t key = sr_key(xv);
    if (key > thr || (key == thr && v < cut)) {
      const float s = xv / p.temp;
      const uint32_t h = rn_fmix32((base + (uint32_t)v) * 0x9E3779B1u + p.key);
      const float u = ((float)(h >> 9) + 0.5f) * 0x1p-23f;              // exact in fp32, inside (0, 1)
      const float y = s - logf(-logf(u));
      mx = fmaxf(mx, s);
      if (y > best || (y == best && v < bi)) { best = y; bi = v; }
    }
  }
  mx = block_max256(mx, sf);
  sv[tid] = best; si[tid] = bi;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      const float y = sv[tid + w]; const int j = si[tid + w];
      if (y > sv[tid] || (y == sv[tid] && j < si[tid])) { sv[tid] = y; si[tid] = j; }
    }
    __syncthreads();
  }
  float sum = 0.f;
  for (int v = tid; v < V; v += 256) {
    const float xv = x[v]; const uint32_t key = sr_key(xv);
    if (key > thr || (key == thr && v < cut)) sum += rn_exp(xv / p.temp - mx);
  }
  sum = block_sum256(sum, sf);
  if (tid == 0) {
    const int tok = si[0] < V ? si[0] : 0;                             // (no entry compared: NaN logits)
    p.tok[row] = tok;
    p.lp[row] = (x[tok] / p.temp - mx) - logf(sum);
  }
}
// ---- scoring: the log-probability of a GIVEN token per row (the reference has no counterpart; DESIGN.md section 9 states the
// definitions, tests/score_ref.py restates them for the CPU)
//   lp[row] = s_k - logsumexp_v s_v ,  s_v = x[row, v] / temp ,  k = tok[row] ;  k outside [0, V): lp = -inf, k is never an index
struct LogprobArgs {
  const float* x; int V;               // logits [rows][V], read only
  float temp;
  const int64_t* tok; float* lp;       // [rows]
};
#define LP_NV 20                       // floats of a row per thread that stay in registers (rows up to 5120, like ce_kernel)
// One workgroup per row, the shape of ce_kernel.  RES: the row is loaded once and stays in registers; else it is read from global
// memory twice (max, then sum).  The maximum is subtracted before the exponentials; same formulas as sample_rows_kernel's
// log-probability (s = x / temp, __expf, logf), so that the two agree on a token the sampler drew.
template <bool RES> __global__ __launch_bounds__(256) void logprob_rows_kernel(const LogprobArgs p) {
  __shared__ float sf[4];
  const int row = blockIdx.x, tid = threadIdx.x, V = p.V;
  const float* x = p.x + (size_t)row * V;
  const long k = p.tok[row];
  const bool in_range = k >= 0 && k < V;
  float mx = -INFINITY, sum = 0.f;
  if (RES) {
    float s[LP_NV];
#pragma unroll
    for (int i = 0; i < LP_NV; ++i) { const int v = tid + 256 * i; s[i] = v < V ? x[v] / p.temp : -INFINITY; }
#pragma unroll
    for (int i = 0; i < LP_NV; ++i) mx = fmaxf(mx, s[i]);
    mx = block_max256(mx, sf);
#pragma unroll
    for (int i = 0; i < LP_NV; ++i) sum += tid + 256 * i < V ? rn_exp(s[i] - mx) : 0.f;
  } else {
    for (int v = tid; v < V; v += 256) mx = fmaxf(mx, x[v] / p.temp);
    mx = block_max256(mx, sf);
    for (int v = tid; v < V; v += 256) sum += rn_exp(x[v] / p.temp - mx);
  }
  sum = block_sum256(sum, sf);
  if (tid == 0) p.lp[row] = in_range ? (x[k] / p.temp - mx) - logf(sum) : -INFINITY;
}
// Per-caption reduction over lp [T][B] / tokens [T][B]: e_b = the first t with tokens[t][b] == <EOS> (2), else T - 1;
// len[b] = e_b + 1; sum[b] = lp[0][b] + ... + lp[e_b][b] in ascending t (one thread per caption, no atomics: two calls give the same
// bits).  Rows behind e_b are not read into the sum (they may hold -inf).  The rule of search.sequence_logprob.
__global__ __launch_bounds__(256) void caption_logprob_kernel(const float* __restrict__ lp, const int64_t* __restrict__ tokens, int T,
                                                              int B, float* __restrict__ sum_out, int32_t* __restrict__ len_out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float s = 0.f; int e = T - 1;
  for (int t = 0; t < T; ++t) {
    s += lp[(size_t)t * B + b];
    if (tokens[(size_t)t * B + b] == 2) { e = t; break; }
  }
  sum_out[b] = s; len_out[b] = e + 1;
}
// record the step's tokens; the reference stops after the first step whose tokens are all <PAD> (eval.py:30,116)
__global__ void search_stop_kernel(const int64_t* __restrict__ tokens, int n, int t, int32_t* __restrict__ n_steps) {
  __shared__ int any;
  if (threadIdx.x == 0) any = 0;
  __syncthreads();
  int a = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) a |= (tokens[i] != 0);
  if (a) atomicOr(&any, 1);
  __syncthreads();
  if (threadIdx.x == 0 && !any && *n_steps == 0) *n_steps = t + 1;
}
__global__ void search_finish_kernel(int32_t* n_steps, int tm) { if (*n_steps == 0) *n_steps = tm; }
// scores[b, i*V + v] = log(sigmoid(logits_i[b, v])) + cum[i, b] / len(i, b)^0.7   (eval.py:51-62)
//   len = position of the last <EOS> in hypothesis i of caption b (+1), or t + 1 when it has none
__global__ __launch_bounds__(256) void beam_score_kernel(const float* __restrict__ logits, const float* __restrict__ cum,
                                                         const int32_t* __restrict__ last_eos, float* __restrict__ scores,
                                                         int B, int V, int nb, int i, int t) {
  const int b = blockIdx.x;
  const int le = last_eos[i * B + b];
  const double len = le >= 0 ? (double)(le + 1) : (double)(t + 1);
  const float norm = cum[i * B + b] / (float)pow(len, 0.7);
  const float* x = logits + (size_t)b * V;
  float* o = scores + (size_t)b * nb * V + (size_t)i * V;
  for (int v = threadIdx.x; v < V; v += 256) o[v] = logf(1.0f / (1.0f + expf(-x[v]))) + norm;
}
// top-k (k <= 8) of each row of scores [B][n], descending, lowest index first among equals; destroys scores
__global__ __launch_bounds__(256) void topk_rows_kernel(float* __restrict__ scores, int n, int k, float* __restrict__ vals,
                                                        int32_t* __restrict__ idx) {
  __shared__ float sv[256]; __shared__ int si[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  float* x = scores + (size_t)b * n;
  for (int j = 0; j < k; ++j) {
    float best = -INFINITY; int bi = 0x7fffffff;
    for (int v = tid; v < n; v += 256) {
      const float y = x[v];
      if (y > best || (y == best && v < bi)) { best = y; bi = v; }
    }
    sv[tid] = best; si[tid] = bi;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w) {
        const float y = sv[tid + w]; const int q = si[tid + w];
        if (y > sv[tid] || (y == sv[tid] && q < si[tid])) { sv[tid] = y; si[tid] = q; }
      }
      __syncthreads();
    }
    if (tid == 0) {
      vals[b * k + j] = sv[0]; idx[b * k + j] = si[0];
      if (si[0] < n) x[si[0]] = -INFINITY;
    }
    __syncthreads();
  }
}
// regather the hypotheses: new beam k of caption b continues old beam src = idx / V with token idx % V (eval.py:66-114)
struct BeamUpdArgs {
  int B, H, V, Tm, bw, t;
  const float* vals; const int32_t* idx;                 // [B][bw]
  const float* h_next; const float* c_next;              // [nb_old][B][H] states after this step
  const int32_t* last_eos_old; const int64_t* hist_old;  // [nb_old][B], [nb_old][B][Tm]
  float* h_new; float* c_new; float* cum_new; int32_t* last_eos_new; int64_t* hist_new; int64_t* tok_new;
  const int32_t* n_steps;                                // != 0: the search already stopped (eval.py:116)
};
__global__ __launch_bounds__(128) void beam_update_kernel(const BeamUpdArgs p) {
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  int flat = p.idx[b * p.bw + k];
  // The reference leaves its loop at the first step whose tokens are all <PAD>; the device loop has a fixed trip
  // count, so from then on the hypotheses are carried over unchanged (same beam order, <PAD> appended).
  if (*p.n_steps != 0) flat = k * p.V;
  const int src = flat / p.V, tok = flat % p.V;
  const size_t so = ((size_t)src * p.B + b), dn = ((size_t)k * p.B + b);
  for (int j = tid; j < p.H; j += 128) {
    p.h_new[dn * p.H + j] = p.h_next[so * p.H + j];
    p.c_new[dn * p.H + j] = p.c_next[so * p.H + j];
  }
  for (int j = tid; j < p.Tm; j += 128) p.hist_new[dn * p.Tm + j] = j < p.t ? p.hist_old[so * p.Tm + j] : (j == p.t ? (int64_t)tok : 0);
  if (tid == 0) {
    p.cum_new[dn] = p.vals[b * p.bw + k];
    p.last_eos_new[dn] = tok == 2 ? p.t : p.last_eos_old[so];
    p.tok_new[dn] = tok;
  }
}
// best[t][b] = hist[beam 0][b][t]
__global__ void beam_best_kernel(const int64_t* __restrict__ hist, int64_t* __restrict__ best, int B, int Tm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * Tm) return;
  const int t = i / B, b = i % B;
  best[i] = hist[(size_t)b * Tm + t];
}

