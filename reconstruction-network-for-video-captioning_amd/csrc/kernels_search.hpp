// RecNet gfx950 kernels: device-side greedy / beam / sampling search, scoring of given captions.
// Included through kernels.hpp.
#pragma once
// =============================================================================================
// inference search on the device (eval.py:19-120): the per-sample Python loops of the reference become kernels
// =============================================================================================
// Arg-max over the 256 threads of a block on 256 floats / ints of LDS each: the larger value wins, the lowest index among equal
// values.  Every thread brings its own candidate; after the call sv[0] / si[0] hold the winner, for every thread to read.
__device__ __forceinline__ void block_argmax256(float value, int index, float* sv, int* si) {
  const int tid = threadIdx.x;
  sv[tid] = value; si[tid] = index;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      const float y = sv[tid + w]; const int j = si[tid + w];
      if (y > sv[tid] || (y == sv[tid] && j < si[tid])) { sv[tid] = y; si[tid] = j; }
    }
    __syncthreads();
  }
}
// out[row] = argmax_v x[row, v]  (lowest index among equal maxima), one workgroup per row
__global__ __launch_bounds__(256) void argmax_rows_kernel(const float* __restrict__ x, int ld, int cols, int64_t* __restrict__ out) {
  __shared__ float sv[256]; __shared__ int si[256];
  const int row = blockIdx.x, tid = threadIdx.x;
  float best = -3.0e38f; int bi = 0x7fffffff;
  for (int v = tid; v < cols; v += 256) {
    const float y = x[(size_t)row * ld + v];
    if (y > best || (y == best && v < bi)) { best = y; bi = v; }
  }
  block_argmax256(best, bi, sv, si);
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
// The nucleus form (tests/nucleus_ref.py restates it): after the top-k cut, the shortest prefix of the allowed
// entries, in the same order, whose mass reaches top_p of the mass of all of them.  top_p = 1: no nucleus cut, the select is skipped.
struct SampleNucArgs : SampleArgs {
  float top_p;                         // in (0, 1]; below 1: V < 2^21, so that the sum of the masses stays below 2^53
  int32_t* n_allowed;                  // [rows], the size of the set drawn from (may be null)
};
template <bool NUC> struct SampleArgsOf { typedef SampleArgs type; };
template <> struct SampleArgsOf<true> { typedef SampleNucArgs type; };
// the float of an order-preserving key (-0 and +0 come back as +0)
__device__ __forceinline__ float sr_unkey(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }
// The integer mass of an entry: floor(exp(s - m) * 2^32), s - m <= 0 and the exponential in fp32 (rn_exp, the one of the
// log-probability).  The scale is a power of two, so the product is exact; the clamps make the conversion defined for every input
// (a NaN becomes 0), and everything the select does with the masses afterwards is integer arithmetic.
__device__ __forceinline__ unsigned long long sr_mass(float xv, float temp, float m) {
  const float f = fminf(fmaxf(rn_exp(xv / temp - m) * 0x1p32f, 0.f), 0x1p32f);
  return f >= 0x1p32f ? 1ull << 32 : (unsigned long long)(uint32_t)f;
}
// inclusive prefix sum of 64-bit words over the 256 threads of a block, in thread order; sm: 4 words of LDS scratch
__device__ __forceinline__ unsigned long long block_scan256_u64(unsigned long long c, unsigned long long* sm) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned long long s = c;
  for (int o = 1; o < 64; o <<= 1) { const unsigned long long y = __shfl_up(s, o); if (lane >= o) s += y; }
  __syncthreads();
  if (lane == 63) sm[w] = s;
  __syncthreads();
  for (int j = 0; j < w; ++j) s += sm[j];
  return s;
}
// Of the entries equal to the cut value (key == thr) the `need` lowest indices are admitted, need >= 1 and fewer than there are:
// every thread counts its equal entries over a contiguous index chunk, a scan, and the thread that owns the need-th one walks to it
// and publishes its index + 1 in sel[0], which every thread takes as `cut`.  A statement of sample_rows_kernel on its x, V, tid, thr,
// sw, sel and cut — a macro, not a function, so that the top-k cut expands to the statements it always had and the instantiations
// without a nucleus keep their code to the instruction.
#define SR_EQUAL_CUT(NEED)                                                                                   \
  {                                                                                                          \
    const int C = (V + 255) / 256, v0 = tid * C, v1 = v0 + C < V ? v0 + C : V;                               \
    int c = 0;                                                                                               \
    for (int v = v0; v < v1; ++v) c += sr_key(x[v]) == thr;                                                  \
    const int incl = block_scan256(c, sw), excl = incl - c;                                                  \
    if (excl < NEED && NEED <= incl) {                                                                       \
      int need = NEED - excl;                                                                                \
      for (int v = v0; v < v1; ++v)                                                                          \
        if (sr_key(x[v]) == thr && --need == 0) { sel[0] = v + 1; break; }                                   \
    }                                                                                                        \
    __syncthreads();                                                                                         \
    cut = (int)sel[0];                                                                                       \
  }
// One workgroup per row.  (1) k > 0: the k-th largest key by a radix select, 8 bits per pass from the top — an LDS histogram of the
// entries that share the prefix found so far, a scan from the top bin down, one thread owns the bin the k-th entry falls in; entries
// equal to the cut value are admitted lowest index first (the order of topk_rows_kernel), by a count over contiguous index chunks
// where they are more than the cut leaves room for.  (2) max of s = x / temp and arg-max of s + g over the allowed entries, lowest
// index among equals.  (3) sum exp(s - max).  Reads the logits only.
// NUC, top_p < 1, between (1) and (2): the allowed set is a prefix of one total order (key descending, index ascending), and so is
// the nucleus; the same radix walk finds its end by mass instead of by count.  One pass takes m = max s over the allowed entries.
// Then per 8 bits a histogram of 256 64-bit sums (ds_add_u64) of the integer masses sr_mass of the allowed entries that share the
// prefix found so far, a 64-bit scan from the top bin down, and the one thread whose bin crosses the remaining target publishes
// digit, remaining target and bin mass; the first pass's grand total Q gives target = max(1, ceil(top_p * Q)) in float64 (exact:
// Q < 2^53).  Integer sums do not depend on the order the atomics arrive in: two calls give the same nucleus.  After four passes
// the cut value and the mass still missing at it are known; its entries all carry one mass q, so ceil(missing / q) of them are
// admitted, lowest indices first (SR_EQUAL_CUT), and the result is again (thr, cut): (2) and (3) are unchanged.  The sel64 words a
// pass reads are given defaults inside that pass, so a row of NaN / inf, whose masses are meaningless, leaves a meaningless but
// in-range (thr, cut).  (3) also counts the allowed entries for n_allowed.
template <bool RES, bool NUC = false> __global__ __launch_bounds__(256)
void sample_rows_kernel(const typename SampleArgsOf<NUC>::type p) {
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
    if (krem < ceq) SR_EQUAL_CUT(krem)   // more entries equal to the cut value than the cut admits: the krem lowest indices
  }
  if constexpr (NUC) {
    if (p.top_p < 1.f) {                                               // (uniform over the grid)
      __shared__ unsigned long long hist64[256], sw64[5], sel64[3];
      float m = -INFINITY;
      for (int v = tid; v < V; v += 256) {
        const float xv = x[v]; const uint32_t key = sr_key(xv);
        if (key > thr || (key == thr && v < cut)) m = fmaxf(m, xv / p.temp);
      }
      m = block_max256(m, sf);
      uint32_t prefix = 0; unsigned long long rem = 1ull, qeq = 0ull;
      for (int shift = 24; shift >= 0; shift -= 8) {
        hist64[tid] = 0ull;
        __syncthreads();
        if (tid == 0) { sel64[0] = 0ull; sel64[1] = 1ull; sel64[2] = 0ull; }   // (what the pass leaves when no bin crosses: NaN rows)
        const uint32_t hi = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        for (int v = tid; v < V; v += 256) {
          const float xv = x[v]; const uint32_t key = sr_key(xv);
          if (((key ^ prefix) & hi) == 0 && (key > thr || (key == thr && v < cut)))
            atomicAdd(&hist64[(key >> shift) & 255], sr_mass(xv, p.temp, m));
        }
        __syncthreads();
        const unsigned long long c = hist64[255 - tid];                // thread order = bins from the top down
        const unsigned long long incl = block_scan256_u64(c, sw64), excl = incl - c;
        if (shift == 24) {                                             // the grand total Q: target = max(1, ceil(top_p * Q))
          if (tid == 255) sw64[4] = incl;                              // (a word the scan does not use)
          __syncthreads();
          const double tq = ceil((double)p.top_p * (double)sw64[4]);
          rem = tq >= 1.0 ? (unsigned long long)tq : 1ull;             // (tq <= Q < 2^53; a NaN takes the 1)
        }
        if (excl < rem && rem <= incl) { sel64[0] = 255 - tid; sel64[1] = rem - excl; sel64[2] = c; }
        __syncthreads();
        prefix |= (uint32_t)sel64[0] << shift; rem = sel64[1]; qeq = sel64[2];
      }
      // the entries equal to the cut value carry one mass q each: qeq / q of them are allowed, ceil(rem / q) are admitted
      unsigned long long q = sr_mass(sr_unkey(prefix), p.temp, m);
      q = q ? q : 1ull;
      const unsigned long long neq64 = (rem + q - 1ull) / q;
      if (prefix != thr) cut = V;                                      // above the top-k cut value: no index cut so far
      thr = prefix;
      if (neq64 < qeq / q) {
        const int neq = (int)neq64;
        if (tid == 0) sel[0] = (uint32_t)V;                            // (published before the scan's barriers inside)
        SR_EQUAL_CUT(neq)
      }
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
  block_argmax256(best, bi, sv, si);
  float sum = 0.f; int na = 0;
  for (int v = tid; v < V; v += 256) {
    const float xv = x[v]; const uint32_t key = sr_key(xv);
    if (key > thr || (key == thr && v < cut)) { sum += rn_exp(xv / p.temp - mx); if (NUC) ++na; }
  }
  sum = block_sum256(sum, sf);
  if constexpr (NUC) {
    if (p.n_allowed) {                                                 // (uniform over the grid)
      na = block_scan256(na, sw);
      if (tid == 255) p.n_allowed[row] = na;
    }
  }
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
// The search stops after the first step that leaves nothing alive.  tokens given: some token of the step is not <PAD> (the reference
// stops after the first step whose tokens are all <PAD>, eval.py:30,116); tokens null: some hypothesis of fin is not finished (the
// N-best search).
__global__ void search_stop_kernel(const int64_t* __restrict__ tokens, const int32_t* __restrict__ fin, int n, int t,
                                   int32_t* __restrict__ n_steps) {
  __shared__ int live;
  if (threadIdx.x == 0) live = 0;
  __syncthreads();
  int a = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) a |= tokens ? tokens[i] != 0 : fin[i] == 0;
  if (a) atomicOr(&live, 1);
  __syncthreads();
  if (threadIdx.x == 0 && !live && *n_steps == 0) *n_steps = t + 1;
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
    block_argmax256(best, bi, sv, si);
    if (tid == 0) {
      vals[b * k + j] = sv[0]; idx[b * k + j] = si[0];
      if (si[0] < n) x[si[0]] = -INFINITY;
    }
    __syncthreads();
  }
}
// Regather the hypotheses: new beam k of caption b continues old beam src = idx / V with token idx % V (eval.py:66-114).  Two forms of
// the per-hypothesis <EOS> word.  Reference search (NBEST false): the position of the last <EOS>, -1 without one; once the search has
// stopped the hypotheses are frozen.  N-best search (NBEST true): fin = position of the first <EOS> + 1 (the length), 0 while it has
// none; only <EOS> (2) finishes a hypothesis, and a finished one stays so.
struct BeamUpdArgs {
  int B, H, V, Tm, bw, t;
  const float* vals; const int32_t* idx;                 // [B][bw]
  const float* h_next; const float* c_next;              // [nb_old][B][H] states after this step (c_next null: a GRU has no c)
  const int32_t* eos_old; const int64_t* hist_old;       // [nb_old][B], [nb_old][B][Tm]
  float* h_new; float* c_new; float* cum_new; int32_t* eos_new; int64_t* hist_new; int64_t* tok_new;
  const int32_t* n_steps;                                // reference search only; != 0: the search already stopped (eval.py:116)
  const float* gum_vals = nullptr; float* gum_new = nullptr;   // stochastic beam search only (section 21): the perturbed scores [B][bw] of
                                                         // the selection, regathered beside cum into [bw][B]; null everywhere else
};
template <bool NBEST> __global__ __launch_bounds__(128) void beam_update_kernel(const BeamUpdArgs p) {
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  int flat = p.idx[b * p.bw + k];
  // The reference leaves its loop at the first step whose tokens are all <PAD>; the device loop has a fixed trip
  // count, so from then on the hypotheses are carried over unchanged (same beam order, <PAD> appended).
  if (!NBEST && *p.n_steps != 0) flat = k * p.V;
  const int src = flat / p.V, tok = flat % p.V;
  const size_t so = ((size_t)src * p.B + b), dn = ((size_t)k * p.B + b);
  for (int j = tid; j < p.H; j += 128) {
    p.h_new[dn * p.H + j] = p.h_next[so * p.H + j];
    if (p.c_next) p.c_new[dn * p.H + j] = p.c_next[so * p.H + j];
  }
  for (int j = tid; j < p.Tm; j += 128) p.hist_new[dn * p.Tm + j] = j < p.t ? p.hist_old[so * p.Tm + j] : (j == p.t ? (int64_t)tok : 0);
  if (tid == 0) {
    const int e = p.eos_old[so];
    p.cum_new[dn] = p.vals[b * p.bw + k];
    if (NBEST && p.gum_new) p.gum_new[dn] = p.gum_vals[b * p.bw + k];
    p.eos_new[dn] = NBEST ? (e ? e : (tok == 2 ? p.t + 1 : 0)) : (tok == 2 ? p.t : e);
    p.tok_new[dn] = tok;
  }
}
// tokens[r][t][b] = hist[order[r][b]][b][t] for the bw ranks of order; order null: beam 0 (bw = 1, the reference search's best)
__global__ void beam_gather_kernel(const int64_t* __restrict__ hist, const int32_t* __restrict__ order, int64_t* __restrict__ tokens,
                                   int B, int Tm, int bw) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= bw * Tm * B) return;
  const int b = i % B, t = (i / B) % Tm, r = i / (B * Tm);
  tokens[i] = hist[((size_t)(order ? order[r * B + b] : 0) * B + b) * Tm + t];
}

// =============================================================================================
// N-best beam search on log-probabilities (the reference has no counterpart; DESIGN.md section 11 states the definitions,
// tests/beam_ref.py restates them for the CPU).  recnet_beam_search above stays the reference's search.
// =============================================================================================
// A candidate (value y, flat index j) as one 64-bit word that orders like the selection: the larger value first, the lower index
// among equal values (the order of topk_rows_kernel); -0 and +0, and all -inf, share a value key.  0 is below every candidate.
__device__ __forceinline__ unsigned long long bs_pack(float y, int j) {
  return ((unsigned long long)sr_key(y) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)j);
}
__device__ __forceinline__ float bs_value(unsigned long long c) {
  const uint32_t k = (uint32_t)(c >> 32);
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}
__device__ __forceinline__ int bs_index(unsigned long long c) { return (int)(0xFFFFFFFFu - (uint32_t)c); }
struct BeamSelArgs {
  const float* x;                      // logits [nb][rows][V], read only
  const float* cum;                    // [nb][rows]
  const int32_t* fin;                  // [nb][rows], != 0: the hypothesis is finished
  int nb, rows, V;
  float* vals; int32_t* idx;           // [rows][BW], descending; idx = i * V + v
};
// The constrained form (tests/beam_constrained_ref.py restates it): a live hypothesis with the generated history
// w_0 .. w_{t-1} (its hist row) does not offer token v when v is one of the static bans, when v = <EOS> and t < min_len, or when
// ngram = n >= 1 and appending v would repeat an n-gram of the history.  Finished hypotheses are untouched.
struct BeamSelCArgs : BeamSelArgs {
  const int64_t* hist;                 // [nb][rows][Tm], entries [0, t) are read (may be null when ngram = 0)
  int Tm, t, ngram, min_len, n_banned; // 0 <= t < Tm; ngram, min_len in [0, Tm); n_banned in [0, 16]
  int32_t banned[16];                  // distinct ids in [0, V), none of them <EOS>
};
template <bool CONSTRAINED> struct BeamSelArgsOf { typedef BeamSelArgs type; };
template <> struct BeamSelArgsOf<true> { typedef BeamSelCArgs type; };
// dynamic LDS of the constrained form: 8 list lengths, then per hypothesis a ban list of at most t + 17 ids
__host__ __device__ __forceinline__ int bs_ban_stride(int t) { return t + 17; }
// The text that beam_select_kernel and beam_select_groups_kernel share, each piece written once: the bit-for-bit promises between the
// two (and with logprob_rows_kernel) rest on it being ONE text.  Statements on the kernels' own names (p, r, tid, V, nb, S, bs_ban, sf,
// s_mx, s_ls, wc, lane, wave, lc and the walk's nban, ban, v) — macros like SR_EQUAL_CUT, not functions: the constrained instantiations
// sit at 104-106 SGPRs, and a function that takes the argument struct (by reference or by value) moves the loads of the 16 banned ids
// and makes the compiler save scalars into vector lanes; the textual form compiles to the code the kernels
// had.  What the phases do and why is told at beam_select_kernel.
// Phase (0), constrained form only: one wave per live hypothesis writes its ban list into LDS; sets S.
#define BS_BAN_LISTS                                                                                                       \
  {                                                                                                                        \
    S = bs_ban_stride(p.t);                                                                                                \
    const int ln = tid & 63, t = p.t, n = p.ngram;                                                                         \
    const int ng = n >= 1 && t >= n - 1 ? t - n + 1 : 0;                                                                   \
    const int used = ng + p.n_banned + (t < p.min_len ? 1 : 0);                 /* <= t + 17 */                            \
    for (int i = tid >> 6; i < nb; i += 4) {                                                                               \
      const bool live = p.fin[i * p.rows + r] == 0;                                                                        \
      int cnt = 0;                                                                                                         \
      for (int c = 0; c < used; c += 64) {                                      /* (uniform over the wave) */              \
        const int j = c + ln;                                                                                              \
        int id = -1;                                                                                                       \
        if (live && j < ng) {                                                   /* (ng > 0 only with ngram >= 1: hist is not null) */ \
          const int64_t* hs = p.hist + ((size_t)i * p.rows + r) * p.Tm;                                                    \
          bool same = true;                                                                                                \
          for (int k = 0; k + 1 < n; ++k) same &= hs[j + k] == hs[t - n + 1 + k];                                          \
          const int64_t w = hs[j + n - 1];                                                                                 \
          if (same && w >= 0 && w < V) id = (int)w;                                                                        \
        } else if (live && j < used) {                                                                                     \
          const int s = j - ng;                                                                                            \
          id = 2;                                                               /* behind the static bans: <EOS> while t < min_len */ \
          _Pragma("unroll")                                                                                                \
          for (int k = 0; k < 16; ++k)                                                                                     \
            if (s == k && k < p.n_banned) id = p.banned[k];                                                                \
        }                                                                                                                  \
        const unsigned long long m = __ballot(id >= 0);                                                                    \
        if (id >= 0) bs_ban[8 + i * S + cnt + __popcll(m & ((1ull << ln) - 1ull))] = id;                                   \
        cnt += __popcll(m);                                                                                                \
      }                                                                                                                    \
      if (ln == 0) bs_ban[i] = cnt;                                                                                        \
    }                                                                                                                      \
  }
// Phase (1): per live hypothesis the maximum and log sum exp(x - max) of its row into s_mx / s_ls, logprob_rows_kernel's formulas and
// summation order.  The caller's next barrier publishes them (and the ban lists).
#define BS_ROW_STATS                                                                                                       \
  for (int i = 0; i < nb; ++i) {                                                                                           \
    if (p.fin[i * p.rows + r]) continue;                               /* (uniform over the workgroup) */                  \
    const float* x = p.x + ((size_t)i * p.rows + r) * V;                                                                   \
    float mx = -INFINITY, sum = 0.f;                                                                                       \
    for (int v = tid; v < V; v += 256) mx = fmaxf(mx, x[v]);                                                               \
    mx = block_max256(mx, sf);                                                                                             \
    for (int v = tid; v < V; v += 256) sum += rn_exp(x[v] - mx);                                                           \
    sum = block_sum256(sum, sf);                                                                                           \
    if (tid == 0) { s_mx[i] = mx; s_ls[i] = logf(sum); }                                                                   \
  }
// Phase (2), once per hypothesis before the walk: declares `mine`, the banned id this thread can meet (v = tid (mod 256)), and `many`
// (it has two or more different ones), from the list ban[0 .. nban).
#define BS_OWN_BAN                                                                                                         \
  int mine = -1; bool many = false;                                                                                        \
  if constexpr (CONSTRAINED) {                                                                                             \
    for (int j = 0; j < nban; ++j) {                                                                                       \
      const int id = ban[j];                                                                                               \
      if ((id & 255) == tid) { many |= mine >= 0 && mine != id; mine = id; }                                               \
    }                                                                                                                      \
  }
// Phase (2), behind the compare that guards an insertion: declares `offered`, whether candidate v is not banned.
#define BS_OFFERED                                                                                                         \
  bool offered = true;                                                                                                     \
  if constexpr (CONSTRAINED) {                                                                                             \
    offered = v != mine;                                                                                                   \
    if (many)                                                          /* (two banned ids 256 apart or more: rare) */      \
      for (int j = 0; j < nban; ++j) offered &= ban[j] != v;                                                               \
  }
// Phase (3), round K: declares `e`, the largest list head lc[0] of the workgroup (0: no candidate left), the same word in every thread:
// a butterfly over the wave, then the four wave maxima through wc[K & 1] (two buffers: one barrier per round).
#define BS_ARGMAX_ROUND(K)                                                                                                 \
  unsigned long long e = lc[0];                                                                                            \
  _Pragma("unroll")                                                                                                        \
  for (int o = 32; o > 0; o >>= 1) {                                                                                       \
    const unsigned long long d = __shfl_xor(e, o);                                                                         \
    e = d > e ? d : e;                                                                                                     \
  }                                                                                                                        \
  if (lane == 0) wc[(K) & 1][wave] = e;                                                                                    \
  __syncthreads();                                                                                                         \
  e = wc[(K) & 1][0];                                                                                                      \
  _Pragma("unroll")                                                                                                        \
  for (int w = 1; w < 4; ++w) e = wc[(K) & 1][w] > e ? wc[(K) & 1][w] : e;
// One workgroup per caption.  (1) Per hypothesis the maximum and sum exp(x - max) of its row, the formulas and summation order of
// logprob_rows_kernel at temperature 1, so that the two agree on a token to the bit.  (2) Every thread walks its strided share of
// the nb * V candidates cum_i + ((x_v - max_i) - log sum_i) in ascending flat index and keeps its best BW in registers (the insertion
// is a fully unrolled compare-exchange chain: no runtime-indexed register array, nothing in scratch).  A finished hypothesis offers
// <PAD> (0) at cum_i and -inf elsewhere: only its first BW + 1 entries can be selected, the others are not visited.  (3) BW block
// arg-max rounds over the list heads; the thread that owned the winner shifts its list.  Value and index travel as one 64-bit word
// (bs_pack): one integer compare orders two candidates.  No score array, one pass over the logits for all winners, no atomics: two
// calls give the same bits.
// CONSTRAINED: (0) one wave per live hypothesis writes its ban list into LDS, 64 entries at a time: lane j < t - n + 1 compares the
// n - 1 tokens at j with the last n - 1 and bans hist[j + n - 1] on a match; the static bans and the conditional <EOS> follow; a
// ballot packs the entries that hold an id, in lane order (duplicates stay, they are harmless).  The barrier that ends (1) publishes
// the lists.  In (2) a thread only ever meets the tokens v = tid (mod 256), so once per hypothesis it reads the list and keeps the
// one banned id of its own residue in a register (`many`: it has two or more, then the list is scanned); the test sits behind the
// compare that guards an insertion, so the common path keeps its one compare and the walk reads no LDS (scanning the list there
// instead costs 50-90 %: a wave takes the branch whenever one of its 64 lanes inserts).  A banned candidate
// enters no thread's list and (3) is unchanged.  The values of the offered candidates are those of the unconstrained form, bit for
// bit: (1) still runs over all V entries (no renormalisation).
template <int BW, bool CONSTRAINED = false> __global__ __launch_bounds__(256)
void beam_select_kernel(const typename BeamSelArgsOf<CONSTRAINED>::type p) {
  __shared__ float sf[4]; __shared__ float s_mx[8], s_ls[8]; __shared__ unsigned long long wc[2][4];
  extern __shared__ __attribute__((aligned(16))) int bs_ban[];
  const int r = blockIdx.x, tid = threadIdx.x, V = p.V, nb = p.nb;
  int S = 0;
  if constexpr (CONSTRAINED) BS_BAN_LISTS
  BS_ROW_STATS
  __syncthreads();
  unsigned long long lc[BW];
#pragma unroll
  for (int k = 0; k < BW; ++k) lc[k] = 0ull;
  for (int i = 0; i < nb; ++i) {
    const float c = p.cum[i * p.rows + r];
    const bool fin = p.fin[i * p.rows + r] != 0;
    const float* x = p.x + ((size_t)i * p.rows + r) * V;
    const float mx = fin ? 0.f : s_mx[i], ls = fin ? 0.f : s_ls[i];
    const int n = fin ? (V < BW + 1 ? V : BW + 1) : V;
    const int nban = CONSTRAINED ? bs_ban[i] : 0;                      // (0 for a finished hypothesis)
    const int* ban = bs_ban + 8 + i * S;
    BS_OWN_BAN
    for (int v = tid; v < n; v += 256) {
      const float y = fin ? (v == 0 ? c : -INFINITY) : c + ((x[v] - mx) - ls);
      unsigned long long e = bs_pack(y, i * V + v);
      if (e > lc[BW - 1]) {
        BS_OFFERED
        if (offered) {
#pragma unroll
          for (int k = 0; k < BW; ++k)
            if (e > lc[k]) { const unsigned long long d = lc[k]; lc[k] = e; e = d; }
        }
      }
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
  for (int k = 0; k < BW; ++k) {
    BS_ARGMAX_ROUND(k)
    if (e != 0ull && lc[0] == e) {           // (candidates are distinct: their indices are)
#pragma unroll
      for (int q = 0; q + 1 < BW; ++q) lc[q] = lc[q + 1];
      lc[BW - 1] = 0ull;
    }
    if (tid == 0) {                           // (e == 0: fewer than BW candidates compared, NaN-free inputs never get here)
      p.vals[(size_t)r * BW + k] = e ? bs_value(e) : -INFINITY; p.idx[(size_t)r * BW + k] = e ? bs_index(e) : 0;
    }
  }
}
// ---- diverse (group) beam search (Vijayakumar et al., "Diverse Beam Search"; the reference has no counterpart; DESIGN.md section 14
// states the definition, tests/beam_diverse_ref.py restates it): the BW = G * W slots of a caption are G groups of W.  The groups of a
// step are decided one after the other, and a live candidate of group g pays lam for every slot of the groups before it whose winner
// of THIS step came from a live hypothesis and carries the same token.  The penalty orders the selection only: vals is the
// un-penalised value.
struct BeamGrpArgs { int G; float lam; };        // G >= 2 groups (one group is beam_select_kernel's), lam finite and >= 0
// beam_select_kernel's launch shape and its phases (0) and (1), once for all nb hypotheses (nb = 1: every group selects from
// hypothesis 0; else nb = G * W and group g owns hypotheses g * W .. g * W + W - 1).  Then per group, inside the workgroup: (2) the
// walk over the group's candidates with a list of W, (3) W arg-max rounds.  The thread that owned a winner recomputes its
// un-penalised value from the index (the same expression as the walk's: the same bits), writes the output pair and, for a live
// hypothesis, appends the token to s_tok, the at most 7 tokens chosen so far in this step (a token chosen twice stands twice); a
// barrier, then the next group.  A penalised candidate is worth less than its pure value (lam * c >= 0, the subtraction is monotone),
// so one that does not beat the tail of the thread's list with its PURE value cannot enter it: the penalty is looked up behind the
// compare that guards an insertion, as the ban lists are, and the candidate is then compared again with its penalised value.  A
// thread only meets the tokens v = tid (mod 256): once per group it reads s_tok and keeps the one chosen token of its residue and
// its count in registers (`pmany`: two different ones, then the list is scanned).  A candidate with count 0 is compared by exactly
// the word beam_select_kernel forms: group 0, and every group at lam = 0, select what that kernel selects at width W, bit for bit.
template <int W, bool CONSTRAINED = false> __global__ __launch_bounds__(256)
void beam_select_groups_kernel(const typename BeamSelArgsOf<CONSTRAINED>::type p, const BeamGrpArgs q) {
  __shared__ float sf[4]; __shared__ float s_mx[8], s_ls[8]; __shared__ unsigned long long wc[2][4];
  __shared__ int s_tok[8]; __shared__ int s_ntok;
  extern __shared__ __attribute__((aligned(16))) int bs_ban[];
  const int r = blockIdx.x, tid = threadIdx.x, V = p.V, nb = p.nb, BW = q.G * W;
  int S = 0;
  if constexpr (CONSTRAINED) BS_BAN_LISTS                              // (0)
  BS_ROW_STATS                                                         // (1)
  if (tid == 0) s_ntok = 0;
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  for (int g = 0; g < q.G; ++g) {
    const int nt = s_ntok;                                             // (<= 7: the last group appends nothing that is read)
    int ptok = -1, pcnt = 0; bool pmany = false;                       // the chosen token this thread can meet, and how often chosen
    for (int j = 0; j < nt; ++j) {
      const int id = s_tok[j];
      if ((id & 255) == tid) {
        if (ptok < 0 || ptok == id) { ptok = id; ++pcnt; } else pmany = true;
      }
    }
    unsigned long long lc[W];
#pragma unroll
    for (int k = 0; k < W; ++k) lc[k] = 0ull;
    const int i0 = nb == 1 ? 0 : g * W, i1 = nb == 1 ? 1 : g * W + W;
    for (int i = i0; i < i1; ++i) {                                    // (2)
      const float c = p.cum[i * p.rows + r];
      const bool fin = p.fin[i * p.rows + r] != 0;
      const float* x = p.x + ((size_t)i * p.rows + r) * V;
      const float mx = fin ? 0.f : s_mx[i], ls = fin ? 0.f : s_ls[i];
      const int n = fin ? (V < W + 1 ? V : W + 1) : V;
      const int nban = CONSTRAINED ? bs_ban[i] : 0;                    // (0 for a finished hypothesis)
      const int* ban = bs_ban + 8 + i * S;
      BS_OWN_BAN
      for (int v = tid; v < n; v += 256) {
        const float y = fin ? (v == 0 ? c : -INFINITY) : c + ((x[v] - mx) - ls);
        unsigned long long e = bs_pack(y, i * V + v);
        if (e > lc[W - 1]) {
          BS_OFFERED
          if (offered) {
            int cnt = v == ptok ? pcnt : 0;
            if (pmany) {                                               // (two chosen tokens 256 apart or more: rare)
              cnt = 0;
              for (int j = 0; j < nt; ++j) cnt += s_tok[j] == v;
            }
            if (cnt > 0 && !fin) e = bs_pack(y - q.lam * (float)cnt, i * V + v);
#pragma unroll
            for (int k = 0; k < W; ++k)
              if (e > lc[k]) { const unsigned long long d = lc[k]; lc[k] = e; e = d; }
          }
        }
      }
    }
    for (int k = 0; k < W; ++k) {                                      // (3)
      BS_ARGMAX_ROUND(k)
      const size_t o = (size_t)r * BW + g * W + k;
      if (e != 0ull && lc[0] == e) {           // (candidates are distinct: their indices are) the one thread that owned the winner
        const int j = bs_index(e), i = j / V, v = j - i * V;
        const float c = p.cum[i * p.rows + r];
        const bool fin = p.fin[i * p.rows + r] != 0;
        const float y = fin ? (v == 0 ? c : -INFINITY) : c + ((p.x[((size_t)i * p.rows + r) * V + v] - s_mx[i]) - s_ls[i]);
        p.vals[o] = bs_value(bs_pack(y, j)); p.idx[o] = j;
        if (!fin) { const int at = s_ntok; s_tok[at & 7] = v; s_ntok = at + 1; }
#pragma unroll
        for (int s = 0; s + 1 < W; ++s) lc[s] = lc[s + 1];
        lc[W - 1] = 0ull;
      }
      if (e == 0ull && tid == 0) { p.vals[o] = -INFINITY; p.idx[o] = 0; }     // (fewer than W candidates compared: NaN-free inputs never get here)
    }
    __syncthreads();                                                   // s_tok / s_ntok of this group, and wc, before the next
  }
}
// group[r][b] = order[r][b] / w: the group of the slot that took rank r (n = bw * B entries)
__global__ void beam_group_kernel(const int32_t* __restrict__ order, int w, int n, int32_t* __restrict__ group) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) group[i] = order[i] / w;
}
// final ranking, one thread per caption: len = fin, or n_steps without an <EOS>; score = cum / len^alpha (alpha = 0: cum);
// descending score, lowest beam index among equals.  order[r][b] = the beam that takes rank r.
__global__ __launch_bounds__(256) void beam_nbest_rank_kernel(const float* __restrict__ cum, const int32_t* __restrict__ fin,
                                                              const int32_t* __restrict__ n_steps, int B, int bw, float alpha,
                                                              float* __restrict__ cum_out, int32_t* __restrict__ len_out,
                                                              float* __restrict__ score_out, int32_t* __restrict__ order) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int ns = *n_steps;
  unsigned taken = 0;
  for (int r = 0; r < bw; ++r) {
    float best = 0.f; int bi = -1;
    for (int i = 0; i < bw; ++i) {
      if (taken >> i & 1) continue;
      const int f = fin[i * B + b], len = f ? f : ns;
      const float c = cum[i * B + b];
      const float s = alpha == 0.f ? c : c / (float)pow((double)len, (double)alpha);
      if (bi < 0 || s > best) { best = s; bi = i; }
    }
    taken |= 1u << bi;
    const int f = fin[bi * B + b];
    cum_out[r * B + b] = cum[bi * B + b]; len_out[r * B + b] = f ? f : ns; score_out[r * B + b] = best; order[r * B + b] = bi;
  }
}

// ---- stochastic beam search (Kool, van Hoof, Welling 2019, "Stochastic Beams and Where to Find Them"; the reference has no
// counterpart; DESIGN.md section 21 states the definition, tests/sbs_ref.py restates it): Gumbel-top-k over whole sequences, done
// lazily inside a beam search.  A hypothesis carries phi (its log-probability, the cum of section 11) and G (its perturbed score).  A
// live hypothesis i offers every v at phi_v = phi_i + log_softmax(x_i / temp)[v]; Gt_v = phi_v + g_v with the Gumbel of section 8 on
// the counter ((t * bw * rows + i * rows + r) * V + v) mod 2^32; the maximum Z_i of the Gt_v is conditioned to be G_i:
//   Ghat_v = -log(exp(-G_i) - exp(-Z_i) + exp(-Gt_v))
// and the bw largest Ghat of the caption become the new hypotheses.  A finished hypothesis offers <PAD> at (phi_i, G_i), no noise.
struct SbsSelArgs {
  const float* x;                      // logits [nb][rows][V], read only
  const float* cum; const float* gum;  // [nb][rows]: phi and G of the hypotheses
  const int32_t* fin;                  // [nb][rows], != 0: the hypothesis is finished
  int nb, rows, V, t;
  float temp; uint32_t key;            // key = rn_site_key(seed, RN_SITE_SAMPLE)
  float* vals; float* gum_out; int32_t* idx;   // [rows][BW], Ghat descending; vals = phi, idx = i * V + v
};
// The transform (G_i, Gt_v, Z_i) -> Ghat_v in double, in the form that neither cancels nor overflows: with a = Gt - Z <= 0,
// l = log(1 - exp(a)) by the branch that is accurate on either side of -ln 2, w = G - Gt + l, Ghat = G - softplus(w).  a = 0 (the
// parent's best child): l = w = -inf and Ghat = G exactly.
__device__ __forceinline__ double sbs_condition(double G, double Gt, double Z) {
  const double a = Gt - Z;
  const double l = a > -0.6931471805599453 ? log(-expm1(a)) : log1p(-exp(a));
  const double w = G - Gt + l;
  if (w == -INFINITY) return G;
  return G - fmax(0.0, w) - log1p(exp(-fabs(w)));
}
// beam_select_kernel's launch shape: one workgroup of 256 per caption.  Within one parent Ghat is increasing in Gt, so the overall
// top BW lie among each parent's top BW by Gt: one pass of noise per candidate is enough.  (1) Row statistics of x / temp per live
// hypothesis, logprob_rows_kernel's formulas and summation order (a division by 1.0f is exact: temperature 1 keeps beam_select_kernel's
// bits).  (2) Per live parent: the per-thread best-BW walk of beam_select_kernel on bs_pack(Gt_v, i * V + v), the Gumbel hashed and
// formed here, once per candidate; then BW arg-max rounds put the parent's BW best (Gt, flat index) into an LDS table, in order: the
// first is Z_i.  A finished parent writes its single entry (and, so that -inf fills a caption that has fewer than BW candidates, its
// next BW - 1 tokens at -inf) without a walk.  (3) Wave 0: lane l owns table entry l (nb * BW <= 64), forms its Ghat in double from
// the fp32 inputs — the one pass through the double-precision code of the launch — rounds it to fp32, and BW butterfly rounds
// pick the largest by (value, lowest flat index); the owner recomputes phi from its row with beam_select_kernel's expression and
// writes the three outputs.  No score array, no atomics: two calls give the same bits.
template <int BW> __global__ __launch_bounds__(256) void sbs_select_kernel(const SbsSelArgs p) {
  __shared__ float sf[4]; __shared__ float s_mx[8], s_ls[8], s_z[8]; __shared__ unsigned long long wc[2][4];
  __shared__ float t_gt[64]; __shared__ int t_idx[64];
  const int r = blockIdx.x, tid = threadIdx.x, V = p.V, nb = p.nb;
  const int lane = tid & 63, wave = tid >> 6;
  for (int i = 0; i < nb; ++i) {                                         // (1)
    if (p.fin[i * p.rows + r]) continue;                                 // (uniform over the workgroup)
    const float* x = p.x + ((size_t)i * p.rows + r) * V;
    float mx = -INFINITY, sum = 0.f;
    for (int v = tid; v < V; v += 256) mx = fmaxf(mx, x[v] / p.temp);
    mx = block_max256(mx, sf);
    for (int v = tid; v < V; v += 256) sum += rn_exp(x[v] / p.temp - mx);
    sum = block_sum256(sum, sf);
    if (tid == 0) { s_mx[i] = mx; s_ls[i] = logf(sum); }
  }
  if (tid < 64) { t_gt[tid] = -INFINITY; t_idx[tid] = -1; }              // -1: no entry
  __syncthreads();
  int rd = 0;                                                            // arg-max rounds so far: wc's two buffers alternate across parents
  for (int i = 0; i < nb; ++i) {                                         // (2)
    const float c = p.cum[i * p.rows + r];
    if (p.fin[i * p.rows + r] != 0) {                                    // (uniform over the workgroup)
      if (tid < BW && tid < V) { t_gt[i * BW + tid] = tid == 0 ? p.gum[i * p.rows + r] : -INFINITY; t_idx[i * BW + tid] = i * V + tid; }
      continue;
    }
    const float* x = p.x + ((size_t)i * p.rows + r) * V;
    const float mx = s_mx[i], ls = s_ls[i];
    const uint32_t base = (((uint32_t)p.t * (uint32_t)BW + (uint32_t)i) * (uint32_t)p.rows + (uint32_t)r) * (uint32_t)V;
    unsigned long long lc[BW];
#pragma unroll
    for (int k = 0; k < BW; ++k) lc[k] = 0ull;
    for (int v = tid; v < V; v += 256) {
      const float phi = c + ((x[v] / p.temp - mx) - ls);
      const uint32_t h = rn_fmix32((base + (uint32_t)v) * 0x9E3779B1u + p.key);
      const float u = ((float)(h >> 9) + 0.5f) * 0x1p-23f;               // exact in fp32, inside (0, 1)
      const float gt = phi - logf(-logf(u));
      unsigned long long e = bs_pack(gt, i * V + v);
      if (e > lc[BW - 1]) {
#pragma unroll
        for (int k = 0; k < BW; ++k)
          if (e > lc[k]) { const unsigned long long d = lc[k]; lc[k] = e; e = d; }
      }
    }
    for (int k = 0; k < BW; ++k, ++rd) {
      BS_ARGMAX_ROUND(rd)
      if (e != 0ull && lc[0] == e) {           // (candidates are distinct: their indices are)
#pragma unroll
        for (int q = 0; q + 1 < BW; ++q) lc[q] = lc[q + 1];
        lc[BW - 1] = 0ull;
      }
      if (tid == 0 && e != 0ull) {             // (e == 0: fewer than BW candidates compared, NaN-free inputs never get here)
        t_gt[i * BW + k] = bs_value(e); t_idx[i * BW + k] = bs_index(e);
        if (k == 0) s_z[i] = bs_value(e);
      }
    }
  }
  __syncthreads();
  if (wave != 0) return;                                                 // (3)  (no barrier follows)
  unsigned long long ent = 0ull; float gh = -INFINITY; int flat = -1, pi = 0;
  if (lane < nb * BW) {
    flat = t_idx[lane]; pi = lane / BW;
    if (flat >= 0) {
      const float gt = t_gt[lane];
      gh = p.fin[pi * p.rows + r] != 0 ? gt : (float)sbs_condition((double)p.gum[pi * p.rows + r], (double)gt, (double)s_z[pi]);
      ent = bs_pack(gh, flat);
    }
  }
  for (int k = 0; k < BW; ++k) {
    unsigned long long e = ent;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long d = __shfl_xor(e, o);
      e = d > e ? d : e;
    }
    const size_t o = (size_t)r * BW + k;
    if (e != 0ull && ent == e) {               // (entries are distinct: their flat indices are) the one lane that owns the winner
      const int v = flat - pi * V;
      const float c = p.cum[pi * p.rows + r];
      const bool fin = p.fin[pi * p.rows + r] != 0;
      p.vals[o] = fin ? (v == 0 ? c : -INFINITY) : c + ((p.x[((size_t)pi * p.rows + r) * V + v] / p.temp - s_mx[pi]) - s_ls[pi]);
      p.gum_out[o] = gh; p.idx[o] = flat;
      ent = 0ull;
    }
    if (e == 0ull && lane == 0) { p.vals[o] = -INFINITY; p.gum_out[o] = -INFINITY; p.idx[o] = 0; }
  }
}
// the outputs of the stochastic beam search, one thread per (rank, caption): the slots after the last step are in rank order (G
// descending, the lowest slot among equals), so rank r is slot r; len = fin, or n_steps without an <EOS>; order = the identity
__global__ __launch_bounds__(256) void sbs_finish_kernel(const float* __restrict__ cum, const float* __restrict__ gum,
                                                         const int32_t* __restrict__ fin, const int32_t* __restrict__ n_steps, int B, int bw,
                                                         float* __restrict__ cum_out, int32_t* __restrict__ len_out,
                                                         float* __restrict__ gum_out, int32_t* __restrict__ order) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= bw * B) return;
  const int f = fin[i];
  cum_out[i] = cum[i]; gum_out[i] = gum[i]; len_out[i] = f ? f : *n_steps; order[i] = i / B;
}

// ---- ensemble decoding: the rows of M decoders mixed into one row of logits (the reference has no counterpart; DESIGN.md section 19
// states the definition, tests/ensemble_ref.py restates it).  With l_m = log_softmax(x_m) by logprob_rows_kernel's formulas at
// temperature 1 and weights w_m > 0 that sum to 1 (lw_m = log w_m, both formed by the host in float64):
//   arithmetic  y[v] = a + log sum_m exp(lw_m + l_m[v] - a),  a = max_m (lw_m + l_m[v])     log of the weighted mean of the probabilities
//   geometric   y[v] = sum_m w_m l_m[v]                                                     weighted mean of the log-probabilities
// Both sums over m run upward from m = 0 in the one thread that owns v: no atomics, two calls give the same bits, equal rows too.
#define ENS_MAX_M 8
#define ENS_LDS_FLOATS 24576           // floats of the M rows that are kept in LDS (96 KB of the CU's 160); above: the streaming form
struct EnsMixArgs {
  const float* x[ENS_MAX_M];           // logits [rows][V] of each member, read only (slots >= M unused); y may be x[0], nothing else
  float w[ENS_MAX_M], lw[ENS_MAX_M];
  int M, V, geo;                       // geo != 0: the geometric mode
  float* y;                            // [rows][V]
};
// rows of LDS start 16 bytes apart at least
__host__ __device__ __forceinline__ int ens_row_stride(int V) { return (V + 3) & ~3; }
template <int VEC> __device__ __forceinline__ void ens_load(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) { const float4 q = *reinterpret_cast<const float4*>(p); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
  else v[0] = *p;
}
// One workgroup per row.  RES: (0) the M rows go to LDS, every logit read from global memory once; else every phase reads global
// memory (the second and third pass mostly from the caches).  (1) per member the maximum and log sum exp(x - max), in the strided
// order and by the formulas of logprob_rows_kernel whichever way the row was loaded, so RES and VEC change no bit.  (2) every thread
// forms the y of its own v (VEC = 4: of four neighbours, V % 4 == 0 and 16-byte aligned rows).  In place over member 0: with RES all
// reads of global memory end at the barrier behind (0); without, (1) ends at a barrier and in (2) the thread that writes y[v] is the
// only one that still reads x_m[v], before it writes.
template <bool RES, int VEC> __global__ __launch_bounds__(256) void ensemble_mix_rows_kernel(const EnsMixArgs p) {
  extern __shared__ __attribute__((aligned(16))) float ens_rows[];
  __shared__ float sf[4]; __shared__ float s_mx[ENS_MAX_M], s_ls[ENS_MAX_M];
  const int tid = threadIdx.x, V = p.V, M = p.M, S = ens_row_stride(V);
  const size_t ro = (size_t)blockIdx.x * V;
  if (RES) {                                                           // (0)
    for (int m = 0; m < M; ++m) {
      const float* x = p.x[m] + ro;
      float* r = ens_rows + m * S;
      for (int q = tid; q < V / VEC; q += 256) {
        float t[VEC];
        ens_load<VEC>(x + q * VEC, t);
#pragma unroll
        for (int j = 0; j < VEC; ++j) r[q * VEC + j] = t[j];
      }
    }
    __syncthreads();
  }
  for (int m = 0; m < M; ++m) {                                        // (1)
    const float* x = RES ? ens_rows + m * S : p.x[m] + ro;
    float mx = -INFINITY, sum = 0.f;
    for (int v = tid; v < V; v += 256) mx = fmaxf(mx, x[v]);
    mx = block_max256(mx, sf);
    for (int v = tid; v < V; v += 256) sum += rn_exp(x[v] - mx);
    sum = block_sum256(sum, sf);
    if (tid == 0) { s_mx[m] = mx; s_ls[m] = logf(sum); }
  }
  __syncthreads();
  for (int q = tid; q < V / VEC; q += 256) {                           // (2)
    float a[VEC], s[VEC], xv[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { a[j] = -INFINITY; s[j] = 0.f; }
    if (p.geo) {
      for (int m = 0; m < M; ++m) {
        ens_load<VEC>((RES ? ens_rows + m * S : p.x[m] + ro) + q * VEC, xv);
#pragma unroll
        for (int j = 0; j < VEC; ++j) s[j] += p.w[m] * ((xv[j] - s_mx[m]) - s_ls[m]);
      }
    } else {
      for (int m = 0; m < M; ++m) {
        ens_load<VEC>((RES ? ens_rows + m * S : p.x[m] + ro) + q * VEC, xv);
#pragma unroll
        for (int j = 0; j < VEC; ++j) a[j] = fmaxf(a[j], p.lw[m] + ((xv[j] - s_mx[m]) - s_ls[m]));
      }
      for (int m = 0; m < M; ++m) {
        ens_load<VEC>((RES ? ens_rows + m * S : p.x[m] + ro) + q * VEC, xv);
#pragma unroll
        for (int j = 0; j < VEC; ++j) s[j] += rn_exp((p.lw[m] + ((xv[j] - s_mx[m]) - s_ls[m])) - a[j]);
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) s[j] = a[j] == -INFINITY ? -INFINITY : a[j] + logf(s[j]);    // (-inf in every member stays -inf)
    }
    float* y = p.y + ro + q * VEC;
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(y) = make_float4(s[0], s[1], s[2], s[3]);
    else y[0] = s[0];
  }
}
// The regather of a further member's recurrent state by the decisions member 0's selection left in idx [B][bw] (src = idx / V):
// beam_update_kernel's state copy alone; history, cum, lengths and tokens exist once, on member 0.  c_next null: a GRU has no c.
__global__ __launch_bounds__(128) void beam_regather_state_kernel(const int32_t* __restrict__ idx, int B, int H, int V, int bw,
                                                                  const float* __restrict__ h_next, const float* __restrict__ c_next,
                                                                  float* __restrict__ h_new, float* __restrict__ c_new) {
  const int k = blockIdx.x, b = blockIdx.y;
  const int src = idx[b * bw + k] / V;
  const size_t so = ((size_t)src * B + b) * H, dn = ((size_t)k * B + b) * H;
  for (int j = threadIdx.x; j < H; j += 128) {
    h_new[dn + j] = h_next[so + j];
    if (c_next) c_new[dn + j] = c_next[so + j];
  }
}

// ---- consensus (minimum-Bayes-risk) reranking: n-gram overlap of hypotheses with a reference set
// The words of a caption column are its tokens before the first <EOS> (2), at most T.  With c_n(g) the occurrences of n-gram g,
//   Q_n(c) = sum_g c_n(g)^2 = sum over the positions p of c of c_n(g(p)),
//   M_n(h, r) = sum_g min(h_n(g), r_n(g)) r_n(g) = sum over the positions q of r of min(h_n(g(q)), r_n(g(q))),
// so every count is "how many positions of caption y start the n-gram that starts at position q of caption x": the match run
// run(p, q) = min(4, equal consecutive words from (p, q)) gives all four orders in one walk over y.  Integers only up to here, in
// any order; the finishing is float64, one thread per hypothesis walking the references upward.
struct ConsensusArgs {
  const int64_t* hyp;        // [Nh][Th][B]
  const int64_t* ref;        // [Nr][Tr][B]; null: the hypotheses are their own references (Nr = Nh, Tr = Th)
  const float* w;            // [Nr][B] or null: util = sum_j w_j sim_ij; null: (sum_j sim_ij) / Nr
  double sigma;              // of the Gaussian length penalty, > 0
  int Nh, Nr, Th, Tr, B, HT; // HT: hypotheses per workgroup (grid = B x ceil(Nh / HT))
  double* util;              // [Nh][B]
  double* sim;               // [Nh][Nr][B] or null
  int32_t* counts;           // [Nh][Nr][B][4] (M_n) or null
  int32_t* q_hyp;            // [Nh][B][4] or null
  int32_t* q_ref;            // [Nr][B][4] or null
  int32_t* len_hyp;          // [Nh][B] or null
  int32_t* len_ref;          // [Nr][B] or null
};
constexpr int CS_PAD = 3;    // words a 4-gram window reads behind a caption's last position
// LDS words of one workgroup: tokens of the references and of the tile's hypotheses (rows padded by CS_PAD), the references' own
// counts per position, lengths, packed Q of both, packed M of the tile's pairs
__host__ __device__ inline int cs_lds_words(int Nr, int Tr, int Th, int HT) {
  return Nr * (Tr + CS_PAD) + HT * (Th + CS_PAD) + Nr * Tr + Nr + HT + 2 * Nr + 2 * HT + 2 * HT * Nr;
}
// the smallest power of two >= T (T in [1, 64]): the lanes one caption's positions take in a wave
__host__ __device__ inline int cs_seg(int T) { int W = 1; while (W < T) W <<= 1; return W; }
// For the n-gram windows (r0), (r0 r1), .. (r0 .. r3): how many positions p < Ly of y start them, in four byte fields (each <= 64).
// y holds -1 from its length on, CS_PAD entries behind its row included; the caller passes -2 for a word behind x's length: the
// two never match, and no real word (>= 0) matches either.
__device__ inline uint32_t cs_count4(const int* y, int Ly, int r0, int r1, int r2, int r3) {
  uint32_t c = 0;
  int a0 = y[0], a1 = y[1], a2 = y[2];
  for (int p = 0; p < Ly; ++p) {
    const int a3 = y[p + 3];
    const bool e1 = a0 == r0, e2 = e1 && a1 == r1, e3 = e2 && a2 == r2, e4 = e3 && a3 == r3;
    c += (uint32_t)e1 + ((uint32_t)e2 << 8) + ((uint32_t)e3 << 16) + ((uint32_t)e4 << 24);
    a0 = a1; a1 = a2; a2 = a3;
  }
  return c;
}
// the four words from position q of x (length L), -2 behind the length
#define CS_WINDOW(x, q, L)                                                                                        \
  const int r0 = (q) < (L) ? (x)[(q)] : -2, r1 = (q) + 1 < (L) ? (x)[(q) + 1] : -2, r2 = (q) + 2 < (L) ? (x)[(q) + 2] : -2, \
            r3 = (q) + 3 < (L) ? (x)[(q) + 3] : -2;
// four byte fields -> fields of 16 bits in two words (sums over <= 64 positions of values <= 64 stay below 2^16)
#define CS_WIDEN(c, lo, hi) lo = ((c) & 0xffu) | (((c) >> 8 & 0xffu) << 16); hi = ((c) >> 16 & 0xffu) | (((c) >> 24) << 16);
// sum over the W lanes of a segment (W a power of two, the segment aligned to it)
#define CS_SEG_SUM(lo, hi, W)                                                                                     \
  for (int off = (W) >> 1; off > 0; off >>= 1) { lo += __shfl_xor(lo, off); hi += __shfl_xor(hi, off); }
// Own counts of ncap captions tok [ncap][S] (lengths len): own [ncap][T] (may be null) gets the byte fields of every position, q2
// [ncap][2] the packed Q_1..Q_4.  A wave takes 64 / W captions at a time, one lane per position.
__device__ inline void cs_own_counts(const int* tok, int S, int T, const int* len, int ncap, uint32_t* own, uint32_t* q2, int tid) {
  const int W = cs_seg(T), per = 64 / W, lane = tid & 63, sub = lane / W, q = lane % W;
  for (int base = (tid >> 6) * per; base < ncap; base += 4 * per) {     // (uniform in the wave: every lane takes part in the sums)
    const int c = base + sub;
    uint32_t cnt = 0, lo, hi;
    if (c < ncap && q < T) {
      const int* x = tok + c * S;
      const int L = len[c];
      CS_WINDOW(x, q, L)
      cnt = cs_count4(x, L, r0, r1, r2, r3);
      if (own) own[c * T + q] = cnt;
    }
    CS_WIDEN(cnt, lo, hi)
    CS_SEG_SUM(lo, hi, W)
    if (c < ncap && q == 0) { q2[2 * c] = lo; q2[2 * c + 1] = hi; }
  }
}
__device__ inline uint32_t cs_min_bytes(uint32_t a, uint32_t b) {
  uint32_t m = 0;
#pragma unroll
  for (int s = 0; s < 32; s += 8) { const uint32_t x = a >> s & 0xffu, y = b >> s & 0xffu; m |= (x < y ? x : y) << s; }
  return m;
}
// One workgroup per (caption column b, tile of HT hypotheses).  (0) tokens of all references and of the tile into LDS as int32
// (exact for ids below 2^31), lengths, -1 from the length on.  (1) own counts and Q.  (2) per pair (hypothesis of the tile,
// reference) and reference position q: min(count in the hypothesis, own count), summed over q inside the wave -> M.  (3) one
// thread per hypothesis: sim and util in float64 over j ascending.
__global__ __launch_bounds__(256) void consensus_rows_kernel(const ConsensusArgs a) {
  extern __shared__ __attribute__((aligned(16))) int cs_lds[];
  const int tid = threadIdx.x, b = blockIdx.x, B = a.B, Nr = a.Nr, Tr = a.Tr, Th = a.Th, HT = a.HT;
  const int i0 = blockIdx.y * HT, nh = a.Nh - i0 < HT ? a.Nh - i0 : HT;
  const int Sr = Tr + CS_PAD, Sh = Th + CS_PAD;
  int* rt = cs_lds;                                   // [Nr][Sr]
  int* ht = rt + Nr * Sr;                             // [HT][Sh]
  uint32_t* own = (uint32_t*)(ht + HT * Sh);          // [Nr][Tr]
  int* rl = (int*)(own + Nr * Tr);                    // [Nr]
  int* hl = rl + Nr;                                  // [HT]
  uint32_t* rq = (uint32_t*)(hl + HT);                // [Nr][2]
  uint32_t* hq = rq + 2 * Nr;                         // [HT][2]
  uint32_t* M = hq + 2 * HT;                          // [HT][Nr][2]
  const int64_t* rsrc = a.ref ? a.ref : a.hyp;
  // (0)
  for (int e = tid; e < Nr * Sr; e += 256) {
    const int c = e / Sr, t = e - c * Sr;
    rt[e] = t < Tr ? (int)rsrc[((size_t)c * Tr + t) * B + b] : -1;
  }
  for (int e = tid; e < nh * Sh; e += 256) {
    const int c = e / Sh, t = e - c * Sh;
    ht[e] = t < Th ? (int)a.hyp[((size_t)(i0 + c) * Th + t) * B + b] : -1;
  }
  __syncthreads();
  for (int c = tid; c < Nr + nh; c += 256) {
    const bool r = c < Nr;
    const int* x = r ? rt + c * Sr : ht + (c - Nr) * Sh;
    const int T = r ? Tr : Th;
    int L = 0;
    while (L < T && x[L] != 2) ++L;
    if (r) rl[c] = L; else hl[c - Nr] = L;
  }
  __syncthreads();
  for (int e = tid; e < Nr * Sr; e += 256) {
    const int c = e / Sr, t = e - c * Sr;
    if (t >= rl[c]) rt[e] = -1;
  }
  for (int e = tid; e < nh * Sh; e += 256) {
    const int c = e / Sh, t = e - c * Sh;
    if (t >= hl[c]) ht[e] = -1;
  }
  __syncthreads();
  // (1)
  cs_own_counts(rt, Sr, Tr, rl, Nr, own, rq, tid);
  cs_own_counts(ht, Sh, Th, hl, nh, nullptr, hq, tid);
  __syncthreads();
  // (2)
  {
    const int W = cs_seg(Tr), per = 64 / W, lane = tid & 63, sub = lane / W, q = lane % W, npairs = nh * Nr;
    for (int base = (tid >> 6) * per; base < npairs; base += 4 * per) {
      const int pr = base + sub;
      uint32_t m = 0, lo, hi;
      if (pr < npairs && q < Tr) {
        const int i = pr / Nr, j = pr - i * Nr;
        const int* x = rt + j * Sr;
        const int L = rl[j];
        CS_WINDOW(x, q, L)
        m = cs_min_bytes(cs_count4(ht + i * Sh, hl[i], r0, r1, r2, r3), own[j * Tr + q]);
      }
      CS_WIDEN(m, lo, hi)
      CS_SEG_SUM(lo, hi, W)
      if (pr < npairs && q == 0) { M[2 * pr] = lo; M[2 * pr + 1] = hi; }
    }
  }
  __syncthreads();
  // the integer outputs (the references' by the first tile alone)
  if (a.counts)
    for (int e = tid; e < nh * Nr * 4; e += 256) {
      const int pr = e >> 2, n = e & 3, i = pr / Nr, j = pr - i * Nr;
      a.counts[(((size_t)(i0 + i) * Nr + j) * B + b) * 4 + n] = (int32_t)(M[2 * pr + (n >> 1)] >> ((n & 1) * 16) & 0xffffu);
    }
  if (a.q_hyp)
    for (int e = tid; e < nh * 4; e += 256) {
      const int i = e >> 2, n = e & 3;
      a.q_hyp[((size_t)(i0 + i) * B + b) * 4 + n] = (int32_t)(hq[2 * i + (n >> 1)] >> ((n & 1) * 16) & 0xffffu);
    }
  if (a.len_hyp)
    for (int i = tid; i < nh; i += 256) a.len_hyp[(size_t)(i0 + i) * B + b] = hl[i];
  if (blockIdx.y == 0) {
    if (a.q_ref)
      for (int e = tid; e < Nr * 4; e += 256) {
        const int j = e >> 2, n = e & 3;
        a.q_ref[((size_t)j * B + b) * 4 + n] = (int32_t)(rq[2 * j + (n >> 1)] >> ((n & 1) * 16) & 0xffffu);
      }
    if (a.len_ref)
      for (int j = tid; j < Nr; j += 256) a.len_ref[(size_t)j * B + b] = rl[j];
  }
  // (3)
  if (tid < nh) {
    const int i = tid;
    const uint32_t qh0 = hq[2 * i], qh1 = hq[2 * i + 1];
    const int Lh = hl[i];
    double u = 0.0;
    for (int j = 0; j < Nr; ++j) {
      const uint32_t m0 = M[2 * (i * Nr + j)], m1 = M[2 * (i * Nr + j) + 1], qr0 = rq[2 * j], qr1 = rq[2 * j + 1];
      double s = 0.0;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const uint32_t sh = (n & 1) * 16;
        const uint32_t m = (n < 2 ? m0 : m1) >> sh & 0xffffu, qh = (n < 2 ? qh0 : qh1) >> sh & 0xffffu, qr = (n < 2 ? qr0 : qr1) >> sh & 0xffffu;
        if (qh > 0 && qr > 0) s += (double)m / sqrt((double)(qh * qr));
      }
      const double d = (double)(Lh - rl[j]);
      s = 0.25 * s * exp(-(d * d) / (2.0 * a.sigma * a.sigma));
      if (a.sim) a.sim[((size_t)(i0 + i) * Nr + j) * B + b] = s;
      u += a.w ? (double)a.w[(size_t)j * B + b] * s : s;
    }
    a.util[(size_t)(i0 + i) * B + b] = a.w ? u : u / (double)Nr;
  }
}
