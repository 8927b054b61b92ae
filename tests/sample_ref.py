"""TEST INFRASTRUCTURE ONLY — numpy restatement of the sampling draw (csrc/kernels_search.hpp: sample_rows_kernel;
DESIGN.md "Sampling search") and of the sampling search loop on top of the CPU oracle's decoder step.

For caption row b of B, step t, vocabulary index v of V:
  idx   = ((t * B + b) * V + v) mod 2^32
  hash  = fmix32(idx * 0x9E3779B1 + site_key(seed, SITE_SAMPLE))          (oracle/dropmask.py)
  u     = ((hash >> 9) + 0.5) * 2^-23           float32: exact, strictly inside (0, 1)
  g     = -log(-log(u))                          float32
  s_v   = logit_v / temperature                  float32
  allowed = everything (top_k 0 or V), else the top_k largest logits, value descending then index ascending
  token   = argmax over allowed v of (s_v + g_v), lowest index among equals
  logprob = s_token - logsumexp over allowed v of s_v
Besides token and log-probability every draw reports its margin: best minus second-best s + g among the allowed entries
(inf when only one is allowed).  A decision whose margin is below NEAR_TIE is left out of token comparisons against the
device (fp32 logit / logf rounding may flip it); that is a condition for exclusion, not a tolerance on results."""
import numpy as np
import torch

from oracle import recnet_oracle as O
from oracle.dropmask import _fmix32, site_key

SITE_SAMPLE = 3
NEAR_TIE = 1e-3
EOS = 2


def gumbel(seed, t, B, V, rows=None):
    """float32 [rows, V] Gumbel noise of step t (rows: the caption indices b, default all B)."""
    b = np.arange(B, dtype=np.uint64) if rows is None else np.asarray(rows, dtype=np.uint64)
    with np.errstate(over="ignore"):
        idx = ((np.uint64(t) * np.uint64(B) + b[:, None]) * np.uint64(V) + np.arange(V, dtype=np.uint64)[None, :]) & np.uint64(0xFFFFFFFF)
        h = _fmix32((idx.astype(np.uint32) * np.uint32(0x9E3779B1) + site_key(seed, SITE_SAMPLE)).astype(np.uint32))
    u = ((h >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    return -np.log(-np.log(u))


def allowed_mask(logits, top_k):
    """bool [rows, V]: the top_k largest entries of each row, value descending then index ascending (0 or V: all)."""
    rows, V = logits.shape
    if top_k == 0 or top_k == V:
        return np.ones((rows, V), dtype=bool)
    order = np.argsort(-logits, axis=1, kind="stable")          # equal values keep index order
    m = np.zeros((rows, V), dtype=bool)
    np.put_along_axis(m, order[:, :top_k], True, axis=1)
    return m


def sample_rows(logits, temperature, top_k, seed, t):
    """logits float32 [rows, V] (B = rows).  Returns tokens int64 [rows], logprobs float64 [rows], margins float64 [rows]."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    rows, V = logits.shape
    ok = allowed_mask(logits, top_k)
    s = logits / np.float32(temperature)
    y = np.where(ok, s + gumbel(seed, t, rows, V), -np.inf).astype(np.float32)
    tok = y.argmax(axis=1)                                       # first (= lowest) index among equal maxima
    if V > 1:
        top2 = np.partition(y, V - 2, axis=1)[:, V - 2:].astype(np.float64)
        with np.errstate(invalid="ignore"):
            margin = top2[:, 1] - top2[:, 0]
        margin[np.isneginf(top2[:, 0])] = np.inf                 # a single allowed entry
    else:
        margin = np.full(rows, np.inf)
    s64 = np.where(ok, s.astype(np.float64), -np.inf)
    mx = s64.max(axis=1)
    lse = mx + np.log(np.exp(s64 - mx[:, None]).sum(axis=1))
    lp = s64[np.arange(rows), tok] - lse
    return tok.astype(np.int64), lp, margin


def sample_search(P, enc, temperature, top_k, seed, caption_max_len=30, cell="LSTM"):
    """The loop of oracle.search_oracle.greedy_search with the draw in place of the arg-max.  Returns tokens [n][B] int64,
    logprobs [n][B] float64, margins [n][B] float64, logit_abs_max [n] (max |logit| of the step, for the error bars)."""
    B = enc.shape[0]
    H = P["rnn.weight_hh_l0"].shape[1]
    tok = torch.full((1, B), O.SOS, dtype=torch.long)
    hid = O.zero_hidden(B, H, cell)
    toks, lps, margins, amax = [], [], [], []
    with torch.no_grad():
        for t in range(caption_max_len + 1):
            logits, hid = O.decoder_step(P, tok, hid, enc, cell=cell, t=t)
            lg = logits.numpy()
            tk, lp, mg = sample_rows(lg, temperature, top_k, seed, t)
            tok = torch.from_numpy(tk).view(1, -1)
            toks.append(tk); lps.append(lp); margins.append(mg); amax.append(float(np.abs(lg).max()))
            if t == caption_max_len or bool((tok == 0).all()):
                break
    return np.stack(toks), np.stack(lps), np.stack(margins), np.array(amax)


def comparable(margins):
    """bool [n][B] for a search: False from a caption's first near-tie decision onward (everything downstream of a decision
    that fp32 rounding may flip depends on it)."""
    near = margins < NEAR_TIE
    return ~(np.cumsum(near, axis=0) > 0)


# ---------------------------------------------------------------------------------- cases shared by the CPU and GPU tests
# (golden case, seed, temperature, top_k) of the search tests: every golden at temperature 1 without a cut, one LSTM and one GRU
# case also sharpened and cut to five.  Seeds from 1..8 for which the restatement excludes no caption
# (tests/test_sample_ref.py holds the cap of one caption per run without a GPU).
SEARCH_RUNS = [("search_small", 4, 1.0, 0), ("search_small_b", 3, 1.0, 0), ("search_eos", 4, 1.0, 0), ("search_stop", 2, 1.0, 0),
               ("search_gru", 7, 1.0, 0), ("search_gru_b", 2, 1.0, 0), ("search_gru_stop", 2, 1.0, 0),
               ("search_small", 5, 0.5, 5), ("search_gru", 6, 0.5, 5),
               # shape_rows160: the shape case rows160 of tests/search_shapes.py (B = 20, H = 320: three slabs), top_k = 20
               ("rows160", 2, 1.0, 20)]

# Kernel-alone cases: one element, the goldens' vocabulary (61), the block size and its neighbours, the benchmark vocabulary,
# and a row longer than the 12288 floats the kernel keeps in LDS.
ROW_VS = (1, 61, 255, 256, 257, 4188, 12500)
ROW_T = (3, 200000)           # the second one wraps (t * B + b) * V + v past 2^32 at the large vocabularies with 7 rows


def row_logits(V, rows, quantised):
    """Fixed host logits; the quantised set holds multiples of 1/4 only (-0.0 among them), so that many equal values
    straddle every top-k cut."""
    rng = np.random.RandomState(1000 * V + 10 * rows + int(quantised))
    x = (rng.randn(rows, V) * 2.0).astype(np.float32)
    return (np.round(x * 4) / 4).astype(np.float32) if quantised else x


def row_cases(V):
    """(rows, quantised, top_k, temperature, t, seed) for every combination the kernel-alone tests run at vocabulary V."""
    out = []
    for rows in (1, 7):
        for quantised in (False, True):
            for top_k in sorted({k for k in (0, 1, 2, 8, V - 1, V) if 0 <= k <= V}):
                for temperature in (1.0, 0.5, 2.0):
                    for t in ROW_T:
                        out.append((rows, quantised, top_k, temperature, t, 1 + (top_k + rows + len(out)) % 8))
    return out
