"""TEST INFRASTRUCTURE ONLY — numpy restatement of the nucleus (top-p) cut of the sampler (csrc/kernels_search.hpp:
sample_rows_kernel<RES, true>) on top of tests/sample_ref.py, whose order, Gumbel noise and draw it uses.

For one row of logits x[0..V), temperature T, top_k and top_p:
  s_v    = x_v / T                                     float32
  K      = the top_k set of sample_ref.allowed_mask, in its order (value descending, index ascending, -0 = +0)
  m      = max over K of s_v
  e_v    = exp(s_v - m)                                float32 subtraction and exponential
  q_v    = floor(e_v * 2^32)                           uint64, exact
  Q      = sum over K of q_v                           integer, >= 2^32
  target = max(1, ceil(float64(float32(top_p)) * float64(Q)))
  n      = the length of the shortest prefix of K whose integer mass reaches target         (top_p == 1: n = |K|, no cut)
Entries equal to the cut value carry one q, so the prefix rule admits ceil((target - mass above) / q) of them, lowest
indices first.  Token and log-probability are sample_ref's draw over the first n entries of the order.

The device differs from this only in its exponential.  Both sides feed the same float32 d = s - m to it; per entry they
differ by at most one ulp of each exponential and |d| * 2^-24 from the device's d * log2(e) product, so a cumulative mass
and the target together move by at most
  b = 2 * (2^-22 + 2^-24 * sum_v q_v |d_v| / Q)
relative to Q.  Every size comes with the band [n_lo, n_hi] of the sizes at target -/+ EPS * Q, EPS = 2^-18, and with b;
the tests assert b <= EPS / 2 on every input they use.  EPS bounds the exponential's rounding; the integer select itself
is exact."""
import numpy as np
import torch

from tests import sample_ref as SR

EPS = 2.0 ** -18


def order(logits):
    """int [rows, V]: every row's indices by value descending, then index ascending (the order of sample_ref.allowed_mask)."""
    return np.argsort(-np.ascontiguousarray(logits, dtype=np.float32), axis=1, kind="stable")


def masses(x_sorted, temperature):
    """The integer masses q (uint64) and the float32 differences d = s - m of logits given in the order."""
    s = (np.asarray(x_sorted, dtype=np.float32) / np.float32(temperature)).astype(np.float32)
    d = (s - s.max()).astype(np.float32)
    e = np.exp(d)
    assert e.dtype == np.float32
    return np.floor(e.astype(np.float64) * 2.0 ** 32).astype(np.uint64), d


def _prefix(cum, target):
    return int(np.searchsorted(cum, np.uint64(target), side="left")) + 1


def nucleus_sizes(logits, temperature, top_k, top_p):
    """logits float32 [rows, V].  Returns n, n_lo, n_hi (int64 [rows]) and b (float64 [rows])."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    rows, V = logits.shape
    k = V if top_k == 0 else top_k
    n, n_lo, n_hi = (np.full(rows, k, dtype=np.int64) for _ in range(3))
    b = np.zeros(rows)
    if top_p == 1.0:
        return n, n_lo, n_hi, b
    od = order(logits)
    for r in range(rows):
        q, d = masses(logits[r, od[r, :k]], temperature)
        cum = np.cumsum(q, dtype=np.uint64)
        Q = int(cum[-1])
        assert 2 ** 32 <= Q < 2 ** 53
        target = max(1, int(np.ceil(np.float64(np.float32(top_p)) * np.float64(Q))))
        slack = int(np.ceil(EPS * Q))
        n[r] = _prefix(cum, target)
        n_lo[r] = _prefix(cum, max(1, target - slack))
        n_hi[r] = _prefix(cum, min(Q, target + slack))
        b[r] = 2.0 * (2.0 ** -22 + 2.0 ** -24 * float((q.astype(np.float64) * np.abs(d.astype(np.float64))).sum()) / Q)
    return n, n_lo, n_hi, b


def prefix_mask(logits, sizes):
    """bool [rows, V]: the first sizes[r] entries of row r in the order."""
    rows, V = logits.shape
    rank = np.empty((rows, V), dtype=np.int64)
    np.put_along_axis(rank, order(logits), np.broadcast_to(np.arange(V), (rows, V)), axis=1)
    return rank < np.asarray(sizes).reshape(rows, 1)


def draw(logits, sizes, temperature, seed, t):
    """sample_ref's draw over the first sizes[r] entries of the order: the other entries are handed to it as -inf, which it never
    draws and which add nothing to its log-sum-exp.  Returns tokens, logprobs float64, margins."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    masked = np.where(prefix_mask(logits, sizes), logits, np.float32(-np.inf)).astype(np.float32)
    return SR.sample_rows(masked, temperature, 0, seed, t)


def sample_rows(logits, temperature, top_k, top_p, seed, t):
    """Returns tokens int64 [rows], logprobs float64 [rows], margins float64 [rows], then n, n_lo, n_hi, b of nucleus_sizes."""
    n, n_lo, n_hi, b = nucleus_sizes(logits, temperature, top_k, top_p)
    return draw(logits, n, temperature, seed, t) + (n, n_lo, n_hi, b)


def sample_search(P, enc, temperature, top_k, top_p, seed, caption_max_len=30, cell="LSTM"):
    """sample_ref.sample_search with the nucleus draw.  Returns a dict of [n_steps][B] arrays tokens, logprobs, margins, n, n_lo,
    n_hi, b and of amax [n_steps] (max |logit| of the step)."""
    O = SR.O
    B = enc.shape[0]
    H = P["rnn.weight_hh_l0"].shape[1]
    tok = torch.full((1, B), O.SOS, dtype=torch.long)
    hid = O.zero_hidden(B, H, cell)
    keys = ("tokens", "logprobs", "margins", "n", "n_lo", "n_hi", "b")
    out = {k: [] for k in keys + ("amax",)}
    with torch.no_grad():
        for t in range(caption_max_len + 1):
            logits, hid = O.decoder_step(P, tok, hid, enc, cell=cell, t=t)
            lg = logits.numpy()
            res = sample_rows(lg, temperature, top_k, top_p, seed, t)
            for k, v in zip(keys, res):
                out[k].append(v)
            out["amax"].append(float(np.abs(lg).max()))
            tok = torch.from_numpy(res[0]).view(1, -1)
            if t == caption_max_len or bool((tok == 0).all()):
                break
    return {k: np.stack(v) if k != "amax" else np.array(v) for k, v in out.items()}


def comparable(run):
    """bool [n][B] for a search: False from a caption's first near-tie decision or first step whose band holds more than one
    size onward."""
    bad = (run["margins"] < SR.NEAR_TIE) | (run["n_lo"] != run["n_hi"])
    return ~(np.cumsum(bad, axis=0) > 0)


# ---------------------------------------------------------------------------------- cases shared by the CPU and GPU tests
# (golden case, seed, temperature, top_k, top_p) of the search tests.  Seeds from 1..8 for which the restatement excludes no
# caption and every band is a single size (tests/test_nucleus_ref.py holds that without a GPU).
SEARCH_RUNS = [("search_small", 2, 1.0, 0, 0.9), ("search_small_b", 1, 1.0, 0, 0.9), ("search_eos", 1, 1.0, 0, 0.9),
               ("search_stop", 1, 1.0, 0, 0.9), ("search_gru", 7, 1.0, 0, 0.9), ("search_gru_b", 1, 1.0, 0, 0.9),
               ("search_gru_stop", 1, 1.0, 0, 0.9), ("search_small", 1, 0.5, 5, 0.8), ("search_gru", 1, 0.5, 5, 0.8),
               ("search_small_b", 1, 1.0, 0, 0.5), ("search_gru_b", 1, 1.0, 0, 0.5),
               # shape_rows160: the shape case rows160 of tests/search_shapes.py (B = 20, H = 320: three slabs)
               ("rows160", 2, 1.0, 20, 0.9)]

ROW_TOP_P = (0.05, 0.5, 0.9, 0.999)


def row_cases(V):
    """(rows, quantised, top_k, temperature, top_p, t, seed) for every combination the kernel-alone tests run at vocabulary V, on
    sample_ref.row_logits."""
    out = []
    for rows in (1, 7):
        for quantised in (False, True):
            for top_k in sorted({k for k in (0, 8, V - 1) if 0 <= k <= V}):
                for temperature in (1.0, 0.5, 2.0):
                    for top_p in ROW_TOP_P:
                        for t in SR.ROW_T:
                            out.append((rows, quantised, top_k, temperature, top_p, t, 1 + (top_k + rows + len(out)) % 8))
    return out
