"""TEST INFRASTRUCTURE ONLY — float64 restatement of the N-best beam search on log-probabilities (DESIGN.md section 11;
csrc/kernels_search.hpp: beam_select_kernel, csrc/abi_search.inc: recnet_beam_search_nbest) on the CPU oracle's decoder step.

Start: <SOS>, zero state, one hypothesis per caption with cum = 0.  At step t a caption has nb hypotheses (1 at t = 0, else bw):
  a live hypothesis i offers      cum_i + log_softmax(logits_i)[v]   for every v   (the maximum subtracted before the exponentials)
  a finished one (it holds <EOS>) offers  cum_i  at v = <PAD> = 0 and -inf at every other v
  the bw largest of the nb * V candidates become the new hypotheses, in descending order, the lowest flat index i * V + v first
  among equal candidates (bw <= V, so -inf is never selected in a search)
Only <EOS> = 2 finishes a hypothesis; len = position of its <EOS> + 1, or the number of steps run when it has none.  The loop ends
after the first step at which every hypothesis of every caption is finished, or after caption_max_len + 1 steps.  Final rank per
caption: cum / len^length_alpha descending, the lowest beam index among equals.

Every decision reports its margin: the smallest non-zero gap between neighbours among the top bw + 1 candidates (among the bw final
scores for the ranking).  Zero gaps are exact ties, which the index rule resolves the same way everywhere; a gap below
sample_ref.NEAR_TIE may be flipped by fp32 rounding on the device, so a caption is compared up to its first such decision only —
a condition for exclusion, not a tolerance on results.

Shares of compared (step, caption) decisions of the runs below, as this restatement measures them (tests/test_beam_ref.py asserts
the caps: 3/4, and 1/2 for the LSTM run at width 8): see RUN_SHARES at the end of the file.

What the device test compares (tests/test_gpu_beam.py).  The device returns final hypotheses only, so a caption's returned tokens,
len, cum and rank order are compared in full only where NONE of its decisions, the final ranking included, is a near-tie
(comparable_captions; RUN_CAPTIONS lists how many captions of each run that is — fewer than the share of decisions suggests, 0 of 4
on search_stop at width 3).  A caption with a near-tie at step t0 is still compared up to it: the beams after step t0 - 1 are the
restatement's and every later hypothesis descends from one of them, so the first t0 tokens of each returned hypothesis must be one
of the restatement's beam histories at that step (trace).  Together the two checks cover exactly the decisions RUN_SHARES counts."""
import numpy as np
import torch

from oracle import recnet_oracle as O
from tests.sample_ref import NEAR_TIE

EOS, PAD = 2, 0


def log_softmax64(x):
    x = np.asarray(x).astype(np.float64)
    mx = x.max(axis=-1, keepdims=True)
    return (x - mx) - np.log(np.exp(x - mx).sum(axis=-1, keepdims=True))


def _margin(sorted_vals):
    """Smallest non-zero gap between neighbours of descending values [rows, k] (inf when there is none)."""
    if sorted_vals.shape[1] < 2:
        return np.full(sorted_vals.shape[0], np.inf)
    with np.errstate(invalid="ignore"):
        gaps = sorted_vals[:, :-1] - sorted_vals[:, 1:]
    gaps = np.where(np.isnan(gaps) | (gaps == 0), np.inf, gaps)          # (-inf) - (-inf): an exact tie as well
    return gaps.min(axis=1)


def select_rows(logits, cum, finished, bw):
    """One selection step.  logits float32 [nb, rows, V], cum [nb, rows], finished [nb, rows] (non-zero: finished).  Returns
    (vals float64 [rows, bw], idx int64 [rows, bw] = i * V + v, margin float64 [rows])."""
    logits = np.asarray(logits, dtype=np.float32)
    nb, rows, V = logits.shape
    cum = np.asarray(cum).astype(np.float64)
    fin = np.asarray(finished) != 0
    cand = cum[:, :, None] + log_softmax64(logits)
    pad_only = np.full((nb, rows, V), -np.inf)
    pad_only[:, :, PAD] = cum
    cand = np.where(fin[:, :, None], pad_only, cand)
    cand = np.transpose(cand, (1, 0, 2)).reshape(rows, nb * V)
    order = np.argsort(-cand, axis=1, kind="stable")                     # equal values keep index order
    k = min(bw + 1, nb * V)
    top = np.take_along_axis(cand, order[:, :k], axis=1)
    return top[:, :bw], order[:, :bw].astype(np.int64), _margin(top)


def beam_search_nbest(P, enc, bw, length_alpha=0.0, caption_max_len=30, cell="LSTM"):
    """Returns a dict: tokens int64 [bw][n_steps][B] rank-major (canonical: <PAD> behind <EOS>), cum float64 [bw][B], len int64
    [bw][B], score float64 [bw][B], n_steps, margins float64 [n_steps][B] of the selection decisions, final_margin [B] of the
    ranking, amax [n_steps] (max |logit| of the step over all hypotheses, for the error bars), and trace: per step the
    (tokens [bw][B], finished-length [bw][B], cum [bw][B], history [bw][B][t + 1]) after the step, in beam order."""
    B = enc.shape[0]
    H = P["rnn.weight_hh_l0"].shape[1]
    Tm = caption_max_len + 1
    toks = [torch.full((1, B), O.SOS, dtype=torch.long)]
    hids = [O.zero_hidden(B, H, cell)]
    cum = np.zeros((1, B))
    fin = np.zeros((1, B), dtype=np.int64)
    hist = np.zeros((1, B, Tm), dtype=np.int64)
    margins, amax, trace = [], [], []
    n_steps = Tm
    ar = np.arange(B)
    with torch.no_grad():
        for t in range(Tm):
            nb = len(toks)
            steps = [O.decoder_step(P, toks[i], hids[i], enc, cell=cell, t=t) for i in range(nb)]
            lg = np.stack([s[0].numpy() for s in steps])                 # [nb, B, V]
            V = lg.shape[2]
            vals, idx, mg = select_rows(lg, cum, fin, bw)
            src, tok = idx // V, idx % V                                 # [B, bw]
            new_hids = []
            for k in range(bw):
                if cell == "GRU":
                    new_hids.append(torch.stack([steps[src[b, k]][1][:, b] for b in range(B)], dim=1))
                else:
                    new_hids.append(tuple(torch.stack([steps[src[b, k]][1][j][:, b] for b in range(B)], dim=1) for j in range(2)))
            new_hist = np.stack([hist[src[:, k], ar] for k in range(bw)])
            new_hist[:, :, t] = tok.T
            old_fin = np.stack([fin[src[:, k], ar] for k in range(bw)])
            fin = np.where(old_fin > 0, old_fin, np.where(tok.T == EOS, t + 1, 0))
            cum, hist, hids = vals.T.copy(), new_hist, new_hids
            toks = [torch.from_numpy(tok[:, k].copy()).view(1, -1) for k in range(bw)]
            margins.append(mg); amax.append(float(np.abs(lg).max())); trace.append((tok.T.copy(), fin.copy(), cum.copy(), hist[:, :, :t + 1].copy()))
            if (fin > 0).all():
                n_steps = t + 1
                break
    ln = np.where(fin > 0, fin, n_steps)
    score = cum / ln.astype(np.float64) ** float(length_alpha)
    order = np.argsort(-score, axis=0, kind="stable")                    # [bw, B]: the lowest beam index among equals
    g = lambda a: np.take_along_axis(a, order, axis=0)
    tokens = np.stack([hist[order[r], ar] for r in range(bw)])           # [bw, B, Tm]
    tokens = np.transpose(tokens, (0, 2, 1))[:, :n_steps]
    return dict(tokens=tokens, cum=g(cum), len=g(ln), score=g(score), n_steps=n_steps, margins=np.stack(margins),
                final_margin=_margin(g(score).T), amax=np.array(amax), trace=trace)


def comparable_steps(margins):
    """bool [n][B]: True for the decisions of a caption before its first near-tie one."""
    near = margins < NEAR_TIE
    return ~(np.cumsum(near, axis=0) > 0)


def comparable_captions(res):
    """bool [B]: no selection decision and not the final ranking of the caption is a near-tie: its returned hypotheses compare."""
    return comparable_steps(res["margins"]).all(axis=0) & (res["final_margin"] >= NEAR_TIE)


def compared_share(res):
    return float(comparable_steps(res["margins"]).mean())


# ---------------------------------------------------------------------------------- cases shared by the CPU and GPU tests
LENGTH_ALPHA = 0.7
# (golden case, beam width, caption_max_len, cap on the share of compared decisions)
SEARCH_RUNS = [("search_small_b", 3, 7, 0.75), ("search_small_b", 5, 7, 0.75), ("search_eos", 3, 7, 0.75), ("search_stop", 3, 7, 0.75),
               ("search_gru", 3, 7, 0.75), ("search_gru", 5, 7, 0.75), ("search_gru", 8, 7, 0.75),
               ("search_gru_b", 3, 7, 0.75), ("search_gru_b", 5, 7, 0.75), ("search_gru_b", 8, 7, 0.75),
               ("search_gru_stop", 3, 7, 0.75), ("search_gru_stop", 5, 7, 0.75), ("search_gru_stop", 8, 7, 0.75),
               ("search_gru_b", 5, 30, 0.75), ("search_gru", 3, 30, 0.75),
               ("search_eos", 8, 7, 0.5)]

# Kernel-alone cases
ROW_VS = (8, 61, 255, 256, 257, 4188, 12500)
ROW_NB = (1, 3, 8)
ROW_BW = (1, 3, 8)
ROW_KINDS = ("continuous", "quantised", "twins", "finished", "all_finished")


def row_case(V, nb, kind, rows=5):
    """Fixed host inputs (logits float32 [nb, rows, V], cum float32 [nb, rows], finished int32 [nb, rows]).  quantised: multiples of
    1/4, equal values inside a row.  twins: the last hypothesis repeats hypothesis 0 (rows and cum): a tie across beams that the
    lower beam wins; exact on the device too, where equal inputs give equal candidates.  finished: every other hypothesis of every
    other row is finished; all_finished: all of them."""
    rng = np.random.RandomState(9000 + 100 * V + 10 * nb + ROW_KINDS.index(kind))
    x = (rng.randn(nb, rows, V) * 2.0).astype(np.float32)
    cum = (-rng.rand(nb, rows) * 6.0).astype(np.float32)
    fin = np.zeros((nb, rows), dtype=np.int32)
    if kind == "quantised":
        x = (np.round(x * 4) / 4).astype(np.float32)
    elif kind == "twins" and nb > 1:
        x[nb - 1] = x[0]; cum[nb - 1] = cum[0]
    elif kind == "finished":
        fin[::2, ::2] = 3
        if nb > 1:
            fin[1, 1] = 1
    elif kind == "all_finished":
        fin[:] = 2
    return x, cum, fin


# share of compared decisions per run, measured by this restatement (python -m tests.beam_ref prints them)
RUN_SHARES = {("search_small_b", 3, 7): 1.000, ("search_small_b", 5, 7): 0.812, ("search_eos", 3, 7): 0.833, ("search_stop", 3, 7): 0.844,
              ("search_gru", 3, 7): 0.938, ("search_gru", 5, 7): 0.854, ("search_gru", 8, 7): 0.854,
              ("search_gru_b", 3, 7): 1.000, ("search_gru_b", 5, 7): 1.000, ("search_gru_b", 8, 7): 1.000,
              ("search_gru_stop", 3, 7): 1.000, ("search_gru_stop", 5, 7): 0.812, ("search_gru_stop", 8, 7): 0.781,
              ("search_gru_b", 5, 30): 0.887, ("search_gru", 3, 30): 0.860, ("search_eos", 8, 7): 0.528}

# captions of each run (of B = 4 or 6) without any near-tie decision: compared in full on the device
RUN_CAPTIONS = {("search_small_b", 3, 7): 4, ("search_small_b", 5, 7): 3, ("search_eos", 3, 7): 5, ("search_stop", 3, 7): 0,
                ("search_gru", 3, 7): 5, ("search_gru", 5, 7): 3, ("search_gru", 8, 7): 3,
                ("search_gru_b", 3, 7): 6, ("search_gru_b", 5, 7): 6, ("search_gru_b", 8, 7): 6,
                ("search_gru_stop", 3, 7): 4, ("search_gru_stop", 5, 7): 3, ("search_gru_stop", 8, 7): 3,
                ("search_gru_b", 5, 30): 4, ("search_gru", 3, 30): 4, ("search_eos", 8, 7): 3}


if __name__ == "__main__":
    from tests.golden_util import load_search_case
    for name, bw, cml, cap in SEARCH_RUNS:
        g, P, enc = load_search_case(name)
        r = beam_search_nbest(P, enc, bw, LENGTH_ALPHA, cml, g["_cell"])
        print(name, bw, cml, "steps", r["n_steps"], "share %.3f" % compared_share(r), "captions compared", int(comparable_captions(r).sum()),
              "of", enc.shape[0], "cap", cap)
