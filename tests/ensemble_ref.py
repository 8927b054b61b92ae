"""TEST INFRASTRUCTURE ONLY — float64 restatement of ensemble decoding (csrc/kernels_search.hpp:
ensemble_mix_rows_kernel, csrc/abi_search.inc: recnet_beam_search_nbest_ensemble / recnet_score_captions_ensemble) on the CPU
oracle's decoder step.

An ensemble is M models (P, cell) with weights w_m > 0, normalised in float64 to sum 1.  For one row, with x_m [V] the float32
logits of member m and l_m = log_softmax(x_m) in float64 (the maximum subtracted before the exponentials):
  arithmetic   y[v] = a + log sum_m exp(log w_m + l_m[v] - a),  a = max_m (log w_m + l_m[v])
  geometric    y[v] = sum_m w_m l_m[v]
y are the ensemble's logits: the search's candidate is cum + log_softmax(y)[v], the scorer's log-probability log_softmax(y)[token];
everything else is tests/beam_ref.py's search and tests/score_ref.py's scoring.  Every member is fed the ensemble's tokens and keeps
its own recurrent state; the regather of a step is applied to each member's.  One member: no mix, y = x_0 (what the device does), so
the functions here return exactly what beam_ref / score_ref return.

Shares of compared (step, caption) decisions of the runs below as this restatement measures them: RUN_SHARES at the end of the file
(python -m tests.ensemble_ref prints them; tests/test_ensemble_ref.py asserts the caps, 3/4 as in tests/test_beam_ref.py)."""
import numpy as np
import torch

from oracle import recnet_oracle as O
from tests import beam_ref as BR
from tests import golden_util as GU
from tests import score_ref as SC
from tests.beam_ref import EOS, PAD, comparable_captions, comparable_steps, compared_share, log_softmax64  # noqa: F401
from tests.sample_ref import NEAR_TIE  # noqa: F401

MODES = ("arithmetic", "geometric")


def norm_weights(w, M):
    w = np.ones(M) if w is None else np.asarray(w, dtype=np.float64)
    assert w.shape == (M,) and (w > 0).all() and np.isfinite(w).all()
    return w / w.sum()


def mix_rows(xs, w, mode):
    """xs: M arrays of float32 logits [..., V]; w [M] (any positive scale); returns y float64 [..., V].  Always mixes, M = 1 too
    (y = log_softmax(x_0)), like recnet_ensemble_mix_rows."""
    assert mode in MODES
    w = norm_weights(w, len(xs))
    ls = [log_softmax64(np.asarray(x, dtype=np.float32)) for x in xs]
    if mode == "geometric":
        y = np.zeros_like(ls[0])
        for m, l in enumerate(ls):
            y = y + w[m] * l
        return y
    t = np.stack([np.log(w[m]) + l for m, l in enumerate(ls)])
    a = t.max(axis=0)
    s = np.zeros_like(a)
    for m in range(len(ls)):
        s = s + np.exp(t[m] - a)
    return a + np.log(s)


def _ensemble_logits(lgs, w, mode):
    """The logits the selection / the scorer see: member 0's own for one member (no mix), else the mix."""
    return lgs[0].astype(np.float64) if len(lgs) == 1 else mix_rows(lgs, w, mode)


def select_rows(y, cum, finished, bw):
    """beam_ref.select_rows on float64 ensemble logits y [nb, rows, V] (that one takes float32 logits)."""
    nb, rows, V = y.shape
    cum = np.asarray(cum).astype(np.float64)
    fin = np.asarray(finished) != 0
    cand = cum[:, :, None] + log_softmax64(y)
    pad_only = np.full((nb, rows, V), -np.inf)
    pad_only[:, :, PAD] = cum
    cand = np.where(fin[:, :, None], pad_only, cand)
    cand = np.transpose(cand, (1, 0, 2)).reshape(rows, nb * V)
    order = np.argsort(-cand, axis=1, kind="stable")
    k = min(bw + 1, nb * V)
    top = np.take_along_axis(cand, order[:, :k], axis=1)
    return top[:, :bw], order[:, :bw].astype(np.int64), BR._margin(top)


def beam_search_nbest(models, enc, bw, length_alpha=0.0, caption_max_len=30, w=None, mode="arithmetic"):
    """tests/beam_ref.beam_search_nbest with M oracle decoder steps per hypothesis.  models: a list of (P, cell).  Returns that
    function's dict; amax [n_steps] is the max |logit| of the step over all hypotheses and members."""
    M = len(models)
    B = enc.shape[0]
    Tm = caption_max_len + 1
    toks = [torch.full((1, B), O.SOS, dtype=torch.long)]
    hids = [[O.zero_hidden(B, P["rnn.weight_hh_l0"].shape[1], cell)] for P, cell in models]        # [m][beam]
    cum = np.zeros((1, B))
    fin = np.zeros((1, B), dtype=np.int64)
    hist = np.zeros((1, B, Tm), dtype=np.int64)
    margins, amax, trace = [], [], []
    n_steps = Tm
    ar = np.arange(B)
    with torch.no_grad():
        for t in range(Tm):
            nb = len(toks)
            steps = [[O.decoder_step(P, toks[i], hids[m][i], enc, cell=cell, t=t) for i in range(nb)] for m, (P, cell) in enumerate(models)]
            lgs = [np.stack([s[0].numpy() for s in steps[m]]) for m in range(M)]          # M x [nb, B, V]
            V = lgs[0].shape[2]
            vals, idx, mg = select_rows(_ensemble_logits(lgs, w, mode), cum, fin, bw)
            src, tok = idx // V, idx % V                                 # [B, bw]
            new_hids = []
            for m, (P, cell) in enumerate(models):
                hm = []
                for k in range(bw):
                    if cell == "GRU":
                        hm.append(torch.stack([steps[m][src[b, k]][1][:, b] for b in range(B)], dim=1))
                    else:
                        hm.append(tuple(torch.stack([steps[m][src[b, k]][1][j][:, b] for b in range(B)], dim=1) for j in range(2)))
                new_hids.append(hm)
            new_hist = np.stack([hist[src[:, k], ar] for k in range(bw)])
            new_hist[:, :, t] = tok.T
            old_fin = np.stack([fin[src[:, k], ar] for k in range(bw)])
            fin = np.where(old_fin > 0, old_fin, np.where(tok.T == EOS, t + 1, 0))
            cum, hist, hids = vals.T.copy(), new_hist, new_hids
            toks = [torch.from_numpy(tok[:, k].copy()).view(1, -1) for k in range(bw)]
            margins.append(mg); amax.append(float(max(np.abs(l).max() for l in lgs)))
            trace.append((tok.T.copy(), fin.copy(), cum.copy(), hist[:, :, :t + 1].copy()))
            if (fin > 0).all():
                n_steps = t + 1
                break
    ln = np.where(fin > 0, fin, n_steps)
    score = cum / ln.astype(np.float64) ** float(length_alpha)
    order = np.argsort(-score, axis=0, kind="stable")
    g = lambda a: np.take_along_axis(a, order, axis=0)
    tokens = np.stack([hist[order[r], ar] for r in range(bw)])
    tokens = np.transpose(tokens, (0, 2, 1))[:, :n_steps]
    return dict(tokens=tokens, cum=g(cum), len=g(ln), score=g(score), n_steps=n_steps, margins=np.stack(margins),
                final_margin=BR._margin(g(score).T), amax=np.array(amax), trace=trace)


def score_captions(models, enc, captions, w=None, mode="arithmetic"):
    """tests/score_ref.score_captions at temperature 1 under the ensemble.  captions int64 [T][B].  Returns (logprobs float64 [T][B],
    amax [T]: max |logit| of the step over the members)."""
    captions = np.asarray(captions, dtype=np.int64)
    T, B = captions.shape
    tok = torch.full((1, B), O.SOS, dtype=torch.long)
    hids = [O.zero_hidden(B, P["rnn.weight_hh_l0"].shape[1], cell) for P, cell in models]
    lps, amax = [], []
    with torch.no_grad():
        for t in range(T):
            lgs = []
            for m, (P, cell) in enumerate(models):
                logits, hids[m] = O.decoder_step(P, tok, hids[m], enc, cell=cell, t=t)
                lgs.append(logits.numpy())
            if len(models) == 1:                                          # (no mix: score_ref's own expression, to the bit)
                lps.append(SC.logprob_rows(lgs[0], captions[t], 1.0))
            else:
                lps.append(log_softmax64(mix_rows(lgs, w, mode))[np.arange(B), captions[t]])
            amax.append(float(max(np.abs(l).max() for l in lgs)))
            tok = torch.from_numpy(captions[t]).view(1, -1)
    return np.stack(lps), np.array(amax)


# ---------------------------------------------------------------------------------- cases shared by the CPU and GPU tests
LENGTH_ALPHA = BR.LENGTH_ALPHA
# the member whose sizes differ from the goldens' (E = 24, H = 48, A = 16 at the V = 97 dims): formula parameters, seed chosen on the
# CPU so that the share of its run below is >= 3/4
ODD_DIMS = dict(E=24, H=48, A=16)
ODD_SEED = 31
ODD = "formula_e24_h48_a16"


def load_member(name):
    """(P, cell, enc, dims) of a member: a search golden by name, or ODD (an LSTM with the dims of search_eos but its own sizes)."""
    if name == ODD:
        g, _, enc = GU.load_search_case("search_eos")
        B, F, D, V = [int(x) for x in g["meta_dims"][:4]]
        P = GU.formula_params(GU.decoder_shapes(V, ODD_DIMS["E"], ODD_DIMS["H"], ODD_DIMS["A"], D), ODD_SEED)
        return P, "LSTM", enc, [B, F, D, V, ODD_DIMS["E"], ODD_DIMS["H"], ODD_DIMS["A"]]
    g, P, enc = GU.load_search_case(name)
    return P, g["_cell"], enc, [int(x) for x in g["meta_dims"]]


def load_models(names):
    """([(P, cell)], enc of member 0: the goldens of a group share B, F, D, V; the features fed are member 0's)."""
    ms = [load_member(n) for n in names]
    return [(m[0], m[1]) for m in ms], ms[0][2]


G97 = ("search_eos", "search_gru_b")
G97GG = ("search_gru", "search_gru_b")
G97_3 = ("search_small", "search_eos", "search_gru")
G61_3 = ("search_small_b", "search_stop", "search_gru_stop")
G97_ODD = ("search_eos", ODD)
G97_8 = ("search_small", "search_eos", "search_gru", "search_gru_b") * 2          # the most members an ensemble takes
# (members, mode, beam width, caption_max_len, weights)
SEARCH_RUNS = [
    (G97, "arithmetic", 3, 7, (1, 1)), (G97, "arithmetic", 5, 7, (1, 2)), (G97, "arithmetic", 8, 7, (1, 1)), (G97, "arithmetic", 3, 30, (1, 1)),
    (G97, "geometric", 3, 7, (1, 1)), (G97, "geometric", 5, 7, (1, 2)), (G97, "geometric", 8, 7, (1, 1)), (G97, "geometric", 3, 30, (1, 1)),
    (G97GG, "arithmetic", 3, 30, (2, 1)), (G97GG, "arithmetic", 8, 7, (1, 1)), (G97GG, "geometric", 5, 7, (1, 3)),
    (G97_3, "arithmetic", 3, 7, (1, 1, 1)), (G97_3, "geometric", 5, 7, (1, 2, 3)), (G97_3, "arithmetic", 3, 30, (1, 1, 1)),
    (G61_3, "arithmetic", 3, 7, (1, 1, 1)), (G61_3, "geometric", 5, 7, (1, 2, 3)),
    (G97_ODD, "arithmetic", 3, 7, (1, 1)),
    (G97_8, "geometric", 5, 7, (1, 2, 3, 4, 5, 6, 7, 8)),
]
SHARE_CAP = 0.75


def run_search(run):
    names, mode, bw, cml, w = run
    models, enc = load_models(names)
    return beam_search_nbest(models, enc, bw, LENGTH_ALPHA, cml, w, mode)


# (share of compared decisions, captions without any near-tie decision: compared in full on the device) per run, in the order of
# SEARCH_RUNS, measured by this restatement
RUN_SHARES = dict(zip(SEARCH_RUNS, [
    (1.000, 6), (0.938, 4), (0.812, 4), (1.000, 6),
    (1.000, 6), (0.854, 5), (1.000, 6), (1.000, 6),
    (1.000, 6), (1.000, 6), (1.000, 6),
    (0.979, 5), (0.854, 5), (0.871, 5),
    (1.000, 4), (0.812, 3),
    (1.000, 6),
    (0.833, 5),
]))


if __name__ == "__main__":
    for run in SEARCH_RUNS:
        r = run_search(run)
        print(run, "steps", r["n_steps"], "share %.3f" % compared_share(r), "captions compared", int(comparable_captions(r).sum()),
              "of", r["cum"].shape[1])
