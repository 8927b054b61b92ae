"""TEST INFRASTRUCTURE ONLY — float64 restatement of the CONSTRAINED N-best beam search (DESIGN.md section 12;
csrc/kernels_search.hpp: beam_select_kernel<BW, true>, csrc/abi_search.inc: recnet_beam_search_nbest_constrained): tests/beam_ref.py
(section 11) with one sentence added to the candidate rule.

At step t a LIVE hypothesis with the generated history w_0 .. w_{t-1} (its hist row; <SOS> is not part of it) does not offer v if
  1. v is one of `banned`;  or
  2. v = <EOS> and t < m (min_length);  or
  3. n >= 1 (no_repeat_ngram), t >= n - 1, and some j in [0, t - n] has (w_j .. w_{j+n-2}) = (w_{t-n+1} .. w_{t-1}) and v = w_{j+n-1}
     (n = 1: both tuples are empty — every token of the history is banned).
Tokens compare as ids.  Finished hypotheses are untouched: <PAD> at cum, -inf elsewhere.  There is no renormalisation: an offered
candidate is still cum_i + log_softmax(logits_i)[v] over all V entries.  A call with a constraint on needs
beam_width + n_banned + t + 1 <= V at every step it runs, so a live hypothesis always has beam_width offered tokens and "not
offered" cannot be told from "offered at -inf": the restatement writes -inf.  A decision's margin is taken among the top
bw + 1 OFFERED candidates (a gap to -inf is infinite and never the smallest).

The run table (RUNS) and the kernel-alone cases (row_cases) are shared by tests/test_beam_constrained_ref.py (no GPU) and
tests/test_gpu_beam_constrained.py."""
import numpy as np
import torch

from oracle import recnet_oracle as O
from tests.beam_ref import (EOS, LENGTH_ALPHA, PAD, _margin, comparable_captions, comparable_steps, compared_share,  # noqa: F401
                            log_softmax64, row_case)

TM_ROWS = 8          # Tm of the kernel-alone cases


def banned_ids(history, t, n, m, banned):
    """The set of ids a live hypothesis with `history` (a sequence; entries [0, t) are read) does not offer at step t."""
    w = [int(x) for x in history[:t]]
    out = {int(v) for v in banned}
    if t < m:
        out.add(EOS)
    if n >= 1 and t >= n - 1:
        suffix = w[t - n + 1:t]
        for j in range(0, t - n + 1):
            if w[j:j + n - 1] == suffix:
                out.add(w[j + n - 1])
    return out


def offered_mask(hist, finished, t, V, n, m, banned):
    """bool [nb, rows, V]: True where hypothesis (i, r) offers v under the ban rule (all True for a finished one: its <PAD>-only
    rule is select_rows')."""
    nb, rows = finished.shape
    ok = np.ones((nb, rows, V), dtype=bool)
    for i in range(nb):
        for r in range(rows):
            if finished[i, r] == 0:
                ids = [v for v in banned_ids(hist[i, r], t, n, m, banned) if 0 <= v < V]
                ok[i, r, ids] = False
    return ok


def select_rows(logits, cum, finished, bw, hist=None, t=0, n=0, m=0, banned=()):
    """beam_ref.select_rows with the ban rule.  hist int64 [nb, rows, Tm] (None: allowed while n = 0)."""
    return select_rows_widths(logits, cum, finished, (bw,), hist, t, n, m, banned)[bw]


def select_rows_widths(logits, cum, finished, bws, hist=None, t=0, n=0, m=0, banned=()):
    """{bw: (vals, idx, margin)} of select_rows for several widths on one set of candidates (sorted once)."""
    logits = np.asarray(logits, dtype=np.float32)
    nb, rows, V = logits.shape
    cum = np.asarray(cum).astype(np.float64)
    fin = np.asarray(finished) != 0
    cand = cum[:, :, None] + log_softmax64(logits)
    if n or m or len(banned):
        h = hist if hist is not None else np.zeros((nb, rows, max(t, 1)), dtype=np.int64)
        cand = np.where(offered_mask(h, np.asarray(finished), t, V, n, m, banned), cand, -np.inf)
    pad_only = np.full((nb, rows, V), -np.inf)
    pad_only[:, :, PAD] = cum
    cand = np.where(fin[:, :, None], pad_only, cand)
    cand = np.transpose(cand, (1, 0, 2)).reshape(rows, nb * V)
    order = np.argsort(-cand, axis=1, kind="stable")                     # equal values keep index order
    out = {}
    for bw in bws:
        k = min(bw + 1, nb * V)
        top = np.take_along_axis(cand, order[:, :k], axis=1)
        out[bw] = (top[:, :bw], order[:, :bw].astype(np.int64), _margin(top))
    return out


def beam_search_nbest(P, enc, bw, length_alpha=0.0, caption_max_len=30, cell="LSTM", n=0, m=0, banned=()):
    """beam_ref.beam_search_nbest with the constrained selection; the same dict."""
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
            vals, idx, mg = select_rows(lg, cum, fin, bw, hist, t, n, m, banned)
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


def violations(tokens, lens, n, m, banned):
    """Over each hypothesis' first len tokens (tokens [bw][n_steps][B], lens [bw][B]; arrays or nested lists): how many repeat an
    n-gram, how many end with <EOS> after fewer than m words, how many contain a banned id.  A constraint that is off counts 0."""
    tokens, lens = np.asarray(tokens), np.asarray(lens)
    rep = short = ban = 0
    bset = {int(v) for v in banned}
    for k in range(tokens.shape[0]):
        for b in range(tokens.shape[2]):
            L = int(lens[k, b])
            w = [int(x) for x in tokens[k, :L, b]]
            if n >= 1:
                grams = [tuple(w[j:j + n]) for j in range(L - n + 1)]
                rep += len(set(grams)) != len(grams)
            short += bool(L and w[L - 1] == EOS and L - 1 < m)
            ban += bool(bset.intersection(w))
    return rep, short, ban


def width1_steps(r1, prec):
    """int [B]: how many decisions of each caption of a WIDTH-1 result precede the first one that the precision could flip.  At
    width 1 every candidate of a step shares cum, so a decision flips only if two log-probabilities swap: those closer than twice
    score_ref.row_bar(prec) at the step's max |logit| (and never fewer than NEAR_TIE, the bar of every other comparison here)."""
    from tests.sample_ref import NEAR_TIE
    from tests.score_ref import row_bar
    guard = np.array([max(NEAR_TIE, 2.0 * row_bar(prec, a, 1.0)) for a in r1["amax"]])[:, None]
    return (~(np.cumsum(r1["margins"] < guard, axis=0) > 0)).sum(axis=0)


def frequent_ids(tokens, lens, count=2):
    """The `count` most frequent ids above 2 among the hypotheses' first len tokens, the lower id among equally frequent ones."""
    tokens, lens = np.asarray(tokens), np.asarray(lens)
    freq = {}
    for k in range(tokens.shape[0]):
        for b in range(tokens.shape[2]):
            for x in tokens[k, :int(lens[k, b]), b]:
                if x > 2:
                    freq[int(x)] = freq.get(int(x), 0) + 1
    return tuple(sorted(sorted(freq, key=lambda v: (-freq[v], v))[:count]))


# ---------------------------------------------------------------------------------- runs shared by the CPU and GPU tests
# golden, width, caption_max_len, n, m, banned, cap on the compared share, n_steps (unconstrained, constrained), hypotheses of the
# UNCONSTRAINED search that violate (repeat, short, banned) of total, share of compared decisions, captions compared in full (of B);
# slack: the constraints (0 repeat, 1 short, 2 banned) that are on in the run without binding on the unconstrained result
RUNS = [
    dict(name="search_small_b", bw=3, cml=7, n=2, m=0, banned=(), cap=0.75, steps=(8, 8), unc=(12, 0, 0), total=12, share=1.000, full=(3, 4)),
    dict(name="search_small_b", bw=5, cml=7, n=3, m=0, banned=(), cap=0.75, steps=(8, 8), unc=(12, 0, 0), total=20, share=0.812, full=(2, 4)),
    # (slack: min_length = 2 is on here, yet the issue's table lists 0 short hypotheses; min_length binds in three other runs)
    dict(name="search_small_b", bw=3, cml=7, n=2, m=2, banned=(51, 52), cap=0.75, steps=(8, 8), unc=(12, 0, 12), total=12, share=0.969, full=(3, 4),
         slack=(1,)),
    dict(name="search_eos", bw=3, cml=7, n=0, m=4, banned=(), cap=0.5, steps=(5, 8), unc=(0, 17, 0), total=18, share=0.542, full=(3, 6)),
    dict(name="search_gru_stop", bw=3, cml=7, n=2, m=0, banned=(), cap=0.75, steps=(8, 8), unc=(12, 0, 0), total=12, share=0.875, full=(3, 4)),
    dict(name="search_gru", bw=3, cml=7, n=2, m=3, banned=(55, 78), cap=0.75, steps=(8, 8), unc=(6, 12, 4), total=18, share=1.000, full=(6, 6)),
    dict(name="search_gru", bw=8, cml=7, n=3, m=0, banned=(), cap=0.75, steps=(8, 8), unc=(16, 0, 0), total=48, share=0.812, full=(3, 6)),
    dict(name="search_gru_b", bw=3, cml=7, n=1, m=0, banned=(), cap=0.75, steps=(8, 8), unc=(14, 0, 0), total=18, share=1.000, full=(6, 6)),
    dict(name="search_gru_b", bw=8, cml=7, n=2, m=3, banned=(33, 39), cap=0.75, steps=(8, 8), unc=(21, 15, 22), total=48, share=1.000, full=(5, 6)),
    dict(name="search_gru_b", bw=5, cml=30, n=3, m=0, banned=(), cap=0.75, steps=(31, 31), unc=(20, 0, 0), total=30, share=0.962, full=(5, 6)),
    dict(name="search_gru", bw=3, cml=30, n=2, m=0, banned=(), cap=0.75, steps=(31, 31), unc=(6, 0, 0), total=18, share=0.855, full=(5, 6)),
    dict(name="search_gru", bw=3, cml=30, n=1, m=0, banned=(), cap=0.75, steps=(31, 26), unc=(6, 0, 0), total=18, share=1.000, full=(6, 6)),
    # shape_rows160: the shape case rows160 of tests/search_shapes.py (B = 20, H = 320): 160 rows, the ring GEMM past one row tile;
    # one banned id, the most frequent one of the unconstrained result
    dict(name="rows160", bw=8, cml=7, n=2, m=3, banned=(72,), cap=0.75, steps=(8, 8), unc=(75, 75, 118), total=160, share=0.838, full=(14, 20)),
]


def run_id(run):
    return "%s-w%d-c%d-n%d-m%d-b%d" % (run["name"], run["bw"], run["cml"], run["n"], run["m"], len(run["banned"]))


# ---------------------------------------------------------------------------------- kernel-alone cases
ROW_VS = (61, 255, 256, 257, 4188)
ROW_NB = (1, 3, 8)
ROW_BW = (1, 3, 8)
ROW_N = (1, 2, 3)
HIST_KINDS = ("random4", "abab", "same", "pad_finished", "twins")


def row_ts(n):
    return sorted({0, 1, n - 1, TM_ROWS - 1})


def make_hist(kind, nb, rows, Tm, rng):
    """Histories int64 [nb, rows, Tm] over small alphabets above <EOS>."""
    if kind == "random4":
        return rng.randint(3, 7, size=(nb, rows, Tm)).astype(np.int64)
    h = np.zeros((nb, rows, Tm), dtype=np.int64)
    if kind == "abab":
        h[:] = 3 + (np.arange(Tm) & 1)
    elif kind == "same":
        h[:] = 5
    elif kind == "pad_finished":                 # hypothesis 0: <PAD> throughout (it is finished below); the others a b a b
        h[:] = 3 + (np.arange(Tm) & 1)
        h[0] = PAD
    elif kind == "twins":                        # the last hypothesis repeats hypothesis 0's logits and cum, not its history
        h[:] = 3 + (np.arange(Tm) & 1)
        h[nb - 1] = 5
    return h


def raise_banned(x, fin, hist, t, n, m, banned, union=None):
    """Every token the rule removes from a live hypothesis gets the row's maximum + 1: a ban decides the outcome.  union: pairs
    (i, j) of hypotheses that receive the union of their two ban sets (twins keep equal logits).  Changes x in place."""
    nb, rows, V = x.shape
    for r in range(rows):
        sets = [banned_ids(hist[i, r], t, n, m, banned) if fin[i, r] == 0 else set() for i in range(nb)]
        for i, j in (union or ()):
            sets[i] = sets[j] = sets[i] | sets[j]
        for i in range(nb):
            ids = [v for v in sets[i] if 0 <= v < V]
            if ids:
                x[i, r, ids] = x[i, r].max() + 1.0


def ban_case(V, nb, n, t, hist_kind, logit_kind="continuous", m=0, banned=(), Tm=TM_ROWS, rows=5):
    """One kernel-alone case: dict(x, cum, fin, hist, t, n, m, banned, tie) — tie: the constructed cross-beam tie is present."""
    x, cum, fin = row_case(V, nb, logit_kind, rows)
    x, cum, fin = x.copy(), cum.copy(), fin.copy()
    rng = np.random.RandomState(7000 + 31 * V + 7 * nb + 3 * n + t + 100 * HIST_KINDS.index(hist_kind))
    hist = make_hist(hist_kind, nb, rows, Tm, rng)
    hist[:, :, t:] = rng.randint(3, 7, size=hist[:, :, t:].shape)          # entries behind t are never read
    union = None
    if hist_kind == "pad_finished":
        fin[0, :] = 2
    if hist_kind == "twins" and nb > 1:
        cum[0] = cum.max(axis=0) + 1.0           # the twins lead, so what only one of them offers is selected
        x[nb - 1] = x[0]; cum[nb - 1] = cum[0]
        union = [(0, nb - 1)]
    raise_banned(x, fin, hist, t, n, m, banned, union)
    return dict(x=x, cum=cum, fin=fin, hist=hist, t=t, n=n, m=m, banned=tuple(banned), tie=hist_kind == "twins" and nb > 1,
                case=(V, nb, n, t, hist_kind, logit_kind, m, len(banned)))


def row_cases(V, nb):
    """The n-gram cases of one (V, nb): random histories with both kinds of logits, the constructed histories with continuous ones."""
    out = []
    for n in ROW_N:
        for t in row_ts(n):
            out.append(ban_case(V, nb, n, t, "random4", "continuous"))
            out.append(ban_case(V, nb, n, t, "random4", "quantised"))
            for kind in HIST_KINDS[1:]:
                out.append(ban_case(V, nb, n, t, kind, "continuous"))
    return out


def min_length_cases(V, nb):
    """<EOS> is the arg-max of every row; t < m (it is not offered) and t >= m (it is)."""
    out = []
    for t, m in ((1, 3), (3, 3), (5, 3), (0, 1)):
        c = ban_case(V, nb, 0, t, "random4", "continuous", m=0)
        c["x"][:, :, EOS] = c["x"].max(axis=2) + 2.0
        c["m"] = m
        c["case"] = c["case"][:6] + (m, 0)
        out.append(c)
    return out


def residue_cases(V, nb, t=5, Tm=TM_ROWS):
    """Banned ids that are 256 apart (the kernel's threads walk the vocabulary in strides of 256: one thread meets them all), as
    static bans and as n-gram bans from a history that holds them.  Empty below V = 600."""
    if V < 600:
        return []
    a = ban_case(V, nb, 0, t, "random4", "continuous", banned=(7, 263, 519), Tm=Tm)
    b = ban_case(V, nb, 1, t, "random4", "continuous", Tm=Tm)
    b["hist"][:, :, 0:3] = (9, 265, 521)
    raise_banned(b["x"], b["fin"], b["hist"], t, 1, 0, ())
    return [a, b]


def static_ban_case(V, nb, t=3, n=2):
    """16 static bans that hold the 16 largest logits of every row (and an n-gram rule beside them)."""
    rng = np.random.RandomState(8000 + V + nb)
    ids = tuple(int(v) for v in np.sort(rng.choice(np.arange(3, V), size=16, replace=False)))
    c = ban_case(V, nb, n, t, "random4", "continuous", banned=ids)
    return c
