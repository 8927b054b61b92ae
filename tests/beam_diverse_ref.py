"""TEST INFRASTRUCTURE ONLY — float64 restatement of the DIVERSE (group) N-best beam search (DESIGN.md section 14;
csrc/kernels_search.hpp: beam_select_groups_kernel, csrc/abi_search.inc: recnet_beam_search_nbest_diverse): tests/beam_ref.py
(section 11) and tests/beam_constrained_ref.py (section 12) with the selection of a step split into groups.

beam_width = G * w.  Slot k of a caption belongs to group k // w.  At t = 0 there is one start hypothesis and every group selects
from it; from t = 1 on group g selects only from its own slots g * w .. g * w + w - 1.  At step t, for g = 0 .. G - 1 in this order:
  c_g[v]  = number of slots of groups < g whose candidate selected at THIS step has token v and came from a LIVE hypothesis
  live i of group g:      pure = cum_i + log_softmax(logits_i)[v],  aug = pure - lambda * c_g[v]   (offered unless section 12 removes v)
  finished i of group g:  pure = aug = cum_i at v = <PAD>, -inf elsewhere (never penalised, never counted)
  the group keeps the w largest by aug, descending, the lowest flat index i * V + v (i: the slot; 0 at t = 0) among equal aug;
  the j-th becomes slot g * w + j with cum = pure (NOT aug), token v, state and history of slot i.
A candidate with c = 0 keeps its pure value untouched.  The margin of a (step, caption) decision is the smallest non-zero gap among
the top w + 1 offered candidates by aug, minimised over the groups.  The loop, <EOS>, len, the stop rule and the final rank over
all bw slots are section 11's; the device runs a fixed trip count, so after an early stop the selection is applied once more to the
all-finished beams (it orders every group by cum, ties by slot, and is a fixed point from then on) before the ranking.

RUNS is shared by tests/test_beam_diverse_ref.py (no GPU) and tests/test_gpu_beam_diverse.py, as are the kernel-alone cases."""
import numpy as np
import torch

from oracle import recnet_oracle as O
from tests.beam_constrained_ref import TM_ROWS, offered_mask
from tests.beam_ref import (EOS, LENGTH_ALPHA, PAD, _margin, comparable_captions, comparable_steps, compared_share,  # noqa: F401
                            log_softmax64, row_case)


def select_rows_groups(logits, cum, finished, bw, G, lam, hist=None, t=0, n=0, m=0, banned=()):
    """One grouped selection step.  logits float32 [nb, rows, V] with nb = 1 (every group selects from hypothesis 0) or nb = bw;
    cum / finished [nb, rows]; hist int64 [nb, rows, Tm] (None: allowed while n = 0).  Returns (vals float64 [rows, bw]: the
    un-penalised pure values, idx int64 [rows, bw] = slot * V + v, margin float64 [rows], aug float64 [rows, bw])."""
    logits = np.asarray(logits, dtype=np.float32)
    nb, rows, V = logits.shape
    assert bw % G == 0 and nb in (1, bw)
    w = bw // G
    cum = np.asarray(cum).astype(np.float64)
    fin = np.asarray(finished) != 0
    pure = cum[:, :, None] + log_softmax64(logits)
    offered = np.ones((nb, rows, V), dtype=bool)
    if n or m or len(banned):
        h = hist if hist is not None else np.zeros((nb, rows, max(t, 1)), dtype=np.int64)
        offered = offered_mask(h, np.asarray(finished), t, V, n, m, banned)
    pad_only = np.full((nb, rows, V), -np.inf)
    pad_only[:, :, PAD] = cum
    pure = np.where(fin[:, :, None], pad_only, pure)
    vals, augs = np.empty((rows, bw)), np.empty((rows, bw))
    idx = np.empty((rows, bw), dtype=np.int64)
    margin = np.full(rows, np.inf)
    for r in range(rows):
        counts = np.zeros(V)
        for g in range(G):
            slots = [0] if nb == 1 else list(range(g * w, g * w + w))
            p = pure[slots, r]                                           # [len(slots), V]
            live = ~fin[slots, r]
            aug = p.copy()
            hit = live[:, None] & (counts > 0)[None, :]                  # c = 0: the pure value, no arithmetic on it
            aug[hit] = (p - lam * counts[None, :])[hit]
            aug = np.where(offered[slots, r], aug, -np.inf).reshape(-1)
            order = np.argsort(-aug, kind="stable")                      # equal values keep (slot, token) order
            k = min(w + 1, aug.size)
            margin[r] = min(margin[r], _margin(aug[order[:k]][None, :])[0])
            for j, f in enumerate(order[:w]):
                li, v = divmod(int(f), V)
                vals[r, g * w + j] = p[li, v]; augs[r, g * w + j] = aug[f]; idx[r, g * w + j] = slots[li] * V + v
                if live[li]:
                    counts[v] += 1
    return vals, idx, margin, augs


def beam_search_nbest(P, enc, bw, G, lam, length_alpha=0.0, caption_max_len=30, cell="LSTM", n=0, m=0, banned=()):
    """beam_constrained_ref.beam_search_nbest with the grouped selection; the same dict plus group int64 [bw][B] (the group of each
    returned rank) and after_stop: None when the search ran all steps, else (cum [bw][B] in slot order after the one further
    selection, the slot permutation [B][bw] it applied, the one a second application gives)."""
    B = enc.shape[0]
    H = P["rnn.weight_hh_l0"].shape[1]
    Tm = caption_max_len + 1
    w = bw // G
    toks = [torch.full((1, B), O.SOS, dtype=torch.long)]
    hids = [O.zero_hidden(B, H, cell)]
    cum = np.zeros((1, B))
    fin = np.zeros((1, B), dtype=np.int64)
    hist = np.zeros((1, B, Tm), dtype=np.int64)
    margins, amax, trace = [], [], []
    n_steps = Tm
    ar = np.arange(B)
    V = None
    with torch.no_grad():
        for t in range(Tm):
            nb = len(toks)
            steps = [O.decoder_step(P, toks[i], hids[i], enc, cell=cell, t=t) for i in range(nb)]
            lg = np.stack([s[0].numpy() for s in steps])                 # [nb, B, V]
            V = lg.shape[2]
            vals, idx, mg, _ = select_rows_groups(lg, cum, fin, bw, G, lam, hist, t, n, m, banned)
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
    after_stop = None
    if n_steps < Tm:                                                     # the fixed trip count: one further selection, then a fixed point
        zeros = np.zeros((bw, B, V), dtype=np.float32)
        vals, idx, _, _ = select_rows_groups(zeros, cum, fin, bw, G, lam, hist, n_steps, n, m, banned)
        src = idx // V
        assert (idx % V == PAD).all() and np.isfinite(vals).all()
        cum2 = vals.T.copy()
        hist = np.stack([hist[src[:, k], ar] for k in range(bw)])
        fin = np.stack([fin[src[:, k], ar] for k in range(bw)])
        _, idx3, _, _ = select_rows_groups(zeros, cum2, fin, bw, G, lam, hist, min(n_steps + 1, Tm - 1), n, m, banned)
        after_stop = (cum2, src, idx3 // V)
        cum = cum2
    ln = np.where(fin > 0, fin, n_steps)
    score = cum / ln.astype(np.float64) ** float(length_alpha)
    order = np.argsort(-score, axis=0, kind="stable")                    # [bw, B]: the lowest slot among equals
    g = lambda a: np.take_along_axis(a, order, axis=0)
    tokens = np.stack([hist[order[r], ar] for r in range(bw)])           # [bw, B, Tm]
    tokens = np.transpose(tokens, (0, 2, 1))[:, :n_steps]
    return dict(tokens=tokens, cum=g(cum), len=g(ln), score=g(score), n_steps=n_steps, margins=np.stack(margins),
                final_margin=_margin(g(score).T), amax=np.array(amax), trace=trace, group=order // w, after_stop=after_stop)


def nbest_diversity(lists):
    """search.nbest_diversity restated: per caption (distinct captions, distinct-1, distinct-2) of its token lists."""
    out = []
    for caps in lists:
        caps = [tuple(int(x) for x in c) for c in caps]
        uni = [x for c in caps for x in c]
        bi = [c[j:j + 2] for c in caps for j in range(len(c) - 1)]
        out.append((len(set(caps)), len(set(uni)) / len(uni) if uni else 0.0, len(set(bi)) / len(bi) if bi else 0.0))
    return out


# ---------------------------------------------------------------------------------- runs shared by the CPU and GPU tests
CAP = 0.6            # on the share of compared (step, caption) decisions, every run


def _run(name, bw, G, lam, cml, steps, share, full, n=0, m=0, banned=()):
    return dict(name=name, bw=bw, G=G, lam=lam, cml=cml, n=n, m=m, banned=banned, steps=steps, share=share, full=full)


RUNS = [
    _run("search_small_b", 4, 2, 0.5, 7, 8, 1.000, (4, 4)),
    _run("search_eos", 6, 3, 1.0, 7, 8, 0.667, (4, 6)),
    _run("search_eos", 4, 2, 0.5, 7, 4, 0.667, (4, 6)),                  # early stop
    _run("search_eos", 2, 2, 0.5, 7, 3, 0.833, (5, 6)),                  # early stop, w = 1
    _run("search_stop", 4, 4, 0.5, 7, 8, 1.000, (4, 4)),                 # the penalty never binds: four equal captions
    _run("search_gru", 6, 2, 0.5, 7, 8, 0.938, (4, 6)),
    _run("search_gru", 8, 4, 1.0, 7, 8, 0.875, (3, 6)),
    _run("search_gru", 8, 8, 0.5, 7, 8, 0.625, (3, 6)),
    _run("search_gru_b", 8, 2, 0.5, 7, 8, 1.000, (6, 6)),
    _run("search_gru_b", 6, 3, 2.0, 7, 8, 1.000, (6, 6)),
    _run("search_gru_stop", 8, 4, 0.5, 7, 8, 0.656, (2, 4)),
    _run("search_gru_b", 8, 4, 0.5, 30, 31, 1.000, (6, 6)),
    _run("search_gru", 6, 3, 1.0, 30, 31, 0.720, (4, 6)),
    _run("search_gru", 8, 4, 1e4, 7, 8, 0.812, (2, 6)),
    _run("search_small_b", 6, 3, 1e4, 7, 8, 0.750, (3, 4)),
    _run("search_gru", 6, 3, 0.5, 30, 26, 0.833, (5, 6), n=1),
    _run("search_gru_b", 8, 4, 0.5, 7, 8, 0.729, (2, 6), n=2, m=3, banned=(33, 39)),
    _run("search_gru", 6, 3, 1.0, 7, 8, 1.000, (6, 6), n=2, m=3, banned=(55, 78)),
    _run("search_gru_stop", 6, 3, 0.5, 7, 8, 0.781, (2, 4), n=2),
    _run("search_small_b", 6, 2, 0.5, 7, 8, 0.750, (2, 4), n=2),
    # shape_rows160: the shape case rows160 of tests/search_shapes.py (B = 20, H = 320): 160 rows, the ring GEMM past one row tile
    _run("rows160", 8, 2, 0.5, 7, 8, 0.994, (18, 20)),
]


def run_id(run):
    return "%s-w%d-g%d-l%g-c%d-n%d-m%d-b%d" % (run["name"], run["bw"], run["G"], run["lam"], run["cml"], run["n"], run["m"], len(run["banned"]))


# ---------------------------------------------------------------------------------- kernel-alone cases
ROW_VS = (8, 61, 255, 256, 257, 4188, 12500)
ROW_BW_G = ((2, 2), (4, 2), (6, 3), (8, 2), (8, 4), (8, 8))
PEAK_GAP = 2.0       # d of the constructed peaks
LAM_HIGH = 100.0     # a penalty no candidate of these cases survives


def _case(label, x, cum, fin, lam, hist=None, t=0, n=0, m=0, banned=(), **extra):
    return dict(label=label, x=x, cum=cum, fin=fin, lam=lam, hist=hist, t=t, n=n, m=m, banned=tuple(banned), **extra)


def _base(V, nb, kind="continuous", rows=5):
    x, cum, fin = row_case(V, nb, kind, rows)
    return x.copy(), cum.copy(), fin.copy()


def _raise(x, tok, gap):
    """token `tok` becomes the arg-max of every row of x [.., V] it is raised in, `gap` above the largest other logit"""
    x[..., tok] = -np.inf
    x[..., tok] = x.max(axis=-1) + np.float32(gap)


def group_cases(V, bw, G, nb):
    """The kernel-alone cases of one (V, bw, G, nb), nb in (1, bw): each a dict(label, x, cum, fin, lam, hist, t, n, m, banned) and,
    for the constructed ones, what test_constructed_cases / the device test read besides (peak, ...)."""
    w = bw // G
    d = PEAK_GAP
    out = []
    # (quantised logits are multiples of 1/4: with a penalty that is one too, a penalised and an un-penalised candidate of one
    # hypothesis tie in exact arithmetic, and fp32 and float64 round the two sides differently: not a tie the index rule resolves
    # the same way everywhere.  0.3141 * c stays 6e-3 or more away from every multiple of 1/4 for c <= 7.)
    for kind, lam in (("continuous", 0.5), ("quantised", 0.3141)):
        x, cum, fin = _base(V, nb, kind)
        out.append(_case(kind, x, cum, fin, lam))
    # a shared peak: below d / 7 every group's first slot keeps it, above d every later group leaves it
    peak = 5 % V
    for lam, label in ((d / 8, "peak_low"), (LAM_HIGH, "peak_high")):
        x, cum, fin = _base(V, nb)
        _raise(x, peak, d)
        out.append(_case(label, x, cum, fin, lam, peak=peak))
    # an all-finished beam in ascending cum (every group is ordered by cum, ties by slot)
    x, cum, fin = _base(V, nb)
    fin[:] = 2
    cum[:] = np.sort(cum, axis=0)
    if nb > 2:
        cum[1] = cum[0]                                                  # (an exact tie: the lower slot first)
    out.append(_case("all_finished_ascending", x, cum, fin, 0.5))
    if nb == bw and w >= 2:
        # two slots of group 0 choose token q: the count is 2 for group 1, whose q leads by 1.5 lambda (one count would keep it)
        q = 6 % V
        x, cum, fin = _base(V, nb)
        lam = 2.0
        x[2:w, :, q] = -30.0
        _raise(x[:2], q, 20.0)
        _raise(x[w:], q, 1.5 * lam)
        cum[:2] = cum[:w].max(axis=0)                                    # (the best cum of the group, twice: slots 0 and 1 lead with q)
        out.append(_case("count_two", x, cum, fin, lam, peak=q))
    if nb == bw and G >= 2:
        # rows 0, 2, 4: group 0 is finished and slot 0 leads, its <PAD> is not counted, so group 1 leads with its <PAD> peak (gap
        # d < lambda; that live pick is counted for the groups behind it); rows 1, 3: slot 0 is live and picks <PAD>: counted, no
        # later group leads with it
        x, cum, fin = _base(V, nb)
        _raise(x, PAD, d)
        fin[:w, ::2] = 2
        cum[0] = cum.max(axis=0) + 1.0
        out.append(_case("finished_pad", x, cum, fin, 2.0 * d, peak=PAD))
        # the token group 0 chose is also banned for the hypotheses of the later groups (n = 1: their history holds it)
        if V >= 61:
            q, t = 9, 3
            x, cum, fin = _base(V, nb)
            _raise(x, q, d)
            rng = np.random.RandomState(4000 + V + bw + G)
            hist = rng.randint(10, 14, size=(nb, x.shape[1], TM_ROWS)).astype(np.int64)
            hist[w:, :, 1] = q
            out.append(_case("chosen_and_banned", x, cum, fin, d / 8, hist=hist, t=t, n=1, peak=q))
    if V >= 61:
        # the constrained form on random histories, static bans and a minimum length beside the penalty
        t = 3 if nb == bw else 0
        x, cum, fin = _base(V, nb)
        rng = np.random.RandomState(4100 + V + bw + G)
        hist = rng.randint(3, 7, size=(nb, x.shape[1], TM_ROWS)).astype(np.int64)
        for tok in (3, 4, 5, 6, EOS):
            x[..., tok] += 6.0
        out.append(_case("constrained", x, cum, fin, 0.5, hist=hist, t=t, n=2, m=5, banned=(5,)))
    if V >= 600:
        # penalised tokens 256 apart: one thread of the kernel meets them all
        x, cum, fin = _base(V, nb)
        for k, tok in enumerate((519, 263, 7)):
            x[..., tok] = np.float32(12.0 + k)
        out.append(_case("residue", x, cum, fin, LAM_HIGH, residue=(7, 263, 519)))
    return out
