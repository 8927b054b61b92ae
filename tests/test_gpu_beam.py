"""The N-best beam search on log-probabilities on the device (recnet_beam_select_rows / recnet_beam_search_nbest) against the
CPU restatement (tests/beam_ref.py): the selection kernel alone on host-made logits, the search on the goldens' decoders,
self-consistency with greedy_search and score_captions in both precisions, the reranking by the reconstructor, evaluate(), and the
argument checks.

Indices / tokens are compared outside the decisions the restatement marks as near-ties (margin below 1e-3; the caps on how many
those may be are held without a GPU by tests/test_beam_ref.py).  A candidate is a cum plus a log-probability: it is held to the
row bar of tests/search_kit.py's lp_bar at temperature 1 (= score_ref.row_bar) plus two units in the last place of |cum|; a
hypothesis' cum to its length times the row bar.  Every test prints its worst error / bar."""
import functools

import numpy as np
import pytest
import torch

import recnet_amd as R
from recnet_amd import _ops, search
from tests import beam_ref as BR
from tests import golden_util as GU
from tests import score_ref as SC
from tests.golden_util import load_search_case
from tests.gpu_util import make_models
from tests.sample_ref import NEAR_TIE
from tests.search_kit import check_nbest_against_restatement, check_self_consistency, decoder_for, rows_engine

pytestmark = pytest.mark.gpu

# the package's own engine module and the _lib whose RecNetError it raises (attributes of the package: no second import of either)
Engine, _lib = R.engine.Engine, R.engine._lib


# ------------------------------------------------------------------------------------------------ 1. the selection kernel alone
@functools.lru_cache(maxsize=None)
def _row_results(V):
    """Every kernel-alone case at vocabulary V, device (two calls) and restatement side by side (computed once)."""
    eng = rows_engine()
    out = []
    for nb in BR.ROW_NB:
        for kind in BR.ROW_KINDS:
            x, cum, fin = BR.row_case(V, nb, kind)
            xd, cd, fd = torch.from_numpy(x).cuda(), torch.from_numpy(cum).cuda(), torch.from_numpy(fin).cuda()
            before = xd.clone()
            for bw in BR.ROW_BW:
                if bw > V:
                    continue
                vals, idx = eng.beam_select_rows(xd, cd, fd, bw)
                vals2, idx2 = eng.beam_select_rows(xd, cd, fd, bw)
                torch.cuda.synchronize()
                same = torch.equal(vals.view(torch.int32), vals2.view(torch.int32)) and torch.equal(idx, idx2)
                untouched = torch.equal(xd.view(torch.int32), before.view(torch.int32))
                rv, ri, margin = BR.select_rows(x, cum, fin, bw)
                out.append(dict(case=(V, nb, kind, bw), x=x, cum=cum, fin=fin, vals=vals.cpu().numpy(), idx=idx.cpu().numpy(),
                                ref_vals=rv, ref_idx=ri, margin=margin, same=same, untouched=untouched))
    return out


@pytest.mark.parametrize("V", BR.ROW_VS)
def test_select_rows(V):
    worst = 0.0
    for r in _row_results(V):
        _, nb, kind, bw = r["case"]
        assert r["untouched"] and r["same"], r["case"]
        idx, vals = r["idx"].astype(np.int64), r["vals"].astype(np.float64)
        assert ((idx >= 0) & (idx < nb * V)).all(), r["case"]
        keep = r["margin"] >= NEAR_TIE
        assert np.array_equal(idx[keep], r["ref_idx"][keep]), (r["case"], idx, r["ref_idx"])
        src, tok = idx // V, idx % V
        if kind == "twins" and nb > 1:          # the constructed tie across beams: exact on every row, the lower beam first
            for row, k in zip(*np.nonzero(src == nb - 1)):
                assert k > 0 and idx[row, k - 1] == idx[row, k] - (nb - 1) * V and r["vals"][row, k - 1] == r["vals"][row, k], r["case"]
        if kind == "quantised":                 # ties inside a row: equal logits give equal candidates, lowest index first
            for row in range(idx.shape[0]):
                for k in range(1, bw):
                    if src[row, k] == src[row, k - 1] and r["x"][src[row, k], row, tok[row, k]] == r["x"][src[row, k], row, tok[row, k - 1]]:
                        assert r["vals"][row, k] == r["vals"][row, k - 1] and idx[row, k] > idx[row, k - 1], r["case"]
        if kind == "all_finished":              # <PAD> at cum, to the bit; then -inf by index
            assert np.array_equal(idx, r["ref_idx"]) and np.array_equal(vals, r["ref_vals"]), r["case"]
        inf = np.isneginf(r["ref_vals"])
        assert np.array_equal(np.isneginf(vals), inf), r["case"]
        live = r["fin"] == 0
        amax = np.abs(r["x"][live]).max() if live.any() else 0.0
        bar = SC.row_bar("f32", amax, 1.0) + 2 * float(np.spacing(np.float32(np.abs(r["cum"]).max())))
        err = np.abs(vals[~inf] - r["ref_vals"][~inf])
        if err.size:
            worst = max(worst, float(err.max() / bar))
            assert err.max() <= bar, (r["case"], float(err.max()), bar)
    print("V", V, "worst candidate error / bar:", worst)


# ------------------------------------------------------------------------------------------------ 2. the search
@pytest.mark.parametrize("name,bw,cml,cap", BR.SEARCH_RUNS)
def test_search_matches_the_restatement(name, bw, cml, cap):
    """fp32 path: n_steps (when no caption is excluded), tokens, len and the rank order equal the restatement on the captions without
    any near-tie decision; cum within len x the row bar, score within the same bar (len^alpha >= 1).  A caption with a near-tie is
    compared up to that decision: the first t0 tokens of each of its returned hypotheses against the restatement's beams."""
    check_nbest_against_restatement(name, bw, cml)


@pytest.mark.parametrize("name", ["search_small", "search_gru"])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_self_consistency(name, prec):
    """Width 1 is greedy_search up to each caption's first <EOS>, exactly (the same step at the same precision, the same tie rule);
    score_captions on each returned rank reproduces len exactly and cum within len x the row bar of the precision; a second call
    gives the same bits; every rank is canonical."""
    check_self_consistency(name, prec)


# ------------------------------------------------------------------------------------------------ 3. reranking, evaluate
@pytest.mark.parametrize("kind", ["global", "local"])
def test_best_of_beam_and_evaluate(kind):
    dims = [6, 5, 32, 41, 12, 24, 8, 8]
    B, F, D, V, E, H, A, RA = dims
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D), 21)
    recP = GU.formula_params(GU.rec_shapes(kind, H, D, RA), 22)
    enc, _ = GU.make_batch(B, F, D, V, [3] * B, 23)
    Cfg, dec, rec = make_models(list(dims), kind, "f32", decP, recP)
    dm, rm = dec["model"].eval(), rec["model"].eval()
    encd = enc.cuda()
    inp = torch.full((1, B), 1, dtype=torch.long, device="cuda")
    hid = (torch.zeros(1, B, H, device="cuda"), torch.zeros(1, B, H, device="cuda"))
    bw, weight = 4, 256.0
    # without a reconstructor at length_alpha = 1 the search's own order is pick_best_of_n's: rank 0
    hyps = R.beam_search_nbest(Cfg, dm, inp, hid, encd, bw, 1.0)
    caps, ks, scores = R.best_of_beam(Cfg, dm, inp, hid, encd, bw, 1.0)
    assert ks == [0] * B and caps == [h[0][0] for h in hyps]
    assert R.best_of_beam(Cfg, dm, inp, hid, encd, bw, 1.0, reconstructor=rm, recon_weight=0.0) == (caps, ks, scores)
    for b in range(B):
        assert scores[b] == hyps[b][0][1] / hyps[b][0][2]
    # with the term: pick_best_of_n on the public reconstruction errors of the returned ranks at the common T = n_steps
    toks, cum, ln, _ = search._beam_nbest(Cfg, dm, inp, hid, encd, bw, 0.7)
    n = toks.shape[1]
    errs = [R.reconstruction_errors(Cfg, dm, rm, encd, toks[k].contiguous(), T=n) for k in range(bw)]
    rk, rs = R.pick_best_of_n(cum.cpu().tolist(), ln.cpu().tolist(), errs, weight)
    caps_w, ks_w, scores_w = R.best_of_beam(Cfg, dm, inp, hid, encd, bw, 0.7, reconstructor=rm, recon_weight=weight)
    assert ks_w == rk and scores_w == rs
    lens = ln.cpu().tolist()
    tl = toks.cpu().tolist()
    for b in range(B):
        assert caps_w[b] == [tl[ks_w[b]][t][b] for t in range(lens[ks_w[b]][b])]
    print(kind, "best of beam", bw, ": ranks chosen with the reconstruction term", ks_w)
    # evaluate
    idx2word = {i: "w%d" % i for i in range(V)}
    names = ["a", "b", "c", "d", "PAD", "PAD"]
    refs = {k: ["w3 w4 w5", "w7 w8"] for k in "abcd"}
    ev = lambda method, **kw: R.evaluate(Cfg, [(names, enc.numpy())], dm, method, idx2word, refs, **kw)
    s_greedy = ev("greedy")
    assert set(ev(("beam_nbest", bw, 0.7))) == set(s_greedy)
    assert ev(("beam_recon", bw, 1.0, 0.0), reconstructor=rm) == ev(("beam_nbest", bw, 1.0))
    assert set(ev(("beam_recon", bw, 0.7, weight), reconstructor=rm)) == set(s_greedy)
    with pytest.raises(ValueError, match="needs a reconstructor"):
        ev(("beam_recon", bw, 0.7, weight))


# ------------------------------------------------------------------------------------------------ 4. errors
def test_library_refuses_bad_arguments_and_recovers():
    g, P, enc = load_search_case("search_small")
    dec, cfg, inp, hid = decoder_for(g, P, "f32")
    encd = enc.cuda()
    B, F, V = enc.shape[0], enc.shape[1], int(g["meta_dims"][3])
    eng = Engine(dec.dims(B, F), None, "f32", dec.hyper(), device=encd.device)
    with pytest.raises(_lib.RecNetError, match="decoder not bound"):
        eng.beam_search_nbest(encd, 3, 0.7)
    eng.bind_decoder({k: v.data for k, v in dec.named_tensors().items()})
    eng.pack_weights()
    good = eng.beam_search_nbest(encd, 3, 0.7)
    for bw in (0, 9, -1):
        with pytest.raises(_lib.RecNetError, match="beam_width"):
            eng.beam_search_nbest(encd, bw, 0.7)
    for alpha in (-0.5, float("nan"), float("inf")):
        with pytest.raises(_lib.RecNetError, match="length_alpha"):
            eng.beam_search_nbest(encd, 3, alpha)
    x, cum, fin = (torch.from_numpy(a).cuda() for a in BR.row_case(8, 3, "continuous"))
    x4 = x[:, :, :4].contiguous()
    with pytest.raises(_lib.RecNetError, match="beam_width"):
        eng.beam_select_rows(x4, cum, fin, 5)              # wider than V
    with pytest.raises(_lib.RecNetError, match="beam_width"):
        eng.beam_select_rows(x, cum, fin, 0)
    with pytest.raises(RuntimeError):
        eng.beam_select_rows(x, cum, fin.long(), 3)
    with pytest.raises(RuntimeError):
        eng.beam_select_rows(x, cum[:2].contiguous(), fin, 3)
    # a vocabulary smaller than the width, through the search
    small = Engine(dict(B=2, F=2, D=8, E=4, H=8, A=4, V=5), None, "f32")
    ops = _ops.load()
    with pytest.raises(RuntimeError, match="beam_width"):
        ops.beam_search_nbest(int(small.handle.value), torch.zeros(2, 2, 8, device="cuda"), 6, 0.0)
    with pytest.raises(RuntimeError):
        ops.beam_select_rows(int(eng.handle.value), x, cum, fin, 9)
    # the Python layer: the start state and the arguments, before an engine is asked for
    with pytest.raises(NotImplementedError):
        R.beam_search_nbest(cfg, dec, inp * 3, hid, encd, 3)
    h1 = (hid[0] + 1, hid[1]) if isinstance(hid, tuple) else hid + 1
    with pytest.raises(NotImplementedError):
        R.beam_search_nbest(cfg, dec, inp, h1, encd, 3)
    for kw in (dict(beam_width=0), dict(beam_width=9), dict(beam_width=V + 1), dict(beam_width=3, length_alpha=-1.0)):
        with pytest.raises(ValueError):
            R.beam_search_nbest(cfg, dec, inp, hid, encd, **kw)
    again = eng.beam_search_nbest(encd, 3, 0.7)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(good, again))
