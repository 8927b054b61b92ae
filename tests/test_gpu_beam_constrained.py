"""The constrained N-best beam search on the device (recnet_beam_select_rows_constrained / recnet_beam_search_nbest_constrained;
DESIGN.md section 12) against the CPU restatement (tests/beam_constrained_ref.py): the selection kernel alone on host-made inputs
whose banned tokens hold the largest logits, the search on the goldens' decoders over the run table, what the device returns
checked on its own in both precisions (no violation, score_captions reproduces cum and len, canonical ranks, equal bits on a
repeat), the constraints switched off against the unconstrained entries bit for bit, the public layer and the argument checks.

As in tests/test_gpu_beam.py: indices / tokens are compared outside the decisions the restatement marks as near-ties (margin below
1e-3 among the offered candidates; tests/test_beam_constrained_ref.py holds the caps on how many those may be); a candidate is held
to score_ref.row_bar at temperature 1 plus two units in the last place of |cum|, a hypothesis' cum to its length times the row
bar.  Every test prints its worst error / bar."""
import functools

import numpy as np
import pytest
import torch

import recnet_amd as R
from recnet_amd import _ops, search
from tests import beam_constrained_ref as CR
from tests import beam_ref as BR
from tests import golden_util as GU
from tests import score_ref as SC
from tests.golden_util import load_search_case
from tests.gpu_util import make_models
from tests.sample_ref import NEAR_TIE
from tests.search_kit import Cfg, decoder_for, rows_engine

pytestmark = pytest.mark.gpu

Engine, _lib = R.engine.Engine, R.engine._lib


# ------------------------------------------------------------------------------------------------ 1. the selection kernel alone
def _run_case(c, bws):
    """One kernel-alone case on the device (two calls per width) next to the restatement; returns the worst error / bar."""
    eng = rows_engine()
    x, cum, fin, hist = c["x"], c["cum"], c["fin"], c["hist"]
    nb, rows, V = x.shape
    t, n, m, banned = c["t"], c["n"], c["m"], c["banned"]
    xd, cd, fd, hd = (torch.from_numpy(a).cuda() for a in (x, cum, fin, hist))
    before = xd.clone()
    ref = CR.select_rows_widths(x, cum, fin, bws, hist, t, n, m, banned)
    sets = [[CR.banned_ids(hist[i, r], t, n, m, banned) if fin[i, r] == 0 else set() for r in range(rows)] for i in range(nb)]
    live = fin == 0
    amax = np.abs(x[live]).max() if live.any() else 0.0
    bar = SC.row_bar("f32", amax, 1.0) + 2 * float(np.spacing(np.float32(np.abs(cum).max())))
    worst = 0.0
    for bw in bws:
        kw = dict(hist=hd, t=t, no_repeat_ngram=n, min_length=m, banned_tokens=banned)
        vals, idx = eng.beam_select_rows(xd, cd, fd, bw, **kw)
        vals2, idx2 = eng.beam_select_rows(xd, cd, fd, bw, **kw)
        torch.cuda.synchronize()
        assert torch.equal(vals.view(torch.int32), vals2.view(torch.int32)) and torch.equal(idx, idx2), c["case"]
        assert torch.equal(xd.view(torch.int32), before.view(torch.int32)), c["case"]
        vals32, idx = vals.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
        vals = vals32.astype(np.float64)
        rv, ri, margin = ref[bw]
        assert ((idx >= 0) & (idx < nb * V)).all(), c["case"]
        keep = margin >= NEAR_TIE
        assert np.array_equal(idx[keep], ri[keep]), (c["case"], bw, idx, ri)
        src, tok = idx // V, idx % V
        inf = np.isneginf(rv)
        assert np.array_equal(np.isneginf(vals), inf), c["case"]
        for r in range(rows):
            for k in range(bw):
                if inf[r, k]:
                    continue
                i = src[r, k]
                if fin[i, r]:                    # a finished hypothesis: <PAD> at cum, to the bit, whatever its history bans
                    assert tok[r, k] == BR.PAD and vals32[r, k] == cum[i, r], (c["case"], r, k)
                else:                            # a banned token is never selected, near-tie or not
                    assert tok[r, k] not in sets[i][r], (c["case"], r, k, tok[r, k])
        if c["tie"]:                             # equal logits and cum, different histories: only the twin offers what beam 0 bans
            for r in range(rows):
                got = {(int(a), int(b)) for a, b in zip(src[r], tok[r])}
                for v in sets[0][r] - sets[nb - 1][r]:
                    assert (0, v) not in got, (c["case"], r, v)
                    if bw == 8:
                        assert (nb - 1, v) in got, (c["case"], r, v)
        err = np.abs(vals[~inf] - rv[~inf])
        if err.size:
            worst = max(worst, float(err.max() / bar))
            assert err.max() <= bar, (c["case"], bw, float(err.max()), bar)
        # the constraints off: the unconstrained entry's bits
        if c.get("off", False):
            v0, i0 = eng.beam_select_rows(xd, cd, fd, bw)
            v1, i1 = eng.beam_select_rows(xd, cd, fd, bw, hist=hd, t=t)
            v2, i2 = eng.beam_select_rows(xd, cd, fd, bw, t=t)
            assert torch.equal(v0.view(torch.int32), v1.view(torch.int32)) and torch.equal(i0, i1), c["case"]
            assert torch.equal(v0.view(torch.int32), v2.view(torch.int32)) and torch.equal(i0, i2), c["case"]
    return worst


@pytest.mark.parametrize("V", CR.ROW_VS)
def test_select_rows_constrained(V):
    worst, count = 0.0, 0
    for nb in CR.ROW_NB:
        cases = CR.row_cases(V, nb) + CR.min_length_cases(V, nb) + CR.residue_cases(V, nb) + [CR.static_ban_case(V, nb)]
        cases[0]["off"] = cases[-1]["off"] = True
        for c in cases:
            worst = max(worst, _run_case(c, CR.ROW_BW))
            count += 1
    print("V", V, "cases", count, "worst candidate error / bar:", worst)


def test_select_rows_constrained_long_rows():
    """V = 12500 (the row is read from global memory three times), 8 hypotheses, width 8, the last step of a 31-step caption."""
    worst = 0.0
    for n in CR.ROW_N:
        c = CR.ban_case(12500, 8, n, 30, "random4", "continuous", m=0, banned=(7, 9) if n == 2 else (), Tm=31)
        worst = max(worst, _run_case(c, (8,)))
    for c in CR.residue_cases(12500, 8, t=30, Tm=31):
        worst = max(worst, _run_case(c, (8,)))
    c = CR.ban_case(12500, 8, 0, 3, "random4", "continuous", Tm=31)
    c["x"][:, :, BR.EOS] = c["x"].max(axis=2) + 2.0
    c["m"] = 30
    worst = max(worst, _run_case(c, (8,)))
    print("V 12500 worst candidate error / bar:", worst)


# ------------------------------------------------------------------------------------------------ 2. the search
@functools.lru_cache(maxsize=None)
def _ref(name, bw, cml, n, m, banned):
    g, P, enc = load_search_case(name)
    return CR.beam_search_nbest(P, enc, bw, BR.LENGTH_ALPHA, cml, g["_cell"], n, m, banned)


def _kw(run):
    return dict(no_repeat_ngram=run["n"], min_length=run["m"], banned_tokens=run["banned"])


@pytest.mark.parametrize("run", CR.RUNS, ids=CR.run_id)
def test_search_matches_the_restatement(run):
    """fp32, as tests/test_gpu_beam.py compares the unconstrained search: captions without a near-tie decision in full (n_steps when no
    caption is excluded, tokens, len, rank order, cum within len x the row bar), the others up to their first near-tie decision."""
    name, bw, cml = run["name"], run["bw"], run["cml"]
    g, P, enc = load_search_case(name)
    r = _ref(name, bw, cml, run["n"], run["m"], run["banned"])
    dec, cfg, inp, hid = decoder_for(g, P, "f32", cml)
    toks, cum, ln, score = search._beam_nbest(cfg, dec, inp, hid, enc.cuda(), bw, BR.LENGTH_ALPHA, **_kw(run))
    toks, cum, ln, score = toks.cpu().numpy(), cum.cpu().numpy().astype(np.float64), ln.cpu().numpy(), score.cpu().numpy().astype(np.float64)
    keep = CR.comparable_captions(r)
    n = toks.shape[1]
    assert toks.shape == (bw, n, enc.shape[0]) and 1 <= n <= cml + 1
    if keep.all():
        assert n == r["n_steps"]
    m = min(n, r["n_steps"])
    assert np.array_equal(ln[:, keep], r["len"][:, keep])
    assert np.array_equal(toks[:, :m][:, :, keep], r["tokens"][:, :m][:, :, keep])
    assert (toks[:, m:][:, :, keep] == 0).all() and (r["tokens"][:, m:][:, :, keep] == 0).all()
    bar = r["len"] * SC.row_bar("f32", r["amax"].max(), 1.0)
    err = np.abs(cum - r["cum"])[:, keep]
    errs = np.abs(score - r["score"])[:, keep]
    worst = float((err / bar[:, keep]).max()) if err.size else 0.0
    print(CR.run_id(run), "steps", n, "captions compared", int(keep.sum()), "of", keep.size, "worst cum error / bar:", worst)
    assert (err <= bar[:, keep]).all() and (errs <= bar[:, keep]).all()
    t0 = CR.comparable_steps(r["margins"]).sum(axis=0)
    prefixes = 0
    for b in np.nonzero(~keep)[0]:
        k = int(t0[b])
        if k == 0:
            continue
        allowed = {tuple(h) for h in r["trace"][k - 1][3][:, b, :k].tolist()}
        for rank in range(bw):
            got = toks[rank, :k, b].tolist()
            got += [0] * (k - len(got))
            assert tuple(got) in allowed, (b, rank, k, got, allowed)
        prefixes += k
    print(CR.run_id(run), "decisions compared through excluded captions' prefixes:", prefixes)
    assert keep.any() or prefixes > 0
    # the public list form of the same call
    hyps = R.beam_search_nbest(cfg, dec, inp, hid, enc.cuda(), bw, BR.LENGTH_ALPHA, **_kw(run))
    assert len(hyps) == enc.shape[0] and all(len(h) == bw for h in hyps)
    for b, h in enumerate(hyps):
        for k, (t, c, l, s) in enumerate(h):
            assert l == ln[k, b] and t == toks[k, :l, b].tolist() and c == float(cum[k, b]) and s == float(score[k, b])


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("run", CR.RUNS, ids=CR.run_id)
def test_what_the_device_returns(run, prec):
    """Independent of the restatement's decisions: no returned hypothesis violates a constraint; score_captions on every returned
    rank gives its len exactly and its cum within len x the row bar of the precision (no renormalisation; in fp32 the same bits are
    expected and counted); ranks are canonical and ordered; a repeat returns equal bits.  Width 1 with the constraints on is the
    restatement's width-1 search up to each caption's first decision that the precision could flip (beam_constrained_ref.width1_steps:
    at width 1 every candidate of a step shares cum, so a decision flips only if two log-probabilities closer than twice the row bar
    swap).  In fp32 every run compares decisions; in bf16 the guard is wide and a single run may compare none:
    tests/test_beam_constrained_ref.py::test_width_one_guard_leaves_decisions_to_compare holds the floor over the runs, which
    depends on the restatement alone."""
    name, bw, cml, n, m, banned = run["name"], run["bw"], run["cml"], run["n"], run["m"], run["banned"]
    g, P, enc = load_search_case(name)
    dec, cfg, inp, hid = decoder_for(g, P, prec, cml)
    encd = enc.cuda()
    amax = _ref(name, bw, cml, n, m, banned)["amax"].max()
    a = search._beam_nbest(cfg, dec, inp, hid, encd, bw, BR.LENGTH_ALPHA, **_kw(run))
    b2 = search._beam_nbest(cfg, dec, inp, hid, encd, bw, BR.LENGTH_ALPHA, **_kw(run))
    assert all(torch.equal(x, y) for x, y in zip(a, b2))
    toks, cum, ln, score = a
    assert CR.violations(toks.cpu().numpy(), ln.cpu().numpy(), n, m, banned) == (0, 0, 0)
    assert (score[:-1] >= score[1:]).all() and bool(torch.isfinite(cum).all())
    worst, other_bits = 0.0, 0
    for k in range(bw):
        assert torch.equal(R.canonical_captions(toks[k]), toks[k])
        _, cap, sl = search._score(dec, encd, toks[k].contiguous(), 1.0, False)
        assert torch.equal(sl.cpu(), ln[k].cpu()), (k, sl, ln[k])
        bar = ln[k].cpu().numpy() * SC.row_bar(prec, amax, 1.0)
        err = np.abs(cap.cpu().numpy().astype(np.float64) - cum[k].cpu().numpy())
        worst = max(worst, float((err / bar).max()))
        other_bits += int((cap.view(torch.int32) != cum[k].view(torch.int32)).sum())
        assert (err <= bar).all(), (k, err, bar)
    print(CR.run_id(run), prec, "worst |score_captions - cum| / (len x row bar):", worst, "hypotheses whose bits differ:", other_bits)
    # width 1
    r1 = _ref(name, 1, cml, n, m, banned)
    t1, c1, l1, _ = search._beam_nbest(cfg, dec, inp, hid, encd, 1, BR.LENGTH_ALPHA, **_kw(run))
    t1, l1 = t1.cpu().numpy()[0], l1.cpu().numpy()[0]
    assert CR.violations(t1[None], l1[None], n, m, banned) == (0, 0, 0)
    upto = CR.width1_steps(r1, prec)              # decisions before the first one that the precision could flip
    compared = 0
    for b in range(enc.shape[0]):
        k = min(int(upto[b]), t1.shape[0])
        assert np.array_equal(t1[:k, b], r1["tokens"][0, :k, b]), (b, k, t1[:, b], r1["tokens"][0, :, b])
        compared += k
        if int(upto[b]) == r1["n_steps"] and (r1["tokens"][0, :, b] == BR.EOS).any():    # (without an <EOS>, len is the run's n_steps)
            assert l1[b] == r1["len"][0, b]
    print(CR.run_id(run), prec, "width 1: decisions compared", compared, "of", r1["margins"].size)
    assert prec != "f32" or compared > 0


@pytest.mark.parametrize("bw", [1, 3, 8])
def test_constraints_off_is_the_unconstrained_search(bw):
    g, P, enc = load_search_case("search_gru")
    dec, cfg, inp, hid = decoder_for(g, P, "f32", 7)
    eng = search._nbest_engine(cfg, dec, enc.cuda())
    ops = _ops.load()
    a = ops.beam_search_nbest(int(eng.handle.value), enc.cuda(), bw, 0.7)
    b = ops.beam_search_nbest_constrained(int(eng.handle.value), enc.cuda(), bw, 0.7, 0, 0, [])
    c = eng.beam_search_nbest(enc.cuda(), bw, 0.7)
    d = eng.beam_search_nbest(enc.cuda(), bw, 0.7, no_repeat_ngram=2)
    torch.cuda.synchronize()
    assert len(a) == len(b) == 5
    for x, y, z in zip(a, b, c):
        assert x.dtype == y.dtype and torch.equal(x, y) and torch.equal(x, z)
    if bw > 1:                                   # (a constraint that binds on this golden at these widths changes the tokens)
        assert not torch.equal(a[0], d[0])


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
    con = dict(no_repeat_ngram=2, min_length=3, banned_tokens=(5, 7))
    free = R.beam_search_nbest(Cfg, dm, inp, hid, encd, bw, 1.0)
    hyps = R.beam_search_nbest(Cfg, dm, inp, hid, encd, bw, 1.0, **con)
    print(kind, "captions whose hypotheses the constraints changed:", sum(a != b for a, b in zip(hyps, free)), "of", B)
    for h in hyps:
        for t, c, l, s in h:
            assert CR.violations(np.array(t)[None, :, None], np.array([[l]]), 2, 3, (5, 7)) == (0, 0, 0)
    # without the term at length_alpha = 1 the search's own order is pick_best_of_n's: rank 0
    caps, ks, scores = R.best_of_beam(Cfg, dm, inp, hid, encd, bw, 1.0, **con)
    assert ks == [0] * B and caps == [h[0][0] for h in hyps]
    assert R.best_of_beam(Cfg, dm, inp, hid, encd, bw, 1.0, reconstructor=rm, recon_weight=0.0, **con) == (caps, ks, scores)
    # with the term: pick_best_of_n on the public reconstruction errors of the returned ranks at the common T = n_steps
    toks, cum, ln, _ = search._beam_nbest(Cfg, dm, inp, hid, encd, bw, 0.7, **con)
    n = toks.shape[1]
    errs = [R.reconstruction_errors(Cfg, dm, rm, encd, toks[k].contiguous(), T=n) for k in range(bw)]
    rk, rs = R.pick_best_of_n(cum.cpu().tolist(), ln.cpu().tolist(), errs, weight)
    caps_w, ks_w, scores_w = R.best_of_beam(Cfg, dm, inp, hid, encd, bw, 0.7, reconstructor=rm, recon_weight=weight, **con)
    assert ks_w == rk and scores_w == rs
    lens, tl = ln.cpu().tolist(), toks.cpu().tolist()
    for b in range(B):
        assert caps_w[b] == [tl[ks_w[b]][t][b] for t in range(lens[ks_w[b]][b])]
    print(kind, "constrained best of beam", bw, ": ranks chosen with the reconstruction term", ks_w)
    # evaluate: both forms with the trailing dict
    idx2word = {i: "w%d" % i for i in range(V)}
    names = ["a", "b", "c", "d", "PAD", "PAD"]
    refs = {k: ["w3 w4 w5", "w7 w8"] for k in "abcd"}
    ev = lambda method, **kw: R.evaluate(Cfg, [(names, enc.numpy())], dm, method, idx2word, refs, **kw)
    s_free = ev(("beam_nbest", bw, 0.7))
    assert set(ev(("beam_nbest", bw, 0.7, con))) == set(s_free)
    assert ev(("beam_nbest", bw, 0.7, {})) == s_free
    assert ev(("beam_recon", bw, 1.0, 0.0, con), reconstructor=rm) == ev(("beam_nbest", bw, 1.0, con))
    assert set(ev(("beam_recon", bw, 0.7, weight, con), reconstructor=rm)) == set(s_free)
    with pytest.raises(ValueError, match="needs a reconstructor"):
        ev(("beam_recon", bw, 0.7, weight, con))
    with pytest.raises(ValueError, match="unknown constraint"):
        ev(("beam_nbest", bw, 0.7, dict(min_len=2)))


# ------------------------------------------------------------------------------------------------ 4. errors
def test_library_refuses_bad_arguments_and_recovers():
    g, P, enc = load_search_case("search_small")
    dec, cfg, inp, hid = decoder_for(g, P, "f32", 7)
    encd = enc.cuda()
    B, F, V = enc.shape[0], enc.shape[1], int(g["meta_dims"][3])
    hy = dec.hyper()
    hy.update(caption_max_len=7)
    eng = Engine(dec.dims(B, F), None, "f32", hy, device=encd.device)
    with pytest.raises(_lib.RecNetError, match="decoder not bound"):
        eng.beam_search_nbest(encd, 3, 0.7, no_repeat_ngram=2)
    eng.bind_decoder({k: v.data for k, v in dec.named_tensors().items()})
    eng.pack_weights()
    good = eng.beam_search_nbest(encd, 3, 0.7, no_repeat_ngram=2, min_length=2, banned_tokens=(5,))
    for kw, what in ((dict(no_repeat_ngram=-1), "no_repeat_ngram"), (dict(no_repeat_ngram=8), "no_repeat_ngram"),
                     (dict(min_length=-1), "min_length"), (dict(min_length=8), "min_length"),
                     (dict(banned_tokens=(5, 5)), "distinct"), (dict(banned_tokens=(2,)), "EOS"), (dict(banned_tokens=(V,)), r"\[0, V\)"),
                     (dict(banned_tokens=(-1,)), r"\[0, V\)"), (dict(banned_tokens=tuple(range(3, 20))), "n_banned")):
        with pytest.raises(_lib.RecNetError, match=what):
            eng.beam_search_nbest(encd, 3, 0.7, **kw)
    with pytest.raises(_lib.RecNetError, match="beam_width"):
        eng.beam_search_nbest(encd, 9, 0.7, min_length=1)
    with pytest.raises(_lib.RecNetError, match="length_alpha"):
        eng.beam_search_nbest(encd, 3, -0.5, min_length=1)
    # the kernel-alone entry
    c = CR.ban_case(61, 3, 2, 3, "random4")
    x, cum, fin, hist = (torch.from_numpy(c[k]).cuda() for k in ("x", "cum", "fin", "hist"))
    with pytest.raises(_lib.RecNetError, match="t in"):
        eng.beam_select_rows(x, cum, fin, 3, hist=hist, t=8, no_repeat_ngram=2)
    with pytest.raises(_lib.RecNetError, match="t in"):
        eng.beam_select_rows(x, cum, fin, 3, hist=hist, t=-1, no_repeat_ngram=2)
    with pytest.raises(_lib.RecNetError, match="null argument"):
        eng.beam_select_rows(x, cum, fin, 3, t=3, no_repeat_ngram=2)                       # an n-gram rule without a history
    with pytest.raises(_lib.RecNetError, match="no_repeat_ngram"):
        eng.beam_select_rows(x, cum, fin, 3, hist=hist, t=3, no_repeat_ngram=8)
    with pytest.raises(_lib.RecNetError, match="beam_width"):
        eng.beam_select_rows(x, cum, fin, 0, hist=hist, t=3, no_repeat_ngram=2)
    with pytest.raises(RuntimeError):
        eng.beam_select_rows(x, cum, fin, 3, hist=hist.int(), t=3, no_repeat_ngram=2)
    with pytest.raises(RuntimeError):
        eng.beam_select_rows(x, cum, fin, 3, hist=hist[:2].contiguous(), t=3, no_repeat_ngram=2)
    with pytest.raises(RuntimeError, match="needs the step"):
        eng.beam_select_rows(x, cum, fin, 3, hist=hist, no_repeat_ngram=2)
    # an infeasible vocabulary: beam_width + n_banned + t + 1 <= V for the kernel alone ...
    x20 = x[:, :, :20].contiguous()
    eng.beam_select_rows(x20, cum, fin, 8, hist=hist, t=7, no_repeat_ngram=2, banned_tokens=(3, 4, 5, 6))       # 8 + 4 + 7 + 1 = 20
    with pytest.raises(_lib.RecNetError, match="too small"):
        eng.beam_select_rows(x20, cum, fin, 8, hist=hist, t=7, no_repeat_ngram=2, banned_tokens=(3, 4, 5, 6, 7))
    eng.beam_select_rows(x20, cum, fin, 8)                                                                           # (unconstrained: 8 <= V)
    # ... and beam_width + n_banned + caption_max_len + 1 <= V for the search, in the library and in the custom op
    torch.manual_seed(3)
    dec12 = R.Decoder("LSTM", 1, 8, 4, 1, 8, 4, 12, 0.5, 0.5, 0.5, precision="f32").cuda().eval()
    cfg12 = Cfg()
    cfg12.batch_size, cfg12.decoder_model, cfg12.caption_max_len = 2, "LSTM", 7
    enc12 = torch.randn(2, 2, 8, device="cuda")
    small = search._nbest_engine(cfg12, dec12, enc12)
    ops = _ops.load()
    with pytest.raises(_lib.RecNetError, match="too small"):
        small.beam_search_nbest(enc12, 5, 0.0, min_length=1)                              # 5 + 0 + 7 + 1 > 12
    with pytest.raises(RuntimeError, match="too small"):
        ops.beam_search_nbest_constrained(int(small.handle.value), enc12, 5, 0.0, 0, 1, [])
    t12, _, l12, _, _ = small.beam_search_nbest(enc12, 4, 0.0, no_repeat_ngram=1, min_length=7)    # 4 + 0 + 7 + 1 = 12: it runs
    assert CR.violations(t12.cpu().numpy(), l12.cpu().numpy(), 1, 7, ()) == (0, 0, 0)
    small.beam_search_nbest(enc12, 8, 0.0)                                                # (unconstrained: 8 <= min(8, V))
    with pytest.raises(RuntimeError, match="at most 16"):
        ops.beam_search_nbest_constrained(int(eng.handle.value), encd, 3, 0.0, 0, 0, list(range(3, 20)))
    with pytest.raises(RuntimeError, match="distinct"):
        ops.beam_select_rows_constrained(int(eng.handle.value), x, cum, fin, hist, 3, 3, 2, 0, [5, 5])
    with pytest.raises(RuntimeError):
        ops.beam_select_rows_constrained(int(eng.handle.value), x, cum, fin, hist.int(), 3, 3, 2, 0, [])
    v_ops, i_ops = ops.beam_select_rows_constrained(int(eng.handle.value), x, cum, fin, hist, 3, 3, 2, 0, [])
    v_eng, i_eng = eng.beam_select_rows(x, cum, fin, 3, hist=hist, t=3, no_repeat_ngram=2)
    assert torch.equal(v_ops, v_eng) and torch.equal(i_ops, i_eng)
    # the Python layer refuses before an engine is asked for
    for kw in (dict(no_repeat_ngram=8), dict(min_length=-1), dict(banned_tokens=(2,)), dict(banned_tokens=(5, 5)), dict(banned_tokens=(V,))):
        with pytest.raises(ValueError):
            R.beam_search_nbest(cfg, dec, inp, hid, encd, 3, **kw)
    with pytest.raises(ValueError, match="too small"):
        R.beam_search_nbest(_tight(cfg, V), dec, inp, hid, encd, 8, no_repeat_ngram=2)
    with pytest.raises(ValueError, match="too small"):
        R.best_of_beam(_tight(cfg, V), dec, inp, hid, encd, 8, min_length=1)
    again = eng.beam_search_nbest(encd, 3, 0.7, no_repeat_ngram=2, min_length=2, banned_tokens=(5,))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(good, again))


def _tight(cfg, V):
    """The config with a caption_max_len that leaves no room for a width-8 constrained search in a vocabulary of V."""
    c = Cfg()
    c.batch_size, c.decoder_model, c.caption_max_len = cfg.batch_size, cfg.decoder_model, V - 8
    return c
