"""The diverse (group) N-best beam search on the device (recnet_beam_select_rows_diverse / recnet_beam_search_nbest_diverse; DESIGN.md
section 14) against the CPU restatement (tests/beam_diverse_ref.py): the grouped selection kernel alone on host-made inputs, the
fp32 search on the goldens' decoders, the exact properties in both precisions (one group is the existing search, lambda = 0 gives
copies of the plain search at the group width, group 0 always is that search), the reranking, evaluate(), and the argument checks
of every layer.

Indices / tokens are compared outside the decisions the restatement marks as near-ties (margin below 1e-3; tests/
test_beam_diverse_ref.py holds the cap of 0.6 on the compared share without a GPU).  Values are held to section 11's bar: the row
bar of score_ref plus two units in the last place of |cum|; a hypothesis' cum to its length times the row bar.  Every test prints
its worst error / bar."""
import numpy as np
import pytest
import torch

import recnet_amd as R
from recnet_amd import _ops, search
from tests import beam_diverse_ref as DR
from tests import beam_ref as BR
from tests import golden_util as GU
from tests import score_ref as SC
from tests.golden_util import load_search_case
from tests.gpu_util import make_models
from tests.sample_ref import NEAR_TIE
from tests.search_kit import decoder_for, rows_engine

pytestmark = pytest.mark.gpu

Engine, _lib = R.engine.Engine, R.engine._lib


# ------------------------------------------------------------------------------------------------ 1. the selection kernel alone
def _dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


@pytest.mark.parametrize("V", DR.ROW_VS)
def test_select_rows_groups(V):
    eng = rows_engine()
    worst, cases, compared, labels = 0.0, 0, 0, set()
    for bw, G in DR.ROW_BW_G:
        if bw > V:
            continue
        w = bw // G
        for nb in (1, bw):
            for c in DR.group_cases(V, bw, G, nb):
                if (c["n"] or c["m"] or c["banned"]) and bw + len(c["banned"]) + c["t"] + 1 > V:
                    continue
                tag = (V, bw, G, nb, c["label"])
                xd, cd, fd, hd = _dev(c["x"]), _dev(c["cum"]), _dev(c["fin"]), _dev(c["hist"])
                before = xd.clone()
                kw = dict(hist=hd, t=c["t"], no_repeat_ngram=c["n"], min_length=c["m"], banned_tokens=c["banned"])
                vals, idx = eng.beam_select_rows_diverse(xd, cd, fd, bw, G, c["lam"], **kw)
                vals2, idx2 = eng.beam_select_rows_diverse(xd, cd, fd, bw, G, c["lam"], **kw)
                # group 0 is the existing kernel at width w on the group's own hypotheses, bit for bit
                k0 = 1 if nb == 1 else w
                if c["n"] or c["m"] or c["banned"]:
                    pv, pi = eng.beam_select_rows(xd[:k0].contiguous(), cd[:k0].contiguous(), fd[:k0].contiguous(), w,
                                                  hist=None if hd is None else hd[:k0].contiguous(), t=c["t"], no_repeat_ngram=c["n"],
                                                  min_length=c["m"], banned_tokens=c["banned"])
                else:
                    pv, pi = eng.beam_select_rows(xd[:k0].contiguous(), cd[:k0].contiguous(), fd[:k0].contiguous(), w)
                torch.cuda.synchronize()
                assert torch.equal(vals.view(torch.int32), vals2.view(torch.int32)) and torch.equal(idx, idx2), tag
                assert torch.equal(xd.view(torch.int32), before.view(torch.int32)), tag
                assert torch.equal(vals[:, :w].contiguous().view(torch.int32), pv.view(torch.int32)) and torch.equal(idx[:, :w], pi), tag
                rv, ri, margin, _ = DR.select_rows_groups(c["x"], c["cum"], c["fin"], bw, G, c["lam"], c["hist"], c["t"], c["n"], c["m"],
                                                          c["banned"])
                idx, vals = idx.cpu().numpy().astype(np.int64), vals.cpu().numpy().astype(np.float64)
                assert ((idx >= 0) & (idx < nb * V)).all(), tag
                keep = margin >= NEAR_TIE
                assert np.array_equal(idx[keep], ri[keep]), (tag, idx, ri)
                if c["label"] == "all_finished_ascending":              # <PAD> at cum, to the bit; then -inf by index
                    assert np.array_equal(idx, ri) and np.array_equal(vals, rv), tag
                inf = np.isneginf(rv)
                assert np.array_equal(np.isneginf(vals[keep]), inf[keep]), tag
                live = c["fin"] == 0
                amax = np.abs(c["x"][live]).max() if live.any() else 0.0
                bar = SC.row_bar("f32", amax, 1.0) + 2 * float(np.spacing(np.float32(np.abs(c["cum"]).max())))
                ok = keep[:, None] & ~inf
                err = np.abs(vals[ok] - rv[ok])
                if err.size:
                    worst = max(worst, float(err.max() / bar))
                    assert err.max() <= bar, (tag, float(err.max()), bar)
                cases += 1; compared += int(keep.sum()); labels.add(c["label"])
    print("V", V, "cases", cases, "rows compared", compared, "of", 5 * cases, "kinds", sorted(labels), "worst candidate error / bar:", worst)
    assert compared > 0.6 * 5 * cases


# ------------------------------------------------------------------------------------------------ 2. the search
@pytest.mark.parametrize("run", DR.RUNS, ids=DR.run_id)
def test_search_matches_the_restatement(run):
    """fp32 path: n_steps (when no caption is excluded), tokens, len, the rank order and the group of every rank equal the
    restatement on the captions without any near-tie decision; cum within len x the row bar.  A caption with a near-tie is compared
    up to that decision: the first t0 tokens of each of its returned hypotheses against the restatement's beams of its group."""
    name, bw, G, lam, cml, n_, m_, banned = (run[k] for k in ("name", "bw", "G", "lam", "cml", "n", "m", "banned"))
    w = bw // G
    g, P, enc = load_search_case(name)
    r = DR.beam_search_nbest(P, enc, bw, G, lam, BR.LENGTH_ALPHA, cml, g["_cell"], n_, m_, banned)
    dec, cfg, inp, hid = decoder_for(g, P, "f32", cml)
    kw = dict(no_repeat_ngram=n_, min_length=m_, banned_tokens=banned, n_groups=G, diversity_penalty=lam)
    toks, cum, ln, score, group = search._beam_nbest(cfg, dec, inp, hid, enc.cuda(), bw, BR.LENGTH_ALPHA, want_groups=True, **kw)
    toks, cum, ln, score, group = (toks.cpu().numpy(), cum.cpu().numpy().astype(np.float64), ln.cpu().numpy(),
                                   score.cpu().numpy().astype(np.float64), group.cpu().numpy())
    keep = DR.comparable_captions(r)
    n = toks.shape[1]
    assert toks.shape == (bw, n, enc.shape[0]) and 1 <= n <= cml + 1
    assert (int(keep.sum()), keep.size) == run["full"]
    if keep.all():
        assert n == r["n_steps"]
    m = min(n, r["n_steps"])
    assert np.array_equal(ln[:, keep], r["len"][:, keep])
    assert np.array_equal(toks[:, :m][:, :, keep], r["tokens"][:, :m][:, :, keep])
    assert (toks[:, m:][:, :, keep] == 0).all() and (r["tokens"][:, m:][:, :, keep] == 0).all()
    assert np.array_equal(group[:, keep], r["group"][:, keep])
    assert all((np.bincount(group[:, b], minlength=G) == w).all() for b in range(enc.shape[0]))
    bar = r["len"] * SC.row_bar("f32", r["amax"].max(), 1.0)
    err = np.abs(cum - r["cum"])[:, keep]
    errs = np.abs(score - r["score"])[:, keep]
    worst = float((err / bar[:, keep]).max()) if err.size else 0.0
    print(DR.run_id(run), "steps", n, "captions compared", int(keep.sum()), "of", keep.size, "worst cum error / bar:", worst)
    assert (err <= bar[:, keep]).all() and (errs <= bar[:, keep]).all()
    t0 = DR.comparable_steps(r["margins"]).sum(axis=0)
    prefixes = 0
    for b in np.nonzero(~keep)[0]:
        k = int(t0[b])
        if k == 0:
            continue
        hist = r["trace"][k - 1][3]
        for rank in range(bw):
            gr = int(group[rank, b])
            allowed = {tuple(h) for h in hist[gr * w:gr * w + w, b, :k].tolist()}
            got = toks[rank, :k, b].tolist()
            got += [0] * (k - len(got))          # (a search that stopped earlier carries <PAD>)
            assert tuple(got) in allowed, (b, rank, gr, k, got, allowed)
        prefixes += k
    print(DR.run_id(run), "decisions compared through excluded captions' prefixes:", prefixes)
    assert keep.any() or prefixes > 0
    # the public list form of the same call, without and with the group
    hyps = R.beam_search_nbest(cfg, dec, inp, hid, enc.cuda(), bw, BR.LENGTH_ALPHA, **kw)
    hyps5 = R.beam_search_nbest(cfg, dec, inp, hid, enc.cuda(), bw, BR.LENGTH_ALPHA, return_groups=True, **kw)
    assert len(hyps) == enc.shape[0] and all(len(h) == bw for h in hyps)
    for b, h in enumerate(hyps):
        for k, (t, c, l, s) in enumerate(h):
            assert l == ln[k, b] and t == toks[k, :l, b].tolist() and c == float(cum[k, b]) and s == float(score[k, b])
            assert hyps5[b][k] == (t, c, l, s, int(group[k, b]))
    lists = [[h[0] for h in hb] for hb in hyps]
    assert R.nbest_diversity(hyps) == DR.nbest_diversity(lists) == R.nbest_diversity(hyps5)


def _by_group(x, group, g):
    """The ranks of group g, in rank order, of x [bw, ..., B] -> [w, ..., B]."""
    B = group.shape[1]
    return torch.stack([x[..., b][group[:, b] == g] for b in range(B)], dim=-1)


@pytest.mark.parametrize("name", ["search_small", "search_gru"])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_exact_properties(name, prec):
    """One group is the existing search bit for bit, through the new entry; lambda = 0 gives G copies of the width-w search and
    lambda > 0 leaves group 0 that search, bit for bit in tokens and cum; score_captions reproduces cum on every rank."""
    g, P, enc = load_search_case(name)
    dec, cfg, inp, hid = decoder_for(g, P, prec)
    encd = enc.cuda()
    eng = search._nbest_engine(cfg, dec, encd)
    ops, h = _ops.load(), int(eng.handle.value)
    for bw in (3, 8):
        plain = ops.beam_search_nbest(h, encd, bw, 0.7)
        one = ops.beam_search_nbest_diverse(h, encd, bw, 0.7, 1, 2.5, 0, 0, [])
        assert all(torch.equal(a, b) for a, b in zip(plain[:4], one[:4])) and torch.equal(plain[4], one[5]) and (one[4] == 0).all()
        con = ops.beam_search_nbest_constrained(h, encd, bw, 0.7, 2, 2, [5])
        one = ops.beam_search_nbest_diverse(h, encd, bw, 0.7, 1, 2.5, 2, 2, [5])
        assert all(torch.equal(a, b) for a, b in zip(con[:4], one[:4])) and torch.equal(con[4], one[5])
        assert all(torch.equal(a, b) for a, b in zip(one, eng.beam_search_nbest_diverse(encd, bw, 0.7, 1, 2.5, 2, 2, (5,))))
    amax = BR.beam_search_nbest(P, enc, 3, 0.7, 30, g["_cell"])["amax"].max()
    worst = 0.0
    for bw, G in ((4, 2), (6, 3), (8, 2), (8, 8)):
        w = bw // G
        pt, pc, pl, ps, pn = ops.beam_search_nbest(h, encd, w, 0.7)
        for lam in (0.0, 0.5, 1e4):
            a = ops.beam_search_nbest_diverse(h, encd, bw, 0.7, G, lam, 0, 0, [])
            b2 = ops.beam_search_nbest_diverse(h, encd, bw, 0.7, G, lam, 0, 0, [])
            assert all(torch.equal(x, y) for x, y in zip(a, b2))
            toks, cum, ln, score, group, n = a
            assert (score[:-1] >= score[1:]).all()
            n, np_ = int(n.item()), int(pn.item())
            assert n >= np_
            for gr in range(G if lam == 0.0 else 1):
                gt, gc, gl = _by_group(toks, group, gr), _by_group(cum, group, gr), _by_group(ln, group, gr)
                assert torch.equal(gc.view(torch.int32), pc.view(torch.int32)), (bw, G, lam, gr)
                # (len too: a plain search that stopped before the last step left no hypothesis without <EOS>)
                assert torch.equal(gt, pt) and torch.equal(gl, pl)
            if lam == 0.0:
                assert n == np_
            for k in range(bw):
                assert torch.equal(R.canonical_captions(toks[k]), toks[k])
                _, cap, sl = search._score(dec, encd, toks[k].contiguous(), 1.0, False)
                assert torch.equal(sl.cpu(), ln[k].cpu()), (k, sl, ln[k])
                bar = ln[k].cpu().numpy() * SC.row_bar(prec, amax, 1.0)
                err = np.abs(cap.cpu().numpy().astype(np.float64) - cum[k].cpu().numpy())
                worst = max(worst, float((err / bar).max()))
                assert (err <= bar).all(), (bw, G, lam, k, err, bar)
    print(name, prec, "worst |score_captions - cum| / (len x row bar):", worst)


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
    div = dict(n_groups=2, diversity_penalty=1.0)
    # the defaults are the call without the keywords
    assert R.beam_search_nbest(Cfg, dm, inp, hid, encd, bw, 0.7, n_groups=1, diversity_penalty=3.0) == R.beam_search_nbest(Cfg, dm, inp, hid, encd, bw, 0.7)
    assert R.best_of_beam(Cfg, dm, inp, hid, encd, bw, 1.0, n_groups=1) == R.best_of_beam(Cfg, dm, inp, hid, encd, bw, 1.0)
    # without a reconstructor at length_alpha = 1 the search's own order is pick_best_of_n's: rank 0
    hyps = R.beam_search_nbest(Cfg, dm, inp, hid, encd, bw, 1.0, **div)
    caps, ks, scores = R.best_of_beam(Cfg, dm, inp, hid, encd, bw, 1.0, **div)
    assert ks == [0] * B and caps == [h[0][0] for h in hyps]
    assert R.best_of_beam(Cfg, dm, inp, hid, encd, bw, 1.0, reconstructor=rm, recon_weight=0.0, **div) == (caps, ks, scores)
    # with the term: pick_best_of_n on the public reconstruction errors of the returned ranks at the common T = n_steps
    toks, cum, ln, _ = search._beam_nbest(Cfg, dm, inp, hid, encd, bw, 0.7, **div)
    n = toks.shape[1]
    errs = [R.reconstruction_errors(Cfg, dm, rm, encd, toks[k].contiguous(), T=n) for k in range(bw)]
    rk, rs = R.pick_best_of_n(cum.cpu().tolist(), ln.cpu().tolist(), errs, weight)
    caps_w, ks_w, scores_w = R.best_of_beam(Cfg, dm, inp, hid, encd, bw, 0.7, reconstructor=rm, recon_weight=weight, **div)
    assert ks_w == rk and scores_w == rs
    lens, tl = ln.cpu().tolist(), toks.cpu().tolist()
    for b in range(B):
        assert caps_w[b] == [tl[ks_w[b]][t][b] for t in range(lens[ks_w[b]][b])]
    plain = R.nbest_diversity(R.beam_search_nbest(Cfg, dm, inp, hid, encd, bw, 0.7))
    grouped = R.nbest_diversity(R.beam_search_nbest(Cfg, dm, inp, hid, encd, bw, 0.7, **div))
    print(kind, "diverse best of beam", bw, ": ranks chosen with the reconstruction term", ks_w, "diversity plain", plain, "grouped", grouped)
    # evaluate: both forms with the new keys
    idx2word = {i: "w%d" % i for i in range(V)}
    names = ["a", "b", "c", "d", "PAD", "PAD"]
    refs = {k: ["w3 w4 w5", "w7 w8"] for k in "abcd"}
    ev = lambda method, **kw: R.evaluate(Cfg, [(names, enc.numpy())], dm, method, idx2word, refs, **kw)
    s_free = ev(("beam_nbest", bw, 0.7))
    assert set(ev(("beam_nbest", bw, 0.7, div))) == set(s_free)
    assert ev(("beam_nbest", bw, 0.7, dict(n_groups=1, diversity_penalty=2.0))) == s_free
    assert ev(("beam_recon", bw, 1.0, 0.0, div), reconstructor=rm) == ev(("beam_nbest", bw, 1.0, div))
    assert set(ev(("beam_recon", bw, 0.7, weight, dict(div, no_repeat_ngram=2)), reconstructor=rm)) == set(s_free)
    with pytest.raises(ValueError, match="n_groups"):
        ev(("beam_nbest", bw, 0.7, dict(n_groups=3)))


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
        eng.beam_search_nbest_diverse(encd, 4, 0.7, 2, 0.5)
    eng.bind_decoder({k: v.data for k, v in dec.named_tensors().items()})
    eng.pack_weights()
    good = eng.beam_search_nbest_diverse(encd, 4, 0.7, 2, 0.5, no_repeat_ngram=2)
    for G in (0, -1, 3, 8):
        with pytest.raises(_lib.RecNetError, match="n_groups"):
            eng.beam_search_nbest_diverse(encd, 4, 0.7, G, 0.5)
    for lam in (-0.5, float("nan"), float("inf")):
        with pytest.raises(_lib.RecNetError, match="diversity_penalty"):
            eng.beam_search_nbest_diverse(encd, 4, 0.7, 2, lam)
    with pytest.raises(_lib.RecNetError, match="beam_width"):
        eng.beam_search_nbest_diverse(encd, 9, 0.7, 3, 0.5)
    with pytest.raises(_lib.RecNetError, match="length_alpha"):
        eng.beam_search_nbest_diverse(encd, 4, -1.0, 2, 0.5)
    with pytest.raises(_lib.RecNetError, match="min_length"):
        eng.beam_search_nbest_diverse(encd, 4, 0.7, 2, 0.5, min_length=8)
    with pytest.raises(_lib.RecNetError, match="EOS"):
        eng.beam_search_nbest_diverse(encd, 4, 0.7, 2, 0.5, banned_tokens=(2,))
    # the C ABI codes through ctypes
    lib = eng.lib
    assert lib.recnet_beam_search_nbest_diverse(eng.handle, encd.data_ptr(), 4, 0.7, 3, 0.5, 0, 0, None, 0, None, None, None, None, None, None, None) == -1
    toks, cum, ln, score, group, n = good
    args = (toks.data_ptr(), cum.data_ptr(), ln.data_ptr(), score.data_ptr())
    assert lib.recnet_beam_search_nbest_diverse(eng.handle, encd.data_ptr(), 4, 0.7, 3, 0.5, 0, 0, None, 0, *args, None, n.data_ptr(), None) == -1
    assert b"n_groups" in lib.recnet_last_error()
    assert lib.recnet_beam_search_nbest_diverse(eng.handle, encd.data_ptr(), 4, 0.7, 2, -1.0, 0, 0, None, 0, *args, None, n.data_ptr(), None) == -1
    assert b"diversity_penalty" in lib.recnet_last_error()
    # the kernel-alone entry
    x, cum3, fin = (torch.from_numpy(a).cuda() for a in BR.row_case(61, 4, "continuous"))
    with pytest.raises(_lib.RecNetError, match="n_groups"):
        eng.beam_select_rows_diverse(x, cum3, fin, 4, 3, 0.5)
    with pytest.raises(_lib.RecNetError, match="diversity_penalty"):
        eng.beam_select_rows_diverse(x, cum3, fin, 4, 2, -0.5)
    with pytest.raises(_lib.RecNetError, match="nb must be 1 or beam_width"):
        eng.beam_select_rows_diverse(x, cum3, fin, 2, 2, 0.5)
    with pytest.raises(_lib.RecNetError, match="beam_width"):
        eng.beam_select_rows_diverse(x, cum3, fin, 0, 1, 0.5)
    with pytest.raises(_lib.RecNetError, match="null argument"):
        eng.beam_select_rows_diverse(x, cum3, fin, 4, 2, 0.5, t=3, no_repeat_ngram=2)          # an n-gram rule without a history
    with pytest.raises(RuntimeError):
        eng.beam_select_rows_diverse(x, cum3, fin.long(), 4, 2, 0.5)
    # the custom ops
    ops, h = _ops.load(), int(eng.handle.value)
    with pytest.raises(RuntimeError, match="n_groups"):
        ops.beam_search_nbest_diverse(h, encd, 4, 0.7, 3, 0.5, 0, 0, [])
    with pytest.raises(RuntimeError, match="diversity_penalty"):
        ops.beam_search_nbest_diverse(h, encd, 4, 0.7, 2, float("nan"), 0, 0, [])
    with pytest.raises(RuntimeError, match="beam_width"):
        ops.beam_search_nbest_diverse(h, encd, 9, 0.7, 3, 0.5, 0, 0, [])
    with pytest.raises(RuntimeError, match="n_groups"):
        ops.beam_select_rows_diverse(h, x, cum3, fin, None, 0, 4, 3, 0.5, 0, 0, [])
    with pytest.raises(RuntimeError, match="nb must be 1 or beam_width"):
        ops.beam_select_rows_diverse(h, x, cum3, fin, None, 0, 2, 2, 0.5, 0, 0, [])
    v_ops, i_ops = ops.beam_select_rows_diverse(h, x, cum3, fin, None, 0, 4, 2, 0.5, 0, 0, [])
    v_eng, i_eng = eng.beam_select_rows_diverse(x, cum3, fin, 4, 2, 0.5)
    assert torch.equal(v_ops, v_eng) and torch.equal(i_ops, i_eng)
    # the Python layer refuses before an engine is asked for
    for kw in (dict(n_groups=3), dict(n_groups=0), dict(n_groups=2, diversity_penalty=-1.0), dict(n_groups=2, diversity_penalty=float("inf"))):
        with pytest.raises(ValueError):
            R.beam_search_nbest(cfg, dec, inp, hid, encd, 4, **kw)
        with pytest.raises(ValueError):
            R.best_of_beam(cfg, dec, inp, hid, encd, 4, **kw)
    with pytest.raises(NotImplementedError):
        R.beam_search_nbest(cfg, dec, inp * 3, hid, encd, 4, n_groups=2)
    again = eng.beam_search_nbest_diverse(encd, 4, 0.7, 2, 0.5, no_repeat_ngram=2)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(good, again))
