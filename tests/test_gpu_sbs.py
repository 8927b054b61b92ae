"""The stochastic beam search on the device (recnet_sbs_select_rows / recnet_stochastic_beam_search /
recnet_stochastic_beam_search_ensemble) against the CPU restatement (tests/sbs_ref.py): the selection kernel
alone on host-made inputs, the search on the goldens' decoders and the shape cases in fp32, self-consistency with score_captions and
sample_search in both precisions, ensembles, the callers (best_of_n(distinct=True), evaluate) and the argument checks.

Indices / tokens are compared outside the decisions the restatement marks as near-ties (its quotient below 1e-3; the caps on how many
those may be are held without a GPU by tests/test_sbs_ref.py).  Bars: a log-probability phi is held to the row bar of
tests/score_ref.py at the run's temperature (plus two units in the last place of |cum| for the kernel alone), a hypothesis' cum to its
length times the row bar; a perturbed score to that bar plus 4 fp32 ulp of max(|G|, 16) (two accurate logarithms, one addition and
the final rounding), both times the amp of the restatement.  Every test prints its worst error / bar."""
import functools

import numpy as np
import pytest
import torch

import recnet_amd as R
from recnet_amd import _ops, search
from tests import beam_ref as BR
from tests import golden_util as GU
from tests import sample_ref as SR
from tests import sbs_ref as SBS
from tests import score_ref as SC
from tests.golden_util import load_search_case
from tests.gpu_util import make_models
from tests.sample_ref import NEAR_TIE
from tests.search_kit import bound_engine, decoder_for, rows_engine, same

pytestmark = pytest.mark.gpu

Engine, _lib = R.engine.Engine, R.engine._lib


def _ulp4(g):
    """4 fp32 units in the last place of max(|G|, 16)."""
    g = np.where(np.isfinite(g), g, 0.0)
    return 4.0 * np.spacing(np.maximum(np.abs(g), 16.0).astype(np.float32)).astype(np.float64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ 1. the selection kernel alone
@functools.lru_cache(maxsize=None)
def _row_results(V):
    """Every kernel-alone case at vocabulary V, device (two calls) and restatement side by side (computed once)."""
    eng = rows_engine()
    out = []
    for nb in BR.ROW_NB:
        gum = SBS.row_gum(nb, 5, V)
        gd = torch.from_numpy(gum).cuda()
        for kind in BR.ROW_KINDS:
            x, cum, fin = BR.row_case(V, nb, kind)
            xd, cd, fd = torch.from_numpy(x).cuda(), torch.from_numpy(cum).cuda(), torch.from_numpy(fin).cuda()
            before = xd.clone()
            for bw in BR.ROW_BW:
                if bw > V:
                    continue
                bv, bi = eng.beam_select_rows(xd, cd, fd, bw)
                for t in SBS.ROW_T:
                    for temp in SBS.ROW_TEMPS:
                        seed = 1 + (V + nb + bw + t) % 8
                        a = eng.sbs_select_rows(xd, cd, gd, fd, bw, temp, seed, t)
                        b = eng.sbs_select_rows(xd, cd, gd, fd, bw, temp, seed, t)
                        idx = a[2].long()
                        i, v = idx // V, idx % V                                                         # [rows, bw]
                        rows = torch.arange(5, device="cuda")[:, None].expand_as(i)
                        lp = eng.logprob_rows(xd[i.reshape(-1), rows.reshape(-1)].contiguous(), v.reshape(-1).contiguous(), temp)
                        torch.cuda.synchronize()
                        out.append(dict(case=(V, nb, kind, bw, t, temp), x=x, cum=cum, gum=gum, fin=fin, vals=a[0].cpu().numpy(),
                                        gout=a[1].cpu().numpy(), idx=a[2].cpu().numpy(), same=same(a, b),
                                        untouched=torch.equal(xd.view(torch.int32), before.view(torch.int32)),
                                        lp=lp.cpu().numpy().reshape(5, bw), beam_vals=bv.cpu().numpy(), beam_idx=bi.cpu().numpy(),
                                        ref=SBS.select_rows(x, cum, gum, fin, bw, temp, seed, t)))
    return out


@pytest.mark.parametrize("V", BR.ROW_VS)
def test_select_rows(V):
    worst_v, worst_g, shared, bits_half = 0.0, 0.0, 0, True
    for r in _row_results(V):
        _, nb, kind, bw, t, temp = r["case"]
        ref = r["ref"]
        assert r["untouched"] and r["same"], r["case"]
        idx = r["idx"].astype(np.int64)
        assert ((idx >= 0) & (idx < nb * V)).all(), r["case"]
        keep = ref["margin"] >= NEAR_TIE
        assert np.array_equal(idx[keep], ref["idx"][keep]), (r["case"], idx, ref["idx"])
        src, tok = idx // V, idx % V
        rows = np.arange(5)[:, None]
        pfin = r["fin"][src, rows] != 0
        # a finished parent's entry carries its G and its phi bit for bit (<PAD>; its further tokens are the -inf fill)
        at_pad = pfin & (tok == 0)
        assert np.array_equal(_bits(r["vals"])[at_pad], _bits(r["cum"][src, rows])[at_pad]), r["case"]
        assert np.array_equal(_bits(r["gout"])[at_pad], _bits(r["gum"][src, rows])[at_pad]), r["case"]
        fill = pfin & (tok != 0)
        assert np.isneginf(r["vals"][fill]).all() and np.isneginf(r["gout"][fill]).all(), r["case"]
        # phi is the fp32 sum of the parent's cum and logprob_rows' log-probability of the token, at temperature 1 to the bit
        live = ~pfin
        formed = (r["cum"][src, rows] + r["lp"]).astype(np.float32)
        if temp == 1.0:
            assert np.array_equal(_bits(r["vals"])[live], _bits(formed)[live]), r["case"]
            # ... and beam_select_rows' value wherever that selection holds the same (i, v)
            for row in range(5):
                for k in range(bw):
                    hit = np.nonzero(r["beam_idx"][row] == idx[row, k])[0]
                    if hit.size and live[row, k]:
                        assert _bits(r["beam_vals"][row, hit[0]]) == _bits(r["vals"][row, k]), r["case"]
                        shared += 1
        else:
            bits_half &= bool(np.array_equal(_bits(r["vals"])[live], _bits(formed)[live]))
        # values: the rows where the index agrees with the restatement (everywhere outside near-ties)
        agree = (idx == ref["idx"]) & np.isfinite(ref["vals"])
        same_idx = idx == ref["idx"]
        assert np.array_equal(np.isneginf(r["vals"])[same_idx], np.isneginf(ref["vals"])[same_idx]), r["case"]
        lv = r["fin"] == 0
        amax = np.abs(r["x"][lv]).max() if lv.any() else 0.0
        bar_v = SC.row_bar("f32", amax, temp) + 2 * float(np.spacing(np.float32(np.abs(r["cum"]).max())))
        with np.errstate(invalid="ignore"):                              # (-inf against -inf outside `agree`)
            err_v = np.abs(r["vals"].astype(np.float64) - ref["vals"])[agree]
            err_g = np.abs(r["gout"].astype(np.float64) - ref["gum"])[agree]
        bar_g = ((bar_v + _ulp4(ref["gum"])) * ref["amp"])[agree]
        if err_v.size:
            worst_v, worst_g = max(worst_v, float(err_v.max() / bar_v)), max(worst_g, float((err_g / bar_g).max()))
            assert err_v.max() <= bar_v and (err_g <= bar_g).all(), (r["case"], float(err_v.max()), bar_v, float((err_g / bar_g).max()))
        # descending in G; a live parent's best selected child has the parent's G, to the bit
        assert (r["gout"][:, :-1] >= r["gout"][:, 1:]).all(), r["case"]
        for row in range(5):
            for i in set(src[row][live[row]].tolist()):
                kids = r["gout"][row][(src[row] == i) & live[row]]
                assert kids.max() == r["gum"][i, row], r["case"]
    print("V", V, "worst phi error / bar:", worst_v, "worst G error / bar:", worst_g, "values shared with beam_select_rows:", shared,
          "phi = cum + logprob_rows to the bit at temperature 0.5:", bits_half)
    assert shared > 0 or V > 257          # (a sampled token is seldom among the mode's best of a long row: counted, not demanded, there)


# ------------------------------------------------------------------------------------------------ 2. the search in fp32
def _device_search(name, bw, cml, temp, seed, prec="f32"):
    g, P, enc = load_search_case(name)
    dec, cfg, inp, hid = decoder_for(g, P, prec, cml)
    return (dec, cfg, inp, hid, enc.cuda()), search._sbs(cfg, dec, inp, hid, enc.cuda(), bw, temp, seed)


@pytest.mark.parametrize("name,bw,cml,temp,seed", SBS.SEARCH_RUNS + SBS.DEVICE_RUNS)
def test_search_matches_the_restatement(name, bw, cml, temp, seed):
    """fp32 path: n_steps (when no caption is excluded), tokens, len and the rank order equal the restatement on the captions without
    a near-tie decision; cum within len x the row bar at the temperature, G within its bar.  A caption with a near-tie is compared up
    to that decision: the first t0 tokens of each of its returned hypotheses against the restatement's beams (beam_ref's rule)."""
    r = SBS.run(name, bw, cml, temp, seed)
    args, out = _device_search(name, bw, cml, temp, seed)
    toks, cum, ln, gum = (x.cpu().numpy() for x in out)
    cum, gum = cum.astype(np.float64), gum.astype(np.float64)
    B = args[4].shape[0]
    keep = SBS.comparable_captions(r)
    n = toks.shape[1]
    assert toks.shape == (bw, n, B) and 1 <= n <= cml + 1
    if keep.all():
        assert n == r["n_steps"]
    m = min(n, r["n_steps"])
    assert np.array_equal(ln[:, keep], r["len"][:, keep])
    assert np.array_equal(toks[:, :m][:, :, keep], r["tokens"][:, :m][:, :, keep])
    assert (toks[:, m:][:, :, keep] == 0).all() and (r["tokens"][:, m:][:, :, keep] == 0).all()
    assert (gum[:-1] >= gum[1:]).all() and (gum[0] == 0).all()            # rank order; rank 0 inherits the root's G = 0 exactly
    bar = r["len"] * SC.row_bar("f32", r["amax"].max(), temp)
    bar_g = (bar + _ulp4(r["gum"])) * r["amp"]
    err, err_g = np.abs(cum - r["cum"])[:, keep], np.abs(gum - r["gum"])[:, keep]
    worst = float((err / bar[:, keep]).max()) if err.size else 0.0
    worst_g = float((err_g / bar_g[:, keep]).max()) if err.size else 0.0
    print(name, "width", bw, "cml", cml, "temperature", temp, "steps", n, "captions compared", int(keep.sum()), "of", keep.size,
          "worst cum error / bar:", worst, "worst G error / bar:", worst_g)
    assert (err <= bar[:, keep]).all() and (err_g <= bar_g[:, keep]).all()
    t0 = SBS.comparable_steps(r["margins"]).sum(axis=0)
    prefixes = 0
    for b in np.nonzero(~keep)[0]:
        k = int(t0[b])
        if k == 0:
            continue
        allowed = {tuple(h) for h in r["trace"][k - 1]["hist"][:, b, :k].tolist()}
        for rank in range(bw):
            got = toks[rank, :k, b].tolist()
            got += [0] * (k - len(got))          # (a search that stopped earlier carries <PAD>)
            assert tuple(got) in allowed, (b, rank, k, got, allowed)
        prefixes += k
    print(name, "width", bw, "decisions compared through excluded captions' prefixes:", prefixes)
    assert keep.any() or prefixes > 0
    # the public list form of the same call
    cfg, dec, inp, hid, encd = args[1], args[0], args[2], args[3], args[4]
    hyps = R.stochastic_beam_search(cfg, dec, inp, hid, encd, bw, temp, seed)
    assert len(hyps) == B and all(len(h) == bw for h in hyps)
    for b, h in enumerate(hyps):
        for k, (t, c, l, gg) in enumerate(h):
            assert l == ln[k, b] and t == toks[k, :l, b].tolist() and c == float(out[1][k, b]) and gg == float(out[3][k, b])


# ------------------------------------------------------------------------------------------------ 3. fp32 and bf16
@pytest.mark.parametrize("name", ["search_small", "search_gru"])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_self_consistency(name, prec):
    """score_captions(temperature) on every returned rank: len exact, cum the same bits at temperature 1 (the selection forms the
    log-probability as the row kernel does and sums it in the same order), within len x the row bar at 0.5, where the test prints
    whether the bits match too; two calls give equal bits, two seeds differ; every rank is canonical, G descends."""
    g, P, enc = load_search_case(name)
    dec, cfg, inp, hid = decoder_for(g, P, prec)
    encd = enc.cuda()
    amax = BR.beam_search_nbest(P, enc, 3, 0.7, 30, g["_cell"])["amax"].max()
    worst, bits_half = 0.0, True
    for bw in (3, 8):
        for temp in (1.0, 0.5):
            a = search._sbs(cfg, dec, inp, hid, encd, bw, temp, 5)
            assert same(a, search._sbs(cfg, dec, inp, hid, encd, bw, temp, 5))
            assert not same(a, search._sbs(cfg, dec, inp, hid, encd, bw, temp, 6))
            toks, cum, ln, gum = a
            assert (gum[:-1] >= gum[1:]).all()
            for k in range(bw):
                assert torch.equal(R.canonical_captions(toks[k]), toks[k])
                _, cap, sl = search._score(dec, encd, toks[k].contiguous(), temp, False)
                assert torch.equal(sl.cpu(), ln[k].cpu()), (k, sl, ln[k])
                equal = torch.equal(cap.view(torch.int32), cum[k].view(torch.int32))
                if temp == 1.0:
                    assert equal, (bw, k, cap, cum[k])
                else:
                    bits_half &= equal
                    bar = ln[k].cpu().numpy() * SC.row_bar(prec, amax, temp)
                    err = np.abs(cap.cpu().numpy().astype(np.float64) - cum[k].cpu().numpy())
                    worst = max(worst, float((err / bar).max()))
                    assert (err <= bar).all(), (k, err, bar)
    print(name, prec, "temperature 0.5: worst |score_captions - cum| / (len x row bar):", worst, "the same bits:", bits_half)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_ranks_are_distinct_at_the_benchmark_decoder(prec):
    (_, _, _, _, encd), (toks, cum, ln, gum) = _device_search("eval_msvd", 8, 7, 1.0, 3, prec)
    t = toks.cpu().numpy()
    for b in range(encd.shape[0]):
        assert len({tuple(t[k, :, b]) for k in range(8)}) == 8, b


@pytest.mark.parametrize("name,temp,seed", SBS.WIDTH1_RUNS)
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_width_one_draws_sample_search_tokens(prec, name, temp, seed):
    """Width 1 against sample_search(temperature, top_k = 0, seed) on the device, up to each caption's <EOS>, on the captions neither
    restatement excludes (their near-ties are where argmax(phi + g) and argmax(s + g) may part)."""
    g, P, enc = load_search_case(name)
    cml = 7
    dec, cfg, inp, hid = decoder_for(g, P, prec, cml)
    encd = enc.cuda()
    r = SBS.run(name, 1, cml, temp, seed)
    _, _, margins, _ = SR.sample_search(P, enc, temp, 0, seed, cml, g["_cell"])
    ok = SBS.comparable_captions(r) & SR.comparable(margins).all(axis=0)
    toks = search._sbs(cfg, dec, inp, hid, encd, 1, temp, seed)[0][0].cpu().numpy()
    drawn = np.array(R.sample_search(cfg, dec, inp, hid, encd, temp, 0, seed)[0], dtype=np.int64)
    compared = 0
    for b in np.nonzero(ok)[0]:
        for t in range(min(toks.shape[0], drawn.shape[0])):
            assert toks[t, b] == drawn[t, b], (b, t, toks[:, b], drawn[:, b])
            compared += 1
            if drawn[t, b] == SBS.EOS:
                break
    print(prec, name, temp, seed, "captions compared", int(ok.sum()), "of", ok.size, "tokens", compared)
    assert prec == "bf16" or compared > 0


# ------------------------------------------------------------------------------------------------ 4. ensembles
@pytest.mark.parametrize("name", ["search_small", "search_gru"])
def test_ensemble_of_one_is_the_model(name):
    g, P, enc = load_search_case(name)
    dec, cfg, inp, hid = decoder_for(g, P, "f32")
    encd = enc.cuda()
    ens = R.Ensemble([dec], [3.0], "geometric")
    for bw in (1, 3, 8):
        assert same(search._sbs(cfg, dec, inp, hid, encd, bw, 1.0, 2), search._sbs(cfg, ens, inp, hid, encd, bw, 1.0, 2)), bw
    assert R.stochastic_beam_search(cfg, dec, inp, hid, encd, 3, seed=4) == R.stochastic_beam_search(cfg, ens, inp, hid, encd, 3, seed=4)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_ensemble_score_captions_reproduces_cum(prec):
    """A two-member arithmetic ensemble: ensemble score_captions on every returned rank gives its len exactly and its cum within
    len x 2 x the row bar of the precision (two device paths, as tests/test_gpu_ensemble.py holds the N-best search)."""
    from tests import ensemble_ref as ER
    from tests.test_gpu_ensemble import _amax, device_members
    names, w = ER.G97, (1, 2)
    decs, cfg, inp, hid, encd = device_members(names, prec)
    ens = R.Ensemble(decs, w, "arithmetic")
    amax = _amax(names, w, "arithmetic")
    worst = 0.0
    for bw in (3, 8):
        a = search._sbs(cfg, ens, inp, hid, encd, bw, 1.0, 7)
        assert same(a, search._sbs(cfg, ens, inp, hid, encd, bw, 1.0, 7))
        toks, cum, ln, gum = a
        assert (gum[:-1] >= gum[1:]).all()
        t = toks.cpu().numpy()
        for b in range(encd.shape[0]):
            assert len({tuple(t[k, :, b]) for k in range(bw)}) == bw
        for k in range(bw):
            _, cap, sl = search._score(ens, encd, toks[k].contiguous(), 1.0, False, cfg.caption_max_len)
            assert torch.equal(sl.cpu(), ln[k].cpu())
            bar = ln[k].cpu().numpy() * 2 * SC.row_bar(prec, amax, 1.0)
            err = np.abs(cap.cpu().numpy().astype(np.float64) - cum[k].cpu().numpy())
            worst = max(worst, float((err / bar).max()))
            assert (err <= bar).all(), (bw, k, err, bar)
    print(prec, "worst |ensemble score_captions - cum| / (len x 2 x row bar):", worst)


# ------------------------------------------------------------------------------------------------ 5. the callers
def test_best_of_n_distinct_and_evaluate():
    dims = [6, 5, 32, 41, 12, 24, 8, 8]
    B, F, D, V, E, H, A, RA = dims
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D), 21)
    recP = GU.formula_params(GU.rec_shapes("global", H, D, RA), 22)
    enc, _ = GU.make_batch(B, F, D, V, [3] * B, 23)
    Cfg, dec, rec = make_models(list(dims), "global", "f32", decP, recP)
    dm, rm = dec["model"].eval(), rec["model"].eval()
    encd = enc.cuda()
    inp = torch.full((1, B), 1, dtype=torch.long, device="cuda")
    hid = (torch.zeros(1, B, H, device="cuda"), torch.zeros(1, B, H, device="cuda"))
    args = (Cfg, dm, inp, hid, encd)
    n, seed = 5, 11
    for temp in (1.0, 0.7):
        toks, cum, ln, gum = search._sbs(*args, n, temp, seed)
        tl, lens = toks.cpu().tolist(), ln.cpu().tolist()
        cums = cum.cpu().tolist()
        if temp != 1.0:                                                   # scores are those of the full distribution at temperature 1
            cums = [R.score_captions(Cfg, dm, encd, toks[k].contiguous())[1] for k in range(n)]
        cut = lambda ks: [[tl[k][t][b] for t in range(lens[k][b])] for b, k in enumerate(ks)]
        # by the model's own score
        ks, scores = R.pick_best_of_n(cums, lens)
        assert R.best_of_n(*args, n, temp, seed=seed, distinct=True) == (cut(ks), ks, scores)
        # with the consensus term: the utilities weigh reference k by its normalised importance weight
        weights = R.sbs_weights(cum.cpu().tolist(), gum.cpu().tolist())
        assert all(abs(sum(w[b] for w in weights) - 1.0) < 1e-12 and weights[n - 1][b] == 0.0 for b in range(B))
        util = R.consensus_scores(toks.contiguous(), weights=weights)
        ks_c, scores_c = R.pick_best_of_n(cums, lens, None, 0.0, util, 3.0)
        assert R.best_of_n(*args, n, temp, seed=seed, consensus_weight=3.0, distinct=True) == (cut(ks_c), ks_c, scores_c)
        assert util != R.consensus_scores(toks.contiguous())             # (the weights are not the uniform ones)
        # with the reconstruction term, all ranks at the common T = n_steps
        errs = [R.reconstruction_errors(Cfg, dm, rm, encd, toks[k].contiguous(), T=toks.shape[1]) for k in range(n)]
        ks_r, scores_r = R.pick_best_of_n(cums, lens, errs, 64.0)
        assert R.best_of_n(*args, n, temp, seed=seed, reconstructor=rm, recon_weight=64.0, distinct=True) == (cut(ks_r), ks_r, scores_r)
        print("temperature", temp, "chosen ranks: own score", ks, "consensus", ks_c, "reconstruction", ks_r)
    # distinct=False is the composition it always was: n rollouts, n scoring passes, the same tail
    cands = [R.sample_search(*args, 0.7, 0, (seed + k) & 0xFFFFFFFF)[0] for k in range(n)]
    scored = [R.score_captions(Cfg, dm, encd, c) for c in cands]
    caps, lens = [s[1] for s in scored], [s[2] for s in scored]
    t_star = max(len(c) for c in cands)
    hyp = [c + [[2] * B] * (t_star - len(c)) for c in cands]
    ks, scores = R.pick_best_of_n(caps, lens, None, 0.0, R.consensus_scores(hyp, device="cuda"), 2.0)
    old = ([[cands[k][t][b] for t in range(lens[k][b])] for b, k in enumerate(ks)], ks, scores)
    assert R.best_of_n(*args, n, 0.7, 0, seed, consensus_weight=2.0) == old == R.best_of_n(*args, n, 0.7, 0, seed, consensus_weight=2.0, distinct=False)
    # evaluate
    idx2word = {i: "w%d" % i for i in range(V)}
    names = ["a", "b", "c", "d", "PAD", "PAD"]
    refs = {k: ["w3 w4 w5", "w7 w8"] for k in "abcd"}
    ev = lambda method, **kw: R.evaluate(Cfg, [(names, enc.numpy())], dm, method, idx2word, refs, **kw)
    s_greedy = ev("greedy")
    for method in (("sbs", 4, 1.0, 3), ("best_of_distinct", 4, 0.7, 3), ("best_of_distinct_consensus", 4, 1.0, 3, 2.0)):
        assert set(ev(method)) == set(s_greedy), method
    assert ev(("best_of_distinct", 1, 1.0, 3)) == ev(("sbs", 1, 1.0, 3))      # one candidate: the sample itself
    with pytest.raises(ValueError, match="fields"):
        ev(("sbs", 4, 1.0))


# ------------------------------------------------------------------------------------------------ 6. errors
def test_library_refuses_bad_arguments_and_recovers():
    g, P, enc = load_search_case("search_small")
    dec, cfg, inp, hid = decoder_for(g, P, "f32")
    encd = enc.cuda()
    B, F, V = enc.shape[0], enc.shape[1], int(g["meta_dims"][3])
    eng = Engine(dec.dims(B, F), None, "f32", dec.hyper(), device=encd.device)
    with pytest.raises(_lib.RecNetError, match="decoder not bound"):
        eng.stochastic_beam_search(encd, 3)
    eng.bind_decoder({k: v.data for k, v in dec.named_tensors().items()})
    eng.pack_weights()
    good = eng.stochastic_beam_search(encd, 3, 0.8, 9)
    for bw in (0, 9, -1):
        with pytest.raises(_lib.RecNetError, match="beam_width"):
            eng.stochastic_beam_search(encd, bw)
    for temp in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(_lib.RecNetError, match="temperature"):
            eng.stochastic_beam_search(encd, 3, temp)
        with pytest.raises(_lib.RecNetError, match="temperature"):
            Engine.stochastic_beam_search_ensemble([eng], encd, 3, temp, weights=[1.0])
    other = bound_engine(dec, B, F, "f32")
    with pytest.raises(_lib.RecNetError, match="distinct handles"):
        Engine.stochastic_beam_search_ensemble([eng, eng], encd, 3)
    with pytest.raises(_lib.RecNetError, match="weights"):
        Engine.stochastic_beam_search_ensemble([eng, other], encd, 3, weights=[1.0, -1.0])
    x, cum, fin = (torch.from_numpy(a).cuda() for a in BR.row_case(8, 3, "continuous"))
    gum = torch.from_numpy(SBS.row_gum(3, 5, 8)).cuda()
    with pytest.raises(_lib.RecNetError, match="beam_width"):
        eng.sbs_select_rows(x[:, :, :4].contiguous(), cum, gum, fin, 5)          # wider than V
    with pytest.raises(_lib.RecNetError, match="beam_width"):
        eng.sbs_select_rows(x, cum, gum, fin, 0)
    with pytest.raises(_lib.RecNetError, match="temperature"):
        eng.sbs_select_rows(x, cum, gum, fin, 3, temperature=0.0)
    with pytest.raises(_lib.RecNetError, match="non-negative"):
        eng.sbs_select_rows(x, cum, gum, fin, 3, t=-1)
    with pytest.raises(RuntimeError):
        eng.sbs_select_rows(x, cum, gum[:2].contiguous(), fin, 3)
    with pytest.raises(RuntimeError):
        eng.sbs_select_rows(x, cum, gum.double(), fin, 3)
    ops = _ops.load()
    with pytest.raises(RuntimeError, match="beam_width"):
        ops.sbs_select_rows(int(eng.handle.value), x, cum, gum, fin, 9, 1.0, 0, 0)
    with pytest.raises(RuntimeError, match="beam_width"):
        ops.stochastic_beam_search(int(eng.handle.value), encd, 9, 1.0, 0)
    with pytest.raises(RuntimeError, match="temperature"):
        ops.stochastic_beam_search(int(eng.handle.value), encd, 3, 0.0, 0)
    assert same(ops.sbs_select_rows(int(eng.handle.value), x, cum, gum, fin, 3, 0.5, 4, 2), eng.sbs_select_rows(x, cum, gum, fin, 3, 0.5, 4, 2))
    again = eng.stochastic_beam_search(encd, 3, 0.8, 9)
    torch.cuda.synchronize()
    assert same(good, again) and same(good, ops.stochastic_beam_search(int(eng.handle.value), encd, 3, 0.8, 9))
