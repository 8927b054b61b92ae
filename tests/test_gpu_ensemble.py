"""Ensemble decoding on the device (recnet_ensemble_mix_rows / recnet_beam_search_nbest_ensemble / recnet_score_captions_ensemble;
DESIGN.md section 19) against the CPU restatement tests/ensemble_ref.py: the mix kernel alone on host-made rows, the search and the
scorer on the goldens' decoders, an ensemble of one against the single-model calls bit for bit, self-consistency of search and
scorer in both precisions, invariance under copies and under the members' order, and the public layer.

Bars.  One log-probability of one member is within score_ref.row_bar (a logit minus a log-sum-exp of logits).  The mix is a convex
combination of the members' log-probabilities in the sup norm (1-Lipschitz), so the ensemble's logits y are within the same bar; a
candidate y[v] - logsumexp(y) doubles it, and one more row bar covers the fp32 rounding of the mix itself (about 1e-5 at these
magnitudes against 8e-5 x max |logit|): 3 x row_bar per step against the restatement, 2 x row_bar per step between two device paths
(as tests/test_gpu_score.py compares scorer and sampler).  Tokens are compared outside the decisions the restatement marks as
near-ties (tests/test_ensemble_ref.py holds the caps on how many those may be without a GPU).  Every test prints its worst error /
bar."""
import functools

import numpy as np
import pytest
import torch

import recnet_amd as R
from recnet_amd import metrics, search
from tests import beam_ref as BR
from tests import ensemble_ref as ER
from tests import score_ref as SC
from tests.golden_util import load
from tests.search_kit import decoder_for, rows_engine, same

pytestmark = pytest.mark.gpu

# the mix kernel keeps the M rows in LDS while M * ceil4(V) <= 24576 floats (ENS_LDS_FLOATS, csrc/kernels_search.hpp)
LDS_FLOATS = 24576
ROW_MS = (1, 2, 3, 8)
# the last V of the LDS form and the first of the streaming form at M = 8, 3 and 2, with neighbours that are no multiple of 4
THRESHOLD_VS = (3071, 3072, 3073, 8192, 8193, 12288, 12289)


def _weights(M, uniform):
    return [1.0] * M if uniform else [float(m + 1) for m in range(M)]


# ------------------------------------------------------------------------------------------------ 1. the mix kernel alone
@pytest.mark.parametrize("V", BR.ROW_VS + THRESHOLD_VS)
def test_mix_rows(V):
    eng = rows_engine()
    worst, forms = 0.0, set()
    for M in ROW_MS:
        for kind in ("continuous", "quantised"):
            x, _, _ = BR.row_case(V, M, kind)                              # [M, 5, V]: one row block per member
            x[:, 4] = x[:, 0]                                              # a copied row
            xd = [torch.from_numpy(x[m]).cuda() for m in range(M)]
            before = [t.clone() for t in xd]
            bar = SC.row_bar("f32", np.abs(x).max(), 1.0)
            forms.add(M * ((V + 3) // 4 * 4) <= LDS_FLOATS)
            for mode in ER.MODES:
                w = _weights(M, uniform=(mode == "arithmetic") == (kind == "continuous"))
                y = eng.ensemble_mix_rows(xd, w, mode)
                y2 = eng.ensemble_mix_rows(xd, w, mode)
                torch.cuda.synchronize()
                assert same([y], [y2]) and same(xd, before), (V, M, kind, mode)
                assert torch.equal(y[0].view(torch.int32), y[4].view(torch.int32)), (V, M, kind, mode)
                ref = ER.mix_rows([x[m] for m in range(M)], w, mode)
                err = float(np.abs(y.cpu().numpy().astype(np.float64) - ref).max())
                worst = max(worst, err / bar)
                assert err <= bar, (V, M, kind, mode, err, bar)
                if kind == "continuous":                                   # in place over member 0's rows: the same bits
                    x0 = xd[0].clone()
                    yi = eng.ensemble_mix_rows([x0] + xd[1:], w, mode, in_place=True)
                    assert yi.data_ptr() == x0.data_ptr() and same([yi], [y]), (V, M, mode)
        # one member with weight 1: y = log_softmax(x), so the scorer reads the same log-probabilities from y as from x
        x, _, _ = BR.row_case(V, 1, "continuous")
        xd = torch.from_numpy(x[0]).cuda()
        tok = torch.from_numpy(np.array([0, V - 1, int(x[0, 2].argmax()), V // 2, 1 % V], dtype=np.int64)).cuda()
        for mode in ER.MODES:
            y = eng.ensemble_mix_rows([xd], [1.0], mode)
            d = (eng.logprob_rows(y, tok) - eng.logprob_rows(xd, tok)).abs().max().item()
            bar = SC.row_bar("f32", np.abs(x).max(), 1.0)
            worst = max(worst, d / bar)
            assert d <= bar, (V, mode, d, bar)
    print("V", V, "LDS form / streaming form run:", sorted(forms), "worst mix error / bar:", worst)


def test_mix_rows_unaligned_rows_and_the_public_face():
    """Rows that start 4 bytes off a 16-byte boundary (V % 4 == 0: the scalar path by alignment alone) give the bits of aligned
    ones; search.ensemble_logits is the same entry."""
    eng = rows_engine()
    V, M = 256, 3
    x, _, _ = BR.row_case(V, M, "continuous")
    xd = [torch.from_numpy(x[m]).cuda() for m in range(M)]
    off = []
    for t in xd:
        buf = torch.empty(t.numel() + 4, device="cuda")
        v = buf[1:1 + t.numel()].view_as(t)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        off.append(v)
    for mode in ER.MODES:
        y = eng.ensemble_mix_rows(xd, [1, 2, 3], mode)
        assert same([eng.ensemble_mix_rows(off, [1, 2, 3], mode)], [y])
        assert same([eng.ensemble_mix_rows([off[0]] + xd[1:], [1, 2, 3], mode)], [y])

        class D:
            output_size, encoder_size = V, 8
        ens = R.Ensemble([D(), D(), D()], [1, 2, 3], mode)
        assert same([R.ensemble_logits(ens, [x[m] for m in range(M)])], [y])
    # the library's refusals, and a good call after them
    _lib = R.engine._lib
    with pytest.raises(_lib.RecNetError, match="positive and finite"):
        eng.ensemble_mix_rows(xd, [1, 0, 1], "arithmetic")
    with pytest.raises(_lib.RecNetError, match="unknown ensemble mode"):
        eng.ensemble_mix_rows(xd, [1, 1, 1], 7)
    with pytest.raises(_lib.RecNetError, match="between 1 and 8"):
        eng.ensemble_mix_rows(xd * 3, None, "arithmetic")
    with pytest.raises(_lib.RecNetError, match="overlap"):
        eng.ensemble_mix_rows([xd[0], xd[0]], None, "arithmetic", in_place=True)      # y is member 1's rows as well
    flat = xd[0].view(-1)
    with pytest.raises(_lib.RecNetError, match="overlap"):                                # y reaches into member 1's rows
        eng.ensemble_mix_rows([flat[:4 * V].view(4, V), flat[V:].view(4, V)], None, "arithmetic", in_place=True)
    assert same([eng.ensemble_mix_rows(xd, [1, 2, 3], "geometric")], [y])


# ------------------------------------------------------------------------------------------------ the members on the device
@functools.lru_cache(maxsize=None)
def device_members(names, prec="f32", cml=30):
    """(decoders, config, <SOS> input, zero state, features on the device) of the named members; config and start state are member
    0's, the features its golden's."""
    decs, first = [], None
    for n in names:
        P, cell, enc, dims = ER.load_member(n)
        dec, cfg, inp, hid = decoder_for({"meta_dims": dims, "_cell": cell}, P, prec, cml)
        decs.append(dec)
        first = first or (cfg, inp, hid, enc.cuda())
    return (decs,) + first


@functools.lru_cache(maxsize=None)
def restated(run):
    return ER.run_search(run)


def _run_id(r):
    return "%s-%s-%d-%d" % ("+".join(r[0]), r[1], r[2], r[3])


# ------------------------------------------------------------------------------------------------ 2. the search
@pytest.mark.parametrize("run", ER.SEARCH_RUNS, ids=_run_id)
def test_search_matches_the_restatement(run):
    """fp32 path, compared the way search_kit.check_nbest_against_restatement compares a single model: n_steps, tokens, len and the
    rank order exact on the captions without a near-tie decision, cum and score within len x 3 x the row bar; a caption with a
    near-tie through the prefix before it."""
    names, mode, bw, cml, w = run
    r = restated(run)
    decs, cfg, inp, hid, encd = device_members(names, "f32", cml)
    ens = R.Ensemble(decs, w, mode)
    toks, cum, ln, score = search._beam_nbest(cfg, ens, inp, hid, encd, bw, ER.LENGTH_ALPHA)
    toks, cum, ln, score = toks.cpu().numpy(), cum.cpu().numpy().astype(np.float64), ln.cpu().numpy(), score.cpu().numpy().astype(np.float64)
    keep = ER.comparable_captions(r)
    n = toks.shape[1]
    assert toks.shape == (bw, n, encd.shape[0]) and 1 <= n <= cml + 1
    if keep.all():
        assert n == r["n_steps"]
    m = min(n, r["n_steps"])
    assert np.array_equal(ln[:, keep], r["len"][:, keep])
    assert np.array_equal(toks[:, :m][:, :, keep], r["tokens"][:, :m][:, :, keep])
    assert (toks[:, m:][:, :, keep] == 0).all() and (r["tokens"][:, m:][:, :, keep] == 0).all()
    bar = r["len"] * 3 * SC.row_bar("f32", r["amax"].max(), 1.0)
    err, errs = np.abs(cum - r["cum"])[:, keep], np.abs(score - r["score"])[:, keep]
    worst = float((err / bar[:, keep]).max()) if err.size else 0.0
    print(_run_id(run), "steps", n, "captions compared", int(keep.sum()), "of", keep.size, "worst cum error / bar:", worst)
    assert (err <= bar[:, keep]).all() and (errs <= bar[:, keep]).all()
    t0 = ER.comparable_steps(r["margins"]).sum(axis=0)
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
    print(_run_id(run), "decisions compared through excluded captions' prefixes:", prefixes)
    assert keep.any() or prefixes > 0
    hyps = R.beam_search_nbest(cfg, ens, inp, hid, encd, bw, ER.LENGTH_ALPHA)
    assert len(hyps) == encd.shape[0] and all(len(h) == bw for h in hyps)
    for b, h in enumerate(hyps):
        for k, (t, c, l, s) in enumerate(h):
            assert l == ln[k, b] and t == toks[k, :l, b].tolist() and c == float(cum[k, b]) and s == float(score[k, b])


# ------------------------------------------------------------------------------------------------ 3. an ensemble of one
@pytest.mark.parametrize("name", ["search_small", "search_gru"])
def test_ensemble_of_one_is_the_model(name):
    decs, cfg, inp, hid, encd = device_members((name,))
    dec, ens = decs[0], R.Ensemble(decs, [3.0], "geometric")
    cases = [(bw, {}) for bw in (1, 3, 8)] + [(3, dict(no_repeat_ngram=2, min_length=3, banned_tokens=(5, 9))),
                                              (8, dict(n_groups=4, diversity_penalty=0.5, want_groups=True)),
                                              (8, dict(n_groups=2, diversity_penalty=1.5, no_repeat_ngram=2, want_groups=True)),
                                              (3, dict(want_groups=True))]
    for bw, kw in cases:
        a = search._beam_nbest(cfg, dec, inp, hid, encd, bw, 0.7, **kw)
        b = search._beam_nbest(cfg, ens, inp, hid, encd, bw, 0.7, **kw)
        assert same(a, b), (bw, kw)
        for k in range(bw):
            caps = a[0][k].contiguous()
            assert same(search._score(dec, encd, caps, 1.0, False, cfg.caption_max_len), search._score(ens, encd, caps, 1.0, False, cfg.caption_max_len))
    caps = load(name)["greedy"]
    assert R.score_captions(cfg, dec, encd, caps.tolist()) == R.score_captions(cfg, ens, encd, caps.tolist())
    assert R.beam_search_nbest(cfg, dec, inp, hid, encd, 3, 0.7) == R.beam_search_nbest(cfg, ens, inp, hid, encd, 3, 0.7)


# ------------------------------------------------------------------------------------------------ 4. search and scorer agree
@functools.lru_cache(maxsize=None)
def _amax(names, w, mode):
    models, enc = ER.load_models(names)
    return float(ER.beam_search_nbest(models, enc, 3, 0.7, 30, w, mode)["amax"].max())


@pytest.mark.parametrize("mode", ER.MODES)
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_self_consistency(prec, mode):
    """Two calls give the same bits, ranks descend, every rank is canonical; ensemble score_captions on every returned rank gives
    its len exactly and its cum within len x 2 x the row bar of the precision (two device paths: the per-step kernels of the
    search, the chain of the scorer)."""
    names, w = ER.G97, (1, 2)
    decs, cfg, inp, hid, encd = device_members(names, prec)
    ens = R.Ensemble(decs, w, mode)
    amax = _amax(names, w, mode)
    worst = 0.0
    for bw, kw in ((3, {}), (8, {}), (8, dict(n_groups=4, diversity_penalty=0.5, no_repeat_ngram=2))):
        a = search._beam_nbest(cfg, ens, inp, hid, encd, bw, 0.7, **kw)
        b = search._beam_nbest(cfg, ens, inp, hid, encd, bw, 0.7, **kw)
        assert same(a, b), (bw, kw)
        toks, cum, ln, score = a
        assert (score[:-1] >= score[1:]).all()
        for k in range(bw):
            assert torch.equal(R.canonical_captions(toks[k]), toks[k])
            _, cap, sl = search._score(ens, encd, toks[k].contiguous(), 1.0, False, cfg.caption_max_len)
            assert torch.equal(sl.cpu(), ln[k].cpu()), (k, sl, ln[k])
            bar = ln[k].cpu().numpy() * 2 * SC.row_bar(prec, amax, 1.0)
            err = np.abs(cap.cpu().numpy().astype(np.float64) - cum[k].cpu().numpy())
            worst = max(worst, float((err / bar).max()))
            assert (err <= bar).all(), (bw, kw, k, err, bar)
    print(prec, mode, "worst |ensemble score_captions - cum| / (len x 2 x row bar):", worst)


def test_members_of_different_precision():
    """An fp32 LSTM and a bf16 GRU member: the search's cum and ensemble score_captions agree within len x 2 x the bf16 row bar, the
    scorer is within 3 x the bf16 row bar of the restatement, and the tokens are the restatement's on the captions whose every
    margin is above twice the bf16 bar of a candidate (their number is printed: none on these goldens, whose margins are far below
    a bf16 bar; the fp32 runs above compare the tokens)."""
    names, w, bw, cml = ER.G97, (1, 1), 3, 7
    d32, cfg, inp, hid, encd = device_members(names[:1], "f32", cml)
    d16 = device_members(names[1:], "bf16", cml)[0]
    models, enc = ER.load_models(names)
    for mode in ER.MODES:
        ens = R.Ensemble(d32 + d16, w, mode)
        r = ER.beam_search_nbest(models, enc, bw, ER.LENGTH_ALPHA, cml, w, mode)
        row = SC.row_bar("bf16", r["amax"].max(), 1.0)
        a = search._beam_nbest(cfg, ens, inp, hid, encd, bw, ER.LENGTH_ALPHA)
        assert same(a, search._beam_nbest(cfg, ens, inp, hid, encd, bw, ER.LENGTH_ALPHA))
        toks, cum, ln, _ = a
        worst = 0.0
        for k in range(bw):
            lps, cap, sl = search._score(ens, encd, toks[k].contiguous(), 1.0, False, cml)
            assert torch.equal(sl, ln[k])
            err = (cap.double() - cum[k].double()).abs().cpu().numpy()
            worst = max(worst, float((err / (ln[k].cpu().numpy() * 2 * row)).max()))
            assert (err <= ln[k].cpu().numpy() * 2 * row).all()
        safe = (r["margins"] >= 2 * 3 * row).all(axis=0) & (r["final_margin"] >= 2 * 3 * row * r["len"].max(axis=0))
        n = min(toks.shape[1], r["n_steps"])
        assert np.array_equal(toks.cpu().numpy()[:, :n][:, :, safe], r["tokens"][:, :n][:, :, safe])
        ref, amax = ER.score_captions(models, enc, r["tokens"][0], w, mode)
        lps = search._score(ens, encd, torch.from_numpy(r["tokens"][0]), 1.0, False, cml)[0].cpu().numpy().astype(np.float64)
        rerr = float((np.abs(lps - ref).max(axis=1) / (3 * np.array([SC.row_bar("bf16", x, 1.0) for x in amax]))).max())
        print("f32 + bf16 members,", mode, "captions with every margin above the bf16 bar:", int(safe.sum()), "worst |score - cum| / bar:", worst,
              "worst row error / (3 x bf16 row bar):", rerr)
        assert rerr <= 1.0


# ------------------------------------------------------------------------------------------------ 5. the scorer
SCORE_CASES = [(ER.G97, (1, 2), "search_eos"), (ER.G97_3, (1, 2, 3), "search_small"), (ER.G97_ODD, (1, 1), "search_eos"),
               (ER.G61_3, (1, 1, 1), "search_stop"), (("search_gru_stop", "search_stop"), (2, 1), "search_gru_stop")]


@pytest.mark.parametrize("names,w,caption_golden", SCORE_CASES, ids=lambda v: v if isinstance(v, str) else None)
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_score_matches_the_restatement(prec, names, w, caption_golden):
    """The golden's greedy captions (31 rows; 1 row on the *_stop goldens) under the ensemble: every row within 3 x the row bar of
    its step and precision, the caption sums within length x that at the largest step, the lengths exact."""
    caps = load(caption_golden)["greedy"].astype(np.int64)
    models, enc = ER.load_models(names)
    decs, cfg, inp, hid, encd = device_members(names, prec)
    worst = 0.0
    for mode in ER.MODES:
        ref, amax = ER.score_captions(models, enc, caps, w, mode)
        rsum, rlen = SC.caption_sums(ref, caps)
        ens = R.Ensemble(decs, w, mode)
        lps, cap, ln = search._score(ens, encd, torch.from_numpy(caps), 1.0, False, cfg.caption_max_len)
        assert same([lps, cap, ln], search._score(ens, encd, torch.from_numpy(caps), 1.0, True, cfg.caption_max_len))
        lps, cap = lps.cpu().numpy().astype(np.float64), cap.cpu().numpy().astype(np.float64)
        assert np.array_equal(ln.cpu().numpy(), rlen)
        for t in range(caps.shape[0]):
            bar = 3 * SC.row_bar(prec, amax[t], 1.0)
            err = float(np.abs(lps[t] - ref[t]).max())
            worst = max(worst, err / bar)
            assert err <= bar, (mode, t, err, bar)
        sbar = rlen * 3 * SC.row_bar(prec, amax.max(), 1.0)
        assert (np.abs(cap - rsum) <= sbar).all(), (mode, np.abs(cap - rsum), sbar)
        pl, pc, pn = R.score_captions(cfg, ens, encd, caps.tolist())       # the public list form
        assert pn == rlen.tolist() and pc == [float(np.float32(v)) for v in cap] and len(pl) == caps.shape[0]
    print(prec, "+".join(names), "T", caps.shape[0], "worst row error / (3 x row bar):", worst)


# ------------------------------------------------------------------------------------------------ 6. copies of one model
@pytest.mark.parametrize("name,bw", [("search_gru_b", 3), ("search_eos", 3), ("search_gru_b", 8)])
def test_two_copies_decode_like_the_model(name, bw):
    """Both means of a distribution with itself are that distribution: on the captions beam_ref marks comparable for the single
    model the ensemble of two copies, weights (1, 3), returns the model's tokens, and its cum within len x 3 x the row bar."""
    cml = 7
    decs, cfg, inp, hid, encd = device_members((name,), "f32", cml)
    P, cell, enc, dims = ER.load_member(name)
    twin = decoder_for({"meta_dims": dims, "_cell": cell}, P, "f32", cml)[0]      # a second decoder object with the same parameters
    r = BR.beam_search_nbest(P, enc, bw, BR.LENGTH_ALPHA, cml, cell)
    keep = BR.comparable_captions(r)
    assert keep.any()
    t1, c1, l1, _ = search._beam_nbest(cfg, decs[0], inp, hid, encd, bw, BR.LENGTH_ALPHA)
    bar = torch.from_numpy(r["len"] * 3 * SC.row_bar("f32", r["amax"].max(), 1.0)).cuda()
    k = torch.from_numpy(keep).cuda()
    for mode in ER.MODES:
        t2, c2, l2, _ = search._beam_nbest(cfg, R.Ensemble([decs[0], twin], (1, 3), mode), inp, hid, encd, bw, BR.LENGTH_ALPHA)
        n = min(t1.shape[1], t2.shape[1])
        assert torch.equal(t1[:, :n][:, :, k], t2[:, :n][:, :, k]) and torch.equal(l1[:, k], l2[:, k])
        err = (c1.double() - c2.double()).abs()
        print(name, bw, mode, "captions compared", int(keep.sum()), "worst |cum - model's cum| / bar:", float((err / bar)[:, k].max()))
        assert (err <= bar)[:, k].all()


# ------------------------------------------------------------------------------------------------ 7. the public layer
def test_evaluate_and_perplexity_take_an_ensemble():
    names, w = ER.G97, (1, 2)
    decs, cfg, inp, hid, encd = device_members(names)
    ens = R.Ensemble(decs, w, "arithmetic")
    B, V = encd.shape[0], decs[0].output_size
    idx2word = {i: "w%d" % i for i in range(V)}
    vids = ["a", "b", "c", "d", "PAD", "PAD"]
    refs = {k: ["w3 w4 w5", "w7 w8"] for k in "abcd"}
    batches = [(vids, encd.cpu().numpy())]
    con = {"n_groups": 2, "diversity_penalty": 0.5}
    got_nbest = R.evaluate(cfg, batches, ens, ("beam_nbest", 3, 0.7), idx2word, refs)
    got_cons = R.evaluate(cfg, batches, ens, ("beam_consensus", 4, 0.7, 0.5, con), idx2word, refs)
    want_nbest = [h[0][0] for h in R.beam_search_nbest(cfg, ens, inp, hid, encd, 3, 0.7)]
    want_cons = R.best_of_beam(cfg, ens, inp, hid, encd, 4, 0.7, consensus_weight=0.5, **con)[0]
    for got, caps in ((got_nbest, want_nbest), (got_cons, want_cons)):
        res = {v: [metrics.indices_to_sentence(c, idx2word)] for v, c in zip(vids, caps) if v != "PAD"}
        assert isinstance(got, dict) and got and got == metrics.score_all({v: refs[v] for v in res}, res)
    div = R.nbest_diversity(R.beam_search_nbest(cfg, ens, inp, hid, encd, 4, 0.7, **con))
    assert len(div) == B and all(1 <= d[0] <= 4 for d in div)
    # perplexity: exp(-sum caption_logprob / sum length) of the public scorer
    targets = load("search_eos")["greedy"].astype(np.int64)
    _, cap, ln = R.score_captions(cfg, ens, encd, targets.tolist())
    ppl = R.perplexity(cfg, ens, [(encd.cpu().numpy(), targets)])
    assert ppl == pytest.approx(float(np.exp(-np.sum(cap) / np.sum(ln))), rel=1e-12)
    print("ensemble perplexity of search_eos' greedy captions:", ppl)


# ------------------------------------------------------------------------------------------------ 8. every member keeps its own state
@pytest.mark.parametrize("names,w", [(ER.G97, (1, 2)), (ER.G97_ODD, (1, 3)), (ER.G97_3, (1, 2, 3))], ids=lambda v: "+".join(v) if isinstance(v[0], str) else None)
def test_the_order_of_the_members_does_not_matter(names, w):
    """LSTM and GRU members, and members of different hidden sizes, in either order (weights permuted with them): the same
    hypotheses on the captions the restatement marks comparable, cum within twice the bar each order is held to against it.  A
    regather that read another member's rows, or rows of another member's size, would not survive the swap."""
    bw, cml = 3, 7
    models, enc = ER.load_models(names)
    for mode in ER.MODES:
        r = ER.beam_search_nbest(models, enc, bw, ER.LENGTH_ALPHA, cml, w, mode)
        keep = ER.comparable_captions(r)
        assert keep.any()
        outs = []
        for order in (names, names[::-1]):
            decs, cfg, inp, hid, _ = device_members(order, "f32", cml)
            encd = device_members(names, "f32", cml)[4]                    # (the features of the first order's member 0, for both)
            wo = w if order == names else w[::-1]
            toks, cum, ln, _ = search._beam_nbest(cfg, R.Ensemble(decs, wo, mode), inp, hid, encd, bw, ER.LENGTH_ALPHA)
            outs.append((toks.cpu().numpy(), cum.cpu().numpy().astype(np.float64), ln.cpu().numpy()))
            assert np.array_equal(outs[-1][0][:, :, keep], r["tokens"][:, :outs[-1][0].shape[1]][:, :, keep])
        (ta, ca, la), (tb, cb, lb) = outs
        assert np.array_equal(ta[:, :, keep], tb[:, :, keep]) and np.array_equal(la[:, keep], lb[:, keep])
        bar = 2 * r["len"] * 3 * SC.row_bar("f32", r["amax"].max(), 1.0)
        err = np.abs(ca - cb)
        print("+".join(names), mode, "captions compared", int(keep.sum()), "worst |cum - cum swapped| / bar:", float((err / bar)[:, keep].max()))
        assert (err <= bar)[:, keep].all()


# ------------------------------------------------------------------------------------------------ 9. the library's refusals
def test_library_refuses_bad_ensembles_and_recovers():
    Engine, _lib = R.engine.Engine, R.engine._lib
    decs, cfg, inp, hid, encd = device_members(ER.G97, "f32", 7)
    engs = [search._nbest_engine(cfg, d, encd) for d in decs]
    nbest = lambda es, **kw: Engine.beam_search_nbest_ensemble(es, encd, kw.pop("bw", 3), 0.7, **kw)
    good = nbest(engs, weights=(1, 2))
    with pytest.raises(_lib.RecNetError, match="distinct handles"):
        nbest([engs[0], engs[0]])
    with pytest.raises(_lib.RecNetError, match="positive and finite"):
        nbest(engs, weights=(1, float("nan")))
    with pytest.raises(_lib.RecNetError, match="unknown ensemble mode"):
        nbest(engs, mode=2)
    with pytest.raises(_lib.RecNetError, match="beam_width"):
        nbest(engs, bw=9)
    with pytest.raises(_lib.RecNetError, match="n_groups"):
        nbest(engs, bw=4, n_groups=3)
    unbound = Engine(decs[0].dims(encd.shape[0], encd.shape[1]), None, "f32", dict(decs[0].hyper(), caption_max_len=7), device=encd.device)
    with pytest.raises(_lib.RecNetError, match="decoder not bound"):
        nbest([engs[0], unbound])
    small, scfg, _, _, senc = device_members(("search_stop",), "f32", 7)
    other_v = search._nbest_engine(scfg, small[0], senc)                   # (the V = 61 group: another B, D and V)
    other_cml = search._cached_engine(decs[1], encd)                       # (the shared engine: caption_max_len 30)
    for bad in (other_v, other_cml):
        with pytest.raises(_lib.RecNetError, match="must agree"):
            nbest([engs[0], bad])
    caps = good[0][0].contiguous()
    with pytest.raises(_lib.RecNetError, match="distinct handles"):
        Engine.score_captions_ensemble([engs[1], engs[1]], encd, caps)
    with pytest.raises(_lib.RecNetError, match="T out of range"):
        Engine.score_captions_ensemble(engs, encd, torch.zeros(9, encd.shape[0], dtype=torch.long, device="cuda"))
    again = nbest(engs, weights=(1, 2))
    torch.cuda.synchronize()
    assert same(good, again)
    # the ctypes face and the op face of the two entries agree
    ens = R.Ensemble(decs, (1, 2), "arithmetic")
    t, c, l, s = search._beam_nbest(cfg, ens, inp, hid, encd, 3, 0.7)
    n = t.shape[1]
    assert same([good[0][:, :n], good[1], good[2], good[3]], [t, c, l, s])
    assert same(Engine.score_captions_ensemble(engs, encd, caps, (1, 2)), search._score(ens, encd, caps, 1.0, False, 7))
