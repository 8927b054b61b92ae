"""Consensus (minimum-Bayes-risk) reranking on the device (recnet_consensus_rows) against the float64
restatement with Counters (tests/consensus_ref.py): the kernel alone on host-made caption sets, the two searches that rerank with
it on the goldens' decoders in both precisions, evaluate(), and the argument checks of the library.

The integers (M_n, Q_n, L) must equal the restatement exactly.  sim and util are held to 1e-12 absolute: every value lies in
[0, 1], and at most 32 terms of about 10 roundings at 1.1e-16 each stay below 1e-13; the bar is one order above that.  Every test
prints its worst error / bar."""
import functools

import numpy as np
import pytest
import torch

import recnet_amd as R
from recnet_amd import _ops, metrics, search
from tests import consensus_ref as CR
from tests import golden_util as GU
from tests.golden_util import load_search_case
from tests.gpu_util import make_models
from tests.search_kit import decoder_for, rows_engine

pytestmark = pytest.mark.gpu

Engine, _lib = R.engine.Engine, R.engine._lib
INTS = ("counts", "q_hyp", "q_ref", "len_hyp", "len_ref")


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
@functools.lru_cache(maxsize=None)
def _case(shape, vocab):
    """The case, its restatement without weights and with them: computed once, shared, never written to."""
    c = CR.make_case(shape, vocab)
    return c, CR.consensus(c["hyp"], c["ref"]), CR.consensus(c["hyp"], c["ref"], c["weights"])


def _dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


def _bits(t):
    return t.view(torch.int64)


@pytest.mark.parametrize("vocab", sorted(CR.VOCABS))
@pytest.mark.parametrize("shape", CR.SHAPES, ids=CR.case_id)
def test_kernel_against_the_restatement(shape, vocab):
    eng = rows_engine()
    c, want, want_w = _case(shape, vocab)
    hyp, ref, w = _dev(c["hyp"]), _dev(c["ref"]), _dev(c["weights"])
    hyp0, ref0 = hyp.clone(), None if ref is None else ref.clone()
    util, sim, ints = eng.consensus_rows(hyp, ref, want_sim=True, want_counts=True)
    util2, sim2, ints2 = eng.consensus_rows(hyp, ref, want_sim=True, want_counts=True)
    alone = eng.consensus_rows(hyp, ref)
    util_w, sim_w = eng.consensus_rows(hyp, ref, weights=w, want_sim=True)
    op = _ops.load().consensus_rows(int(eng.handle.value), hyp, ref, w, 6.0, True, True)
    torch.cuda.synchronize()
    # the inputs are untouched; a second call, the call without the optional outputs and the custom op give the same bits
    assert torch.equal(hyp, hyp0) and (ref is None or torch.equal(ref, ref0))
    assert torch.equal(_bits(util), _bits(util2)) and torch.equal(_bits(sim), _bits(sim2)) and torch.equal(_bits(util), _bits(alone))
    assert all(torch.equal(ints[k], ints2[k]) for k in INTS)
    assert torch.equal(_bits(op[0]), _bits(util_w)) and torch.equal(_bits(op[1]), _bits(sim)) and torch.equal(_bits(sim_w), _bits(sim))
    assert all(torch.equal(o, ints[k]) for o, k in zip(op[2:], INTS))
    # the integers: exactly the restatement's
    for k in INTS:
        assert np.array_equal(ints[k].cpu().numpy().astype(np.int64), want[k]), k
    if shape[2] == 64:
        assert want["q_hyp"].max() == 4096                      # one word 64 times is among the columns
    # sim and util, without and with weights
    e_sim = float(np.abs(sim.cpu().numpy() - want["sim"]).max())
    e_u = float(np.abs(util.cpu().numpy() - want["util"]).max())
    e_w = float(np.abs(util_w.cpu().numpy() - want_w["util"]).max())
    print(CR.case_id(shape), vocab, "worst sim error / bar:", e_sim / CR.BAR, "util:", e_u / CR.BAR, "weighted util:", e_w / CR.BAR)
    assert e_sim <= CR.BAR and e_u <= CR.BAR and e_w <= CR.BAR
    assert float(sim.min()) >= 0.0 and float(sim.max()) <= 1.0
    # copied columns: bit-equal utilities
    for k1, k2, b in c["copies"]:
        assert np.array_equal(c["hyp"][k1, :, b], c["hyp"][k2, :, b])
        assert _bits(util)[k1, b] == _bits(util)[k2, b] and _bits(util_w)[k1, b] == _bits(util_w)[k2, b], (k1, k2, b)
    assert c["copies"] or shape[0] == 1
    # no references = the hypotheses passed as references, to the bit
    if ref is None:
        e_util, e_sim2, e_ints = eng.consensus_rows(hyp, hyp.clone(), want_sim=True, want_counts=True)
        assert torch.equal(_bits(e_util), _bits(util)) and torch.equal(_bits(e_sim2), _bits(sim))
        assert all(torch.equal(e_ints[k], ints[k]) for k in INTS)
        assert torch.equal(ints["q_hyp"], ints["q_ref"]) and torch.equal(ints["len_hyp"], ints["len_ref"])
        d = torch.arange(shape[0])
        full = ints["len_hyp"] > 3                               # a caption against itself: 1 from four words on, n / 4 below
        assert (sim[d, d][full] == 1.0).all()


def test_hand_case_on_the_device():
    H = CR.HAND
    hyp = np.full((3, 6, 1), CR.EOS, np.int64)
    hyp[0, :, 0], hyp[1, :5, 0], hyp[2, :, 0] = CR.HAND_H, CR.HAND_R, CR.HAND_H
    util, sim, ints = rows_engine().consensus_rows(_dev(hyp), want_sim=True, want_counts=True)
    assert ints["counts"][0, 1, 0].tolist() == H["M"] and ints["q_hyp"][0, 0].tolist() == H["Qh"] and ints["q_ref"][1, 0].tolist() == H["Qr"]
    got = [sim[0, 1, 0].item(), sim[1, 0, 0].item(), sim[0, 0, 0].item()] + util[:, 0].tolist()
    exp = [H["sim_hr"], H["sim_rh"], H["sim_hh"]] + list(H["util"])
    err = max(abs(g - e) for g, e in zip(got, exp))
    print("hand case: worst error / bar:", err / CR.BAR)
    assert err <= CR.BAR and sim[0, 0, 0].item() == 1.0 and _bits(util)[0, 0] == _bits(util)[2, 0]


def test_library_refuses_bad_arguments_and_recovers():
    eng = rows_engine()
    hyp = _dev(CR.make_case((2, None, 4, None, 3), "forty")["hyp"])
    good = eng.consensus_rows(hyp)
    z = lambda *s: torch.zeros(*s, dtype=torch.long, device="cuda")
    for bad, match in ((z(33, 4, 3), "N_h"), (z(2, 65, 3), "T_h")):
        with pytest.raises(_lib.RecNetError, match=match):
            eng.consensus_rows(bad)
        with pytest.raises(_lib.RecNetError, match=match.replace("h", "r")):
            eng.consensus_rows(hyp, bad)
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.RecNetError, match="sigma"):
            eng.consensus_rows(hyp, sigma=sigma)
    with pytest.raises(RuntimeError):
        eng.consensus_rows(hyp, z(2, 4, 4))                      # B disagrees
    with pytest.raises(RuntimeError):
        eng.consensus_rows(hyp.int())
    with pytest.raises(RuntimeError):
        eng.consensus_rows(hyp, weights=torch.ones(3, 3, device="cuda"))
    lib = eng.lib
    args = (None, 6.0, good.data_ptr(), None, None, None, None, None, None, None)
    assert lib.recnet_consensus_rows(eng.handle, None, 2, 4, None, 2, 4, 3, *args) == -1 and b"null" in lib.recnet_last_error()
    assert lib.recnet_consensus_rows(eng.handle, hyp.data_ptr(), 2, 4, None, 0, 0, 0, *args) == -1 and b"B must" in lib.recnet_last_error()
    assert lib.recnet_consensus_rows(eng.handle, hyp.data_ptr(), 0, 4, None, 2, 4, 3, *args) == -1 and b"N_h" in lib.recnet_last_error()
    ops, h = _ops.load(), int(eng.handle.value)
    for bad_call in (lambda: ops.consensus_rows(h, z(33, 4, 3), None, None, 6.0, False, False),
                     lambda: ops.consensus_rows(h, hyp, z(2, 65, 3), None, 6.0, False, False),
                     lambda: ops.consensus_rows(h, hyp, z(2, 4, 4), None, 6.0, False, False),
                     lambda: ops.consensus_rows(h, hyp, None, torch.ones(3, 3, device="cuda"), 6.0, False, False),
                     lambda: ops.consensus_rows(h, hyp, None, None, 0.0, False, False),
                     lambda: ops.consensus_rows(h, hyp.cpu(), None, None, 6.0, False, False)):
        with pytest.raises((RuntimeError, NotImplementedError)):
            bad_call()
    again = eng.consensus_rows(hyp)
    torch.cuda.synchronize()
    assert torch.equal(_bits(good), _bits(again))


# ------------------------------------------------------------------------------------------------ 2. the searches
def _against_restatement(sets, util):
    """|util - restatement| of host caption sets (lists [T_k][B], continued with <EOS> as consensus_scores does)."""
    T = max(len(s) for s in sets)
    hyp = np.stack([np.array(list(s) + [[CR.EOS] * len(s[0])] * (T - len(s)), np.int64) for s in sets])
    return float(np.abs(np.array(util) - CR.consensus(hyp)["util"]).max())


@pytest.mark.parametrize("name", ["search_small", "search_gru"])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_best_of_n_with_the_consensus_term(name, prec, monkeypatch):
    g, P, enc = load_search_case(name)
    dec, cfg, inp, hid = decoder_for(g, P, prec)
    encd = enc.cuda()
    n, temp, top_k, seed, cw = 4, 1.3, 0, 5, 0.5
    got = R.best_of_n(cfg, dec, inp, hid, encd, n, temp, top_k, seed, consensus_weight=cw)
    # the tables, rebuilt from the public calls
    cands = [R.sample_search(cfg, dec, inp, hid, encd, temp, top_k, seed + k)[0] for k in range(n)]
    scored = [R.score_captions(cfg, dec, encd, c) for c in cands]
    caps, lens = [s[1] for s in scored], [s[2] for s in scored]
    U = R.consensus_scores(cands, device=encd.device)
    ks, scores = R.pick_best_of_n(caps, lens, None, 0.0, U, cw)
    assert got[1] == ks and got[2] == scores
    assert got[0] == [[cands[k][t][b] for t in range(lens[k][b])] for b, k in enumerate(ks)]
    err = _against_restatement(cands, U)
    plain = R.best_of_n(cfg, dec, inp, hid, encd, n, temp, top_k, seed)
    print(name, prec, "best of", n, ": chosen with the consensus term", ks, "without", plain[1], "worst util error / bar:", err / CR.BAR)
    assert err <= CR.BAR
    # weight 0: the parent's outputs to the bit, and nothing of the consensus is touched
    def boom(*a, **k):
        raise AssertionError("consensus_weight = 0 asked for the consensus engine")
    monkeypatch.setattr(search, "_consensus_engine", boom)
    assert R.best_of_n(cfg, dec, inp, hid, encd, n, temp, top_k, seed, consensus_weight=0.0) == plain
    assert R.best_of_n(cfg, dec, inp, hid, encd, n, temp, top_k, seed, consensus_weight=0) == plain


@pytest.mark.parametrize("name", ["search_small", "search_gru"])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_best_of_beam_with_the_consensus_term(name, prec, monkeypatch):
    g, P, enc = load_search_case(name)
    dec, cfg, inp, hid = decoder_for(g, P, prec)
    encd = enc.cuda()
    bw, cw = 8, 0.5
    worst = 0.0
    for div in (dict(), dict(n_groups=4, diversity_penalty=1.0)):
        got = R.best_of_beam(cfg, dec, inp, hid, encd, bw, 0.7, consensus_weight=cw, **div)
        toks, cum, ln, _ = search._beam_nbest(cfg, dec, inp, hid, encd, bw, 0.7, **div)
        U = R.consensus_scores(toks.contiguous())
        lens, tl = ln.cpu().tolist(), toks.cpu().tolist()
        ks, scores = R.pick_best_of_n(cum.cpu().tolist(), lens, None, 0.0, U, cw)
        assert got[1] == ks and got[2] == scores
        assert got[0] == [[tl[k][t][b] for t in range(lens[k][b])] for b, k in enumerate(ks)]
        worst = max(worst, float(np.abs(np.array(U) - CR.consensus(toks.cpu().numpy())["util"]).max()))
        plain = R.best_of_beam(cfg, dec, inp, hid, encd, bw, 0.7, **div)
        print(name, prec, div, "ranks chosen with the consensus term", ks, "without", plain[1])
        with monkeypatch.context() as m:
            m.setattr(search, "_consensus_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("weight 0 asked for the engine")))
            assert R.best_of_beam(cfg, dec, inp, hid, encd, bw, 0.7, consensus_weight=0.0, **div) == plain
    print(name, prec, "worst util error / bar:", worst / CR.BAR)
    assert worst <= CR.BAR


# ------------------------------------------------------------------------------------------------ 3. with a reconstructor; evaluate
@pytest.mark.parametrize("kind", ["global", "local"])
def test_reconstructor_combined_and_evaluate(kind):
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
    bw, rw, cw = 8, 256.0, 0.5
    div = dict(n_groups=4, diversity_penalty=1.0)
    # all three terms: cum / length - recon_weight * rec_error + consensus_weight * U
    toks, cum, ln, _ = search._beam_nbest(Cfg, dm, inp, hid, encd, bw, 0.7, **div)
    errs = [R.reconstruction_errors(Cfg, dm, rm, encd, toks[k].contiguous(), T=toks.shape[1]) for k in range(bw)]
    U = R.consensus_scores(toks.contiguous())
    ks, scores = R.pick_best_of_n(cum.cpu().tolist(), ln.cpu().tolist(), errs, rw, U, cw)
    got = R.best_of_beam(Cfg, dm, inp, hid, encd, bw, 0.7, reconstructor=rm, recon_weight=rw, consensus_weight=cw, **div)
    assert got[1] == ks and got[2] == scores
    lens, tl = ln.cpu().tolist(), toks.cpu().tolist()
    assert got[0] == [[tl[k][t][b] for t in range(lens[k][b])] for b, k in enumerate(ks)]
    n, temp, top_k, seed = 4, 1.2, 6, 3
    cands = [R.sample_search(Cfg, dm, inp, hid, encd, temp, top_k, seed + k)[0] for k in range(n)]
    scored = [R.score_captions(Cfg, dm, encd, c) for c in cands]
    t_star = max(len(c) for c in cands)
    errs_n = [R.reconstruction_errors(Cfg, dm, rm, encd, c, T=t_star) for c in cands]
    U_n = R.consensus_scores(cands, device=encd.device)
    want_n = R.pick_best_of_n([s[1] for s in scored], [s[2] for s in scored], errs_n, rw, U_n, cw)
    got_n = R.best_of_n(Cfg, dm, inp, hid, encd, n, temp, top_k, seed, rm, rw, consensus_weight=cw)
    assert (got_n[1], got_n[2]) == want_n
    print(kind, "beam ranks chosen", ks, "samples chosen", got_n[1])
    # evaluate: the two new methods are the direct calls
    idx2word = {i: "w%d" % i for i in range(V)}
    names = ["a", "b", "c", "d", "PAD", "PAD"]
    refs = {k: ["w3 w4 w5", "w7 w8"] for k in "abcd"}
    ev = lambda method: R.evaluate(Cfg, [(names, enc.numpy())], dm, method, idx2word, refs)

    def scores_of(caps):
        res = {v: [metrics.indices_to_sentence(c, idx2word)] for v, c in zip(names, caps) if v != "PAD"}
        return metrics.score_all({v: refs[v] for v in res}, res)
    assert ev(("best_of_consensus", n, temp, top_k, seed, cw)) == scores_of(R.best_of_n(Cfg, dm, inp, hid, encd, n, temp, top_k, seed, consensus_weight=cw)[0])
    assert ev(("best_of_consensus", n, temp, top_k, seed, cw, 0.9)) == scores_of(R.best_of_n(Cfg, dm, inp, hid, encd, n, temp, top_k, seed, top_p=0.9, consensus_weight=cw)[0])
    assert ev(("beam_consensus", bw, 0.7, cw)) == scores_of(R.best_of_beam(Cfg, dm, inp, hid, encd, bw, 0.7, consensus_weight=cw)[0])
    assert ev(("beam_consensus", bw, 0.7, cw, div)) == scores_of(R.best_of_beam(Cfg, dm, inp, hid, encd, bw, 0.7, consensus_weight=cw, **div)[0])
    assert ev(("beam_consensus", bw, 1.0, 0.0, div)) == ev(("beam_nbest", bw, 1.0, div))
    with pytest.raises(ValueError):
        ev(("beam_consensus", bw, 0.7))
    with pytest.raises(ValueError, match="consensus_weight"):
        ev(("best_of_consensus", n, temp, top_k, seed, float("nan")))
