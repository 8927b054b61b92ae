"""Caption scoring on the device (recnet_logprob_rows / recnet_score_captions, search.score_captions / best_of_n,
loop.perplexity) against the CPU restatement (tests/score_ref.py), the reference's own eval-mode logits, and the sampler's
log-probabilities of the tokens it drew.

Bars (tests/score_ref.py: row_bar): one log-probability is a logit minus a log-sum-exp of logits, each within the per-step logits
bar of tests/test_gpu_parity.py, so 2 * TOL[prec]["hid"] * 4 * max(1, max |logit|) / temperature; a caption sum gets its length
times that; two device kernels compared with each other get twice the row bar.  Every test prints its worst error / bar;
the ratios of one MI355X run are in DESIGN.md section 9 (all below 0.02; scorer and sampler return the same bits in fp32)."""
import functools

import numpy as np
import pytest
import torch

import recnet_amd as R
from recnet_amd.engine import Engine, _lib      # the engine's own _lib: the module whose RecNetError it raises
from tests import golden_util as GU
from tests import score_ref as SC
from tests.golden_util import CASES, load_search_case
from tests.gpu_util import load_case, make_models
from tests.search_kit import bound_engine, decoder_for, rows_engine

pytestmark = pytest.mark.gpu


def _dims_decoder(P, dims7, cell, prec):
    """search_kit.decoder_for on bare dims and a cell instead of a search golden."""
    return decoder_for({"meta_dims": dims7, "_cell": cell}, P, prec)


def _first_eos_lengths(tokens):
    tokens = np.asarray(tokens)
    T, B = tokens.shape
    return np.array([next((t + 1 for t in range(T) if tokens[t, b] == 2), T) for b in range(B)])


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("V", SC.ROW_VS)
def test_logprob_rows(V):
    """Gaussian, Gaussian x 60 and quantised logits, rows 1 and 7, three temperatures; tokens 0, V - 1, the arg-max, -1 and V:
    in-range results finite and within the fp32 row bar of the float64 restatement, out-of-range ones -inf, V = 1 exactly 0, the
    logits bit-identical afterwards."""
    eng = rows_engine()
    worst = 0.0
    seen_out = 0
    for rows, kind, temperature, shift in SC.row_cases(V):
        x = SC.row_logits(V, rows, kind)
        tok = SC.row_case_tokens(x, shift)
        xd = torch.from_numpy(x).cuda()
        before = xd.clone()
        lp = eng.logprob_rows(xd, torch.from_numpy(tok).cuda(), temperature)
        torch.cuda.synchronize()
        assert torch.equal(xd.view(torch.int32), before.view(torch.int32)), (rows, kind, temperature)
        lp = lp.cpu().numpy()
        ok = (tok >= 0) & (tok < V)
        seen_out += int((~ok).sum())
        assert lp.dtype == np.float32 and np.isneginf(lp[~ok]).all(), (rows, kind, temperature, lp, tok)
        assert np.isfinite(lp[ok]).all() and (lp[ok] <= 0).all(), (rows, kind, temperature, lp, tok)
        if V == 1:
            assert (lp[ok] == 0.0).all()
        if ok.any():
            ref = SC.logprob_rows(x, tok, temperature)
            err = np.abs(lp[ok].astype(np.float64) - ref[ok])
            bar = SC.row_bar("f32", np.abs(x[ok]).max(), temperature)
            worst = max(worst, float(err.max() / bar))
            assert err.max() <= bar, (rows, kind, temperature, float(err.max()), bar)
    assert seen_out > 0
    print("V", V, "worst log-probability error / bar:", worst)


# ------------------------------------------------------------------------------------------------ 2. eval goldens, fp32
@pytest.mark.parametrize("name", SC.EVAL_GOLDENS)
def test_eval_goldens_f32(name):
    """Targets as captions: device logprobs against log_softmax(step_logits)[target] of the reference's own logits on every row up to
    the caption's <EOS>; caption sums and lengths against the restatement."""
    g, dims, kind, decP, recP, enc, targets = load_case(name)
    cell = g["_cells"][0]
    T = g["step_logits"].shape[0]
    caps = targets[:T].contiguous()
    dec, _, _, _ = _dims_decoder(decP, dims[:7], cell, "f32")
    eng = bound_engine(dec, dims[0], dims[1], "f32")
    lps, cap, ln = (x.cpu().numpy() for x in eng.score_captions(enc.cuda(), caps.cuda(), 1.0))
    ref = SC.golden_logprobs(g["step_logits"], caps.numpy())
    rlp, amax = SC.score_captions(decP, enc, caps.numpy(), 1.0, cell=cell)
    rsum, rlen = SC.caption_sums(rlp, caps.numpy())
    assert lps.shape == (T, dims[0]) and ln.dtype == np.int32 and np.array_equal(ln, rlen)
    worst = 0.0
    for t in range(T):
        live = rlen > t
        err = np.abs(lps[t] - ref[t])[live]
        bar = SC.row_bar("f32", np.abs(g["step_logits"][t]).max(), 1.0)
        if err.size:
            worst = max(worst, float(err.max() / bar))
            assert err.max() <= bar, (t, float(err.max()), bar)
    sbar = rlen * SC.row_bar("f32", amax.max(), 1.0)
    serr = np.abs(cap - rsum)
    worst_s = float((serr / sbar).max())
    assert (serr <= sbar).all(), (serr, sbar)
    print(name, "T", T, "worst row error / bar:", worst, "worst caption-sum error / bar:", worst_s)


# ------------------------------------------------------------------------------------------------ 3. scorer and sampler, fp32
@pytest.mark.parametrize("temperature", [1.0, 0.7])
@pytest.mark.parametrize("name", CASES)
def test_scorer_and_sampler_agree_f32(name, temperature):
    """sample_search(top_k = 0) rollouts re-scored at the same temperature: per-step values equal the sampler's on all n_steps rows
    within twice the row bar (two kernels, each within it), caption sums equal sequence_logprob within length times that; the
    scorer also meets the single row bar against the restatement.  The *_stop goldens give T = 1."""
    g, P, enc = load_search_case(name)
    dims7 = [int(x) for x in g["meta_dims"]]
    dec, cfg, inp, hid = _dims_decoder(P, dims7, g["_cell"], "f32")
    encd = enc.cuda()
    toks, lps = R.sample_search(cfg, dec, inp, hid, encd, temperature=temperature, top_k=0, seed=3)
    n = len(toks)
    if name.endswith("_stop"):
        assert n == 1
    slp, scap, slen = R.score_captions(cfg, dec, encd, toks, temperature)
    slp, lps = np.array(slp, dtype=np.float64), np.array(lps, dtype=np.float64)
    assert slp.shape == lps.shape == (n, dims7[0])
    assert slen == _first_eos_lengths(toks).tolist()
    rlp, amax = SC.score_captions(P, enc, toks, temperature, cell=g["_cell"])
    worst = worst_r = 0.0
    for t in range(n):
        bar = SC.row_bar("f32", amax[t], temperature)
        err, err_r = np.abs(slp[t] - lps[t]).max(), np.abs(slp[t] - rlp[t]).max()
        worst, worst_r = max(worst, float(err / (2 * bar))), max(worst_r, float(err_r / bar))
        assert err <= 2 * bar, (t, float(err), 2 * bar)
        assert err_r <= bar, (t, float(err_r), bar)
    seq = np.array(R.sequence_logprob(toks, lps.tolist()))
    sbar = np.array(slen) * 2 * SC.row_bar("f32", amax.max(), temperature)
    serr = np.abs(np.array(scap) - seq)
    assert (serr <= sbar).all(), (serr, sbar)
    print(name, temperature, "steps", n, "scorer vs sampler / (2 bar):", worst, "scorer vs restatement / bar:", worst_r,
          "caption sums / bar:", float((serr / sbar).max()))


# ------------------------------------------------------------------------------------------------ 4. bf16, persistent chain
CHAIN_CASES = ("lr_global_chain", "full_dec_B8")      # (B 24, F 6, D 64, V 61, E 16, H 32, A 16) and (B 8, V 4188, H 512)


@functools.lru_cache(maxsize=None)
def _chain_case(name):
    g, dims, kind, decP, recP, enc, targets = load_case(name)
    cell = g["_cells"][0]
    caps = targets.contiguous()
    rlp, amax = SC.score_captions(decP, enc, caps.numpy(), 1.0, cell=cell)
    rsum, rlen = SC.caption_sums(rlp, caps.numpy())
    return dims[:7], cell, decP, enc, caps, rlp, amax, rsum, rlen


@pytest.mark.parametrize("per_step", [False, True], ids=["chain", "per_step"])
@pytest.mark.parametrize("name", CHAIN_CASES)
def test_bf16_chain_and_per_step(name, per_step, monkeypatch):
    """The goldens' targets as captions on the bf16 path: one launch of the persistent decoder chain (counted through the profile
    site), resp. the per-step kernels when the engine is created under RN_PER_STEP=dec — both within the bf16 row bar of the
    restatement."""
    if per_step:
        monkeypatch.setenv("RN_PER_STEP", "dec")
    dims7, cell, decP, enc, caps, rlp, amax, rsum, rlen = _chain_case(name)
    dec, _, _, _ = _dims_decoder(decP, dims7, cell, "bf16")
    eng = bound_engine(dec, dims7[0], dims7[1], "bf16")
    encd, capd = enc.cuda(), caps.cuda()
    out = []
    n_chain = eng.profile_site(9, lambda: out.append(eng.score_captions(encd, capd, 1.0)), 1)[0]      # RECNET_SITE_DEC_CHAIN_FWD
    assert (n_chain == 0) if per_step else (n_chain >= 1), n_chain
    assert eng.chain_status() == 0
    lps, cap, ln = (x.cpu().numpy() for x in out[0])
    assert np.array_equal(ln, rlen)
    worst = 0.0
    for t in range(caps.shape[0]):
        bar = SC.row_bar("bf16", amax[t], 1.0)
        err = np.abs(lps[t] - rlp[t]).max()
        worst = max(worst, float(err / bar))
        assert err <= bar, (t, float(err), bar)
    sbar = rlen * SC.row_bar("bf16", amax.max(), 1.0)
    serr = np.abs(cap - rsum)
    assert (serr <= sbar).all(), (serr, sbar)
    print(name, "per-step" if per_step else "chain", "launches", n_chain, "worst row error / bar:", worst,
          "worst caption-sum error / bar:", float((serr / sbar).max()))


@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_bf16_sampler_rollouts_rescored_through_the_chain(temperature):
    """lr_global_chain's decoder, bf16: the sampler runs the per-step kernels, the scorer the persistent chain; on the sampler's
    own tokens the two agree within twice the bf16 row bar."""
    dims7, cell, decP, enc, _, _, _, _, _ = _chain_case("lr_global_chain")
    dec, cfg, inp, hid = _dims_decoder(decP, dims7, cell, "bf16")
    encd = enc.cuda()
    toks, lps = R.sample_search(cfg, dec, inp, hid, encd, temperature=temperature, top_k=0, seed=5)
    slp, scap, slen = R.score_captions(cfg, dec, encd, toks, temperature)
    _, amax = SC.score_captions(decP, enc, toks, temperature, cell=cell)
    slp, lps = np.array(slp, dtype=np.float64), np.array(lps, dtype=np.float64)
    worst = 0.0
    for t in range(len(toks)):
        bar = 2 * SC.row_bar("bf16", amax[t], temperature)
        err = np.abs(slp[t] - lps[t]).max()
        worst = max(worst, float(err / bar))
        assert err <= bar, (t, float(err), bar)
    assert slen == _first_eos_lengths(toks).tolist()
    print("bf16", temperature, "steps", len(toks), "scorer (chain) vs sampler (per-step) / (2 bar):", worst)


# ------------------------------------------------------------------------------------------------ 5. shared invariants, determinism
@pytest.mark.parametrize("which", ["f32_per_step", "bf16_chain"])
def test_shared_invariants_and_determinism(which):
    """score(enc, A) then score(None, B) equals score(enc, B) bit for bit; two identical calls are bit-identical; the Python mirror's
    reuse_features does the same; a greedy search returns the same tokens before and after scoring."""
    if which == "f32_per_step":
        g, P, enc = load_search_case("search_small")
        dims7, cell, prec = [int(x) for x in g["meta_dims"]], g["_cell"], "f32"
    else:
        dims7, cell, P, enc = _chain_case("lr_global_chain")[:4]
        prec = "bf16"
    B, F, V = dims7[0], dims7[1], dims7[3]
    dec, cfg, inp, hid = _dims_decoder(P, dims7, cell, prec)
    encd = enc.cuda()
    greedy = R.greedy_search(cfg, dec, inp, hid, encd)
    rs = np.random.RandomState(3)
    A = torch.from_numpy(rs.randint(0, V, size=(9, B))).cuda()
    Bt = torch.from_numpy(rs.randint(0, V, size=(31, B))).cuda()
    eng = bound_engine(dec, B, F, prec)
    eng.score_captions(encd, A)
    reuse = eng.score_captions(None, Bt)
    full = eng.score_captions(encd, Bt)
    again = eng.score_captions(encd, Bt)
    torch.cuda.synchronize()
    for x, y, z in zip(reuse, full, again):
        assert torch.equal(x, y) and torch.equal(y, z)
    assert torch.isfinite(full[0]).all() and torch.isfinite(full[1]).all()
    # the Python mirror: lists in, lists out, the same numbers
    R.score_captions(cfg, dec, encd, A.cpu().tolist())
    py_reuse = R.score_captions(cfg, dec, encd, Bt.cpu().tolist(), reuse_features=True)
    py_full = R.score_captions(cfg, dec, encd, Bt)
    assert py_reuse == py_full
    assert py_full[0] == full[0].cpu().tolist() and py_full[1] == full[1].cpu().tolist() and py_full[2] == full[2].cpu().tolist()
    assert R.greedy_search(cfg, dec, inp, hid, encd) == greedy


# ------------------------------------------------------------------------------------------------ 6. state and argument errors
def test_state_and_argument_errors():
    dims = [4, 5, 40, 37, 10, 24, 16, 16]
    B, F, D, V, E, H, A, RA = dims
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D), 1)
    recP = GU.formula_params(GU.rec_shapes("global", H, D, RA), 2)
    _, dec, rec = make_models(dims, "global", "f32", decP, recP)
    step = R.TrainStep(dec, rec)
    eng = step.engine
    enc, tg = GU.make_batch(B, F, D, V, [3, 1, 4, 2], 3)
    encd, tgd = enc.cuda(), tg.cuda()
    T, w = step.prepare(tg.numpy())
    # a scoring pass overwrites the saved forward: the backward is refused, never run on it
    eng.forward_decoder(encd, tgd, T, w, train=True, seed=1)
    first = eng.score_captions(encd, tgd[:T].contiguous())
    with pytest.raises(_lib.RecNetError, match="before forward"):
        eng.backward_decoder(encd, tgd, None, 1.0)
    with pytest.raises(_lib.RecNetError, match="no decoder hidden states"):
        eng.forward_reconstructor(encd, None, T)
    with pytest.raises(_lib.RecNetError, match="T out of range"):
        eng.score_captions(encd, torch.zeros(0, B, dtype=torch.long, device="cuda"))
    with pytest.raises(_lib.RecNetError, match="T out of range"):
        eng.score_captions(encd, torch.zeros(32, B, dtype=torch.long, device="cuda"))
    for bad in (0.0, float("nan"), float("inf"), -1.0):
        with pytest.raises(_lib.RecNetError, match="temperature must be positive and finite"):
            eng.score_captions(encd, tgd[:T].contiguous(), bad)
        with pytest.raises(_lib.RecNetError, match="temperature must be positive and finite"):
            eng.logprob_rows(torch.zeros(2, V, device="cuda"), torch.zeros(2, dtype=torch.long, device="cuda"), bad)
    unbound = Engine(dict(B=B, F=F, D=D, E=E, H=H, A=A, V=V), None, "f32")
    with pytest.raises(_lib.RecNetError, match="decoder not bound"):
        unbound.score_captions(encd, tgd[:T].contiguous())
    # the next valid calls succeed: the same scores, and a forward + backward pair
    second = eng.score_captions(encd, tgd[:T].contiguous())
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    eng.forward_decoder(encd, tgd, T, w, train=True, seed=1)
    eng.backward_decoder(encd, tgd, None, 1.0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. best_of_n / evaluate / perplexity
@functools.lru_cache(maxsize=None)
def _corpus():
    """The tiny corpus of tests/test_gpu_sample.py::test_evaluate_accepts_the_sample_method."""
    from recnet_amd import feed
    V = 41
    C = R.make_config(use_recon=True, reconstructor_type="local", batch_size=6, encoder_output_len=5, encoder_output_size=32,
                      embedding_size=12, decoder_hidden_size=24, decoder_attn_size=8, reconstructor_hidden_size=32,
                      reconstructor_attn_size=8, precision="f32")
    torch.manual_seed(1)
    model = R.build_decoder(V, C)["model"]
    rng = np.random.RandomState(9)
    vids = [rng.randn(5, 32).astype(np.float32) for _ in range(6)]
    caps = [feed.pad_caption(rng.randint(3, V, size=4), 30) for _ in range(6)]
    enc, targets = feed.collate_batch(vids, caps, 6)
    idx2word = {i: "w%d" % i for i in range(V)}
    names = ["a", "b", "c", "d", "PAD", "PAD"]
    refs = {k: ["w3 w4 w5", "w7 w8"] for k in "abcd"}
    return C, model, enc, targets, idx2word, names, refs


def test_evaluate_accepts_the_best_of_method():
    C, model, enc, _, idx2word, names, refs = _corpus()
    ev = lambda method: R.evaluate(C, [(names, enc)], model, method, idx2word, refs)
    assert ev(("best_of", 1, 0.8, 5, 3)) == ev(("sample", 0.8, 5, 3))            # one candidate: the sample itself
    assert ev(("best_of", 3, 1.0, 1, 0)) == ev("greedy")                         # top_k = 1: every candidate is the arg-max
    assert set(ev(("best_of", 4, 1.0, 0, 2))) == set(ev("greedy"))
    with pytest.raises(NotImplementedError):
        ev(("nucleus", 0.9))
    with pytest.raises(NotImplementedError):
        ev("best_of")


def test_best_of_n_equals_a_host_recomputation():
    """n = 4: the chosen candidates and scores equal what four separate sample_search + score_captions calls (invariants recomputed
    every time) give under the selection rule — the shared invariants change nothing."""
    C, model, enc, _, _, _, _ = _corpus()
    B, H = C.batch_size, model.hidden_size
    encd = torch.from_numpy(enc).cuda()
    inp = torch.full((1, B), 1, dtype=torch.long, device="cuda")
    hid = (torch.zeros(1, B, H, device="cuda"), torch.zeros(1, B, H, device="cuda"))
    model.eval()
    caps, ks, scores = R.best_of_n(C, model, inp, hid, encd, 4, temperature=1.0, top_k=0, seed=0xFFFFFFFE)      # seeds wrap
    cands, sums, lens = [], [], []
    for k in range(4):
        toks, _ = R.sample_search(C, model, inp, hid, encd, 1.0, 0, (0xFFFFFFFE + k) & 0xFFFFFFFF)
        _, cap, ln = R.score_captions(C, model, encd, toks)
        cands.append(toks); sums.append(cap); lens.append(ln)
    rk, rscores = R.pick_best_of_n(sums, lens)
    assert ks == rk and scores == rscores
    assert cands[0] != cands[1]                                                     # different seeds, different rollouts
    for b in range(B):
        want = [cands[ks[b]][t][b] for t in range(lens[ks[b]][b])]
        assert caps[b] == want and (want[-1] == 2 or len(want) == len(cands[ks[b]]))
        assert all(scores[b] >= sums[k][b] / lens[k][b] for k in range(4))
    print("best of 4: chosen", ks, "scores", scores)


def test_perplexity_equals_the_restatement():
    C, model, enc, targets, _, _, _ = _corpus()
    ppl = R.perplexity(C, model, [(enc, targets), (enc, targets)])
    P = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    rlp, amax = SC.score_captions(P, torch.from_numpy(enc), targets, 1.0, cell="LSTM")
    rsum, rlen = SC.caption_sums(rlp, targets)
    ref = float(np.exp(-rsum.sum() / rlen.sum()))
    # |sum_dev - sum_ref| <= sum_b length_b * row bar, so the mean per-token log-probability is within one row bar
    bar = SC.row_bar("f32", amax.max(), 1.0)
    err = abs(np.log(ppl) - np.log(ref))
    print("perplexity", ppl, "restatement", ref, "log error / bar:", err / bar)
    assert rlen.tolist() == [5] * 6 and 1.0 < ref < 41.0 ** 2
    assert err <= bar, (ppl, ref, err, bar)
