"""Sampling on the device (recnet_sample_rows / recnet_sample_search) against the CPU restatement of the draw
(tests/sample_ref.py): the kernel alone on host-made logits, the search loop on the goldens' decoders, top_k = 1 against
greedy_search, determinism, evaluate(), and the library's argument checks.

Tokens are compared outside the decisions the restatement itself marks as near-ties (margin below 1e-3; the caps on how
many those may be are held without a GPU by tests/test_sample_ref.py).  Log-probabilities are held to twice the per-step
logits bar of tests/test_gpu_parity.py's fp32 path (4e-5 * max(1, max |logit|)), divided by the temperature: the value is a
logit minus a log-sum-exp of logits, each within that bar."""
import functools

import numpy as np
import pytest
import torch

import recnet_amd as R
from recnet_amd.engine import _lib      # the engine's own _lib: the module whose RecNetError it raises
from tests import sample_ref as SR
from tests.golden_util import CASES, load_search_case
from tests.search_kit import bound_engine, decoder_for, lp_bar, rows_engine

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _row_results(V):
    """Every kernel-alone case at vocabulary V, device and restatement side by side (computed once, shared by the tests)."""
    eng = rows_engine()
    out = []
    for rows, quantised, top_k, temperature, t, seed in SR.row_cases(V):
        x = SR.row_logits(V, rows, quantised)
        xd = torch.from_numpy(x).cuda()
        before = xd.clone()
        tok, lp = eng.sample_rows(xd, temperature, top_k, seed, t)
        torch.cuda.synchronize()
        untouched = torch.equal(xd.view(torch.int32), before.view(torch.int32))
        rt, rl, margin = SR.sample_rows(x, temperature, top_k, seed, t)
        out.append(dict(case=(rows, quantised, top_k, temperature, t, seed), x=x, tok=tok.cpu().numpy(), lp=lp.cpu().numpy(),
                        ref_tok=rt, ref_lp=rl, margin=margin, untouched=untouched))
    return out


@pytest.mark.parametrize("V", SR.ROW_VS)
def test_sample_rows_tokens(V):
    """The kernel alone: tokens equal the restatement outside its near-tie rows; top_k = 1 is numpy's arg-max on every row; a
    drawn token always lies in the restatement's allowed set (on the quantised logits, where equal values straddle every cut,
    that holds only if exactly top_k entries are admitted, lowest indices first); the logits are left bit-identical."""
    for r in _row_results(V):
        rows, quantised, top_k, temperature, t, seed = r["case"]
        assert r["untouched"], r["case"]
        assert r["tok"].dtype == np.int64 and ((r["tok"] >= 0) & (r["tok"] < V)).all(), r["case"]
        keep = r["margin"] >= SR.NEAR_TIE
        assert np.array_equal(r["tok"][keep], r["ref_tok"][keep]), (r["case"], r["tok"], r["ref_tok"])
        assert SR.allowed_mask(r["x"], top_k)[np.arange(rows), r["tok"]].all(), r["case"]
        if top_k == 1:
            assert np.array_equal(r["tok"], r["x"].argmax(axis=1)), r["case"]
            assert (r["lp"] == 0.0).all(), r["case"]


@pytest.mark.parametrize("V", SR.ROW_VS)
def test_sample_rows_logprobs(V):
    """Log-probabilities of the same calls on the compared rows, against the restatement's float64 log-sum-exp.
    The test prints the worst error / bar ratio per vocabulary; no measured figure is recorded here yet."""
    worst = 0.0
    for r in _row_results(V):
        rows, quantised, top_k, temperature, t, seed = r["case"]
        keep = r["margin"] >= SR.NEAR_TIE
        err = np.abs(r["lp"][keep].astype(np.float64) - r["ref_lp"][keep])
        bar = lp_bar(np.abs(r["x"]).max(), temperature)
        if err.size:
            worst = max(worst, float(err.max() / bar))
            assert err.max() <= bar, (r["case"], float(err.max()), bar)
    print("V", V, "worst log-probability error / bar:", worst)


# ------------------------------------------------------------------------------------------------ search
@pytest.mark.parametrize("name,seed,temperature,top_k", SR.SEARCH_RUNS)
def test_sample_search_matches_the_restated_loop(name, seed, temperature, top_k):
    """fp32 path: n_steps, tokens and log-probabilities equal the restatement's loop outside excluded captions; the *_stop
    goldens end after one step."""
    g, P, enc = load_search_case(name)
    rt, rl, margins, amax = SR.sample_search(P, enc, temperature, top_k, seed, cell=g["_cell"])
    dec, cfg, inp, hid = decoder_for(g, P, "f32")
    toks, lps = R.sample_search(cfg, dec, inp, hid, enc.cuda(), temperature=temperature, top_k=top_k, seed=seed)
    toks, lps = np.array(toks, dtype=np.int64), np.array(lps, dtype=np.float64)
    assert toks.shape == rt.shape and lps.shape == rt.shape, (toks.shape, rt.shape)
    if name.endswith("_stop"):
        assert toks.shape[0] == 1
    keep = SR.comparable(margins)
    assert (~keep).any(axis=0).sum() <= 1
    assert np.array_equal(toks[keep], rt[keep])
    worst = 0.0
    for t in range(rt.shape[0]):
        err = np.abs(lps[t] - rl[t])[keep[t]]
        bar = lp_bar(amax[t], temperature)
        if err.size:
            worst = max(worst, float(err.max() / bar))
            assert err.max() <= bar, (t, float(err.max()), bar)
    print(name, "worst log-probability error / bar:", worst)


@pytest.mark.parametrize("name,prec", [(n, "f32") for n in CASES] + [("search_small", "bf16"), ("search_gru", "bf16")])
def test_top_k_one_is_greedy_search(name, prec):
    """Both searches run the same step at the same precision with the same tie rule: exact, for every seed."""
    g, P, enc = load_search_case(name)
    dec, cfg, inp, hid = decoder_for(g, P, prec)
    encd = enc.cuda()
    greedy = R.greedy_search(cfg, dec, inp, hid, encd)
    if prec == "f32":
        assert np.array_equal(np.array(greedy, dtype=np.int64), g["greedy"])
    for seed, temperature in ((1, 1.0), (2, 0.5)):
        toks, lps = R.sample_search(cfg, dec, inp, hid, encd, temperature=temperature, top_k=1, seed=seed)
        assert toks == greedy, (seed, temperature)
        assert all(v == 0.0 for row in lps for v in row)


def test_determinism_and_seeds():
    g, P, enc = load_search_case("search_small")
    dec, cfg, inp, hid = decoder_for(g, P, "f32")
    encd = enc.cuda()
    greedy = R.greedy_search(cfg, dec, inp, hid, encd)
    B, F = enc.shape[0], enc.shape[1]
    eng = bound_engine(dec, B, F, "f32")
    a = eng.sample_search(encd, 1.0, 0, 1)
    b = eng.sample_search(encd, 1.0, 0, 1)
    c = eng.sample_search(encd, 1.0, 0, 2)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert tuple(a[0].shape) == (31, B) and tuple(a[1].shape) == (31, B) and int(a[2].item()) == 31
    assert not torch.equal(a[0], c[0])
    toks, _ = R.sample_search(cfg, dec, inp, hid, encd, seed=1)
    assert toks == a[0].cpu().tolist()                                   # the Python mirror and the engine agree
    assert R.greedy_search(cfg, dec, inp, hid, encd) == greedy           # and neither disturbed the greedy search
    # a <EOS> can be sampled anywhere: sequence_logprob sums up to it
    lp = R.sequence_logprob(toks, a[1].cpu().tolist())
    assert len(lp) == B and all(np.isfinite(v) and v < 0 for v in lp)


def test_evaluate_accepts_the_sample_method():
    """("sample", 1.0, 1, 0) is the arg-max: the score dict of "greedy" on a tiny corpus."""
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
    enc = feed.collate_batch(vids, caps, 6)[0]
    idx2word = {i: "w%d" % i for i in range(V)}
    names = ["a", "b", "c", "d", "PAD", "PAD"]
    refs = {k: ["w3 w4 w5", "w7 w8"] for k in "abcd"}
    s_greedy = R.evaluate(C, [(names, enc)], model, "greedy", idx2word, refs)
    s_sample = R.evaluate(C, [(names, enc)], model, ("sample", 1.0, 1, 0), idx2word, refs)
    assert s_sample == s_greedy
    s_free = R.evaluate(C, [(names, enc)], model, ("sample", 1.0, 0, 3), idx2word, refs)
    assert set(s_free) == set(s_greedy)
    with pytest.raises(NotImplementedError):
        R.evaluate(C, [(names, enc)], model, ("nucleus", 0.9), idx2word, refs)


def test_library_refuses_bad_arguments_and_recovers():
    g, P, enc = load_search_case("search_small")
    dec, cfg, inp, hid = decoder_for(g, P, "f32")
    encd = enc.cuda()
    B, F, V = enc.shape[0], enc.shape[1], int(g["meta_dims"][3])
    eng = bound_engine(dec, B, F, "f32")
    x = torch.from_numpy(SR.row_logits(V, 3, False)).cuda()
    with pytest.raises(_lib.RecNetError, match="top_k"):
        eng.sample_search(encd, 1.0, V + 1, 1)
    with pytest.raises(_lib.RecNetError, match="temperature"):
        eng.sample_search(encd, 0.0, 0, 1)
    with pytest.raises(_lib.RecNetError, match="top_k"):
        eng.sample_rows(x, 1.0, V + 1, 1, 0)
    with pytest.raises(_lib.RecNetError, match="temperature"):
        eng.sample_rows(x, 0.0, 0, 1, 0)
    with pytest.raises(_lib.RecNetError, match="temperature"):
        eng.sample_rows(x, float("nan"), 0, 1, 0)
    toks, lps, n = eng.sample_search(encd, 1.0, V, 4)                    # top_k = V behaves as 0
    rt, _, margins, _ = SR.sample_search(P, enc, 1.0, 0, 4, cell=g["_cell"])
    assert int(n.item()) == rt.shape[0] and np.array_equal(toks.cpu().numpy()[:rt.shape[0]], rt)
    tok, _ = eng.sample_rows(x, 1.0, 1, 1, 0)
    assert np.array_equal(tok.cpu().numpy(), x.cpu().numpy().argmax(axis=1))
