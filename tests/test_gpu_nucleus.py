"""Nucleus (top-p) sampling on the device (recnet_sample_rows_nucleus / recnet_sample_search_nucleus)
against the CPU restatement (tests/nucleus_ref.py): the kernel alone on host-made logits, the search loop on the goldens'
decoders, top_p = 1 against the calls without it, best_of_n, evaluate(), and the argument checks.

The size of the set a token was drawn from is held to the restatement's band [n_lo, n_hi] (the sizes at target -/+ 2^-18 of
the mass: the two exponentials' rounding, tests/nucleus_ref.py; tests/test_nucleus_ref.py holds without a GPU that the band is
a single size on at least 3/4 of the rows of every vocabulary and on every step of the search runs).  Token and
log-probability are then compared at the device's own size: tokens outside the restatement's near-tie decisions,
log-probabilities within the bar of tests/search_kit.py, 2 * 4e-5 * max(1, max |logit|) / temperature."""
import functools

import numpy as np
import pytest
import torch

import recnet_amd as R
from recnet_amd.engine import _lib      # the engine's own _lib: the module whose RecNetError it raises
from tests import nucleus_ref as NR
from tests import sample_ref as SR
from tests import score_ref as SC
from tests.golden_util import load_search_case
from tests.search_kit import bound_engine, decoder_for, lp_bar, nucleus_row_sizes, rows_engine

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _device_logits(V, rows, quantised):
    return torch.from_numpy(SR.row_logits(V, rows, quantised)).cuda()


@functools.lru_cache(maxsize=None)
def _row_results(V):
    """Every kernel-alone case at vocabulary V, device and restatement side by side (computed once, shared by the tests)."""
    eng = rows_engine()
    out = []
    for case in NR.row_cases(V):
        rows, quantised, top_k, temperature, top_p, t, seed = case
        x = SR.row_logits(V, rows, quantised)
        xd = _device_logits(V, rows, quantised)
        tok, lp, na = eng.sample_rows_nucleus(xd, temperature, top_k, top_p, seed, t)
        untouched = torch.equal(xd.cpu().view(torch.int32), torch.from_numpy(x).view(torch.int32))
        n, n_lo, n_hi, b = nucleus_row_sizes(V)[(rows, quantised, top_k, temperature, top_p)]
        out.append(dict(case=case, x=x, tok=tok.cpu().numpy(), lp=lp.cpu().numpy(), na=na.cpu().numpy().astype(np.int64),
                        n_lo=n_lo, n_hi=n_hi, untouched=untouched))
    return out


def _restated_at_device_size(r):
    """The restated draw over the first n_allowed entries of the order, the device's own n_allowed (band-checked first)."""
    rows, quantised, top_k, temperature, top_p, t, seed = r["case"]
    assert ((r["n_lo"] <= r["na"]) & (r["na"] <= r["n_hi"])).all(), (r["case"], r["na"], r["n_lo"], r["n_hi"])
    if "ref" not in r:                                                  # (computed once, shared by the two tests)
        r["ref"] = NR.draw(r["x"], r["na"], temperature, seed, t)
    return r["ref"]


@pytest.mark.parametrize("V", SR.ROW_VS)
def test_nucleus_rows_sizes_and_tokens(V):
    """The kernel alone: n_allowed lies in the restatement's band (a single size on most rows); the token is the restated draw
    over that many entries of the order outside near-ties, and always one of them; the logits are left bit-identical."""
    exact = total = 0
    for r in _row_results(V):
        rows = r["case"][0]
        assert r["untouched"], r["case"]
        assert r["na"].dtype == np.int64 and r["tok"].dtype == np.int64 and ((r["tok"] >= 0) & (r["tok"] < V)).all(), r["case"]
        rt, _, margin = _restated_at_device_size(r)
        keep = margin >= SR.NEAR_TIE
        assert np.array_equal(r["tok"][keep], rt[keep]), (r["case"], r["tok"], rt)
        assert NR.prefix_mask(r["x"], r["na"])[np.arange(rows), r["tok"]].all(), r["case"]
        total += rows
        exact += int((r["n_lo"] == r["n_hi"]).sum())
    print("V", V, "rows", total, "of them held to a single size", exact)


@pytest.mark.parametrize("V", SR.ROW_VS)
def test_nucleus_rows_logprobs(V):
    """Log-probabilities of the same calls against the float64 log-sum-exp over the same set.  Prints the worst error / bar."""
    worst = 0.0
    for r in _row_results(V):
        temperature = r["case"][3]
        _, rl, margin = _restated_at_device_size(r)
        keep = margin >= SR.NEAR_TIE
        err = np.abs(r["lp"][keep].astype(np.float64) - rl[keep])
        bar = lp_bar(np.abs(r["x"]).max(), temperature)
        if err.size:
            worst = max(worst, float(err.max() / bar))
            assert err.max() <= bar, (r["case"], float(err.max()), bar)
    print("V", V, "worst log-probability error / bar:", worst)


@pytest.mark.parametrize("V", SR.ROW_VS)
def test_top_p_one_is_sample_rows(V):
    """No nucleus cut: the tokens and the bits of the log-probabilities of recnet_sample_rows; n_allowed is top_k, or V."""
    eng = rows_engine()
    for rows in (1, 7):
        for quantised in (False, True):
            xd = _device_logits(V, rows, quantised)
            for top_k in sorted({k for k in (0, 1, 8, V - 1, V) if 0 <= k <= V}):
                for temperature, t, seed in ((1.0, SR.ROW_T[0], 3), (0.5, SR.ROW_T[1], 4)):
                    tok, lp, na = eng.sample_rows_nucleus(xd, temperature, top_k, 1.0, seed, t)
                    tok0, lp0 = eng.sample_rows(xd, temperature, top_k, seed, t)
                    tok1, lp1 = eng.sample_rows(xd, temperature, top_k, seed, t, top_p=1.0)
                    assert torch.equal(tok, tok0) and torch.equal(lp.view(torch.int32), lp0.view(torch.int32)), (rows, quantised, top_k)
                    assert torch.equal(tok1, tok0) and torch.equal(lp1.view(torch.int32), lp0.view(torch.int32))
                    assert (na.cpu().numpy() == (top_k or V)).all(), (rows, quantised, top_k, na)


@pytest.mark.parametrize("V", SR.ROW_VS)
def test_one_entry_left_is_the_arg_max(V):
    """top_k = 1 with any top_p, and a tiny top_p with any top_k: numpy's arg-max, log-probability 0, n_allowed 1."""
    eng = rows_engine()
    for quantised in (False, True):
        x = SR.row_logits(V, 7, quantised)
        xd = _device_logits(V, 7, quantised)
        for top_k, top_p in [(1, p) for p in (0.05, 0.5, 0.9, 0.999, 1.0)] + [(k, 1e-6) for k in sorted({0, min(8, V), V})]:
            tok, lp, na = eng.sample_rows_nucleus(xd, 0.5, top_k, top_p, 5, 2)
            assert np.array_equal(tok.cpu().numpy(), x.argmax(axis=1)), (quantised, top_k, top_p)
            assert (lp.cpu().numpy() == 0.0).all() and (na.cpu().numpy() == 1).all(), (quantised, top_k, top_p)


def test_determinism_where_the_band_is_widest():
    """V = 12500, quantised, top_p = 0.999: hundreds of equal values at the cut and a band up to 20 sizes wide — the integer
    masses make the size a pure function of the logits, so two calls agree in every output."""
    eng = rows_engine()
    xd = _device_logits(12500, 7, True)
    for top_k, temperature in ((0, 1.0), (12499, 2.0)):
        a = eng.sample_rows_nucleus(xd, temperature, top_k, 0.999, 6, 3)
        b = eng.sample_rows_nucleus(xd, temperature, top_k, 0.999, 6, 3)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# ------------------------------------------------------------------------------------------------ search
@pytest.mark.parametrize("name,seed,temperature,top_k,top_p", NR.SEARCH_RUNS)
def test_nucleus_search_matches_the_restated_loop(name, seed, temperature, top_k, top_p):
    """fp32 path: n_steps, tokens, log-probabilities and n_allowed equal the restatement's loop on every compared entry (no
    caption is excluded for these runs); the *_stop goldens end after one step.  search.sample_search returns the same tokens."""
    g, P, enc = load_search_case(name)
    run = NR.sample_search(P, enc, temperature, top_k, top_p, seed, cell=g["_cell"])
    dec, cfg, inp, hid = decoder_for(g, P, "f32")
    encd = enc.cuda()
    toks, lps, na, n = bound_engine(dec, *encd.shape[:2], "f32").sample_search_nucleus(encd, temperature, top_k, top_p, seed)
    n = int(n.item())
    rt = run["tokens"]
    assert n == rt.shape[0]
    if name.endswith("_stop"):
        assert n == 1
    toks, lps, na = toks[:n].cpu().numpy(), lps[:n].cpu().numpy().astype(np.float64), na[:n].cpu().numpy()
    keep = NR.comparable(run)
    assert keep.all()
    assert np.array_equal(toks[keep], rt[keep])
    assert np.array_equal(na[keep], run["n"][keep])
    worst = 0.0
    for t in range(n):
        err = np.abs(lps[t] - run["logprobs"][t])[keep[t]]
        bar = lp_bar(run["amax"][t], temperature)
        worst = max(worst, float(err.max() / bar))
        assert err.max() <= bar, (t, float(err.max()), bar)
    print(name, "worst log-probability error / bar:", worst)
    ptoks, plps = R.sample_search(cfg, dec, inp, hid, encd, temperature=temperature, top_k=top_k, seed=seed, top_p=top_p)
    assert ptoks == toks.tolist() and np.array_equal(np.array(plps), lps)


def test_top_p_one_through_sample_search_is_the_call_without_it():
    for name in ("search_small", "search_gru"):
        g, P, enc = load_search_case(name)
        dec, cfg, inp, hid = decoder_for(g, P, "f32")
        encd = enc.cuda()
        for temperature, top_k, seed in ((1.0, 0, 2), (0.5, 5, 3)):
            a = R.sample_search(cfg, dec, inp, hid, encd, temperature, top_k, seed)
            b = R.sample_search(cfg, dec, inp, hid, encd, temperature, top_k, seed, top_p=1.0)
            assert a == b
        eng = bound_engine(dec, *encd.shape[:2], "f32")
        u = eng.sample_search(encd, 1.0, 0, 2)
        v = eng.sample_search(encd, 1.0, 0, 2, top_p=1.0)
        w = eng.sample_search_nucleus(encd, 1.0, 0, 1.0, 2)
        assert all(torch.equal(x, y) for x, y in zip(u, v))
        assert torch.equal(u[0], w[0]) and torch.equal(u[1].view(torch.int32), w[1].view(torch.int32)) and torch.equal(u[2], w[3])
        assert (w[2].cpu().numpy() == int(g["meta_dims"][3])).all()


@pytest.mark.parametrize("name,seed", [("search_small_b", 3), ("search_gru_b", 5)])
def test_best_of_n_with_a_nucleus(name, seed):
    """best_of_n(n = 3, top_p = 0.8): the chosen captions are the restated rollouts of seeds seed .. seed + 2, scored by the
    restated teacher-forced log-probabilities at temperature 1 on the full distribution and picked by pick_best_of_n.  For these
    seeds the restatement excludes no caption and the best two scores of a caption are at least 0.04 apart."""
    g, P, enc = load_search_case(name)
    cands, sums, lens = [], [], []
    for k in range(3):
        run = NR.sample_search(P, enc, 1.0, 0, 0.8, seed + k, cell=g["_cell"])
        assert NR.comparable(run).all()
        lp, _ = SC.score_captions(P, enc, run["tokens"], 1.0, cell=g["_cell"])
        c, ln = SC.caption_sums(lp, run["tokens"])
        cands.append(run["tokens"]); sums.append(c.tolist()); lens.append(ln.tolist())
    score = np.sort(np.array(sums) / np.array(lens), axis=0)
    assert (score[-1] - score[-2]).min() > 0.03
    rk, rscores = R.pick_best_of_n(sums, lens)
    dec, cfg, inp, hid = decoder_for(g, P, "f32")
    caps, ks, scores = R.best_of_n(cfg, dec, inp, hid, enc.cuda(), 3, temperature=1.0, top_k=0, seed=seed, top_p=0.8)
    assert ks == rk
    for b in range(enc.shape[0]):
        assert caps[b] == cands[ks[b]][:lens[ks[b]][b], b].tolist()
        assert abs(scores[b] - rscores[b]) <= 1e-3


def test_evaluate_takes_a_trailing_top_p():
    """On the tiny corpus of tests/test_gpu_sample.py::test_evaluate_accepts_the_sample_method: a trailing top_p = 1.0 changes
    nothing on the three sampling methods, a tiny top_p is the greedy search, and there is no method called "nucleus"."""
    from recnet_amd import feed
    V = 41
    C = R.make_config(use_recon=True, reconstructor_type="local", batch_size=6, encoder_output_len=5, encoder_output_size=32,
                      embedding_size=12, decoder_hidden_size=24, decoder_attn_size=8, reconstructor_hidden_size=32,
                      reconstructor_attn_size=8, precision="f32")
    torch.manual_seed(1)
    built = R.build_decoder(V, C)
    model = built["model"]
    torch.manual_seed(2)
    rec = R.build_reconstructor(C)["model"]
    rng = np.random.RandomState(9)
    vids = [rng.randn(5, 32).astype(np.float32) for _ in range(6)]
    caps = [feed.pad_caption(rng.randint(3, V, size=4), 30) for _ in range(6)]
    enc = feed.collate_batch(vids, caps, 6)[0]
    idx2word = {i: "w%d" % i for i in range(V)}
    names = ["a", "b", "c", "d", "PAD", "PAD"]
    refs = {k: ["w3 w4 w5", "w7 w8"] for k in "abcd"}
    ev = lambda method, **kw: R.evaluate(C, [(names, enc)], model, method, idx2word, refs, **kw)
    assert ev(("sample", 1.0, 0, 3, 1.0)) == ev(("sample", 1.0, 0, 3))
    assert ev(("best_of", 3, 1.0, 0, 2, 1.0)) == ev(("best_of", 3, 1.0, 0, 2))
    assert ev(("best_of_recon", 3, 1.0, 0, 2, 0.5, 1.0), reconstructor=rec) == ev(("best_of_recon", 3, 1.0, 0, 2, 0.5), reconstructor=rec)
    assert ev(("sample", 1.0, 0, 0, 1e-6)) == ev("greedy")
    assert set(ev(("best_of", 3, 1.0, 0, 2, 0.8))) == set(ev("greedy"))
    with pytest.raises(ValueError):
        ev(("sample", 1.0, 0, 3, 0.9, 0.9))
    with pytest.raises(ValueError, match="top_p"):
        ev(("sample", 1.0, 0, 3, 0.0))
    with pytest.raises(NotImplementedError):
        ev(("nucleus", 0.9))


def test_library_refuses_a_bad_top_p_and_recovers():
    g, P, enc = load_search_case("search_small")
    dec, cfg, inp, hid = decoder_for(g, P, "f32")
    encd = enc.cuda()
    V = int(g["meta_dims"][3])
    eng = bound_engine(dec, *encd.shape[:2], "f32")
    x = torch.from_numpy(SR.row_logits(V, 3, False)).cuda()
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(_lib.RecNetError, match="top_p"):
            eng.sample_search_nucleus(encd, 1.0, 0, bad, 1)
        with pytest.raises(_lib.RecNetError, match="top_p"):
            eng.sample_rows_nucleus(x, 1.0, 0, bad, 1, 0)
        with pytest.raises(_lib.RecNetError, match="top_p"):
            eng.sample_search(encd, 1.0, 0, 1, top_p=bad)
        with pytest.raises(_lib.RecNetError, match="top_p"):
            eng.sample_rows(x, 1.0, 0, 1, 0, top_p=bad)
        with pytest.raises(ValueError, match="top_p"):
            R.sample_search(cfg, dec, inp, hid, encd, top_p=bad)
    with pytest.raises(_lib.RecNetError, match="top_k"):
        eng.sample_rows_nucleus(x, 1.0, V + 1, 0.9, 1, 0)
    with pytest.raises(_lib.RecNetError, match="temperature"):
        eng.sample_search_nucleus(encd, 0.0, 0, 0.9, 1)
    toks, lps, na, n = eng.sample_search_nucleus(encd, 1.0, 0, 0.9, 2)             # the next valid call still works
    run = NR.sample_search(P, enc, 1.0, 0, 0.9, 2, cell=g["_cell"])
    assert int(n.item()) == run["tokens"].shape[0] and np.array_equal(toks.cpu().numpy()[:run["tokens"].shape[0]], run["tokens"])
    tok, _, na = eng.sample_rows_nucleus(x, 1.0, 1, 0.9, 1, 0)
    assert np.array_equal(tok.cpu().numpy(), x.cpu().numpy().argmax(axis=1)) and (na.cpu().numpy() == 1).all()
