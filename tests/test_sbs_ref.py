"""The stochastic beam search without a GPU: the restatement tests/sbs_ref.py is held to the statistics it
claims on a toy model with known leaf probabilities (samples without replacement, unbiased importance weights), to
tests/score_ref.py and tests/sample_ref.py on the search goldens, and to its own invariants; the caps on near-ties the device tests
rely on; the host layer (search.sbs_weights, the declared exports and op schemas, argument checks before any engine is built)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import sample_ref as SR
from tests import sbs_ref as SBS
from tests import score_ref as SC
from tests.golden_util import load_search_case
from tests.search_kit import no_library

# ------------------------------------------------------------------------------------------------ 1. statistics on a toy model
# Two steps, V = 3, fixed conditional tables: nine leaves (a, b) with p = P0[a] * P1[a][b]
P0 = np.array([0.5, 0.3, 0.2])
P1 = np.array([[0.6, 0.3, 0.1], [0.2, 0.5, 0.3], [0.3, 0.3, 0.4]])
TOY_SEEDS = range(1, 20001)


@functools.lru_cache(maxsize=None)
def _toy_draws():
    """Per seed the two leaves of a width-2 search in rank order with their (phi, G): int [n, 2], float64 [n, 2], float64 [n, 2]."""
    l0 = np.log(P0).astype(np.float32)[None, None, :]
    zeros, live1, live2 = np.zeros((1, 1)), np.zeros((1, 1), np.int32), np.zeros((2, 1), np.int32)
    leaves, phis, gums = [], [], []
    for seed in TOY_SEEDS:
        a = SBS.select_rows(l0, zeros, zeros, live1, 2, 1.0, seed, 0)
        tok0 = a["idx"][0]                                               # nb = 1: the flat index is the token
        l1 = np.log(P1[tok0]).astype(np.float32)[:, None, :]
        b = SBS.select_rows(l1, a["vals"].T, a["gum"].T, live2, 2, 1.0, seed, 1)
        src, tok1 = b["idx"][0] // 3, b["idx"][0] % 3
        leaves.append(tok0[src] * 3 + tok1); phis.append(b["vals"][0]); gums.append(b["gum"][0])
    return np.array(leaves), np.array(phis), np.array(gums)


def _chi2_quantile_999(dof):
    """0.999 quantile of chi^2(dof): scipy when present, else Wilson-Hilferty with z = 3.090232 (Phi(z) = 0.999)."""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(0.999, dof))
    except ImportError:
        z = 3.090232
        return dof * (1.0 - 2.0 / (9.0 * dof) + z * math.sqrt(2.0 / (9.0 * dof))) ** 3


def test_toy_pairs_are_a_sample_without_replacement():
    """The frequency of each ordered pair of leaves (A first, B second) against p_A * p_B / (1 - p_A) by chi^2, below the 0.999
    quantile for its 71 degrees of freedom.  The seeds are fixed, so the outcome is deterministic."""
    leaves, phis, _ = _toy_draws()
    p = (P0[:, None] * P1).reshape(9)
    assert np.allclose(np.exp(phis), p[leaves], rtol=1e-6)               # phi is the leaf's log-probability (float32 tables)
    assert (leaves[:, 0] != leaves[:, 1]).all()
    n = len(leaves)
    counts = np.zeros((9, 9))
    np.add.at(counts, (leaves[:, 0], leaves[:, 1]), 1)
    expect = n * p[:, None] * p[None, :] / (1.0 - p[:, None])
    off = ~np.eye(9, dtype=bool)
    assert abs(expect[off].sum() - n) < 1e-6 and expect[off].min() > 5
    chi2 = float(((counts[off] - expect[off]) ** 2 / expect[off]).sum())
    z = (counts[off] - expect[off]) / np.sqrt(expect[off])
    print("ordered pairs seen", int((counts[off] > 0).sum()), "of 72; chi^2", chi2, "bound", _chi2_quantile_999(71), "worst z", float(np.abs(z).max()))
    assert (counts[off] > 0).all()
    assert chi2 < _chi2_quantile_999(71)
    # rank 0 alone is an exact sample from the model
    first = np.bincount(leaves[:, 0], minlength=9)
    assert float(((first - n * p) ** 2 / (n * p)).sum()) < _chi2_quantile_999(8)


def test_toy_importance_weights_are_unbiased():
    """The mean over seeds of sum_k w_k f(leaf_k) with normalize=False equals the exact E f within 4 standard errors, for two f."""
    from recnet_amd import search
    leaves, phis, gums = _toy_draws()
    p = (P0[:, None] * P1).reshape(9)
    w = np.array(search.sbs_weights(phis.T, gums.T, normalize=False)).T    # [n, 2]
    assert np.allclose(w[:200], SBS.weights(phis[:200].T, gums[:200].T, normalize=False).T, rtol=1e-9, atol=0)
    assert (w[:, 1] == 0).all() and (w[:, 0] >= p[leaves[:, 0]] * (1 - 1e-12)).all()         # q <= 1
    for name, f in (("indicator of the rarest leaf's row", (np.arange(9) // 3 == 2).astype(np.float64)), ("leaf index squared", np.arange(9.0) ** 2)):
        est = (w * f[leaves]).sum(axis=1)
        exact = float((p * f).sum())
        se = float(est.std(ddof=1) / math.sqrt(len(est)))
        print(name, "estimate", float(est.mean()), "exact", exact, "standard error", se, "z", (float(est.mean()) - exact) / se)
        assert abs(est.mean() - exact) <= 4 * se
    wn = np.array(search.sbs_weights(phis.T, gums.T)).T
    assert np.allclose(wn.sum(axis=1), 1.0) and np.array_equal(wn[:, 0], np.ones(len(wn)))   # width 2: all weight on rank 0


# ------------------------------------------------------------------------------------------------ 2. the search goldens and rows160
@pytest.mark.parametrize("name,bw,cml,temp,seed", SBS.SEARCH_RUNS)
def test_restated_search_holds_its_invariants(name, bw, cml, temp, seed):
    g, P, enc = load_search_case(name)
    r = SBS.run(name, bw, cml, temp, seed)
    B, n = enc.shape[0], r["n_steps"]
    # the cap on near-ties, and the recorded share
    share = SBS.compared_share(r)
    assert share >= SBS.CAP, share
    assert abs(share - SBS.RUN_SHARES[(name, bw, cml, temp, seed)]) < 5e-4
    # cum / len of every rank are score_ref's on its own tokens at the run's temperature
    assert r["tokens"].shape == (bw, n, B)
    for k in range(bw):
        lp, _ = SC.score_captions(P, enc, r["tokens"][k], temp, g["_cell"])
        sums, lens = SC.caption_sums(lp, r["tokens"][k])
        assert np.array_equal(lens, r["len"][k])
        assert np.allclose(sums, r["cum"][k], rtol=0, atol=1e-9 * n)
    # ranks are pairwise different as canonical rows
    for b in range(B):
        assert len({tuple(r["tokens"][k, :, b]) for k in range(bw)}) == bw
    # G descending over the slots after every step, non-increasing along every history; a parent's best child has its G exactly;
    # finished hypotheses never change
    for t, s in enumerate(r["trace"]):
        assert (s["gum"][:-1] >= s["gum"][1:]).all()
        nb = s["pgum"].shape[0]
        for b in range(B):
            parent_g = s["pgum"][s["src"][:, b], b]
            assert (s["gum"][:, b] <= parent_g).all()
            for i in range(nb):
                kids = np.nonzero(s["src"][:, b] == i)[0]
                if kids.size:
                    assert s["gum"][kids, b].max() == s["pgum"][i, b]
                if s["pfin"][i, b]:
                    assert kids.size <= 1
                    for k in kids:
                        assert s["tok"][k, b] == SBS.PAD and s["cum"][k, b] == s["pcum"][i, b] and s["fin"][k, b] == s["pfin"][i, b]
                        assert (s["hist"][k, b, :t] == r["trace"][t - 1]["hist"][i, b]).all()
    # the stop rule: the first step that leaves every hypothesis finished, or caption_max_len + 1
    done = [bool((s["fin"] > 0).all()) for s in r["trace"]]
    assert len(r["trace"]) == n and not any(done[:-1]) and (done[-1] or n == cml + 1)
    assert np.array_equal(r["len"], np.where(r["trace"][-1]["fin"] > 0, r["trace"][-1]["fin"], n))


@pytest.mark.parametrize("name,temp,seed", SBS.WIDTH1_RUNS)
def test_width_one_draws_sample_search_tokens(name, temp, seed):
    """The counters and the site are sample_search's: argmax(phi + g) against argmax(s + g) can differ at near-ties only.  Compared
    up to each caption's <EOS> (the sampler goes on behind it), outside the near-ties of either restatement."""
    g, P, enc = load_search_case(name)
    cml = 7
    r = SBS.run(name, 1, cml, temp, seed)
    toks, _, margins, _ = SR.sample_search(P, enc, temp, 0, seed, cml, g["_cell"])
    ok_s, ok_r = SR.comparable(margins), SBS.comparable_steps(r["margins"])
    compared = 0
    for b in range(enc.shape[0]):
        for t in range(min(r["n_steps"], toks.shape[0])):
            if not (ok_s[t, b] and ok_r[t, b]):
                break
            assert r["tokens"][0, t, b] == toks[t, b], (b, t)
            compared += 1
            if toks[t, b] == SBS.EOS:
                break
    print(name, temp, seed, "decisions compared", compared)
    assert compared >= enc.shape[0]


# ------------------------------------------------------------------------------------------------ 3. the host layer
def test_sbs_weights_edge_cases():
    from recnet_amd import search
    assert search.sbs_weights([[-1.0, -2.0]], [[-0.5, -3.0]]) == [[1.0, 1.0]]                       # width 1
    assert search.sbs_weights([[-1.0, -2.0]], [[-0.5, -3.0]], normalize=False) == [[1.0, 1.0]]
    cum = [[-1.0, -0.5], [-2.0, -1.5], [-3.0, -4.0]]
    gum = [[0.3, 1.0], [-0.2, -0.5], [-1.0, -2.5]]
    w = np.array(search.sbs_weights(cum, gum))
    assert (w[2] == 0).all() and np.allclose(w.sum(axis=0), 1.0) and (w[:2] > 0).all()
    raw = np.array(search.sbs_weights(torch.tensor(cum), torch.tensor(gum), normalize=False))
    assert np.allclose(raw, SBS.weights(cum, gum, normalize=False), rtol=1e-9, atol=0) and (raw[2] == 0).all()
    assert np.allclose(raw / raw.sum(axis=0), w, rtol=1e-12) and np.allclose(SBS.weights(cum, gum), w, rtol=1e-9)
    # between the plug-in weight p / q(kappa = gum[bw - 1]), which it exceeds (the pinned maximum makes kappa too high: biased low),
    # and 1 / (exp(-kappa) - 1) + p, the bound from 1 / (1 - exp(-x)) < 1 / x + 1
    c, kappa = np.array(cum), np.array(gum)[2]
    plug_in = np.exp(c[:2]) / -np.expm1(-np.exp(c[:2] - kappa))
    assert (raw[:2] > plug_in).all() and (raw[:2] < 1.0 / np.expm1(-kappa) + np.exp(c[:2])).all()
    # a threshold far below everything: every rank above it is certain to be kept, w = p
    deep = np.array(search.sbs_weights([[-1.0], [-2.0], [-3.0]], [[0.0], [-1.0], [-60.0]], normalize=False))
    assert np.allclose(deep[:2, 0], np.exp([-1.0, -2.0]), rtol=1e-12)
    # p = 0 and a threshold at the maximum itself are finite
    odd = np.array(search.sbs_weights([[-2000.0, -1.0], [-1.0, -1.0], [-1.0, -2.0]], [[0.0, 0.0], [-0.1, 0.0], [-0.2, 0.0]], normalize=False))
    assert np.isfinite(odd).all() and (odd[:2] > 0).all()
    with pytest.raises(ValueError):
        search.sbs_weights([[-1.0]], [[-1.0], [-2.0]])


def test_exports_and_op_schemas_list_the_three_entries():
    from recnet_amd import _lib, _ops
    names = ("recnet_sbs_select_rows", "recnet_stochastic_beam_search", "recnet_stochastic_beam_search_ensemble")
    assert all(n in _lib.EXPORTS for n in names)
    assert all(n in _ops.OP_NAMES for n in ("sbs_select_rows", "stochastic_beam_search", "stochastic_beam_search_ensemble"))
    ops = _ops.load()
    s = str(ops.sbs_select_rows.default._schema)
    assert "Tensor logits, Tensor cum, Tensor gum, Tensor finished, int beam_width, float temperature, int seed, int t" in s
    assert "-> (Tensor vals, Tensor gum_out, Tensor idx)" in s
    s = str(ops.stochastic_beam_search.default._schema)
    assert "Tensor encoder_outputs, int beam_width, float temperature, int seed) -> (Tensor tokens, Tensor cum, Tensor lengths, Tensor gum, Tensor n_steps)" in s
    assert "int[] more_handles, float[] weights, int mode, Tensor encoder_outputs, int beam_width, float temperature, int seed" in \
        str(ops.stochastic_beam_search_ensemble.default._schema)
    # the library refuses a NULL handle / handle list first, the version is unchanged
    lib = _lib.load()
    assert lib.recnet_abi_version() == 12
    assert lib.recnet_sbs_select_rows(None, None, None, None, None, 1, 1, 8, 1, 1.0, 0, 0, None, None, None, None) == -2
    assert lib.recnet_stochastic_beam_search(None, None, 3, 1.0, 0, None, None, None, None, None, None) == -2
    assert lib.recnet_stochastic_beam_search_ensemble(None, 2, None, 0, None, 3, 1.0, 0, None, None, None, None, None, None) == -1
    assert b"null argument" in lib.recnet_last_error()


class _Dec:
    def __init__(self, V=61, D=32):
        self.output_size, self.encoder_size, self.hidden_size = V, D, 8

    def eval(self):
        return self

    def parameters(self):
        return iter([torch.zeros(1)])


def _search_args(dec, cml=7):
    class Cfg:
        caption_max_len = cml
        batch_size = 4
        decoder_model = "GRU"
    return Cfg(), dec, torch.full((1, 4), 1, dtype=torch.long), torch.zeros(1, 4, 8), torch.zeros(4, 5, 32)


def test_python_layer_checks_its_arguments_before_any_engine(monkeypatch):
    import recnet_amd as R
    no_library(monkeypatch)
    args = _search_args(_Dec())
    for width in (0, 9, -1, 2.5, "3"):
        with pytest.raises(ValueError, match="beam_width"):
            R.stochastic_beam_search(*args, width)
    with pytest.raises(ValueError, match="beam_width"):
        R.stochastic_beam_search(*_search_args(_Dec(V=5)), 6)              # wider than the vocabulary
    for temp in (0.0, -1.0, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError, match="temperature"):
            R.stochastic_beam_search(*args, 3, temperature=temp)
    cfg, dec, inp, hid, enc = args
    with pytest.raises(NotImplementedError):
        R.stochastic_beam_search(cfg, dec, inp * 3, hid, enc, 3)
    with pytest.raises(NotImplementedError):
        R.stochastic_beam_search(cfg, dec, inp, hid + 1, enc, 3)
    # best_of_n(distinct=True): at most 8, no cuts, the search's own checks
    with pytest.raises(ValueError, match="at most 8"):
        R.best_of_n(*args, 9, distinct=True)
    with pytest.raises(ValueError, match="top_k must be 0"):
        R.best_of_n(*args, 4, top_k=5, distinct=True)
    with pytest.raises(ValueError, match="top_k must be 0"):
        R.best_of_n(*args, 4, top_p=0.9, distinct=True)
    with pytest.raises(ValueError, match="temperature"):
        R.best_of_n(*args, 4, temperature=0.0, distinct=True)
    with pytest.raises(ValueError, match="consensus_weight"):
        R.best_of_n(*args, 4, consensus_weight=float("nan"), distinct=True)
    with pytest.raises(ValueError, match="needs a reconstructor"):
        R.best_of_n(*args, 4, recon_weight=1.0, distinct=True)
    # an Ensemble samples at temperature 1 only, and best_of_n takes none
    ens = R.Ensemble([_Dec(), _Dec()])
    with pytest.raises(NotImplementedError, match="temperature 1"):
        R.stochastic_beam_search(cfg, ens, inp, hid, enc, 3, temperature=0.5)
    with pytest.raises(NotImplementedError, match="best_of_n"):
        R.best_of_n(cfg, ens, inp, hid, enc, 4, distinct=True)
    # evaluate: the arity of the three methods
    ev = lambda method: R.evaluate(cfg, [(["a", "b", "c", "d"], np.zeros((4, 5, 32), np.float32))], dec, method, {3: "x"}, {v: ["x"] for v in "abcd"})
    for method in (("sbs", 3, 1.0), ("best_of_distinct", 4, 1.0), ("best_of_distinct_consensus", 4, 1.0, 0), ("sbs", 3, 1.0, 0, 0.9)):
        with pytest.raises(ValueError, match="fields"):
            ev(method)
    with pytest.raises(ValueError, match="beam_width"):
        ev(("sbs", 9, 1.0, 0))
