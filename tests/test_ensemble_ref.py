"""CPU checks of ensemble decoding: the restatement tests/ensemble_ref.py against hand-computed rows, against
tests/beam_ref.py / tests/score_ref.py for one member and under a permutation of the members; the shares of decisions the device test
(tests/test_gpu_ensemble.py) compares; the argument checks of search.Ensemble and of the calls that take one, which come before the
library; the three exports with NULL arguments."""
import math

import numpy as np
import pytest
import torch

from tests import beam_ref as BR
from tests import ensemble_ref as ER
from tests import score_ref as SC
from tests.golden_util import load_search_case
from tests.search_kit import no_library

LN2 = math.log(2.0)


# ------------------------------------------------------------------------------------------------ the restatement
def test_hand_computed_mix():
    """Two members over three words with probabilities (1/2, 1/4, 1/4) and (1/4, 1/4, 1/2), their logits shifted by constants
    (a log-softmax does not see them).  The logits are float32: the expected values hold to a few float32 roundings of them."""
    p1, p2 = np.array([[0.5, 0.25, 0.25]]), np.array([[0.25, 0.25, 0.5]])
    x1, x2 = (np.log(p1) + 3.0).astype(np.float32), (np.log(p2) - 1.5).astype(np.float32)
    tol = 1e-6
    y = ER.mix_rows([x1, x2], (1, 1), "arithmetic")
    assert np.abs(y - np.log([[3 / 8, 1 / 4, 3 / 8]])).max() < tol
    y = ER.mix_rows([x1, x2], (1, 3), "arithmetic")                       # weights 1/4, 3/4
    assert np.abs(y - np.log([[5 / 16, 4 / 16, 7 / 16]])).max() < tol
    assert abs(np.exp(y).sum() - 1.0) < tol                               # a mean of distributions is one: logsumexp(y) = 0
    y = ER.mix_rows([x1, x2], (2, 2), "geometric")                        # (the scale of the weights does not matter)
    assert np.abs(y - np.array([[-1.5 * LN2, -2.0 * LN2, -1.5 * LN2]])).max() < tol
    y = ER.mix_rows([x1, x2], (1, 3), "geometric")
    assert np.abs(y - np.array([[-(0.25 + 1.5) * LN2, -2.0 * LN2, -(0.5 + 0.75) * LN2]])).max() < tol
    # one member: its log-softmax, in both modes
    for mode in ER.MODES:
        assert np.abs(ER.mix_rows([x1], (5,), mode) - np.log(p1)).max() < tol
    # the renormalised geometric mean: sqrt(p1 p2) / Z
    g = np.sqrt(p1 * p2)
    assert np.abs(BR.log_softmax64(ER.mix_rows([x1, x2], (1, 1), "geometric")) - np.log(g / g.sum())).max() < tol


@pytest.mark.parametrize("name,bw,cml", [("search_gru", 3, 7), ("search_eos", 5, 7)])
def test_one_member_is_beam_ref(name, bw, cml):
    g, P, enc = load_search_case(name)
    a = BR.beam_search_nbest(P, enc, bw, BR.LENGTH_ALPHA, cml, g["_cell"])
    for mode in ER.MODES:
        b = ER.beam_search_nbest([(P, g["_cell"])], enc, bw, BR.LENGTH_ALPHA, cml, (2.5,), mode)
        for k in ("tokens", "cum", "len", "score", "margins", "final_margin", "amax"):
            assert np.array_equal(a[k], b[k]), (mode, k)
        assert a["n_steps"] == b["n_steps"]
        lp, amax = ER.score_captions([(P, g["_cell"])], enc, a["tokens"][0], None, mode)
        lp0, amax0 = SC.score_captions(P, enc, a["tokens"][0], 1.0, g["_cell"])
        assert np.array_equal(lp, lp0) and np.array_equal(amax, amax0)


def test_permuting_members_with_their_weights_changes_nothing():
    names, mode, bw, cml, w = ER.SEARCH_RUNS[12]                          # three members, geometric, weights (1, 2, 3)
    assert len(names) == 3 and len(set(w)) == 3
    models, enc = ER.load_models(names)
    a = ER.beam_search_nbest(models, enc, bw, ER.LENGTH_ALPHA, cml, w, mode)
    for m in ER.MODES:
        a = ER.beam_search_nbest(models, enc, bw, ER.LENGTH_ALPHA, cml, w, m)
        for perm in ((2, 0, 1), (1, 2, 0)):
            b = ER.beam_search_nbest([models[i] for i in perm], enc, bw, ER.LENGTH_ALPHA, cml, [w[i] for i in perm], m)
            keep = ER.comparable_captions(a)
            assert keep.any() and np.array_equal(a["tokens"][:, :, keep], b["tokens"][:, :, keep])
            assert np.abs(a["cum"] - b["cum"])[:, keep].max() < 1e-12 and np.abs(a["margins"] - b["margins"]).max() < 1e-12
        caps = a["tokens"][0]
        la, _ = ER.score_captions(models, enc, caps, w, m)
        lb, _ = ER.score_captions(models[::-1], enc, caps, w[::-1], m)
        assert np.abs(la - lb).max() < 1e-12


def test_score_reproduces_the_search_cum():
    """The promise the device test holds the device to, on the restatement itself: scoring a returned hypothesis under the ensemble
    gives its cum."""
    for run in (ER.SEARCH_RUNS[1], ER.SEARCH_RUNS[12]):
        names, mode, bw, cml, w = run
        models, enc = ER.load_models(names)
        r = ER.run_search(run)
        for k in range(bw):
            lp, _ = ER.score_captions(models, enc, r["tokens"][k], w, mode)
            sums, lens = SC.caption_sums(lp, r["tokens"][k])
            assert np.array_equal(lens, r["len"][k]) and np.abs(sums - r["cum"][k]).max() < 1e-10


@pytest.mark.parametrize("run", ER.SEARCH_RUNS, ids=lambda r: "%s-%s-%d-%d" % ("+".join(r[0]), r[1], r[2], r[3]))
def test_shares_of_compared_decisions(run):
    r = ER.run_search(run)
    share, captions = ER.compared_share(r), int(ER.comparable_captions(r).sum())
    print(run, "share %.3f" % share, "captions compared in full", captions)
    assert share >= ER.SHARE_CAP
    assert (round(share, 3), captions) == ER.RUN_SHARES[run]
    assert captions > 0                                                   # the device test compares tokens in full somewhere


def test_the_odd_member_differs_in_every_size():
    P, cell, enc, dims = ER.load_member(ER.ODD)
    P0, _, _, dims0 = ER.load_member("search_eos")
    assert dims[:4] == dims0[:4] and all(a != b for a, b in zip(dims[4:], dims0[4:]))
    assert P["rnn.weight_hh_l0"].shape[1] == 48 and P["embedding.weight"].shape == (97, 24)


# ------------------------------------------------------------------------------------------------ argument checks before the library
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


@pytest.mark.parametrize("what,make,match", [
    ("empty", lambda: ([], None, "arithmetic"), "between 1 and 8"),
    ("nine members", lambda: ([_Dec() for _ in range(9)], None, "arithmetic"), "between 1 and 8"),
    ("weights length", lambda: ([_Dec(), _Dec()], (1.0,), "arithmetic"), "weights for 2 members"),
    ("zero weight", lambda: ([_Dec(), _Dec()], (1.0, 0.0), "arithmetic"), "positive finite"),
    ("negative weight", lambda: ([_Dec(), _Dec()], (1.0, -2.0), "arithmetic"), "positive finite"),
    ("nan weight", lambda: ([_Dec(), _Dec()], (float("nan"), 1.0), "geometric"), "positive finite"),
    ("inf weight", lambda: ([_Dec(), _Dec()], (1.0, float("inf")), "geometric"), "positive finite"),
    ("string weight", lambda: ([_Dec(), _Dec()], (1.0, "1"), "geometric"), "positive finite"),
    ("mode", lambda: ([_Dec(), _Dec()], None, "harmonic"), "mode must be"),
    ("different V", lambda: ([_Dec(61), _Dec(97)], None, "arithmetic"), "vocabulary"),
    ("different D", lambda: ([_Dec(61, 32), _Dec(61, 64)], None, "arithmetic"), "feature size"),
])
def test_ensemble_checks_its_arguments_on_construction(what, make, match, monkeypatch):
    import recnet_amd as R
    no_library(monkeypatch)
    decs, w, mode = make()
    with pytest.raises(ValueError, match=match):
        R.Ensemble(decs, w, mode)


def test_the_same_decoder_twice_is_refused(monkeypatch):
    import recnet_amd as R
    no_library(monkeypatch)
    d = _Dec()
    with pytest.raises(ValueError, match="different objects"):
        R.Ensemble([d, d])


def test_a_good_ensemble_loads_nothing_and_stands_in_for_member_0(monkeypatch):
    import recnet_amd as R
    no_library(monkeypatch)
    a, b = _Dec(), _Dec()
    b.hidden_size = 24
    ens = R.Ensemble([a, b], (1, 3), "geometric")
    assert ens.weights == [0.25, 0.75] and ens.mode == "geometric" and ens.members == [a, b]
    assert ens.hidden_size == 8 and ens.output_size == 61 and ens.eval() is ens and len(list(ens.parameters())) == 2
    assert R.Ensemble([a]).weights == [1.0]


def test_calls_out_of_scope_refuse_an_ensemble_by_name(monkeypatch):
    import recnet_amd as R
    no_library(monkeypatch)
    ens = R.Ensemble([_Dec(), _Dec()])
    args = _search_args(ens)
    cfg, _, inp, hid, enc = args

    class Rec:
        kind = "global"
    calls = {
        "greedy_search": lambda: R.greedy_search(*args),
        "beam_search": lambda: R.beam_search(cfg, 3, None, ens, inp, hid, enc),
        "sample_search": lambda: R.sample_search(*args),
        "best_of_n": lambda: R.best_of_n(*args, 4),
        "reconstruction_errors": lambda: R.reconstruction_errors(cfg, ens, Rec(), enc, [[3] * 4]),
        "best_of_beam": lambda: R.best_of_beam(*args, 3, reconstructor=Rec(), recon_weight=1.0),
    }
    for name, call in calls.items():
        with pytest.raises(NotImplementedError, match=name):
            call()
    with pytest.raises(NotImplementedError, match="best_of_beam"):
        R.best_of_beam(*args, 3, reconstructor=Rec())                     # (also with the weight left at 0)
    with pytest.raises(NotImplementedError, match="temperature 1"):
        R.score_captions(cfg, ens, enc, [[3] * 4], temperature=0.5)
    # evaluate: the methods that search by one of those calls
    ev = lambda method: R.evaluate(cfg, [(["a", "b", "c", "d"], np.zeros((4, 5, 32), np.float32))], ens, method, {3: "x"}, {v: ["x"] for v in "abcd"})
    for method in ("greedy", ("beam", 3), ("sample", 1.0, 0, 0), ("best_of", 2, 1.0, 0, 0)):
        with pytest.raises(NotImplementedError, match="Ensemble"):
            ev(method)


def test_searches_check_their_own_arguments_with_an_ensemble_before_the_library(monkeypatch):
    import recnet_amd as R
    no_library(monkeypatch)
    ens = R.Ensemble([_Dec(), _Dec()])
    args = _search_args(ens)
    for kw in (dict(beam_width=0), dict(beam_width=9), dict(beam_width=3, length_alpha=-1.0), dict(beam_width=4, n_groups=3),
               dict(beam_width=3, banned_tokens=[2])):
        with pytest.raises(ValueError):
            R.beam_search_nbest(*args, **kw)
    with pytest.raises(ValueError, match="consensus_weight"):
        R.best_of_beam(*args, 3, consensus_weight=float("nan"))
    with pytest.raises(ValueError, match="not a token"):
        R.score_captions(args[0], ens, args[4], [[61] * 4])
    with pytest.raises(ValueError, match="rows of logits for 2 members"):
        R.ensemble_logits(ens, [np.zeros((2, 61), np.float32)])
    with pytest.raises(ValueError, match="one shape"):
        R.ensemble_logits(ens, [np.zeros((2, 61), np.float32), np.zeros((2, 60), np.float32)])
    with pytest.raises(ValueError, match="must be an Ensemble"):
        R.ensemble_logits(_Dec(), [np.zeros((2, 61), np.float32)])


# ------------------------------------------------------------------------------------------------ the exports
def test_library_exports_and_null_arguments():
    """The three entries refuse NULL handles / a NULL handle list first (no GPU needed); ops and prototypes are declared."""
    import ctypes as C
    from recnet_amd import _lib, _ops
    lib = _lib.load()
    names = ("recnet_ensemble_mix_rows", "recnet_beam_search_nbest_ensemble", "recnet_score_captions_ensemble")
    assert all(n in _lib.EXPORTS for n in names)
    assert all(n in _ops.OP_NAMES for n in ("ensemble_mix_rows", "beam_search_nbest_ensemble", "score_captions_ensemble"))
    assert lib.recnet_abi_version() == 12
    assert lib.recnet_ensemble_mix_rows(None, None, 2, None, 0, 5, 8, None, None) == -2
    assert b"workspace" in lib.recnet_last_error()
    nbest = lambda hs, M: lib.recnet_beam_search_nbest_ensemble(hs, M, None, 0, None, 3, 0.7, 1, 0.0, 0, 0, None, 0, None, None, None, None,
                                                                None, None, None)
    score = lambda hs, M: lib.recnet_score_captions_ensemble(hs, M, None, 0, None, None, 4, None, None, None, None)
    two_nulls = (C.c_void_p * 2)(None, None)
    for call in (nbest, score):
        assert call(None, 2) == -1 and b"null argument" in lib.recnet_last_error()
        assert call(two_nulls, 2) == -1 and b"null ensemble member" in lib.recnet_last_error()
        for M in (0, 9, -1):
            assert call(two_nulls, M) == -1 and b"between 1 and 8" in lib.recnet_last_error()
