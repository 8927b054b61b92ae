"""The consensus (minimum-Bayes-risk) scores without a GPU: the float64 restatement (tests/consensus_ref.py)
against the hand case of the contract and against metrics.cider on corpora with a uniform idf, the properties the reranking rests
on (duplicates get bit-equal utilities; weights), the new arguments of pick_best_of_n, and the argument checks of the Python
layer, which all come before any engine is asked for."""
import math
import sys

import numpy as np
import pytest
import torch

from tests import consensus_ref as CR


# ------------------------------------------------------------------------------------------------ the restatement
def test_hand_case_to_the_last_digit():
    H = CR.HAND
    h, r = CR.HAND_H, CR.HAND_R
    ch, cr = CR.ngram_counts(CR.words(h)), CR.ngram_counts(CR.words(r))
    assert CR.overlap(ch, cr) == H["M"] and CR.squares(ch) == H["Qh"] and CR.squares(cr) == H["Qr"]
    assert CR.sim(h, r) == H["sim_hr"] and CR.sim(r, h) == H["sim_rh"] and CR.sim(h, h) == H["sim_hh"]
    assert CR.sim((5, CR.EOS), (5, CR.EOS)) == H["sim_one_word"]
    for other in (h, r, (CR.EOS,), (5,)):
        assert CR.sim((CR.EOS, 5, 6), other) == 0.0 and CR.sim(other, (CR.EOS,)) == 0.0      # an empty caption, either side
    # whatever stands behind the first <EOS> is ignored, further <EOS> included; without an <EOS> all T tokens are words
    assert CR.sim(h + (9, 9, CR.EOS, 5), r + (CR.EOS, 7)) == H["sim_hr"]
    assert CR.sim(h[:-1], r[:-1]) == H["sim_hr"]
    # <PAD> is a word like any other
    # <PAD> is a word like any other (two words have no 3- and 4-grams: two of the four orders count)
    assert CR.sim((0, 0, CR.EOS), (0, 0, CR.EOS)) == 0.5 and CR.sim((0, CR.EOS), (5, CR.EOS)) == 0.0
    hyp = np.full((3, 6, 1), CR.EOS, np.int64)
    hyp[0, :, 0], hyp[1, :5, 0], hyp[2, :, 0] = h, r, h
    out = CR.consensus(hyp)
    assert tuple(out["util"][:, 0].tolist()) == H["util"]
    assert out["counts"][0, 1, 0].tolist() == H["M"] and out["q_hyp"][0, 0].tolist() == H["Qh"] and out["q_ref"][1, 0].tolist() == H["Qr"]
    assert out["len_hyp"][:, 0].tolist() == [5, 4, 5]


def _disjoint_corpus(rng, n_ids):
    """A corpus in which no word is shared between two ids (so no n-gram is shared between the reference sets of two ids): the idf
    of metrics.cider is then the same for every n-gram.  Captions of >= 1 word from a small vocabulary per id."""
    gts, res, cols = {}, {}, {}
    for k in range(n_ids):
        vocab = [10 * k + 3 + v for v in range(int(rng.integers(1, 6)))]
        cap = lambda: [int(vocab[i]) for i in rng.integers(0, len(vocab), int(rng.integers(1, 12)))]
        h, rs = cap(), [cap() for _ in range(int(rng.integers(1, 5)))]
        gts[k], res[k] = [" ".join(map(str, r)) for r in rs], [" ".join(map(str, h))]
        cols[k] = (h + [CR.EOS], [r + [CR.EOS] for r in rs])
    return gts, res, cols


def test_cider_cross_check_on_uniform_idf_corpora():
    """metrics.cider is pinned to the reference's scorer (tests/test_metrics.py); with a uniform idf its per-id score is
    10 * mean_j sim(h, r_j)."""
    from recnet_amd import metrics
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(200):
        gts, res, cols = _disjoint_corpus(rng, int(rng.integers(2, 6)))
        _, per_id = metrics.cider(gts, res)
        for k, (h, rs) in cols.items():
            mine = 10.0 * (sum(CR.sim(h, r) for r in rs) / len(rs))
            worst = max(worst, abs(mine - float(per_id[k])))
    print("worst |10 mean sim - cider per id| over 200 corpora:", worst, "/ bar", CR.BAR)
    assert worst <= CR.BAR


def test_duplicates_get_bit_equal_utilities():
    rng = np.random.default_rng(11)
    pairs = 0
    for trial in range(300):
        N, T, B = int(rng.integers(2, 9)), int(rng.integers(1, 9)), 2
        hyp = rng.integers(2, 6, (N, T, B))                       # words 3..5 and <EOS>: short captions, many duplicates
        hyp[N - 1, :, 0] = hyp[0, :, 0]
        out = CR.consensus(hyp)
        for b in range(B):
            w = [CR.words(hyp[k, :, b]) for k in range(N)]
            for i in range(N):
                for j in range(i + 1, N):
                    if w[i] == w[j]:
                        pairs += 1
                        assert out["util"][i, b].tobytes() == out["util"][j, b].tobytes(), (trial, b, i, j)
    assert pairs > 300


def test_prefix_weights_agree_with_the_uniform_call():
    rng = np.random.default_rng(13)
    worst = 0.0
    for _ in range(50):
        Nh, Nr, T, B = int(rng.integers(1, 5)), int(rng.integers(2, 7)), int(rng.integers(1, 8)), 3
        hyp, ref = rng.integers(2, 7, (Nh, T, B)), rng.integers(2, 7, (Nr, T + 1, B))
        k = int(rng.integers(1, Nr + 1))
        w = np.zeros((Nr, B))
        w[:k] = 1.0 / k
        worst = max(worst, float(np.abs(CR.consensus(hyp, ref, w)["util"] - CR.consensus(hyp, ref[:k])["util"]).max()))
    print("worst |weighted - uniform on the prefix|:", worst, "/ bar", CR.BAR)
    assert worst <= CR.BAR


# ------------------------------------------------------------------------------------------------ pick_best_of_n
def test_pick_best_of_n_with_the_consensus_term():
    from recnet_amd import pick_best_of_n
    caps = [[-4.0, -6.0, -3.0], [-2.0, -8.0, -3.0], [-3.0, -9.0, -3.0]]
    lens = [[2, 2, 2], [2, 4, 2], [2, 3, 2]]
    errs = [[0.5, 0.0, 0.0], [0.0, 0.0, 0.0], [0.25, 1.0, 0.0]]
    U = [[0.75, 0.5, 0.5], [0.25, 0.5, 0.5], [0.5, 0.0, 0.5]]
    # the old calls compute what they did
    assert pick_best_of_n(caps, lens) == ([1, 1, 0], [-1.0, -2.0, -1.5])
    assert pick_best_of_n(caps, lens, errs, 2.0) == ([1, 1, 0], [-1.0, -2.0, -1.5])
    assert pick_best_of_n(caps, lens, None, 0.0, None, 5.0) == pick_best_of_n(caps, lens)
    assert pick_best_of_n(caps, lens, errs, 2.0, None, 5.0) == pick_best_of_n(caps, lens, errs, 2.0)
    # the term is ADDED: b0: k = 0 gains 2 * 0.75 = 1.5 on -2.0 and passes k = 1 (-1.0 + 0.5); b2: all equal -> the lowest k
    assert pick_best_of_n(caps, lens, None, 0.0, U, 2.0) == ([0, 1, 0], [-0.5, -1.0, -0.5])
    # a negative weight subtracts: b1: k = 1 and k = 2 both reach -3.0 (k = 0: -4.0) -> the lower of the two
    assert pick_best_of_n(caps, lens, None, 0.0, U, -2.0) == ([1, 1, 0], [-1.5, -3.0, -2.5])
    # with both terms: caption_logprob / length - recon_weight * err + consensus_weight * U
    ks, scores = pick_best_of_n(caps, lens, errs, 2.0, U, 2.0)
    assert ks == [1, 1, 0] and scores == [-1.0 - 0.0 + 0.5, -2.0 - 0.0 + 1.0, -1.5 + 1.0]
    assert pick_best_of_n(caps, lens, None, 0.0, U, 0.0) == pick_best_of_n(caps, lens)
    # equal scores from bit-equal utilities: the lowest k, also when it is not the first
    assert pick_best_of_n([[-4.0], [-2.0], [-2.0]], [[2], [2], [2]], None, 0.0, [[0.1], [0.3], [0.3]], 1.0)[0] == [1]


# ------------------------------------------------------------------------------------------------ argument checks
def _no_engine(monkeypatch):
    """No library and no engine: a check that lets a bad argument through fails loudly."""
    from recnet_amd import search

    def boom(*a, **k):
        raise AssertionError("an engine / the library was asked for")
    loaders = [m for n, m in list(sys.modules.items()) if n.endswith(("_amd._lib", "_amd._ops")) and m is not None]
    assert loaders
    for m in loaders:
        monkeypatch.setattr(m, "load", boom)
    for name in ("_consensus_engine", "_nbest_engine", "_rec_engine", "_cached_engine"):
        monkeypatch.setattr(search, name, boom)


_G = [[[3, 4, 5], [6, 2, 2]], [[3, 4, 5], [2, 7, 8]]]          # N = 2 sets of [T = 2][B = 3]
_T = torch.tensor(_G)
BAD_SCORES = [
    ("N 33", dict(captions=[_G[0]] * 33), "between 1 and 32"),
    ("N 0", dict(captions=[]), "between 1 and 32"),
    ("tensor N 33", dict(captions=torch.zeros(33, 2, 3, dtype=torch.long)), "between 1 and 32"),
    ("T 65", dict(captions=[[[3, 4, 5]] * 65]), "steps"),
    ("T 0", dict(captions=[[]]), "steps"),
    ("tensor T 65", dict(captions=torch.zeros(2, 65, 3, dtype=torch.long)), "steps"),
    ("tensor B 0", dict(captions=torch.zeros(2, 3, 0, dtype=torch.long)), "at least one caption"),
    ("tensor dims", dict(captions=torch.zeros(2, 3, dtype=torch.long)), "LongTensor"),
    ("tensor dtype", dict(captions=torch.zeros(2, 3, 3)), "LongTensor"),
    ("negative token", dict(captions=[[[3, -1, 5]]]), r"captions\[0\]\[0\]\[1\] = -1"),
    ("token 2^31", dict(captions=[[[3, 4, 2 ** 31]]]), r"captions\[0\]\[0\]\[2\] = 2147483648"),
    ("fractional token", dict(captions=[[[3, 4.5, 5]]]), "not a token"),
    ("tensor negative token", dict(captions=torch.tensor([[[3, -7, 5]]])), "token -7"),
    ("tensor token 2^31", dict(captions=torch.tensor([[[3, 2 ** 31, 5]]])), "token 2147483648"),
    ("ragged B", dict(captions=[[[3, 4, 5], [6, 2]]]), r"captions\[0\]\[1\]"),
    ("sets disagree in B", dict(captions=[_G[0], [[3, 4], [6, 2]]]), r"captions\[1\]\[0\]"),
    ("refs disagree in B", dict(captions=_G, refs=[[[3, 4], [6, 2]]]), "refs hold 2 captions per step, captions 3"),
    ("tensor refs disagree in B", dict(captions=_T, refs=torch.zeros(2, 2, 4, dtype=torch.long)), "refs hold 4"),
    ("refs N 33", dict(captions=_G, refs=[_G[0]] * 33), "refs must hold between 1 and 32"),
    ("refs T 65", dict(captions=_G, refs=torch.zeros(2, 65, 3, dtype=torch.long)), "refs must have between 1 and 64 steps"),
    ("refs negative token", dict(captions=_G, refs=[[[3, 4, -5]]]), r"refs\[0\]\[0\]\[2\] = -5"),
    ("sigma 0", dict(captions=_G, sigma=0.0), "sigma"),
    ("sigma negative", dict(captions=_G, sigma=-6.0), "sigma"),
    ("sigma nan", dict(captions=_G, sigma=float("nan")), "sigma"),
    ("sigma inf", dict(captions=_G, sigma=float("inf")), "sigma"),
    ("sigma text", dict(captions=_G, sigma="6"), "sigma"),
    ("weights rows", dict(captions=_G, weights=[[1.0, 1.0, 1.0]]), "weights must be"),
    ("weights columns", dict(captions=_G, weights=[[1.0, 1.0], [1.0, 1.0]]), "weights must be"),
    ("weights follow the refs", dict(captions=_G, refs=[_G[0]] * 3, weights=[[1.0] * 3] * 2), "weights must be"),
    ("tensor weights shape", dict(captions=_T, weights=torch.ones(3, 2)), "weights must be"),
    ("weights negative", dict(captions=_G, weights=[[1.0, -0.5, 1.0], [1.0, 1.0, 1.0]]), "finite and >= 0"),
    ("weights nan", dict(captions=_G, weights=[[1.0, float("nan"), 1.0], [1.0, 1.0, 1.0]]), "finite and >= 0"),
    ("tensor weights inf", dict(captions=_T, weights=torch.full((2, 3), float("inf"))), "finite and >= 0"),
]


@pytest.mark.parametrize("what,kw,match", BAD_SCORES, ids=[c[0] for c in BAD_SCORES])
def test_consensus_scores_checks_its_arguments_before_any_engine(what, kw, match, monkeypatch):
    import recnet_amd as R
    _no_engine(monkeypatch)
    with pytest.raises(ValueError, match=match):
        R.consensus_scores(**kw)


def test_good_arguments_pass_the_checks_and_reach_the_engine(monkeypatch):
    """Valid arguments get past every check: the engine is the next thing asked for, once, with the device."""
    import recnet_amd as R
    from recnet_amd import search
    reached = []

    def engine(device):
        reached.append(torch.device(device))
        raise KeyError("engine")
    monkeypatch.setattr(search, "_consensus_engine", engine)
    long_and_short = [[[3, 4, 5]] * 64, [[6, 2, 2]]]                       # T_k differ: brought to a common T
    for kw in (dict(captions=_G), dict(captions=_T, refs=_G, weights=[[0.5] * 3, [0.0] * 3]), dict(captions=[_G[0]] * 32, sigma=2),
               dict(captions=long_and_short, weights=torch.ones(2, 3)), dict(captions=[[[2 ** 31 - 1, 0, 2]]], device="cuda:0")):
        with pytest.raises(KeyError):
            R.consensus_scores(**kw)
    assert len(reached) == 5 and reached[-1] == torch.device("cuda:0")


def test_caption_sets_are_continued_with_eos():
    """A shorter set is continued with <EOS> rows: the words of its captions stay what they are, also without an <EOS> of their own."""
    from recnet_amd import search
    t = search._pad_eos(torch.tensor([[3, 4], [5, 2]]), 4)
    assert t.tolist() == [[3, 4], [5, 2], [2, 2], [2, 2]]
    assert CR.words(t[:, 0].tolist()) == (3, 5) and CR.words(t[:, 1].tolist()) == (4,)
    assert search._pad_eos(t, 4) is t
    stacked = search._consensus_set([[[3, 4]], [[5, 6], [7, 2], [8, 8]]], "captions")
    assert stacked.shape == (2, 3, 2) and stacked[0].tolist() == [[3, 4], [2, 2], [2, 2]]


class _Dec:
    output_size = 61
    hidden_size = 8


def _search_args(cml=7):
    class Cfg:
        caption_max_len = cml
    return Cfg(), _Dec(), torch.full((1, 4), 1, dtype=torch.long), torch.zeros(1, 4, 8), torch.zeros(4, 5, 32)


@pytest.mark.parametrize("w", [float("nan"), float("inf"), -float("inf"), "1", None])
def test_searches_refuse_a_bad_consensus_weight_before_any_engine(w, monkeypatch):
    import recnet_amd as R
    _no_engine(monkeypatch)
    with pytest.raises(ValueError, match="consensus_weight"):
        R.best_of_n(*_search_args(), 4, consensus_weight=w)
    with pytest.raises(ValueError, match="consensus_weight"):
        R.best_of_beam(*_search_args(), 4, consensus_weight=w)


def test_searches_refuse_what_the_kernel_cannot_take_before_any_engine(monkeypatch):
    import recnet_amd as R
    _no_engine(monkeypatch)
    with pytest.raises(ValueError, match="at most 32 candidates"):
        R.best_of_n(*_search_args(), 33, consensus_weight=0.5)
    with pytest.raises(ValueError, match=r"caption_max_len \+ 1 <= 64"):
        R.best_of_n(*_search_args(64), 4, consensus_weight=0.5)
    with pytest.raises(ValueError, match=r"caption_max_len \+ 1 <= 64"):
        R.best_of_beam(*_search_args(64), 4, consensus_weight=-0.5)
    # the older checks still come first / still hold
    with pytest.raises(ValueError, match="n must be"):
        R.best_of_n(*_search_args(), 0, consensus_weight=0.5)
    with pytest.raises(ValueError, match="beam_width"):
        R.best_of_beam(*_search_args(), 9, consensus_weight=0.5)
    with pytest.raises(ValueError, match="n_groups"):
        R.best_of_beam(*_search_args(), 4, consensus_weight=0.5, n_groups=3)


def test_zero_weight_lifts_the_limits(monkeypatch):
    """consensus_weight = 0 is the call without it: n = 33 and caption_max_len = 64 get past the checks to the engine."""
    import recnet_amd as R
    from recnet_amd import search

    def engine(*a, **k):
        raise KeyError("engine")
    monkeypatch.setattr(search, "_cached_engine", engine)
    monkeypatch.setattr(search, "_nbest_engine", engine)
    with pytest.raises(KeyError):
        R.best_of_n(*_search_args(64), 33, consensus_weight=0.0)
    with pytest.raises(KeyError):
        R.best_of_beam(*_search_args(64), 4, consensus_weight=0)


def test_evaluate_parses_the_two_new_methods(monkeypatch):
    import recnet_amd as R
    from recnet_amd import loop
    calls = []

    def bon(config, decoder, inp, hid, enc, n, temperature, top_k, seed, **kw):
        calls.append(("bon", n, temperature, top_k, seed, kw))
        return [[3, 2] for _ in range(enc.shape[0])], None, None

    def bob(config, decoder, inp, hid, enc, width, length_alpha, **kw):
        calls.append(("bob", width, length_alpha, kw))
        return [[3, 2] for _ in range(enc.shape[0])], None, None
    monkeypatch.setattr(loop, "best_of_n", bon)
    monkeypatch.setattr(loop, "best_of_beam", bob)
    monkeypatch.setattr(loop.metrics, "score_all", lambda gts, res: dict(res))

    class Cfg:
        batch_size, decoder_model, caption_max_len = 2, "GRU", 7
    dec = torch.nn.Linear(2, 2)
    dec.hidden_size = 4
    feats = np.zeros((2, 3, 4), dtype=np.float32)
    ev = lambda method: R.evaluate(Cfg, [(["a", "b"], feats)], dec, method, {3: "x", 2: "<EOS>"}, {v: ["x"] for v in "ab"})
    div = dict(n_groups=2, diversity_penalty=1.0)
    assert set(ev(("best_of_consensus", 4, 0.9, 5, 7, 0.5))) == set("ab")
    ev(("best_of_consensus", 4, 0.9, 5, 7, 0.5, 0.8))
    ev(("beam_consensus", 8, 0.7, 0.25))
    ev(["beam_consensus", 8, 0.7, 0.25, div])
    assert calls == [("bon", 4, 0.9, 5, 7, dict(top_p=1.0, consensus_weight=0.5)), ("bon", 4, 0.9, 5, 7, dict(top_p=0.8, consensus_weight=0.5)),
                     ("bob", 8, 0.7, dict(consensus_weight=0.25)), ("bob", 8, 0.7, dict(consensus_weight=0.25, **div))]
    for bad in (("best_of_consensus", 4, 0.9, 5, 7), ("best_of_consensus", 4, 0.9, 5), ("best_of_consensus", 4, 0.9, 5, 7, 0.5, 0.8, 1),
                ("beam_consensus", 8, 0.7), ("beam_consensus", 8), ("beam_consensus", 8, 0.7, 0.25, 2), ("beam_consensus", 8, 0.7, 0.25, div, div),
                ("beam_consensus", 8, 0.7, 0.25, dict(groups=2))):
        with pytest.raises(ValueError):
            ev(bad)
    assert len(calls) == 4


def test_library_exports_and_null_handle():
    """The C ABI refuses a NULL handle first (no GPU needed); the op and the prototype are declared."""
    from recnet_amd import _lib, _ops
    lib = _lib.load()
    assert "recnet_consensus_rows" in _lib.EXPORTS and "consensus_rows" in _ops.OP_NAMES
    assert lib.recnet_consensus_rows(None, None, 2, 4, None, 2, 4, 3, None, 6.0, None, None, None, None, None, None, None, None) == -2
    assert math.isfinite(CR.BAR)
