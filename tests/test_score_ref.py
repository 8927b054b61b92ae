"""Caption scoring without a GPU: the CPU restatement (tests/score_ref.py) is pinned to the reference's own eval-mode logits
and to the sampling restatement's rollouts, its per-caption rule is search.sequence_logprob's, and the host side of the feature
— search.score_captions' argument checks, best_of_n's selection rule — is held where no engine exists."""
import math

import numpy as np
import pytest
import torch

from tests import golden_util as GU
from tests import sample_ref as SR
from tests import score_ref as SC
from tests.golden_util import load_search_case
from tests.gpu_util import load_case
from tests.search_kit import Cfg, no_library


@pytest.mark.parametrize("name", SC.EVAL_GOLDENS)
def test_restatement_reproduces_the_references_eval_logits(name):
    """Targets as captions: the restatement's per-step values equal log_softmax(step_logits)[target] of the reference's own
    step_logits on every row up to each caption's <EOS>, within the fp32 row bar."""
    g, dims, kind, decP, recP, enc, targets = load_case(name)
    assert not int(g["meta_train_mode"])
    T = g["step_logits"].shape[0]
    caps = targets.numpy()[:T]
    lp, amax = SC.score_captions(decP, enc, caps, 1.0, cell=g["_cells"][0])
    ref = SC.golden_logprobs(g["step_logits"], caps)
    _, lens = SC.caption_sums(lp, caps)
    worst = 0.0
    for t in range(T):
        live = lens > t
        assert live.any() or t > 0
        err = np.abs(lp[t] - ref[t])[live]
        bar = SC.row_bar("f32", np.abs(g["step_logits"][t]).max(), 1.0)
        if err.size:
            worst = max(worst, float(err.max() / bar))
            assert err.max() <= bar, (t, float(err.max()), bar)
    print(name, "T", T, "worst error / bar:", worst)


@pytest.mark.parametrize("name,seed,temperature,top_k", [r for r in SR.SEARCH_RUNS if r[3] == 0])
def test_restatement_reproduces_the_sampling_loops_logprobs(name, seed, temperature, top_k):
    """Rollouts of the sampling restatement, re-scored at the same temperature: the same log-probabilities on all n_steps rows
    (same float32 logits, same float64 log-sum-exp), caption sums equal to sequence_logprob, lengths = first <EOS> + 1 or
    n_steps."""
    from recnet_amd import sequence_logprob
    g, P, enc = load_search_case(name)
    toks, lps, _, amax = SR.sample_search(P, enc, temperature, top_k, seed, cell=g["_cell"])
    n, B = toks.shape
    if name.endswith("_stop"):
        assert n == 1
    lp, amax2 = SC.score_captions(P, enc, toks, temperature, cell=g["_cell"])
    assert lp.shape == (n, B) and np.array_equal(amax, amax2)
    assert np.abs(lp - lps).max() <= 1e-12 * max(1.0, np.abs(lps).max())
    sums, lens = SC.caption_sums(lp, toks)
    seq = sequence_logprob(toks.tolist(), lp.tolist())
    assert np.abs(sums - np.array(seq)).max() <= 1e-12 * max(1.0, np.abs(sums).max())
    for b in range(B):
        hit = [t for t in range(n) if toks[t][b] == 2]
        assert lens[b] == (hit[0] + 1 if hit else n)


def test_hand_made_edge_cases():
    from recnet_amd import sequence_logprob
    ninf = -np.inf
    #                 b0: <EOS> at step 0   b1: at the last step   b2: none   b3: in the middle, -inf behind it
    tokens = np.array([[2, 5, 6, 7], [9, 8, 9, 2], [0, 2, 9, 0]])
    lp = np.array([[-1.0, -0.5, -0.25, -4.0], [ninf, -2.0, -0.125, -8.0], [ninf, -16.0, -32.0, ninf]])
    sums, lens = SC.caption_sums(lp, tokens)
    assert lens.tolist() == [1, 3, 3, 2]
    assert sums.tolist() == [-1.0, -18.5, -32.375, -12.0] and np.isfinite(sums).all()
    assert sequence_logprob(tokens.tolist(), lp.tolist()) == sums.tolist()
    # a -inf row at or before the <EOS> does enter the sum
    s2, _ = SC.caption_sums(np.array([[ninf], [-1.0]]), np.array([[5], [2]]))
    assert s2[0] == ninf
    # V = 1: exactly 0 at every temperature; out-of-range tokens: -inf
    for temperature in (0.5, 1.0, 2.0):
        assert SC.logprob_rows(np.array([[3.5]], dtype=np.float32), [0], temperature).tolist() == [0.0]
    x = SC.row_logits(61, 5, "gauss60")
    lpr = SC.logprob_rows(x, [0, 60, -1, 61, int(x[4].argmax())], 0.5)
    assert np.isfinite(lpr[[0, 1, 4]]).all() and (lpr[[0, 1, 4]] <= 0).all() and np.isneginf(lpr[[2, 3]]).all()
    # the log-probabilities of a row sum to one
    p = np.exp(SC.logprob_rows(np.repeat(x[:1], 61, axis=0), np.arange(61), 2.0)).sum()
    assert abs(p - 1.0) < 1e-12


def test_row_cases_cover_every_kind_of_token():
    for V in SC.ROW_VS:
        kinds = set()
        for rows, kind, temperature, shift in SC.row_cases(V):
            x = SC.row_logits(V, rows, kind)
            tok = SC.row_case_tokens(x, shift)
            kinds |= {"neg" if k < 0 else "over" if k >= V else "in" for k in tok}
            assert np.isfinite(SC.logprob_rows(x, tok, temperature)[(tok >= 0) & (tok < V)]).all()
        assert kinds == {"neg", "over", "in"}, V


# ------------------------------------------------------------------------------------------------ host side of the feature
_V = 41
_GOOD = [[3, 4, 5, 6], [7, 2, 2, 8]]
BAD_CALLS = [
    ("temperature zero", dict(captions=_GOOD, temperature=0.0), "temperature"),
    ("temperature negative", dict(captions=_GOOD, temperature=-1.0), "temperature"),
    ("temperature nan", dict(captions=_GOOD, temperature=float("nan")), "temperature"),
    ("temperature inf", dict(captions=_GOOD, temperature=float("inf")), "temperature"),
    ("ragged", dict(captions=[[3, 4, 5, 6], [7, 2, 2]]), r"captions\[1\]"),
    ("no steps", dict(captions=[]), "steps"),
    ("too many steps", dict(captions=[[3, 4, 5, 6]] * 32), "steps"),
    ("wrong B", dict(captions=[[3, 4, 5], [7, 2, 2]]), r"captions\[0\]"),
    ("token V", dict(captions=[[3, 4, 5, 6], [7, 2, _V, 8]]), r"captions\[1\]\[2\] = 41"),
    ("token negative", dict(captions=[[3, -1, 5, 6]]), r"captions\[0\]\[1\] = -1"),
    ("tensor no steps", dict(captions=torch.zeros(0, 4, dtype=torch.long)), "steps"),
    ("tensor too many steps", dict(captions=torch.zeros(32, 4, dtype=torch.long)), "steps"),
    ("tensor wrong B", dict(captions=torch.zeros(3, 5, dtype=torch.long)), "captions"),
    ("tensor token V", dict(captions=torch.tensor([[3, 4, 5, 6], [7, 2, _V, 8]])), "token 41"),
    ("tensor token negative", dict(captions=torch.tensor([[3, -7, 5, 6]])), "token -7"),
    ("tensor dtype", dict(captions=torch.zeros(2, 4)), "LongTensor"),
]


@pytest.mark.parametrize("what,kw,match", BAD_CALLS, ids=[c[0] for c in BAD_CALLS])
def test_score_captions_checks_its_arguments_before_the_library(what, kw, match, monkeypatch):
    import recnet_amd as R
    no_library(monkeypatch)
    dec = R.Decoder("LSTM", 1, 32, 12, 1, 24, 8, _V, 0.5, 0.5, 0.5, precision="f32")
    with pytest.raises(ValueError, match=match):
        R.score_captions(Cfg(), dec, torch.zeros(4, 5, 32), **kw)


def test_good_arguments_pass_the_checks_and_reach_the_engine():
    """The same call with valid arguments gets past every check: on a box without a GPU it fails at engine creation."""
    import recnet_amd as R
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import __graft_entry__ as g
    g.build()
    dec = R.Decoder("LSTM", 1, 32, 12, 1, 24, 8, _V, 0.5, 0.5, 0.5, precision="f32")
    for caps in (_GOOD, torch.tensor(_GOOD), [[3, 4, 5, 6]] * 31):
        with pytest.raises(RuntimeError, match="needs a GPU"):
            R.score_captions(Cfg(), dec, torch.zeros(4, 5, 32), caps)


def test_best_of_n_selection_rule():
    from recnet_amd import pick_best_of_n
    #        b0: plain maximum   b1: the longer caption wins on the normalised score   b2: tie -> lowest k   b3: single best last
    caps = [[-4.0, -6.0, -3.0, -9.0],
            [-2.0, -8.0, -6.0, -9.0],
            [-3.0, -9.0, -1.5, -2.0]]
    lens = [[2, 2, 2, 3],
            [2, 4, 4, 3],
            [2, 3, 1, 1]]
    ks, scores = pick_best_of_n(caps, lens)
    assert ks == [1, 1, 0, 2]
    assert scores == [-1.0, -2.0, -1.5, -2.0]
    # one candidate: it is chosen; all equal: the first
    assert pick_best_of_n([[-1.0, -2.0]], [[1, 4]]) == ([0, 0], [-1.0, -0.5])
    assert pick_best_of_n([[-2.0], [-2.0], [-2.0]], [[2], [2], [2]]) == ([0], [-1.0])
    # equal normalised scores from different (sum, length) pairs are still a tie
    assert pick_best_of_n([[-3.0], [-1.5]], [[4], [2]])[0] == [0]
    assert pick_best_of_n([], []) == ([], [])
    assert all(math.isfinite(s) for s in scores)


def test_best_of_n_checks_n_before_the_library(monkeypatch):
    import recnet_amd as R
    no_library(monkeypatch)
    dec = R.Decoder("LSTM", 1, 32, 12, 1, 24, 8, _V, 0.5, 0.5, 0.5, precision="f32")
    inp = torch.full((1, 4), 1, dtype=torch.long)
    hid = (torch.zeros(1, 4, 24), torch.zeros(1, 4, 24))
    for n in (0, -1, 2.5):
        with pytest.raises(ValueError, match="n must be"):
            R.best_of_n(Cfg(), dec, inp, hid, torch.zeros(4, 5, 32), n)
