"""The per-caption reconstruction error without a GPU: the float64 restatement (tests/recon_ref.py) is pinned to the reference's own
MSE term on the eval goldens — mean_b err[b] == rec_mse — and four plausible wrong definitions are shown to miss that pin; the host
side of the feature (search.canonical_captions, pick_best_of_n's combined score, the argument checks of
search.reconstruction_errors) is held where no engine exists."""

import numpy as np
import pytest
import torch

from tests import recon_ref as RR
from tests.gpu_util import TOL, load_case
from tests.search_kit import Cfg, no_library

PIN = TOL["f32"]["loss"]          # relative bar of mean(err) against the golden rec_mse (the gap is the reference's own float32)


def _golden(name):
    g, dims, kind, decP, recP, enc, targets = load_case(name)
    assert not int(g["meta_train_mode"])
    return g, kind, recP, enc, g["_cells"][1]


def _gap(g, kind, recP, enc, cell, mutation=None):
    err, _ = RR.per_caption_error(recP, kind, g["hiddens"], enc, cell=cell, mutation=mutation)
    ref = float(g["rec_mse"])
    return abs(float(err.mean()) - ref) / abs(ref), err


@pytest.mark.parametrize("name", RR.GOLDENS)
def test_mean_of_the_per_caption_errors_is_the_references_mse(name):
    g, kind, recP, enc, cell = _golden(name)
    gap, err = _gap(g, kind, recP, enc, cell)
    print(name, "relative gap to rec_mse:", gap, "per-caption spread:", float(err.min()), float(err.max()))
    assert err.shape == (enc.shape[0],) and (err > 0).all()
    assert gap <= PIN, (gap, PIN)


@pytest.mark.parametrize("mutation", RR.MUTATIONS)
def test_wrong_definitions_miss_the_pin(mutation):
    """Dropping the / T, summing instead of averaging, dropping the caption_max_len / T^2 rescale of the pooled states, comparing
    against frame 0 instead of the frame mean: each exceeds the bar on every golden it applies to (the local form has no T, no
    pooled states and no frame mean: only the sum applies)."""
    seen = 0
    for name in RR.GOLDENS:
        g, kind, recP, enc, cell = _golden(name)
        if kind == "local" and mutation != "sum_not_mean":
            continue
        gap, _ = _gap(g, kind, recP, enc, cell, mutation)
        print(name, mutation, "relative gap:", gap)
        assert gap > PIN, (name, mutation, gap)
        seen += 1
    assert seen >= 1


def test_reconstruction_has_the_public_layout():
    g, kind, recP, enc, cell = _golden("local_eval")
    err, recon = RR.per_caption_error(recP, kind, g["hiddens"], enc, cell=cell)
    assert recon.shape == tuple(enc.shape)
    assert np.allclose(err, ((recon - enc.numpy().astype(np.float64)) ** 2).mean((1, 2)), rtol=1e-12)
    g, kind, recP, enc, cell = _golden("global_eval")
    err, recon = RR.per_caption_error(recP, kind, g["hiddens"], enc, cell=cell)
    assert recon.shape == (enc.shape[0], enc.shape[2])


# ------------------------------------------------------------------------------------------------ canonical_captions
CANON_CASES = [
    #  captions [T0][B]                                                       T     expected
    ("eos at row 0", [[2, 5, 2], [7, 8, 9], [2, 2, 3]], None, [[2, 5, 2], [0, 8, 0], [0, 2, 0]]),
    ("no eos at all", [[3, 4], [5, 6], [7, 8]], None, [[3, 4], [5, 6], [7, 8]]),
    ("padding", [[3, 2], [2, 9]], 4, [[3, 2], [2, 0], [0, 0], [0, 0]]),
    ("T equals T0", [[3, 2], [4, 2]], 2, [[3, 2], [4, 0]]),
    ("already canonical", [[3, 4], [2, 5], [0, 2], [0, 0]], 5, [[3, 4], [2, 5], [0, 2], [0, 0], [0, 0]]),
    ("tokens behind eos incl. pad and eos", [[4], [2], [0], [2], [6]], None, [[4], [2], [0], [0], [0]]),
]


@pytest.mark.parametrize("what,caps,T,want", CANON_CASES, ids=[c[0] for c in CANON_CASES])
def test_canonical_captions(what, caps, T, want):
    from recnet_amd import canonical_captions
    for given in (caps, torch.tensor(caps)):
        out = canonical_captions(given, T)
        assert out.dtype == torch.long and out.tolist() == want
    assert RR.canonical(caps, T).tolist() == want
    if isinstance(given, torch.Tensor):
        assert given.tolist() == caps                     # the argument is not modified


def test_canonical_captions_random_tables_and_errors():
    from recnet_amd import canonical_captions
    rs = np.random.RandomState(5)
    for _ in range(20):
        T0, B = rs.randint(1, 9), rs.randint(1, 6)
        caps = rs.randint(0, 6, size=(T0, B))
        T = None if rs.rand() < 0.3 else T0 + rs.randint(0, 4)
        assert canonical_captions(torch.from_numpy(caps), T).tolist() == RR.canonical(caps, T).tolist()
    with pytest.raises(ValueError, match="T must be"):
        canonical_captions([[3, 4], [5, 6]], 1)
    with pytest.raises(ValueError, match="LongTensor"):
        canonical_captions(torch.zeros(2, 3))
    # other ids for <EOS> / <PAD>
    assert canonical_captions([[7, 3], [4, 7], [5, 5]], 4, eos=7, pad=9).tolist() == [[7, 3], [9, 7], [9, 9], [9, 9]]


# ------------------------------------------------------------------------------------------------ pick_best_of_n
def _parent_pick(caption_logprobs, lengths):
    """pick_best_of_n as it was before the reconstruction term."""
    n = len(caption_logprobs)
    B = len(caption_logprobs[0]) if n else 0
    ks, scores = [], []
    for b in range(B):
        best_k, best = 0, caption_logprobs[0][b] / lengths[0][b]
        for k in range(1, n):
            s = caption_logprobs[k][b] / lengths[k][b]
            if s > best:
                best_k, best = k, s
        ks.append(best_k); scores.append(best)
    return ks, scores


def _tables(rs, n, B, ties):
    lens = rs.randint(1, 9, size=(n, B))
    lp = -rs.randint(1, 40, size=(n, B)) / 4.0 if ties else -rs.rand(n, B) * 20
    er = rs.randint(0, 6, size=(n, B)) / 8.0 if ties else rs.rand(n, B)
    return lp.tolist(), lens.tolist(), er.tolist()


def test_pick_best_of_n_defaults_are_the_parent_rule():
    from recnet_amd import pick_best_of_n
    rs = np.random.RandomState(11)
    for i in range(40):
        lp, lens, er = _tables(rs, rs.randint(1, 6), rs.randint(1, 7), ties=i % 2 == 0)
        want = _parent_pick(lp, lens)
        assert pick_best_of_n(lp, lens) == want
        assert pick_best_of_n(lp, lens, None, 3.0) == want            # no errors given: the weight has nothing to weigh
        ks, scores = pick_best_of_n(lp, lens, er, 0.0)                # weight 0 with errors: the same choice and values
        assert ks == want[0] and scores == want[1]
    assert pick_best_of_n([], []) == ([], [])


def test_pick_best_of_n_with_errors_is_the_brute_force_argmax():
    from recnet_amd import pick_best_of_n
    rs = np.random.RandomState(12)
    changed = 0
    for i in range(60):
        lp, lens, er = _tables(rs, rs.randint(2, 6), rs.randint(1, 7), ties=i % 2 == 0)
        w = float(rs.choice([0.25, 1.0, 8.0]))
        got = pick_best_of_n(lp, lens, er, w)
        assert got == RR.pick(lp, lens, er, w)
        changed += got[0] != _parent_pick(lp, lens)[0]
    assert changed > 10                                               # the term does change winners
    # hand-made: the error decides, a tie goes to the lowest k, a negative weight prefers the larger error
    lp, lens = [[-2.0, -2.0, -2.0], [-2.0, -2.0, -4.0]], [[2, 2, 2], [2, 2, 2]]
    er = [[0.5, 0.25, 0.0], [0.25, 0.25, 0.0]]
    assert pick_best_of_n(lp, lens, er, 1.0) == ([1, 0, 0], [-1.25, -1.25, -1.0])
    assert pick_best_of_n(lp, lens, er, -1.0)[0] == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ argument checks before any launch
_V = 41
_GOOD = [[3, 4, 5, 6], [7, 2, 2, 8]]
BAD_CALLS = [
    ("ragged", dict(captions=[[3, 4, 5, 6], [7, 2, 2]]), r"captions\[1\]"),
    ("no steps", dict(captions=[]), "steps"),
    ("too many steps", dict(captions=[[3, 4, 5, 6]] * 32), "steps"),
    ("wrong B", dict(captions=[[3, 4, 5], [7, 2, 2]]), r"captions\[0\]"),
    ("token V", dict(captions=[[3, 4, 5, 6], [7, 2, _V, 8]]), r"captions\[1\]\[2\] = 41"),
    ("token negative", dict(captions=[[3, -1, 5, 6]]), r"captions\[0\]\[1\] = -1"),
    ("tensor token V", dict(captions=torch.tensor([[3, 4, 5, 6], [7, 2, _V, 8]])), "token 41"),
    ("tensor dtype", dict(captions=torch.zeros(2, 4)), "LongTensor"),
    ("tensor rank", dict(captions=torch.zeros(2, 4, 1, dtype=torch.long)), "LongTensor"),
    ("T below the captions", dict(captions=_GOOD, T=1), "T must be"),
    ("T above caption_max_len + 1", dict(captions=_GOOD, T=32), "T must be"),
    ("T fractional", dict(captions=_GOOD, T=2.5), "T must be"),
    ("features rank", dict(captions=_GOOD, encoder_outputs=torch.zeros(4, 32)), "encoder_outputs must be"),
    ("features size", dict(captions=_GOOD, encoder_outputs=torch.zeros(4, 5, 16)), "features per frame"),
    ("no reconstructor", dict(captions=_GOOD, reconstructor=None), "reconstructor must be"),
]


@pytest.mark.parametrize("kind", ["global", "local"])
@pytest.mark.parametrize("what,kw,match", BAD_CALLS, ids=[c[0] for c in BAD_CALLS])
def test_reconstruction_errors_checks_its_arguments_before_the_library(what, kw, match, kind, monkeypatch):
    import recnet_amd as R
    no_library(monkeypatch)
    dec = R.Decoder("LSTM", 1, 32, 12, 1, 24, 8, _V, 0.5, 0.5, 0.5, precision="f32")
    rec = (R.GlobalReconstructor("LSTM", 1, 24, 32, 0.5, 0.5, 30, precision="f32") if kind == "global"
           else R.LocalReconstructor("LSTM", 1, 24, 32, 0.5, 0.5, 8, precision="f32"))
    kw = dict(kw)
    enc = kw.pop("encoder_outputs", torch.zeros(4, 5, 32))
    rec = kw.pop("reconstructor", rec)
    with pytest.raises(ValueError, match=match):
        R.reconstruction_errors(Cfg(), dec, rec, enc, **kw)


def test_mismatched_models_are_refused_before_the_library(monkeypatch):
    import recnet_amd as R
    no_library(monkeypatch)
    dec = R.Decoder("LSTM", 1, 32, 12, 1, 24, 8, _V, 0.5, 0.5, 0.5, precision="f32")
    enc = torch.zeros(4, 5, 32)
    with pytest.raises(ValueError, match="decoder states"):
        R.reconstruction_errors(Cfg(), dec, R.LocalReconstructor("LSTM", 1, 16, 32, 0.5, 0.5, 8, precision="f32"), enc, _GOOD)
    with pytest.raises(ValueError, match="caption_max_len"):
        R.reconstruction_errors(Cfg(), dec, R.GlobalReconstructor("LSTM", 1, 24, 32, 0.5, 0.5, 20, precision="f32"), enc, _GOOD)
    with pytest.raises(ValueError, match="precision"):
        R.reconstruction_errors(Cfg(), dec, R.LocalReconstructor("LSTM", 1, 24, 32, 0.5, 0.5, 8, precision="bf16"), enc, _GOOD)
    inp = torch.full((1, 4), 1, dtype=torch.long)
    hid = (torch.zeros(1, 4, 24), torch.zeros(1, 4, 24))
    with pytest.raises(ValueError, match="needs a reconstructor"):
        R.best_of_n(Cfg(), dec, inp, hid, enc, 2, recon_weight=0.5)
    with pytest.raises(ValueError, match="finite"):
        R.best_of_n(Cfg(), dec, inp, hid, enc, 2, reconstructor=R.LocalReconstructor("LSTM", 1, 24, 32, 0.5, 0.5, 8, precision="f32"),
                    recon_weight=float("nan"))
