"""The CPU restatement of the N-best beam search (tests/beam_ref.py) pinned to truths the suite already holds: width 1 is the
reference's greedy search, a hypothesis' cum is score_ref's caption log-probability of its own tokens, finished hypotheses never
change, ranks are ordered; and the share of decisions each run used on the GPU compares (the caps of the issue)."""
import functools

import numpy as np
import pytest

from tests import beam_ref as BR
from tests import score_ref as SC
from tests.golden_util import CASES, load_search_case


@functools.lru_cache(maxsize=None)
def _run(name, bw, cml, alpha=BR.LENGTH_ALPHA):
    g, P, enc = load_search_case(name)
    return BR.beam_search_nbest(P, enc, bw, alpha, cml, g["_cell"])


@pytest.mark.parametrize("name", CASES)
def test_width_one_is_greedy_up_to_eos(name):
    """Greedy goes on after <EOS>, the beam carries <PAD>: equal up to each caption's first <EOS>, over greedy's steps."""
    g, P, enc = load_search_case(name)
    r = _run(name, 1, 30)
    greedy = np.asarray(g["greedy"])                 # [n][B]
    toks = r["tokens"][0]
    for b in range(greedy.shape[1]):
        n = min(greedy.shape[0], toks.shape[0])
        eos = np.nonzero(greedy[:n, b] == BR.EOS)[0]
        upto = int(eos[0]) + 1 if eos.size else n
        assert np.array_equal(toks[:upto, b], greedy[:upto, b]), (name, b)


@pytest.mark.parametrize("name,bw,cml,cap", BR.SEARCH_RUNS)
def test_runs_hold_their_caps_and_invariants(name, bw, cml, cap):
    g, P, enc = load_search_case(name)
    r = _run(name, bw, cml)
    share = BR.compared_share(r)
    print(name, bw, cml, "share of compared decisions:", share, "captions compared:", int(BR.comparable_captions(r).sum()))
    assert share >= cap, (name, bw, cml, share)
    assert abs(share - BR.RUN_SHARES[(name, bw, cml)]) < 1e-3
    keep = BR.comparable_captions(r)
    assert int(keep.sum()) == BR.RUN_CAPTIONS[(name, bw, cml)]
    # what the device test can check: captions in full, or the prefixes of the excluded ones
    assert keep.any() or BR.comparable_steps(r["margins"]).sum(axis=0)[~keep].max() > 0
    n, B = r["n_steps"], enc.shape[0]
    assert r["tokens"].shape == (bw, n, B) and 1 <= n <= cml + 1
    # cum is the caption log-probability of the hypothesis' own tokens, len the scorer's length; ranks are canonical
    for k in range(bw):
        toks = r["tokens"][k]
        lp, _ = SC.score_captions(P, enc, toks, 1.0, cell=g["_cell"])
        sums, lens = SC.caption_sums(lp, toks)
        assert np.array_equal(lens, r["len"][k]), (k, lens, r["len"][k])
        assert np.allclose(sums, r["cum"][k], rtol=0, atol=1e-4), (k, sums, r["cum"][k])      # (the oracle's step is fp32)
        for b in range(B):
            assert (toks[r["len"][k][b]:, b] == BR.PAD).all()
            assert (toks[:r["len"][k][b] - 1, b] != BR.EOS).all()
    assert np.allclose(r["score"], r["cum"] / r["len"] ** BR.LENGTH_ALPHA)
    assert (np.diff(r["score"], axis=0) <= 0).all()
    # selection order: cum descending after every step; a finished hypothesis that stays in the beam never changes
    prev = None
    for t, (tok, fin, cum, hist) in enumerate(r["trace"]):
        assert (np.diff(cum, axis=0) <= 0).all()
        assert ((fin == 0) | (fin <= t + 1)).all()
        assert (tok[fin == t + 1] == BR.EOS).all() and (tok[(fin > 0) & (fin <= t)] == BR.PAD).all()
        for k, b in zip(*np.nonzero((fin > 0) & (fin <= t))):
            pf, pc, ph = prev
            assert any(pf[j, b] == fin[k, b] and pc[j, b] == cum[k, b] and np.array_equal(ph[j, b], hist[k, b, :t]) for j in range(bw))
        prev = (fin, cum, hist)
    if (r["trace"][-1][1] > 0).all():
        assert all((tr[1] == 0).any() for tr in r["trace"][:-1])           # it stopped at the FIRST all-finished step
    else:
        assert n == cml + 1


def test_alpha_zero_ranks_by_the_raw_sum():
    r = _run("search_eos", 3, 7, 0.0)
    assert np.array_equal(r["score"], r["cum"]) and (np.diff(r["cum"], axis=0) <= 0).all()


@pytest.mark.parametrize("V,nb", [(8, 1), (8, 3), (61, 8), (257, 3)])
def test_select_rows_rules(V, nb):
    """Ties by flat index, finished hypotheses offer <PAD> alone, -inf only when the candidates run out."""
    for kind in BR.ROW_KINDS:
        x, cum, fin = BR.row_case(V, nb, kind)
        for bw in BR.ROW_BW:
            if bw > V:
                continue
            vals, idx, margin = BR.select_rows(x, cum, fin, bw)
            assert (vals[:, 1:] <= vals[:, :-1]).all()
            src, tok = idx // V, idx % V
            for r in range(x.shape[1]):
                assert len(set(idx[r])) == bw
                for k in range(bw):
                    if fin[src[r, k], r] and np.isfinite(vals[r, k]):
                        assert tok[r, k] == BR.PAD and vals[r, k] == np.float64(cum[src[r, k], r])
                    if k and vals[r, k] == vals[r, k - 1]:
                        assert idx[r, k] > idx[r, k - 1]
            if kind == "twins" and nb > 1 and bw > 1:
                for r, k in zip(*np.nonzero(src == nb - 1)):             # the twin in the higher beam follows its equal in beam 0
                    assert k > 0 and idx[r, k - 1] == idx[r, k] - (nb - 1) * V and vals[r, k - 1] == vals[r, k]
            if kind == "all_finished":
                assert np.isfinite(vals[:, :min(bw, nb)]).all() and np.isneginf(vals[:, nb:]).all()


def test_library_exports_and_argument_checks():
    """The C ABI refuses its arguments before anything is launched (no GPU needed: a NULL handle is refused first)."""
    from recnet_amd import _lib
    assert _lib.ABI_VERSION == 12
    lib = _lib.load()
    assert lib.recnet_beam_select_rows(None, None, None, None, 1, 1, 8, 1, None, None, None) == -2
    assert lib.recnet_beam_search_nbest(None, None, 3, 0.7, None, None, None, None, None, None) == -2


@pytest.mark.parametrize("kw", [dict(beam_width=0), dict(beam_width=9), dict(beam_width=2.5), dict(beam_width=3, length_alpha=-0.1),
                                dict(beam_width=3, length_alpha=float("nan")), dict(beam_width=3, length_alpha=float("inf"))])
def test_python_search_checks_its_arguments_before_the_library(kw, monkeypatch):
    import torch
    import recnet_amd as R
    from recnet_amd import search

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(search, "_nbest_engine", boom)

    class Dec:
        output_size = 61
    inp = torch.full((1, 4), 1, dtype=torch.long)
    with pytest.raises(ValueError):
        R.beam_search_nbest(None, Dec(), inp, torch.zeros(1, 4, 8), torch.zeros(4, 5, 32), **kw)
    with pytest.raises(ValueError):
        R.best_of_beam(None, Dec(), inp, torch.zeros(1, 4, 8), torch.zeros(4, 5, 32), **kw)
    with pytest.raises(ValueError, match="needs a reconstructor"):
        R.best_of_beam(None, Dec(), inp, torch.zeros(1, 4, 8), torch.zeros(4, 5, 32), 3, recon_weight=0.5)
