"""The CPU restatement of the diverse (group) N-best beam search (tests/beam_diverse_ref.py) pinned to what the
suite already holds: with one group it is tests/beam_constrained_ref.py's search, with lambda = 0 every group is a copy of the plain
search at the group width, group 0 always is, cum stays score_ref's log-probability of the hypothesis' own tokens, and each run
keeps the share of compared decisions the issue lists (cap 0.6).  Then the constructed kernel-alone cases, nbest_diversity, the
argument checks of the Python layer and of the C ABI, and evaluate()'s new keys."""
import functools

import numpy as np
import pytest

from tests import beam_constrained_ref as CR
from tests import beam_diverse_ref as DR
from tests import beam_ref as BR
from tests import score_ref as SC
from tests.golden_util import load_search_case


@functools.lru_cache(maxsize=None)
def _plain(name, bw, cml, n=0, m=0, banned=()):
    g, P, enc = load_search_case(name)
    return CR.beam_search_nbest(P, enc, bw, BR.LENGTH_ALPHA, cml, g["_cell"], n, m, banned)


@functools.lru_cache(maxsize=None)
def _diverse(name, bw, G, lam, cml, n=0, m=0, banned=()):
    g, P, enc = load_search_case(name)
    return DR.beam_search_nbest(P, enc, bw, G, lam, BR.LENGTH_ALPHA, cml, g["_cell"], n, m, banned)


def _run_args(run):
    return run["name"], run["bw"], run["G"], run["lam"], run["cml"], run["n"], run["m"], run["banned"]


_ONE_GROUP = [("search_small_b", 3, 7, 0, 0, ()), ("search_eos", 3, 7, 0, 0, ()), ("search_gru", 8, 7, 0, 0, ()),
              ("search_gru_b", 5, 30, 0, 0, ()), ("search_eos", 3, 7, 0, 4, ()), ("search_gru", 3, 7, 2, 3, (55, 78)),
              ("search_gru", 3, 30, 1, 0, ())]


@pytest.mark.parametrize("name,bw,cml,n,m,banned", _ONE_GROUP)
@pytest.mark.parametrize("lam", [0.0, 2.0])
def test_one_group_is_the_existing_restatement(name, bw, cml, n, m, banned, lam):
    """Where the existing search stops early the slots are in cum order already, so the further selection changes nothing."""
    a, b = _plain(name, bw, cml, n, m, banned), _diverse(name, bw, 1, lam, cml, n, m, banned)
    for k in ("tokens", "cum", "len", "score", "margins", "final_margin", "amax"):
        assert np.array_equal(a[k], b[k]), k
    assert a["n_steps"] == b["n_steps"] and len(a["trace"]) == len(b["trace"])
    for ta, tb in zip(a["trace"], b["trace"]):
        assert all(np.array_equal(x, y) for x, y in zip(ta, tb))
    assert (b["group"] == 0).all()


def _assert_group_is_plain(r, g, w, plain):
    """Slots g * w .. g * w + w - 1 of every step of r are the plain width-w search's beams."""
    assert len(plain["trace"]) <= len(r["trace"])
    for (tok, fin, cum, hist), (ptok, pfin, pcum, phist) in zip(r["trace"], plain["trace"]):
        s = slice(g * w, g * w + w)
        assert np.array_equal(tok[s], ptok) and np.array_equal(fin[s], pfin) and np.array_equal(cum[s], pcum) and np.array_equal(hist[s], phist)


@pytest.mark.parametrize("run", [r for r in DR.RUNS if r["lam"] == 0.5 and not r["banned"]][:8], ids=DR.run_id)
def test_lambda_zero_gives_equal_copies(run):
    name, bw, G, _, cml, n, m, banned = _run_args(run)
    w = bw // G
    r, plain = _diverse(name, bw, G, 0.0, cml, n, m, banned), _plain(name, w, cml, n, m, banned)
    for g in range(G):
        _assert_group_is_plain(r, g, w, plain)
    if plain["n_steps"] == r["n_steps"]:
        # the ranks: every plain rank G times, the groups in ascending order among the equal scores
        for k in ("cum", "len", "score"):
            assert np.array_equal(r[k], np.repeat(plain[k], G, axis=0)), k
        assert np.array_equal(r["tokens"], np.repeat(plain["tokens"], G, axis=0))
        assert np.array_equal(r["group"], np.tile(np.arange(G)[:, None], (w, r["group"].shape[1])))


@pytest.mark.parametrize("run", DR.RUNS[:6] + DR.RUNS[15:18], ids=DR.run_id)
@pytest.mark.parametrize("lam", [0.5, 1e4])
def test_group_zero_is_the_plain_search(run, lam):
    name, bw, G, _, cml, n, m, banned = _run_args(run)
    w = bw // G
    _assert_group_is_plain(_diverse(name, bw, G, lam, cml, n, m, banned), 0, w, _plain(name, w, cml, n, m, banned))


def _live_tokens(r, t):
    """(tokens [bw][B] of step t, True where the candidate came from a live hypothesis)"""
    tok, fin = r["trace"][t][0], r["trace"][t][1]
    return tok, (fin == 0) | (fin == t + 1)


@pytest.mark.parametrize("run", DR.RUNS, ids=DR.run_id)
def test_runs_hold_their_table(run):
    name, bw, G, lam, cml, n, m, banned = _run_args(run)
    w = bw // G
    g, P, enc = load_search_case(name)
    B, V = enc.shape[0], int(g["meta_dims"][3])
    r = _diverse(name, bw, G, lam, cml, n, m, banned)
    share, keep = DR.compared_share(r), DR.comparable_captions(r)
    lists = [[r["tokens"][k, :r["len"][k, b], b].tolist() for k in range(bw)] for b in range(B)]
    print(DR.run_id(run), "steps", r["n_steps"], "share %.3f" % share, "captions compared in full", int(keep.sum()), "of", B,
          "diversity", DR.nbest_diversity(lists))
    assert r["n_steps"] == run["steps"]
    assert share >= DR.CAP and abs(share - run["share"]) < 1e-3
    assert (int(keep.sum()), B) == run["full"]
    if n or m or banned:
        assert bw + len(banned) + cml + 1 <= V
        assert CR.violations(r["tokens"], r["len"], n, m, banned) == (0, 0, 0)
    # cum is the model's log-probability of the hypothesis' own tokens (no penalty in the value), len the scorer's length
    ns = r["n_steps"]
    assert r["tokens"].shape == (bw, ns, B) and np.isfinite(r["cum"]).all()
    for k in range(bw):
        toks = r["tokens"][k]
        lp, _ = SC.score_captions(P, enc, toks, 1.0, cell=g["_cell"])
        sums, lens = SC.caption_sums(lp, toks)
        assert np.array_equal(lens, r["len"][k]), (k, lens, r["len"][k])
        assert np.allclose(sums, r["cum"][k], rtol=0, atol=1e-4), (k, sums, r["cum"][k])      # (the oracle's step is fp32)
        for b in range(B):
            assert (toks[r["len"][k][b]:, b] == BR.PAD).all()
    assert np.allclose(r["score"], r["cum"] / r["len"] ** BR.LENGTH_ALPHA) and (np.diff(r["score"], axis=0) <= 0).all()
    assert ((r["group"] >= 0) & (r["group"] < G)).all() and all((np.bincount(r["group"][:, b], minlength=G) == w).all() for b in range(B))
    for t, (tok, fin, cum, hist) in enumerate(r["trace"]):
        assert np.isfinite(cum).all()
        for k, b in zip(*np.nonzero((fin == 0) | (fin == t + 1))):
            assert int(tok[k, b]) not in CR.banned_ids(hist[k, b], t, n, m, banned), (t, k, b)
    if lam >= 1e4:
        # a live hypothesis never takes a token that an earlier group's live hypothesis took at the same step
        for t in range(len(r["trace"])):
            tok, live = _live_tokens(r, t)
            for b in range(B):
                for k in range(w, bw):
                    earlier = {int(tok[j, b]) for j in range((k // w) * w) if live[j, b]}
                    assert not live[k, b] or int(tok[k, b]) not in earlier, (t, b, k)
    if name == "search_stop":                    # the "penalty too small" side: it never binds, the groups return one caption
        assert all(d[0] == 1 for d in DR.nbest_diversity(lists))


@pytest.mark.parametrize("run", [r for r in DR.RUNS if r["steps"] < r["cml"] + 1], ids=DR.run_id)
def test_fixed_point_after_the_stop(run):
    """Once every hypothesis is finished a further selection orders each group by cum descending, ties by slot; a second one
    changes nothing."""
    r = _diverse(*_run_args(run))
    w = run["bw"] // run["G"]
    cum2, perm, perm3 = r["after_stop"]
    B = cum2.shape[1]
    assert np.array_equal(perm3, np.tile(np.arange(run["bw"]), (B, 1)))
    last = r["trace"][-1][2]
    for b in range(B):
        for g in range(run["G"]):
            s = slice(g * w, g * w + w)
            assert (np.diff(cum2[s, b]) <= 0).all() and sorted(perm[b, s]) == list(range(g * w, g * w + w))
            assert np.array_equal(cum2[s, b], last[perm[b, s], b])


def test_a_group_is_not_in_cum_order():
    """Within a group the slots are ordered by the penalised value: some run's trace holds a group whose cum ascends somewhere."""
    found = 0
    for run in DR.RUNS:
        w = run["bw"] // run["G"]
        if w < 2:
            continue
        for tok, fin, cum, hist in _diverse(*_run_args(run))["trace"]:
            for g in range(1, run["G"]):
                found += int((np.diff(cum[g * w:g * w + w], axis=0) > 0).any())
    assert found > 0


# ---------------------------------------------------------------------------------- the kernel-alone cases
@pytest.mark.parametrize("V,bw,G", [(8, 2, 2), (8, 8, 4), (61, 6, 3), (257, 8, 2), (700, 8, 8), (700, 4, 2)])
def test_constructed_cases(V, bw, G):
    w = bw // G
    labels = set()
    for nb in (1, bw):
        for c in DR.group_cases(V, bw, G, nb):
            labels.add(c["label"])
            args = (c["x"], c["cum"], c["fin"], bw, G)
            kw = dict(hist=c["hist"], t=c["t"], n=c["n"], m=c["m"], banned=c["banned"])
            vals, idx, margin, aug = DR.select_rows_groups(*args, c["lam"], **kw)
            src, tok = idx // V, idx % V
            rows = idx.shape[0]
            # the value is the un-penalised candidate; slots of a group are distinct and in penalised order
            pure = c["cum"].astype(np.float64)[:, :, None] + BR.log_softmax64(c["x"])
            for r in range(rows):
                for k in range(bw):
                    i = src[r, k]
                    assert i == 0 if nb == 1 else i // w == k // w
                    if c["fin"][i, r]:
                        assert vals[r, k] == (np.float64(c["cum"][i, r]) if tok[r, k] == BR.PAD else -np.inf)
                    else:
                        assert vals[r, k] == pure[i, r, tok[r, k]] and aug[r, k] <= vals[r, k]
                        if c["hist"] is not None:
                            assert tok[r, k] not in CR.banned_ids(c["hist"][i, r], c["t"], c["n"], c["m"], c["banned"])
                for g in range(G):
                    s = slice(g * w, g * w + w)
                    assert len(set(idx[r, s])) == w and not (aug[r, s][1:] > aug[r, s][:-1]).any()
            # group 0 is the plain selection at width w on its own hypotheses
            pv, pi, _ = CR.select_rows(c["x"][:1 if nb == 1 else w], c["cum"][:1 if nb == 1 else w], c["fin"][:1 if nb == 1 else w], w,
                                       None if c["hist"] is None else c["hist"][:1 if nb == 1 else w], c["t"], c["n"], c["m"], c["banned"])
            assert np.array_equal(vals[:, :w], pv) and np.array_equal(idx[:, :w], pi)
            lab = c["label"]
            if lab == "peak_low":
                assert (tok[:, ::w] == c["peak"]).all()
            elif lab == "peak_high":
                assert (tok[:, :w] == c["peak"]).any(axis=1).all() and (tok[:, w:] != c["peak"]).all()
            elif lab == "all_finished_ascending":
                for g in range(G if nb == bw else 0):
                    s = slice(g * w, g * w + w)
                    assert (np.diff(vals[:, s], axis=1) <= 0).all() and (tok[:, s] == BR.PAD).all()
                    if g == 0 and w > 2:         # ascending input with slots 0 and 1 tied: the largest first, the tie by slot
                        assert (src[:, 0] == w - 1).all() and (src[:, w - 2] == 0).all() and (src[:, w - 1] == 1).all()
            elif lab == "count_two":
                assert (tok[:, :2] == c["peak"]).all() and (tok[:, 2:w] != c["peak"]).all() and (tok[:, w] != c["peak"]).all()
                kept = DR.select_rows_groups(*args, 0.7 * c["lam"], **kw)[1] % V      # (2 x 0.7 lambda < the lead of 1.5 lambda < 2 lambda)
                assert (kept[:, w] == c["peak"]).all()
            elif lab == "finished_pad":
                assert (tok[0::2, w] == BR.PAD).all() and (tok[1::2, w::w] != BR.PAD).all() and (tok[:, 0] == BR.PAD).all()
                assert (tok[0::2, 2 * w::w] != BR.PAD).all()                      # (group 1's live <PAD> is counted for the groups behind it)
            elif lab == "chosen_and_banned":
                assert (tok[:, 0] == c["peak"]).all() and (tok[:, w:] != c["peak"]).all()
            elif lab == "residue":
                if G >= 4 and w == 1:
                    assert (tok[:, 0] == 7).all() and (tok[:, 1] == 263).all() and (tok[:, 2] == 519).all() and not np.isin(tok[:, 3], c["residue"]).any()
    assert {"continuous", "quantised", "peak_low", "peak_high", "all_finished_ascending"} <= labels
    if G >= 2 and bw // G >= 2:
        assert "count_two" in labels
    if V >= 600:
        assert "residue" in labels


def test_nbest_diversity():
    from recnet_amd import search
    hyps = [[([3, 4, 2], -1.0, 3, -1.0), ([3, 4, 2], -2.0, 3, -2.0), ([3, 5, 2], -3.0, 3, -3.0)],
            [([7], -1.0, 1, -1.0), ([7], -1.0, 1, -1.0)],
            [([], 0.0, 0, 0.0)],
            [[3, 4, 5, 6], [6, 5, 4, 3]]]
    got = search.nbest_diversity(hyps)
    assert got[0] == (2, 4 / 9, 4 / 6)           # unigrams 3 4 2 5 of 9; bigrams (3,4) (4,2) (3,5) (5,2) of 6
    assert got[1] == (1, 1 / 2, 0.0)
    assert got[2] == (1, 0.0, 0.0)
    assert got[3] == (2, 4 / 8, 6 / 6)
    assert got == DR.nbest_diversity([[h[0] if isinstance(h, tuple) else h for h in hb] for hb in hyps])
    # with the group as a fifth field, and on a restatement's result
    assert search.nbest_diversity([[([3, 2], -1.0, 2, -1.0, 0), ([4, 2], -1.0, 2, -1.0, 1)]]) == [(2, 3 / 4, 1.0)]


def test_library_exports_and_argument_checks():
    """The C ABI refuses a NULL handle first, for both new symbols (no GPU needed)."""
    from recnet_amd import _lib, _ops
    lib = _lib.load()
    assert "recnet_beam_select_rows_diverse" in _lib.EXPORTS and "recnet_beam_search_nbest_diverse" in _lib.EXPORTS
    assert "beam_select_rows_diverse" in _ops.OP_NAMES and "beam_search_nbest_diverse" in _ops.OP_NAMES
    assert lib.recnet_beam_select_rows_diverse(None, None, None, None, None, 1, 1, 61, 8, 0, 4, 2, 0.5, 0, 0, None, 0, None, None, None) == -2
    assert lib.recnet_beam_search_nbest_diverse(None, None, 4, 0.7, 2, 0.5, 0, 0, None, 0, None, None, None, None, None, None, None) == -2
    assert _lib.ABI_VERSION == 12


_BAD = [dict(n_groups=0), dict(n_groups=-1), dict(n_groups=3), dict(n_groups=8), dict(n_groups=1.5), dict(n_groups="2"), dict(n_groups=None),
        dict(n_groups=2, diversity_penalty=-0.5), dict(n_groups=2, diversity_penalty=float("nan")), dict(n_groups=2, diversity_penalty=float("inf")),
        dict(diversity_penalty=-1.0), dict(diversity_penalty="1"), dict(beam_width=0, n_groups=2), dict(beam_width=6, n_groups=4)]


@pytest.mark.parametrize("kw", _BAD, ids=[str(i) for i in range(len(_BAD))])
def test_python_search_checks_its_arguments_before_the_library(kw, monkeypatch):
    import torch
    import recnet_amd as R
    from recnet_amd import search

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(search, "_nbest_engine", boom)

    class Dec:
        output_size = 61

    class Cfg:
        caption_max_len = 7
    kw = dict(dict(beam_width=4), **kw)
    inp = torch.full((1, 4), 1, dtype=torch.long)
    with pytest.raises(ValueError):
        R.beam_search_nbest(Cfg(), Dec(), inp, torch.zeros(1, 4, 8), torch.zeros(4, 5, 32), **kw)
    with pytest.raises(ValueError):
        R.best_of_beam(Cfg(), Dec(), inp, torch.zeros(1, 4, 8), torch.zeros(4, 5, 32), **kw)


def test_python_search_names_the_rule_and_accepts_good_arguments(monkeypatch):
    import torch
    import recnet_amd as R
    from recnet_amd import search
    reached = []

    def engine(*a, **k):
        reached.append(1)
        raise KeyError("engine")
    monkeypatch.setattr(search, "_nbest_engine", engine)

    class Dec:
        output_size = 61

    class Cfg:
        caption_max_len = 7
    args = (Cfg(), Dec(), torch.full((1, 4), 1, dtype=torch.long), torch.zeros(1, 4, 8), torch.zeros(4, 5, 32))
    with pytest.raises(ValueError, match="n_groups must be an integer >= 1 that divides beam_width"):
        R.beam_search_nbest(*args, 6, n_groups=4)
    with pytest.raises(ValueError, match="diversity_penalty must be a finite number >= 0"):
        R.beam_search_nbest(*args, 6, n_groups=3, diversity_penalty=-1.0)
    assert reached == []
    for kw in (dict(n_groups=3, diversity_penalty=0.5), dict(n_groups=6), dict(n_groups=1, diversity_penalty=3.0),
               dict(n_groups=np.int64(2), diversity_penalty=np.float32(1.0), return_groups=True)):
        with pytest.raises(KeyError):
            R.beam_search_nbest(*args, 6, **kw)
    assert reached == [1] * 4


def test_evaluate_takes_the_new_keys(monkeypatch):
    import torch
    import recnet_amd as R
    from recnet_amd import loop
    calls = []

    def nbest(config, decoder, inp, hid, enc, width, length_alpha, **kw):
        calls.append(("nbest", width, length_alpha, kw))
        return [[([3, 2], -1.0, 2, -1.0)] for _ in range(enc.shape[0])]

    def bob(config, decoder, inp, hid, enc, width, length_alpha, reconstructor, recon_weight, **kw):
        calls.append(("bob", width, length_alpha, recon_weight, kw))
        return [[3, 2] for _ in range(enc.shape[0])], None, None
    monkeypatch.setattr(loop, "beam_search_nbest", nbest)
    monkeypatch.setattr(loop, "best_of_beam", bob)
    monkeypatch.setattr(loop.metrics, "score_all", lambda gts, res: dict(res))

    class Cfg:
        batch_size, decoder_model, caption_max_len = 2, "GRU", 7
    dec = torch.nn.Linear(2, 2)
    dec.hidden_size = 4
    rec = torch.nn.Linear(2, 2)
    feats = np.zeros((2, 3, 4), dtype=np.float32)
    batches = [(["a", "b"], feats), (["c", "PAD"], feats)]
    ev = lambda method, **kw: R.evaluate(Cfg, batches, dec, method, {3: "x", 2: "<EOS>"}, {v: ["x"] for v in "abc"}, **kw)
    div = dict(n_groups=2, diversity_penalty=0.5)
    both = dict(div, no_repeat_ngram=2)
    ev(("beam_nbest", 4, 0.7, div))
    ev(("beam_recon", 4, 0.5, 2.0, both), reconstructor=rec)
    ev(("beam_nbest", 4, 0.7, dict(n_groups=4)))
    want = [("nbest", 4, 0.7, div), ("bob", 4, 0.5, 2.0, both), ("nbest", 4, 0.7, dict(n_groups=4))]
    assert calls == [c for c in want for _ in batches]
    with pytest.raises(ValueError, match="unknown constraint"):
        ev(("beam_nbest", 4, 0.7, dict(groups=2)))
