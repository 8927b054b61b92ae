"""The CPU restatement of the constrained N-best beam search (tests/beam_constrained_ref.py) pinned to what the suite already holds:
with the constraints off it is tests/beam_ref.py's search; with them on no returned hypothesis violates them while the
unconstrained search's do (no run passes vacuously), cum stays score_ref's log-probability of the hypothesis' own tokens, and each
run keeps the share of compared decisions the issue lists.  Then the ban rule against a brute-force statement, the argument checks
of the Python layer and of the C ABI, and evaluate()'s tuple parsing."""
import functools
import itertools

import numpy as np
import pytest

from tests import beam_constrained_ref as CR
from tests import beam_ref as BR
from tests import score_ref as SC
from tests.golden_util import load_search_case


@functools.lru_cache(maxsize=None)
def _unconstrained(name, bw, cml):
    g, P, enc = load_search_case(name)
    return BR.beam_search_nbest(P, enc, bw, BR.LENGTH_ALPHA, cml, g["_cell"])


@functools.lru_cache(maxsize=None)
def _constrained(name, bw, cml, n, m, banned):
    g, P, enc = load_search_case(name)
    return CR.beam_search_nbest(P, enc, bw, BR.LENGTH_ALPHA, cml, g["_cell"], n, m, banned)


@pytest.mark.parametrize("name,bw,cml,cap", BR.SEARCH_RUNS)
def test_constraints_off_is_the_unconstrained_restatement(name, bw, cml, cap):
    a, b = _unconstrained(name, bw, cml), _constrained(name, bw, cml, 0, 0, ())
    for k in ("tokens", "cum", "len", "score", "margins", "final_margin", "amax"):
        assert np.array_equal(a[k], b[k]), k
    assert a["n_steps"] == b["n_steps"] and len(a["trace"]) == len(b["trace"])
    for ta, tb in zip(a["trace"], b["trace"]):
        assert all(np.array_equal(x, y) for x, y in zip(ta, tb))


@pytest.mark.parametrize("run", CR.RUNS, ids=CR.run_id)
def test_runs_hold_their_table(run):
    name, bw, cml, n, m, banned = run["name"], run["bw"], run["cml"], run["n"], run["m"], run["banned"]
    g, P, enc = load_search_case(name)
    B = enc.shape[0]
    u = _unconstrained(name, bw, cml)
    r = _constrained(name, bw, cml, n, m, banned)
    if banned:                                   # the hard-coded ids are what the rule gives on the unconstrained result
        assert CR.frequent_ids(u["tokens"], u["len"], len(banned)) == banned
    assert bw + len(banned) + cml + 1 <= int(g["meta_dims"][3])
    # the constraints bind on the unconstrained result, in every constraint the run switches on, and hold on the constrained one
    uv = CR.violations(u["tokens"], u["len"], n, m, banned)
    share = CR.compared_share(r)
    keep = CR.comparable_captions(r)
    print(CR.run_id(run), "steps", u["n_steps"], "->", r["n_steps"], "unconstrained violations", uv, "of", bw * B, "share %.3f" % share,
          "captions compared in full", int(keep.sum()), "of", B)
    assert uv == run["unc"] and bw * B == run["total"]
    # a constraint that is off counts nothing; one that is on binds, except where the run's `slack` names it (beam_constrained_ref.RUNS)
    on = (n > 0, m > 0, bool(banned))
    for k in range(3):
        assert (uv[k] > 0) == (on[k] and k not in run.get("slack", ())), (k, uv, on)
    assert any(uv[k] > 0 for k in range(3) if on[k])
    assert CR.violations(r["tokens"], r["len"], n, m, banned) == (0, 0, 0)
    assert (u["n_steps"], r["n_steps"]) == run["steps"]
    assert share >= run["cap"] and abs(share - run["share"]) < 1e-3
    assert (int(keep.sum()), B) == run["full"]
    assert keep.any() or CR.comparable_steps(r["margins"]).sum(axis=0)[~keep].max() > 0
    # cum is still the model's log-probability of the hypothesis' own tokens (no renormalisation), len the scorer's length
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
    for t, (tok, fin, cum, hist) in enumerate(r["trace"]):
        assert (np.diff(cum, axis=0) <= 0).all() and np.isfinite(cum).all()
        # the rule held at the step itself, hypothesis by hypothesis
        for k, b in zip(*np.nonzero((fin == 0) | (fin == t + 1))):
            assert int(tok[k, b]) not in CR.banned_ids(hist[k, b], t, n, m, banned), (t, k, b)


def test_width_one_guard_leaves_decisions_to_compare():
    """The device test compares a width-1 search with the restatement up to the first decision the precision could flip
    (width1_steps).  That must not be vacuous: in fp32 every run keeps decisions, and in bf16, where the guard is twice a row bar of
    8e-2 x max |logit|, the runs together keep at least a tenth of theirs and more than one run keeps some."""
    total, kept, runs_with = 0, {"f32": 0, "bf16": 0}, {"f32": 0, "bf16": 0}
    for run in CR.RUNS:
        r1 = _constrained(run["name"], 1, run["cml"], run["n"], run["m"], run["banned"])
        total += r1["margins"].size
        for prec in kept:
            k = int(CR.width1_steps(r1, prec).sum())
            kept[prec] += k
            runs_with[prec] += k > 0
    print("width-1 decisions", total, "kept", kept, "runs with some", runs_with)
    assert runs_with["f32"] == len(CR.RUNS) and kept["f32"] >= 0.75 * total
    assert kept["bf16"] >= 0.1 * total and runs_with["bf16"] > 1


def _brute_banned(w, n):
    """The tokens v such that w + [v] holds an n-gram twice, given that w holds none twice... stated without that premise: v is banned
    iff the n-gram that v would complete already occurs in w."""
    t = len(w)
    if t < n - 1:
        return set()
    grams = {tuple(w[j:j + n]) for j in range(t - n + 1)}
    return {v for v in range(4) if tuple(w[t - n + 1:] + [v]) in grams}


def test_ban_rule_against_the_set_of_ngrams():
    rng = np.random.RandomState(5)
    for n in (1, 2, 3, 4):
        for t in range(0, 9):
            hists = [list(h) for h in itertools.product(range(4), repeat=t)] if t <= 4 else [list(rng.randint(0, 4, size=t)) for _ in range(200)]
            for w in hists:
                pad = w + [int(x) for x in rng.randint(0, 4, size=3)]     # entries behind t are not read
                assert CR.banned_ids(pad, t, n, 0, ()) == _brute_banned(w, n), (n, t, w)
    assert CR.banned_ids([3, 4, 3], 3, 2, 5, (7, 9)) == {4, 7, 9, BR.EOS}
    assert CR.banned_ids([3, 4, 3], 3, 2, 3, (7,)) == {4, 7}
    assert CR.banned_ids([0, 0], 2, 1, 0, ()) == {BR.PAD}                 # <PAD> from a live hypothesis is a token like any other


@pytest.mark.parametrize("V,nb", [(61, 1), (61, 3), (257, 8), (700, 3)])
def test_select_rows_rules(V, nb):
    """No banned id is selected from a live hypothesis, a finished one still offers <PAD> at cum, -inf is never selected, and the
    values of what is selected are the unconstrained candidates' (no renormalisation)."""
    cases = CR.row_cases(V, nb) + CR.min_length_cases(V, nb) + CR.residue_cases(V, nb) + [CR.static_ban_case(V, nb)]
    decided = twin_wins = 0
    for c in cases:
        free_v, free_i, _ = BR.select_rows(c["x"], c["cum"], c["fin"], 8)
        allc = c["cum"].astype(np.float64)[:, :, None] + BR.log_softmax64(c["x"])
        for bw in CR.ROW_BW:
            assert bw + len(c["banned"]) + c["t"] + 1 <= V
            vals, idx, margin = CR.select_rows(c["x"], c["cum"], c["fin"], bw, c["hist"], c["t"], c["n"], c["m"], c["banned"])
            assert np.isfinite(vals[(c["fin"] == 0).any(axis=0)]).all() and (vals[:, 1:] <= vals[:, :-1]).all()
            src, tok = idx // V, idx % V
            for r in range(idx.shape[0]):
                assert len(set(idx[r])) == bw
                for k in range(bw):
                    i = src[r, k]
                    if np.isneginf(vals[r, k]):          # (the candidates ran out: every hypothesis of the row is finished)
                        continue
                    if c["fin"][i, r]:
                        assert tok[r, k] == BR.PAD and vals[r, k] == np.float64(c["cum"][i, r])
                    else:
                        assert tok[r, k] not in CR.banned_ids(c["hist"][i, r], c["t"], c["n"], c["m"], c["banned"]), c["case"]
                        assert vals[r, k] == allc[i, r, tok[r, k]]
            decided += int((idx != free_i[:, :bw]).any())
        if c["tie"]:                             # the twin offers what hypothesis 0's history bans, at the same value
            vals, idx, _ = CR.select_rows(c["x"], c["cum"], c["fin"], 8, c["hist"], c["t"], c["n"], c["m"], c["banned"])
            b0 = CR.banned_ids(c["hist"][0, 0], c["t"], c["n"], c["m"], c["banned"])
            b1 = CR.banned_ids(c["hist"][nb - 1, 0], c["t"], c["n"], c["m"], c["banned"])
            got = {(int(i) // V, int(i) % V) for i in idx[0]}
            for v in b0 - b1:
                assert (0, v) not in got and (nb - 1, v) in got, c["case"]
                twin_wins += 1
    assert decided > len(cases)                  # the bans decide outcomes: the raised logits would otherwise win
    assert nb == 1 or twin_wins > 0


def test_library_exports_and_argument_checks():
    """The C ABI refuses a NULL handle first, for both new symbols (no GPU needed)."""
    from recnet_amd import _lib, _ops
    lib = _lib.load()
    assert "recnet_beam_select_rows_constrained" in _lib.EXPORTS and "recnet_beam_search_nbest_constrained" in _lib.EXPORTS
    assert "beam_select_rows_constrained" in _ops.OP_NAMES and "beam_search_nbest_constrained" in _ops.OP_NAMES
    assert lib.recnet_beam_select_rows_constrained(None, None, None, None, None, 1, 1, 61, 8, 0, 1, 2, 0, None, 0, None, None, None) == -2
    assert lib.recnet_beam_search_nbest_constrained(None, None, 3, 0.7, 2, 0, None, 0, None, None, None, None, None, None) == -2


_BAD = [dict(no_repeat_ngram=-1), dict(no_repeat_ngram=8), dict(no_repeat_ngram=1.5), dict(no_repeat_ngram="2"),
        dict(min_length=-1), dict(min_length=8), dict(min_length=2.5),
        dict(banned_tokens=(5, 5)), dict(banned_tokens=(2,)), dict(banned_tokens=(61,)), dict(banned_tokens=(-1,)), dict(banned_tokens=(3.5,)),
        dict(banned_tokens=tuple(range(3, 20))), dict(banned_tokens=7),
        dict(beam_width=0, no_repeat_ngram=2), dict(length_alpha=-1.0, min_length=2)]


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
    kw = dict(dict(beam_width=3), **kw)
    inp = torch.full((1, 4), 1, dtype=torch.long)
    with pytest.raises(ValueError):
        R.beam_search_nbest(Cfg(), Dec(), inp, torch.zeros(1, 4, 8), torch.zeros(4, 5, 32), **kw)
    with pytest.raises(ValueError):
        R.best_of_beam(Cfg(), Dec(), inp, torch.zeros(1, 4, 8), torch.zeros(4, 5, 32), **kw)


def test_python_search_refuses_an_infeasible_vocabulary(monkeypatch):
    import torch
    import recnet_amd as R
    from recnet_amd import search
    reached = []

    def engine(*a, **k):
        reached.append(1)
        raise KeyError("engine")
    monkeypatch.setattr(search, "_nbest_engine", engine)

    class Dec:
        output_size = 20

    class Cfg:
        caption_max_len = 7
    args = (Cfg(), Dec(), torch.full((1, 4), 1, dtype=torch.long), torch.zeros(1, 4, 8), torch.zeros(4, 5, 32))
    # 8 + 4 + 7 + 1 = 20 <= V: accepted (the engine is asked for); one more ban, or one more beam: refused before it
    with pytest.raises(KeyError):
        R.beam_search_nbest(*args, 8, no_repeat_ngram=2, banned_tokens=(3, 4, 5, 6))
    assert reached == [1]
    with pytest.raises(ValueError, match="too small"):
        R.beam_search_nbest(*args, 8, no_repeat_ngram=2, banned_tokens=(3, 4, 5, 6, 7))
    with pytest.raises(ValueError, match="too small"):
        R.best_of_beam(*args, 8, min_length=1, banned_tokens=(3, 4, 5, 6, 7))
    Dec.output_size = 12
    with pytest.raises(ValueError, match="too small"):
        R.beam_search_nbest(*args, 5, min_length=1)
    with pytest.raises(KeyError):                # the constraint-free check stays beam_width <= min(8, V)
        R.beam_search_nbest(*args, 8)
    assert reached == [1, 1]


def test_evaluate_parses_the_trailing_dict(monkeypatch):
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
    # three batches: the method is parsed for every batch, and every batch is decoded with the constraints
    feats = np.zeros((2, 3, 4), dtype=np.float32)
    batches = [(["a", "b"], feats), (["c", "d"], feats), (["e", "PAD"], feats)]
    ev = lambda method, **kw: R.evaluate(Cfg, batches, dec, method, {3: "x", 2: "<EOS>"}, {v: ["x"] for v in "abcde"}, **kw)
    con = dict(no_repeat_ngram=2, min_length=3, banned_tokens=(5, 6))
    assert set(ev(("beam_nbest", 3, 0.7))) == set("abcde")
    ev(("beam_nbest", 3, 0.7, con))
    ev(("beam_nbest", 3, 0.7, dict(min_length=1)))
    ev(("beam_recon", 4, 0.5, 2.0), reconstructor=rec)
    ev(("beam_recon", 4, 0.5, 2.0, con), reconstructor=rec)
    ev(["beam_nbest", 3, 0.7, con])                                           # (a list is a method as well)
    want = [("nbest", 3, 0.7, {}), ("nbest", 3, 0.7, con), ("nbest", 3, 0.7, dict(min_length=1)), ("bob", 4, 0.5, 2.0, {}),
            ("bob", 4, 0.5, 2.0, con), ("nbest", 3, 0.7, con)]
    assert calls == [c for c in want for _ in batches]
    with pytest.raises(ValueError, match="unknown constraint"):
        ev(("beam_nbest", 3, 0.7, dict(min_len=1)))
    with pytest.raises(ValueError):
        ev(("beam_nbest", 3, 0.7, 2))
    with pytest.raises(ValueError):
        ev(("beam_recon", 4, 0.5, 2.0, con, con), reconstructor=rec)
    with pytest.raises(ValueError, match="needs a reconstructor"):
        ev(("beam_recon", 4, 0.5, 2.0, con))
