"""loop.evaluate's method grammar without a GPU: for each of the nine forms, with and without its optional tail, the exact
positional and keyword arguments that reach the runner, batch by batch (the method is parsed again for every batch), and for
each malformed form the exception type and its whole message.  Every runner name in `loop` and metrics.score_all are recorders."""
import numpy as np
import pytest
import torch

B, H = 2, 4
CAPS = [[3, 2] for _ in range(B)]                     # what every recorder decodes: the word "x", then <EOS>
STEPS = [[3] * B, [2] * B]
RETURNS = dict(greedy_search=STEPS, beam_search=CAPS, sample_search=(STEPS, None), best_of_n=(CAPS, None, None),
               best_of_beam=(CAPS, None, None), beam_search_nbest=[[([3, 2], -1.0, 2, -1.0)] for _ in range(B)])


class Cfg:
    batch_size, decoder_model, caption_max_len = B, "LSTM", 7


class GruCfg(Cfg):
    decoder_model = "GRU"


class _Model(torch.nn.Linear):
    def __init__(self):
        super().__init__(2, 2)
        self.hidden_size = H
        self.evals = 0

    def eval(self):
        self.evals += 1
        return super().eval()


def _seen(x, names):
    """An argument as the tests compare it: the objects evaluate was given by name, a tensor by dtype, shape and its one value."""
    for name, obj in names.items():
        if x is obj:
            return name
    if isinstance(x, torch.Tensor):
        assert bool((x == x.flatten()[0]).all())
        return (str(x.dtype).split(".")[1], tuple(x.shape), float(x.flatten()[0]))
    if isinstance(x, tuple):
        return tuple(_seen(y, names) for y in x)
    return x


INP = ("int64", (1, B), 1.0)
ZERO = ("float32", (1, B, H), 0.0)
ENC = ("float32", (B, 3, 4), 0.5)
LSTM = ("config", "decoder", INP, (ZERO, ZERO), ENC)       # the five leading arguments of every runner but beam_search


@pytest.fixture
def ev(monkeypatch):
    """ev(method, ...) runs evaluate over two batches; ev.calls is what reached the runners, ev.dec / ev.rec the two models."""
    import recnet_amd as R
    from recnet_amd import loop
    dec, rec = _Model(), _Model()
    calls = []
    names = dict(decoder=dec, reconstructor=rec)

    def recorder(name):
        def run(*args, **kw):
            calls.append((name, tuple(_seen(a, names) for a in args), {k: _seen(v, names) for k, v in kw.items()}))
            return RETURNS[name]
        return run
    for name in RETURNS:
        monkeypatch.setattr(loop, name, recorder(name))
    monkeypatch.setattr(loop.metrics, "score_all", lambda gts, res: ("scored", gts, res))
    feats = np.full((B, 3, 4), 0.5, dtype=np.float32)
    batches = [(["a", "b"], feats), (["c", "PAD"], feats)]

    def run(method, reconstructor=None, config=Cfg):
        names["config"] = config
        kw = {} if reconstructor is None else dict(reconstructor=rec)
        return R.evaluate(config, batches, dec, method, {3: "x", 2: "<EOS>"}, {v: [v + " ref"] for v in "abc"}, **kw)
    run.calls, run.dec, run.rec, run.n_batches = calls, dec, rec, len(batches)
    return run


CON = dict(no_repeat_ngram=2, min_length=3, banned_tokens=(5, 6), n_groups=2, diversity_penalty=1.5)

# (the method, whether evaluate is given the reconstructor, the runner, its positional arguments, its keyword arguments)
FORMS = [
    ("greedy", False, "greedy_search", LSTM, {}),
    (("beam", 5), False, "beam_search", ("config", 5, None, "decoder", INP, (ZERO, ZERO), ENC), {}),
    (("beam", 5, "ignored", 7), False, "beam_search", ("config", 5, None, "decoder", INP, (ZERO, ZERO), ENC), {}),   # no arity check
    (("sample", 0.9, 5, 7), False, "sample_search", LSTM + (0.9, 5, 7, 1.0), {}),
    (("sample", 0.9, 5, 7, 0.8), False, "sample_search", LSTM + (0.9, 5, 7, 0.8), {}),
    (("best_of", 4, 0.9, 5, 7), False, "best_of_n", LSTM + (4, 0.9, 5, 7), dict(top_p=1.0)),
    (("best_of", 4, 0.9, 5, 7, 0.8), False, "best_of_n", LSTM + (4, 0.9, 5, 7), dict(top_p=0.8)),
    (("best_of_recon", 4, 0.9, 5, 7, 2.0), True, "best_of_n", LSTM + (4, 0.9, 5, 7, "reconstructor", 2.0, 1.0), {}),
    (("best_of_recon", 4, 0.9, 5, 7, 2.0, 0.8), True, "best_of_n", LSTM + (4, 0.9, 5, 7, "reconstructor", 2.0, 0.8), {}),
    (("best_of_consensus", 4, 0.9, 5, 7, 0.5), False, "best_of_n", LSTM + (4, 0.9, 5, 7), dict(top_p=1.0, consensus_weight=0.5)),
    (("best_of_consensus", 4, 0.9, 5, 7, 0.5, 0.8), False, "best_of_n", LSTM + (4, 0.9, 5, 7), dict(top_p=0.8, consensus_weight=0.5)),
    (("beam_consensus", 8, 0.7, 0.25), False, "best_of_beam", LSTM + (8, 0.7), dict(consensus_weight=0.25)),
    (("beam_consensus", 8, 0.7, 0.25, CON), False, "best_of_beam", LSTM + (8, 0.7), dict(consensus_weight=0.25, **CON)),
    (("beam_nbest", 3, 0.7), False, "beam_search_nbest", LSTM + (3, 0.7), {}),
    (("beam_nbest", 3, 0.7, CON), False, "beam_search_nbest", LSTM + (3, 0.7), dict(CON)),
    (("beam_nbest", 3, 0.7, {}), False, "beam_search_nbest", LSTM + (3, 0.7), {}),
    (("beam_recon", 4, 0.5, 2.0), True, "best_of_beam", LSTM + (4, 0.5, "reconstructor", 2.0), {}),
    (("beam_recon", 4, 0.5, 2.0, CON), True, "best_of_beam", LSTM + (4, 0.5, "reconstructor", 2.0), dict(CON)),
    # a reconstructor that the method does not use is left alone
    (("beam_nbest", 3, 0.7), True, "beam_search_nbest", LSTM + (3, 0.7), {}),
    (("best_of", 4, 0.9, 5, 7), True, "best_of_n", LSTM + (4, 0.9, 5, 7), dict(top_p=1.0)),
]


@pytest.mark.parametrize("as_list", [False, True], ids=["tuple", "list"])
@pytest.mark.parametrize("method, with_rec, runner, args, kwargs", FORMS, ids=[repr(f[0]) + ("+rec" if f[1] else "") for f in FORMS])
def test_what_reaches_the_runner(ev, method, with_rec, runner, args, kwargs, as_list):
    if as_list and not isinstance(method, str):
        method = list(method)                                   # (a list is a method as well)
    out = ev(method, reconstructor=with_rec or None)
    assert ev.calls == [(runner, args, kwargs)] * ev.n_batches
    # the first caption of every video, "PAD" dropped; the references of exactly those videos
    assert out == ("scored", {v: [v + " ref"] for v in "abc"}, {v: ["x"] for v in "abc"})
    uses_rec = not isinstance(method, str) and method[0] in ("best_of_recon", "beam_recon")
    assert ev.dec.evals == 1 and ev.rec.evals == (ev.n_batches if uses_rec else 0)
    assert CON == dict(no_repeat_ngram=2, min_length=3, banned_tokens=(5, 6), n_groups=2, diversity_penalty=1.5)   # the caller's dict stays


def test_the_constraints_reach_the_runner_as_a_copy(ev, monkeypatch):
    """The runner gets a dict of its own for every batch: what it does to it does not reach the next batch or the caller."""
    from recnet_amd import loop
    seen = []
    inner = loop.best_of_beam

    def bob(*args, **kw):
        seen.append(dict(kw))
        kw.clear()
        return inner(*args)
    monkeypatch.setattr(loop, "best_of_beam", bob)
    con = dict(min_length=1)
    ev(("beam_consensus", 8, 0.7, 0.25, con))
    assert seen == [dict(consensus_weight=0.25, min_length=1)] * ev.n_batches and con == dict(min_length=1)


def test_a_gru_starts_from_one_state(ev):
    ev("greedy", config=GruCfg)
    ev(("sample", 0.9, 5, 7), config=GruCfg)
    gru = ("config", "decoder", INP, ZERO, ENC)
    assert ev.calls == [("greedy_search", gru, {})] * 2 + [("sample_search", gru + (0.9, 5, 7, 1.0), {})] * 2


def _top_p(name, n, got):
    return "the %r method takes %d fields and an optional top_p (got %r)" % (name, n, got)


def _constraints(name, n, got):
    return "the %r method takes %d fields and an optional dict of constraints (got %r)" % (name, n, got)


UNKNOWN_KEY = "unknown constraint %s: the keys are no_repeat_ngram, min_length, banned_tokens, n_groups, diversity_penalty"

# (the method, whether evaluate is given the reconstructor, the exception, its whole message)
MALFORMED = [
    # wrong arity: one field short, two fields long
    (("sample", 0.9, 5), False, ValueError, _top_p("sample", 4, ("sample", 0.9, 5))),
    (("sample", 0.9, 5, 7, 0.8, 1), False, ValueError, _top_p("sample", 4, ("sample", 0.9, 5, 7, 0.8, 1))),
    (["sample", 0.9, 5], False, ValueError, _top_p("sample", 4, ["sample", 0.9, 5])),                     # (a list is shown as given)
    (("best_of", 4, 0.9, 5), False, ValueError, _top_p("best_of", 5, ("best_of", 4, 0.9, 5))),
    (("best_of", 4, 0.9, 5, 7, 0.8, 1), False, ValueError, _top_p("best_of", 5, ("best_of", 4, 0.9, 5, 7, 0.8, 1))),
    (("best_of_recon", 4, 0.9, 5, 7), True, ValueError, _top_p("best_of_recon", 6, ("best_of_recon", 4, 0.9, 5, 7))),
    (("best_of_recon", 4, 0.9, 5, 7, 2.0, 0.8, 1), True, ValueError, _top_p("best_of_recon", 6, ("best_of_recon", 4, 0.9, 5, 7, 2.0, 0.8, 1))),
    (("best_of_consensus", 4, 0.9, 5, 7), False, ValueError, _top_p("best_of_consensus", 6, ("best_of_consensus", 4, 0.9, 5, 7))),
    (("best_of_consensus", 4, 0.9, 5, 7, 0.5, 0.8, 1), False, ValueError,
     _top_p("best_of_consensus", 6, ("best_of_consensus", 4, 0.9, 5, 7, 0.5, 0.8, 1))),
    (("beam_consensus", 8, 0.7), False, ValueError, _constraints("beam_consensus", 4, ("beam_consensus", 8, 0.7))),
    (("beam_consensus", 8, 0.7, 0.25, {}, {}), False, ValueError, _constraints("beam_consensus", 4, ("beam_consensus", 8, 0.7, 0.25, {}, {}))),
    (("beam_nbest", 3), False, ValueError, _constraints("beam_nbest", 3, ("beam_nbest", 3))),
    (("beam_nbest", 3, 0.7, {}, {}), False, ValueError, _constraints("beam_nbest", 3, ("beam_nbest", 3, 0.7, {}, {}))),
    (["beam_nbest", 3], False, ValueError, _constraints("beam_nbest", 3, ("beam_nbest", 3))),            # (a list is shown as a tuple)
    (("beam_recon", 4, 0.5), True, ValueError, _constraints("beam_recon", 4, ("beam_recon", 4, 0.5))),
    (("beam_recon", 4, 0.5, 2.0, {}, {}), True, ValueError, _constraints("beam_recon", 4, ("beam_recon", 4, 0.5, 2.0, {}, {}))),
    # a tail that is no dict
    (("beam_consensus", 8, 0.7, 0.25, 2), False, ValueError, _constraints("beam_consensus", 4, ("beam_consensus", 8, 0.7, 0.25, 2))),
    (("beam_nbest", 3, 0.7, 2), False, ValueError, _constraints("beam_nbest", 3, ("beam_nbest", 3, 0.7, 2))),
    (("beam_nbest", 3, 0.7, [("min_length", 1)]), False, ValueError, _constraints("beam_nbest", 3, ("beam_nbest", 3, 0.7, [("min_length", 1)]))),
    (("beam_recon", 4, 0.5, 2.0, None), True, ValueError, _constraints("beam_recon", 4, ("beam_recon", 4, 0.5, 2.0, None))),
    # an unknown constraint key (all of them, sorted)
    (("beam_nbest", 3, 0.7, dict(min_len=1)), False, ValueError, UNKNOWN_KEY % "'min_len'"),
    (("beam_consensus", 8, 0.7, 0.25, dict(groups=2, min_length=1, banned=())), False, ValueError, UNKNOWN_KEY % "'banned', 'groups'"),
    (("beam_recon", 4, 0.5, 2.0, dict(top_p=0.5)), True, ValueError, UNKNOWN_KEY % "'top_p'"),
    # a recon method without a reconstructor — and the split's error comes first
    (("best_of_recon", 4, 0.9, 5, 7, 2.0), False, ValueError, 'the "best_of_recon" method needs a reconstructor'),
    (("best_of_recon", 4, 0.9, 5, 7, 2.0, 0.8), False, ValueError, 'the "best_of_recon" method needs a reconstructor'),
    (("beam_recon", 4, 0.5, 2.0), False, ValueError, 'the "beam_recon" method needs a reconstructor'),
    (("beam_recon", 4, 0.5, 2.0, CON), False, ValueError, 'the "beam_recon" method needs a reconstructor'),
    (("best_of_recon", 4, 0.9, 5, 7), False, ValueError, _top_p("best_of_recon", 6, ("best_of_recon", 4, 0.9, 5, 7))),
    (("beam_recon", 4, 0.5), False, ValueError, _constraints("beam_recon", 4, ("beam_recon", 4, 0.5))),
    (("beam_recon", 4, 0.5, 2.0, dict(top_p=0.5)), False, ValueError, UNKNOWN_KEY % "'top_p'"),
    # an unknown name, whatever follows it; a string other than "greedy"
    (("beam_best", 3, 0.7), False, NotImplementedError, "Unknown search method: beam_best"),
    (("Beam", 3), True, NotImplementedError, "Unknown search method: Beam"),
    (("greedy",), False, NotImplementedError, "Unknown search method: greedy"),
    ("beam", False, NotImplementedError, "Unknown search method: beam"),
    ("Greedy", False, NotImplementedError, "Unknown search method: Greedy"),
    ("", False, NotImplementedError, "Unknown search method: "),
]


@pytest.mark.parametrize("method, with_rec, exc, message", MALFORMED, ids=[repr(m[0]) + ("+rec" if m[1] else "") for m in MALFORMED])
def test_what_a_malformed_method_raises(ev, method, with_rec, exc, message):
    with pytest.raises(exc) as e:
        ev(method, reconstructor=with_rec or None)
    assert type(e.value) is exc and str(e.value) == message
    assert ev.calls == [] and ev.rec.evals == 0


def test_beam_without_a_width_is_an_index_error(ev):
    """("beam", width) is read by position, with no arity check of its own: fields behind the width are ignored (above), and the
    bare name fails where the width is read."""
    with pytest.raises(IndexError):
        ev(("beam",))
    assert ev.calls == []
