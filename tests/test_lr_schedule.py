"""Learning-rate schedules, host side (no GPU): the pure-Python restatement of the formula
(tests/lr_schedule_ref.py) against torch's schedulers and hand-computed points, recnet_lr_at — the inline function the Adam
kernels call — against the restatement, the range checks of recnet_set_lr_schedule on a host-only handle, FusedAdam's state
dicts and engine propagation on a stub engine, and Trainer's reduce-on-plateau logic on stub optimisers."""
import ctypes as C
import math

import pytest
import torch

import recnet_amd as R
from tests import lr_schedule_ref as LR

REL = 1e-12      # a thousand double ulps, for cos / pow of two math libraries; four orders below one fp32 ulp, where the value is consumed
BASE = 3e-4


def _close(a, b, rel=REL):
    return abs(a - b) <= rel * abs(b)


# every kind with a warm-up, and the parameters that matter for it (cosine: min_factor >= 0.1, so the end of the curve is no cancellation)
SCHEDULES = {
    "constant": dict(kind="constant", warmup_steps=4),
    "linear": dict(kind="linear", warmup_steps=4, total_steps=20, min_factor=0.25),
    "cosine": dict(kind="cosine", warmup_steps=4, total_steps=20, min_factor=0.1),
    "invsqrt": dict(kind="invsqrt", warmup_steps=4, min_factor=0.3),
    "step": dict(kind="step", warmup_steps=4, period=3, gamma=0.5, min_factor=0.05),
    "linear_no_warmup": dict(kind="linear", total_steps=10),
    "cosine_no_warmup": dict(kind="cosine", total_steps=7, min_factor=0.5),
    "step_no_floor": dict(kind="step", period=2, gamma=0.9),
    "invsqrt_no_warmup": dict(kind="invsqrt"),
}


# ------------------------------------------------------------------------------------------- 1. the restatement
def test_restatement_at_hand_computed_points():
    """W = 4, total = 20: n = 1, W - 1, W, W + 1, total, beyond it, and the floor."""
    f = LR.factor
    lin = SCHEDULES["linear"]
    assert f(lin, 1) == 0.25 and f(lin, 3) == 0.75 and f(lin, 4) == 1.0                       # warm-up n / W; its last step is W - 1
    assert f(lin, 5) == 1.0 - 0.75 * 1 / 16 and f(lin, 12) == 1.0 - 0.75 * 8 / 16
    assert f(lin, 20) == 0.25 and f(lin, 21) == 0.25 and f(lin, 10 ** 9) == 0.25              # the end, and beyond it
    cos = SCHEDULES["cosine"]
    assert f(cos, 1) == 0.25 and f(cos, 3) == 0.75 and f(cos, 4) == 1.0
    assert _close(f(cos, 5), 0.1 + 0.9 * 0.5 * (1 + math.cos(math.pi / 16)))
    assert _close(f(cos, 12), 0.55)                                                           # half way: fmin + (1 - fmin) / 2
    assert _close(f(cos, 20), 0.1) and _close(f(cos, 400), 0.1)
    inv = SCHEDULES["invsqrt"]
    assert f(inv, 1) == 0.25 and f(inv, 3) == 0.75 and f(inv, 4) == 1.0 and f(inv, 5) == math.sqrt(4 / 5)
    assert f(inv, 16) == 0.5 and f(inv, 44) == math.sqrt(4 / 44) and f(inv, 45) == 0.3 and f(inv, 10 ** 6) == 0.3      # sqrt(4/45) < 0.3
    stp = SCHEDULES["step"]
    assert f(stp, 1) == 0.25 and f(stp, 4) == 1.0 and f(stp, 6) == 1.0 and f(stp, 7) == 0.5 and f(stp, 10) == 0.25
    assert f(stp, 16) == 0.0625 and f(stp, 19) == 0.05 and f(stp, 10 ** 6) == 0.05            # 0.5^5 < 0.05: the floor
    con = SCHEDULES["constant"]
    assert [f(con, n) for n in (1, 2, 3, 4, 5, 1000)] == [0.25, 0.5, 0.75, 1.0, 1.0, 1.0]
    assert f(None, 1) == 1.0 and f(None, 12345) == 1.0
    assert f(SCHEDULES["invsqrt_no_warmup"], 1) == 1.0 and f(SCHEDULES["invsqrt_no_warmup"], 4) == 0.5
    assert LR.lr_at(lin, BASE, 12, scale=0.5) == BASE * 0.5 * 0.625


def _torch_lrs(make, steps):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=BASE)
    sched = make(opt)
    out = []
    for _ in range(steps):
        out.append(opt.param_groups[0]["lr"])      # the lr of optimiser step n = len(out)
        opt.step()
        sched.step()
    return out


def test_restatement_against_torch_schedulers():
    """Index mapping: torch's schedulers count epochs e = 0, 1, ... and the lr of epoch e is what the (e + 1)-th optimiser step
    uses, so e = n - 1.
      StepLR(step_size = p, gamma): lr_e = base gamma^floor(e / p)          = step with W = 1: m = n - 1 = e, warm(n >= 1) = 1
      LinearLR(start_factor = 1, end_factor = fmin, total_iters = M): lr_e = base (1 - (1 - fmin) min(e, M) / M)
                                                                            = linear with W = 1, total_steps = M + 1
      CosineAnnealingLR(T_max = M, eta_min = base fmin), closed form for e <= M: eta_min + (base - eta_min)(1 + cos(pi e / M)) / 2
                                                                            = cosine with W = 1, total_steps = M + 1
    (torch's chained / recursive forms round differently from the closed form: 1e-9 relative covers sixty recursive steps.)"""
    from torch.optim import lr_scheduler as S
    N = 60
    got = _torch_lrs(lambda o: S.StepLR(o, step_size=7, gamma=0.6), N)
    ours = [LR.lr_at(dict(kind="step", warmup_steps=1, period=7, gamma=0.6), BASE, n) for n in range(1, N + 1)]
    assert all(_close(a, b, 1e-9) for a, b in zip(ours, got)), (ours[:10], got[:10])
    got = _torch_lrs(lambda o: S.LinearLR(o, start_factor=1.0, end_factor=0.2, total_iters=25), N)
    ours = [LR.lr_at(dict(kind="linear", warmup_steps=1, total_steps=26, min_factor=0.2), BASE, n) for n in range(1, N + 1)]
    assert all(_close(a, b, 1e-9) for a, b in zip(ours, got)), (ours[:10], got[:10])
    M = 40
    got = _torch_lrs(lambda o: S.CosineAnnealingLR(o, T_max=M, eta_min=BASE * 0.1), M + 1)      # (beyond T_max torch's curve rises again)
    ours = [LR.lr_at(dict(kind="cosine", warmup_steps=1, total_steps=M + 1, min_factor=0.1), BASE, n) for n in range(1, M + 2)]
    assert all(_close(a, b, 1e-9) for a, b in zip(ours, got)), (ours[:10], got[:10])
    closed = [BASE * 0.1 + (BASE - BASE * 0.1) * (1 + math.cos(math.pi * e / M)) / 2 for e in range(M + 1)]
    assert all(_close(a, b) for a, b in zip(ours, closed))
    # a linear warm-up: LinearLR(start_factor = 1 / W, total_iters = W - 1) is e -> (e + 1) / W = n / W
    W = 8
    got = _torch_lrs(lambda o: S.LinearLR(o, start_factor=1.0 / W, end_factor=1.0, total_iters=W - 1), 20)
    ours = [LR.lr_at(dict(kind="constant", warmup_steps=W), BASE, n) for n in range(1, 21)]
    assert all(_close(a, b, 1e-9) for a, b in zip(ours, got)), (ours, got)


# ------------------------------------------------------------------------------------------- 2. recnet_lr_at
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from recnet_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_lr_at_matches_the_restatement(lib, name):
    from recnet_amd import _lib
    s = SCHEDULES[name]
    W, total = s.get("warmup_steps", 0), s.get("total_steps", 0) or 20
    points = sorted(set([1, max(W - 1, 1), max(W, 1), W + 1, total, total + 1, 3 * total, 10 ** 6, 2 ** 31 + 5]) | set(range(1, 2 * total + 1)))
    worst = 0.0
    for scale in (1.0, 0.37):
        for n in points:
            got, ref = _lib.lr_at(s, scale, BASE, n), LR.lr_at(s, BASE, n, scale)
            worst = max(worst, abs(got - ref) / abs(ref) if ref else abs(got))      # (gamma ^ 10^6 underflows to 0 on both sides)
            assert _close(got, ref), (name, n, scale, got, ref)
    print("%s: worst relative difference %.2e over %d steps" % (name, worst, len(points)))


def test_lr_at_without_a_schedule_is_the_base_lr_bit_for_bit(lib):
    from recnet_amd import _lib
    for base in (BASE, 1e-5, 1e-6, 0.1, 1.0 / 3.0):
        for n in (1, 2, 7, 10 ** 5):
            assert _lib.lr_at(None, 1.0, base, n) == base
            assert _lib.lr_at(dict(kind="constant"), 1.0, base, n) == base
    assert _lib.lr_at(None, 0.5, BASE, 3) == BASE * 0.5      # the scale applies without a schedule too


# ------------------------------------------------------------------------------------------- 3. validation and symbols
def _handle(lib):
    from recnet_amd import _lib
    c = _lib.Config()
    c.batch_size, c.encoder_output_len, c.encoder_output_size, c.embedding_size = 100, 28, 1536, 468
    c.decoder_hidden_size, c.decoder_attn_size, c.n_vocabs = 512, 128, 4188
    c.reconstructor_hidden_size, c.reconstructor_attn_size, c.caption_max_len = 1536, 128, 30
    c.reconstructor_type, c.precision, c.global_batch_size = _lib.REC_GLOBAL, _lib.PREC_BF16, 100
    h = C.c_void_p()
    assert lib.recnet_create(C.byref(c), C.byref(h)) == 0
    return h


NAN = float("nan")
INVALID = [
    (dict(kind=6), b"kind"), (dict(kind=-1), b"kind"),
    (dict(kind=1, warmup_steps=-1), b"negative"), (dict(kind=1, total_steps=-3), b"negative"),
    (dict(kind=2, warmup_steps=5, total_steps=5), b"total_steps"), (dict(kind=3, warmup_steps=5, total_steps=4), b"total_steps"),
    (dict(kind=2), b"total_steps"),
    (dict(kind=5, period=0), b"period"), (dict(kind=5, period=-2), b"period"),
    (dict(kind=1, min_factor=-0.1), b"min_factor"), (dict(kind=1, min_factor=1.5), b"min_factor"), (dict(kind=1, min_factor=NAN), b"min_factor"),
    (dict(kind=5, period=2, gamma=0.0), b"gamma"), (dict(kind=5, period=2, gamma=1.01), b"gamma"), (dict(kind=5, period=2, gamma=NAN), b"gamma"),
    (dict(kind=1, scale=0.0), b"scale"), (dict(kind=1, scale=-1.0), b"scale"), (dict(kind=1, scale=NAN), b"scale"),
    (dict(kind=0, scale=float("inf")), b"scale"),
]


def _desc(**kw):
    from recnet_amd import _lib
    d = _lib.LRScheduleDesc(0, 0, 0, 0, 0.0, 1.0, 1.0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_set_lr_schedule_checks_its_descriptor_on_a_host_only_handle(lib):
    from recnet_amd import _lib
    assert C.sizeof(_lib.LRScheduleDesc) == 4 * 4 + 3 * 8
    h = _handle(lib)
    got = _lib.LRScheduleDesc()
    for which in (0, 1):      # a handle's state at creation: no schedule, scale 1
        assert lib.recnet_get_lr_schedule(h, which, C.byref(got)) == 0
        assert (got.kind, got.warmup_steps, got.total_steps, got.period, got.min_factor, got.gamma, got.scale) == (0, 0, 0, 0, 0.0, 1.0, 1.0)
    good = _desc(kind=_lib.LR_COSINE, warmup_steps=2, total_steps=6, min_factor=0.1, scale=0.5)
    assert lib.recnet_set_lr_schedule(h, 1, C.byref(good), None) == 0, lib.recnet_last_error()
    for kw, msg in INVALID:
        assert lib.recnet_set_lr_schedule(h, 0, C.byref(_desc(**kw)), None) == -1, kw
        assert msg in lib.recnet_last_error(), (kw, lib.recnet_last_error())
        out = C.c_double(0.0)
        assert lib.recnet_lr_at(C.byref(_desc(**kw)), 1e-3, 1, C.byref(out)) == -1, kw
    for which in (-1, 2):
        assert lib.recnet_set_lr_schedule(h, which, C.byref(good), None) == -1 and b"model index" in lib.recnet_last_error()
        assert lib.recnet_get_lr_schedule(h, which, C.byref(got)) == -1
    assert lib.recnet_set_lr_schedule(h, 0, None, None) == -1 and lib.recnet_set_lr_schedule(None, 0, C.byref(good), None) == -1
    out = C.c_double(0.0)
    assert lib.recnet_lr_at(C.byref(good), 1e-3, 0, C.byref(out)) == -1 and b"step" in lib.recnet_last_error()
    # nothing of the refused descriptors was kept: the decoder's is untouched, the reconstructor's is the valid one
    assert lib.recnet_get_lr_schedule(h, 0, C.byref(got)) == 0 and (got.kind, got.scale) == (0, 1.0)
    assert lib.recnet_get_lr_schedule(h, 1, C.byref(got)) == 0
    assert (got.kind, got.warmup_steps, got.total_steps, got.period, got.min_factor, got.gamma, got.scale) == (3, 2, 6, 0, 0.1, 1.0, 0.5)
    # every kind round-trips, as api.LRSchedule describes it
    for name, s in SCHEDULES.items():
        d = _lib.lr_desc(R.LRSchedule.from_dict(s).to_dict(), 0.75)
        assert lib.recnet_set_lr_schedule(h, 0, C.byref(d), None) == 0, (name, lib.recnet_last_error())
        assert lib.recnet_get_lr_schedule(h, 0, C.byref(got)) == 0
        assert all(getattr(got, f) == getattr(d, f) for f, _ in _lib.LRScheduleDesc._fields_), name
    assert lib.recnet_read_lr(h, (C.c_double * 2)(), None) == -2 and b"workspace" in lib.recnet_last_error()      # no device memory yet
    lib.recnet_destroy(h)


def test_header_exports_and_library_agree_on_the_new_symbols(lib):
    import os
    import re
    from recnet_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "recnet_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("recnet_set_lr_schedule", "recnet_get_lr_schedule", "recnet_lr_at", "recnet_read_lr"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS and hasattr(lib, name), name
    body = hdr[hdr.index("typedef struct recnet_lr_schedule {"):hdr.index("} recnet_lr_schedule;")]
    fields = []
    for _, names in re.findall(r"\b(int32_t|double)\s+([^;{]+);", body):
        fields += [x.strip() for x in names.split(",")]
    assert fields == [f[0] for f in _lib.LRScheduleDesc._fields_]
    for name, value in (("NONE", _lib.LR_NONE), ("CONSTANT", _lib.LR_CONSTANT), ("LINEAR", _lib.LR_LINEAR), ("COSINE", _lib.LR_COSINE),
                        ("INVSQRT", _lib.LR_INVSQRT), ("STEP", _lib.LR_STEP)):
        assert int(re.search(r"#define\s+RECNET_LR_%s\s+(\d+)" % name, hdr).group(1)) == value
    assert sorted(_lib.LR_KINDS) == sorted(R.LRSchedule.KINDS) == sorted(LR.KINDS)


# ------------------------------------------------------------------------------------------- 4. state dicts and propagation
class _StubEngine:
    """What FusedAdam's pushes touch of an Engine (the real one needs a GPU)."""

    def __init__(self, hyper):
        self.opt_hyper = {0: hyper, 1: hyper}
        self.lr_sched = {0: (None, 1.0), 1: (None, 1.0)}
        self.captured_steps = set()
        self.calls = []

    def set_optimizer_hyper(self, which, *hp):
        self.opt_hyper[which] = hp

    def set_lr_schedule(self, which, fields, scale=1.0):
        self.calls.append((which, fields, scale))
        self.lr_sched[which] = (fields, scale)


def _decoder(**cfg):
    C_ = R.make_config(device="cpu", encoder_output_size=16, reconstructor_hidden_size=16, embedding_size=8, decoder_hidden_size=8,
                       decoder_attn_size=4, **cfg)
    return R.build_decoder(20, C_)


def test_lr_schedule_is_a_plain_value():
    s = R.LRSchedule("cosine", warmup_steps=2, total_steps=6, min_factor=0.1)
    d = s.to_dict()
    assert d == dict(kind="cosine", warmup_steps=2, total_steps=6, period=0, min_factor=0.1, gamma=1.0)
    assert R.LRSchedule.from_dict(d) == s and R.LRSchedule.from_dict(dict(kind="cosine", warmup_steps=2, total_steps=6, min_factor=0.1)) == s
    assert R.LRSchedule.from_dict(None) is None and R.LRSchedule.from_dict(s) is s
    assert R.LRSchedule("constant").to_dict() == dict(kind="constant", warmup_steps=0, total_steps=0, period=0, min_factor=0.0, gamma=1.0)
    with pytest.raises(ValueError, match="kind"):
        R.LRSchedule("exponential")
    with pytest.raises(ValueError, match="field"):
        R.LRSchedule.from_dict(dict(kind="step", step_size=3))


def test_fused_adam_hands_schedule_and_scale_to_its_engines_also_under_a_live_graph(lib):
    dec = _decoder()
    opt = dec["optimizer"]
    first = (1e-5, 1e-5, 0.9, 0.999, 1e-8)
    a, b = _StubEngine(first), _StubEngine(first)
    dec["_state"].engines.update({("x",): a, ("y",): b})
    assert opt.lr_schedule is None and opt.lr_scale == 1.0
    opt.push_hyper()
    assert a.calls == [] and b.calls == []                                   # nothing set: nothing is sent
    b.captured_steps.add(object())                                           # a live GraphedStep is no obstacle: that is the feature
    s = R.LRSchedule("step", period=2, gamma=0.5)
    opt.set_lr_schedule(s)
    assert a.calls == [(0, s.to_dict(), 1.0)] and b.calls == a.calls and opt.lr_schedule == s
    opt.push_hyper()
    assert len(a.calls) == 1                                                 # compare, then push only on change
    assert opt.scale_lr(0.5) == 0.5 and opt.lr_scale == 0.5
    assert a.calls[-1] == (0, s.to_dict(), 0.5) and b.calls[-1] == a.calls[-1] and len(a.calls) == 2
    c = _StubEngine(first)                                                   # an engine bound later gets both at the next step's push
    dec["_state"].engines[("z",)] = c
    opt.push_hyper()
    assert c.calls == [(0, s.to_dict(), 0.5)] and len(a.calls) == 2
    opt.set_lr_schedule(None)
    opt.lr_scale = 1.0
    assert a.lr_sched[0] == (None, 1.0) and c.lr_sched[0] == (None, 1.0) and opt.lr_schedule is None
    # the base lr keeps meaning what it meant: editing it under a live graph raises as before
    opt.param_groups[0]["lr"] = 3e-4
    with pytest.raises(RuntimeError, match="capture again"):
        opt.push_hyper()
    opt.param_groups[0]["lr"] = 1e-5
    # what the library refuses is not stored (_lib.RecNetError, a RuntimeError)
    n = len(a.calls)
    for bad in (dict(kind="linear", warmup_steps=5, total_steps=5), dict(kind="step", period=0), dict(kind="constant", min_factor=2.0)):
        with pytest.raises(RuntimeError, match="lr schedule"):
            opt.set_lr_schedule(bad)
    with pytest.raises(RuntimeError, match="scale"):
        opt.lr_scale = 0.0
    assert opt.lr_schedule is None and opt.lr_scale == 1.0 and len(a.calls) == n


def test_get_last_lr_is_the_schedule_at_the_models_step_count(lib):
    s = dict(kind="cosine", warmup_steps=2, total_steps=6, min_factor=0.1)
    dec = _decoder(decoder_lr_schedule=s, decoder_learning_rate=2e-3)      # installed by build_decoder from the config
    opt = dec["optimizer"]
    assert opt.lr_schedule == R.LRSchedule.from_dict(s)
    assert opt.get_last_lr() == pytest.approx(LR.lr_at(s, 2e-3, 1), rel=REL)      # before the first step: step 1's
    for n in (1, 2, 3, 6, 9):
        dec["_state"].step = n
        assert _close(opt.get_last_lr(), LR.lr_at(s, 2e-3, n))
    opt.scale_lr(0.5)
    assert _close(opt.get_last_lr(), LR.lr_at(s, 2e-3, 9, 0.5))
    plain = _decoder()
    assert plain["optimizer"].lr_schedule is None and plain["optimizer"].get_last_lr() == 1e-5


def test_state_dicts_carry_the_schedule_and_load_without_it(lib):
    dec = _decoder()
    opt = dec["optimizer"]
    s = R.LRSchedule("linear", warmup_steps=2, total_steps=5, min_factor=0.25)
    opt.set_lr_schedule(s)
    opt.scale_lr(0.25)
    sd = opt.state_dict()
    assert sd["param_groups"][0]["lr_schedule"] == s.to_dict() and sd["param_groups"][0]["lr_scale"] == 0.25
    assert set(sd["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}      # torch.optim.Adam's layout otherwise
    other = _decoder()
    eng = _StubEngine((1e-5, 1e-5, 0.9, 0.999, 1e-8))
    other["_state"].engines[("x",)] = eng
    other["optimizer"].load_state_dict(sd)
    assert other["optimizer"].lr_schedule == s and other["optimizer"].lr_scale == 0.25
    assert eng.lr_sched[0] == (s.to_dict(), 0.25)                            # and it reached the engine
    assert other["optimizer"].state_dict()["param_groups"][0]["lr_schedule"] == s.to_dict()
    none = _decoder()
    none["optimizer"].load_state_dict(_decoder()["optimizer"].state_dict())  # ours, with "no schedule" in it
    assert none["optimizer"].lr_schedule is None and none["optimizer"].lr_scale == 1.0
    # a reference-style dict: torch.optim.Adam's own, which has neither key
    fresh = _decoder()
    P = [torch.nn.Parameter(p.detach().clone()) for p in fresh["model"].parameters()]
    adam = torch.optim.Adam(P, lr=1e-4, amsgrad=True)
    for p in P:
        p.grad = torch.ones_like(p)
    adam.step()
    ref_sd = adam.state_dict()
    assert "lr_schedule" not in ref_sd["param_groups"][0]
    fresh["optimizer"].load_state_dict(ref_sd)
    assert fresh["optimizer"].lr_schedule is None and fresh["optimizer"].lr_scale == 1.0
    assert fresh["_state"].step == 1 and fresh["optimizer"].param_groups[0]["lr"] == 1e-4
    assert fresh["optimizer"].state_dict()["param_groups"][0]["lr_schedule"] is None


# ------------------------------------------------------------------------------------------- 5. reduce-on-plateau
class _StubOpt:
    def __init__(self):
        self._scale, self.calls = 1.0, []

    @property
    def lr_scale(self):
        return self._scale

    @lr_scale.setter
    def lr_scale(self, v):
        self.calls.append(("set", v))
        self._scale = v

    def scale_lr(self, factor):
        self.calls.append(("scale", factor))
        self._scale *= factor
        return self._scale


def _trainer(plateau, rec=True):
    tr = R.Trainer.__new__(R.Trainer)      # the host logic alone: no models, no engine
    tr.decoder = {"optimizer": _StubOpt()}
    tr.reconstructor = {"optimizer": _StubOpt()} if rec else None
    tr._plateau_init(plateau)
    return tr, tr.decoder["optimizer"], (tr.reconstructor["optimizer"] if rec else None)


def test_plateau_counts_patience_and_scales_the_named_optimisers():
    tr, d, r = _trainer(dict(factor=0.5, patience=2, min_scale=0.2))
    for loss in (3.0, 2.5, 2.4, 2.0):                                        # improving: never a call
        assert tr.plateau_step(loss) is False
    assert d.calls == [] and r.calls == []
    assert tr.plateau_step(2.0) is False and d.calls == []                   # one validation without a new best (equal is none)
    assert tr.plateau_step(2.1) is True                                      # the second in a row
    assert d.calls == [("scale", 0.5)] and r.calls == [("scale", 0.5)] and d.lr_scale == 0.5
    assert tr.plateau_step(2.2) is False                                     # the count started again
    assert tr.plateau_step(1.9) is False and tr.plateau_step(1.95) is False  # a new best resets it
    assert tr.plateau_step(1.95) is True and d.lr_scale == 0.25 and len(d.calls) == 2
    # the floor: 0.25 * 0.5 < 0.2 -> 0.2 once, then nothing is sent
    assert tr.plateau_step(5.0) is False and tr.plateau_step(5.0) is True
    assert d.lr_scale == 0.2 and d.calls[-1] == ("set", 0.2) and r.lr_scale == 0.2
    n = len(d.calls)
    assert tr.plateau_step(5.0) is False and tr.plateau_step(5.0) is False
    assert len(d.calls) == n and d.lr_scale == 0.2


def test_plateau_which_and_defaults():
    tr, d, r = _trainer(dict(patience=1, which=(1,)))
    assert tr.plateau_step(1.0) is False and tr.plateau_step(1.0) is True
    assert d.calls == [] and r.calls == [("scale", 0.5)]                     # the default factor, the reconstructor only
    tr, d, _ = _trainer(dict(patience=1), rec=False)                         # no reconstructor: the decoder alone
    assert tr.plateau_step(1.0) is False and tr.plateau_step(2.0) is True and d.lr_scale == 0.5
    tr, d, r = _trainer(None)
    assert all(tr.plateau_step(x) is False for x in (1.0, 2.0, 3.0, 4.0)) and d.calls == [] and r.calls == []
    for bad in (dict(factor=1.0), dict(factor=0.0), dict(patience=0), dict(min_scale=-0.1), dict(which=(2,)), dict(cooldown=3)):
        with pytest.raises(ValueError, match="plateau"):
            _trainer(bad)
