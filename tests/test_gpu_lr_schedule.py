"""Learning-rate schedules under graph replay: the schedule descriptor and the reduce-on-plateau scale
live in device memory, every Adam launch — adam_chunk_kernel and the Adam epilogue of the pending d W_hh product — multiplies
the base lr by the schedule's factor at the step the update belongs to, and writes the lr it used into a slot the host can read
(FusedAdam.read_lr).  Held to the float64 restatement tests/lr_schedule_ref.py, to the procedure the feature replaces (edit the
param group, capture again), to the immediate update where the reconstructor's is deferred, and to a float64 Adam.

Shape: optim_ref.CHAIN = SHAPES["chains"] of tests/test_gpu_deferred.py, the smallest that runs the persistent chains and, for the
split update, the GEMM-epilogue Adam.  Only the one-graph form is run: tests/test_gpu_dp.py reaches the three-graph form through
worker processes only."""
import gc

import numpy as np
import pytest
import torch

import recnet_amd as R
from recnet_amd import _lib
from tests import golden_util as GU
from tests import lr_schedule_ref as LR
from tests import optim_ref as OR
from tests.gpu_util import make_models

pytestmark = pytest.mark.gpu

DIMS = OR.CHAIN
REL = 1e-12      # the bound of tests/test_lr_schedule.py: a thousand double ulps for cos / pow of two math libraries

COSINE = dict(kind="cosine", warmup_steps=2, total_steps=6, min_factor=0.1)
STEP = dict(kind="step", period=2, gamma=0.5)
LINEAR = dict(kind="linear", warmup_steps=2, total_steps=5, min_factor=0.25)      # factors 0.5, 1, 0.75, 0.5, 0.25: up to 4 x apart


def _close(a, b):
    return abs(a - b) <= REL * abs(b)


def _build(kind="global", prec="bf16", **cfg):
    B, F, D, V, E, H, A, RA = DIMS
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D), 3)
    recP = GU.formula_params(GU.rec_shapes(kind, H, D, RA), 4)
    _, dec, rec = make_models(list(DIMS), kind, prec, decP, recP, **cfg)
    step = R.DataParallelTrainStep(dec, rec, B, 0, 1, n_frames=F)
    return dec, rec, step, recP


def _full_batch(step, seed=9):
    """One batch whose longest caption has the full length: T = caption_max_len + 1."""
    B, F, D, V = DIMS[:4]
    lens = [30] + [int(x) for x in np.random.RandomState(1).randint(1, 30, size=B - 1)]
    enc, targets = GU.make_batch(B, F, D, V, lens, seed)
    T, w = step.prepare(targets.numpy())
    return enc.cuda(), targets.cuda(), T, w


def _base(md):
    return md["optimizer"].param_groups[0]["lr"]


# ---- the comparator of tests/test_gpu_deferred.py, restated
def _state(md):
    st = md["_state"].flat()
    out = {"p." + k: v.detach().clone() for k, v in md["model"].state_dict().items()}
    for name in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if md["_state"].amsgrad else ()):
        for k, v in st[name].views.items():
            out[name + "." + k] = v.detach().clone()
    return out


def _atomic(name):
    """Gradients summed with float atomics (column sums, the embedding scatter): reproducible to fp32 rounding only."""
    return any(t in name for t in ("bias", "attn_b", "attn_w.", "embedding"))


def _same(a, b, name, exact):
    if exact and not _atomic(name):
        return torch.equal(a, b)
    return torch.allclose(a, b, rtol=2e-4, atol=2e-8)


def _hold_states(a, b, loss_rtol=1e-6, exact_rec=True):
    """a, b: (decoder state, reconstructor state, losses [steps, 8])."""
    assert np.allclose(a[2][:, :7], b[2][:, :7], rtol=loss_rtol, atol=0), (a[2][:, 6], b[2][:, 6])
    for k in a[0]:
        assert _same(a[0][k], b[0][k], k, True), ("decoder", k, float((a[0][k] - b[0][k]).abs().max()))
    for k in a[1]:
        assert _same(a[1][k], b[1][k], k, exact_rec), ("reconstructor", k, float((a[1][k] - b[1][k]).abs().max()))


# ------------------------------------------------------------------------------------------- 6. the lr the device used
def test_replayed_step_uses_the_schedule_installed_after_its_capture():
    dec, rec, step, _ = _build()
    enc, targets, T, w = _full_batch(step)
    run = R.GraphedStep(step, enc, targets, T, w, warmup=0)
    od, orr = dec["optimizer"], rec["optimizer"]
    od.set_lr_schedule(COSINE)                       # after the capture, a different kind on each optimiser
    orr.set_lr_schedule(R.LRSchedule.from_dict(STEP))
    scale = 1.0
    for i in range(6):
        if i == 4:
            assert od.scale_lr(0.5) == 0.5 and orr.scale_lr(0.5) == 0.5      # reduce-on-plateau between two replays
            scale = 0.5
        run()
        n = dec["_state"].step
        assert n == i + 1 and rec["_state"].step == n
        got = (od.read_lr(), orr.read_lr())
        ref = (LR.lr_at(COSINE, _base(dec), n, scale), LR.lr_at(STEP, _base(rec), n, scale))
        host = (od.get_last_lr(), orr.get_last_lr())
        print("step %d: device %r, restatement %r, host %r" % (n, got, ref, host))
        assert _close(got[0], ref[0]) and _close(got[1], ref[1]), (n, got, ref)
        assert _close(got[0], host[0]) and _close(got[1], host[1]), (n, got, host)
        if i == 4:                                   # the next value after scale_lr(0.5) is half of what it would have been
            assert _close(got[0], 0.5 * LR.lr_at(COSINE, _base(dec), n)) and _close(got[1], 0.5 * LR.lr_at(STEP, _base(rec), n))
    eng = step.step_impl.engine
    assert eng.read_lr() == (od.read_lr(), orr.read_lr())
    assert eng.chain_status() == 0
    assert eng.images_stale() == 0


# ------------------------------------------------------------------------------------------- 7. equal to the procedure it replaces
def _run_device_schedule(sched, steps=4, defer=False, prec="bf16", change=None, want_split=False):
    """A GraphedStep with `sched` on both optimisers, `steps` replays of one full-length batch.  change = (after_step, schedule):
    both optimisers get another schedule between two replays.  Returns (states and losses, the lr pairs read after every step,
    the reconstructor's lr read right after the change, initial reconstructor parameters)."""
    dec, rec, step, recP = _build(prec=prec)
    enc, targets, T, w = _full_batch(step)
    run = R.GraphedStep(step, enc, targets, T, w, warmup=0, defer_reconstructor_update=defer)
    assert run.deferred == bool(defer)
    eng = step.step_impl.engine
    if want_split:      # RECNET_DIM_SPLIT_FITS: the split update is applied here, so the GEMM epilogue is what updates W_hh
        assert eng.lib.recnet_dim(eng.handle, _lib.DIM_SPLIT_FITS) == 1
    dec["optimizer"].set_lr_schedule(sched)
    rec["optimizer"].set_lr_schedule(sched)
    losses, lrs, at_change = [], [], None
    for i in range(steps):
        if change is not None and i == change[0]:
            dec["optimizer"].set_lr_schedule(change[1])      # (completes the pending update of step i first, with the old schedule)
            at_change = rec["optimizer"].read_lr()
            rec["optimizer"].set_lr_schedule(change[1])
        losses.append(run().clone())
        lrs.append(eng.read_lr())
    run.flush()
    torch.cuda.synchronize()
    lrs.append(eng.read_lr())                                # after the flush
    assert eng.chain_status() == 0
    assert eng.images_stale() == 0
    return (_state(dec), _state(rec), torch.stack(losses).cpu().numpy()), lrs, at_change, recP


def test_device_schedule_equals_editing_the_param_group_and_capturing_again():
    a, lrs, _, _ = _run_device_schedule(LINEAR)
    base = (1e-5, 1e-6)
    for n in range(1, 5):
        assert all(_close(lrs[n - 1][k], LR.lr_at(LINEAR, base[k], n)) for k in (0, 1)), (n, lrs[n - 1])
    # run B: fresh models, no schedule; before every step the lr of both param groups is set to the double run A reported, a new
    # GraphedStep is captured and replayed once — today's "drop, edit, capture again"
    dec, rec, step, _ = _build()
    enc, targets, T, w = _full_batch(step)
    losses = []
    for n in range(1, 5):
        dec["optimizer"].param_groups[0]["lr"], rec["optimizer"].param_groups[0]["lr"] = lrs[n - 1]
        run = R.GraphedStep(step, enc, targets, T, w, warmup=0)
        losses.append(run().clone())
        torch.cuda.synchronize()
        assert step.step_impl.engine.read_lr() == lrs[n - 1]      # no schedule: the param group's double, bit for bit
        del run
        gc.collect()
    assert dec["_state"].step == 4
    b = (_state(dec), _state(rec), torch.stack(losses).cpu().numpy())
    _hold_states(a, b)
    assert step.step_impl.engine.chain_status() == 0


# ------------------------------------------------------------------------------------------- 8. the deferred update's lr
def _rec_moved_alike(a, b, recP):
    """The reconstructor's movement in two runs.  Where the comparator holds a tensor to rtol 2e-4 of its VALUE, an update of lr 1e-6
    taken with another step's factor hides: 1e-6 against weights of 0.1.  So also: || (a - init) - (b - init) || <= 2 % of
    || b - init || per tensor.  Two correct runs see gradients equal to fp32 rounding, take Adam steps of lr x factor per element and
    differ by the rare parameter rounding that falls the other way: far below a percent.  One step's factor shifted by one
    (0.5, 1, 0.75, 0.5 in place of 1, 0.75, 0.5, 0.25 for a pending update taken at the next step's count) is 9 % of the sum."""
    for k, v in recP.items():
        da, db = a["p." + k].cpu().double() - v.double(), b["p." + k].cpu().double() - v.double()
        assert float(db.norm()) > 0, k
        assert float((da - db).norm()) <= 2e-2 * float(db.norm()), (k, float((da - db).norm()), float(db.norm()))


@pytest.mark.parametrize("prec", ["bf16", "f32"])
@pytest.mark.parametrize("mode", [True, "recurrent"])
def test_deferred_update_takes_the_lr_of_its_own_step(mode, prec):
    """The exactness classes of test_deferred_update_equals_the_immediate_one_once_flushed at full lengths and the reference's
    learning rates: losses to 1e-6 (3e-6 for the split update, whose in-step half is another grouped launch), the decoder bit for
    bit, the reconstructor bit for bit where the whole update is deferred."""
    split = mode == "recurrent" and prec == "bf16"
    imm, lrs0, _, recP = _run_device_schedule(LINEAR, prec=prec)
    dfr, lrs1, _, _ = _run_device_schedule(LINEAR, defer=mode, prec=prec, want_split=split)
    ref = [(LR.lr_at(LINEAR, 1e-5, n), LR.lr_at(LINEAR, 1e-6, n)) for n in range(1, 5)]
    print("immediate %r\ndeferred %r\nrestatement %r" % (lrs0, lrs1, ref))
    for n in range(1, 5):
        assert _close(lrs0[n - 1][0], ref[n - 1][0]) and _close(lrs0[n - 1][1], ref[n - 1][1])
        assert _close(lrs1[n - 1][0], ref[n - 1][0])
        if mode == "recurrent":      # the in-step half is the last reconstructor launch of step n
            assert _close(lrs1[n - 1][1], ref[n - 1][1])
        else:                        # step n's update runs in replay n + 1 (or, where the handle does not defer, in step n)
            either = [ref[n - 1][1]] + ([ref[n - 2][1]] if n > 1 else [0.0])      # (0.0: no reconstructor launch has run yet)
            assert any(lrs1[n - 1][1] == x or _close(lrs1[n - 1][1], x) for x in either), (n, lrs1[n - 1][1], either)
    assert _close(lrs1[4][1], ref[3][1])      # flushed: the last pending update was step 4's and took step 4's lr
    _hold_states(imm, dfr, loss_rtol=1e-6 if mode is True else 3e-6, exact_rec=mode is True)
    _rec_moved_alike(dfr[1], imm[1], recP)
    assert any(not torch.equal(dfr[1]["p." + k].cpu(), v) for k, v in recP.items())


@pytest.mark.parametrize("mode", [True, "recurrent"])
def test_schedule_change_completes_the_pending_update_with_the_old_schedule(mode):
    """Between replay 2 and 3 both optimisers get another schedule (a factor of 1e-3 at step 3 against 0.75).  The pending
    update of step 2 is completed by that call, with the schedule it belongs to."""
    other = dict(kind="step", period=1, gamma=0.1)
    imm, lrs0, at0, recP = _run_device_schedule(LINEAR, change=(2, other))
    dfr, lrs1, at1, _ = _run_device_schedule(LINEAR, defer=mode, change=(2, other), want_split=mode == "recurrent")
    old2 = LR.lr_at(LINEAR, 1e-6, 2)
    print("reconstructor lr right after the change: immediate %r, deferred %r, old schedule at step 2 %r, new one %r"
          % (at0, at1, old2, LR.lr_at(other, 1e-6, 2)))
    assert _close(at0, old2) and _close(at1, old2)
    for n in (3, 4):
        assert _close(lrs1[n - 1][0], LR.lr_at(other, 1e-5, n)) and _close(lrs0[n - 1][1], LR.lr_at(other, 1e-6, n))
    assert _close(lrs1[4][1], LR.lr_at(other, 1e-6, 4))
    _hold_states(imm, dfr, loss_rtol=1e-6 if mode is True else 3e-6, exact_rec=mode is True)
    _rec_moved_alike(dfr[1], imm[1], recP)


# ------------------------------------------------------------------------------------------- 9. the chunk kernel against float64 Adam
def _adam_chain(P, grads, amsgrad, lrs, dtype):
    """optim_ref.adam_stage step after step from zero moments, each step with its own lr, everything kept in `dtype`."""
    zeros = {k: torch.zeros_like(v) for k, v in P.items()}
    p, m, v, vm = P, zeros, zeros, zeros
    hy = {k: x for k, x in OR.HYPER.items() if k != "lr"}
    for n, (g, lr) in enumerate(zip(grads, lrs), 1):
        r = OR.adam_stage(p, g, m, v, vm if amsgrad else None, lr=lr, amsgrad=amsgrad, step=n, dtype=dtype, **hy)
        p, m, v, vm = r["p"], r["exp_avg"], r["exp_avg_sq"], r["max_exp_avg_sq"]
    return {q: r[q] for q in ("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")}


@pytest.mark.parametrize("amsgrad", [(True, False), (False, True)], ids=["ams_dec", "ams_rec"])
@pytest.mark.parametrize("kind", ["global", "local"])
def test_fused_adam_step_with_a_schedule_matches_float64_adam(kind, amsgrad):
    """Three FusedAdam.step() calls on preloaded gradients at optim_ref.HYPER with a cosine schedule (factors 0.5, 1, 0.87), against
    optim_ref.adam_stage in float64 with lr = lr_schedule_ref(n) per step, at the bars of its float32 run."""
    dims = OR.RAGGED
    B, F, D, V, E, H, A, RA = dims
    shapes = (GU.decoder_shapes(V, E, H, A, D), GU.rec_shapes(kind, H, D, RA))
    P = tuple(OR.model_params(s, 11 + w) for w, s in enumerate(shapes))
    lr, wd, (b1, b2) = OR.HYPER["lr"], OR.HYPER["weight_decay"], OR.HYPER["betas"]
    _, dec, rec = make_models(list(dims), kind, "bf16", P[0], P[1], decoder_learning_rate=lr, reconstructor_learning_rate=lr,
                              decoder_weight_decay=wd, reconstructor_weight_decay=wd, adam_beta1=b1, adam_beta2=b2,
                              adam_eps=OR.HYPER["eps"], decoder_use_amsgrad=amsgrad[0], reconstructor_use_amsgrad=amsgrad[1])
    for w, md in enumerate((dec, rec)):
        opt, ms = md["optimizer"], md["_state"]
        assert ms.amsgrad == amsgrad[w]
        opt.set_lr_schedule(COSINE)
        grads = [OR.make_inputs(shapes[w], 51 + 10 * i + w)["grad"] for i in range(3)]
        lrs = [LR.lr_at(COSINE, lr, n) for n in (1, 2, 3)]
        Pw = {k: P[w][k] for k in ms.params()}
        r64, r32 = _adam_chain(Pw, grads, ms.amsgrad, lrs, torch.float64), _adam_chain(Pw, grads, ms.amsgrad, lrs, torch.float32)
        views = ms.flat()["grad"].views
        for n, g in enumerate(grads, 1):
            for k, v in views.items():
                v.copy_(g[k])
            opt.step()
            assert _close(opt.read_lr(), lrs[n - 1]) and _close(opt.get_last_lr(), lrs[n - 1]), (n, opt.read_lr(), lrs[n - 1])
        torch.cuda.synchronize()
        fl = ms.flat()
        got = {"p": {k: p.detach().cpu() for k, p in ms.params().items()}, "max_exp_avg_sq": None}
        for q in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            if q in fl:
                got[q] = {k: v.cpu() for k, v in fl[q].views.items()}
        bar, err = OR.bars(r32, r64), OR.errors(got, r64)
        print("%s model %d amsgrad %s: " % (kind, w, ms.amsgrad) + ", ".join("%s %.2e (bar %.2e)" % (q, err[q], bar[q]) for q in bar))
        assert set(err) == set(bar) and all(err[q] <= bar[q] for q in bar), (w, err, bar)
        # the schedule was applied: at the constant base lr the parameters end up further away than the bar
        const = _adam_chain(Pw, grads, ms.amsgrad, [lr] * 3, torch.float64)
        assert OR.errors(const, r64)["p"] > 100 * bar["p"]
        eng = ms.engines[("opt",)]
        assert eng.chain_status() == 0
        assert eng.images_stale() == 0


# ------------------------------------------------------------------------------------------- 10. nothing moves without a schedule
def test_a_schedule_installed_and_removed_leaves_the_step_as_it_was():
    def run(touch):
        dec, rec, step, _ = _build()
        enc, targets, T, w = _full_batch(step)
        g = R.GraphedStep(step, enc, targets, T, w, warmup=0)
        if touch:
            for md in (dec, rec):
                md["optimizer"].set_lr_schedule(COSINE)
                md["optimizer"].scale_lr(0.25)
                md["optimizer"].set_lr_schedule(None)
                md["optimizer"].lr_scale = 1.0
        losses = [g().clone() for _ in range(4)]
        torch.cuda.synchronize()
        eng = step.step_impl.engine
        assert eng.read_lr() == (_base(dec), _base(rec))      # base_lr * 1.0 * 1.0: the param group's double, bit for bit
        assert eng.chain_status() == 0
        return _state(dec), _state(rec), torch.stack(losses).cpu().numpy()

    _hold_states(run(False), run(True))


# ------------------------------------------------------------------------------------------- 11. eager paths
def test_eager_steps_report_the_same_lr_sequence():
    dec, rec, step, _ = _build()
    enc, targets, T, w = _full_batch(step)
    od, orr = dec["optimizer"], rec["optimizer"]
    od.set_lr_schedule(COSINE)
    orr.set_lr_schedule(STEP)
    for n in range(1, 7):                            # TrainStep.__call__: the fused step, launched eagerly
        step.step_impl(enc, targets, T, w)
        assert dec["_state"].step == n
        got, ref = (od.read_lr(), orr.read_lr()), (LR.lr_at(COSINE, _base(dec), n), LR.lr_at(STEP, _base(rec), n))
        assert _close(got[0], ref[0]) and _close(got[1], ref[1]), (n, got, ref)
        assert _close(got[0], od.get_last_lr()) and _close(got[1], orr.get_last_lr())
    step(enc, targets, T, w)                         # forward + backward, then the optimiser step as its own call
    assert _close(od.read_lr(), LR.lr_at(COSINE, _base(dec), 7)) and _close(orr.read_lr(), LR.lr_at(STEP, _base(rec), 7))
    od.step()                                        # FusedAdam.step(): each optimiser alone, at its model's next step
    orr.step()
    assert dec["_state"].step == 8 and rec["_state"].step == 8
    assert _close(od.read_lr(), LR.lr_at(COSINE, _base(dec), 8)) and _close(orr.read_lr(), LR.lr_at(STEP, _base(rec), 8))
    assert step.step_impl.engine.chain_status() == 0
