"""The optimiser stage alone — norms, gradient clip, AMSGrad / Adam, the in-pass re-pack of the weight images
(csrc/kernels_optim.hpp, csrc/common.hpp: rn_adam_update) — held to a float64 torch.optim.Adam (tests/optim_ref.py).

The whole-step parity tests reach this stage through bf16 gradients, at the reference's default settings only: the clip is
never active there (dec_grad_norm <= 0.86 against a bar of 50), AMSGrad's max always picks the fresh value, and their
tolerances pass an error of a few percent of one update.  Here the stage is driven with chosen gradients and chosen moments
through the product's own engine, bindings and flat buffers: one train-mode forward + backward (it refreshes the parameter
norms the regulariser reads), then gradients and moments are overwritten with generated values and Engine.optimizer_step
runs.  The master update is fp32 whatever the precision of the packed images, so one set of bars holds.

Bars: per compared quantity, 8 x the error of the reference's own float32 run against its float64 run on the same inputs
(optim_ref.bars; never less than one fp32 ulp of the largest magnitude) — parameters: maximum absolute difference, moments:
per-tensor relative norm, total norm: relative.  tests/test_optim_ref.py shows that each of six plausible mistakes exceeds
them at least tenfold at these inputs.

Measured on an MI355X over the matrix below — largest error, and the case that came closest to its bar (every test prints
its own figures before it asserts; the bars differ per case):
  parameters (max abs)            1.2e-7    closest: 1.6e-8 against a bar of 7.9e-8 (0.21)
  exp_avg (rel. norm per tensor)  1.0e-7    closest: 1.0e-7 against 5.3e-7 (0.20)
  exp_avg_sq                      2.5e-7    closest: 2.5e-7 against 9.0e-7 (0.28)
  max_exp_avg_sq                  2.4e-7    closest: 2.4e-7 against 8.7e-7 (0.28)
  RN_SCAL_GNORM (relative)        1.4e-7    closest: 9.2e-8 against 1.2e-7, the one-ulp floor (0.75)
  stand-alone clip, norm          1.1e-7    closest: 1.1e-7 against 1.2e-7, the one-ulp floor (0.93)
  stand-alone clip, gradients     9.9e-8    closest: 9.9e-8 against 3.1e-7 (0.32)
  param_groups / load_state_dict  parameters 6.0e-8 against 4.8e-7, moments <= 8.1e-8 against >= 3.4e-7"""
import itertools

import numpy as np
import pytest
import torch

import recnet_amd as R
from tests import golden_util as GU
from tests import optim_ref as OR
from tests.gpu_util import make_models

pytestmark = pytest.mark.gpu

KINDS, CELLS, PRECS = ("global", "local"), (("LSTM", "LSTM"), ("GRU", "GRU")), ("f32", "bf16")
GNORM = 7      # scalars[7]: RN_SCAL_GNORM, the decoder's total gradient norm before clipping


class Stage:
    """The product's models, one TrainStep engine and the state after one forward + backward, for one engine-level setting."""

    def __init__(self, dims, kind, cells, prec, config):
        cfg = OR.CONFIGS[config]
        B, F, D, V, E, H, A, RA = dims
        self.cfg, self.kind, self.in_use = cfg, kind, False
        self.shapes = (GU.decoder_shapes(V, E, H, A, D, cells[0]), GU.rec_shapes(kind, H, D, RA, cells[1]))
        self.P = tuple(OR.model_params(s, 11 + w) for w, s in enumerate(self.shapes))
        lr, wd, (b1, b2) = OR.HYPER["lr"], OR.HYPER["weight_decay"], OR.HYPER["betas"]
        _, dec, rec = make_models(list(dims), kind, prec, self.P[0], self.P[1], cells=cells, decoder_learning_rate=lr,
                                  reconstructor_learning_rate=lr, decoder_weight_decay=wd, reconstructor_weight_decay=wd,
                                  adam_beta1=b1, adam_beta2=b2, adam_eps=OR.HYPER["eps"], decoder_use_amsgrad=cfg["amsgrad"][0],
                                  reconstructor_use_amsgrad=cfg["amsgrad"][1], gradient_clip=cfg["clip"],
                                  use_gradient_clip=cfg["use_clip"], decoder_lambda_reg=cfg["lam"][0],
                                  reconstructor_lambda_reg=cfg["lam"][1], lambda_recon=cfg["lam"][2])
        self.models = (dec, rec)
        self.step = R.TrainStep(dec, rec)
        self.eng = self.step.engine
        lens = [int(x) for x in np.random.RandomState(3).randint(1, 13, size=B)]
        enc, targets = GU.make_batch(B, F, D, V, lens, 77)
        T, w = self.step.prepare(targets.numpy())
        self.step.fwd_bwd(enc.cuda(), targets.cuda(), T, w, seed=5)
        torch.cuda.synchronize()
        for w_, md in enumerate(self.models):
            assert ("max_exp_avg_sq" in md["_state"].flat()) == cfg["amsgrad"][w_]      # no buffer is bound without AMSGrad

    def load(self, inputs):
        """Parameters back to their initial values (the norms the forward left stay valid), images re-packed, gradients and
        moments from `inputs` = (decoder's, reconstructor's)."""
        for md, P, inp in zip(self.models, self.P, inputs):
            for k, p in md["_state"].params().items():
                p.data.copy_(P[k])
            fl = md["_state"].flat()
            for q, fs in fl.items():
                fs.flat.zero_()
                for k, v in fs.views.items():
                    v.copy_(inp[q][k])
        self.eng.pack_weights()

    def read(self, which):
        md = self.models[which]
        fl = md["_state"].flat()
        out = {"p": {k: p.detach().cpu().clone() for k, p in md["_state"].params().items()}, "max_exp_avg_sq": None}
        for q in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq", "grad"):
            if q in fl:
                out[q] = {k: v.detach().cpu().clone() for k, v in fl[q].views.items()}
        return out

    def done(self):
        self.in_use = False

    def healthy(self):
        assert self.eng.chain_status() == 0
        assert self.eng.images_stale() == 0      # the packed images follow the parameters, whoever was (not) updated


@pytest.fixture(scope="module")
def stage():
    """stage(dims, kind, cells, prec, config): one live Stage at a time (the tests are ordered so that those of one setting
    follow each other), dropped with its engine, workspace and models when this module is done.  A test says st.done() as its
    last statement; a Stage whose test did not get there (it failed between a load and the end) is not handed on but built anew."""
    cache = {}

    def get(dims, kind, cells, prec, config):
        key = (tuple(dims), kind, cells, prec, config)
        st = cache.get(key)
        if st is None or st.in_use:
            st = None
            cache.clear()
            st = cache[key] = Stage(dims, kind, cells, prec, config)
        st.in_use = True
        return st

    yield get
    cache.clear()


def _same_bits(a, b):
    return all(torch.equal(a[q][k], b[q][k]) for q in ("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq") if a.get(q) is not None
               for k in a[q])


def _run_case(st, case):
    """Loads the case's inputs, runs the stage, returns ((inputs, reference kwargs) per model, device results per model)."""
    c = OR.CASES[case]
    io = [OR.case_inputs(case, st.shapes[w], st.P[w], w) for w in (0, 1)]
    st.load([x[0] for x in io])
    st.eng.scalars.zero_()
    if c.get("reg_first"):      # the autograd-compatible path: the regulariser's gradient added to the buffers first
        st.eng.add_reg_grad(0, 1.0)
        st.eng.add_reg_grad(1, st.cfg["lam"][2])
    st.eng.optimizer_step(c["step"], c["flags"])
    torch.cuda.synchronize()
    got = [st.read(0), st.read(1)]
    if io[0][1]["max_norm"] and not c["flags"] & OR.OPT_SKIP_DECODER:
        got[0]["total_norm"] = float(st.eng.scalars[GNORM])
    st.healthy()
    return io, got


def _hold(case, tag, which, P, inp, kw, got):
    """One model's device results against the float64 reference, at the bars the float32 reference run sets."""
    r64, r32 = OR.run_ref(P, inp, kw, torch.float64), OR.run_ref(P, inp, kw, torch.float32)
    bar, err = OR.bars(r32, r64), OR.errors(got, r64)
    if not kw["max_norm"]:
        del bar["total_norm"]      # (the device forms the total norm only where it clips)
    print("%s %s %s: " % (case, tag, ("decoder", "reconstructor")[which]) +
          ", ".join("%s %.2e (bar %.2e)" % (q, err[q], bar[q]) for q in bar))
    assert set(err) == set(bar), (err.keys(), bar.keys())      # every quantity of the reference was read back
    assert all(err[q] <= bar[q] for q in bar), (case, tag, which, {q: (err[q], bar[q]) for q in bar if not err[q] <= bar[q]})
    zk = [k for k, p in P.items() if not bool(p.any())]
    assert zk and all(not bool(got[q][k].any()) for k in zk for q in ("p", "exp_avg", "exp_avg_sq")), "the all-zero tensor stays zero"
    return r64


def _matrix(cases, dims_list=(OR.RAGGED,)):
    """(dims, kind, cells, prec, case) ordered by engine-level setting."""
    cases = sorted(cases, key=lambda c: OR.CASES[c]["config"])
    out = []
    for dims, kind, cells, prec in itertools.product(dims_list, KINDS, CELLS, PRECS):
        out += [pytest.param(dims, kind, cells, prec, c, id="-".join(("ragged" if dims == OR.RAGGED else "chain", kind, cells[0], prec, c)))
                for c in cases]
    return out


PLAIN = [c for c in OR.CASES if c not in ("edge_below", "skip_decoder", "skip_reconstructor")]


@pytest.mark.parametrize("dims,kind,cells,prec,case", _matrix(PLAIN) + _matrix(["clip_step2", "ams_both"], (OR.CHAIN,)))
def test_stage_matches_float64_adam(stage, dims, kind, cells, prec, case):
    """Clip active at about 10 x the bar (steps 1, 2, 1000, 100000: the bias corrections early and late) and just above it;
    clip off three ways (gradient_clip 0, use_gradient_clip False, flags without OPT_CLIP) with the same large gradients; AMSGrad
    swapped between the models, on for both, off for both, with about half of the elements taking the stored maximum;
    regulariser folded into the step or added to the gradients first, also with lambda_recon != 1; gradients small enough for
    eps to matter.  Both models against the reference, RN_SCAL_GNORM against the float64 norm of g + reg where the clip ran."""
    st = stage(dims, kind, cells, prec, OR.CASES[case]["config"])
    io, got = _run_case(st, case)
    for w in (0, 1):
        r64 = _hold(case, prec, w, st.P[w], io[w][0], io[w][1], got[w])
        assert ("max_exp_avg_sq" in r64 and r64["max_exp_avg_sq"] is not None) == st.cfg["amsgrad"][w]
        moved = max(float((got[w]["p"][k] - st.P[w][k]).abs().max()) for k in st.P[w])
        assert moved > 1e-3, "the update happened"
    if io[0][1]["max_norm"]:
        assert "total_norm" in got[0]
    st.done()


@pytest.mark.parametrize("dims,kind,cells,prec,case", _matrix(["edge_below"]))
def test_clip_just_below_the_bar_is_no_clip_bit_for_bit(stage, dims, kind, cells, prec, case):
    """|| g + reg || = clip * (1 - 1e-3): the coefficient clamps to exactly 1, so the step equals the one without OPT_CLIP
    bit for bit — and both are the reference's."""
    st = stage(dims, kind, cells, prec, "base")
    io, got = _run_case(st, case)
    for w in (0, 1):
        _hold(case, prec, w, st.P[w], io[w][0], io[w][1], got[w])
    st.load([x[0] for x in io])
    st.eng.optimizer_step(OR.CASES[case]["step"], OR.OPT_REG)
    torch.cuda.synchronize()
    assert _same_bits(got[0], st.read(0)) and _same_bits(got[1], st.read(1))
    st.healthy()
    st.done()


@pytest.mark.parametrize("dims,kind,cells,prec,case", _matrix(["skip_decoder", "skip_reconstructor"]))
def test_skip_flags_leave_one_model_untouched(stage, dims, kind, cells, prec, case):
    st = stage(dims, kind, cells, prec, "base")
    io, got = _run_case(st, case)      # (healthy(): the skipped model's images still equal a fresh pack of its parameters)
    skipped = 0 if case == "skip_decoder" else 1
    before = {"p": st.P[skipped], **{q: io[skipped][0][q] for q in ("exp_avg", "exp_avg_sq")},
              "max_exp_avg_sq": io[skipped][0]["max_exp_avg_sq"] if st.cfg["amsgrad"][skipped] else None}
    assert _same_bits(before, got[skipped]), "the skipped model's parameters and moments are unchanged bit for bit"
    _hold(case, prec, 1 - skipped, st.P[1 - skipped], io[1 - skipped][0], io[1 - skipped][1], got[1 - skipped])
    st.done()


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", KINDS)
def test_stand_alone_clip_grad_norm(stage, kind, prec, which):
    """api.clip_grad_norm_ (recnet_clip_grad_norm: the tensor_norm + norm_finalize pair and scale_grads_kernel, which the fused
    step does not take) against torch.nn.utils.clip_grad_norm_ in float64: the returned norm, the gradients scaled in place with
    max_norm below the norm, untouched bit for bit with max_norm above it."""
    st = stage(OR.RAGGED, kind, CELLS[0], prec, "base")
    io = [OR.case_inputs("flags_without_clip", st.shapes[w], st.P[w], w) for w in (0, 1)]
    g = io[which][0]["grad"]
    norm = OR.clip_ref(g, 1.0)[0]
    for max_norm in (2.0 * norm, 0.1 * norm):
        st.load([x[0] for x in io])
        ret = float(R.clip_grad_norm_(st.models[which], max_norm))
        torch.cuda.synchronize()
        got = st.read(which)["grad"]
        (n64, g64), (n32, g32) = OR.clip_ref(g, max_norm, torch.float64), OR.clip_ref(g, max_norm, torch.float32)
        nbar = max(OR.BAR_FACTOR * abs(n32 - n64) / n64, OR.EPS32)
        gerr = max(float((got[k].double() - g64[k]).norm()) / float(g64[k].norm()) for k in g if float(g64[k].norm()) > 0)
        gbar = max(OR.BAR_FACTOR * max(float((g32[k].double() - g64[k]).norm()) / float(g64[k].norm()) for k in g if float(g64[k].norm()) > 0),
                   OR.EPS32)
        print("clip_grad_norm_ %s %s model %d max_norm %.1f: norm %.2e (bar %.2e), gradients %.2e (bar %.2e)"
              % (kind, prec, which, max_norm, abs(ret - n64) / n64, nbar, gerr, gbar))
        assert abs(ret - n64) <= nbar * n64
        assert gerr <= gbar
        if max_norm > norm:
            assert all(torch.equal(got[k], g[k]) for k in g), "max_norm above the norm: gradients untouched bit for bit"
        else:
            assert abs(float(torch.sqrt(sum((x.double() ** 2).sum() for x in got.values()))) / max_norm - 1.0) < 1e-5
        assert all(not bool(got[k].any()) for k in g if not bool(g[k].any()))
        other = st.read(1 - which)["grad"]
        assert all(torch.equal(other[k], io[1 - which][0]["grad"][k]) for k in other), "the other model's gradients are not touched"
    st.healthy()
    st.done()


# ------------------------------------------------------------------------------------------- hyper-parameters edited later
def _adam_two_steps(P, g1, g2, amsgrad, hy0, dtype, edit=None):
    """torch.optim.Adam: one step with g1 at hy0 in float32 (the state a checkpoint holds), then — from those fp32 values — a
    second step with g2 in `dtype` after `edit` of the param group.  Returns (state_dict after step 1, parameters after step
    1, results of step 2)."""
    names = list(P)
    T = [P[k].clone().requires_grad_(True) for k in names]
    opt = torch.optim.Adam(T, amsgrad=amsgrad, foreach=False, **hy0)
    for t, k in zip(T, names):
        t.grad = g1[k].clone()
    opt.step()
    sd = opt.state_dict()
    P1 = {k: t.detach().clone() for k, t in zip(names, T)}
    T2 = [t.detach().to(dtype).clone().requires_grad_(True) for t in T]
    opt2 = torch.optim.Adam(T2, amsgrad=amsgrad, foreach=False, **hy0)
    for t2, t, k in zip(T2, T, names):
        opt2.state[t2] = {q: (v.clone() if q == "step" else v.to(dtype).clone()) for q, v in opt.state[t].items()}
        t2.grad = g2[k].to(dtype).clone()
    opt2.param_groups[0].update(edit or {})
    opt2.step()
    out = {"p": {k: t.detach() for k, t in zip(names, T2)}, "max_exp_avg_sq": None}
    for q in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if amsgrad else ()):
        out[q] = {k: opt2.state[t][q] for k, t in zip(names, T2)}
    return sd, P1, out


@pytest.mark.parametrize("path", ["param_groups", "load_state_dict"])
@pytest.mark.parametrize("kind", KINDS)
def test_param_group_edits_reach_the_device(kind, path):
    """The FusedAdams of build_decoder / build_reconstructor.  param_groups: one step with generated gradients, then
    param_groups[0]['lr'] x 100 and weight_decay = 1e-2 (an lr schedule), a second step.  load_state_dict: the state dict of a
    torch.optim.Adam saved after one step with another lr / betas / eps / weight decay (how a reference checkpoint arrives), then
    a step.  Both against a float64 torch.optim.Adam that received the same edits, at the bars of the float32 one."""
    dims = OR.RAGGED
    B, F, D, V, E, H, A, RA = dims
    shapes = (GU.decoder_shapes(V, E, H, A, D), GU.rec_shapes(kind, H, D, RA))
    P = tuple(OR.model_params(s, 11 + w) for w, s in enumerate(shapes))
    _, dec, rec = make_models(list(dims), kind, "bf16", P[0], P[1])
    for w, md in enumerate((dec, rec)):
        opt, ms = md["optimizer"], md["_state"]
        g0 = opt.param_groups[0]
        hy0 = dict(lr=g0["lr"], betas=tuple(g0["betas"]), eps=g0["eps"], weight_decay=g0["weight_decay"])
        g1, g2 = OR.make_inputs(shapes[w], 51 + w)["grad"], OR.make_inputs(shapes[w], 61 + w)["grad"]
        if path == "param_groups":
            edit = dict(lr=hy0["lr"] * 100, weight_decay=1e-2)
            saved_hy = hy0
        else:
            saved_hy = dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=1e-2)
            edit = {}
        Pw = {k: P[w][k] for k in ms.params()}      # the model's parameter order: what the ids of a state dict count
        sd, P1, r64 = _adam_two_steps(Pw, g1, g2, ms.amsgrad, saved_hy, torch.float64, edit)
        _, _, r32 = _adam_two_steps(Pw, g1, g2, ms.amsgrad, saved_hy, torch.float32, edit)
        grads = ms.flat()["grad"].views
        if path == "param_groups":
            for k, v in grads.items():
                v.copy_(g1[k])
            opt.step()
            opt.param_groups[0]["lr"] = edit["lr"]
            opt.param_groups[0]["weight_decay"] = edit["weight_decay"]
        else:
            for k, p in ms.params().items():
                p.data.copy_(P1[k])
            opt.load_state_dict(sd)
            assert ms.step == 1 and opt.param_groups[0]["betas"] == (0.8, 0.95)
        for k, v in grads.items():
            v.copy_(g2[k])
        opt.step()
        torch.cuda.synchronize()
        fl = ms.flat()
        got = {"p": {k: p.detach().cpu() for k, p in ms.params().items()}, "max_exp_avg_sq": None}
        for q in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            if q in fl:
                got[q] = {k: v.cpu() for k, v in fl[q].views.items()}
        bar, err = OR.bars(r32, r64), OR.errors(got, r64)
        print("%s %s model %d: " % (path, kind, w) + ", ".join("%s %.2e (bar %.2e)" % (q, err[q], bar[q]) for q in bar))
        assert set(err) == set(bar) and all(err[q] <= bar[q] for q in bar), (path, w, err, bar)
        assert int(float(opt.state_dict()["state"][0]["step"])) == 2
        eng = ms.engines[("opt",)]      # the engine FusedAdam.step made for itself
        assert eng.chain_status() == 0
        assert eng.images_stale() == 0


def test_amsgrad_edit_raises_and_a_live_graph_refuses_new_hyper_parameters():
    """`amsgrad` in the param group that disagrees with how the state was bound raises instead of running the other variant; a
    captured step holds the hyper-parameters as kernel arguments, so an edit while it is alive is refused."""
    dims = OR.CHAIN
    B, F, D, V, E, H, A, RA = dims
    P = (GU.formula_params(GU.decoder_shapes(V, E, H, A, D), 3), GU.formula_params(GU.rec_shapes("global", H, D, RA), 4))
    _, dec, rec = make_models(list(dims), "global", "bf16", P[0], P[1])
    step = R.DataParallelTrainStep(dec, rec, B, 0, 1, n_frames=F)
    enc, targets = GU.make_batch(B, F, D, V, [4] * B, 9)
    T, w = step.prepare(targets.numpy())
    run = R.GraphedStep(step, enc.cuda(), targets.cuda(), T, w, warmup=0)
    run()
    torch.cuda.synchronize()
    lr = dec["optimizer"].param_groups[0]["lr"]
    dec["optimizer"].param_groups[0]["lr"] = 10 * lr
    with pytest.raises(RuntimeError, match="capture again"):
        dec["optimizer"].step()
    with pytest.raises(RuntimeError, match="capture again"):
        run()                                  # a replay would step with the old lr: it refuses as well (host-side, nothing is enqueued)
    assert dec["_state"].step == 1
    dec["optimizer"].param_groups[0]["lr"] = lr
    run()                                      # the edit taken back: the captured values are the param group's again
    torch.cuda.synchronize()
    dec["optimizer"].param_groups[0]["amsgrad"] = False
    with pytest.raises(ValueError, match="amsgrad"):
        dec["optimizer"].step()
    assert step.step_impl.engine.chain_status() == 0
