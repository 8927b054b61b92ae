"""CPU checks of the optimiser reference (tests/optim_ref.py) that tests/test_gpu_optimizer.py holds the HIP stage to.

1. The float32 run of the reference stays within the bars against its float64 run, for every case of the matrix (the bars are
   built from that run: this guards the helper, bars() and errors()).
2. The bars can see a wrong formula without a GPU: a float64 restatement of the update with ONE mistake built in — each of the
   mistakes the product's kernels could make unnoticed by the whole-step parity tests — exceeds the bar in at least one compared
   quantity, in at least one case.  Without a mistake the restatement agrees with torch.optim.Adam to float64 rounding."""
import pytest
import torch

from tests import golden_util as GU
from tests import optim_ref as OR

MUTATIONS = ("eps_inside_sqrt", "bc2_omitted", "decay_before_clip", "clip_not_on_regulariser", "amsgrad_max_dropped",
             "clip_without_clamp")


def _models(dims=OR.RAGGED, kind="local"):
    B, F, D, V, E, H, A, RA = dims
    return ((0, GU.decoder_shapes(V, E, H, A, D)), (1, GU.rec_shapes(kind, H, D, RA)))


_CACHE = {}


def _refs(case, which, shapes):
    """(params, inputs, kwargs, float64 result, bars) of one model of one case; computed once."""
    key = (case, which)
    if key not in _CACHE:
        P = OR.model_params(shapes, 11 + which)
        inp, kw = OR.case_inputs(case, shapes, P, which)
        r64, r32 = OR.run_ref(P, inp, kw, torch.float64), OR.run_ref(P, inp, kw, torch.float32)
        _CACHE[key] = (P, inp, kw, r64, r32, OR.bars(r32, r64))
    return _CACHE[key]


def restated(P, inp, kw, mutation=None):
    """The stage in float64, written out (the formula of csrc/common.hpp: rn_adam_update), with one optional mistake."""
    b1, b2 = kw["betas"]
    lr, eps, wd, n = kw["lr"], kw["eps"], kw["weight_decay"], kw["step"]
    reg = OR.reg_grad(P, kw["lam"])
    g = {k: inp["grad"][k].double() for k in P}
    total = float(torch.sqrt(sum(((g[k] + reg[k]) ** 2).sum() for k in P)))
    cl = 1.0
    if kw["max_norm"]:
        cl = kw["max_norm"] / (total + 1e-6)
        if mutation != "clip_without_clamp":
            cl = min(cl, 1.0)
    bc1, bc2 = 1.0 - b1 ** n, 1.0 - b2 ** n
    out = {"p": {}, "exp_avg": {}, "exp_avg_sq": {}, "max_exp_avg_sq": {} if kw["amsgrad"] else None, "total_norm": total}
    for k in P:
        p = P[k].double()
        if mutation == "decay_before_clip":
            gp = (g[k] + reg[k] + wd * p) * cl
        elif mutation == "clip_not_on_regulariser":
            gp = g[k] * cl + reg[k] + wd * p
        else:
            gp = (g[k] + reg[k]) * cl + wd * p
        m = inp["exp_avg"][k].double() * b1 + (1 - b1) * gp
        v = inp["exp_avg_sq"][k].double() * b2 + (1 - b2) * gp * gp
        vh = v
        if kw["amsgrad"]:
            vmx = inp["max_exp_avg_sq"][k].double()
            vh = v if mutation == "amsgrad_max_dropped" else torch.maximum(vmx, v)
            out["max_exp_avg_sq"][k] = vh
        c2 = 1.0 if mutation == "bc2_omitted" else bc2
        denom = torch.sqrt(vh / c2 + eps) if mutation == "eps_inside_sqrt" else torch.sqrt(vh) / c2 ** 0.5 + eps
        out["p"][k] = p - (lr / bc1) * m / denom
        out["exp_avg"][k], out["exp_avg_sq"][k] = m, v
    return out


@pytest.mark.parametrize("case", list(OR.CASES))
def test_float32_run_is_within_the_bars_and_the_restatement_is_the_reference(case):
    for which, shapes in _models():
        P, inp, kw, r64, r32, bar = _refs(case, which, shapes)
        err = OR.errors(r32, r64)
        assert set(err) == set(bar) and all(err[q] <= bar[q] for q in bar), (case, which, err, bar)
        assert ("max_exp_avg_sq" in bar) == kw["amsgrad"]
        # the fp32 run's error is fp32 rounding: nothing here is looser than a few 1e-6
        assert bar["p"] < 2e-5 and all(bar[q] < 1e-5 for q in bar if q != "p"), (case, which, bar)
        # the hand-written formula without a mistake is torch's, to float64 rounding
        e0 = OR.errors(restated(P, inp, kw), r64)
        assert all(v <= 1e-12 for v in e0.values()), (case, which, e0)
        # the all-zero tensor gets the reference's value, which is zero
        zk = OR.zero_key(shapes)
        assert not bool(r64["p"][zk].any()) and not bool(r64["exp_avg_sq"][zk].any())


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_every_mistake_exceeds_the_bars_in_some_case(mutation):
    seen = []
    for case in OR.CASES:
        for which, shapes in _models():
            P, inp, kw, r64, _, bar = _refs(case, which, shapes)
            err = OR.errors(restated(P, inp, kw, mutation), r64)
            seen += [(case, which, q, err[q] / bar[q]) for q in bar if err[q] > bar[q]]
    print(mutation, "caught in", len(seen), "(case, model, quantity); worst ratio to the bar %.3g" % max([s[3] for s in seen] or [0]))
    assert seen, "no case of the matrix tells %s from the reference: the inputs are too tame" % mutation
    assert max(s[3] for s in seen) >= 10, (mutation, "only marginally above the bar", seen)


def test_case_inputs_are_what_the_cases_need():
    """About 10 x the clip bar with the generated gradients; the edge cases 1e-3 to either side of it; half of the elements on
    either side of AMSGrad's max; the regulariser's share of the gradient is what the rescaling accounts for."""
    (_, dsh), _ = _models()
    P, inp, kw, r64, _, _ = _refs("clip_step2", 0, dsh)
    assert 8 * OR.CLIP < r64["total_norm"] < 12 * OR.CLIP, r64["total_norm"]
    for case, side in (("edge_below", -1), ("edge_above", 1)):
        r = _refs(case, 0, dsh)[3]
        assert abs(r["total_norm"] / OR.CLIP - (1 + side * 1e-3)) < 1e-6, (case, r["total_norm"])
    v, vm = torch.cat([x.flatten() for x in r64["exp_avg_sq"].values()]), torch.cat([x.flatten() for x in inp["max_exp_avg_sq"].values()])
    frac = float((vm.double() > v).double().mean())
    assert 0.2 < frac < 0.8, frac
    for q in ("grad", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
        assert all(int((x == 0).sum()) >= 1 for x in inp[q].values()), q
        assert not bool(inp[q][OR.zero_key(dsh)].any())
