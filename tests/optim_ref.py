"""The end of a train step (train.py:269-273) for ONE model, restated with torch on the CPU in a chosen dtype: the
regulariser's gradient, torch.nn.utils.clip_grad_norm_, one torch.optim.Adam.step() on preloaded state.  Run in float64 it
is the reference of tests/test_gpu_optimizer.py; run in float32 it is the error scale of that reference, from which the bars
are built (bars()).  Also here, because the CPU suite (tests/test_optim_ref.py) and the GPU suite share them: the generated
inputs and the case matrix.  Nothing in this module touches a GPU."""
import math

import numpy as np
import torch

from tests import golden_util as GU

EPS32 = 2.0 ** -23
BAR_FACTOR = 8.0      # a correct fp32 kernel may differ from torch's own fp32 by a few roundings per element (FMA contraction,
#                       another summation order of the norms): eight times the fp32 run's own error, see bars()

# the shapes: [B, F, D, V, E, H, A, RA]
RAGGED = [7, 5, 88, 101, 18, 36, 20, 12]      # tests/test_gpu_parity.py: test_packed_images_follow_update_at_ragged_shapes
CHAIN = [24, 6, 64, 61, 16, 32, 16, 16]       # tests/test_gpu_deferred.py: SHAPES["chains"]

# hyper-parameters where they matter (the defaults — lr 1e-5, weight decay 1e-5, betas 0.9 / 0.999, eps 1e-8 — hide a wrong formula)
HYPER = dict(lr=1e-2, weight_decay=1e-2, betas=(0.8, 0.95), eps=1e-6)
CLIP = 50.0
OPT_REG, OPT_CLIP, OPT_SKIP_DECODER, OPT_SKIP_RECONSTRUCTOR = 1, 2, 4, 8


def adam_stage(params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq=None, *, lam=0.0, max_norm=0.0, lr, betas, eps, weight_decay,
               amsgrad, step, dtype=torch.float64):
    """params / grads / moments: {name: tensor}, taken as given (cast to `dtype`).  lam: the coefficient of sum_p ||p||_2 in the
    loss (lambda_reg, times lambda_recon for the reconstructor), 0: no regulariser; max_norm: clip_grad_norm_'s, 0: no clipping;
    step: the number of the Adam step taken (state['step'] is preloaded with step - 1).
    Returns {"p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq" (None without amsgrad): {name: tensor of dtype}, "total_norm": the
    norm of g + regulariser gradient over all tensors, before clipping}."""
    names = list(params)
    P = [params[k].detach().to(dtype).clone().requires_grad_(True) for k in names]
    for p, k in zip(P, names):
        p.grad = grads[k].detach().to(dtype).clone()
    if lam:
        # train.py:69-70 / 103-104 / 129-130: loss += lambda * sum_p ||p||; torch.norm's backward gives zero for a tensor of zeros
        (lam * sum(p.norm() for p in P)).backward()
    total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in P]))
    if max_norm:
        torch.nn.utils.clip_grad_norm_(P, max_norm)      # train.py:270
    opt = torch.optim.Adam(P, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, foreach=False)
    for p, k in zip(P, names):
        st = {"step": torch.tensor(float(step - 1)), "exp_avg": exp_avg[k].detach().to(dtype).clone(),
              "exp_avg_sq": exp_avg_sq[k].detach().to(dtype).clone()}
        if amsgrad:
            st["max_exp_avg_sq"] = max_exp_avg_sq[k].detach().to(dtype).clone()
        opt.state[p] = st
    opt.step()                                            # train.py:271-273
    out = {"p": {k: p.detach() for k, p in zip(names, P)}, "total_norm": float(total.double()),
           "grad": {k: p.grad.detach() for k, p in zip(names, P)}}
    for q in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
        out[q] = {k: opt.state[p][q] for k, p in zip(names, P)} if (amsgrad or q != "max_exp_avg_sq") else None
    return out


def clip_ref(grads, max_norm, dtype=torch.float64):
    """torch.nn.utils.clip_grad_norm_ on {name: gradient}: (total norm, {name: clipped gradient})."""
    P = [torch.zeros_like(g, dtype=dtype).requires_grad_(True) for g in grads.values()]
    for p, g in zip(P, grads.values()):
        p.grad = g.detach().to(dtype).clone()
    total = torch.nn.utils.clip_grad_norm_(P, max_norm)
    return float(total.double()), {k: p.grad for k, p in zip(grads, P)}


# ------------------------------------------------------------------------------------------- inputs
def zero_key(shapes):
    """The tensor that is all zeros in parameters, gradient and state: attn_b (the global reconstructor has none: out.bias)."""
    return "attn_b" if "attn_b" in shapes else "out.bias"


def model_params(shapes, seed):
    P = GU.formula_params(shapes, seed)
    P[zero_key(shapes)] = torch.zeros(shapes[zero_key(shapes)])
    return P


def make_inputs(shapes, seed, gscale=3.0, mscale=0.1, vmax=0.01):
    """Generated on the CPU from a seed: gradients N(0,1) * gscale, exp_avg N(0,1) * mscale, exp_avg_sq and max_exp_avg_sq
    uniform in [0, vmax] and independent (about half of the elements on each side of AMSGrad's max), a few exact zeros in each
    (at positions of their own), and the zero_key tensor all zeros.  Returns {"grad", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}."""
    g = torch.Generator().manual_seed(int(seed))
    out = {q: {} for q in ("grad", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")}
    zk = zero_key(shapes)
    for k in sorted(shapes):
        shp = tuple(shapes[k])
        n = int(np.prod(shp))
        t = {"grad": torch.randn(shp, generator=g) * gscale, "exp_avg": torch.randn(shp, generator=g) * mscale,
             "exp_avg_sq": torch.rand(shp, generator=g) * vmax, "max_exp_avg_sq": torch.rand(shp, generator=g) * vmax}
        for q, x in t.items():
            nz = min(3, max(1, n // 8))
            x.view(-1)[torch.randperm(n, generator=g)[:nz]] = 0.0
            if k == zk:
                x.zero_()
            out[q][k] = x
    return out


def reg_grad(params, lam):
    """{name: lam * p / ||p||} in float64 (zero for a tensor of zeros)."""
    out = {}
    for k, p in params.items():
        p = p.double()
        n = float(p.norm())
        out[k] = lam * p / n if n > 0 else torch.zeros_like(p)
    return out


def rescale_grads(grads, params, lam, target):
    """The gradients times the s > 0 for which || s * g + regulariser gradient || = target in float64 (then rounded to fp32:
    a relative 1e-8 of the norm)."""
    r = reg_grad(params, lam)
    gg = sum(float((g.double() ** 2).sum()) for g in grads.values())
    gr = sum(float((grads[k].double() * r[k]).sum()) for k in grads)
    rr = sum(float((x ** 2).sum()) for x in r.values())
    s = (-gr + math.sqrt(gr * gr - gg * (rr - target * target))) / gg
    return {k: (g.double() * s).float() for k, g in grads.items()}


# ------------------------------------------------------------------------------------------- cases
# Engine-level settings (what a handle is created with); every one also carries HYPER.
#   amsgrad: (decoder, reconstructor); clip: gradient_clip; use_clip: use_gradient_clip; lam: (decoder_lambda_reg,
#   reconstructor_lambda_reg, lambda_recon)
DEFAULT_LAM = (1e-3, 1e-2, 1.0)
CONFIGS = {
    "base": dict(amsgrad=(True, False), clip=CLIP, use_clip=True, lam=DEFAULT_LAM),
    "ams_swapped": dict(amsgrad=(False, True), clip=CLIP, use_clip=True, lam=DEFAULT_LAM),
    "ams_both": dict(amsgrad=(True, True), clip=CLIP, use_clip=True, lam=DEFAULT_LAM),
    "ams_none": dict(amsgrad=(False, False), clip=CLIP, use_clip=True, lam=DEFAULT_LAM),
    "clip_zero": dict(amsgrad=(True, False), clip=0.0, use_clip=True, lam=DEFAULT_LAM),
    "clip_unused": dict(amsgrad=(True, False), clip=CLIP, use_clip=False, lam=DEFAULT_LAM),
    "lambdas": dict(amsgrad=(True, True), clip=CLIP, use_clip=True, lam=(0.5, 0.25, 0.5)),
}
# One optimiser stage each.  flags: recnet_optimizer_step's; norm: None = the generated gradients as they are (about 10 x CLIP),
# else the decoder's gradients rescaled so that || g + reg || = norm * CLIP; reg_first: add_reg_grad, then a step without OPT_REG;
# quiet: gradients and moments 1e-3 as large (eps matters next to sqrt(v)); seed: of make_inputs.
_RC = OPT_REG | OPT_CLIP
CASES = {
    "clip_step1": dict(config="base", step=1, flags=_RC),
    "clip_step2": dict(config="base", step=2, flags=_RC),
    "clip_step1000": dict(config="base", step=1000, flags=_RC),
    "clip_step100000": dict(config="base", step=100000, flags=_RC),
    "edge_below": dict(config="base", step=2, flags=_RC, norm=1.0 - 1e-3),
    "edge_above": dict(config="base", step=2, flags=_RC, norm=1.0 + 1e-3),
    "quiet": dict(config="base", step=1000, flags=_RC, quiet=True),
    "flags_without_clip": dict(config="base", step=2, flags=OPT_REG),
    "clip_zero": dict(config="clip_zero", step=2, flags=_RC),
    "clip_unused": dict(config="clip_unused", step=2, flags=_RC),
    "ams_swapped": dict(config="ams_swapped", step=2, flags=_RC),
    "ams_swapped_late": dict(config="ams_swapped", step=100000, flags=_RC),
    "ams_both": dict(config="ams_both", step=1000, flags=_RC),
    "ams_none": dict(config="ams_none", step=2, flags=_RC),
    "reg_first": dict(config="base", step=2, flags=OPT_CLIP, reg_first=True),
    "lambdas": dict(config="lambdas", step=2, flags=_RC),
    "lambdas_reg_first": dict(config="lambdas", step=1000, flags=OPT_CLIP, reg_first=True),
    "skip_decoder": dict(config="base", step=2, flags=_RC | OPT_SKIP_DECODER),
    "skip_reconstructor": dict(config="base", step=2, flags=_RC | OPT_SKIP_RECONSTRUCTOR),
}


def case_inputs(case, shapes, params, which, seed=31):
    """The generated inputs of one model (which: 0 decoder, 1 reconstructor) for a case, and the reference's arguments:
    (inputs, kwargs of adam_stage without dtype).  Clipping acts on the decoder only (train.py:270)."""
    c = dict(CASES[case]) if isinstance(case, str) else dict(case)
    cfg = CONFIGS[c["config"]]
    q = 1e-3 if c.get("quiet") else 1.0
    inp = make_inputs(shapes, seed + which, gscale=3.0 * q, mscale=0.1 * q, vmax=0.01 * q * q)
    lam_d, lam_r, lam_recon = cfg["lam"]
    lam = lam_d if which == 0 else lam_r * lam_recon
    regd = bool(c["flags"] & OPT_REG) or bool(c.get("reg_first"))
    clip_on = which == 0 and bool(c["flags"] & OPT_CLIP) and cfg["use_clip"] and cfg["clip"] > 0
    if c.get("norm") is not None and which == 0:
        inp["grad"] = rescale_grads(inp["grad"], params, lam if regd else 0.0, c["norm"] * cfg["clip"])
    kw = dict(lam=lam if regd else 0.0, max_norm=cfg["clip"] if clip_on else 0.0, amsgrad=cfg["amsgrad"][which], step=c["step"], **HYPER)
    return inp, kw


def run_ref(params, inp, kw, dtype):
    return adam_stage(params, inp["grad"], inp["exp_avg"], inp["exp_avg_sq"], inp["max_exp_avg_sq"] if kw["amsgrad"] else None,
                      dtype=dtype, **kw)


# ------------------------------------------------------------------------------------------- errors and bars
QUANTITIES = ("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq", "total_norm")


def errors(got, ref):
    """Worst error per compared quantity of `got` against `ref` (results of adam_stage, or the device's in the same layout):
    parameters: maximum absolute difference over all tensors; moments: the largest per-tensor ||got - ref|| / ||ref|| (a tensor
    whose reference is all zeros counts as 0 if it is exactly zero, else inf); total norm: relative."""
    e = {}
    for q in QUANTITIES:
        if ref.get(q) is None or got.get(q) is None:
            continue
        if q == "total_norm":
            e[q] = abs(got[q] - ref[q]) / ref[q]
            continue
        w = 0.0
        for k, r in ref[q].items():
            a, r = got[q][k].detach().cpu().double(), r.detach().cpu().double()
            if not bool(torch.isfinite(a).all()):
                w = float("inf")
            elif q == "p":
                w = max(w, float((a - r).abs().max()))
            else:
                n = float(r.norm())
                w = max(w, float((a - r).norm()) / n if n > 0 else (0.0 if not bool(a.any()) else float("inf")))
        e[q] = w
    return e


def bars(ref32, ref64):
    """The bar of every quantity: BAR_FACTOR times the float32 run's error against the float64 run on the same inputs, and at
    least one fp32 ulp of the largest magnitude (parameters: of the largest |p|; moments: of the largest element, relative to
    the tensor's norm — the smallest such ratio over the tensors; total norm: 2^-23)."""
    e = errors(ref32, ref64)
    b = {}
    for q, v in e.items():
        if q == "total_norm":
            floor = EPS32
        elif q == "p":
            floor = EPS32 * max(float(r.abs().max()) for r in ref64[q].values())
        else:
            floor = min(EPS32 * float(r.abs().max()) / float(r.norm()) for r in ref64[q].values() if float(r.norm()) > 0)
        b[q] = max(BAR_FACTOR * v, floor)
    return b
