"""The deferred reconstructor update of the fused step (include/recnet_hip.h: recnet_set_deferred_reconstructor_update;
api.GraphedStep(defer_reconstructor_update=True)): step n leaves the reconstructor's weight-gradient products and Adam step
pending, step n + 1 runs them on a third stream under its decoder forward chain.  train.py:272-273 steps the two optimisers
at the end of the iteration; nothing reads the reconstructor's parameters before the next iteration's reconstructor
forward (train.py:256), so the result has to be — and is held to be — BIT-IDENTICAL to the non-deferred step's once
flushed: parameters, Adam moments, losses of every step."""
import numpy as np
import pytest
import torch

import recnet_amd as R
from recnet_amd import _lib
from tests import golden_util as GU
from tests.gpu_util import make_models

pytestmark = pytest.mark.gpu

# persistent-chain shape (H % 32, R % 32) and a ragged one that takes the per-step kernels
# "row_groups": 120 captions = two row groups of 60 — the split update is not applied there (recnet_create), the step updates at once
# and defers only the refresh of the derived weight images to the next step's start (round 5: img_defer_now, csrc/api.hip)
SHAPES = {"chains": [24, 6, 64, 61, 16, 32, 16, 16], "per_step": [9, 5, 40, 61, 12, 24, 8, 8], "row_groups": [120, 6, 64, 61, 16, 32, 16, 16]}


def _state(md):
    st = md["_state"].flat()
    out = {"p." + k: v.detach().clone() for k, v in md["model"].state_dict().items()}
    for name in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if md["_state"].amsgrad else ()):      # (no third set without AMSGrad)
        for k, v in st[name].views.items():
            out[name + "." + k] = v.detach().clone()
    return out


def _atomic(name):
    """Gradients summed with float atomics (column sums, the embedding scatter): reproducible to fp32 rounding only, with or
    without deferral (tests/test_gpu_fullsize.py: the step is a pure function ... 'to fp32 rounding for the ones summed
    with atomics')."""
    return any(t in name for t in ("bias", "attn_b", "attn_w.", "embedding"))


def _same(a, b, name, exact):
    if exact and not _atomic(name):
        return torch.equal(a, b)
    return torch.allclose(a, b, rtol=2e-4, atol=2e-8)


LL, GG, LG = ("LSTM", "LSTM"), ("GRU", "GRU"), ("LSTM", "GRU")      # (decoder cell, reconstructor cell)

# the optimiser settings the reference's defaults never reach: AMSGrad on the reconstructor (the ad_vmax branch of the GEMM
# epilogue, the split update), a weight decay that matters, other betas
HYPER = dict(reconstructor_use_amsgrad=True, decoder_weight_decay=1e-2, reconstructor_weight_decay=1e-2, adam_beta1=0.8, adam_beta2=0.95)


def _preload_vmax(md, seed):
    """max_exp_avg_sq of the GEMM-produced recurrent weights spread log-uniformly over 1e-12 .. 1 instead of zero: whatever the
    scale of exp_avg_sq, some elements keep the stored maximum through every step, some take the fresh value from the first
    step on and some change sides in between — an update that wrote v in place of max(vmax, v) differs from one that did not."""
    g = torch.Generator().manual_seed(seed)
    for k, v in md["_state"].flat()["max_exp_avg_sq"].views.items():
        if k.startswith("rnn.weight_"):
            v.copy_((10.0 ** (-12.0 * torch.rand(v.shape, generator=g))).to(v.device))


def _run(kind, prec, dims, deferred, lens_sets, order, lr=None, hyper=None, epilogue=False, cells=LL):
    B, F, D, V, E, H, A, RA = dims
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D, cells[0]), 3)
    recP = GU.formula_params(GU.rec_shapes(kind, H, D, RA, cells[1]), 4)
    cfg = {} if lr is None else dict(decoder_learning_rate=lr, reconstructor_learning_rate=lr)
    cfg.update(hyper or {})
    _, dec, rec = make_models(list(dims), kind, prec, decP, recP, cells=cells, **cfg)
    step = R.DataParallelTrainStep(dec, rec, B, 0, 1, n_frames=F)
    if hyper and hyper.get("reconstructor_use_amsgrad"):
        _preload_vmax(rec, 21)
    graphs, losses = [], []
    for i, lens in enumerate(lens_sets):
        enc, targets = GU.make_batch(B, F, D, V, lens, 9 + i)
        T, w = step.prepare(targets.numpy())
        graphs.append(R.GraphedStep(step, enc.cuda(), targets.cuda(), T, w, warmup=0, defer_reconstructor_update=deferred))
        assert graphs[-1].deferred == (bool(deferred) and (kind == "global" or deferred == "recurrent"))
    for i in order:
        losses.append(graphs[i]().clone())
    graphs[0].flush()
    torch.cuda.synchronize()
    assert step.step_impl.engine.chain_status() == 0
    if epilogue:      # RECNET_DIM_SPLIT_FITS: the split update is applied at this shape, so the GEMM epilogue is what updated W_hh
        eng = step.step_impl.engine
        assert eng.lib.recnet_dim(eng.handle, _lib.DIM_SPLIT_FITS) == 1
    import os
    if not os.environ.get("RN_T_SKIP_IMAGES"):
        assert step.step_impl.engine.images_stale() == 0      # the operand images follow the parameters, whichever path updated them
    return _state(dec), _state(rec), torch.stack(losses).cpu().numpy()


@pytest.mark.parametrize("prec", ["bf16", "f32"])
@pytest.mark.parametrize("kind", ["global", "local"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("lengths", ["full", "alternating"])
@pytest.mark.parametrize("mode", [True, "recurrent"])      # whole update deferred / only the recurrent weights' (mode 2)
@pytest.mark.parametrize("lr", [None, 1e-2])
def test_deferred_update_equals_the_immediate_one_once_flushed(lr, mode, lengths, shape, kind, prec):
    _deferred_equals_immediate(lr, mode, lengths, shape, kind, prec)


@pytest.mark.parametrize("prec", ["bf16", "f32"])
@pytest.mark.parametrize("kind", ["global", "local"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("lengths", ["full", "alternating"])
@pytest.mark.parametrize("mode", [True, "recurrent"])
@pytest.mark.parametrize("lr", [None, 1e-2])
@pytest.mark.parametrize("cells", [GG, LG], ids=["GG", "LG"])
def test_deferred_update_equals_the_immediate_one_once_flushed_with_gru_cells(cells, lr, mode, lengths, shape, kind, prec):
    """The cells axis of the test above (which is its LSTM / LSTM value and keeps its ids): a GRU reconstructor behind either decoder
    cell.  The pending d W_hh is two members of the grouped launch under GRU and its fused Adam epilogue has two windows
    (csrc/host_reconstructor.inc); same matrix, same assertions."""
    _deferred_equals_immediate(lr, mode, lengths, shape, kind, prec, cells=cells)


@pytest.mark.parametrize("prec", ["bf16", "f32"])
@pytest.mark.parametrize("mode,kind", [(True, "global"), ("recurrent", "global"), ("recurrent", "local")])
def test_deferred_update_equals_the_immediate_one_at_other_hyper_parameters(mode, kind, prec):
    """The hyper-parameter axis of the test above, restricted to shape "chains", full lengths and lr 1e-2 (HYPER: AMSGrad on the
    reconstructor, weight decay 1e-2, betas 0.8 / 0.95), held to the bars that lr has there; max_exp_avg_sq is compared too.
    bf16, mode "recurrent": the update of W_hh is the Adam epilogue of its weight-gradient product (csrc/gemm_lds.hpp) with the
    stored maximum (ad_vmax).  tests/test_gpu_optimizer.py holds the immediate update to a float64 Adam; this holds the
    epilogue to the immediate update."""
    _deferred_equals_immediate(1e-2, mode, "full", "chains", kind, prec, HYPER)


def _deferred_equals_immediate(lr, mode, lengths, shape, kind, prec, hyper=None, cells=LL):
    """lr None: the reference's learning rates (1e-5 / 1e-6) — the updates are too small to feed rounding differences of the
    atomically summed gradients back into the next step, so GEMM-produced tensors can be held BIT for bit.  lr 1e-2 (at
    the defaults four steps move a weight by less than the tolerances, so a missing update would pass): every step moves every
    parameter by ~1e-2, the two schedules are compared relative to that movement, and the losses of the later steps are those of
    the updated weights."""
    if kind == "local" and mode is True:
        pytest.skip("the whole-update mode exists for the global reconstructor")
    dims = SHAPES[shape]
    B = dims[0]
    rs = np.random.RandomState(1)
    if lengths == "full":
        # T = caption_max_len + 1 in every step: the deferred products have the shapes of the immediate ones, so every
        # GEMM-produced gradient — and with it every parameter and Adam moment it feeds — is BIT-identical
        sets = [[30] + [int(x) for x in rs.randint(1, 30, size=B - 1)]]
        order = [0, 0, 0, 0]
    else:
        # two caption-length sets with DIFFERENT decode lengths T, replayed alternately: the deferred products of one graph
        # run on the gate gradients the OTHER graph's step left.  The global reconstructor's deferred products always cover
        # caption_max_len + 1 steps (zero gate gradients beyond T): another split of K, so equal to fp32 rounding
        sets = [[int(x) for x in rs.randint(1, 6, size=B)], [int(x) for x in rs.randint(3, 12, size=B)]]
        order = [0, 1, 1, 0, 1, 0]
    # (mode "recurrent": the in-step half is a different grouped launch than the immediate update's — other split factors,
    # equal to fp32 rounding)
    exact = lengths == "full" and mode is True
    d0, r0, l0 = _run(kind, prec, dims, False, sets, order, lr, hyper, cells=cells)
    d1, r1, l1 = _run(kind, prec, dims, mode, sets, order, lr, hyper,
                      epilogue=hyper is not None and prec == "bf16" and mode == "recurrent" and shape == "chains", cells=cells)
    if hyper and hyper.get("reconstructor_use_amsgrad"):
        # the stored maximum is the larger operand for some elements of W_hh and the smaller for others, after the last step too
        v, vmax = r1["exp_avg_sq.rnn.weight_hh_l0"], r1["max_exp_avg_sq.rnn.weight_hh_l0"]
        kept, fresh = int((vmax > v).sum()), int((vmax == v).sum())
        assert kept + fresh == v.numel() and kept > v.numel() // 20 and fresh > v.numel() // 20, (kept, fresh, v.numel())
    recP = GU.formula_params(GU.rec_shapes(kind, dims[5], dims[2], dims[7], cells[1]), 4)
    if lr is None:
        assert np.allclose(l0[:, :7], l1[:, :7], rtol=1e-6 if mode is True else 3e-6, atol=0), (l0[:, 6], l1[:, 6])
        for k in d0:
            # (the decoder sees the reconstructor's parameters through d loss / d hiddens: bit-identical only where they are)
            # (B = 120 on the fp32 path: the per-step backward sums d Uv over frame chunks with float atomics — reproducible to rounding)
            assert _same(d0[k], d1[k], k, shape != "row_groups"), ("decoder", k, float((d0[k] - d1[k]).abs().max()))
        for k in r0:
            # (row groups: the reconstructor reads the decoder's states, which are reproducible to rounding only there — see above)
            assert _same(r0[k], r1[k], k, exact and shape != "row_groups"), ("reconstructor", k, float((r0[k] - r1[k]).abs().max()))
        assert any(not torch.equal(r1["p." + k].cpu(), v) for k, v in recP.items())
        return
    # large updates: rounding differences of the atomically summed gradients (biases, embedding rows) are fed back through the
    # parameters, so nothing stays bit-identical over four steps; the schedules agree to a small fraction of how far each tensor moved
    assert np.allclose(l0[:, :7], l1[:, :7], rtol=2e-5, atol=0), (l0[:, 6], l1[:, 6])
    decP = GU.formula_params(GU.decoder_shapes(dims[3], dims[4], dims[5], dims[6], dims[2], cells[0]), 3)
    for st0, st1, P in ((d0, d1, decP), (r0, r1, recP)):
        for k, v in P.items():
            a, b = st0["p." + k].cpu().double(), st1["p." + k].cpu().double()
            moved = float((b - v.double()).norm())
            assert moved > 3e-3 * np.sqrt(v.numel()), (k, moved)            # every update happened: a sizeable fraction of lr per element and step
            assert float((a - b).norm()) <= 2e-3 * moved, (k, float((a - b).norm()), moved)
            for name in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if "max_exp_avg_sq." + k in st1 else ()):
                a, b = st0[name + "." + k].cpu().double(), st1[name + "." + k].cpu().double()
                assert float((a - b).norm()) <= 2e-3 * float(b.norm()), (name, k)
    if lengths == "full":      # the same batch four times: the loss falls by far more than the bar above
        assert abs(l1[-1, 6] - l1[0, 6]) > 1e-3 * abs(l1[0, 6]), l1[:, 6]


def test_without_flush_the_last_update_is_pending_and_entry_points_flush_themselves():
    dims = SHAPES["chains"]
    B, F, D, V, E, H, A, RA = dims
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D), 3)
    recP = GU.formula_params(GU.rec_shapes("global", H, D, RA), 4)
    enc, targets = GU.make_batch(B, F, D, V, [3] * B, 9)

    def build(deferred):
        _, dec, rec = make_models(list(dims), "global", "bf16", decP, recP)
        step = R.DataParallelTrainStep(dec, rec, B, 0, 1, n_frames=F)
        T, w = step.prepare(targets.numpy())
        return dec, rec, step, R.GraphedStep(step, enc.cuda(), targets.cuda(), T, w, warmup=0, defer_reconstructor_update=deferred), T, w

    dec0, rec0, step0, g0, T, w = build(False)
    dec1, rec1, step1, g1, _, _ = build(True)
    for _ in range(3):
        g0(); g1()
    torch.cuda.synchronize()
    w0 = rec0["model"].state_dict()["rnn.weight_hh_l0"]
    w1 = rec1["model"].state_dict()["rnn.weight_hh_l0"]
    assert not torch.equal(w0, w1), "the third update should still be pending"
    # an eager step through the ordinary entry points (fwd_bwd + optimizer_step) completes the pending update first
    step0(enc.cuda(), targets.cuda(), T, w)
    step1(enc.cuda(), targets.cuda(), T, w)
    torch.cuda.synchronize()
    for k, v in rec0["model"].state_dict().items():
        assert _same(v, rec1["model"].state_dict()[k], k, True), k
    for k, v in dec0["model"].state_dict().items():
        assert _same(v, dec1["model"].state_dict()[k], k, True), k


def test_local_reconstructor_keeps_the_immediate_update():
    """The deferred form is implemented for the global reconstructor only; asking for it with the local one is ignored."""
    dims = SHAPES["chains"]
    a = _run("local", "bf16", dims, False, [[4] * dims[0]], [0, 0])
    b = _run("local", "bf16", dims, True, [[4] * dims[0]], [0, 0])
    for k in a[1]:
        assert _same(a[1][k], b[1][k], k, True), k


@pytest.mark.parametrize("kind", ["global", "local"])
def test_split_update_runs_beside_the_decoder_chain_in_the_replayed_graph(kind):
    """Mode 2 is only worth having if the replayed graph really runs the pending W_hh update BESIDE the next step's decoder
    forward chain.  Round 4 lost that once without any test noticing (a change of the graph's cross-stream edges made the runtime
    run it BEHIND the chain at the local reconstructor's benchmark shape: 2.27 against 2.15 ms).  The kernels' own stamps of a
    replayed step (Engine.read_stamps, no tracer) say where it ran: it has to start before the chain is a third through."""
    B, F, D, V = 100, 28, 1536, 4188
    dims = [B, F, D, V, 468, 512, 128, 128]
    decP = GU.formula_params(GU.decoder_shapes(V, 468, 512, 128, D), 3)
    recP = GU.formula_params(GU.rec_shapes(kind, 512, D, 128), 4)
    _, dec, rec = make_models(dims, kind, "bf16", decP, recP)
    step = R.DataParallelTrainStep(dec, rec, B, 0, 1, n_frames=F)
    enc, targets = GU.make_batch(B, F, D, V, [30] * B, 11)
    T, w = step.prepare(targets.numpy())
    run = R.GraphedStep(step, enc.cuda(), targets.cuda(), T, w, warmup=2, defer_reconstructor_update="recurrent")
    eng = step.step_impl.engine
    assert eng.lib.recnet_dim(eng.handle, _lib.DIM_SPLIT_FITS) == 1, "the split update is applied at the benchmark shapes"
    beside = 0
    for _ in range(6):
        run()
        st = eng.read_stamps()
        c0, c1 = st["chains"]["decoder_forward"]
        p0, p1 = st["groups"]["pending_recurrent_update"]
        beside += p0 < c0 + (c1 - c0) / 3
    run.flush()
    assert eng.chain_status() == 0
    assert beside >= 5, "the pending update ran behind the decoder's forward chain instead of beside it"
