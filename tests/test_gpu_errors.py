"""Error behaviour of the boundary on a GPU box: the library reports misuse through return codes (surfaced as
RecNetError with recnet_last_error()'s text), the Python mirror raises like the reference does — nothing falls back
silently to another path."""
import numpy as np
import pytest
import torch

import recnet_amd as R
from recnet_amd import _lib
from recnet_amd.engine import Engine
from tests import golden_util as GU
from tests.gpu_util import make_models

pytestmark = pytest.mark.gpu

DIMS = [4, 5, 40, 37, 10, 24, 16, 16]


def _models(kind="global"):
    B, F, D, V, E, H, A, RA = DIMS
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D), 1)
    recP = GU.formula_params(GU.rec_shapes(kind, H, D, RA), 2)
    return make_models(DIMS, kind, "f32", decP, recP)


def test_wrong_shapes_devices_and_dtypes_are_rejected():
    C, dec, rec = _models()
    step = R.TrainStep(dec, rec)
    enc, tg = GU.make_batch(4, 5, 40, 37, [3, 1, 4, 2], 3)
    T, w = step.prepare(tg.numpy())
    with pytest.raises(RuntimeError):                       # CPU tensor: there is no CPU path
        step(enc, tg.cuda(), T, w)
    with pytest.raises(RuntimeError):                       # wrong batch size
        step(enc[:3].cuda(), tg.cuda(), T, w)
    with pytest.raises(RuntimeError):                       # targets must be int64 [31, B]
        step(enc.cuda(), tg.cuda().int(), T, w)
    with pytest.raises(RuntimeError):
        step(enc.cuda(), tg[:10].cuda(), T, w)


def test_library_return_codes():
    C, dec, rec = _models()
    step = R.TrainStep(dec, rec)
    eng = step.engine
    enc, tg = GU.make_batch(4, 5, 40, 37, [3, 1, 4, 2], 3)
    encd, tgd = enc.cuda(), tg.cuda()
    T, w = step.prepare(tg.numpy())
    with pytest.raises(_lib.RecNetError, match="T out of range"):
        eng.train_step_fwd_bwd(encd, tgd, 32, torch.ones(32, device="cuda"), 1)
    with pytest.raises(_lib.RecNetError, match="before forward"):
        eng.backward_decoder(encd, tgd, None, 1.0)
    with pytest.raises(_lib.RecNetError, match="beam_width"):
        eng.beam_search(encd, 9)
    # a handle without a reconstructor refuses reconstructor calls
    e2 = Engine(dict(B=4, F=5, D=40, E=10, H=24, A=16, V=37), None, "f32")
    with pytest.raises(_lib.RecNetError):
        e2.forward_reconstructor(encd, None, T)
    # and an unbound handle refuses to run
    with pytest.raises(_lib.RecNetError, match="not bound"):
        e2.train_step_fwd_bwd(encd, tgd, T, w, 1)


def test_config_validation():
    with pytest.raises(_lib.RecNetError, match="reconstructor_hidden_size == encoder_output_size"):
        Engine(dict(B=2, F=2, D=8, E=4, H=8, A=4, V=8, R=16, RA=4), "local", "bf16")
    with pytest.raises(_lib.RecNetError, match="non-positive"):
        Engine(dict(B=0, F=2, D=8, E=4, H=8, A=4, V=8), None, "bf16")
    with pytest.raises(KeyError):
        Engine(dict(B=2, F=2, D=8, E=4, H=8, A=4, V=8, dec_cell="RNN"), None, "bf16")


# ---- an abandoned step leaves nothing behind (recnet_abort_step)
CHAIN_DIMS = [24, 6, 64, 61, 16, 32, 16, 16]      # the persistent-chain shape of tests/test_gpu_knobs.py
CHAIN_LR = 1e-2


def _chain_step(kind):
    B, F, D, V, E, H, A, RA = CHAIN_DIMS
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D), 3)
    recP = GU.formula_params(GU.rec_shapes(kind, H, D, RA), 4)
    _, dec, rec = make_models(list(CHAIN_DIMS), kind, "bf16", decP, recP, decoder_learning_rate=CHAIN_LR,
                              reconstructor_learning_rate=CHAIN_LR)
    return R.TrainStep(dec, rec), dec, rec, decP, recP


def _params(dec, rec, decP, recP):
    out = {}
    for name, md, P in (("dec", dec, decP), ("rec", rec, recP)):
        for k, v in md["model"].state_dict().items():
            out[name + "." + k] = (v.detach().double().cpu(), P[k].double())
    return out


@pytest.mark.parametrize("kind", ["global", "local"])
def test_abort_step_after_part_one_leaves_no_trace(kind):
    """Part 1 of a data-parallel step with the side stream left open (recnet_set_dp_overlap), abandoned with recnet_abort_step: the
    fused step that follows computes what it computes on a fresh handle — the same schedule state, so the same arithmetic (the bars
    are those of tests/test_gpu_knobs.py, which compares two schedules of one arithmetic)."""
    B, F, D, V = CHAIN_DIMS[:4]
    rs = np.random.RandomState(2)
    enc, targets = GU.make_batch(B, F, D, V, [30] + [int(x) for x in rs.randint(1, 30, size=B - 1)], 11)
    encd, tgd = enc.cuda(), targets.cuda()
    res = []
    for abandoned in (True, False):
        step, dec, rec, decP, recP = _chain_step(kind)
        eng = step.engine
        T, w = step.prepare(targets.numpy())
        if abandoned:
            eng.set_dp_overlap(True)
            eng.train_step_part_dev(1, encd, tgd, T, w, 7)
            torch.cuda.synchronize()
            eng.abort_step()
        eng.train_step(encd, tgd, T, w, seed=5, step=1)
        torch.cuda.synchronize()
        assert eng.chain_status() == 0
        res.append((_params(dec, rec, decP, recP), eng.scalars.cpu().numpy()[:7].copy()))
    (pa, la), (pb, lb) = res
    print("losses after abort:", la, "fresh:", lb)
    assert np.allclose(la, lb, rtol=1e-4, atol=0), (la, lb)
    for k in pa:
        (a, init), (b, _) = pa[k], pb[k]
        moved = float((a - init).norm())
        diff = float((a - b).norm())
        print(k, "moved", moved, "diff", diff)
        assert moved > 3e-3 * np.sqrt(a.numel()), (k, moved)
        assert diff <= 2e-3 * moved, (k, diff, moved)
