"""The per-caption reconstruction error on the device (recnet_reconstruction_error, Engine.reconstruction_error,
search.reconstruction_errors, best_of_n's reconstruction term) against the float64 restatement (tests/recon_ref.py), the
reference's own MSE term on the eval goldens, and the rec_mse that recnet_forward_reconstructor(train = 0) exports.

Bar of one err[b] (tests/recon_ref.py: err_bar): every reconstructed value within the project's output bar tau = TOL[prec]["hid"]
moves a mean of squares e by at most 2 tau sqrt(e) + tau^2; the global error is that mean / T.  Two device paths compared with each
other get twice that.  Every test prints its worst error / bar; the ratios of one MI355X run are in DESIGN.md section 10."""
import functools

import numpy as np
import pytest
import torch

import recnet_amd as R
from recnet_amd import _ops
from recnet_amd.engine import Engine, _lib, _ptr, _stream      # the engine's own _lib: the module whose RecNetError it raises
from tests import golden_util as GU
from tests import recon_ref as RR
from tests import sample_ref as SR
from tests import score_ref as SC
from tests.gpu_util import TOL, load_case, make_models, rel_err

pytestmark = pytest.mark.gpu


def _step(dims, kind, prec, decP, recP, cells=("LSTM", "LSTM")):
    """(config, decoder dict, reconstructor dict, TrainStep) — the step's engine has both models bound."""
    Cfg, dec, rec = make_models(list(dims), kind, prec, decP, recP, cells=cells)
    return Cfg, dec, rec, R.TrainStep(dec, rec)


def _worst(err, ref, prec, kind, T, factor=1.0):
    """(worst |err - ref| / bar, ok) for per-caption errors against restated ones."""
    bar = factor * RR.err_bar(prec, kind, ref, T)
    d = np.abs(np.asarray(err, dtype=np.float64) - ref)
    return float((d / bar).max()), bool((d <= bar).all())


@functools.lru_cache(maxsize=None)
def _golden(name):
    """The golden's batch with the restatement on its own hidden states and on those of the teacher-forced eval pass over
    targets[:T]."""
    g, dims, kind, decP, recP, enc, targets = load_case(name)
    cells = g["_cells"]
    T = g["hiddens"].shape[0]
    err_h, recon_h = RR.per_caption_error(recP, kind, g["hiddens"], enc, cell=cells[1])
    caps = targets[:T].contiguous()
    hid_t = RR.decoder_hiddens(decP, enc, caps.numpy(), cell=cells[0])
    err_t, recon_t = RR.per_caption_error(recP, kind, hid_t, enc, cell=cells[1])
    return dict(g=g, dims=dims, kind=kind, decP=decP, recP=recP, enc=enc, targets=targets, cells=cells, T=T, caps=caps,
                err_h=err_h, recon_h=recon_h, err_t=err_t, recon_t=recon_t)


# ------------------------------------------------------------------------------------------------ 1. fp32, hidden states handed in
@pytest.mark.parametrize("name", RR.GOLDENS)
def test_f32_hiddens_path(name):
    c = _golden(name)
    _, _, _, step = _step(c["dims"], c["kind"], "f32", c["decP"], c["recP"], c["cells"])
    err, recon = step.engine.reconstruction_error(c["enc"].cuda(), hiddens=torch.from_numpy(c["g"]["hiddens"]).cuda(), want_recon=True)
    err, recon = err.cpu().numpy(), recon.cpu().numpy()
    assert err.dtype == np.float32 and err.shape == (c["dims"][0],) and recon.shape == c["recon_h"].shape
    ratio, ok = _worst(err, c["err_h"], "f32", c["kind"], c["T"])
    gap = abs(float(err.astype(np.float64).mean()) - float(c["g"]["rec_mse"])) / abs(float(c["g"]["rec_mse"]))
    rworst = float(np.abs(recon - c["recon_h"]).max())
    print(name, "T", c["T"], "worst err / bar:", ratio, "mean(err) vs golden rec_mse / bar:", gap / TOL["f32"]["loss"],
          "worst recon error / tau:", rworst / TOL["f32"]["hid"])
    assert ok, (err, c["err_h"])
    assert gap <= TOL["f32"]["loss"], gap
    assert rworst <= TOL["f32"]["hid"], rworst          # the public layout: a wrong transposition of the local form fails here


# ------------------------------------------------------------------------------------------------ 2. fp32, tokens path
@pytest.mark.parametrize("name", RR.GOLDENS)
def test_f32_tokens_path(name):
    """targets[:T] as tokens against the restatement composed with the decoder restatement; T = 1; a table whose first row is all
    <EOS> (every later row <PAD>)."""
    c = _golden(name)
    _, _, _, step = _step(c["dims"], c["kind"], "f32", c["decP"], c["recP"], c["cells"])
    eng, encd, B = step.engine, c["enc"].cuda(), c["dims"][0]
    tables = [("targets[:T]", c["caps"].numpy(), c["err_t"], c["recon_t"])]
    first = np.zeros((3, B), dtype=np.int64)
    first[0] = 2
    for what, caps in (("T = 1", c["caps"].numpy()[:1]), ("first row <EOS>", first)):
        hid = RR.decoder_hiddens(c["decP"], c["enc"], caps, cell=c["cells"][0])
        e, r = RR.per_caption_error(c["recP"], c["kind"], hid, c["enc"], cell=c["cells"][1])
        tables.append((what, caps, e, r))
    for what, caps, ref, rref in tables:
        err, recon = eng.reconstruction_error(encd, tokens=torch.from_numpy(np.ascontiguousarray(caps)).cuda(), want_recon=True)
        err, recon = err.cpu().numpy(), recon.cpu().numpy()
        ratio, ok = _worst(err, ref, "f32", c["kind"], caps.shape[0])
        rworst = float(np.abs(recon - rref).max())
        print(name, what, "worst err / bar:", ratio, "worst recon error / tau:", rworst / TOL["f32"]["hid"])
        assert np.isfinite(err).all() and ok, (what, err, ref)
        assert rworst <= TOL["f32"]["hid"], (what, rworst)


@pytest.mark.parametrize("name", RR.GOLDENS)
def test_f32_reconstruction_through_the_torch_op(name):
    """search.reconstruction_errors(want_recon=True): the torch op sizes the reconstruction from recnet_dim — [B, R] for the global
    kinds, [B, F, D] for the local one — and returns the engine layer's values."""
    c = _golden(name)
    Cfg, dec, rec, _ = _step(c["dims"], c["kind"], "f32", c["decP"], c["recP"], c["cells"])
    B, F, D = c["dims"][:3]
    caps = c["caps"].numpy()
    canon = RR.canonical(caps)
    if np.array_equal(canon, caps):
        ref, rref = c["err_t"], c["recon_t"]
    else:
        ref, rref = RR.per_caption_error(c["recP"], c["kind"], RR.decoder_hiddens(c["decP"], c["enc"], canon, cell=c["cells"][0]), c["enc"],
                                         cell=c["cells"][1])
    err, recon = R.reconstruction_errors(Cfg, dec["model"], rec["model"], c["enc"].cuda(), c["caps"].cuda(), want_recon=True)
    assert isinstance(err, list) and len(err) == B
    assert recon.is_cuda and recon.dtype == torch.float32 and tuple(recon.shape) == ((B, F, D) if c["kind"] == "local" else (B, D))
    ratio, ok = _worst(err, ref, "f32", c["kind"], c["T"])
    rworst = float(np.abs(recon.cpu().numpy() - rref).max())
    print(name, "torch op, want_recon: worst err / bar:", ratio, "worst recon error / tau:", rworst / TOL["f32"]["hid"])
    assert ok, (err, ref)
    assert rworst <= TOL["f32"]["hid"], rworst
    assert R.reconstruction_errors(Cfg, dec["model"], rec["model"], c["enc"].cuda(), c["caps"].cuda()) == err      # without it: the same errors


# ------------------------------------------------------------------------------------------------ 3. scalar loads, several parts per caption
@pytest.mark.parametrize("kind", ["global", "local"])
@pytest.mark.parametrize("D", [42, 520], ids=["D42_scalar", "D520_parts"])
def test_f32_scalar_loads_and_several_parts(D, kind):
    """D = R = 42 (R % 4 != 0: the scalar form; the local caption is cut into 4 parts) and D = R = 520 (16-byte form, 3 parts of a
    global caption, 11 of a local one: the second stage of the sum), B = 3, F = 5, both paths."""
    dims = [3, 5, D, 37, 10, 24, 16, 16]
    B, F, _, V, E, H, A, RA = dims
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D), 5)
    recP = GU.formula_params(GU.rec_shapes(kind, H, D, RA), 6)
    enc, tg = GU.make_batch(B, F, D, V, [4, 2, 6], 7)
    _, _, _, step = _step(dims, kind, "f32", decP, recP)
    eng, encd = step.engine, enc.cuda()
    T = 7
    hid = torch.tanh(torch.randn(T, 1, B, H, generator=torch.Generator().manual_seed(8)))
    ref, rref = RR.per_caption_error(recP, kind, hid, enc)
    err, recon = eng.reconstruction_error(encd, hiddens=hid.cuda(), want_recon=True)
    r1, ok1 = _worst(err.cpu().numpy(), ref, "f32", kind, T)
    w1 = float(np.abs(recon.cpu().numpy() - rref).max())
    caps = tg[:T].contiguous()
    ref_t, rref_t = RR.per_caption_error(recP, kind, RR.decoder_hiddens(decP, enc, caps.numpy()), enc)
    err_t, recon_t = eng.reconstruction_error(encd, tokens=caps.cuda(), want_recon=True)
    r2, ok2 = _worst(err_t.cpu().numpy(), ref_t, "f32", kind, T)
    w2 = float(np.abs(recon_t.cpu().numpy() - rref_t).max())
    none = eng.reconstruction_error(encd, tokens=caps.cuda())                  # without the reconstruction: the same errors
    print(kind, "D", D, "worst err / bar (hiddens, tokens):", r1, r2, "worst recon error / tau:", w1 / TOL["f32"]["hid"], w2 / TOL["f32"]["hid"])
    assert ok1 and ok2
    assert w1 <= TOL["f32"]["hid"] and w2 <= TOL["f32"]["hid"]
    assert none[1] is None and torch.equal(none[0], err_t)


# ------------------------------------------------------------------------------------------------ 4. bf16 through the chains
CHAIN_CASES = ("lr_global_chain", "lr_local_chain", "lr_gru_global_chain")      # B 24, F 6, D 64, H 32


@pytest.mark.parametrize("per_step", [False, True], ids=["chain", "per_step"])
@pytest.mark.parametrize("name", CHAIN_CASES)
def test_bf16_chain_and_per_step(name, per_step, monkeypatch):
    """bf16 at the chain shapes: the persistent reconstructor chain runs (counted through the profile site), resp. the per-step kernels
    when the engine is created under RN_PER_STEP=rec,loc — both within the bf16 bar of the restatement, on both paths."""
    if per_step:
        monkeypatch.setenv("RN_PER_STEP", "rec,loc")
    c = _golden(name)
    _, _, _, step = _step(c["dims"], c["kind"], "bf16", c["decP"], c["recP"], c["cells"])
    eng, encd = step.engine, c["enc"].cuda()
    hidd, capd = torch.from_numpy(c["g"]["hiddens"]).cuda(), c["caps"].cuda()
    out = []
    n_chain = eng.profile_site(7, lambda: out.append(eng.reconstruction_error(encd, hiddens=hidd, want_recon=True)), 1)[0]      # RECNET_SITE_REC_CHAIN_FWD
    assert (n_chain == 0) if per_step else (n_chain >= 1), n_chain
    out.append(eng.reconstruction_error(encd, tokens=capd, want_recon=True))
    assert eng.chain_status() == 0
    tau = TOL["bf16"]["hid"]
    for what, (err, recon), ref, rref in (("hiddens", out[0], c["err_h"], c["recon_h"]), ("tokens", out[1], c["err_t"], c["recon_t"])):
        ratio, ok = _worst(err.cpu().numpy(), ref, "bf16", c["kind"], c["T"])
        rworst = float(np.abs(recon.cpu().numpy() - rref).max())
        print(name, "per-step" if per_step else "chain", "launches", n_chain, what, "worst err / bar:", ratio, "worst recon error / tau:", rworst / tau)
        assert ok, (what, err, ref)
        assert rworst <= tau, (what, rworst)


# ------------------------------------------------------------------------------------------------ 5. two device paths
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["lr_global_chain", "lr_local_chain"])
def test_mean_error_equals_the_forward_passes_rec_mse(name, prec):
    """mean(err) equals the rec_mse recnet_forward_reconstructor(train = 0) exports for the same hidden states on the same handle
    (its loss epilogues / MSE pass on one side, the outputs-only forward and the row kernel on the other)."""
    c = _golden(name)
    _, _, _, step = _step(c["dims"], c["kind"], prec, c["decP"], c["recP"], c["cells"])
    eng, encd, hidd = step.engine, c["enc"].cuda(), torch.from_numpy(c["g"]["hiddens"]).cuda()
    eng.forward_reconstructor(encd, hidd, c["T"], train=False, seed=0)
    mse = eng.scalar_dict()["rec_mse"]
    err, _ = eng.reconstruction_error(encd, hiddens=hidd)
    eng.forward_reconstructor(encd, hidd, c["T"], train=False, seed=0)          # and the forward pass is not disturbed by the call
    mse2 = eng.scalar_dict()["rec_mse"]
    gap = abs(float(err.double().mean()) - mse) / abs(mse)
    print(name, prec, "mean(err) vs rec_mse of the forward pass / (2 bar):", gap / (2 * TOL[prec]["loss"]))
    assert mse2 == mse
    assert gap <= 2 * TOL[prec]["loss"], (gap, mse)


# ------------------------------------------------------------------------------------------------ 6. row independence, determinism
@pytest.mark.parametrize("name,prec", [("global_eval", "f32"), ("local_eval", "f32"), ("lr_global_chain", "bf16"), ("lr_local_chain", "bf16")])
def test_row_independence_and_determinism(name, prec):
    """Permuting the captions together with their features permutes err (twice the bar: two device results); two identical calls
    are bit-identical in err and in the reconstruction, on both paths."""
    c = _golden(name)
    _, _, _, step = _step(c["dims"], c["kind"], prec, c["decP"], c["recP"], c["cells"])
    eng, B = step.engine, c["dims"][0]
    encd, hidd, capd = c["enc"].cuda(), torch.from_numpy(c["g"]["hiddens"]).cuda(), c["caps"].cuda()
    perm = torch.from_numpy(np.random.RandomState(4).permutation(B)).cuda()
    worst = 0.0
    for kw, kwp, ref in ((dict(hiddens=hidd), dict(hiddens=hidd[:, :, perm].contiguous()), c["err_h"]),
                         (dict(tokens=capd), dict(tokens=capd[:, perm].contiguous()), c["err_t"])):
        a = eng.reconstruction_error(encd, want_recon=True, **kw)
        b = eng.reconstruction_error(encd, want_recon=True, **kw)
        p = eng.reconstruction_error(encd[perm].contiguous(), want_recon=True, **kwp)
        torch.cuda.synchronize()
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        ratio, ok = _worst(p[0].cpu().numpy(), a[0][perm].cpu().numpy().astype(np.float64), prec, c["kind"], c["T"], factor=2.0)
        worst = max(worst, ratio)
        assert ok, (p[0], a[0][perm])
        assert float((p[1] - a[1][perm]).abs().max()) <= 2 * TOL[prec]["hid"]
    print(name, prec, "permuted vs unpermuted err / (2 bar):", worst)


# ------------------------------------------------------------------------------------------------ 7. no stale state
@pytest.mark.parametrize("name", ["lr_global_chain", "lr_local_chain"])
def test_a_train_step_behind_the_call_is_undisturbed(name):
    """bf16 at the chain shapes: a fused train step behind a recnet_reconstruction_error call equals the step of a twin handle
    that never made the call (same parameters, same seed) in scalars, gradients and updated parameters; a backward directly behind
    the call is refused."""
    c = _golden(name)
    encd, tgd = c["enc"].cuda(), c["targets"].cuda()
    runs = []
    for with_call in (True, False):
        _, dec, rec, step = _step(c["dims"], c["kind"], "bf16", c["decP"], c["recP"], c["cells"])
        T, w = step.prepare(c["targets"].numpy())
        if with_call:
            step.engine.reconstruction_error(encd, tokens=c["caps"].cuda(), want_recon=True)
            step.engine.reconstruction_error(encd, hiddens=torch.from_numpy(c["g"]["hiddens"]).cuda())
        step(encd, tgd, T, w, seed=1)
        torch.cuda.synchronize()
        assert step.engine.chain_status() == 0
        sc = step.engine.scalar_dict()
        grads = {grp + k: v.cpu().numpy().copy() for grp, md in (("dec.", dec), ("rec.", rec)) for k, v in md["_state"].flat()["grad"].views.items()}
        params = {grp + k: v.detach().cpu().numpy().copy() for grp, md in (("dec.", dec), ("rec.", rec)) for k, v in md["model"].state_dict().items()}
        runs.append((sc, grads, params, step))
    (sa, ga, pa, step_a), (sb, gb, pb, _) = runs
    tol = TOL["bf16"]
    wl = max(abs(sa[k] - sb[k]) / max(abs(sb[k]), 1e-12) for k in ("dec_loss", "rec_mse", "rec_loss", "total_loss"))
    wg = max(rel_err(ga[k], gb[k]) for k in gb)
    wp = max(float(np.abs(pa[k] - pb[k]).max()) for k in pb)
    print(name, "step behind the call vs twin: loss", wl / tol["loss"], "gradient", wg / tol["grad"], "parameter", wp / tol["param"], "(of their bars)")
    assert np.isfinite(sa["total_loss"]) and wl <= tol["loss"] and wg <= tol["grad"] and wp <= tol["param"]
    step_a.engine.reconstruction_error(encd, tokens=c["caps"].cuda())
    with pytest.raises(_lib.RecNetError, match="before forward"):
        step_a.engine.backward_reconstructor(encd)
    with pytest.raises(_lib.RecNetError, match="before forward"):
        step_a.engine.backward_decoder(encd, tgd, None, 1.0)
    with pytest.raises(_lib.RecNetError, match="no decoder hidden states"):
        step_a.engine.forward_reconstructor(encd, None, c["T"])


# ------------------------------------------------------------------------------------------------ 8. errors
def test_argument_and_state_errors(monkeypatch):
    dims = [4, 5, 40, 37, 10, 24, 16, 16]
    B, F, D, V, E, H, A, RA = dims
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D), 1)
    recP = GU.formula_params(GU.rec_shapes("global", H, D, RA), 2)
    Cfg, dec, rec, step = _step(dims, "global", "f32", decP, recP)
    eng = step.engine
    enc, tg = GU.make_batch(B, F, D, V, [3, 1, 4, 2], 3)
    encd, caps = enc.cuda(), tg[:5].contiguous().cuda()
    hid = torch.zeros(5, 1, B, H, device="cuda")
    good = eng.reconstruction_error(encd, tokens=caps)[0]
    # the C return codes
    err = torch.zeros(B, device="cuda")
    call = lambda e, t, h, T, o: eng.lib.recnet_reconstruction_error(eng.handle, _ptr(e), _ptr(t), _ptr(h), T, _ptr(o), None, _stream())
    assert call(encd, caps, hid, 5, err) == -1 and b"exactly one" in eng.lib.recnet_last_error()
    assert call(encd, None, None, 5, err) == -1 and b"exactly one" in eng.lib.recnet_last_error()
    assert call(None, caps, None, 5, err) == -1 and call(encd, caps, None, 5, None) == -1
    assert call(encd, caps, None, 0, err) == -1 and b"T out of range" in eng.lib.recnet_last_error()
    assert call(encd, caps, None, 32, err) == -1 and call(encd, None, hid, 32, err) == -1
    assert call(encd, caps, None, 5, err) == 0
    dec_only = Engine(dict(B=B, F=F, D=D, E=E, H=H, A=A, V=V), None, "f32")
    dec_only.bind_decoder({k: v.data for k, v in dec["model"].named_tensors().items()})
    assert dec_only.lib.recnet_reconstruction_error(dec_only.handle, _ptr(encd), _ptr(caps), None, 5, _ptr(err), None, _stream()) == -2
    unbound = Engine(dict(B=B, F=F, D=D, E=E, H=H, A=A, V=V, R=D), "global", "f32")
    with pytest.raises(_lib.RecNetError, match="reconstructor not bound"):
        unbound.reconstruction_error(encd, tokens=caps)
    rec_only = Engine(dict(B=B, F=F, D=D, E=E, H=H, A=A, V=V, R=D), "global", "f32")
    rec_only.bind_reconstructor({k: v.data for k, v in rec["model"].named_tensors().items()})
    with pytest.raises(_lib.RecNetError, match="decoder not bound"):
        rec_only.reconstruction_error(encd, tokens=caps)
    rec_only.pack_weights()
    assert torch.isfinite(rec_only.reconstruction_error(encd, hiddens=hid)[0]).all()          # hidden states need no decoder
    # the engine layer: ranks, dtypes, shapes, both / neither
    for kw in (dict(tokens=caps, hiddens=hid), dict(), dict(tokens=caps[:, :3].contiguous()), dict(tokens=caps.int()), dict(tokens=caps[0]),
               dict(hiddens=hid[:, 0]), dict(hiddens=hid.double()), dict(hiddens=torch.zeros(5, 1, B, H + 1, device="cuda")),
               dict(tokens=caps.cpu())):
        with pytest.raises(RuntimeError):
            eng.reconstruction_error(encd, **kw)
    with pytest.raises(RuntimeError):
        eng.reconstruction_error(encd[:, :, :8].contiguous(), tokens=caps)
    with pytest.raises(_lib.RecNetError, match="T out of range"):
        eng.reconstruction_error(encd, tokens=torch.zeros(32, B, dtype=torch.long, device="cuda"))
    with pytest.raises(_lib.RecNetError, match="T out of range"):
        eng.reconstruction_error(encd, hiddens=torch.zeros(32, 1, B, H, device="cuda"))
    with pytest.raises(_lib.RecNetError):          # T = 0: a tensor without rows has no storage, so the library is handed neither input
        eng.reconstruction_error(encd, tokens=torch.zeros(0, B, dtype=torch.long, device="cuda"))
    # the torch op
    ops = _ops.load()
    for args in ((encd, caps, hid, False), (encd, None, None, False), (encd, caps[:, :3].contiguous(), None, False),
                 (encd, None, hid[:, 0].contiguous(), False), (encd, torch.zeros(32, B, dtype=torch.long, device="cuda"), None, False)):
        with pytest.raises(RuntimeError):
            ops.reconstruction_error(int(eng.handle.value), *args)
    # the Python layer refuses all of these before any launch: the engine it would use is poisoned
    def poisoned(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setitem(R.reconstruction_errors.__globals__, "_rec_engine", poisoned)
    bad = [dict(captions=caps[:, :3].contiguous()), dict(captions=caps.int()), dict(captions=caps[0]), dict(captions=torch.zeros(0, B, dtype=torch.long)),
           dict(captions=torch.zeros(32, B, dtype=torch.long)), dict(captions=torch.full((2, B), V, dtype=torch.long, device="cuda")),
           dict(captions=torch.full((2, B), -1, dtype=torch.long)), dict(captions=[[3] * B, [V] * B]), dict(captions=caps, T=4), dict(captions=caps, T=32)]
    for kw in bad:
        with pytest.raises(ValueError):
            R.reconstruction_errors(Cfg, dec["model"], rec["model"], encd, **kw)
    with pytest.raises(ValueError):
        R.reconstruction_errors(Cfg, dec["model"], rec["model"], encd[0], caps)
    with pytest.raises(ValueError):
        R.reconstruction_errors(Cfg, dec["model"], None, encd, caps)
    with pytest.raises(AssertionError, match="an engine was asked for"):
        R.reconstruction_errors(Cfg, dec["model"], rec["model"], encd, caps)              # a good call does reach the engine
    monkeypatch.undo()
    # the next valid calls succeed: the same errors through every layer
    again = eng.reconstruction_error(encd, tokens=caps)[0]
    py = R.reconstruction_errors(Cfg, dec["model"], rec["model"], encd, caps)
    torch.cuda.synchronize()
    assert torch.equal(good, again) and py == good.cpu().tolist()


# ------------------------------------------------------------------------------------------------ 9. best_of_n
N_CAND, SEED, WEIGHT = 4, 1, 256.0      # chosen on the CPU restatements (see _best_of_design): one winner changes, every margin > 2 bars


@functools.lru_cache(maxsize=None)
def _best_of_design():
    """A tiny global model and, from the CPU restatements alone (tests/sample_ref.py, score_ref.py, recon_ref.py): the n candidate
    sets, their normalised log-probabilities and reconstruction errors at the common T*, and per video the winning margin over the
    combined bar (row bar of the normalised log-probability + weight x bar of the error)."""
    dims = [6, 5, 32, 41, 12, 24, 8, 8]
    B, F, D, V, E, H, A, RA = dims
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D), 21)
    recP = GU.formula_params(GU.rec_shapes("global", H, D, RA), 22)
    enc, _ = GU.make_batch(B, F, D, V, [3] * B, 23)
    cands = []
    for k in range(N_CAND):
        toks, _, margins, _ = SR.sample_search(decP, enc, 1.0, 0, SEED + k)
        assert (margins >= SR.NEAR_TIE).all()                    # the device draws the same tokens
        cands.append(toks)
    t_star = max(len(t) for t in cands)
    lpn, errs, lbar, ebar = [], [], [], []
    for toks in cands:
        lp, amax = SC.score_captions(decP, enc, toks, 1.0)
        s, ln = SC.caption_sums(lp, toks)
        lpn.append(s / ln); lbar.append(SC.row_bar("f32", amax.max(), 1.0))
        e, _ = RR.per_caption_error(recP, "global", RR.decoder_hiddens(decP, enc, RR.canonical(toks, t_star)), enc)
        errs.append(e); ebar.append(RR.err_bar("f32", "global", e, t_star))
    lpn, errs = np.array(lpn), np.array(errs)
    score = lpn - WEIGHT * errs
    srt = np.sort(score, axis=0)
    bar = max(lbar) + WEIGHT * np.array(ebar).max(0)
    clear = (srt[-1] - srt[-2]) > 2 * bar
    return dict(dims=dims, decP=decP, recP=recP, enc=enc, cands=cands, t_star=t_star, lp_winner=lpn.argmax(0), winner=score.argmax(0),
                clear=clear, ratio=(srt[-1] - srt[-2]) / (2 * bar))


def test_best_of_n_with_the_reconstruction_term():
    d = _best_of_design()
    B, H = d["dims"][0], d["dims"][5]
    assert int((d["winner"] != d["lp_winner"]).sum()) >= 1                   # the term changes at least one winner ...
    assert int((~d["clear"]).sum()) == 0 <= B // 4                          # ... and no video is excluded by the margin condition
    Cfg, dec, rec, _ = _step(d["dims"], "global", "f32", d["decP"], d["recP"])
    dm, rm = dec["model"].eval(), rec["model"].eval()
    encd = d["enc"].cuda()
    inp = torch.full((1, B), 1, dtype=torch.long, device="cuda")
    hid = (torch.zeros(1, B, H, device="cuda"), torch.zeros(1, B, H, device="cuda"))
    # defaults / weight 0: what the function returned before the term existed (the host recomputation under the old rule)
    plain = R.best_of_n(Cfg, dm, inp, hid, encd, N_CAND, 1.0, 0, SEED)
    assert R.best_of_n(Cfg, dm, inp, hid, encd, N_CAND, 1.0, 0, SEED, reconstructor=rm, recon_weight=0.0) == plain
    assert R.best_of_n(Cfg, dm, inp, hid, encd, N_CAND, 1.0, 0, SEED, reconstructor=None) == plain
    cands, sums, lens = [], [], []
    for k in range(N_CAND):
        toks, _ = R.sample_search(Cfg, dm, inp, hid, encd, 1.0, 0, SEED + k)
        _, cap, ln = R.score_captions(Cfg, dm, encd, toks)
        cands.append(toks); sums.append(cap); lens.append(ln)
        assert toks == d["cands"][k].tolist()
    ks0, sc0 = [], []
    for b in range(B):
        s = [sums[k][b] / lens[k][b] for k in range(N_CAND)]
        ks0.append(s.index(max(s))); sc0.append(max(s))
    assert plain[1] == ks0 and plain[2] == sc0 and plain[1] == d["lp_winner"].tolist()
    # with the term: the host recomputation from the public functions, and the CPU restatement's winners
    caps, ks, scores = R.best_of_n(Cfg, dm, inp, hid, encd, N_CAND, 1.0, 0, SEED, reconstructor=rm, recon_weight=WEIGHT)
    t_star = max(len(t) for t in cands)
    errs = [R.reconstruction_errors(Cfg, dm, rm, encd, toks, T=t_star) for toks in cands]
    rk, rs = R.pick_best_of_n(sums, lens, errs, WEIGHT)
    assert t_star == d["t_star"] and ks == rk and scores == rs
    for b in range(B):
        assert caps[b] == [cands[ks[b]][t][b] for t in range(lens[ks[b]][b])]
    assert [k for k, c in zip(ks, d["clear"]) if c] == [int(k) for k, c in zip(d["winner"], d["clear"]) if c]
    assert ks != plain[1]
    assert R.best_of_n(Cfg, dm, inp, hid, encd, N_CAND, 1.0, 0, SEED, reconstructor=rm, recon_weight=np.float32(WEIGHT)) == (caps, ks, scores)      # a numpy scalar
    print("best of", N_CAND, "weight", WEIGHT, ": log-probability winners", plain[1], "with the reconstruction term", ks,
          "smallest winning margin / (2 combined bars):", float(d["ratio"].min()))


def test_evaluate_accepts_the_best_of_recon_method():
    d = _best_of_design()
    B = d["dims"][0]
    Cfg, dec, rec, _ = _step(d["dims"], "global", "f32", d["decP"], d["recP"])
    dm, rm = dec["model"], rec["model"]
    idx2word = {i: "w%d" % i for i in range(d["dims"][3])}
    names = ["a", "b", "c", "d", "PAD", "PAD"]
    refs = {k: ["w3 w4 w5", "w7 w8"] for k in "abcd"}
    enc = d["enc"].numpy()
    ev = lambda method, **kw: R.evaluate(Cfg, [(names, enc)], dm, method, idx2word, refs, **kw)
    assert ev(("best_of_recon", N_CAND, 1.0, 0, SEED, 0.0), reconstructor=rm) == ev(("best_of", N_CAND, 1.0, 0, SEED))
    assert set(ev(("best_of_recon", N_CAND, 1.0, 0, SEED, WEIGHT), reconstructor=rm)) == set(ev("greedy"))
    assert ev(("best_of_recon", 1, 0.8, 5, 3, WEIGHT), reconstructor=rm) == ev(("sample", 0.8, 5, 3))      # one candidate: the sample itself
    with pytest.raises(ValueError, match="needs a reconstructor"):
        ev(("best_of_recon", N_CAND, 1.0, 0, SEED, WEIGHT))
