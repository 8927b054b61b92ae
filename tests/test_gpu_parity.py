"""Parity of the HIP train-step path (through the C ABI) with
  (a) the golden vectors produced by the reference itself (tests/golden/*.npz) and
  (b) the CPU oracle on the same seeded inputs.
Tolerances per precision are in tests/gpu_util.TOL (fp32-MFMA path: tight; bf16-MFMA path: the
bf16 operand-rounding bars of SURVEY.md §8d)."""
import os

import numpy as np
import pytest
import torch

import recnet_amd as R
from oracle import recnet_oracle as O
from tests import golden_util as GU
from tests.gpu_util import LR_TOL, REG_SLACK, TOL, cosine, load_case, make_models, moved, oracle_grads, rel_err

pytestmark = pytest.mark.gpu

SMALL = ["dec_eval", "dec_train", "dec_T31", "dec_T4_samelen", "global_train", "global_eval", "local_train",
         "local_eval", "local_T31", "gru_local_train", "gru_global_eval", "gru_dec_train", "gru_global_train",
         "gru_local_train3"]
FULL = ["full_dec_B8", "full_global_B8", "full_local_B8", "full_gru_global_B8", "full_gru_local_B8"]
# config.py:48,50 moved (tests/golden/make_golden.py): caption_max_len = 44 with captions of 40 and 33 tokens, V = 5200
AXES = ["global_cml44", "dec_V5200"]


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("name", SMALL + FULL)
def test_step_api_matches_reference(name, prec):
    """Decoder.forward (decoder.py:45-70) step by step: logits and (h, c) against the golden vectors."""
    g, dims, kind, decP, recP, enc, targets = load_case(name)
    C, dec, _ = make_models(dims, None, prec, decP, None, cells=g["_cells"])
    model = dec["model"]
    gru = g["_cells"][0] == "GRU"
    train = bool(int(g["meta_train_mode"]))
    model.train(train)
    model.dropout_seed = int(g["meta_drop_seed"])
    B, H = dims[0], dims[5]
    encd = enc.cuda()
    tok = torch.full((1, B), 1, dtype=torch.long, device="cuda")
    # hidden: (h, c) for LSTM, a single tensor for GRU (train.py:28-35)
    hid = torch.zeros(1, B, H, device="cuda") if gru else (torch.zeros(1, B, H, device="cuda"), torch.zeros(1, B, H, device="cuda"))
    tol = TOL[prec]
    for t in range(int(g["T"])):
        logits, hid = model(tok, hid, encd)
        tok = targets[t].view(1, -1).cuda()
        assert np.abs((hid if gru else hid[0])[0].cpu().numpy() - g["step_h"][t]).max() <= tol["hid"], t
        if not gru:
            assert np.abs(hid[1][0].cpu().numpy() - g["step_c"][t]).max() <= 2 * tol["hid"], t
        if "step_logits" in g:
            ref = g["step_logits"][t]
            assert np.abs(logits.cpu().numpy() - ref).max() <= tol["hid"] * 4 * max(1.0, np.abs(ref).max()), t


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("name", SMALL + FULL + AXES)
def test_autograd_api_losses_and_grads(name, prec):
    """forward_decoder / forward_*_reconstructor + loss.backward() (train.py:250-268) against the goldens:
    losses, hidden states, every parameter gradient (norm-regulariser term included)."""
    g, dims, kind, decP, recP, enc, targets = load_case(name)
    C, dec, rec = make_models(dims, kind, prec, decP, recP, cells=g["_cells"], caption_max_len=GU.caption_max_len_of(g))
    train = bool(int(g["meta_train_mode"]))
    seed = int(g["meta_drop_seed"])
    dec["model"].train(train)
    encd, tg = enc.cuda(), targets.cuda()
    dl, hid, _ = R.forward_decoder(dec, encd, tg, tg > 0, 1.0, seed=seed)
    loss = dl
    if kind:
        rec["model"].train(train)
        fwd = R.forward_global_reconstructor if kind == "global" else R.forward_local_reconstructor
        rl = fwd(hid, encd, rec, seed=seed)
        loss = dl + 1.0 * rl
    dec["optimizer"].zero_grad()
    if kind:
        rec["optimizer"].zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    tol = TOL[prec]
    assert hid.shape[0] == int(g["T"])
    assert np.abs(hid.detach().cpu().numpy() - g["hiddens"]).max() <= tol["hid"]
    # The reference's regulariser sum_p ||p|| is a float32 torch.norm on the CPU, itself only good to
    # ~1e-4 relative on multi-million-element tensors (measured: 118.7493 vs the exact 118.7635); the CE and
    # MSE parts are compared tightly, the totals with REG_SLACK * lambda * reg on top.
    assert abs(float(dl.detach()) - float(g["dec_loss"])) <= tol["loss"] * abs(float(g["dec_loss"])) + REG_SLACK * 1e-3 * float(g["dec_reg"])
    sc = dec["_state"].engines[("dec", dims[0], dims[1])].scalar_dict()
    assert abs(sc["dec_ce"] - float(g["dec_ce"])) <= tol["loss"] * abs(float(g["dec_ce"])) + 3e-7 * abs(float(g["dec_loss"]))
    if kind:
        assert abs(float(rl.detach()) - float(g["rec_loss"])) <= tol["loss"] * abs(float(g["rec_loss"])) + REG_SLACK * 1e-2 * float(g["rec_reg"])
        sr = rec["_state"].engines[("rec", dims[0], dims[1])].scalar_dict()
        assert abs(sr["rec_mse"] - float(g["rec_mse"])) <= tol["loss"] * abs(float(g["rec_mse"])) + 3e-7 * abs(float(g["rec_loss"]))
    bad = []
    for grp, md in (("dec", dec), ("rec", rec)):
        if md is None:
            continue
        for k, p in md["model"].named_parameters():
            gg = p.grad.detach().cpu().numpy()
            ref_n = float(g["%s_gnorm/%s" % (grp, k)])
            key = "%s_grad/%s" % (grp, k)
            if key in g:
                e = rel_err(gg, g[key])
                if np.linalg.norm(g[key]) > 0 and cosine(gg, g[key]) < tol["cos"]:
                    bad.append((grp, k, "cosine", cosine(gg, g[key])))
            else:
                e = abs(np.linalg.norm(gg.astype(np.float64)) - ref_n) / max(ref_n, 1e-12)
                sl = g["%s_gslice/%s" % (grp, k)]
                e = max(e, float(np.abs(gg.reshape(-1)[:64] - sl).max() / max(np.abs(sl).max(), 1e-12)) * 0.25)
            # full-shape cases: the regulariser gradient lambda * p / ||p|| dominates the reconstructor's weight
            # gradients at initialisation, and the reference's float32 CPU ||p|| is itself ~1e-4 off on these
            # multi-million-element tensors (see REG_SLACK above)
            lim = tol["grad"] if key in g else max(tol["grad"], REG_SLACK)
            if e > lim:
                bad.append((grp, k, e))
    assert not bad, bad


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["dec_train", "global_train", "local_train", "gru_dec_train", "gru_global_train",
                                  "gru_local_train3"])
def test_fused_train_steps_match_reference_optimizer(name, prec):
    """TrainStep (train.py:248-273 fused: fwd, bwd, regulariser, clip, AMSGrad + Adam) for 3 iterations:
    parameters and Adam state against what the reference produced."""
    g, dims, kind, decP, recP, enc, targets = load_case(name)
    C, dec, rec = make_models(dims, kind, prec, decP, recP, cells=g["_cells"])
    step = R.TrainStep(dec, rec)
    encd, tg = enc.cuda(), targets.cuda()
    T, w = step.prepare(targets.numpy())
    assert T == int(g["T"])
    seed0 = int(g["meta_drop_seed"])
    tol = TOL[prec]
    n = int(g["meta_n_steps"])
    for it in range(n):
        sc = step(encd, tg, T, w, seed=seed0 + it)
        total = float(sc[6])
        assert abs(total - float(g["loss_step%d" % it])) <= (tol["loss"] + REG_SLACK) * abs(float(g["loss_step%d" % it])), it
        if it == 0:
            assert abs(float(sc[7]) - float(g["dec_grad_norm"])) <= max(tol["grad"], 1e-4) * float(g["dec_grad_norm"])
    for grp, md in (("dec", dec), ("rec", rec)):
        if md is None:
            continue
        for k, v in GU.group(g, "%s_after%d" % (grp, n)).items():
            got = md["model"].state_dict()[k].cpu().numpy()
            assert np.abs(got - v.numpy()).max() <= tol["param"], (grp, k)
    fl = dec["_state"].flat()
    for k in decP:
        assert rel_err(fl["exp_avg"].views[k].cpu().numpy(), g["dec_opt/exp_avg/" + k]) <= max(tol["grad"], 1e-4) * 2
        assert rel_err(fl["exp_avg_sq"].views[k].cpu().numpy(), g["dec_opt/exp_avg_sq/" + k]) <= max(tol["grad"], 1e-4) * 4


LR_CASES = ["lr_global_chain", "lr_local_chain", "lr_gru_global_chain",
            # GRU local chains, the reference's default pair (GRU decoder, LSTM local reconstructor), LSTM decoder + GRU global chains
            "lr_gru_local_chain", "lr_refcells_local_chain", "lr_lstm_gru_global_chain"]
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ["eager", "graph", "graph_split_update"])
@pytest.mark.parametrize("name", LR_CASES)
def test_benchmarked_update_path_matches_reference_optimizer(name, mode, prec):
    """train.py:149,186,271-273 through the path bench.py times: GraphedStep (device-side step counter and dropout seed), the split
    reconstructor update (d W_hh and its Adam step left pending and run by the next replay: mode "recurrent"), Adam in the epilogue
    of that grouped product with both operand images of W_hh written there — against four iterations OF THE REFERENCE at learning
    rates of 1e-2 (tests/golden/make_golden.py: lr_*_chain; shapes the persistent chains take).  Every update moves every
    parameter by ~1e-2: the losses of iterations 2-4 are those of the UPDATED weights (a stale bf16 image or transposed image of
    W_hh changes them by far more than the bar), the parameters and both optimisers' moments are compared relative to how far they
    moved; the operand images are compared word for word with a fresh pack of the parameters (Engine.images_stale).
    tests/test_gpu_faults.py shows that a skipped parameter / image / moment store in that epilogue fails this test."""
    g, dims, kind, decP, recP, enc, targets = load_case(name)
    lr = g["meta_lr"]
    C, dec, rec = make_models(dims, kind, prec, decP, recP, cells=g["_cells"], decoder_learning_rate=float(lr[0]),
                              reconstructor_learning_rate=float(lr[1]))
    B, F = dims[0], dims[1]
    encd, tg = enc.cuda(), targets.cuda()
    seed0, n = int(g["meta_drop_seed"]), int(g["meta_n_steps"])
    tol, lt = TOL[prec], LR_TOL[prec]
    losses = []
    if mode == "eager":
        step = R.TrainStep(dec, rec)
        T, w = step.prepare(targets.numpy())
        for it in range(n):
            losses.append(step(encd, tg, T, w, seed=seed0 + it).clone())
        eng = step.engine
    else:
        step = R.DataParallelTrainStep(dec, rec, B, 0, 1, n_frames=F)
        step.step_impl.seed_base = seed0 - 1          # the device-side rule: dropout seed of optimiser step n (1-based) = base + n
        T, w = step.prepare(targets.numpy())
        run = R.GraphedStep(step, encd, tg, T, w, warmup=0,
                            defer_reconstructor_update="recurrent" if mode == "graph_split_update" else False)
        eng = step.step_impl.engine
        if mode == "graph_split_update":
            assert run.deferred and run.defer_mode == "recurrent"
            if prec == "bf16":       # the product + Adam-epilogue launch is what runs (csrc/host_reconstructor.inc: rec_hh_fused_ok)
                assert eng.lib.recnet_dim(eng.handle, 10) == 1, "the split update is not applied at this shape"
        for it in range(n):
            losses.append(run().clone())
        run.flush()
    torch.cuda.synchronize()
    assert eng.chain_status() == 0
    assert T == int(g["T"])
    # every packed operand image (bf16 copies, transposes) is what a fresh pack of the master parameters gives: Adam's normalised
    # update makes the parameters themselves insensitive to a stale image (a fault-injection run with the image stores left out
    # passed the comparisons below), so the images are held directly
    assert eng.images_stale() == 0
    ref_l = [float(g["loss_step%d" % it]) for it in range(n)]
    assert min(abs(ref_l[it + 1] - ref_l[it]) for it in range(n - 1)) > 10 * tol["loss"] * abs(ref_l[0]), ref_l   # the steps differ
    for it in range(n):
        sc = losses[it].cpu().numpy()
        assert abs(float(sc[6]) - ref_l[it]) <= (tol["loss"] + REG_SLACK) * abs(ref_l[it]), (it, float(sc[6]), ref_l[it])
        # CE + MSE parts without the regulariser (40 % of the value at initialisation)
        assert abs(float(sc[2]) - float(g["dec_loss_step%d" % it])) <= (tol["loss"] + REG_SLACK) * abs(float(g["dec_loss_step%d" % it])), it
        assert abs(float(sc[5]) - float(g["rec_loss_step%d" % it])) <= (tol["loss"] + REG_SLACK) * abs(float(g["rec_loss_step%d" % it])), it
    bad = []
    for grp, md in (("dec", dec), ("rec", rec)):
        init = GU.group(g, grp + "_init")
        fl = md["_state"].flat()
        for k, v in GU.group(g, "%s_after%d" % (grp, n)).items():
            got = md["model"].state_dict()[k].cpu().numpy()
            e, d = moved(got, v.numpy(), init[k].numpy())
            assert d > 1e-3, (grp, k, d)
            if e > lt["move"]:
                bad.append((grp, k, "param", e))
            em = rel_err(fl["exp_avg"].views[k].cpu().numpy(), g["%s_opt/exp_avg/%s" % (grp, k)])
            ev = rel_err(fl["exp_avg_sq"].views[k].cpu().numpy(), g["%s_opt/exp_avg_sq/%s" % (grp, k)])
            if em > lt["m"]:
                bad.append((grp, k, "exp_avg", em))
            if ev > lt["v"]:
                bad.append((grp, k, "exp_avg_sq", ev))
    assert not bad, bad


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("cells", [("LSTM", "LSTM"), ("GRU", "GRU")])
@pytest.mark.parametrize("kind", ["global", "local"])
def test_packed_images_follow_update_at_ragged_shapes(kind, cells, prec):
    """The windows of the packed weight images where they can go wrong: the ragged dims of test_fused_step_vs_oracle_ragged_shapes
    (E = 18 puts the column split of rnn.weight_ih_l0 off the 4-column grid: the element-wise pack stores run; GRU: 3 gate blocks
    into the 4-block layout; local: [W_ih | W_hh] behind a column offset).  Two eager steps at learning rates of 1e-2: the images
    equal a fresh pack of the parameters, and — the independent check, the pack and the Adam kernel read one table — the second
    step's losses are the oracle's losses of the parameters the first step left."""
    dims = [7, 5, 88, 101, 18, 36, 20, 12]
    B, F, D, V, E, H, A, RA = dims
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D, cells[0]), 11)
    recP = GU.formula_params(GU.rec_shapes(kind, H, D, RA, cells[1]), 12)
    enc, targets = GU.make_batch(B, F, D, V, [9, 2, 5, 12, 1, 7, 4], 77)
    C, dec, rec = make_models(dims, kind, prec, decP, recP, cells=cells, decoder_learning_rate=1e-2, reconstructor_learning_rate=1e-2)
    step = R.TrainStep(dec, rec)
    encd, tg = enc.cuda(), targets.cuda()
    T, w = step.prepare(targets.numpy())
    step(encd, tg, T, w, seed=5)
    torch.cuda.synchronize()
    dec1 = {k: dec["model"].state_dict()[k].detach().cpu().clone() for k in decP}
    rec1 = {k: rec["model"].state_dict()[k].detach().cpu().clone() for k in recP}
    assert all(float((dec1[k] - decP[k]).abs().max()) > 1e-3 for k in decP), "the first step moved every decoder tensor"
    assert all(float((rec1[k] - recP[k]).abs().max()) > 1e-3 for k in recP), "the first step moved every reconstructor tensor"
    sc = step(encd, tg, T, w, seed=6).clone()
    torch.cuda.synchronize()
    assert step.engine.chain_status() == 0
    assert step.engine.images_stale() == 0
    ref = oracle_grads(dec1, rec1, kind, enc, targets, True, 6, cells=cells)
    tol = TOL[prec]
    print("dec_loss %.8f oracle %.8f | rec_loss %.8f oracle %.8f" % (float(sc[2]), ref["dec_loss"], float(sc[5]), ref["rec_loss"]))
    assert abs(float(sc[2]) - ref["dec_loss"]) <= tol["loss"] * abs(ref["dec_loss"])
    assert abs(float(sc[5]) - ref["rec_loss"]) <= tol["loss"] * abs(ref["rec_loss"])


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["tf_half_global", "tf_half_local"])
def test_teacher_forcing_ratio_below_one_in_the_train_step(name, prec):
    """config.py:71 decoder_teacher_forcing_ratio < 1 (train.py:38,251): TrainStep draws `random.random() <= ratio` per call
    like the reference; a False draw runs the free-running iteration (arg-max fed back, differentiated, stepped).  Four
    reference iterations from random.seed(py_seed) — teacher-forced and free-running mixed: the tokens fed back, every loss, and
    (fp32) the parameters after the fourth step.  bf16: a near-tie of the arg-max may flip, which changes that caption's later
    inputs — losses are held only up to the first iteration whose tokens differ."""
    import random
    g, dims, kind, decP, recP, enc, targets = load_case(name)
    C, dec, rec = make_models(dims, kind, prec, decP, recP, cells=g["_cells"])
    ratio, n = float(g["meta_tf_ratio"]), int(g["meta_n_steps"])
    step = R.TrainStep(dec, rec, teacher_forcing_ratio=ratio)
    encd, tg = enc.cuda(), targets.cuda()
    T, w = step.prepare(targets.numpy())
    seed0 = int(g["meta_drop_seed"])
    tol = TOL[prec]
    random.seed(int(g["meta_py_seed"]))
    same = True
    for it in range(n):
        sc = step(encd, tg, T, w, seed=seed0 + it)
        torch.cuda.synchronize()
        assert step.engine.chain_status() == 0
        tf = bool(g["meta_tf_pattern"][it])
        assert (step.output_indices is None) == tf, it
        if not tf:
            agree = step.output_indices.cpu().numpy() == g["output_indices_step%d" % it]
            if prec == "f32":
                assert agree.all(), it
            same = same and bool(agree.all())
        if same:
            ref = float(g["loss_step%d" % it])
            assert abs(float(sc[6]) - ref) <= (tol["loss"] + REG_SLACK) * abs(ref), it
        assert np.isfinite(float(sc[6]))
    if prec == "f32":
        for grp, md in (("dec", dec), ("rec", rec)):
            for k, v in GU.group(g, "%s_after%d" % (grp, n)).items():
                got = md["model"].state_dict()[k].cpu().numpy()
                assert np.abs(got - v.numpy()).max() <= tol["param"], (grp, k)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("cells", [("LSTM", "LSTM"), ("GRU", "GRU"), ("GRU", "LSTM")])
@pytest.mark.parametrize("kind", [None, "global", "local"])
def test_fused_step_vs_oracle_ragged_shapes(kind, prec, cells):
    """Shapes that are multiples of nothing (B=7, V=101, E=18, D=R=88, H=36, A=20, F=5), train mode with
    dropout: fused fwd+bwd gradients against the CPU oracle's autograd; LSTM and GRU cells."""
    if kind is None and cells == ("GRU", "LSTM"):
        pytest.skip("same as GRU/GRU without a reconstructor")
    dims = [7, 5, 88, 101, 18, 36, 20, 12]
    B, F, D, V, E, H, A, RA = dims
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D, cells[0]), 11)
    recP = GU.formula_params(GU.rec_shapes(kind, H, D, RA, cells[1]), 12) if kind else None
    enc, targets = GU.make_batch(B, F, D, V, [9, 2, 5, 12, 1, 7, 4], 77)
    C, dec, rec = make_models(dims, kind, prec, decP, recP, cells=cells)
    step = R.TrainStep(dec, rec)
    T, w = step.prepare(targets.numpy())
    step.fwd_bwd(enc.cuda(), targets.cuda(), T, w, seed=5)
    step.engine.add_reg_grad(0, 1.0)
    if kind:
        step.engine.add_reg_grad(1, 1.0)
    torch.cuda.synchronize()
    ref = oracle_grads(decP, recP, kind, enc, targets, True, 5, cells=cells)
    sc = step.engine.scalar_dict()
    tol = TOL[prec]
    assert abs(sc["dec_loss"] - ref["dec_loss"]) <= tol["loss"] * abs(ref["dec_loss"])
    if kind:
        assert abs(sc["rec_loss"] - ref["rec_loss"]) <= tol["loss"] * abs(ref["rec_loss"])
    bad = []
    for grp, md in (("dec", dec), ("rec", rec)):
        if md is None:
            continue
        gv = md["_state"].flat()["grad"].views
        for k in gv:
            e = rel_err(gv[k].cpu().numpy(), ref[grp + "_grad"][k])
            if e > tol["grad"]:
                bad.append((grp, k, e))
    assert not bad, bad


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["free_dec", "free_global", "free_local_gru"])
def test_free_running_validation_pass(name, prec):
    """forward_decoder with the reference's default teacher_forcing_ratio (0: the validation call, train.py:327) in eval
    mode: on-device arg-max feedback; tokens exact in the fp32 path, then the reconstructor on those hidden states."""
    g, dims, kind, decP, recP, enc, targets = load_case(name)
    C, dec, rec = make_models(dims, kind, prec, decP, recP, cells=g["_cells"])
    dec["model"].eval()
    encd, tg = enc.cuda(), targets.cuda()
    dl, hid, idx = R.forward_decoder(dec, encd, tg, tg > 0)
    tol = TOL[prec]
    T = int(g["T"])
    assert tuple(idx.shape) == (T, dims[0]) and not idx.requires_grad
    agree = float((idx.cpu().numpy() == g["output_indices"]).mean())
    if prec == "f32":
        assert agree == 1.0
        assert np.abs(hid.detach().cpu().numpy() - g["hiddens"]).max() <= tol["hid"]
        assert abs(float(dl.detach()) - float(g["dec_loss"])) <= tol["loss"] * abs(float(g["dec_loss"]))
    else:
        assert agree >= 0.6          # one flipped near-tie changes every later token of that caption
        # ... and nothing else may differ: up to and including the step of a caption's FIRST flipped token its hidden states are
        # the reference's to the bf16 bar (the flipped token only feeds the NEXT step) — divergence follows a flip, never precedes it
        same = idx.cpu().numpy() == g["output_indices"]                      # [T, B]
        first_flip = np.where(same.all(axis=0), T, (~same).argmax(axis=0))   # per caption: first step whose token differs
        hd = np.abs(hid.detach().cpu().numpy() - g["hiddens"]).reshape(T, -1, dims[0], hid.shape[-1]).max(axis=(1, 3))      # [T, B]
        before = np.arange(T)[:, None] <= first_flip[None, :]
        assert hd[before].max() <= tol["hid"], (float(hd[before].max()), tol["hid"])
        assert int((first_flip == T).sum()) >= dims[0] // 2                  # at least half of the captions never flip
    if kind and prec == "f32":
        rec["model"].eval()
        fwd = R.forward_global_reconstructor if kind == "global" else R.forward_local_reconstructor
        rl = fwd(hid, encd, rec)
        assert abs(float(rl.detach()) - float(g["rec_loss"])) <= tol["loss"] * abs(float(g["rec_loss"]))


@pytest.mark.parametrize("cells", [("LSTM", "LSTM"), ("GRU", "GRU")])
@pytest.mark.parametrize("kind", [None, "local"])
def test_free_running_pass_is_differentiable(kind, cells):
    """teacher_forcing_ratio = 0 in TRAIN mode (dropout on) with loss.backward(), against the oracle's autograd of the
    same free-running unroll: same tokens, losses and gradients (the embedding gradient follows the fed tokens)."""
    dims = [6, 5, 48, 41, 12, 24, 16, 16]
    B, F, D, V, E, H, A, RA = dims
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D, cells[0]), 41)
    decP["out.weight"] = decP["out.weight"] * 6.0          # decisive arg-max
    recP = GU.formula_params(GU.rec_shapes(kind, H, D, RA, cells[1]), 42) if kind else None
    enc, targets = GU.make_batch(B, F, D, V, [5, 2, 7, 3, 1, 4], 79)
    C, dec, rec = make_models(dims, kind, "f32", decP, recP, cells=cells)
    encd, tg = enc.cuda(), targets.cuda()
    dl, hid, idx = R.forward_decoder(dec, encd, tg, tg > 0, 0.0, seed=8)
    loss = dl
    if kind:
        rl = R.forward_local_reconstructor(hid, encd, rec, seed=8)
        loss = dl + rl
    loss.backward()
    torch.cuda.synchronize()
    # oracle
    st = O.TrainState(decP, recP, kind, cell=cells[0], rec_cell=cells[1])
    drop = O.Dropper("hash", seed=8)
    odl, ohid, oidx, oce, _ = O.forward_decoder(st.dec, enc, targets, targets > 0, cell=cells[0], drop=drop,
                                                teacher_forcing=False, return_parts=True)
    oloss = odl
    if kind:
        oloss = odl + O.forward_local_reconstructor(st.rec, ohid, enc, cell=cells[1], drop=drop)
    oloss.backward()
    assert np.array_equal(idx.cpu().numpy(), oidx.numpy())
    tol = TOL["f32"]
    assert abs(float(loss.detach()) - float(oloss)) <= tol["loss"] * abs(float(oloss))
    for k, p in dec["model"].named_parameters():
        assert rel_err(p.grad.cpu().numpy(), st.dec[k].grad.numpy()) <= tol["grad"], k
    if kind:
        for k, p in rec["model"].named_parameters():
            assert rel_err(p.grad.cpu().numpy(), st.rec[k].grad.numpy()) <= tol["grad"], k


# shapes that leave the fast paths of the kernels (F > 32 as in BASELINE config C4, attention sizes > 128 / > 256,
# H > 512 so a caption spans several cell workgroups) and the degenerate ends (one caption, one frame, one step)
EDGE = {
    "F40_C4_frames": ([6, 40, 64, 53, 12, 64, 128, 128], [9, 2, 5, 12, 1, 7]),
    "A136": ([5, 6, 48, 41, 12, 40, 136, 136], [4, 2, 6, 1, 3]),
    "A264": ([4, 5, 40, 37, 10, 24, 264, 264], [3, 5, 1, 2]),
    "H1032": ([3, 4, 32, 29, 8, 1032, 16, 16], [2, 4, 1]),
    "B1": ([1, 5, 40, 37, 10, 24, 16, 16], [6]),
    "F1": ([4, 1, 40, 37, 10, 24, 16, 16], [3, 5, 1, 2]),
    "T1_empty_captions": ([4, 5, 40, 37, 10, 24, 16, 16], [0, 0, 0, 0]),
    "T31_all_full": ([3, 5, 40, 37, 10, 24, 16, 16], [30, 30, 30]),
    # batches with rows in both halves of the persistent reconstructor chain's row split (csrc/rec_chain.hpp)
    "B100_two_row_halves": ([100, 3, 48, 29, 8, 24, 16, 16], [(7 * i) % 9 for i in range(100)]),
    "B57_second_half_one_row": ([57, 3, 32, 29, 8, 24, 16, 16], [(5 * i) % 7 for i in range(57)]),
    "B112_R40_all_rows": ([112, 2, 40, 29, 8, 24, 16, 16], [(3 * i) % 6 for i in range(112)]),
    # shapes the persistent decoder chains take (csrc/dec_chain.hpp: H % 16 == 0, (4H + A) % 16 == 0, H <= 512, A <= 128)
    # (the two A = 40 shapes do NOT: 4H + A = 232 — they hold the per-step kernels; tests/test_gpu_cells.py has A = 48 twins on the chains)
    "H32_A16_persistent_decoder": ([100, 5, 48, 29, 8, 32, 16, 16], [(7 * i) % 9 for i in range(100)]),
    "H48_A40_F3_partial_ksteps": ([37, 3, 32, 29, 8, 48, 40, 16], [(5 * i) % 8 for i in range(37)]),
    "H512_A128_one_chunk": ([9, 4, 32, 29, 8, 512, 128, 16], [3, 1, 4, 1, 5, 2, 6, 5, 3]),
    "H32_T1_chain_without_barriers": ([5, 3, 32, 29, 8, 32, 16, 16], [0, 0, 0, 0, 0]),
    "H32_T2_one_hand_over": ([70, 3, 32, 29, 8, 32, 16, 16], [i % 2 for i in range(70)]),
    "H32_T31_longest": ([3, 3, 32, 29, 8, 32, 16, 16], [30, 7, 30]),
    # frames 32 .. 47 of the decoder chains come from LDS (csrc/dec_chain.hpp, XF)
    "F33_one_extra_frame": ([7, 33, 64, 53, 12, 32, 128, 16], [9, 2, 5, 12, 1, 7, 3]),
    "F48_A40_all_extra_frames": ([5, 48, 32, 29, 8, 48, 40, 16], [4, 2, 6, 1, 3]),
    # shapes the local reconstructor's chains take (csrc/loc_chain.hpp: R % 32 == 0, H % 32 == 0, RA % 4 == 0): two row
    # parts / one part of 64 / of 32 rows; attention sizes that are not multiples of 16; the longest caption
    "LOC_R64_B100_RA24": ([100, 4, 64, 29, 8, 32, 16, 24], [(7 * i) % 9 for i in range(100)]),
    "LOC_R96_B40_RA128": ([40, 3, 96, 29, 8, 64, 16, 128], [(5 * i) % 8 for i in range(40)]),
    "LOC_R32_B20_RA8_T31": ([20, 2, 32, 29, 8, 32, 16, 8], [30] + [(3 * i) % 6 for i in range(19)]),
    "LOC_R128_B65_F1": ([65, 1, 128, 29, 8, 32, 16, 12], [(5 * i) % 7 for i in range(65)]),
    # batches above the 112-row exchange panels (csrc/api.hip: row groups — every chain runs once per group of <= 112 captions):
    # one caption over the limit (57 + 56), two full panels, three uneven groups (77 + 77 + 76); all six chain kernels
    "GROUPS_B113_two_groups": ([113, 3, 64, 29, 8, 32, 16, 16], [(7 * i) % 9 for i in range(113)]),
    "GROUPS_B224_two_full_panels": ([224, 2, 32, 29, 8, 32, 16, 8], [(5 * i) % 7 for i in range(224)]),
    "GROUPS_B230_three_groups_T31": ([230, 2, 32, 29, 8, 32, 16, 8], [30] + [(3 * i) % 6 for i in range(229)]),
}
# K = 4R = 4096: two K parts in the backward chain's X' role (lcb_xsplit_role), second row part with two rows
EDGE_KSPLIT = {"LOC_R1024_B34_two_k_parts": ([34, 2, 1024, 29, 8, 64, 16, 16], [(5 * i) % 6 for i in range(34)])}
# round 4: at R = 2048 the local chains do not fit the chip with more than 64 rows (279 workgroups): such a batch runs them in row
# groups of <= 64 captions of their own — 70 captions as 35 + 35 beside ONE decoder group; 130 as 44 + 44 + 42 beside two of 65
EDGE_LOC_GROUPS = {"LOC_R2048_B70_two_local_groups": ([70, 2, 2048, 29, 8, 32, 16, 16], [(5 * i) % 7 for i in range(70)], 2),
                   "LOC_R2048_B130_three_local_groups": ([130, 2, 2048, 29, 8, 64, 16, 8], [(3 * i) % 5 for i in range(130)], 3)}


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["global", "local"])
@pytest.mark.parametrize("case", sorted(EDGE))
def test_fused_step_vs_oracle_edge_shapes(case, kind, prec):
    dims, lens = EDGE[case] if case in EDGE else (EDGE_KSPLIT[case] if case in EDGE_KSPLIT else EDGE_LOC_GROUPS[case][:2])
    B, F, D, V, E, H, A, RA = dims
    if H > 512 and kind == "local":
        pytest.skip("the H > 512 case exercises the decoder cell kernels; one reconstructor is enough")
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D), 31)
    recP = GU.formula_params(GU.rec_shapes(kind, H, D, RA), 32)
    enc, targets = GU.make_batch(B, F, D, V, lens, 78)
    C, dec, rec = make_models(dims, kind, prec, decP, recP)
    step = R.TrainStep(dec, rec)
    T, w = step.prepare(targets.numpy())
    assert T == max(lens) + 1
    step.engine.poison_lds()       # NaN in every CU's LDS: a kernel reading LDS it never wrote cannot pass by luck
    step.fwd_bwd(enc.cuda(), targets.cuda(), T, w, seed=6)
    step.engine.add_reg_grad(0, 1.0)
    step.engine.add_reg_grad(1, 1.0)
    torch.cuda.synchronize()
    ref = oracle_grads(decP, recP, kind, enc, targets, True, 6)
    sc = step.engine.scalar_dict()
    tol = TOL[prec]
    assert abs(sc["dec_loss"] - ref["dec_loss"]) <= tol["loss"] * abs(ref["dec_loss"])
    assert abs(sc["rec_loss"] - ref["rec_loss"]) <= tol["loss"] * abs(ref["rec_loss"])
    bad = []
    for grp, md in (("dec", dec), ("rec", rec)):
        gv = md["_state"].flat()["grad"].views
        for k in gv:
            e = rel_err(gv[k].cpu().numpy(), ref[grp + "_grad"][k])
            if e > tol["grad"]:
                bad.append((grp, k, e))
    assert not bad, bad


# R above 2048: the hybrid forward chain of the local reconstructor (12 k-steps per wave resident in registers, the rest
# streamed every step; csrc/loc_chain.hpp), with the relay workgroup and — R = 3584 with 64 captions, BASELINE configs[4]:
# 224 + 32 workgroups = every CU — without it (every waiter polls the arrival flags)
HYBRID = {
    "LOC_R2560_B20_hybrid": ([20, 2, 2560, 29, 8, 32, 16, 8], [(3 * i) % 6 for i in range(20)]),
    "LOC_R3584_B64_hybrid_no_relay": ([64, 3, 3584, 29, 8, 32, 16, 12], [(5 * i) % 7 for i in range(64)]),
    # H % 64 == 0: the backward runs the phased chain of csrc/loc_big.hpp too (P / C / L phases of (H + R) / 64 * 4 workgroups)
    "LOC_R3584_H64_B64_big_backward": ([64, 3, 3584, 29, 8, 64, 16, 16], [(5 * i) % 7 for i in range(64)]),
    "LOC_R3072_H128_B37_big_backward_T31": ([37, 2, 3072, 29, 8, 128, 16, 24], [30] + [(3 * i) % 6 for i in range(36)]),
    # round 4: the phased backward chain at every even R / 128 in 18 ... 32, not only the benchmark's 24 / 28 / 32
    "LOC_R2304_H64_B48_big_backward": ([48, 3, 2304, 29, 8, 64, 16, 16], [(5 * i) % 7 for i in range(48)]),
    "LOC_R2560_H64_B20_big_backward": ([20, 3, 2560, 29, 8, 64, 16, 8], [(3 * i) % 6 for i in range(20)]),
    "LOC_R3840_H64_B24_big_backward": ([24, 3, 3840, 29, 8, 64, 16, 16], [(7 * i) % 9 for i in range(24)]),
    # round 6: batches above 64 captions at R > 2048 run both local chains in row groups of <= 64
    "LOC_R3584_H64_B65_row_groups_big_backward": ([65, 3, 3584, 29, 8, 64, 16, 16], [(5 * i) % 7 for i in range(65)]),
    "LOC_R3584_H64_B128_row_groups_big_backward": ([128, 3, 3584, 29, 8, 64, 16, 16], [(5 * i) % 7 for i in range(128)]),
}


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("case", sorted(HYBRID))
def test_hybrid_forward_chain_vs_oracle(case, prec, monkeypatch):
    """The regulariser is left out on both sides (lambda_reg = 0 in the oracle, no add_reg_grad): the reference's float32
    `torch.norm` over the 26-51 M elements of W_hh is off by up to 3e-3 (tests/test_gpu_configs.py), which is the oracle's
    error.  CE and MSE parts and every gradient are compared.  bf16: also against the per-step kernels (RN_ALT=loc_no_hybrid, RN_PER_STEP=loc_big)."""
    dims, lens = HYBRID[case]
    B, F, D, V, E, H, A, RA = dims
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D), 31)
    recP = GU.formula_params(GU.rec_shapes("local", H, D, RA), 32)
    enc, targets = GU.make_batch(B, F, D, V, lens, 78)

    def run():
        C, dec, rec = make_models(dims, "local", prec, decP, recP)
        step = R.TrainStep(dec, rec)
        T, w = step.prepare(targets.numpy())
        step.engine.poison_lds()
        e, t = enc.cuda(), targets.cuda()
        n_chain = step.engine.profile_site(7, lambda: step.fwd_bwd(e, t, T, w, seed=6), 1)[0]
        torch.cuda.synchronize()
        assert step.engine.chain_status() == 0
        g = {grp: {k: v.cpu().numpy().copy() for k, v in md["_state"].flat()["grad"].views.items()} for grp, md in (("dec", dec), ("rec", rec))}
        return step.engine.scalar_dict(), g, n_chain

    sc, g, n_chain = run()
    n_groups = (B + 63) // 64      # (row groups of the local chains above 64 captions)
    assert n_chain == (n_groups if prec == "bf16" else 0), "the hybrid chain kernel is the bf16 path's forward for this shape"
    if prec == "bf16" and "big_backward" in case:
        C, dec, rec = make_models(dims, "local", prec, decP, recP)
        st0 = R.TrainStep(dec, rec)
        T0, w0 = st0.prepare(targets.numpy())
        assert st0.engine.profile_site(8, lambda: st0.fwd_bwd(enc.cuda(), targets.cuda(), T0, w0, seed=6), 1)[0] == n_groups, "loc_big backward chain not taken"
    st = O.TrainState(decP, recP, "local")
    drop = O.Dropper("hash", seed=6)
    dl, hid, _, ce, _ = O.forward_decoder(st.dec, enc, targets, targets > 0, drop=drop, lambda_reg=0.0, return_parts=True)
    rl, mse, _ = O.forward_local_reconstructor(st.rec, hid, enc, drop=drop, lambda_reg=0.0, return_parts=True)
    (dl + rl).backward()
    tol = TOL[prec]
    assert abs(sc["dec_ce"] - float(ce.detach())) <= tol["loss"] * abs(float(ce.detach()))
    assert abs(sc["rec_mse"] - float(mse.detach())) <= tol["loss"] * abs(float(mse.detach()))
    bad = []
    for grp, P in (("dec", st.dec), ("rec", st.rec)):
        for k, v in P.items():
            e = rel_err(g[grp][k], v.grad.numpy())
            if e > tol["grad"]:
                bad.append((grp, k, e))
                if os.environ.get("RN_TEST_DUMP"):
                    np.savez(os.path.join(os.environ["RN_TEST_DUMP"], "%s_%s_%s.npz" % (case, grp, k)), got=g[grp][k], want=v.grad.numpy())
    assert not bad, bad
    if prec == "bf16":
        monkeypatch.setenv("RN_ALT", "loc_no_hybrid")
        monkeypatch.setenv("RN_PER_STEP", "loc_big")
        sc0, g0, n0 = run()
        assert n0 == 0
        for grp in g:
            for k in g[grp]:
                assert rel_err(g[grp][k], g0[grp][k]) <= 5e-3, (grp, k)


@pytest.mark.parametrize("kind", ["global", "local"])
def test_batches_above_112_captions_stay_on_the_persistent_chains(kind, monkeypatch):
    """RC_PAN_ROWS = 112 gated every chain kernel; now a larger batch runs each chain once per row group.
    The results are held to the oracle by the GROUPS_* edge shapes above; this checks that the chain kernels really are what
    ran (one bracketed launch per group for the reconstructor's chains, one bracket around the groups for the decoder's),
    and that RN_ROW_GROUPS=0 restores the per-step kernels."""
    dims, lens = EDGE["GROUPS_B224_two_full_panels"]
    B, F, D, V, E, H, A, RA = dims
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D), 31)
    recP = GU.formula_params(GU.rec_shapes(kind, H, D, RA), 32)
    enc, targets = GU.make_batch(B, F, D, V, lens, 78)

    def launches():
        C, dec, rec = make_models(dims, kind, "bf16", decP, recP)
        step = R.TrainStep(dec, rec)
        T, w = step.prepare(targets.numpy())
        e, t = enc.cuda(), targets.cuda()
        return [step.engine.profile_site(site, lambda: step.fwd_bwd(e, t, T, w, seed=6), 1)[0] for site in (7, 8, 9, 10)]

    assert launches() == [2, 2, 1, 1]
    monkeypatch.setenv("RN_ROW_GROUPS", "0")
    assert launches() == [0, 0, 0, 0]


@pytest.mark.parametrize("case", [c for c in sorted(EDGE) if c.startswith("LOC_")] + sorted(EDGE_KSPLIT))
def test_local_backward_chain_with_k_split_forced(case, monkeypatch):
    """lcb_xsplit_role is selected from R = 512 up; forced here so the small ragged shapes run through it as well."""
    monkeypatch.setenv("RN_ALT", "loc_xsplit_always")
    test_fused_step_vs_oracle_edge_shapes(case, "local", "bf16")


@pytest.mark.parametrize("case", sorted(EDGE_LOC_GROUPS))
def test_local_chains_in_row_groups_of_their_own(case):
    """The bf16 step against the oracle, and that the local chain kernels are what ran: one forward and one backward launch per
    LOCAL row group (recnet_create: bgrp_loc), whatever the decoder's grouping is.  (The fp32 path has no chain kernels, and at
    R = 2048 its loss bar of 1e-5 is below the error of the ORACLE's float32 norm over the 16.7 M elements of W_hh — 1.2e-4 of the
    reconstructor's loss, see tests/test_gpu_configs.py.)"""
    test_fused_step_vs_oracle_edge_shapes(case, "local", "bf16")
    dims, lens, ngroups = EDGE_LOC_GROUPS[case]
    B, F, D, V, E, H, A, RA = dims
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D), 31)
    recP = GU.formula_params(GU.rec_shapes("local", H, D, RA), 32)
    enc, targets = GU.make_batch(B, F, D, V, lens, 78)
    C, dec, rec = make_models(dims, "local", "bf16", decP, recP)
    step = R.TrainStep(dec, rec)
    T, w = step.prepare(targets.numpy())
    e, t = enc.cuda(), targets.cuda()
    assert step.engine.profile_site(7, lambda: step.fwd_bwd(e, t, T, w, seed=6), 1)[0] == ngroups
    assert step.engine.profile_site(8, lambda: step.fwd_bwd(e, t, T, w, seed=6), 1)[0] == ngroups
    assert step.engine.chain_status() == 0


@pytest.mark.parametrize("cell,B,R", [("LSTM", 100, 1536), ("GRU", 37, 256)])
def test_reconstructor_input_written_by_the_decoder_chain_equals_the_separate_kernel(cell, B, R, monkeypatch):
    """dec_chain_kernel writes the global reconstructor's LSTM input [h_t ; drop_t(mp)] (global_reconstructor.py:38-41) itself
    (RN_ALT=dec_no_xcat: xcat_global_kernel behind the chain)."""
    _chain_variants({"RN_ALT": "dec_no_xcat"}, cell, monkeypatch, [B, 2, R, 29, 8, 32, 16, 16], [(7 * i) % 5 for i in range(B)])


@pytest.mark.parametrize("cell,B,R", [("LSTM", 100, 1536), ("GRU", 100, 1536), ("LSTM", 57, 1040), ("LSTM", 112, 2048)])
def test_output_layer_epilogue_of_the_forward_chain_equals_the_separate_kernels(cell, B, R, monkeypatch):
    """rec_chain_kernel's epilogue (out = mean_t h_t . W_o^T + b_o, squared-error partial sums, d out and its operand copy behind one more
    barrier phase: train.py:96-103) against the split-K GEMM + reduction + MSE kernel it replaces (RN_ALT=rec_epilogue_0): the headline size,
    the GRU cells, the smallest batch that takes the two-row-part tiling with a ragged last unit group, every panel row at 16 k-steps."""
    _chain_variants({"RN_ALT": "rec_epilogue_0"}, cell, monkeypatch, [B, 2, R, 29, 8, 32, 16, 16], [(7 * i) % 5 for i in range(B)])


@pytest.mark.parametrize("cell,B,R", [("LSTM", 100, 1536), ("GRU", 100, 1536), ("LSTM", 65, 1056), ("LSTM", 112, 1280)])
def test_global_backward_chain_wide_tiling_equals_the_narrow_one(cell, B, R, monkeypatch):
    """rec_chain_bwd_kernel<48, 3, 2, 2, 16> (32 units x 32 rows, a third of the weights in LDS; B > 64, R in (1024, 1536]):
    the headline size, the GRU block map, one row in the third row part with the fewest k-steps, every panel row in use."""
    _chain_variants({"RN_ALT": "rec_bwd_narrow"}, cell, monkeypatch, [B, 2, R, 29, 8, 32, 16, 16], [(7 * i) % 5 for i in range(B)])


@pytest.mark.parametrize("cell", ["LSTM", "GRU"])
@pytest.mark.parametrize("env", [{"RN_PER_STEP": "rec"}, {"RN_PER_STEP": "rec_bwd"}, {"RN_ALT": "rec_row_parts_1"}, {"RN_ALT": "rec_row_parts_2"},
                                 {"RN_PER_STEP": "dec"}, {"RN_PER_STEP": "dec_bwd"}],
                         ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_persistent_reconstructor_chain_variants(env, cell, monkeypatch):
    _chain_variants(env, cell, monkeypatch, [100, 3, 48, 29, 8, 32, 16, 16], [(7 * i) % 9 for i in range(100)])


@pytest.mark.parametrize("env", [{"RN_PER_STEP": "rec"}, {"RN_PER_STEP": "rec_bwd"}], ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_persistent_reconstructor_chains_R2048(env, monkeypatch):
    """The largest reconstructor the chain kernels take (16 / 64 k-steps of resident weights per wave)."""
    _chain_variants(env, "LSTM", monkeypatch, [60, 2, 2048, 29, 8, 32, 16, 16], [(5 * i) % 4 for i in range(60)])


def _chain_variants(env, cell, monkeypatch, dims, lens):
    """The persistent chain kernels (csrc/rec_chain.hpp: reconstructor forward in both tilings and backward;
    csrc/dec_chain.hpp: decoder forward and BPTT) against the per-step paths they replace: same losses and gradients
    (fp32 summation order differs; the decoder BPTT also forms da = P . dgates from the bf16 dgates)."""
    B, F, D, V, E, H, A, RA = dims
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D, cell), 31)
    recP = GU.formula_params(GU.rec_shapes("global", H, D, RA, cell), 32)
    enc, targets = GU.make_batch(B, F, D, V, lens, 78)

    def run():
        C, dec, rec = make_models(list(dims), "global", "bf16", decP, recP, cells=(cell, cell))
        step = R.TrainStep(dec, rec)
        T, w = step.prepare(targets.numpy())
        step.fwd_bwd(enc.cuda(), targets.cuda(), T, w, seed=6)
        torch.cuda.synchronize()
        sc = step.engine.scalar_dict()
        g = {grp + "." + k: v.cpu().numpy().copy() for grp, md in (("dec", dec), ("rec", rec))
             for k, v in md["_state"].flat()["grad"].views.items()}
        return sc, g
    sc0, g0 = run()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc1, g1 = run()
    assert abs(sc0["rec_loss"] - sc1["rec_loss"]) <= 1e-5 * abs(sc0["rec_loss"])
    assert abs(sc0["dec_loss"] - sc1["dec_loss"]) <= 1e-6 * abs(sc0["dec_loss"])
    bar = 1e-2 if env.get("RN_PER_STEP", "").startswith("dec") else 2e-3    # bf16 dgates in the attention backward
    bad = [(k, rel_err(g1[k], g0[k])) for k in g0 if rel_err(g1[k], g0[k]) > bar]
    assert not bad, bad
