"""The train step on the far side of the two settings of the reference's config.py that select other kernels (what V
and caption_max_len select) — every other dimension small (B <= 8, F 3, D 32, E 8, H 32, A 16, RA 16; H = 32 puts the bf16 path on
the persistent chains wherever recnet_create allows them).

  min_count (config.py:48) sets the vocabulary: V <= 5120 keeps a row of ce_kernel in registers, above it the row is streamed, with its
      own loss and dlogits expressions and its own zero fill of the operand padding [V, ldV) that the output layer's backward
      products read.  V = 5120, 5121 (ldV = 5128, one element in the last pass), 5692 and 13501 (the reference's own).
  caption_max_len (config.py:50): Tm = caption_max_len + 1 switches ctx_all_kernel / ctx_all_slow_kernel and the local chains at
      32 and every persistent chain at 60; T, the steps of the batch, switches the T <= 32 paths of the local attention kernels.

Every case: one fused forward + backward in train mode with dropout and both regulariser gradients, LDS poisoned, against the CPU
oracle's autograd (tests/test_oracle_golden.py pins the oracle to the reference at caption_max_len = 44 and at V = 5200) to the
project's bars, tests/gpu_util.TOL: losses relative, every gradient tensor ||d|| / ||g||.  Each case prints its worst error / bar."""
import functools

import numpy as np
import pytest
import torch

import recnet_amd as R
from oracle import recnet_oracle as O
from tests import golden_util as GU
from tests import recon_ref as RR
from tests import score_ref as SC
from tests.gpu_util import LR_TOL, REG_SLACK, TOL, make_models, moved, oracle_grads, rel_err

pytestmark = pytest.mark.gpu

F, D, E, H, A, RA = 3, 32, 8, 32, 16, 16
SEED = 6
REG = {"dec": 1e-3, "rec": 1e-2}          # lambda of the norm regulariser (train.py:69,103)


def _params(V, kind):
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D), 31)
    recP = GU.formula_params(GU.rec_shapes(kind, H, D, RA), 32) if kind else None
    return decP, recP


def _grads(dec, rec):
    return {grp: {k: v.cpu().numpy().copy() for k, v in md["_state"].flat()["grad"].views.items()}
            for grp, md in (("dec", dec), ("rec", rec)) if md is not None}


def _fwd_bwd(step, kind, encd, tgd, T, w, site=None, poison_padding=False):
    """One poisoned forward + backward with the regulariser gradients; returns (scalars, gradients before the regulariser,
    gradients, launches of `site`)."""
    eng = step.engine
    eng.poison_lds()       # NaN in every CU's LDS: a kernel reading LDS it never wrote cannot pass by luck
    if poison_padding:
        eng.poison_dlogits_padding(T)
    run = lambda: step.fwd_bwd(encd, tgd, T, w, seed=SEED)
    n = eng.profile_site(site, run, 1)[0] if site is not None else run()
    torch.cuda.synchronize()
    pre = _grads(step.decoder, step.reconstructor)
    eng.add_reg_grad(0, 1.0)
    if kind:
        eng.add_reg_grad(1, 1.0)
    torch.cuda.synchronize()
    return eng.scalar_dict(), pre, _grads(step.decoder, step.reconstructor), n


def _hold(sc, g, ref, kind, prec):
    """Losses and every gradient tensor against the oracle; returns the worst error / bar."""
    tol = TOL[prec]
    ratios = {"dec_loss": abs(sc["dec_loss"] - ref["dec_loss"]) / (tol["loss"] * abs(ref["dec_loss"]))}
    if kind:
        ratios["rec_loss"] = abs(sc["rec_loss"] - ref["rec_loss"]) / (tol["loss"] * abs(ref["rec_loss"]))
    for grp in g:
        for k in g[grp]:
            ratios[grp + "." + k] = rel_err(g[grp][k], ref[grp + "_grad"][k]) / tol["grad"]
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}          # (a NaN is bad)
    assert not bad, bad
    return max(ratios.values())


def _same_run(a, b):
    """Two runs of one step on one engine: bit for bit, except what is summed with float atomics in an order the hardware
    chooses (scalars, bias / attn_b column sums, the embedding scatter — the rule of tests/test_gpu_acquire_inv.py)."""
    (sa, ga), (sb, gb) = a, b
    for k in sa:
        assert np.isclose(sa[k], sb[k], rtol=2e-5, atol=1e-7), k
    for grp in ga:
        for k, x in ga[grp].items():
            y = gb[grp][k]
            if x.ndim == 1 or x.shape[0] == 1 or k == "embedding.weight":
                assert np.allclose(x, y, rtol=2e-5, atol=1e-7), (grp, k)
            else:
                assert np.array_equal(x, y), (grp, k)


# ================================================================================================ 1. vocabulary
VOCABS = (5120, 5121, 5692, 13501)
V_LENS = [6, 3, 0, 5, 1, 4, 2, 6]
V_PAD_CAPTION = 2


@functools.lru_cache(maxsize=None)
def _vocab_batch(V):
    """Eight captions of up to six tokens with the tokens put in that the row kernel's branches turn on: V - 1 (twice: the scatter
    of the embedding gradient meets it again), 5120 and one from the middle of the streamed tail where V has them, tokens below
    256, and one caption that is <PAD> in every row."""
    enc, targets = GU.make_batch(len(V_LENS), F, D, V, V_LENS, 78, Tm=7)
    targets[:, V_PAD_CAPTION] = 0
    targets[0, 0] = V - 1
    targets[3, 7] = V - 1
    targets[2, 3] = 7
    targets[0, 1] = 255
    if V > 5120:
        targets[1, 0] = 5120
        targets[2, 0] = (5120 + V) // 2
    return enc, targets


def _check_vocab_batch(V, targets):
    t = targets.numpy()
    assert t.shape == (7, 8) and t.max() == V - 1 and int((t == V - 1).sum()) >= 2
    assert (t[:, V_PAD_CAPTION] == 0).all(), "the all-<PAD> caption"
    assert ((t > 0) & (t < 256)).any() and (t == 255).any()
    if V > 5120:
        assert (t >= 5120).any() and (t == 5120).any()
    if V > 5122:
        assert ((t > 5120) & (t < V - 1)).any()
    live = (t > 0).sum(axis=0)
    assert live[0] == 7 and live[7] == 7      # the captions that carry the high tokens run to the last step
    return sorted(set(int(x) for x in t.ravel() if x >= 5120 or x == V - 1))


@functools.lru_cache(maxsize=None)
def _vocab_ref(V, kind):
    decP, recP = _params(V, kind)
    enc, targets = _vocab_batch(V)
    return oracle_grads(decP, recP, kind, enc, targets, True, SEED, caption_max_len=6)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("kind", [None, "global"])
@pytest.mark.parametrize("V", VOCABS)
def test_train_step_vs_oracle_across_the_register_row_limit(V, kind, prec):
    """ce_kernel on both sides of V = 20 * 256.  The padding columns [V, ldV) of the dlogits operand are poisoned with NaN before the
    step: the kernel's zero fill is what keeps them out of dlogits . W_o, dlogits^T . Hs and the bias column sum.  Beside the
    per-tensor bars, the embedding.weight and out.weight gradient rows of every token >= 5120 of the batch (and of V - 1) are
    held row by row — ||d_row|| / ||g_row|| within the same TOL[prec]["grad"], a whole-tensor norm would hide one wrong row among
    13501 — and their data part (before the regulariser adds lambda p / ||p|| to every row) is not zero."""
    dims = [8, F, D, V, E, H, A, RA]
    decP, recP = _params(V, kind)
    enc, targets = _vocab_batch(V)
    high = _check_vocab_batch(V, targets)
    C, dec, rec = make_models(dims, kind, prec, decP, recP, caption_max_len=6)
    step = R.TrainStep(dec, rec)
    T, w = step.prepare(targets.numpy())
    assert T == 7
    npad = (-V) % 8
    assert npad == {5120: 0, 5121: 7, 5692: 4, 13501: 3}[V]
    sc, pre, g, _ = _fwd_bwd(step, kind, enc.cuda(), targets.cuda(), T, w, poison_padding=True)
    assert step.engine.chain_status() == 0
    ref = _vocab_ref(V, kind)
    worst = _hold(sc, g, ref, kind, prec)
    worst_row = 0.0
    for k in ("embedding.weight", "out.weight"):
        p64 = decP[k].double().numpy()
        reg_rows = REG["dec"] * p64 / np.linalg.norm(p64)
        for tok in high:
            want = ref["dec_grad"][k][tok]
            assert np.linalg.norm(want - reg_rows[tok]) > 1e-3 * np.linalg.norm(want), (k, tok, "the oracle's row is regulariser only")
            assert np.linalg.norm(pre["dec"][k][tok]) > 0, (k, tok)
            e = rel_err(g["dec"][k][tok], want)
            worst_row = max(worst_row, e / TOL[prec]["grad"])
            assert e <= TOL[prec]["grad"], (k, tok, e)
    print("V", V, kind, prec, "padding columns", npad, "worst error / bar:", worst, "worst high-token row / bar:", worst_row)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_step_api_in_train_mode_at_the_first_streamed_vocabulary(prec):
    """Decoder.forward in train mode (logits_drop_kernel over [B, 5121]) for three steps against the oracle's step with the same
    counter-based masks; the bars of tests/test_gpu_parity.py: test_step_api_matches_reference."""
    V = 5121
    dims = [8, F, D, V, E, H, A, RA]
    decP, _ = _params(V, None)
    enc, targets = _vocab_batch(V)
    C, dec, _ = make_models(dims, None, prec, decP, None, caption_max_len=6)
    m = dec["model"]
    m.train(True)
    m.dropout_seed = 13
    drop = O.Dropper("hash", seed=13)
    encd = enc.cuda()
    tok = torch.full((1, 8), 1, dtype=torch.long, device="cuda")
    hid = (torch.zeros(1, 8, H, device="cuda"), torch.zeros(1, 8, H, device="cuda"))
    ohid = O.zero_hidden(8, H, "LSTM")
    tol, worst, dropped = TOL[prec], 0.0, 0
    for t in range(3):
        lg, hid = m(tok, hid, encd)
        with torch.no_grad():
            olg, ohid = O.decoder_step(decP, tok.cpu(), ohid, enc, drop=drop, t=t)
        lg, olg = lg.cpu().numpy(), olg.numpy()
        assert lg.shape == (8, V)
        dropped += int((olg == 0).sum())
        assert ((lg == 0) == (olg == 0)).all(), "the dropout mask of the logits"
        bar = tol["hid"] * 4 * max(1.0, float(np.abs(olg).max()))
        eh = float(np.abs(hid[0][0].cpu().numpy() - ohid[0][0].numpy()).max())
        worst = max(worst, float(np.abs(lg - olg).max()) / bar, eh / tol["hid"])
        assert np.abs(lg - olg).max() <= bar and eh <= tol["hid"], t
        tok = targets[t].view(1, -1).cuda()
    assert 0.4 * 3 * 8 * V < dropped < 0.6 * 3 * 8 * V      # train mode: about half of the logits are dropped
    print("step API, train mode, V", V, prec, "worst error / bar:", worst)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_score_captions_at_a_streamed_vocabulary(prec):
    """search.score_captions on the batch's captions at V = 5692, eval mode, against tests/score_ref.py with its row bar."""
    V = 5692
    dims = [8, F, D, V, E, H, A, RA]
    decP, _ = _params(V, None)
    enc, targets = _vocab_batch(V)
    _check_vocab_batch(V, targets)
    C, dec, _ = make_models(dims, None, prec, decP, None, caption_max_len=6)
    dec["model"].eval()
    caps = targets.contiguous()
    lps, cap, ln = R.score_captions(C, dec["model"], enc.cuda(), caps.cuda())
    rlp, amax = SC.score_captions(decP, enc, caps.numpy(), 1.0)
    rsum, rlen = SC.caption_sums(rlp, caps.numpy())
    assert ln == rlen.tolist()
    lps, worst = np.array(lps, dtype=np.float64), 0.0
    for t in range(caps.shape[0]):
        bar = SC.row_bar(prec, amax[t], 1.0)
        err = float(np.abs(lps[t] - rlp[t]).max())
        worst = max(worst, err / bar)
        assert err <= bar, (t, err, bar)
    sbar = rlen * SC.row_bar(prec, amax.max(), 1.0)
    serr = np.abs(np.array(cap) - rsum)
    assert (serr <= sbar).all(), (serr, sbar)
    print("score_captions V", V, prec, "worst row error / bar:", worst, "worst caption sum / bar:", float((serr / sbar).max()))


# ================================================================================================ 2. caption length
V_LEN = 61
# name: (caption_max_len, lens, T)
LENGTHS = {
    "Tm32_T32_fast_paths_full": (31, [31, 3, 0, 7, 1, 12], 32),
    "Tm33_T33_first_on_slow_paths": (32, [32, 3, 0, 9, 1], 33),
    "Tm45_T7_Tm_and_T_disagree": (44, [6, 2, 0, 5, 1, 4, 3, 6], 7),
    "Tm60_T60_chain_limit": (59, [59, 59, 1, 0, 30, 17], 60),
    "Tm61_T61_every_chain_off": (60, [60, 2, 17, 0, 33], 61),
}
SITES = (7, 8, 9, 10)        # csrc/launch.hpp: reconstructor chain forward / backward, decoder chain forward / backward


def _expected_launches(kind, Tm):
    """recnet_create (csrc/api.hip) at these dims, bf16, one row group: persist_dec / persist_dec_bwd and the global
    reconstructor's persist_rec / persist_rec_bwd ask for Tm <= 60, the local reconstructor's persist_loc / persist_loc_bwd for
    Tm <= 32; every other condition of theirs holds at H = R = 32, A = RA = 16, F = 3, B <= 8."""
    dec = 1 if Tm <= 60 else 0
    rec = 0 if kind is None else (dec if kind == "global" else (1 if Tm <= 32 else 0))
    return [rec, rec, dec, dec]


def _length_batch(case):
    cml, lens, T = LENGTHS[case]
    enc, targets = GU.make_batch(len(lens), F, D, V_LEN, lens, 78, Tm=cml + 1)
    return cml, lens, T, enc, targets


@functools.lru_cache(maxsize=None)
def _length_ref(case, kind):
    cml, lens, T, enc, targets = _length_batch(case)
    decP, recP = _params(V_LEN, kind)
    return oracle_grads(decP, recP, kind, enc, targets, True, SEED, caption_max_len=cml)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("kind", [None, "global", "local"])
@pytest.mark.parametrize("case", sorted(LENGTHS))
def test_train_step_vs_oracle_across_the_caption_length_switches(case, kind, prec):
    """bf16: the step runs once per profile site on ONE engine — the launches of each chain kernel are what the rules of
    recnet_create say (decoder and global chains on through Tm = 60, local chains off from Tm = 33, everything off at 61),
    chain_status stays 0, every run is held to the oracle, and every later run equals the first (the stamped words epoch << 6 | t
    and barrier words epoch << 7 | phase of a launch are not cleared: the later launches are the ones that meet the earlier
    ones' stamps)."""
    cml, lens, T_want, enc, targets = _length_batch(case)
    Tm = cml + 1
    dims = [len(lens), F, D, V_LEN, E, H, A, RA]
    assert targets.shape[0] == Tm and max(lens) + 1 == T_want and 0 in lens
    decP, recP = _params(V_LEN, kind)
    C, dec, rec = make_models(dims, kind, prec, decP, recP, caption_max_len=cml)
    step = R.TrainStep(dec, rec)
    assert step.engine.lib.recnet_dim(step.engine.handle, 9) == Tm
    T, w = step.prepare(targets.numpy())
    assert T == T_want
    encd, tgd = enc.cuda(), targets.cuda()
    ref = _length_ref(case, kind)
    assert ref["hiddens"].shape[0] == T
    worst, runs, launches = 0.0, [], []
    for site in (SITES if prec == "bf16" else (None,)):
        sc, _, g, n = _fwd_bwd(step, kind, encd, tgd, T, w, site=site)
        assert step.engine.chain_status() == 0
        worst = max(worst, _hold(sc, g, ref, kind, prec))
        runs.append((sc, g))
        launches.append(n)
    if prec == "bf16":
        assert launches == _expected_launches(kind, Tm), (launches, _expected_launches(kind, Tm))
        for later in runs[1:]:
            _same_run(runs[0], later)
    print(case, kind, prec, "T", T, "Tm", Tm, "chain launches", launches if prec == "bf16" else "-", "worst error / bar:", worst)


def test_benchmark_shape_rules_are_where_the_length_cases_put_them():
    """The expected launch counts above against the ends recnet_create names: Tm = 31 (the benchmark's) takes every chain."""
    assert _expected_launches("global", 31) == [1, 1, 1, 1] and _expected_launches("local", 31) == [1, 1, 1, 1]
    assert _expected_launches("local", 32) == [1, 1, 1, 1] and _expected_launches("local", 33) == [0, 0, 1, 1]
    assert _expected_launches("global", 60) == [1, 1, 1, 1] and _expected_launches("global", 61) == [0, 0, 0, 0]
    assert _expected_launches(None, 60) == [0, 0, 1, 1] and _expected_launches(None, 61) == [0, 0, 0, 0]


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_replayed_update_path_at_Tm45(prec):
    """The path bench.py times (DataParallelTrainStep + GraphedStep, replay mode "graph" of tests/test_gpu_parity.py:
    test_benchmarked_update_path_matches_reference_optimizer, with that test's measures and bars) at caption_max_len = 44 with
    captions of 40 and 33 tokens, global reconstructor, learning rates of 1e-2: three replays against three steps of the
    oracle's train step (torch.optim.Adam as the reference builds it; pinned to the reference at these learning rates by
    tests/test_oracle_golden.py: test_large_learning_rate_runs_pin_the_update_rule) — every loss, the parameters and both
    moments relative to how far they moved, the packed operand images word for word."""
    cml, lens, n = 44, [40, 3, 0, 33, 7, 12], 3
    dims = [len(lens), F, D, V_LEN, E, H, A, RA]
    decP, recP = _params(V_LEN, "global")
    enc, targets = GU.make_batch(len(lens), F, D, V_LEN, lens, 78, Tm=cml + 1)
    C, dec, rec = make_models(dims, "global", prec, decP, recP, caption_max_len=cml, decoder_learning_rate=1e-2,
                              reconstructor_learning_rate=1e-2)
    step = R.DataParallelTrainStep(dec, rec, dims[0], 0, 1, n_frames=F)
    seed0 = 42
    step.step_impl.seed_base = seed0 - 1          # the device-side rule: dropout seed of optimiser step n (1-based) = base + n
    T, w = step.prepare(targets.numpy())
    assert T == 41
    run = R.GraphedStep(step, enc.cuda(), targets.cuda(), T, w, warmup=0, defer_reconstructor_update=False)
    eng = step.step_impl.engine
    losses = [run().clone() for _ in range(n)]
    run.flush()
    torch.cuda.synchronize()
    assert eng.chain_status() == 0
    assert eng.images_stale() == 0
    st = O.TrainState(decP, recP, "global", dec_lr=1e-2, rec_lr=1e-2, caption_max_len=cml)
    masks = targets > 0
    ref_l = [st.step(enc, targets, masks, O.Dropper("hash", seed=seed0 + it)) for it in range(n)]
    tol, lt = TOL[prec], LR_TOL[prec]
    assert min(abs(ref_l[it + 1][2] - ref_l[it][2]) for it in range(n - 1)) > 10 * tol["loss"] * abs(ref_l[0][2]), ref_l   # the steps differ
    worst = 0.0
    for it in range(n):
        sc = losses[it].cpu().numpy()
        for slot, want in ((6, ref_l[it][2]), (2, ref_l[it][0]), (5, ref_l[it][1])):
            worst = max(worst, abs(float(sc[slot]) - want) / ((tol["loss"] + REG_SLACK) * abs(want)))
            assert abs(float(sc[slot]) - want) <= (tol["loss"] + REG_SLACK) * abs(want), (it, slot, float(sc[slot]), want)
    bad = []
    for grp, md, P0, P, opt in (("dec", dec, decP, st.dec, st.dec_opt), ("rec", rec, recP, st.rec, st.rec_opt)):
        fl = md["_state"].flat()
        for k in P0:
            got = md["model"].state_dict()[k].cpu().numpy()
            e, d = moved(got, P[k].detach().numpy(), P0[k].numpy())
            assert d > 1e-3, (grp, k, d)
            s = opt.state[P[k]]
            em = rel_err(fl["exp_avg"].views[k].cpu().numpy(), s["exp_avg"].numpy())
            ev = rel_err(fl["exp_avg_sq"].views[k].cpu().numpy(), s["exp_avg_sq"].numpy())
            worst = max(worst, e / lt["move"], em / lt["m"], ev / lt["v"])
            bad += [(grp, k, what, x) for what, x, bar in (("param", e, lt["move"]), ("exp_avg", em, lt["m"]), ("exp_avg_sq", ev, lt["v"]))
                    if not x <= bar]
    assert not bad, bad
    print("graph replay, Tm 45, T 41,", prec, "worst error / bar:", worst)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_score_captions_longer_than_31_rows(prec):
    """search.score_captions documents 1 <= T <= caption_max_len + 1.  At caption_max_len = 44 captions of 41 rows used to be
    refused ("T out of range"): the scorer ran on the engine it shares with Decoder.forward, which is built for 31 rows.  It now
    takes the engine keyed by the config's caption_max_len; held to tests/score_ref.py with its row bar, and twice with
    reuse_features (the second call reads the invariants the first left on that engine)."""
    cml, lens = 44, [40, 3, 0, 33, 7, 12]
    dims = [len(lens), F, D, V_LEN, E, H, A, RA]
    decP, _ = _params(V_LEN, None)
    enc, targets = GU.make_batch(len(lens), F, D, V_LEN, lens, 78, Tm=cml + 1)
    C, dec, _ = make_models(dims, None, prec, decP, None, caption_max_len=cml)
    dec["model"].eval()
    caps = targets[:41].contiguous()
    assert not bool(targets[41:].any()) and bool(targets[40].any())
    encd = enc.cuda()
    lps, cap, ln = R.score_captions(C, dec["model"], encd, caps.cuda())
    assert R.score_captions(C, dec["model"], encd, caps.cuda(), reuse_features=True) == (lps, cap, ln)
    rlp, amax = SC.score_captions(decP, enc, caps.numpy(), 1.0)
    rsum, rlen = SC.caption_sums(rlp, caps.numpy())
    assert ln == rlen.tolist() and max(ln) == 41
    lps, worst = np.array(lps, dtype=np.float64), 0.0
    for t in range(41):
        bar = SC.row_bar(prec, amax[t], 1.0)
        worst = max(worst, float(np.abs(lps[t] - rlp[t]).max()) / bar)
        assert np.abs(lps[t] - rlp[t]).max() <= bar, t
    assert (np.abs(np.array(cap) - rsum) <= rlen * SC.row_bar(prec, amax.max(), 1.0)).all()
    with pytest.raises(ValueError):
        R.score_captions(C, dec["model"], encd, torch.zeros(46, len(lens), dtype=torch.long, device="cuda"))
    print("score_captions, 41 rows at caption_max_len 44,", prec, "worst row error / bar:", worst)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["global", "local"])
def test_search_entry_points_at_Tm45(kind, prec):
    """search.reconstruction_errors and search.score_captions on the batch's own captions with an engine of Tm = 45: the chains
    with outputs only, recon_err's part count clamped by Tm — at the captions' own T = 7 and padded to T = 45 (the decoder and
    global chains over 45 steps; the local attention over T > 32 states) — against tests/recon_ref.py and tests/score_ref.py
    with their bars."""
    cml, lens, T0, enc, targets = _length_batch("Tm45_T7_Tm_and_T_disagree")
    dims = [len(lens), F, D, V_LEN, E, H, A, RA]
    decP, recP = _params(V_LEN, kind)
    C, dec, rec = make_models(dims, kind, prec, decP, recP, caption_max_len=cml)
    dec["model"].eval()
    rec["model"].eval()
    caps = targets[:T0].contiguous()
    encd = enc.cuda()
    worst = 0.0
    for T in (None, cml + 1):
        canon = RR.canonical(caps.numpy(), T)
        Tn = canon.shape[0]
        assert Tn == (T0 if T is None else 45)
        want, _ = RR.per_caption_error(recP, kind, RR.decoder_hiddens(decP, enc, canon), enc, caption_max_len=cml)
        err = np.array(R.reconstruction_errors(C, dec["model"], rec["model"], encd, caps.cuda(), T=T), dtype=np.float64)
        bar = RR.err_bar(prec, kind, want, Tn)
        assert np.isfinite(err).all()
        worst = max(worst, float((np.abs(err - want) / bar).max()))
        assert (np.abs(err - want) <= bar).all(), (T, err, want, bar)
    lps, cap, ln = R.score_captions(C, dec["model"], encd, caps.cuda())
    rlp, amax = SC.score_captions(decP, enc, caps.numpy(), 1.0)
    rsum, rlen = SC.caption_sums(rlp, caps.numpy())
    assert ln == rlen.tolist()
    lps, worst_lp = np.array(lps, dtype=np.float64), 0.0
    for t in range(T0):
        bar = SC.row_bar(prec, amax[t], 1.0)
        worst_lp = max(worst_lp, float(np.abs(lps[t] - rlp[t]).max()) / bar)
        assert np.abs(lps[t] - rlp[t]).max() <= bar, t
    assert (np.abs(np.array(cap) - rsum) <= rlen * SC.row_bar(prec, amax.max(), 1.0)).all()
    print("search at Tm 45", kind, prec, "worst reconstruction error / bar:", worst, "worst log-probability / bar:", worst_lp)
