"""The cell matrix: GRU and mixed-cell train steps on every persistent chain kernel, against the CPU oracle.

The reference's own configuration is a GRU decoder with an LSTM local reconstructor (config.py:31-32,76).  Every chain kernel
(csrc/dec_chain.hpp, rec_chain.hpp, loc_chain.hpp, loc_big.hpp) carries a GRU branch and the host code GRU paths of its own (two
members for d W_hh, two windows of the fused Adam epilogue); the shape tables of tests/test_gpu_parity.py ran LSTM/LSTM only.  Here
each shape runs with the cell pairs that put a GRU into the chain the shape was chosen for:

    GG = (GRU, GRU)    GL = (GRU, LSTM), the reference's default    LG = (LSTM, GRU)

Parameters: tests/cells_kit.cell_params (formula_params 31 / 32, the GRU bias vectors times BIAS_SCALE — tests/test_cells_ref.py shows
that with them a wrong GRU in either cell moves some gradient by ten times the bar used here).  Bars: tests/gpu_util.TOL, unchanged.
Every bf16 case also asserts that the chain kernels are what ran: the launch counts of profile sites 7-10 are those recnet_create's
eligibility rules (csrc/api.hip) give for the shape — restated in chain_launches below, with no cell in them: a GRU model takes every
chain its LSTM twin takes.  Each test prints its figures over their bars before it asserts."""
import time

import pytest
import torch

import recnet_amd as R
from oracle import recnet_oracle as O
from tests import golden_util as GU
from tests.cells_kit import GG, GL, LG, PAIR_ID, cell_params, oracle_grads_no_reg
from tests.gpu_util import TOL, make_models, oracle_grads, rel_err
from tests.test_gpu_parity import EDGE, EDGE_KSPLIT, EDGE_LOC_GROUPS, HYBRID

pytestmark = pytest.mark.gpu


def chain_launches(dims, kind, prec, ncu, alt=(), per_step=()):
    """[reconstructor forward, reconstructor backward, decoder forward, decoder BPTT] chain launches of one fused forward + backward:
    recnet_create's rules (csrc/api.hip) at caption_max_len 30.  The reconstructor's chains are bracketed once per row group, the
    decoder's once around its groups (csrc/host_reconstructor.inc: rc_launch; csrc/host_decoder.inc: prof_bracket_begin)."""
    B, F, D, V, E, H, A, RA = dims
    if prec != "bf16":
        return [0, 0, 0, 0]
    on = lambda name: name not in per_step and "all" not in per_step
    cdiv = lambda a, b: (a + b - 1) // b
    Rr, PAN, MAXG, CPW = D, 112, 4, 2          # RC_PAN_ROWS, RN_MAX_ROW_GROUPS, LC_CPW
    ng = cdiv(B, PAN)
    Bg = cdiv(B, ng) if 1 <= ng <= MAXG else B
    N = 4 * H + A
    NA = N // 16
    p_dec = on("dec") and H % 8 == 0 and H <= 512 and F <= 32 + 16 and A <= 128 and N % 16 == 0 and Bg <= PAN and max(NA, Bg) + 1 <= ncu
    NAb = ((H + 63) >> 6) * 4 * 4              # DCB_NA: CS_PARTS * DCB_KS workgroups per 64 units
    p_dec_bwd = on("dec_bwd") and p_dec and (B <= 128 or Bg < B) and H % 16 == 0 and max(NAb, Bg) + 1 <= ncu
    if kind == "global":
        p_rec = on("rec") and Bg <= PAN and Rr % 8 == 0 and Rr <= 2048 and Rr // 8 <= ncu
        p_rec_bwd = on("rec_bwd") and p_rec and Rr % 16 == 0
        groups = cdiv(B, Bg)
        return [groups * int(p_rec), groups * int(p_rec_bwd), int(p_dec), int(p_dec_bwd)]
    Bl = Bg                                    # row groups of the local chains
    if Bl > 64 and (Rr > 2048 or (Rr // 16) * 2 + cdiv(Bl, CPW) + 1 > ncu):
        ngl = (B + 63) // 64
        if ngl <= 2 * MAXG:
            Bl = cdiv(B, ngl)
    ms = 2 if Bl > 64 else 1
    lc_ng, lc_nc = Rr // 16, cdiv(Bl, CPW)
    nwg = lc_ng * ms + lc_nc + 1
    if nwg - 1 == ncu:
        nwg -= 1
    hyb = "loc_no_hybrid" not in alt
    p_loc = (on("loc") and Bl <= PAN and Rr % 32 == 0 and (Rr <= 2048 or (hyb and Rr <= 4096 and Rr % 256 == 0)) and lc_ng <= 256 and
             H % 32 == 0 and H <= 512 and RA <= 128 and RA % 4 == 0 and F + 1 < 128 and nwg <= ncu and nwg - 1 <= 256)
    nwb = lc_ng + (H // 16) * (2 if Bl > 64 else 1) + lc_nc + 1
    ksx = (4 * Rr + 2047) // 2048
    nwx = lc_ng + ((H + 63) // 64) * ((Bl + 31) // 32) * ksx + lc_nc + 1
    fx = 0 if "loc_xsplit_never" in alt else (2 if "loc_xsplit_always" in alt else 1)
    if fx and ksx <= 4 and (Rr >= 512 or fx == 2) and nwx <= ncu and nwx - 1 <= 256:
        nwb = nwx
    steps, nwg_big = Rr // 128, (H + Rr) // 64 * 4
    p_big = (on("loc_big") and on("loc_bwd") and Rr > 2048 and Rr % 128 == 0 and 18 <= steps <= 32 and steps % 2 == 0 and H % 64 == 0 and
             H <= 512 and RA <= 128 and RA % 8 == 0 and Bl <= 64 and B <= 64 * 2 * MAXG and F <= 40 and nwg_big <= ncu and nwg_big <= 256 and
             Rr // 16 < nwg_big and Bl < nwg_big)
    p_loc_bwd = on("loc_bwd") and p_loc and Rr <= 2048 and H % 16 == 0 and not (Bl > 64 and Rr > 1536) and nwb <= ncu and nwb - 1 <= 256
    groups = cdiv(B, Bl)
    return [groups * int(p_loc), groups * int(p_big or p_loc_bwd), int(p_dec), int(p_dec_bwd)]


def test_launch_rule_restatement_gives_the_counts_the_lstm_tests_assert():
    """tests/test_gpu_parity.py asserts these for the LSTM models at a chip of 256 CUs."""
    assert chain_launches(EDGE["GROUPS_B224_two_full_panels"][0], "global", "bf16", 256) == [2, 2, 1, 1]
    assert chain_launches(EDGE["GROUPS_B224_two_full_panels"][0], "local", "bf16", 256) == [2, 2, 1, 1]
    for case, (dims, lens, n) in EDGE_LOC_GROUPS.items():
        assert chain_launches(dims, "local", "bf16", 256)[:2] == [n, n], case
    for case, (dims, lens) in HYBRID.items():
        n = (dims[0] + 63) // 64
        assert chain_launches(dims, "local", "bf16", 256)[:2] == [n, n if "big_backward" in case else 0], case
        assert chain_launches(dims, "local", "bf16", 256, alt=("loc_no_hybrid",), per_step=("loc_big",))[:2] == [0, 0], case
        assert chain_launches(dims, "local", "f32", 256) == [0, 0, 0, 0], case


_ORACLE = {}


def _shape(case):
    for tab in (EDGE, EDGE_KSPLIT, HYBRID, VARIANT_SHAPES, A48_SHAPES):
        if case in tab:
            return tab[case][:2]
    return EDGE_LOC_GROUPS[case][:2]


def _oracle(case, kind, pair, reg):
    """One oracle run per (shape, kind, pair), shared by the precisions and the forced variants; never modified."""
    key = (case, kind, pair, reg)
    if key not in _ORACLE:
        dims, lens = _shape(case)
        B, F, D, V, E, H, A, RA = dims
        decP, recP = cell_params(dims, kind, pair)
        enc, targets = GU.make_batch(B, F, D, V, lens, 78)
        if reg:
            _ORACLE[key] = oracle_grads(decP, recP, kind, enc, targets, True, 6, cells=pair)
        else:
            _ORACLE[key] = oracle_grads_no_reg(decP, recP, kind, enc, targets, pair, 6)
    return _ORACLE[key]


def _step_vs_oracle(family, case, kind, pair, prec, reg=True, alt=()):
    dims, lens = _shape(case)
    B, F, D, V, E, H, A, RA = dims
    decP, recP = cell_params(dims, kind, pair)
    enc, targets = GU.make_batch(B, F, D, V, lens, 78)
    t0 = time.time()
    ref = _oracle(case, kind, pair, reg)
    t_oracle = time.time() - t0
    C, dec, rec = make_models(dims, kind, prec, decP, recP, cells=pair)
    step = R.TrainStep(dec, rec)
    T, w = step.prepare(targets.numpy())
    assert T == max(lens) + 1
    eng = step.engine
    eng.poison_lds()       # NaN in every CU's LDS: a kernel reading LDS it never wrote cannot pass by luck
    e, t = enc.cuda(), targets.cuda()
    fn = lambda: step.fwd_bwd(e, t, T, w, seed=6)
    t0 = time.time()
    counts = [eng.profile_site(7, fn, 1)[0]]
    if reg:
        eng.add_reg_grad(0, 1.0)
        eng.add_reg_grad(1, 1.0)
    torch.cuda.synchronize()
    t_dev = time.time() - t0
    status = eng.chain_status()
    sc = eng.scalar_dict()
    got = {grp: {k: v.cpu().numpy().copy() for k, v in md["_state"].flat()["grad"].views.items()} for grp, md in (("dec", dec), ("rec", rec))}
    tol = TOL[prec]
    ld, lr = ("dec_loss", "rec_loss") if reg else ("dec_ce", "rec_mse")
    e_dec, e_rec = abs(sc[ld] - ref[ld]) / abs(ref[ld]), abs(sc[lr] - ref[lr]) / abs(ref[lr])
    errs = {grp + "." + k: rel_err(got[grp][k], ref[grp + "_grad"][k]) for grp in got for k in got[grp]}
    kmax = max(errs, key=errs.get)
    if prec == "bf16":     # the other three sites on the same step object (the gradients above are already copied)
        counts += [eng.profile_site(site, fn, 1)[0] for site in (8, 9, 10)]
        torch.cuda.synchronize()
        status |= eng.chain_status()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    want = chain_launches(dims, kind, prec, ncu, alt=alt)
    print("cells %s %s %s %s %s%s: loss/bar dec %.3f rec %.3f, worst gradient/bar %.3f (%s), launches %s, oracle %.2f s device %.2f s" % (
        family, case, PAIR_ID.get(pair, "LL"), kind, prec, " " + ",".join(alt) if alt else "", e_dec / tol["loss"], e_rec / tol["loss"],
        errs[kmax] / tol["grad"], kmax, counts, t_oracle, t_dev))
    assert status == 0
    if prec == "bf16":
        assert counts == want, "chain launches (reconstructor forward / backward, decoder forward / BPTT): %s, recnet_create's rules give %s" % (counts, want)
    else:
        assert counts == [0]
    assert e_dec <= tol["loss"] and e_rec <= tol["loss"], (e_dec, e_rec)
    bad = [(k, v) for k, v in errs.items() if not v <= tol["grad"]]
    assert not bad, bad


# ---- decoder chains (csrc/dec_chain.hpp): a GRU decoder with either reconstructor cell, both reconstructor kinds
DEC_CASES = ["H32_A16_persistent_decoder", "H48_A40_F3_partial_ksteps", "H512_A128_one_chunk", "H32_T1_chain_without_barriers", "H32_T2_one_hand_over",
             "H32_T31_longest", "F33_one_extra_frame", "F48_A40_all_extra_frames", "F40_C4_frames", "GROUPS_B113_two_groups"]


@pytest.mark.parametrize("prec", ["bf16", "f32"])
@pytest.mark.parametrize("kind", ["global", "local"])
@pytest.mark.parametrize("pair", [GL, GG], ids=lambda p: PAIR_ID[p])
@pytest.mark.parametrize("case", DEC_CASES)
def test_gru_decoder_chains_vs_oracle(case, pair, kind, prec):
    _step_vs_oracle("decoder", case, kind, pair, prec)


# H48_A40_F3_partial_ksteps and F48_A40_all_extra_frames do NOT take the decoder chains, under either cell: 4H + A = 232 is no multiple
# of 16 (recnet_create: (N & 15) == 0), so chain_launches gives 0 for them above and the per-step kernels are what those two cases
# hold.  Their A = 48 twins (4H + A = 240) do take the chains: partial k-steps, and all sixteen extra frames from LDS.  LSTM / LSTM
# runs them too, since no LSTM test ever put a chain there either.
A48_SHAPES = {"H48_A48_F3_partial_ksteps_on_the_chain": ([37, 3, 32, 29, 8, 48, 48, 16], [(5 * i) % 8 for i in range(37)]),
              "F48_A48_all_extra_frames_on_the_chain": ([5, 48, 32, 29, 8, 48, 48, 16], [4, 2, 6, 1, 3])}


@pytest.mark.parametrize("pair", [GL, GG, ("LSTM", "LSTM")], ids=["GL", "GG", "LL"])
@pytest.mark.parametrize("case", sorted(A48_SHAPES))
def test_decoder_chains_at_H48_with_a_chain_eligible_attention_size(case, pair):
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert chain_launches(A48_SHAPES[case][0], "global", "bf16", ncu)[2:] == [1, 1]
    _step_vs_oracle("decoder", case, "global", pair, "bf16")


# ---- global reconstructor chains (csrc/rec_chain.hpp): a GRU reconstructor behind either decoder cell.  The last four are the shapes
# of tests/test_gpu_parity.py's _chain_variants that select the other tilings (wide backward, two row parts with a ragged last unit
# group, one row in the third row part, R = 2048), until now compared device against device only
VARIANT_SHAPES = {
    "VAR_B100_R1536": ([100, 2, 1536, 29, 8, 32, 16, 16], [(7 * i) % 5 for i in range(100)]),
    "VAR_B57_R1040": ([57, 2, 1040, 29, 8, 32, 16, 16], [(7 * i) % 5 for i in range(57)]),
    "VAR_B65_R1056": ([65, 2, 1056, 29, 8, 32, 16, 16], [(7 * i) % 5 for i in range(65)]),
    "VAR_B60_R2048": ([60, 2, 2048, 29, 8, 32, 16, 16], [(5 * i) % 4 for i in range(60)]),
}
GLOBAL_CASES = ["B100_two_row_halves", "B57_second_half_one_row", "B112_R40_all_rows", "GROUPS_B224_two_full_panels"] + sorted(VARIANT_SHAPES)


@pytest.mark.parametrize("prec", ["bf16", "f32"])
@pytest.mark.parametrize("pair", [LG, GG], ids=lambda p: PAIR_ID[p])
@pytest.mark.parametrize("case", GLOBAL_CASES)
def test_gru_global_reconstructor_chains_vs_oracle(case, pair, prec):
    if prec == "f32" and _shape(case)[0][2] >= 2048:
        pytest.skip("the fp32 loss bar is below the error of the oracle's float32 norm over W_hh at R = 2048 (tests/test_gpu_parity.py: "
                    "test_local_chains_in_row_groups_of_their_own)")
    # fp32 at R >= 1024: without the regulariser on either side.  The oracle's float32 torch.norm over the 3.2 - 7.1 M elements of the GRU's
    # W_hh is off by 1.4e-3 ... 6.8e-3 in sum_p ||p||, i.e. lambda times that = 1.4e-5 ... 6.8e-5 of a loss near 1.5 — above the fp32 loss bar
    # of 1e-5 (measured against a float64 norm; the same reason as above, from a smaller R on).  CE, MSE and every gradient are compared.
    _step_vs_oracle("global", case, "global", pair, prec, reg=not (prec == "f32" and _shape(case)[0][2] >= 1024))


# ---- local reconstructor chains (csrc/loc_chain.hpp): a GRU reconstructor (LG, GG), and the LSTM chains under a GRU decoder (GL)
LOCAL_CASES = ["LOC_R64_B100_RA24", "LOC_R96_B40_RA128", "LOC_R32_B20_RA8_T31", "LOC_R128_B65_F1", "LOC_R1024_B34_two_k_parts",
               "LOC_R2048_B70_two_local_groups"]


@pytest.mark.parametrize("pair", [LG, GG, GL], ids=lambda p: PAIR_ID[p])
@pytest.mark.parametrize("case", LOCAL_CASES)
def test_gru_local_reconstructor_chains_vs_oracle(case, pair):
    _step_vs_oracle("local", case, "local", pair, "bf16")


@pytest.mark.parametrize("case", LOCAL_CASES[:4])
def test_gru_local_backward_chain_with_k_split_forced(case, monkeypatch):
    monkeypatch.setenv("RN_ALT", "loc_xsplit_always")
    _step_vs_oracle("local", case, "local", LG, "bf16", alt=("loc_xsplit_always",))


# ---- hybrid forward chain and phased backward chain (loc_chain_kernel's hybrid form, csrc/loc_big.hpp), GRU reconstructor; no
# regulariser on either side, as in tests/test_gpu_parity.py's test_hybrid_forward_chain_vs_oracle
@pytest.mark.parametrize("case", ["LOC_R3584_B64_hybrid_no_relay", "LOC_R3072_H128_B37_big_backward_T31", "LOC_R3584_H64_B65_row_groups_big_backward"])
def test_gru_hybrid_forward_and_phased_backward_vs_oracle(case):
    _step_vs_oracle("hybrid", case, "local", LG, "bf16", reg=False)


# ---- per-step kernels off the fast paths, both precisions
# (the H > 512 case exercises the decoder cell kernels; one reconstructor is enough)
PER_STEP_CASES = [(c, k) for c in ("A136", "A264", "H1032", "B1", "F1", "T1_empty_captions", "T31_all_full") for k in ("global", "local")
                  if not (c == "H1032" and k == "local")]


@pytest.mark.parametrize("prec", ["bf16", "f32"])
@pytest.mark.parametrize("pair", [GG, GL], ids=lambda p: PAIR_ID[p])
@pytest.mark.parametrize("case,kind", PER_STEP_CASES)
def test_gru_per_step_kernels_off_the_fast_paths_vs_oracle(case, kind, pair, prec):
    _step_vs_oracle("per_step", case, kind, pair, prec)


# ---- the streamed-fragment images of the R > 2048 chains follow a GRU update
def test_streamed_fragment_images_follow_the_gru_update():
    """LOC_R2560_H64_B20_big_backward, LSTM decoder + GRU local reconstructor, bf16, both learning rates 1e-2: two fused train steps.
    The fused W_hh product + Adam epilogue has two GRU windows (csrc/host_reconstructor.inc: img_row0 = 0 and 3R) and writes the
    [W_ih | W_hh] image, its transpose and the streamed-fragment images; after the second step every image equals a fresh pack of the
    parameters, and the second step's CE / MSE are the oracle's second step's."""
    case, pair = "LOC_R2560_H64_B20_big_backward", LG
    dims, lens = HYBRID[case]
    B, F, D, V, E, H, A, RA = dims
    decP, recP = cell_params(dims, "local", pair)
    enc, targets = GU.make_batch(B, F, D, V, lens, 78)
    C, dec, rec = make_models(dims, "local", "bf16", decP, recP, cells=pair, decoder_learning_rate=1e-2, reconstructor_learning_rate=1e-2)
    step = R.TrainStep(dec, rec)
    encd, tg = enc.cuda(), targets.cuda()
    T, w = step.prepare(targets.numpy())
    step(encd, tg, T, w, seed=6)
    step(encd, tg, T, w, seed=7)
    torch.cuda.synchronize()
    sc = step.engine.scalar_dict()
    assert step.engine.chain_status() == 0
    stale = step.engine.images_stale()
    st = O.TrainState(decP, recP, "local", cell=pair[0], rec_cell=pair[1], dec_lr=1e-2, rec_lr=1e-2)
    st.step(enc, targets, targets > 0, O.Dropper("hash", seed=6))
    with torch.no_grad():
        _, _, _, ce, mse = st.losses(enc, targets, targets > 0, O.Dropper("hash", seed=7))
    tol = TOL["bf16"]
    e_ce, e_mse = abs(sc["dec_ce"] - float(ce)) / abs(float(ce)), abs(sc["rec_mse"] - float(mse)) / abs(float(mse))
    print("cells update %s LG local bf16: second step CE %.6f oracle %.6f, MSE %.6f oracle %.6f, loss/bar dec %.3f rec %.3f, stale image words %d" % (
        case, sc["dec_ce"], float(ce), sc["rec_mse"], float(mse), e_ce / tol["loss"], e_mse / tol["loss"], stale))
    assert stale == 0
    assert e_ce <= tol["loss"] and e_mse <= tol["loss"], (e_ce, e_mse)


# ---- device against device: the local chains against the per-step kernels they replace, GRU reconstructor
LOCAL_VARIANTS = [{"RN_PER_STEP": "loc"}, {"RN_PER_STEP": "loc_bwd"}, {"RN_PER_STEP": "loc_big"}, {"RN_ALT": "loc_no_hybrid"}]
_DEFAULT = {}


def _device_run(case, pair):
    dims, lens = _shape(case)
    B, F, D, V, E, H, A, RA = dims
    decP, recP = cell_params(dims, "local", pair, bias_scale=1.0)
    enc, targets = GU.make_batch(B, F, D, V, lens, 78)
    C, dec, rec = make_models(list(dims), "local", "bf16", decP, recP, cells=pair)
    step = R.TrainStep(dec, rec)
    T, w = step.prepare(targets.numpy())
    step.fwd_bwd(enc.cuda(), targets.cuda(), T, w, seed=6)
    torch.cuda.synchronize()
    assert step.engine.chain_status() == 0
    sc = step.engine.scalar_dict()
    g = {grp + "." + k: v.cpu().numpy().copy() for grp, md in (("dec", dec), ("rec", rec)) for k, v in md["_state"].flat()["grad"].views.items()}
    return sc, g


@pytest.mark.parametrize("env", LOCAL_VARIANTS, ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
@pytest.mark.parametrize("case", ["LOC_R64_B100_RA24", "LOC_R2560_H64_B20_big_backward"])
def test_gru_local_chain_variants(case, env, monkeypatch):
    """The local twin of tests/test_gpu_parity.py's _chain_variants, LSTM decoder + GRU local reconstructor: losses to 1e-5 / 1e-6,
    gradients to 2e-3 — 5e-3 at R = 2560, where each of the four switches replaces the hybrid forward or the phased backward chain by
    the per-step kernels (the bar test_hybrid_forward_chain_vs_oracle has for that pair).
    The standard formula_params (GRU biases not scaled: no oracle is involved here, and the sensitivity test of tests/test_cells_ref.py
    is about the oracle comparisons).

    What this test found: at LOC_R64_B100_RA24 the reconstructor's attn_b gradient differed by 2.6e-3 between the backward chain and the
    per-step backward (every other tensor within the bar, the losses equal to 1e-7).  Both forms summed it from the bf16 copies of
    dWhr_s, which they round at different points, and the sum nearly cancels (attn_b is shared by all frames and the softmax gradient
    sums to zero over them).  It is now the column sum of the fp32 dUd, which holds the same terms (csrc/host_reconstructor.inc:
    bwd_rec_local_deferred).  (Below R = 2048 "loc" takes the backward chain off as well — recnet_create: persist_loc_bwd needs
    persist_loc — so "loc" and "loc_bwd" compare the same pair of backward forms there.)"""
    if case not in _DEFAULT:
        _DEFAULT[case] = _device_run(case, LG)
    sc0, g0 = _DEFAULT[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc1, g1 = _device_run(case, LG)
    bar = 5e-3 if _shape(case)[0][2] > 2048 else 2e-3      # (R > 2048: each of the four switches replaces half of the hybrid / phased pair)
    e_rec, e_dec = abs(sc0["rec_loss"] - sc1["rec_loss"]) / abs(sc0["rec_loss"]), abs(sc0["dec_loss"] - sc1["dec_loss"]) / abs(sc0["dec_loss"])
    errs = {k: rel_err(g1[k], g0[k]) for k in g0}
    kmax = max(errs, key=errs.get)
    print("cells variants %s LG %s: loss/bar rec %.3f dec %.3f, worst gradient/bar %.3f (%s)" % (
        case, env, e_rec / 1e-5, e_dec / 1e-6, errs[kmax] / bar, kmax))
    assert e_rec <= 1e-5 and e_dec <= 1e-6
    bad = [(k, v) for k, v in errs.items() if not v <= bar]
    assert not bad, bad
