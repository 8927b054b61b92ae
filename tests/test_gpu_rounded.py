"""The bf16 chain kernels against the operand-rounded restatement (oracle/recnet_rounded.py, float64), elementwise.

The plain oracle rounds nothing, so the bars that hold the bf16 path to it (tests/gpu_util.TOL["bf16"]) have to leave room for the
operand rounding itself — room in which one caption at one step can be wrong (tests/test_rounded_ref.py shows it with
named mistakes).  The restatement rounds what the product rounds, and what is left between it and the device is summation order:
bars TOL["bf16_rounded"], 16 x the floors tests/test_rounded_ref.py measures on the CPU, per family.

One fused forward + backward per case at the smallest shape that selects each form of each chain kernel (the rows of
tests/test_gpu_parity.py's EDGE / EDGE_KSPLIT / HYBRID tables, restated in tests/rounded_kit.DIMS), LDS poisoned, no regulariser
on either side.  Compared: CE and MSE (relative); the hidden states of forward_decoder (autograd API, train mode) per (t, b) row; every
gradient tensor as a norm ratio, by slice (rounded_kit.slices) and by its worst element.  The chain launch counts are those
recnet_create's rules give (tests/test_gpu_cells.chain_launches) and chain_status() is 0.  Every case prints its figures over their
bars before it asserts."""
import time

import pytest
import torch

import recnet_amd as R
from tests import rounded_kit as K
from tests.gpu_util import TOL, make_models
from tests.test_gpu_cells import chain_launches

pytestmark = pytest.mark.gpu

# case -> RN_ALT: the K split of the local backward chain forced, as test_local_backward_chain_with_k_split_forced forces it
ALT = {"LOC_R1024_B34_two_k_parts": "loc_xsplit_always"}


@pytest.mark.parametrize("family,case,pair", K.GPU_CASES, ids=[K.case_id(c) for c in K.GPU_CASES])
def test_chain_kernels_vs_rounded_restatement(family, case, pair, monkeypatch):
    kind = K.KIND[family]
    alt = (ALT[case],) if case in ALT else ()
    if alt:
        monkeypatch.setenv("RN_ALT", alt[0])
    dims, lens, decP, recP, enc, targets = K.inputs(case, kind, pair)
    ref, t_ref = K.restated(case, kind, pair)
    C, dec, rec = make_models(dims, kind, "bf16", decP, recP, cells=pair)
    step = R.TrainStep(dec, rec)
    T, w = step.prepare(targets.numpy())
    assert T == max(lens) + 1
    eng = step.engine
    eng.poison_lds()       # NaN in every CU's LDS: a kernel reading LDS it never wrote cannot pass by luck
    e, t = enc.cuda(), targets.cuda()
    fn = lambda: step.fwd_bwd(e, t, T, w, seed=K.DROP_SEED)
    t0 = time.time()
    counts = [eng.profile_site(7, fn, 1)[0]]
    torch.cuda.synchronize()
    t_dev = time.time() - t0
    status = eng.chain_status()
    sc = eng.scalar_dict()
    got = dict(dec_ce=sc["dec_ce"], rec_mse=sc["rec_mse"])
    for grp, md in (("dec", dec), ("rec", rec)):
        got[grp + "_grad"] = {k: v.cpu().numpy().copy() for k, v in md["_state"].flat()["grad"].views.items()}
    counts += [eng.profile_site(site, fn, 1)[0] for site in (8, 9, 10)]      # the other three sites (the gradients above are already copied)
    torch.cuda.synchronize()
    status |= eng.chain_status()
    dec["model"].train()
    _, hid, _ = R.forward_decoder(dec, e, t, t > 0, teacher_forcing_ratio=1.0, seed=K.DROP_SEED)
    got["hiddens"] = hid.detach().cpu().numpy()[:, 0]
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    want = chain_launches(dims, kind, "bf16", ncu, alt=alt)
    q, skipped = K.compare(got, ref, dims, kind, pair)
    bars = TOL["bf16_rounded"][family]
    share = {k: q[k][0] / bars[k] for k in K.QUANTITIES}
    worst = max(share, key=share.get)
    nskip = sum(n for n, m in skipped.values())
    print("rounded %s: worst %s %.3e = %.3f of its bar (%s); " % (K.case_id((family, case, pair)), worst, q[worst][0], share[worst], q[worst][1]) +
          ", ".join("%s %.2e/%.1e %s" % (k, q[k][0], bars[k], q[k][1]) for k in K.QUANTITIES) +
          "; skipped slices %d; launches %s, restatement %.2f s device %.2f s" % (nskip, counts, t_ref, t_dev))
    assert status == 0
    assert counts == want, "chain launches (reconstructor forward / backward, decoder forward / BPTT): %s, recnet_create's rules give %s" % (counts, want)
    assert not K.skip_cap_ok(skipped), K.skip_cap_ok(skipped)
    bad = {k: (q[k], bars[k]) for k in K.QUANTITIES if not q[k][0] <= bars[k]}
    assert not bad, bad
