"""CPU tests of the operand-rounded restatement (oracle/recnet_rounded.py) that tests/test_gpu_rounded.py holds the bf16 chain
kernels to.

  rounding off   the restatement equals the plain oracle at the fp32 bars: pins the re-factoring (P hoist, batched input projections,
                 one output-layer product on mean_t hr_t, deferred weight gradients) independently of the rounding.
  the floor      the rounded restatement in float32, contractions in chunks of 32 summed last chunk first, against itself in float64:
                 what summation order alone moves.  The bars are 16 x the worst floor of a family (tests/gpu_util.ROUNDED_FLOOR, measured
                 over every GPU case and three dropout seeds by `python -m tests.test_rounded_ref`); the test here measures the two
                 cheapest shapes again and asserts 16 x floor <= bar, so that the bars cannot drift away from their source.
  the skip cap   at every GPU case the restatement's own gradients leave at most 10 % of a tensor's slices below the skip threshold.
  power          named local mistakes (tests/rounded_kit.MISTAKES) applied to the rounded restatement: (a) against the PLAIN oracle
                 each passes today's check (TOL["bf16"]: loss, hidden states, per-tensor norm ratio) — it is a gap; (b) against the
                 clean restatement the proving ones exceed a new bar of their family at least 4 x.  Measured (seed 6), quantity over
                 its new bar:
                     hand_over_slip        hidden 7.3e-3 / 3.2e-5 = 226 x      rec_reads_zero      MSE 1.25e-5 / 1.97e-6 = 6.3 x
                     mask_t_plus_1         slice 7.4e-2 / 1.02e-2 = 7.3 x      stale_frame_weight  hidden 5.1e-4 / 3.2e-5 = 15.7 x
                     rec_hand_over_slip    MSE 1.27e-5 / 1.97e-6 = 6.4 x
                 and three that stay inside both checks (proves = False): the same hand-over slip and a frame left out under the
                 DECODER family's bars, which the floor of H512_A128_one_chunk sets (hidden 4.9e-3), and one (t, b) row missing from
                 the deferred d W_hh (norm ratio 1.1e-2 against 4 x 4.1e-3).  For those (a) is asserted and (b) printed."""
import numpy as np
import pytest
import torch

from oracle import recnet_rounded as RR
from tests import rounded_kit as K
from tests.cells_kit import GG
from tests.gpu_util import ROUNDED_FLOOR, TOL

SEEDS = (6, 7, 8)


@pytest.mark.parametrize("pair", [K.LL, GG], ids=["LL", "GG"])
@pytest.mark.parametrize("kind", ["global", "local"])
@pytest.mark.parametrize("case", ["RAGGED_B7", "H32_A16_persistent_decoder"])
def test_rounding_off_equals_the_oracle(case, kind, pair):
    dims, lens, decP, recP, enc, targets = K.inputs(case, kind, pair)
    ref = K.plain_oracle(case, kind, pair, 5)
    got = RR.step_grads(decP, recP, kind, enc, targets, pair, 5, round=False)
    q, _ = K.compare(got, ref, dims, kind, pair)
    tol = TOL["f32"]
    print("rounding off %s %s %s: %s" % (case, kind, pair, {k: "%.2e %s" % v for k, v in q.items()}))
    assert q["loss"][0] <= tol["loss"] and q["hid"][0] <= tol["hid"], q
    assert q["grad"][0] <= tol["grad"] and q["slice"][0] <= tol["grad"] and q["elem"][0] <= tol["grad"], q


def floor_of(case, kind, pair, seeds=SEEDS):
    """Worst of each quantity: float32 with reordered contractions against float64, same rounding sites."""
    dims, lens, decP, recP, enc, targets = K.inputs(case, kind, pair)
    worst = {k: 0.0 for k in K.QUANTITIES}
    for seed in seeds:
        ref, _ = K.restated(case, kind, pair, seed)
        got = RR.step_grads(decP, recP, kind, enc, targets, pair, seed, dtype=torch.float32, chunk=True)
        q, _ = K.compare(got, ref, dims, kind, pair)
        for k in worst:
            worst[k] = max(worst[k], q[k][0])
    return worst


@pytest.mark.parametrize("family,case", [("decoder", "H32_T2_one_hand_over"), ("local", "LOC_R128_B65_F1")])
def test_bars_are_sixteen_floors(family, case):
    fl = floor_of(case, K.KIND[family], K.LL)
    bars = TOL["bf16_rounded"][family]
    print("floor %s %s: %s; bars %s" % (family, case, {k: "%.2e" % v for k, v in fl.items()}, {k: "%.2e" % v for k, v in bars.items()}))
    for k in K.QUANTITIES:
        assert bars[k] <= 16.0 * ROUNDED_FLOOR[family][k] * (1 + 1e-12), k      # a bar is 16 x its recorded floor or today's bar, whichever is lower
        assert 16.0 * fl[k] <= bars[k], (k, fl[k], bars[k])


@pytest.mark.parametrize("family,case,pair", K.GPU_CASES, ids=[K.case_id(c) for c in K.GPU_CASES])
def test_restatement_stays_inside_the_skip_cap(family, case, pair):
    kind = K.KIND[family]
    ref, _ = K.restated(case, kind, pair)
    q, skipped = K.compare(ref, ref, K.inputs(case, kind, pair)[0], kind, pair)
    print("skipped slices %s: %d" % (K.case_id((family, case, pair)), sum(n for n, m in skipped.values())))
    assert not K.skip_cap_ok(skipped), K.skip_cap_ok(skipped)
    assert all(v[0] == 0.0 for v in q.values())


def _todays_check(q):
    tol = TOL["bf16"]
    return q["loss"][0] <= tol["loss"] and q["hid"][0] <= tol["hid"] and q["grad"][0] <= tol["grad"]


@pytest.mark.parametrize("name", sorted(K.MISTAKES))
def test_named_mistakes(name):
    family, case, mist, proves = K.MISTAKES[name]
    kind = K.KIND[family]
    dims, lens, decP, recP, enc, targets = K.inputs(case, kind, K.LL)
    clean, _ = K.restated(case, kind, K.LL)
    wrong = RR.step_grads(decP, recP, kind, enc, targets, K.LL, K.DROP_SEED, mistake=mist)
    qa, _ = K.compare(wrong, K.plain_oracle(case, kind, K.LL), dims, kind, K.LL)
    qb, _ = K.compare(wrong, clean, dims, kind, K.LL)
    bars = TOL["bf16_rounded"][family]
    over = {k: qb[k][0] / bars[k] for k in K.QUANTITIES}
    best = max(over, key=over.get)
    print("mistake %s at %s: old check loss %.2e hid %.2e grad %.2e; new check %s; best %s %.1f x its bar (%s)" % (
        name, case, qa["loss"][0], qa["hid"][0], qa["grad"][0], {k: "%.2e" % qb[k][0] for k in K.QUANTITIES}, best, over[best], qb[best][1]))
    assert max(qb[k][0] for k in K.QUANTITIES) > 0.0, "the mistake changed nothing"
    assert _todays_check(qa), "visible to today's check: not evidence of a gap"
    if proves:
        assert over[best] >= 4.0, over


def test_at_least_four_mistakes_prove_the_new_check():
    assert sum(1 for v in K.MISTAKES.values() if v[3]) >= 4


def test_clean_restatement_passes_todays_check_against_the_plain_oracle():
    """The rounding alone stays inside today's bars (else (a) above would say nothing)."""
    for family, case in (("global", "B100_two_row_halves"), ("decoder", "H32_A16_persistent_decoder")):
        kind = K.KIND[family]
        q, _ = K.compare(K.restated(case, kind, K.LL)[0], K.plain_oracle(case, kind, K.LL), K.inputs(case, kind, K.LL)[0], kind, K.LL)
        print("rounding alone %s: loss %.2e hid %.2e grad %.2e" % (case, q["loss"][0], q["hid"][0], q["grad"][0]))
        assert _todays_check(q)


def measure_floors():
    """Every GPU case, three seeds: the table of tests/gpu_util.ROUNDED_FLOOR."""
    worst = {}
    for family, case, pair in K.GPU_CASES:
        fl = floor_of(case, K.KIND[family], pair)
        print("%-48s %s" % (K.case_id((family, case, pair)), "  ".join("%s %.3e" % (k, fl[k]) for k in K.QUANTITIES)), flush=True)
        for k, v in fl.items():
            if v > worst.get((family, k), (0.0, None))[0]:
                worst[(family, k)] = (v, case)
    for family in ("decoder", "global", "local"):
        print(family, "  ".join("%s=%.3e (%s)" % (k, *worst[(family, k)]) for k in K.QUANTITIES))


if __name__ == "__main__":
    measure_floors()
