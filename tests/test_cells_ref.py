"""The inputs of the cell matrix (tests/test_gpu_cells.py, the lr_* update-path goldens) can tell a wrong GRU from a right one.
CPU only, on the oracle alone: each of three classic GRU mistakes (tests/cells_kit.py: b_hn outside the r product, z and 1 - z
exchanged, r gating the whole candidate pre-activation) is applied to the decoder's cell alone and to the reconstructor's cell
alone; at one representative shape per input family (decoder chains, global chains, local chains, hybrid / phased local chains,
update path) some gradient tensor has to move by at least ten times the bf16 gradient bar the GPU tests hold the kernels to.
The losses do not carry this: they move by 1e-5 ... 8e-3, mostly under the bf16 loss bar."""
import pytest
import torch

from tests import golden_util as GU
from tests.cells_kit import GG, GL, LG, MISTAKES, PAIR_ID, cell_params, oracle_grads_no_reg, worst_move
from tests.gpu_util import TOL
from tests.test_gpu_parity import EDGE, HYBRID

TOL_BF16_GRAD = TOL["bf16"]["grad"]
FACTOR = 10.0

# family -> (case, kind, the pairs the GPU tests run that family with)
FAMILIES = {
    "decoder": ("H48_A40_F3_partial_ksteps", "global", (GL, GG)),
    "global": ("B57_second_half_one_row", "global", (LG, GG)),
    "local": ("LOC_R96_B40_RA128", "local", (LG, GG, GL)),
    "hybrid": ("LOC_R2560_H64_B20_big_backward", "local", (LG,)),
}
UPDATE = ["lr_lstm_gru_global_chain", "lr_gru_local_chain", "lr_refcells_local_chain"]

_cache = {}


def _inputs(family, pair):
    if family in FAMILIES:
        case, kind, _ = FAMILIES[family]
        dims, lens = (EDGE[case] if case in EDGE else HYBRID[case])[:2]
        B, F, D, V, E, H, A, RA = dims
        decP, recP = cell_params(dims, kind, pair)
        enc, targets = GU.make_batch(B, F, D, V, lens, 78)
        return decP, recP, kind, enc, targets, 6
    g = GU.load(family)
    assert GU.cells_of(g) == pair
    kind = "global" if "global" in family else "local"
    return (GU.group(g, "dec_init"), GU.group(g, "rec_init"), kind, torch.from_numpy(g["enc"]), torch.from_numpy(g["targets"]),
            int(g["meta_drop_seed"]))


def _right(family, pair):
    key = (family, pair)
    if key not in _cache:
        decP, recP, kind, enc, targets, seed = _inputs(family, pair)
        _cache[key] = oracle_grads_no_reg(decP, recP, kind, enc, targets, pair, seed)
    return _cache[key]


CASES = [(f, p) for f, (_, _, pairs) in FAMILIES.items() for p in pairs] + \
        [(n, {"lr_lstm_gru_global_chain": LG, "lr_gru_local_chain": GG, "lr_refcells_local_chain": GL}[n]) for n in UPDATE]


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
@pytest.mark.parametrize("family,pair", CASES, ids=["%s-%s" % (f, PAIR_ID[p]) for f, p in CASES])
def test_a_wrong_gru_in_one_cell_moves_a_gradient_far_beyond_the_bar(family, pair, mistake):
    decP, recP, kind, enc, targets, seed = _inputs(family, pair)
    right = _right(family, pair)
    for where, cell in (("dec", pair[0]), ("rec", pair[1])):
        if cell != "GRU":
            continue
        wrong = oracle_grads_no_reg(decP, recP, kind, enc, targets, pair, seed, mistake=mistake, where=where)
        e, k = worst_move(wrong, right)
        print("%s %s %s in %s: worst gradient move %.3f (%s); CE %.2e MSE %.2e" % (
            family, PAIR_ID[pair], mistake, where, e, k, abs(wrong["dec_ce"] - right["dec_ce"]) / abs(right["dec_ce"]),
            abs(wrong["rec_mse"] - right["rec_mse"]) / abs(right["rec_mse"])))
        assert e >= FACTOR * TOL_BF16_GRAD, (where, e, k)
        # a mistake in the reconstructor's cell cannot reach the decoder's loss; one in the decoder's reaches everything
        if where == "rec":
            assert wrong["dec_ce"] == right["dec_ce"]
