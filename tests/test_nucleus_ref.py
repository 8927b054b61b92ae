"""The nucleus (top-p) cut without a GPU: the CPU restatement (tests/nucleus_ref.py) against a direct float64 computation and
against exact rational arithmetic on rows of equal values, the prefix property, a chi^2 test of the restated draw, the
conditions under which tests/test_gpu_nucleus.py compares the device with it, and the argument checks of the boundary."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from recnet_amd import search                   # (not `from recnet_amd.search import`: that would load a second copy of the module)
from tests import nucleus_ref as NR
from tests import sample_ref as SR
from tests.golden_util import load_search_case
from tests.search_kit import chi2_quantile_1m1e6, no_library, nucleus_row_sizes, step0_logits

_check_top_p = search._check_top_p              # (these tests belong to the feature: without it the module does not import)
TOP_PS = (1e-6, 0.05, 0.5, 0.9, 0.999, 1.0)


def _small_rows():
    """(name, row) for V in 1..12: Gaussian rows, rows quantised to multiples of 1/2 (equal values on every cut), all-equal rows."""
    rng = np.random.RandomState(7)
    for V in range(1, 13):
        yield "gauss", (rng.randn(V) * 2.0).astype(np.float32)
        yield "quantised", (np.round(rng.randn(V) * 2.0) / 2).astype(np.float32)
        yield "equal", np.full(V, rng.randn(), dtype=np.float32)


def _brute_force(x, temperature, top_k, top_p):
    """Sort, cumulative softmax in float64, first crossing.  Returns (n, the least distance of a cumulative share from top_p)."""
    k = len(x) if top_k == 0 else top_k
    xs = x[np.argsort(-x, kind="stable")][:k]
    s = (xs / np.float32(temperature)).astype(np.float32)
    d = (s - s.max()).astype(np.float32).astype(np.float64)
    share = np.cumsum(np.exp(d)) / np.exp(d).sum()
    p = float(np.float32(top_p))
    hit = np.nonzero(share >= p)[0]
    return (int(hit[0]) + 1 if hit.size else k), float(np.abs(share - p).min())


def test_restatement_against_a_direct_float64_computation():
    """Every small row, every top_k, temperatures 1 / 0.5 / 2: wherever no cumulative share lies within 1e-6 of top_p (the
    float32 exponential and the 2^-32 grain of the masses move a share by far less) the sizes are equal; everywhere the direct
    size lies in the band; top_p = 1 is |K|."""
    decided = total = 0
    for name, x in _small_rows():
        V = len(x)
        for top_k in range(0, V + 1):
            for temperature in (1.0, 0.5, 2.0):
                for top_p in TOP_PS:
                    n, n_lo, n_hi, b = (int(a[0]) if a.dtype != np.float64 else float(a[0])
                                        for a in NR.nucleus_sizes(x[None, :], temperature, top_k, top_p))
                    k = V if top_k == 0 else top_k
                    assert 1 <= n_lo <= n <= n_hi <= k, (name, x, top_k, temperature, top_p)
                    if top_p == 1.0:
                        assert n == n_lo == n_hi == k
                        continue
                    assert b <= NR.EPS / 2
                    nb, gap = _brute_force(x, temperature, top_k, top_p)
                    assert n_lo <= nb <= n_hi, (name, x, top_k, temperature, top_p, n, nb)
                    total += 1
                    if gap > 1e-6:
                        decided += 1
                        assert n == nb, (name, x, top_k, temperature, top_p, n, nb)
                    if top_p == 1e-6:
                        assert n == 1
    print("decided", decided, "of", total)
    assert decided >= 0.8 * total


@pytest.mark.parametrize("k", [1, 2, 3, 4, 6, 7, 12, 61])
def test_equal_values_are_admitted_by_exact_integer_arithmetic(k):
    """A row of equal values: every mass is 2^32, so n = ceil(float32(top_p) * k) in exact rational arithmetic — where a float
    cumulative sum such as 3 * (1 / 6) against 0.5 may land on either side.  The same holds for the top_k = k cut of a longer
    row whose entries at the cut are equal."""
    for top_p in (1e-6, 0.05, 0.25, 0.5, 0.75, 0.9, 0.999):
        want = max(1, math.ceil(Fraction(float(np.float32(top_p))) * k))
        x = np.full((1, k), -1.25, dtype=np.float32)
        assert int(NR.nucleus_sizes(x, 0.5, 0, top_p)[0][0]) == want, (k, top_p)
        longer = np.full((1, k + 5), -1.25, dtype=np.float32)
        assert int(NR.nucleus_sizes(longer, 2.0, k, top_p)[0][0]) == want, (k, top_p)
        mask = NR.prefix_mask(longer, [want])
        assert mask[0, :want].all() and not mask[0, want:].any()              # lowest indices first


def test_allowed_set_is_a_prefix_of_the_top_k_order():
    for V in (1, 61, 257):
        for quantised in (False, True):
            x = SR.row_logits(V, 7, quantised)
            for top_k in sorted({0, 1, 8, V - 1, V} & set(range(V + 1))):
                inside = SR.allowed_mask(x, top_k)
                k = V if top_k == 0 else top_k
                for top_p in TOP_PS:
                    n = NR.nucleus_sizes(x, 1.0, top_k, top_p)[0]
                    mask = NR.prefix_mask(x, n)
                    assert (n >= 1).all() and (mask.sum(axis=1) == n).all()
                    assert not (mask & ~inside).any()
                    if top_p == 1.0:
                        assert (n == k).all() and np.array_equal(mask, inside)
                    # a prefix: nothing outside the set is larger than, or equal to with a lower index than, something inside
                    for r in range(7):
                        od = NR.order(x[r:r + 1])[0]
                        assert mask[r, od[:n[r]]].all()


def test_top_p_one_is_the_draw_without_the_cut():
    x = SR.row_logits(257, 7, True)
    for top_k in (0, 8):
        a = NR.sample_rows(x, 0.5, top_k, 1.0, 3, 5)
        b = SR.sample_rows(x, 0.5, top_k, 3, 5)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_restated_draw_samples_the_renormalised_nucleus():
    """Pearson chi^2 of 20 000 draws of one row (row 0 of search_small_b's step-0 logits, tiled so that every copy has its own
    counters, (seed, t) varied) against the renormalised nucleus at top_p = 0.9; nothing outside it is ever drawn."""
    row = step0_logits()[0]
    copies, n_calls = 200, 100
    lg = np.tile(row, (copies, 1))
    V = row.shape[0]
    counts = np.zeros(V)
    for i in range(n_calls):
        tok = NR.sample_rows(lg, 1.0, 0, 0.9, seed=1 + i % 97, t=i // 97)[0]
        counts += np.bincount(tok, minlength=V)
    n = int(NR.nucleus_sizes(row[None, :], 1.0, 0, 0.9)[0][0])
    ok = NR.prefix_mask(row[None, :], [n])[0]
    assert 2 <= n < V and counts.sum() == copies * n_calls
    assert (counts[~ok] == 0).all()
    p = np.where(ok, np.exp(row.astype(np.float64) - row.max()), 0.0)
    p /= p.sum()
    e = copies * n_calls * p[ok]
    chi2 = float(((counts[ok] - e) ** 2 / e).sum())
    bar = chi2_quantile_1m1e6(n - 1)
    print("nucleus", n, "of", V, "chi2", chi2, "bar", bar, "least expected count", e.min())
    assert chi2 < bar


# ------------------------------------------------------------------------- the conditions of the GPU tests, held on the CPU
@pytest.mark.parametrize("V", SR.ROW_VS)
def test_row_cases_keep_the_rounding_bound_and_mostly_single_valued_bands(V):
    """b <= EPS / 2 on every row case, and at least 3/4 of the rows have n_lo == n_hi, so that the size check is exact there."""
    total = single = 0
    worst = 0.0
    for key, (n, n_lo, n_hi, b) in nucleus_row_sizes(V).items():
        assert (b <= NR.EPS / 2).all(), (V, key, b.max())
        assert ((1 <= n_lo) & (n_lo <= n) & (n <= n_hi)).all()
        worst = max(worst, float(b.max()))
        total += len(n)
        single += int((n_lo == n_hi).sum())
    print("V", V, "rows", total, "single-valued bands", single, "worst b / EPS", worst / NR.EPS)
    assert single >= 0.75 * total, (V, single, total)


@pytest.mark.parametrize("V", SR.ROW_VS)
def test_near_tie_exclusion_stays_inside_its_cap_for_the_row_cases(V):
    """At most 2 % of the rows drop out of the token comparison (sample_ref's cap), at the restatement's own sizes."""
    n = near = 0
    for rows, quantised, top_k, temperature, top_p, t, seed in NR.row_cases(V):
        size = nucleus_row_sizes(V)[(rows, quantised, top_k, temperature, top_p)][0]
        margins = NR.draw(SR.row_logits(V, rows, quantised), size, temperature, seed, t)[2]
        n += rows
        near += int((margins < SR.NEAR_TIE).sum())
    print("V", V, "rows", n, "near ties", near)
    assert near <= 0.02 * n, (V, near, n)


@pytest.mark.parametrize("name,seed,temperature,top_k,top_p", NR.SEARCH_RUNS)
def test_search_runs_exclude_no_caption(name, seed, temperature, top_k, top_p):
    g, P, enc = load_search_case(name)
    run = NR.sample_search(P, enc, temperature, top_k, top_p, seed, cell=g["_cell"])
    excluded = int((~NR.comparable(run)).any(axis=0).sum())
    print(name, seed, "steps", run["tokens"].shape[0], "excluded", excluded, "sizes", run["n"].min(), "..", run["n"].max(),
          "worst b / EPS", run["b"].max() / NR.EPS)
    assert excluded == 0
    assert (run["n_lo"] == run["n_hi"]).all() and (run["b"] <= NR.EPS / 2).all()
    if name.endswith("_stop"):
        assert run["tokens"].shape[0] == 1 and (run["n"] == 1).all()


# ---------------------------------------------------------------------------------------------- boundary
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from recnet_amd import _lib
    return _lib.load()


def test_nucleus_entry_points_need_a_bound_workspace(lib):
    from recnet_amd import _lib, _ops
    assert "sample_rows_nucleus" in _ops.OP_NAMES and "sample_search_nucleus" in _ops.OP_NAMES
    c = _lib.Config()
    c.batch_size, c.encoder_output_len, c.encoder_output_size, c.embedding_size = 4, 5, 32, 12
    c.decoder_hidden_size, c.decoder_attn_size, c.n_vocabs, c.caption_max_len = 24, 8, 41, 30
    c.reconstructor_type, c.precision, c.global_batch_size = _lib.REC_NONE, _lib.PREC_F32, 4
    h = C.c_void_p()
    assert lib.recnet_create(C.byref(c), C.byref(h)) == 0
    assert lib.recnet_sample_rows_nucleus(h, None, 1, 41, 1.0, 0, 0.9, 0, 0, None, None, None, None) == -2
    assert b"workspace" in lib.recnet_last_error()
    assert lib.recnet_sample_search_nucleus(h, None, 1.0, 0, 0.9, 0, None, None, None, None, None) == -2
    assert b"workspace" in lib.recnet_last_error()
    lib.recnet_destroy(h)


def test_python_accepts_every_top_p_in_range():
    for top_p in (1.0, 1, 1e-6, 0.9, np.float32(0.9), np.float64(0.5)):
        _check_top_p(top_p)


@pytest.mark.parametrize("top_p", [0.0, -0.1, 1.5, float("nan"), float("inf"), "0.9", None])
def test_python_checks_top_p_before_the_library(top_p, monkeypatch):
    import recnet_amd as R
    no_library(monkeypatch)
    dec = R.Decoder("LSTM", 1, 32, 12, 1, 24, 8, 41, 0.5, 0.5, 0.5, precision="f32")
    inp = torch.full((1, 4), 1, dtype=torch.long)
    hid = (torch.zeros(1, 4, 24), torch.zeros(1, 4, 24))
    with pytest.raises(ValueError, match="top_p"):
        R.sample_search(None, dec, inp, hid, torch.zeros(4, 5, 32), top_p=top_p)
    with pytest.raises(ValueError, match="top_p"):
        R.best_of_n(None, dec, inp, hid, torch.zeros(4, 5, 32), 2, top_p=top_p)
