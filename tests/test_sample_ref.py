"""The sampling draw without a GPU: the CPU restatement (tests/sample_ref.py) samples the distribution it claims to, its
top_k = 1 form is the reference's greedy search, the near-tie exclusion stays inside its caps for every case the GPU tests
compare, sequence_logprob, and the boundary's argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import search_oracle as S
from tests import sample_ref as SR
from tests.golden_util import CASES, load_search_case
from tests.search_kit import chi2_quantile_1m1e6, no_library, step0_logits


@pytest.mark.parametrize("top_k", [0, 5])
def test_restated_sampler_samples_the_softmax(top_k):
    """Pearson chi^2 of >= 20 000 draws (all rows of search_small_b's step-0 logits, (seed, t) varied) against softmax(logits),
    resp. against the renormalised five largest with no token outside them."""
    lg = step0_logits()
    B, V = lg.shape
    assert V == 61
    n_calls = -(-20000 // B)
    counts = np.zeros((B, V))
    for i in range(n_calls):
        tok, _, _ = SR.sample_rows(lg, 1.0, top_k, seed=1 + i % 97, t=i // 97)
        counts[np.arange(B), tok] += 1
    assert counts.sum() >= 20000
    ok = SR.allowed_mask(lg, top_k)
    p = np.where(ok, np.exp(lg.astype(np.float64) - lg.max(axis=1, keepdims=True)), 0.0)
    p /= p.sum(axis=1, keepdims=True)
    assert (counts[~ok] == 0).all()                              # nothing outside the allowed set is ever drawn
    dof = (top_k or V) - 1
    bar = chi2_quantile_1m1e6(dof)
    for b in range(B):
        e = n_calls * p[b][ok[b]]
        chi2 = float(((counts[b][ok[b]] - e) ** 2 / e).sum())
        print("row", b, "chi2", chi2, "bar", bar, "dof", dof)
        assert chi2 < bar, (b, chi2, bar)


@pytest.mark.parametrize("name", CASES)
def test_top_k_one_is_the_greedy_search(name):
    g, P, enc = load_search_case(name)
    for seed, temperature in ((1, 1.0), (5, 0.5)):
        toks, lps, margins, _ = SR.sample_search(P, enc, temperature, 1, seed, cell=g["_cell"])
        assert np.array_equal(toks, g["greedy"])
        assert (lps == 0.0).all() and np.isinf(margins).all()


def test_near_tie_exclusion_stays_inside_its_caps_for_the_search_runs():
    """At most one caption per run drops out of the token comparison (none for the seeds chosen)."""
    for name, seed, temperature, top_k in SR.SEARCH_RUNS:
        g, P, enc = load_search_case(name)
        toks, _, margins, _ = SR.sample_search(P, enc, temperature, top_k, seed, cell=g["_cell"])
        excluded = int((~SR.comparable(margins)).any(axis=0).sum())
        print(name, seed, temperature, top_k, "steps", toks.shape[0], "excluded", excluded, "least margin", margins.min())
        assert excluded <= 1, (name, seed, temperature, top_k, excluded)
        if name.endswith("_stop"):
            assert toks.shape[0] == 1 and margins.min() > 2


@pytest.mark.parametrize("V", SR.ROW_VS)
def test_near_tie_exclusion_stays_inside_its_caps_for_the_row_cases(V):
    """At most 2 % of the rows of the kernel-alone cases drop out."""
    n = near = 0
    for rows, quantised, top_k, temperature, t, seed in SR.row_cases(V):
        _, _, margins = SR.sample_rows(SR.row_logits(V, rows, quantised), temperature, top_k, seed, t)
        n += rows
        near += int((margins < SR.NEAR_TIE).sum())
    print("V", V, "rows", n, "near ties", near)
    assert near <= 0.02 * n, (V, near, n)


def test_allowed_set_takes_equal_values_lowest_index_first():
    x = np.array([[1.0, 2.0, 2.0, 0.0, 2.0, -0.0, 2.0]], dtype=np.float32)
    assert SR.allowed_mask(x, 3).tolist() == [[False, True, True, False, True, False, False]]
    assert SR.allowed_mask(x, 6).tolist() == [[True, True, True, True, True, False, True]]     # 0.0 before -0.0: equal, by index
    assert SR.allowed_mask(x, 0).all() and SR.allowed_mask(x, 7).all()


def test_sequence_logprob():
    from recnet_amd import sequence_logprob
    #          b0: EOS in the middle, b1: EOS at the last position, b2: none, b3: EOS at position 0
    tokens = [[5, 7, 9, 2], [2, 8, 9, 4], [6, 8, 9, 2], [7, 2, 9, 3]]
    lps = [[-1.0, -0.5, -0.25, -4.0], [-2.0, -0.5, -0.25, -8.0], [-16.0, -0.5, -0.25, -32.0], [-64.0, -0.5, -0.25, -128.0]]
    assert sequence_logprob(tokens, lps) == [-3.0, -2.0, -1.0, -4.0]
    assert sequence_logprob([], []) == []


# ---------------------------------------------------------------------------------------------- boundary
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from recnet_amd import _lib
    return _lib.load()


def test_sampling_entry_points_need_a_bound_workspace(lib):
    from recnet_amd import _lib
    c = _lib.Config()
    c.batch_size, c.encoder_output_len, c.encoder_output_size, c.embedding_size = 4, 5, 32, 12
    c.decoder_hidden_size, c.decoder_attn_size, c.n_vocabs, c.caption_max_len = 24, 8, 41, 30
    c.reconstructor_type, c.precision, c.global_batch_size = _lib.REC_NONE, _lib.PREC_F32, 4
    h = C.c_void_p()
    assert lib.recnet_create(C.byref(c), C.byref(h)) == 0
    assert lib.recnet_sample_rows(h, None, 1, 41, 1.0, 0, 0, 0, None, None, None) == -2
    assert b"workspace" in lib.recnet_last_error()
    assert lib.recnet_sample_search(h, None, 1.0, 0, 0, None, None, None, None) == -2
    assert b"workspace" in lib.recnet_last_error()
    lib.recnet_destroy(h)


@pytest.mark.parametrize("kw", [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")),
                                dict(temperature=float("inf")), dict(top_k=-1), dict(top_k=42), dict(top_k=2.5)])
def test_python_sample_search_checks_its_arguments_before_the_library(kw, monkeypatch):
    import recnet_amd as R
    no_library(monkeypatch)
    dec = R.Decoder("LSTM", 1, 32, 12, 1, 24, 8, 41, 0.5, 0.5, 0.5, precision="f32")
    inp = torch.full((1, 4), 1, dtype=torch.long)
    hid = (torch.zeros(1, 4, 24), torch.zeros(1, 4, 24))
    with pytest.raises(ValueError):
        R.sample_search(None, dec, inp, hid, torch.zeros(4, 5, 32), **kw)
