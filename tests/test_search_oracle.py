"""Pin the CPU restatement of eval.py's greedy / beam search against the reference's own outputs."""
import numpy as np
import pytest
import torch

from oracle import search_oracle as S
from tests.golden_util import CASES, load_search_case


@pytest.mark.parametrize("name", CASES)
def test_greedy_matches_reference(name):
    g, P, enc = load_search_case(name)
    with torch.no_grad():
        out = S.greedy_search(P, enc, cell=g["_cell"])
    assert np.array_equal(out, g["greedy"])


@pytest.mark.parametrize("bw", [1, 3, 5])
@pytest.mark.parametrize("name", CASES)
def test_beam_matches_reference(name, bw):
    g, P, enc = load_search_case(name)
    with torch.no_grad():
        out = S.beam_search(P, enc, bw, cell=g["_cell"])
    assert np.array_equal(out, g["beam%d" % bw])
