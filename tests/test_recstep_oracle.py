"""The oracle's per-step reconstructor functions against goldens produced by the reference's own modules in the
reference's own time loops (tests/golden/make_golden_recstep.py; train.py:82-94, 112-123)."""
import numpy as np
import pytest

from oracle import recnet_oracle as O
from tests.golden_util import RECSTEP_CASES, load_recstep_case


@pytest.mark.parametrize("name", RECSTEP_CASES)
def test_oracle_step_functions_match_reference_loops(name):
    g, (B, T, F, H, R, RA), kind, cell, P, hid = load_recstep_case(name)
    drop = O.Dropper("hash", seed=int(g["meta_drop_seed"])) if int(g["meta_train_mode"]) else O.Dropper("eval")
    hidden = O.zero_hidden(B, R, cell)
    n = T if kind == "global" else F
    for t in range(n):
        if kind == "global":
            out, hidden = O.global_rec_step(P, hid[t], hidden, hid, cell=cell, drop=drop, t=t)
        else:
            out, hidden = O.local_rec_step(P, hidden, hid, cell=cell, drop=drop, t=t)
        h = (hidden[0] if cell == "LSTM" else hidden)[0]
        assert np.abs(out.numpy() - g["out"][t]).max() <= 2e-6, (name, t)
        assert np.abs(h.numpy() - g["h"][t]).max() <= 2e-6, (name, t)
        if cell == "LSTM":
            assert np.abs(hidden[1][0].numpy() - g["c"][t]).max() <= 2e-6, (name, t)
