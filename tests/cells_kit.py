"""Shared by tests/test_cells_ref.py (CPU) and tests/test_gpu_cells.py: the cell pairs, the parameters of a cell-matrix case and
the three named GRU mistakes applied to ONE cell of the oracle."""
import numpy as np
import torch

from oracle import recnet_oracle as O
from tests import golden_util as GU

GG, GL, LG = ("GRU", "GRU"), ("GRU", "LSTM"), ("LSTM", "GRU")
PAIR_ID = {GG: "GG", GL: "GL", LG: "LG"}

# The GRU cells' bias vectors are scaled by this in every cell-matrix case and in the three update-path goldens of this matrix.  At the
# standard formula_params (biases in +-0.05) the gates sit near 1/2 and "z and 1 - z exchanged" in the RECONSTRUCTOR's cell alone moves
# no gradient tensor by more than 0.05 ... 0.19 at the local, hybrid and update-path inputs (tests/test_cells_ref.py asks for 0.2).
BIAS_SCALE = 10.0


def cell_params(dims, kind, cells, bias_scale=BIAS_SCALE):
    """formula_params at the seeds of the edge tests (31 / 32); bias_scale multiplies the GRU cells' bias vectors."""
    B, F, D, V, E, H, A, RA = dims
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D, cells[0]), 31)
    recP = GU.formula_params(GU.rec_shapes(kind, H, D, RA, cells[1]), 32)
    if bias_scale != 1.0:
        for P, cell in ((decP, cells[0]), (recP, cells[1])):
            if cell == "GRU":
                for k in ("rnn.bias_ih_l0", "rnn.bias_hh_l0"):
                    P[k] = P[k] * bias_scale
    return decP, recP


def _gates(x, h, w_ih, w_hh, b_ih):
    gi = x @ w_ih.t() + b_ih
    gh = h @ w_hh.t()
    return gi.chunk(3, dim=1), gh.chunk(3, dim=1)


def bias_outside(x, h, w_ih, w_hh, b_ih, b_hh):
    """b_hn added outside the r * (W_hn h) product."""
    (ir, iz, in_), (hr, hz, hn) = _gates(x, h, w_ih, w_hh, b_ih)
    br, bz, bn = b_hh.chunk(3)
    r = torch.sigmoid(ir + hr + br)
    z = torch.sigmoid(iz + hz + bz)
    n = torch.tanh(in_ + r * hn + bn)
    return (1.0 - z) * n + z * h


def z_exchanged(x, h, w_ih, w_hh, b_ih, b_hh):
    """z and 1 - z exchanged in the state update."""
    (ir, iz, in_), (hr, hz, hn) = _gates(x, h, w_ih, w_hh, b_ih)
    br, bz, bn = b_hh.chunk(3)
    r = torch.sigmoid(ir + hr + br)
    z = torch.sigmoid(iz + hz + bz)
    n = torch.tanh(in_ + r * (hn + bn))
    return z * n + (1.0 - z) * h


def r_on_all(x, h, w_ih, w_hh, b_ih, b_hh):
    """r gating the whole candidate pre-activation."""
    (ir, iz, in_), (hr, hz, hn) = _gates(x, h, w_ih, w_hh, b_ih)
    br, bz, bn = b_hh.chunk(3)
    r = torch.sigmoid(ir + hr + br)
    z = torch.sigmoid(iz + hz + bz)
    n = torch.tanh(r * (in_ + hn + bn))
    return (1.0 - z) * n + z * h


MISTAKES = {"bias_outside": bias_outside, "z_exchanged": z_exchanged, "r_on_all": r_on_all}


def oracle_grads_no_reg(decP, recP, kind, enc, targets, cells, seed=6, mistake=None, where=None):
    """CE, MSE and every gradient of the oracle without the regulariser (as tests/test_gpu_parity.py's hybrid test takes them).
    mistake / where: one of MISTAKES applied to the GRU cell of `where` ("dec" or "rec") alone — the cell function is told apart by
    the recurrent weight it is handed."""
    st = O.TrainState(decP, recP, kind, cell=cells[0], rec_cell=cells[1], dec_lambda_reg=0.0, rec_lambda_reg=0.0)
    good = O.gru_cell
    if mistake is not None:
        target = (st.dec if where == "dec" else st.rec)["rnn.weight_hh_l0"]
        wrong = MISTAKES[mistake]
        O.gru_cell = lambda x, h, w_ih, w_hh, b_ih, b_hh: (wrong if w_hh is target else good)(x, h, w_ih, w_hh, b_ih, b_hh)
    try:
        dl, rl, hid, ce, mse = st.losses(enc, targets, targets > 0, O.Dropper("hash", seed=seed))
        (dl + rl).backward()
    finally:
        O.gru_cell = good
    return dict(dec_ce=float(ce), rec_mse=float(mse), dec_grad={k: v.grad.numpy().copy() for k, v in st.dec.items()},
                rec_grad={k: v.grad.numpy().copy() for k, v in st.rec.items()})


def worst_move(a, b):
    """Largest ||a - b|| / ||b|| over the gradient tensors of two oracle_grads_no_reg results."""
    out = (0.0, None)
    for grp in ("dec_grad", "rec_grad"):
        for k, v in b[grp].items():
            e = float(np.linalg.norm((a[grp][k] - v).astype(np.float64)) / max(np.linalg.norm(v.astype(np.float64)), 1e-12))
            if e > out[0]:
                out = (e, grp[:3] + "." + k)
    return out
