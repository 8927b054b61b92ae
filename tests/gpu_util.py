"""Shared helpers for the -m gpu parity tests: build the product's models from golden / formula
parameters and compare against the CPU oracle."""
import numpy as np
import torch

import recnet_amd as R
from oracle import recnet_oracle as O
from tests import golden_util as GU

TOL = {
    # The parity bars of SURVEY.md §8d.  precision: loss rel, hidden-state abs, per-tensor gradient ||d||/||g||,
    # parameter abs after the optimiser steps.  Measured worst cases over the golden set (tools/parity_report.py):
    # f32 path: hidden 2.4e-7, loss 1.9e-7, gradient 6.8e-7; bf16 path: hidden 3.0e-3, loss 1.0e-5, gradient 7.3e-3.
    "f32": dict(loss=1e-5, hid=1e-5, grad=1e-4, param=2e-6, cos=0.999999),
    # bf16: 3 Adam steps of lr 1e-5: a sign flip of a tiny gradient moves a parameter by up to 2*lr per step
    "bf16": dict(loss=1e-3, hid=1e-2, grad=2e-2, param=6e-5, cos=0.9995),
}
# The bf16 chain kernels against the operand-rounded restatement in float64 (oracle/recnet_rounded.py; tests/test_gpu_rounded.py).
# FLOOR: the restatement in float32 with every contraction summed in chunks of 32, last chunk first, against itself in float64 — the
# worst over every case of the family (tests/rounded_kit.GPU_CASES) and the dropout seeds 6, 7, 8, measured by
# `python -m tests.test_rounded_ref`.  loss: CE / MSE relative; hid: hidden states, abs; grad: ||d|| / ||g|| per tensor; slice: the same
# per slice (rounded_kit.slices); elem: worst element over the tensor's largest.  What is left once both sides round the same values
# is which way a value on a rounding boundary falls: one flipped bf16 of P or h_t moves a gate by up to an ulp, so the floors grow with
# the number of rounded values per gradient row — the decoder's worst is H512_A128_one_chunk (9 captions, 73 k values of P), the local
# one's attn_W at R = 2560 with 20 captions.
ROUNDED_FLOOR = {
    "decoder": dict(loss=1.153e-5, hid=3.061e-4, grad=1.295e-3, slice=1.947e-3, elem=2.782e-3),
    "global": dict(loss=1.233e-7, hid=2.030e-6, grad=2.546e-4, slice=6.393e-4, elem=4.637e-4),
    "local": dict(loss=1.562e-7, hid=6.032e-5, grad=2.654e-3, slice=2.654e-3, elem=3.535e-3),
}
# The bars: 16 x the family's floor — the margin for what the CPU floor cannot contain (MFMA k-tiles, split-K slabs, the 4-wave LDS
# reduction, the fast exp / reciprocal forms), never read off the kernels — and never above today's bar for the same quantity.
TOL["bf16_rounded"] = {fam: {q: min(16.0 * v, TOL["bf16"].get(q, 1.0)) for q, v in fl.items()} for fam, fl in ROUNDED_FLOOR.items()}
REG_SLACK = 3e-4
# update-path bars at learning rates of 1e-2: ||(got - init) - (ref - init)|| / ||ref - init|| per tensor, and the same for the
# Adam moments.  An update that did not happen is an error of 1.0 (0.25 for one of four); bf16 operand rounding flips the sign of
# near-zero gradient elements, each of which moves its parameter by 2 lr instead of 0 in the first step.
LR_TOL = {"f32": dict(move=2e-3, m=1e-3, v=2e-3), "bf16": dict(move=8e-2, m=3e-2, v=6e-2)}


def moved(got, ref, init):
    d = np.linalg.norm((ref - init).astype(np.float64))
    return float(np.linalg.norm(((got - init) - (ref - init)).astype(np.float64)) / max(d, 1e-30)), d


def make_models(dims, kind, precision, decP, recP, device="cuda", batch=None, cells=("LSTM", "LSTM"), attn_normalize="none",
                **config):
    """config: further TrainConfig attributes (e.g. decoder_learning_rate, reconstructor_learning_rate)."""
    B, F, D, V, E, H, A, RA = dims
    C = R.make_config(batch_size=B, encoder_output_len=F, encoder_output_size=D, embedding_size=E,
                      decoder_hidden_size=H, decoder_attn_size=A, use_recon=kind is not None,
                      reconstructor_type=kind or "local", reconstructor_hidden_size=D,
                      reconstructor_attn_size=RA, precision=precision, device=device, decoder_model=cells[0],
                      reconstructor_model=cells[1], decoder_attn_normalize=attn_normalize, **config)
    dec = R.build_decoder(V, C)
    dec["model"].load_state_dict({k: v.clone() for k, v in decP.items()})
    rec = None
    if kind:
        rec = R.build_reconstructor(C)
        rec["model"].load_state_dict({k: v.clone() for k, v in recP.items()})
    return C, dec, rec


def load_case(name):
    g = GU.load(name)
    dims = [int(x) for x in g["meta_dims"]]
    B, F, D, V, E, H, A, RA = dims
    kind = "global" if "global" in name else ("local" if "local" in name else None)
    fs = int(g["meta_formula_seed"])
    cells = g["_cells"] = GU.cells_of(g)
    if fs >= 0:
        decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D, cells[0]), fs)
        recP = GU.formula_params(GU.rec_shapes(kind, H, D, RA, cells[1]), fs + 1) if kind else None
        enc, targets = GU.make_batch(B, F, D, V, g["meta_lens"], int(g["meta_batch_seed"]), Tm=GU.caption_max_len_of(g) + 1)
    else:
        decP, recP = GU.group(g, "dec_init"), (GU.group(g, "rec_init") if kind else None)
        enc, targets = torch.from_numpy(g["enc"]), torch.from_numpy(g["targets"])
    return g, dims, kind, decP, recP, enc, targets


def cosine(a, b):
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    return float(a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-300))


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12))


def oracle_grads(decP, recP, kind, enc, targets, train, seed, B_global=None, b_offset=0, cells=("LSTM", "LSTM"), caption_max_len=30):
    """Reference gradients (incl. the regulariser term) from the CPU oracle's autograd."""
    st = O.TrainState(decP, recP, kind, cell=cells[0], rec_cell=cells[1], caption_max_len=caption_max_len)
    drop = O.Dropper("hash", seed=seed) if train else O.Dropper("eval")
    masks = targets > 0
    dl, rl, hid, ce, mse = st.losses(enc, targets, masks, drop)
    loss = dl if rl is None else dl + rl
    loss.backward()
    out = dict(dec_loss=float(dl), dec_ce=float(ce), hiddens=hid.detach().numpy(),
               dec_grad={k: v.grad.numpy().copy() for k, v in st.dec.items()})
    if rl is not None:
        out.update(rec_loss=float(rl), rec_mse=float(mse),
                   rec_grad={k: v.grad.numpy().copy() for k, v in st.rec.items()})
    return out
