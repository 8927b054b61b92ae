"""Shared by tests/test_rounded_ref.py (CPU) and tests/test_gpu_rounded.py: the cases that hold the bf16 chain kernels to the
operand-rounded restatement (oracle/recnet_rounded.py), the compared quantities, and the named local mistakes."""
import time

import numpy as np
import torch

from oracle import recnet_rounded as RR
from tests import golden_util as GU
from tests.cells_kit import GG, GL, PAIR_ID, cell_params

LL = ("LSTM", "LSTM")
DIMS = {      # [B, F, D = R, V, E, H, A, RA], caption lengths: the rows of tests/test_gpu_parity.py's EDGE, EDGE_KSPLIT and HYBRID tables
    "H32_T2_one_hand_over": ([70, 3, 32, 29, 8, 32, 16, 16], [i % 2 for i in range(70)]),
    "H32_A16_persistent_decoder": ([100, 5, 48, 29, 8, 32, 16, 16], [(7 * i) % 9 for i in range(100)]),
    "H32_T31_longest": ([3, 3, 32, 29, 8, 32, 16, 16], [30, 7, 30]),
    "F33_one_extra_frame": ([7, 33, 64, 53, 12, 32, 128, 16], [9, 2, 5, 12, 1, 7, 3]),
    "H512_A128_one_chunk": ([9, 4, 32, 29, 8, 512, 128, 16], [3, 1, 4, 1, 5, 2, 6, 5, 3]),
    "GROUPS_B113_two_groups": ([113, 3, 64, 29, 8, 32, 16, 16], [(7 * i) % 9 for i in range(113)]),
    "B57_second_half_one_row": ([57, 3, 32, 29, 8, 24, 16, 16], [(5 * i) % 7 for i in range(57)]),
    "B100_two_row_halves": ([100, 3, 48, 29, 8, 24, 16, 16], [(7 * i) % 9 for i in range(100)]),
    "B112_R40_all_rows": ([112, 2, 40, 29, 8, 24, 16, 16], [(3 * i) % 6 for i in range(112)]),
    "LOC_R64_B100_RA24": ([100, 4, 64, 29, 8, 32, 16, 24], [(7 * i) % 9 for i in range(100)]),
    "LOC_R32_B20_RA8_T31": ([20, 2, 32, 29, 8, 32, 16, 8], [30] + [(3 * i) % 6 for i in range(19)]),
    "LOC_R128_B65_F1": ([65, 1, 128, 29, 8, 32, 16, 12], [(5 * i) % 7 for i in range(65)]),
    "LOC_R1024_B34_two_k_parts": ([34, 2, 1024, 29, 8, 64, 16, 16], [(5 * i) % 6 for i in range(34)]),
    "LOC_R2560_B20_hybrid": ([20, 2, 2560, 29, 8, 32, 16, 8], [(3 * i) % 6 for i in range(20)]),
    "LOC_R2560_H64_B20_big_backward": ([20, 3, 2560, 29, 8, 64, 16, 8], [(3 * i) % 6 for i in range(20)]),
}
RAGGED = ([7, 5, 88, 101, 18, 36, 20, 12], [9, 2, 5, 12, 1, 7, 4])      # test_fused_step_vs_oracle_ragged_shapes
FAMILY = {"decoder": ["H32_T2_one_hand_over", "H32_A16_persistent_decoder", "H32_T31_longest", "F33_one_extra_frame", "H512_A128_one_chunk",
                      "GROUPS_B113_two_groups"],
          "global": ["B57_second_half_one_row", "B100_two_row_halves", "B112_R40_all_rows"],
          "local": ["LOC_R64_B100_RA24", "LOC_R32_B20_RA8_T31", "LOC_R128_B65_F1", "LOC_R1024_B34_two_k_parts", "LOC_R2560_B20_hybrid",
                    "LOC_R2560_H64_B20_big_backward"]}
KIND = {"decoder": "global", "global": "global", "local": "local"}      # the decoder chains run in front of a global reconstructor
# (family, case, cell pair): LSTM / LSTM everywhere, GRU / GRU at the first shape of each family, the reference's pair at one local shape
GPU_CASES = [(f, c, LL) for f in ("decoder", "global", "local") for c in FAMILY[f]] + [(f, FAMILY[f][0], GG) for f in ("decoder", "global", "local")] + \
            [("local", "LOC_R32_B20_RA8_T31", GL)]
BATCH_SEED, DROP_SEED = 78, 6
QUANTITIES = ("loss", "hid", "grad", "slice", "elem")


def case_id(c):
    return "%s-%s-%s" % (c[0], c[1], PAIR_ID.get(c[2], "LL"))


def inputs(case, kind, pair):
    dims, lens = RAGGED if case == "RAGGED_B7" else DIMS[case]
    B, F, D, V, E, H, A, RA = dims
    if case == "RAGGED_B7":
        decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D, pair[0]), 11)
        recP = GU.formula_params(GU.rec_shapes(kind, H, D, RA, pair[1]), 12)
        enc, targets = GU.make_batch(B, F, D, V, lens, 77)
    else:
        decP, recP = cell_params(dims, kind, pair)
        enc, targets = GU.make_batch(B, F, D, V, lens, BATCH_SEED)
    return dims, lens, decP, recP, enc, targets


_RESTATED = {}


def restated(case, kind, pair, seed=DROP_SEED):
    """One float64 run of the rounded restatement per (case, kind, pair, seed), shared and never modified; (result, seconds)."""
    key = (case, kind, pair, seed)
    if key not in _RESTATED:
        dims, lens, decP, recP, enc, targets = inputs(case, kind, pair)
        t0 = time.time()
        r = RR.step_grads(decP, recP, kind, enc, targets, pair, seed)
        _RESTATED[key] = (r, time.time() - t0)
    return _RESTATED[key]


_PLAIN = {}


def plain_oracle(case, kind, pair, seed=DROP_SEED):
    """The unrounded fp32 oracle at the same inputs (CE, MSE, gradients without the regulariser, hidden states [T, B, H]); cached."""
    from oracle import recnet_oracle as O
    from tests.cells_kit import oracle_grads_no_reg
    key = (case, kind, pair, seed)
    if key not in _PLAIN:
        dims, lens, decP, recP, enc, targets = inputs(case, kind, pair)
        r = oracle_grads_no_reg(decP, recP, kind, enc, targets, pair, seed)
        st = O.TrainState(decP, recP, kind, cell=pair[0], rec_cell=pair[1], dec_lambda_reg=0.0, rec_lambda_reg=0.0)
        with torch.no_grad():
            hid = st.losses(enc, targets, targets > 0, O.Dropper("hash", seed=seed))[2]
        r["hiddens"] = hid.numpy()[:, 0].astype(np.float64)
        _PLAIN[key] = r
    return _PLAIN[key]


# ----------------------------------------------------------------------------- slices
def slices(grp, key, shape, dims, kind, cells):
    """Index tuples that cut a gradient tensor where different products (or different captions' rows) meet: rows of the embedding by
    token; the gate blocks of the rnn.* tensors — times the [:, :E] | [:, E:] windows of the decoder's weight_ih and the
    [:, :H] | [:, H:] windows of the global reconstructor's, which are different products; 16-row blocks of every other matrix."""
    B, F, D, V, E, H, A, RA = dims
    if key == "embedding.weight":
        return [(slice(v, v + 1),) for v in range(shape[0])]
    if key.startswith("rnn."):
        G = 3 if cells[0 if grp == "dec" else 1] == "GRU" else 4
        n = shape[0] // G
        rows = [slice(g * n, (g + 1) * n) for g in range(G)]
        cut = None
        if key == "rnn.weight_ih_l0" and grp == "dec":
            cut = E
        elif key == "rnn.weight_ih_l0" and kind == "global":
            cut = H
        if cut is None:
            return [(r,) for r in rows]
        return [(r, c) for r in rows for c in (slice(0, cut), slice(cut, shape[1]))]
    if len(shape) == 2 and shape[0] > 16:
        return [(slice(r, min(r + 16, shape[0])),) for r in range(0, shape[0], 16)]
    return [(slice(None),)]


def _norm(x):
    return float(np.linalg.norm(np.asarray(x, dtype=np.float64)))


def compare(got, ref, dims, kind, cells):
    """The compared quantities of `got` against `ref` (two results in the layout of recnet_rounded.step_grads; `hiddens` optional in
    got): dict quantity -> (worst value, where), and the skipped-slice counts per tensor {name: (skipped, slices)}.
      loss   relative error of CE and of MSE
      hid    max abs over the hidden states, per (t, b) row
      grad   ||d|| / ||g|| per gradient tensor
      slice  the same per slice (above).  A slice whose reference is exactly zero (an embedding row of a token no caption has) must be
             exactly zero in `got` as well — it counts as an infinite error otherwise — and a slice whose reference norm is below 1e-3
             of the tensor's largest slice is skipped and counted
      elem   the largest |d| of a tensor over its largest |g|"""
    out = {q: (0.0, None) for q in QUANTITIES}
    skipped = {}

    def put(q, v, where):
        if not v <= out[q][0]:
            out[q] = (float(v), where)

    put("loss", abs(got["dec_ce"] - ref["dec_ce"]) / abs(ref["dec_ce"]), "CE")
    if "rec_mse" in ref:
        put("loss", abs(got["rec_mse"] - ref["rec_mse"]) / abs(ref["rec_mse"]), "MSE")
    if got.get("hiddens") is not None:
        d = np.abs(np.asarray(got["hiddens"], dtype=np.float64).reshape(ref["hiddens"].shape) - ref["hiddens"]).max(axis=2)
        t, b = np.unravel_index(int(d.argmax()), d.shape)
        put("hid", d.max(), "h[t=%d, b=%d]" % (t, b))
    for grp in ("dec", "rec"):
        if grp + "_grad" not in ref:
            continue
        for k, g in ref[grp + "_grad"].items():
            a = np.asarray(got[grp + "_grad"][k], dtype=np.float64)
            name = grp + "." + k
            put("grad", _norm(a - g) / max(_norm(g), 1e-300), name)
            put("elem", np.abs(a - g).max() / max(np.abs(g).max(), 1e-300), name)
            sl = slices(grp, k, g.shape, dims, kind, cells)
            norms = [_norm(g[ix]) for ix in sl]
            top, nskip = max(norms), 0
            for ix, n in zip(sl, norms):
                if n == 0.0:
                    if _norm(a[ix]) != 0.0:
                        put("slice", float("inf"), "%s%s (reference exactly zero)" % (name, _ix(ix)))
                elif n < 1e-3 * top:
                    nskip += 1
                else:
                    put("slice", _norm(a[ix] - g[ix]) / n, name + _ix(ix))
            skipped[name] = (nskip, len(sl))
    return out, skipped


def _ix(ix):
    return "[" + ", ".join("%s:%s" % (s.start if s.start is not None else "", s.stop if s.stop is not None else "") for s in ix) + "]"


def skip_cap_ok(skipped):
    """At most 10 % of a tensor's slices may be skipped."""
    return [(k, n, m) for k, (n, m) in skipped.items() if n > 0.1 * m]


# ----------------------------------------------------------------------------- named local mistakes
def _at(name, **want):
    """mistake callable of recnet_rounded: (True, index) at the one place `want` names, None elsewhere."""
    idx = want.pop("idx")

    def mist(kind, **where):
        if kind != name or any(where.get(k) != v for k, v in want.items()):
            return None
        return (True, idx)
    return mist


# Each touches ONE caption at ONE step (or one element): what a slip in a hand-over panel, a stamp, a row half, a row group or the LDS
# frames would do.
# name -> (family whose bars apply, case, the mistake, proves).  proves: invisible to today's check AND at least 4 x over a new bar
# (tests/test_rounded_ref.py asserts both); the others are invisible to today's check and stay below 4 x the new bars of their family —
# the part of the gap this restatement does not close.
MISTAKES = {
    "hand_over_slip": ("global", "B100_two_row_halves", _at("hand_over_slip", t=3, idx=90), True),       # caption 90 at step 3 consumes h of step t - 2
    "rec_reads_zero": ("global", "B100_two_row_halves", _at("rec_reads_zero", idx=0), True),             # the reconstructor reads one element of hiddens[T - 1, b = 0] as zero
    "mask_t_plus_1": ("global", "B100_two_row_halves", _at("mask_t_plus_1", t=1, idx=64), True),          # caption 64's SITE_REC_INPUT mask of step 1 taken at step 2
    "stale_frame_weight": ("global", "B100_two_row_halves", _at("stale_frame_weight", t=4, idx=71), True),   # caption 71 at step 4 weighs frame F - 1 with step 3's energy
    "rec_hand_over_slip": ("global", "B57_second_half_one_row", _at("rec_hand_over_slip", t=2, idx=3), True),   # the reconstructor's chain: caption 3 at step 2 consumes hr of step t - 2
    "hand_over_slip_H32": ("decoder", "H32_A16_persistent_decoder", _at("hand_over_slip", t=3, idx=5), False),  # the same slip under the decoder family's bars
    "frame_left_out_F33": ("decoder", "F33_one_extra_frame", _at("frame_left_out", t=2, idx=3), False),    # frame F - 1 (the one served from LDS) left out of caption 3's sum at step 2
    "dwhh_row_missing": ("global", "B100_two_row_halves", _at("dwhh_row_missing", t=4, idx=17), False),   # row (t = 4, b = 17) missing from the deferred d W_hh
}
