"""TEST INFRASTRUCTURE ONLY — search cases without golden files, at the shapes that make the decode step of the device-side searches
(csrc/abi_search.inc: dec_step) select its OTHER kernels.  golden_util.load_search_case resolves the names of SHAPES like the names
of the search goldens: parameters by golden_util.search_params, features randn(B, F, D) from Generator(seed + 50).

Kernel selection on the bf16 path, as csrc/host_common.inc (gemm_slabs, launch_dec_cell) and csrc/gemm.hip (rn_pick_splitk,
rn_launch_gemm) decide it — restated in recurrent_plan / cell_plan below, and held as plain integers by
tests/test_search_shapes_ref.py so that an edit of a case cannot move it off its rule silently:
  recurrent product h . [W_hh ; W]^T: M = rows, N = 4H + A, K = H in 64-deep k-tiles, split <= 4.  rows <= 128 and <= 4 k-tiles per
    slice: gemm_chain_kernel (NKT 2 or 4); otherwise the 4-stage gemm_lds_kernel writing slabs.  The cell kernel sums S slabs.
  cell kernel: dec_cell_vec_kernel when H % 8 == 0, F <= 32, A <= 128 and A % 4 == 0, with ceil(H / 512) unit blocks; otherwise
    dec_cell_kernel with 4 x 64 / 128 / 256 threads (its fast attention loop needs A <= 128 and F <= 8 waves' worth of frames).
The fp32 path runs the register-tiled fp32 GEMM and dec_cell_kernel<float> at every shape; its k-tiles are 32 deep.

`python -m tests.search_shapes` prints what the tables at the end of the file record."""
import functools

import numpy as np

# name: dims = (B, F, D, V, E, H, A), the cell, the parameter recipe, widths = the beam widths the runs below use (3 and 8 are the
# widths of the self-consistency test on every case), and what the case exists for.  "seen": the recurrent-product and cell kernels a
# kernel trace of the case's bf16 step test and bf16 self-consistency test showed on an MI355X
SHAPES = {
    # width 5: 100 rows, chain GEMM (NKT 2), S = 3 (5 k-tiles in slices of 2: the S4 clamp of dec_cell_vec_kernel);
    # width 8: 160 rows, ring GEMM, a second row tile of 32 rows
    # seen: gemm_chain_kernel<1, 2, 1>, gemm_lds_kernel<false, false, 4, 1, 128> (width 8), dec_cell_vec_kernel<bf16>
    "rows160": dict(dims=(20, 5, 72, 97, 20, 320, 24), cell="LSTM", seed=611, scale=40.0, eos_bias=2.0, pad_bias=0.0, widths=(3, 5, 8)),
    "rows160_gru": dict(dims=(20, 5, 72, 97, 20, 320, 24), cell="GRU", seed=612, scale=40.0, eos_bias=2.0, pad_bias=0.0, widths=(3, 5, 8)),
    # the benchmark's decoder (MSVD).  width 8: 136 rows = one full row tile + 8, ring GEMM, S = 4, padded ldE (E = 468)
    # seen: gemm_chain_kernel<1, 2, 1>, gemm_lds_kernel<false, false, 4, 1, 128> (width 8), dec_cell_vec_kernel<bf16>; score_captions
    # runs dec_chain_kernel<false, true>
    "eval_msvd": dict(dims=(17, 28, 1536, 4188, 468, 512, 128), cell="LSTM", seed=626, scale=100.0, eos_bias=2.0, pad_bias=0.0, widths=(3, 5, 8)),
    "eval_msvd_gru": dict(dims=(17, 28, 1536, 4188, 468, 512, 128), cell="GRU", seed=622, scale=100.0, eos_bias=2.0, pad_bias=0.0, widths=(3, 8)),
    # MSR-VTT: F = 40 > 32: bf16 runs the generic dec_cell_kernel<bf16> with 1024 threads, frames 32..39 in its tail loop
    # seen: gemm_chain_kernel<1, 2, 1>, dec_cell_kernel<bf16>; score_captions runs dec_chain_kernel<true, false>
    "eval_msrvtt": dict(dims=(7, 40, 2048, 4188, 468, 512, 128), cell="LSTM", seed=631, scale=100.0, eos_bias=2.0, pad_bias=0.0, widths=(3, 8)),
    # H = 1032: three unit blocks of the vector kernel (the last of 8 units), 17 k-tiles (the last 8 deep) in slices of 5: ring GEMM
    # at <= 128 rows
    # seen: gemm_lds_kernel<false, false, 4, 1, 128> and no chain GEMM, dec_cell_vec_kernel<bf16>
    "H1032": dict(dims=(5, 6, 64, 61, 16, 1032, 16), cell="LSTM", seed=641, scale=40.0, eos_bias=2.0, pad_bias=0.0, widths=(3, 8)),
    "H1032_gru": dict(dims=(5, 6, 64, 61, 16, 1032, 16), cell="GRU", seed=642, scale=40.0, eos_bias=2.0, pad_bias=0.0, widths=(3, 8)),
    # A = 136 > 128 and F = 33 > 32: the generic kernel's plain attention loop (!fastA), one frame past 32
    # seen: gemm_chain_kernel<1, 2, 1>, dec_cell_kernel<bf16>
    "A136_F33": dict(dims=(6, 33, 64, 61, 16, 32, 136), cell="LSTM", seed=652, scale=40.0, eos_bias=2.0, pad_bias=0.0, widths=(3, 8)),
    # A = 18, not a multiple of 4: the generic kernel on bf16 (the vector kernel's 16-byte LDS stores need A % 4 == 0)
    # seen: gemm_chain_kernel<1, 2, 1>, dec_cell_kernel<bf16>
    "A18": dict(dims=(6, 5, 72, 97, 20, 40, 18), cell="LSTM", seed=654, scale=40.0, eos_bias=2.0, pad_bias=0.0, widths=(3, 8)),
    # B = 260: every loop over B past 256 (fill_i64, search_stop, caption_logprob, beam_gather, beam_update's blockIdx.y);
    # width 3: 780 rows, seven row tiles of the ring GEMM
    # seen: gemm_lds_kernel<false, false, 4, 1, 128> and no chain GEMM (the step test's 260 rows included), dec_cell_vec_kernel<bf16>
    "B260": dict(dims=(260, 3, 16, 29, 8, 16, 8), cell="LSTM", seed=671, scale=40.0, eos_bias=2.0, pad_bias=0.0, widths=(3, 8)),
    # the same with an <EOS> bias under which every hypothesis of all 260 captions finishes at step 1: search_stop_kernel's early end
    "B260_eos": dict(dims=(260, 3, 16, 29, 8, 16, 8), cell="LSTM", seed=654, scale=40.0, eos_bias=10.0, pad_bias=0.0, widths=(3, 8)),
}


def cdiv(a, b):
    return (a + b - 1) // b


def recurrent_plan(rows, B, H, A, bk=64, cap=4):
    """(k-tiles per slice, slab count S, kernel) of gemm_slabs(RN_TAG_DEC_FWD) on the bf16 path, line by line: rn_pick_splitk
    (chain = 1), halved while s slabs of rows x N floats exceed the handle's 32 B N, at least 2 asked for, rn_effective_splitk, then
    rn_launch_gemm's choice between the chain kernel and the ring kernel."""
    N = 4 * H + A
    tiles = cdiv(rows, 128) * cdiv(N, 128)
    nkt = cdiv(H, bk)
    s = 1
    while s * 2 <= cap and tiles * s * 2 <= 320 and nkt // (s * 2) >= 1:
        s *= 2
    slab_floats = 32 * B * N
    while s > 1 and s * rows * N > slab_floats:
        s >>= 1
    s = max(s, 2)
    nkt = max(nkt, 1)
    s = min(s, nkt)
    per = cdiv(nkt, s)
    S = cdiv(nkt, per)
    assert S * rows * N <= slab_floats                                  # what the launch writes fits the slabs
    return per, S, ("chain" if rows <= 128 and per <= 4 else "ring")


def cell_plan(F, H, A):
    """(kernel, unit blocks, threads) of launch_dec_cell on the bf16 path."""
    if H % 8 == 0 and F <= 32 and A <= 128 and A % 4 == 0:
        return "vec", cdiv(H, 512), 256
    uc = 256 if H >= 256 else (128 if H >= 128 else 64)
    return "generic", cdiv(H, uc), 4 * uc


LENGTH_ALPHA = 0.7
# ---- the N-best runs (tests/test_gpu_search_shapes.py: against beam_ref.beam_search_nbest on the fp32 path):
# (case, beam width, caption_max_len, cap on the share of compared decisions: beam_ref's, 3/4, and 1/2 at width 8)
NBEST_RUNS = [("rows160", 5, 7, 0.75), ("rows160", 8, 7, 0.5), ("rows160_gru", 5, 7, 0.75), ("rows160_gru", 8, 7, 0.5),
              ("eval_msvd", 5, 7, 0.75), ("eval_msvd", 8, 7, 0.5), ("eval_msvd_gru", 8, 7, 0.5), ("eval_msvd", 5, 30, 0.75),
              ("eval_msrvtt", 3, 7, 0.75), ("H1032", 3, 7, 0.75), ("H1032_gru", 3, 7, 0.75),
              ("A136_F33", 3, 7, 0.75), ("A18", 3, 7, 0.75), ("B260", 3, 7, 0.75),
              ("B260_eos", 3, 7, 0.75)]
# ---- the reference-form beam search (recnet_beam_search: beam_score_kernel, topk_rows_kernel, beam_update_kernel<false>) against
# oracle.search_oracle.beam_search on the fp32 path, on engines of caption_max_len = 7.  It scores by log(sigmoid(logit)), so its
# top candidates lie within NEAR_TIE of one another wherever the logits are large: the cases above (out.* scale 40 / 100, diverse
# tokens) compare few decisions, the *_s8 copies at the lowest scale compare more and emit few distinct tokens.  Both are run.
# The device returns the final top-1 alone: a caption without any near-tie is compared in full, another one up to its first
# near-tie t0 — its first t0 tokens are the history of one of the oracle's beams after step t0 - 1.
REF_SHAPES = {
    "rows160_s8": dict(SHAPES["rows160"], seed=613, scale=8.0),
    "eval_msvd_s8": dict(SHAPES["eval_msvd"], scale=8.0),
    "B260_s8": dict(SHAPES["B260"], scale=8.0),
}
REFBEAM_CML = 7
REFBEAM_RUNS = [(name, bw) for name in ("rows160", "rows160_s8", "eval_msvd", "eval_msvd_s8", "B260", "B260_s8") for bw in (3, 5)]
# ---- greedy_search against the width-1 restatement: every case, over the restatement's caption_max_len + 1 = 8 steps
GREEDY_CML = 7


@functools.lru_cache(maxsize=None)
def case(name):
    from tests.golden_util import load_search_case
    return load_search_case(name)


@functools.lru_cache(maxsize=None)
def nbest_run(name, bw, cml):
    """beam_ref.beam_search_nbest of a run, computed once per process and left unchanged."""
    import torch
    from tests import beam_ref as BR
    g, P, enc = case(name)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return BR.beam_search_nbest(P, enc, bw, LENGTH_ALPHA, cml, g["_cell"])


@functools.lru_cache(maxsize=None)
def refbeam_run(name, bw):
    """oracle.search_oracle.beam_search of a run with its margins and per-step beams, computed once per process and left unchanged:
    dict(best [B][n], margins [n][B], beams: per step the histories [bw][B][t + 1], ok: bool [n][B], the decisions of a caption
    before its first near-tie one — a gap of exactly 0 among the top bw + 1 scores counts as one here: log(sigmoid(.)) rounds
    neighbouring logits onto one value on one device and not on the other)."""
    import torch
    from oracle import search_oracle as SO
    from tests.beam_ref import NEAR_TIE
    g, P, enc = case(name)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    with torch.no_grad():
        best, margins, steps = SO.beam_search(P, enc, bw, REFBEAM_CML, g["_cell"], margins=True, beams=True)
    gap = np.stack([(top[:, :-1] - top[:, 1:]).min(axis=1) for _, top in steps])
    near = (margins < NEAR_TIE) | ~(gap >= NEAR_TIE)
    return dict(best=best, margins=margins, beams=[h for h, _ in steps], ok=~(np.cumsum(near, axis=0) > 0), n_steps=best.shape[1])


# share of compared decisions / captions without any near-tie, measured by the restatements (python -m tests.search_shapes)
RUN_SHARES = {("rows160", 5, 7): 1.000, ("rows160", 8, 7): 0.981, ("rows160_gru", 5, 7): 0.956, ("rows160_gru", 8, 7): 0.819,
              ("eval_msvd", 5, 7): 0.934, ("eval_msvd", 8, 7): 0.882, ("eval_msvd_gru", 8, 7): 0.787, ("eval_msvd", 5, 30): 0.806,
              ("eval_msrvtt", 3, 7): 0.875, ("H1032", 3, 7): 0.825, ("H1032_gru", 3, 7): 1.000, ("A136_F33", 3, 7): 0.938,
              ("A18", 3, 7): 1.000, ("B260", 3, 7): 0.983, ("B260_eos", 3, 7): 0.992}
RUN_CAPTIONS = {("rows160", 5, 7): 20, ("rows160", 8, 7): 17, ("rows160_gru", 5, 7): 17, ("rows160_gru", 8, 7): 14,
                ("eval_msvd", 5, 7): 13, ("eval_msvd", 8, 7): 11, ("eval_msvd_gru", 8, 7): 11, ("eval_msvd", 5, 30): 10,
                ("eval_msrvtt", 3, 7): 5, ("H1032", 3, 7): 4, ("H1032_gru", 3, 7): 5, ("A136_F33", 3, 7): 4, ("A18", 3, 7): 6,
                ("B260", 3, 7): 248, ("B260_eos", 3, 7): 258}
# greedy_search: share of the (step, caption) decisions of the width-1 restatement before a caption's first near-tie
GREEDY_SHARES = {"rows160": 1.000, "rows160_gru": 1.000, "eval_msvd": 1.000, "eval_msvd_gru": 0.985, "eval_msrvtt": 1.000, "H1032": 1.000,
                 "H1032_gru": 1.000, "A136_F33": 1.000, "A18": 1.000, "B260": 1.000, "B260_eos": 1.000}
# recnet_beam_search: share of the (step, caption) decisions before a caption's first near-tie / captions without any near-tie
REFBEAM_SHARES = {("rows160", 3): 0.294, ("rows160", 5): 0.156, ("rows160_s8", 3): 0.637, ("rows160_s8", 5): 0.369,
                  ("eval_msvd", 3): 0.000, ("eval_msvd", 5): 0.000, ("eval_msvd_s8", 3): 0.625, ("eval_msvd_s8", 5): 0.206,
                  ("B260", 3): 0.272, ("B260", 5): 0.187, ("B260_s8", 3): 0.654, ("B260_s8", 5): 0.431}
REFBEAM_CAPTIONS = {("rows160", 3): 0, ("rows160", 5): 0, ("rows160_s8", 3): 3, ("rows160_s8", 5): 0, ("eval_msvd", 3): 0, ("eval_msvd", 5): 0,
                    ("eval_msvd_s8", 3): 0, ("eval_msvd_s8", 5): 0, ("B260", 3): 3, ("B260", 5): 1, ("B260_s8", 3): 13, ("B260_s8", 5): 0}
# name: the worst |logit error| of the fp32 path over the 3 steps of tests/test_gpu_search_shapes.py::test_decode_step_matches_the_oracle
# as an MI355X printed it.  tests/test_search_shapes_ref.py holds NEAR_TIE at least 10 x above each.
STEP_LOGIT_ERR = {"rows160": 1.91e-06, "rows160_gru": 3.81e-06, "eval_msvd": 9.54e-06, "eval_msvd_gru": 1.53e-05, "eval_msrvtt": 8.58e-06,
                  "H1032": 2.38e-06, "H1032_gru": 2.86e-06, "A136_F33": 8.34e-07, "A18": 1.91e-06, "B260": 2.38e-06, "B260_eos": 1.91e-06}


if __name__ == "__main__":
    from tests import beam_ref as BR
    shares, caps, greedy = [], [], []
    for name, bw, cml, cap in NBEST_RUNS:
        r = nbest_run(name, bw, cml)
        keep = BR.comparable_captions(r)
        print(name, bw, cml, "steps", r["n_steps"], "share %.3f" % BR.compared_share(r), "captions compared", int(keep.sum()), "of", keep.size,
              "cap", cap, "amax %.1f" % r["amax"].max(), "distinct tokens", len(np.unique(r["tokens"])))
        shares.append('("%s", %d, %d): %.3f' % (name, bw, cml, BR.compared_share(r)))
        caps.append('("%s", %d, %d): %d' % (name, bw, cml, int(keep.sum())))
    for name in SHAPES:
        r = nbest_run(name, 1, GREEDY_CML)
        print("greedy", name, "steps", r["n_steps"], "share %.3f" % BR.compared_share(r), "distinct tokens", len(np.unique(r["tokens"])))
        greedy.append('"%s": %.3f' % (name, BR.compared_share(r)))
    rs, rc = [], []
    for name, bw in REFBEAM_RUNS:
        r = refbeam_run(name, bw)
        print("reference beam", name, bw, "steps", r["n_steps"], "share %.3f" % r["ok"].mean(), "captions in full", int(r["ok"].all(axis=0).sum()),
              "distinct tokens", len(np.unique(r["best"])))
        rs.append('("%s", %d): %.3f' % (name, bw, r["ok"].mean()))
        rc.append('("%s", %d): %d' % (name, bw, int(r["ok"].all(axis=0).sum())))
    print("REFBEAM_SHARES = {" + ", ".join(rs) + "}")
    print("REFBEAM_CAPTIONS = {" + ", ".join(rc) + "}")
    print("RUN_SHARES = {" + ", ".join(shares) + "}")
    print("RUN_CAPTIONS = {" + ", ".join(caps) + "}")
    print("GREEDY_SHARES = {" + ", ".join(greedy) + "}")
