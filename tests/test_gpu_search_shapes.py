"""The device-side searches at the shapes of tests/search_shapes.py, where the decode step (csrc/abi_search.inc: dec_step) selects
the kernels no golden reaches: the ring GEMM past one row tile or past four k-tiles per slice, three and four slabs, the vector cell
kernel with three unit blocks, the generic cell kernel at 1024 threads with frames past 32, its plain attention loop, A % 4 != 0,
and every loop over B past 256.  Which kernels a case selects is recorded in SHAPES and held as integers by
tests/test_search_shapes_ref.py, which also holds the caps on near-ties of the runs compared here.

a. the decode step through Decoder.forward against oracle.recnet_oracle.decoder_step, both precisions, at the bars of
   tests/test_gpu_parity.py::test_step_api_matches_reference;
b. the N-best search against tests/beam_ref.py on the fp32 path (the body of tests/test_gpu_beam.py, search_kit);
c. self-consistency in both precisions (the same): it depends on no near-tie and carries the bf16 path;
d. greedy_search against the width-1 restatement on the fp32 path, up to each caption's first near-tie or <EOS>; and the
   reference-form beam search (recnet_beam_search) against oracle.search_oracle.beam_search: captions without a near-tie in full,
   the others up to their first near-tie, and for every caption what depends on no near-tie.
Every test prints its worst error / bar or the number of decisions it compared."""
import functools

import numpy as np
import pytest
import torch

import recnet_amd as R
from recnet_amd import search
from oracle import recnet_oracle as O
from tests import beam_ref as BR
from tests import search_shapes as SS
from tests.gpu_util import TOL
from tests.search_kit import check_nbest_against_restatement, check_self_consistency, decoder_for

pytestmark = pytest.mark.gpu

STEPS = 3


# ------------------------------------------------------------------------------------------------ a. the decode step
@functools.lru_cache(maxsize=None)
def _step_reference(name):
    """(tokens fed at steps 1.., and per step the oracle's logits, h, c or None), computed once for both precisions."""
    g, P, enc = SS.case(name)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B, V, H = int(g["meta_dims"][0]), int(g["meta_dims"][3]), int(g["meta_dims"][5])
    fed = torch.randint(3, V, (STEPS, B), generator=torch.Generator().manual_seed(int(g["meta_seed"]) + 77))
    tok, hid, out = torch.full((1, B), O.SOS, dtype=torch.long), O.zero_hidden(B, H, g["_cell"]), []
    with torch.no_grad():
        for t in range(STEPS):
            logits, hid = O.decoder_step(P, tok, hid, enc, cell=g["_cell"], t=t)
            h, c = (hid, None) if g["_cell"] == "GRU" else hid
            out.append((logits.numpy(), h[0].numpy(), None if c is None else c[0].numpy()))
            tok = fed[t].view(1, -1)
    return fed, out


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(SS.SHAPES))
def test_decode_step_matches_the_oracle(name, prec):
    """Three steps of Decoder.forward in eval mode from <SOS> / the zero state on fixed tokens in [3, V), the state fed back from the
    device: h within TOL[prec]["hid"], c within twice that, logits within hid * 4 * max(1, max |logit|)."""
    g, P, enc = SS.case(name)
    fed, ref = _step_reference(name)
    dec, cfg, tok, hid = decoder_for(g, P, prec)
    encd, gru, hb = enc.cuda(), g["_cell"] == "GRU", TOL[prec]["hid"]
    worst = dict(h=0.0, c=0.0, logits=0.0)
    abs_logit = 0.0
    with torch.no_grad():
        for t in range(STEPS):
            logits, hid = dec(tok, hid, encd)
            tok = fed[t].view(1, -1).cuda()
            rl, rh, rc = ref[t]
            worst["h"] = max(worst["h"], float(np.abs((hid if gru else hid[0])[0].cpu().numpy() - rh).max()) / hb)
            if not gru:
                worst["c"] = max(worst["c"], float(np.abs(hid[1][0].cpu().numpy() - rc).max()) / (2 * hb))
            e = float(np.abs(logits.cpu().numpy() - rl).max())
            abs_logit = max(abs_logit, e)
            worst["logits"] = max(worst["logits"], e / (hb * 4 * max(1.0, float(np.abs(rl).max()))))
    print(name, prec, "rows", enc.shape[0], "worst error / bar: h %.3g c %.3g logits %.3g ; worst |logit error| %.3g at max |logit| %.1f"
          % (worst["h"], worst["c"], worst["logits"], abs_logit, max(float(np.abs(r[0]).max()) for r in ref)))
    assert worst["h"] <= 1.0 and worst["c"] <= 1.0 and worst["logits"] <= 1.0, worst
    # the near-tie threshold of the searches stays 10 x above the fp32 path's logit error (tests/search_shapes.py: STEP_LOGIT_ERR)
    assert prec != "f32" or 10 * abs_logit <= BR.NEAR_TIE, abs_logit


# ------------------------------------------------------------------------------------------------ b. the N-best search
@pytest.mark.parametrize("name,bw,cml,cap", SS.NBEST_RUNS)
def test_nbest_matches_the_restatement(name, bw, cml, cap):
    check_nbest_against_restatement(name, bw, cml, SS.nbest_run(name, bw, cml))


# ------------------------------------------------------------------------------------------------ c. self-consistency
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(SS.SHAPES))
def test_self_consistency(name, prec):
    """Widths 3 and 8 (and 1 against greedy_search) over 31 steps; max |logit| for the row bar from the case's first N-best run."""
    run = next(r for r in SS.NBEST_RUNS if r[0] == name)
    check_self_consistency(name, prec, amax=SS.nbest_run(*run[:3])["amax"].max())


# ------------------------------------------------------------------------------------------------ d. greedy
@pytest.mark.parametrize("name", list(SS.SHAPES))
def test_greedy_matches_the_width_one_restatement(name):
    """fp32 path: the device's greedy tokens equal the width-1 restatement's at every step of a caption before its first near-tie
    decision (beam_ref.comparable_steps), up to and including its first <EOS> (greedy goes on behind it, the restatement carries
    <PAD>)."""
    g, P, enc = SS.case(name)
    r = SS.nbest_run(name, 1, SS.GREEDY_CML)
    ok, ref = BR.comparable_steps(r["margins"]), r["tokens"][0]                        # [n][B]
    dec, cfg, inp, hid = decoder_for(g, P, "f32")
    greedy = np.array(R.greedy_search(cfg, dec, inp, hid, enc.cuda()), dtype=np.int64)   # [n_dev][B]
    assert greedy.ndim == 2 and greedy.shape[1] == enc.shape[0]
    compared = 0
    for b in range(enc.shape[0]):
        eos = np.nonzero(ref[:, b] == BR.EOS)[0]
        upto = min(int(ok[:, b].sum()), int(eos[0]) + 1 if eos.size else ref.shape[0])
        assert greedy.shape[0] >= upto
        assert np.array_equal(greedy[:upto, b], ref[:upto, b]), (b, greedy[:ref.shape[0], b], ref[:, b])
        compared += upto
    print(name, "greedy decisions compared:", compared, "of", ref.size)
    assert compared > 0


@pytest.mark.parametrize("name,bw", SS.REFBEAM_RUNS)
def test_reference_beam_search_against_the_oracle(name, bw):
    """recnet_beam_search (beam_score_kernel, topk_rows_kernel, beam_update_kernel<false> with blockIdx.y = b, beam_gather_kernel) on
    an engine of caption_max_len = 7, fp32 path.  Against oracle.search_oracle.beam_search: a caption none of whose decisions is a
    near-tie equals the oracle's top-1; of any other the first t0 tokens (t0: its first near-tie) are the history of one of the
    oracle's beams after step t0 - 1, since the device's beams are those up to there and the final top-1 descends from one of them.
    On no near-tie depend: the shape (B, 8), tokens in [0, V), a second call gives the same bits, and width 1 on the same engine
    equals greedy_search up to each caption's first near-tie of the width-1 oracle (log(sigmoid(.)) is monotone; where it rounds
    two logits onto one score the oracle reports a near-tie).  Shares: tests/search_shapes.py: REFBEAM_SHARES."""
    g, P, enc = SS.case(name)
    r = SS.refbeam_run(name, bw)
    B, V = enc.shape[0], int(g["meta_dims"][3])
    dec, cfg, inp, hid = decoder_for(g, P, "f32", SS.REFBEAM_CML)
    encd = enc.cuda()
    eng = search._nbest_engine(cfg, dec, encd)
    best, n = eng.beam_search(encd, bw)
    best2, n2 = eng.beam_search(encd, bw)
    assert torch.equal(best, best2) and torch.equal(n, n2)
    n = int(n.item())
    best = best[:n].t().cpu().numpy()                                                  # [B][n]
    assert best.shape == (B, SS.REFBEAM_CML + 1) and n == r["n_steps"]                   # (the oracle's runs all go 8 steps)
    assert best.min() >= 0 and best.max() < V
    t0 = r["ok"].sum(axis=0)
    full = prefixes = 0
    for b in range(B):
        k = int(t0[b])
        if k == n:
            assert np.array_equal(best[b], r["best"][b]), (b, best[b], r["best"][b])
            full += 1
        elif k > 0:
            allowed = {tuple(h) for h in r["beams"][k - 1][:, b].tolist()}
            assert tuple(best[b, :k].tolist()) in allowed, (b, k, best[b], allowed)
            prefixes += k
    print(name, "width", bw, "captions compared in full:", full, "of", B, "; decisions compared through prefixes:", prefixes, "of", B * n)
    assert full == SS.REFBEAM_CAPTIONS[(name, bw)] and full * n + prefixes == int(r["ok"].sum())
    # width 1 against greedy_search on the same engine
    r1 = SS.refbeam_run(name, 1)
    w1, n1 = eng.beam_search(encd, 1)
    gr, ng = eng.greedy_search(encd)
    w1, gr, ng = w1[:int(n1.item())].cpu().numpy(), gr.cpu().numpy(), int(ng.item())   # [n][B]
    same = 0
    for b in range(B):
        k = min(int(r1["ok"][:, b].sum()), ng)
        assert np.array_equal(w1[:k, b], gr[:k, b]) and np.array_equal(w1[:k, b], r1["best"][b, :k]), (b, k, w1[:, b], gr[:, b])
        same += k
    print(name, "width 1 decisions equal to greedy_search and the oracle:", same, "of", B * n)
