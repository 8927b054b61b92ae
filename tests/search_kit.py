"""What the search tests share (a plain module: no fixtures): the config and the decoder of a search golden with its start state,
engines of a test's own, the guard that shows a check comes before the library, bit-equality of op outputs, the statistics the
sampling tests hold their draws to, and the two test bodies tests/test_gpu_beam.py shares with tests/test_gpu_search_shapes.py."""
import functools
import math
import sys

import numpy as np
import torch

import recnet_amd as R
from recnet_amd import search
from tests import beam_ref as BR
from tests import nucleus_ref as NR
from tests import sample_ref as SR
from tests import score_ref as SC
from tests.golden_util import load_search_case
from tests.gpu_util import TOL


class Cfg:
    caption_max_len = 30
    decoder_model = "LSTM"


def decoder_for(g, P, prec, cml=30):
    """(Decoder module on the device in eval mode, config, <SOS> input, zero hidden state) for the Python searches, from a search
    golden g (its meta_dims and _cell are read) and its parameters P."""
    B, F, D, V, E, H, A = [int(x) for x in g["meta_dims"]]
    cell = g["_cell"]
    dec = R.Decoder(cell, 1, D, E, 1, H, A, V, 0.5, 0.5, 0.5, precision=prec)
    dec.load_state_dict(P)
    dec = dec.cuda().eval()
    cfg = Cfg()
    cfg.batch_size, cfg.decoder_model, cfg.caption_max_len = B, cell, cml
    inp = torch.full((1, B), 1, dtype=torch.long, device="cuda")
    hid = (torch.zeros(1, B, H, device="cuda"), torch.zeros(1, B, H, device="cuda"))
    if cell == "GRU":
        hid = hid[0]                                     # a single tensor (eval.py:136-141)
    return dec, cfg, inp, hid


def bound_engine(dec, B, F, prec):
    """An engine of the test's own with the decoder's parameters bound and packed."""
    eng = R.engine.Engine(dec.dims(B, F), None, prec, dec.hyper(), device="cuda")
    eng.bind_decoder({k: v.data for k, v in dec.named_tensors().items()})
    eng.pack_weights()
    return eng


@functools.lru_cache(maxsize=None)
def rows_engine():
    """A handle for the kernel-alone entries (recnet_*_rows): it supplies the device only, no decoder is bound."""
    return R.engine.Engine.device_only()


def no_library(monkeypatch):
    """From here on loading the library fails the test: what still passes came before it."""
    def refuse(*a, **k):
        raise AssertionError("the library was loaded")
    # the package is importable under two names; patch every loaded copy of the two loader modules
    loaders = [m for n, m in list(sys.modules.items()) if n.endswith(("_amd._lib", "_amd._ops")) and m is not None]
    assert loaders
    for m in loaders:
        monkeypatch.setattr(m, "load", refuse)


def bits(outs):
    return [o.view(torch.int32) if o.dtype == torch.float32 else o for o in outs]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(bits(a), bits(b)))


def lp_bar(logit_abs_max, temperature):
    """The bar of one sampled log-probability: twice the per-step logits bar of the fp32 path, divided by the temperature."""
    return 2.0 * (TOL["f32"]["hid"] * 4 * max(1.0, float(logit_abs_max))) / temperature


def chi2_quantile_1m1e6(dof):
    """1 - 1e-6 quantile of chi^2(dof): scipy when present, else Wilson-Hilferty with z = 4.753424 (Phi(z) = 1 - 1e-6)."""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1.0 - 1e-6, dof))
    except ImportError:
        z = 4.753424
        return dof * (1.0 - 2.0 / (9.0 * dof) + z * math.sqrt(2.0 / (9.0 * dof))) ** 3


def step0_logits():
    """The restated step-0 logits [B, V] of search_small_b."""
    g, P, enc = load_search_case("search_small_b")
    B, H = enc.shape[0], P["rnn.weight_hh_l0"].shape[1]
    with torch.no_grad():
        logits, _ = SR.O.decoder_step(P, torch.full((1, B), 1, dtype=torch.long), SR.O.zero_hidden(B, H, g["_cell"]), enc,
                                      cell=g["_cell"], t=0)
    return logits.numpy()


@functools.lru_cache(maxsize=None)
def nucleus_row_sizes(V):
    """{(rows, quantised, top_k, temperature, top_p): nucleus_ref.nucleus_sizes} of the kernel-alone nucleus cases at vocabulary V."""
    out = {}
    for rows, quantised, top_k, temperature, top_p, t, seed in NR.row_cases(V):
        key = (rows, quantised, top_k, temperature, top_p)
        if key not in out:
            out[key] = NR.nucleus_sizes(SR.row_logits(V, rows, quantised), temperature, top_k, top_p)
    return out


def check_nbest_against_restatement(name, bw, cml, r=None):
    """The body of tests/test_gpu_beam.py::test_search_matches_the_restatement (its docstring says what is held), shared with
    tests/test_gpu_search_shapes.py.  r: beam_ref.beam_search_nbest(P, enc, bw, BR.LENGTH_ALPHA, cml, cell) of the case when the
    caller has it already."""
    g, P, enc = load_search_case(name)
    if r is None:
        r = BR.beam_search_nbest(P, enc, bw, BR.LENGTH_ALPHA, cml, g["_cell"])
    dec, cfg, inp, hid = decoder_for(g, P, "f32", cml)
    toks, cum, ln, score = search._beam_nbest(cfg, dec, inp, hid, enc.cuda(), bw, BR.LENGTH_ALPHA)
    toks, cum, ln, score = toks.cpu().numpy(), cum.cpu().numpy().astype(np.float64), ln.cpu().numpy(), score.cpu().numpy().astype(np.float64)
    keep = BR.comparable_captions(r)
    n = toks.shape[1]
    assert toks.shape == (bw, n, enc.shape[0]) and 1 <= n <= cml + 1
    if keep.all():
        assert n == r["n_steps"]
    m = min(n, r["n_steps"])
    assert np.array_equal(ln[:, keep], r["len"][:, keep])
    assert np.array_equal(toks[:, :m][:, :, keep], r["tokens"][:, :m][:, :, keep])
    assert (toks[:, m:][:, :, keep] == 0).all() and (r["tokens"][:, m:][:, :, keep] == 0).all()
    bar = r["len"] * SC.row_bar("f32", r["amax"].max(), 1.0)
    err = np.abs(cum - r["cum"])[:, keep]
    errs = np.abs(score - r["score"])[:, keep]
    worst = float((err / bar[:, keep]).max()) if err.size else 0.0
    print(name, "width", bw, "cml", cml, "steps", n, "captions compared", int(keep.sum()), "of", keep.size, "worst cum error / bar:", worst)
    assert (err <= bar[:, keep]).all() and (errs <= bar[:, keep]).all()
    # an excluded caption is compared up to its first near-tie decision t0: the beams after step t0 - 1 are the restatement's, and
    # every returned hypothesis descends from one of them, so its first t0 tokens are one of their histories
    t0 = BR.comparable_steps(r["margins"]).sum(axis=0)
    prefixes = 0
    for b in np.nonzero(~keep)[0]:
        k = int(t0[b])
        if k == 0:
            continue
        allowed = {tuple(h) for h in r["trace"][k - 1][3][:, b, :k].tolist()}
        for rank in range(bw):
            got = toks[rank, :k, b].tolist()
            got += [0] * (k - len(got))          # (a search that stopped earlier carries <PAD>)
            assert tuple(got) in allowed, (b, rank, k, got, allowed)
        prefixes += k
    print(name, "width", bw, "decisions compared through excluded captions' prefixes:", prefixes)
    assert keep.any() or prefixes > 0            # every run checks tokens on the device
    # the public list form of the same call
    hyps = R.beam_search_nbest(cfg, dec, inp, hid, enc.cuda(), bw, BR.LENGTH_ALPHA)
    assert len(hyps) == enc.shape[0] and all(len(h) == bw for h in hyps)
    for b, h in enumerate(hyps):
        for k, (t, c, l, s) in enumerate(h):
            assert l == ln[k, b] and t == toks[k, :l, b].tolist() and c == float(cum[k, b]) and s == float(score[k, b])


def check_self_consistency(name, prec, amax=None):
    """The body of tests/test_gpu_beam.py::test_self_consistency, shared with tests/test_gpu_search_shapes.py.  amax: max |logit| of
    the case for the row bar, when the caller has a restatement of it already (default: the width-3 restatement over 31 steps).
    Returns the worst error / bar."""
    g, P, enc = load_search_case(name)
    dec, cfg, inp, hid = decoder_for(g, P, prec)
    encd = enc.cuda()
    greedy = np.array(R.greedy_search(cfg, dec, inp, hid, encd), dtype=np.int64)      # [n][B]
    t1, _, l1, _ = search._beam_nbest(cfg, dec, inp, hid, encd, 1, 0.0)
    t1, l1 = t1.cpu().numpy()[0], l1.cpu().numpy()[0]
    for b in range(enc.shape[0]):
        n = min(greedy.shape[0], t1.shape[0])
        eos = np.nonzero(greedy[:n, b] == BR.EOS)[0]
        upto = int(eos[0]) + 1 if eos.size else n
        assert np.array_equal(t1[:upto, b], greedy[:upto, b]), (b, t1[:, b], greedy[:, b])
        assert l1[b] == (upto if eos.size else t1.shape[0])
    if amax is None:
        amax = BR.beam_search_nbest(P, enc, 3, 0.7, 30, g["_cell"])["amax"].max()
    worst = 0.0
    for bw in (3, 8):
        a = search._beam_nbest(cfg, dec, inp, hid, encd, bw, 0.7)
        b2 = search._beam_nbest(cfg, dec, inp, hid, encd, bw, 0.7)
        assert all(torch.equal(x, y) for x, y in zip(a, b2))
        toks, cum, ln, score = a
        assert (score[:-1] >= score[1:]).all()
        for k in range(bw):
            assert torch.equal(R.canonical_captions(toks[k]), toks[k])
            _, cap, sl = search._score(dec, encd, toks[k].contiguous(), 1.0, False)
            assert torch.equal(sl.cpu(), ln[k].cpu()), (k, sl, ln[k])
            bar = ln[k].cpu().numpy() * SC.row_bar(prec, amax, 1.0)
            err = np.abs(cap.cpu().numpy().astype(np.float64) - cum[k].cpu().numpy())
            worst = max(worst, float((err / bar).max()))
            assert (err <= bar).all(), (k, err, bar)
    print(name, prec, "worst |score_captions - cum| / (len x row bar):", worst)
    return worst
