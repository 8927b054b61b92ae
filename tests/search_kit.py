"""What the search tests share (a plain module: no fixtures): the config and the decoder of a search golden with its start state,
engines of a test's own, the guard that shows a check comes before the library, bit-equality of op outputs, and the statistics the
sampling tests hold their draws to."""
import functools
import math
import sys

import torch

import recnet_amd as R
from tests import nucleus_ref as NR
from tests import sample_ref as SR
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
