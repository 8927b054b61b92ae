"""Helpers shared by tests/golden/make_golden.py (the generator) and the tests that consume the
vectors: deterministic synthetic batches and formula-defined parameters that can be regenerated
on any box without the reference."""
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def make_batch(B, F, D, V, lens, seed, Tm=31):
    """Tm = caption_max_len + 1 rows of targets; the draws do not depend on it (tests/test_golden_util.py)."""
    g = torch.Generator().manual_seed(int(seed))
    enc = torch.randn(B, F, D, generator=g)
    targets = torch.zeros(int(Tm), B, dtype=torch.long)
    for b, L in enumerate(lens):
        L = int(L)
        targets[:L, b] = torch.randint(3, V, (L,), generator=g)
        targets[L, b] = 2
    return enc, targets


def formula_params(shapes, seed):
    """shapes: {state_dict key: shape}.  Keys visited in sorted order; U(-k,k), k = 1/sqrt(last dim)
    for matrices, 0.05 for vectors; embedding N(0,1)*0.5; attn_b ones."""
    g = torch.Generator().manual_seed(int(seed))
    out = {}
    for k in sorted(shapes.keys()):
        shp = tuple(shapes[k])
        if k == "attn_b":
            out[k] = torch.ones(shp)
        elif k == "embedding.weight":
            out[k] = torch.randn(shp, generator=g) * 0.5
        else:
            kk = 1.0 / np.sqrt(shp[-1]) if len(shp) > 1 else 0.05
            out[k] = (torch.rand(shp, generator=g) * 2 - 1) * kk
    return out


def decoder_shapes(V, E, H, A, D, cell="LSTM"):
    G = 4 if cell == "LSTM" else 3
    return {"attn_b": (A,), "embedding.weight": (V, E), "attn_W.weight": (A, H), "attn_U.weight": (A, D),
            "attn_w.weight": (1, A), "rnn.weight_ih_l0": (G * H, E + D), "rnn.weight_hh_l0": (G * H, H),
            "rnn.bias_ih_l0": (G * H,), "rnn.bias_hh_l0": (G * H,), "out.weight": (V, H), "out.bias": (V,)}


def rec_shapes(kind, H, R, A, cell="LSTM"):
    G = 4 if cell == "LSTM" else 3
    s = {}
    if kind == "local":
        s.update({"attn_b": (A,), "attn_W.weight": (A, R), "attn_U.weight": (A, H), "attn_w.weight": (1, A)})
    s.update({"rnn.weight_ih_l0": (G * R, H if kind == "local" else 2 * H), "rnn.weight_hh_l0": (G * R, R),
              "rnn.bias_ih_l0": (G * R,), "rnn.bias_hh_l0": (G * R,), "out.weight": (R, R), "out.bias": (R,)})
    return s


def cells_of(g):
    """(decoder cell, reconstructor cell) of a golden case; cases written before GRU support are LSTM/LSTM."""
    mc = g.get("meta_cells")
    if mc is None:
        return ("LSTM", "LSTM")
    return tuple("GRU" if int(x) else "LSTM" for x in mc)


def caption_max_len_of(g):
    """config.py:50 caption_max_len of a golden case; cases written before it was varied are at the reference's 30."""
    return int(g["meta_caption_max_len"]) if "meta_caption_max_len" in g else 30


def load(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    return {k: z[k] for k in z.files}


CASES = ["search_small", "search_small_b", "search_eos", "search_stop", "search_gru", "search_gru_b", "search_gru_stop"]


def search_params(dims, seed, scale, eos_bias, pad_bias, cell):
    """The decoder parameters of a search case: formula_params at `seed`, out.* times `scale` (peaked distributions: few near-ties),
    then the <EOS> / <PAD> biases.  dims = (B, F, D, V, E, H, A)."""
    B, F, D, V, E, H, A = [int(x) for x in dims]
    P = formula_params(decoder_shapes(V, E, H, A, D, cell), int(seed))
    sc = float(scale)
    P["out.weight"] = P["out.weight"] * sc
    P["out.bias"] = P["out.bias"] * sc
    P["out.bias"][2] += float(eos_bias)
    P["out.bias"][0] += float(pad_bias)
    return P


def load_search_case(name):
    """(golden, decoder parameters, features) of one of the search goldens (CASES), or of a shape case of tests/search_shapes.py
    (SHAPES, REF_SHAPES): those have no .npz behind them — g holds the meta_* entries and _cell only, the features are randn(B, F, D) from
    Generator(seed + 50)."""
    from tests.search_shapes import REF_SHAPES, SHAPES
    if name in SHAPES or name in REF_SHAPES:
        c = SHAPES[name] if name in SHAPES else REF_SHAPES[name]
        g = {"meta_dims": np.array(c["dims"], dtype=np.int64), "meta_seed": np.int64(c["seed"]), "meta_scale": np.float64(c["scale"]),
             "meta_eos_bias": np.float64(c["eos_bias"]), "meta_pad_bias": np.float64(c["pad_bias"]), "_cell": c["cell"]}
        B, F, D = c["dims"][:3]
        enc = torch.randn(B, F, D, generator=torch.Generator().manual_seed(int(c["seed"]) + 50))
    else:
        g = load(name)
        g["_cell"] = cells_of(g)[0]
        enc = torch.from_numpy(g["enc"])
    P = search_params(g["meta_dims"], g["meta_seed"], g["meta_scale"], g["meta_eos_bias"], g["meta_pad_bias"], g["_cell"])
    return g, P, enc


RECSTEP_CASES = ["recstep_global_eval", "recstep_global_train", "recstep_local_eval", "recstep_local_train",
                 "recstep_global_gru", "recstep_local_gru"]


def load_recstep_case(name):
    """(golden, dims, kind, cell, reconstructor parameters, seeded decoder hiddens [T, 1, B, H]) of one of RECSTEP_CASES."""
    g = load(name)
    B, T, F, H, R, RA = [int(x) for x in g["meta_dims"]]
    kind = "global" if "global" in name else "local"
    cell = "GRU" if int(g["meta_gru"]) else "LSTM"
    P = formula_params(rec_shapes(kind, H, R, RA, cell), int(g["meta_seed"]))
    gen = torch.Generator().manual_seed(int(g["meta_seed"]) + 50)
    hid = torch.tanh(torch.randn(T, 1, B, H, generator=gen)) * 0.6
    return g, (B, T, F, H, R, RA), kind, cell, P, hid


def group(g, prefix):
    """{'key': tensor} for every entry 'prefix/key'."""
    n = len(prefix) + 1
    return {k[n:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith(prefix + "/")}
