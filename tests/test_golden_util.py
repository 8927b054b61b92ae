"""CPU checks of the shared batch helper and of the property the caption-length tests lean on.

1. tests/golden_util.make_batch grew a keyword Tm (rows of targets = caption_max_len + 1).  The goldens and every seeded test
   depend on its generator order: at the default, and at Tm = 31 given explicitly, it returns the tensors it returned before the
   keyword existed (SHA-256 of the raw bytes, recorded from the function as it stood then), and a larger Tm only appends <PAD> rows.
2. Padding invariance of the oracle: the reference's loops stop at the first all-<PAD> row (train.py:66), so rows of <PAD> behind it
   change nothing — tests/test_gpu_vocab_length.py compares engines built for caption_max_len up to 60 with the oracle on
   such padded batches."""
import hashlib

import numpy as np
import pytest
import torch

from oracle import recnet_oracle as O
from tests import golden_util as GU
from tests.gpu_util import oracle_grads

# (B, F, D, V, lens, seed): smoke()'s batch and a decoder-sized vocabulary with an empty and two full-length captions
BEFORE = [
    ((6, 5, 64, 61, [5, 2, 7, 3, 1, 4], 9),
     "1c79c7f5f439d9c17d04fa94199e9480b11571e2f9f0e3771d48e79aab1e864b", "315576c21591d6f5b9ecaece9440ea51d9235dd58d30c9bdc1278932d627234b"),
    ((8, 3, 32, 4188, [30, 1, 0, 12, 7, 30, 2, 5], 17),
     "2ad7e70fb1f15d3c4f3ec95cf8398f0b0ad0aeec945262045d41120f1531f5b8", "4a1ee7d5115139e43c0c190d6daad6640e2aba4590e078c55ca2a3d97ff12661"),
]


def _sha(t):
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("args,enc_sha,tgt_sha", BEFORE)
def test_make_batch_is_unchanged_at_31_rows(args, enc_sha, tgt_sha):
    for kw in ({}, {"Tm": 31}):
        enc, targets = GU.make_batch(*args, **kw)
        assert tuple(targets.shape) == (31, args[0]) and targets.dtype == torch.long and enc.dtype == torch.float32
        assert _sha(enc) == enc_sha and _sha(targets) == tgt_sha
    enc61, tg61 = GU.make_batch(*args, Tm=61)
    assert _sha(enc61) == enc_sha
    assert tuple(tg61.shape) == (61, args[0]) and _sha(tg61[:31].contiguous()) == tgt_sha and not bool(tg61[31:].any())


def _equal(a, b):
    assert a["dec_loss"] == b["dec_loss"] and np.array_equal(a["hiddens"], b["hiddens"])
    for k in a["dec_grad"]:
        assert np.array_equal(a["dec_grad"][k], b["dec_grad"][k]), k
    if "rec_loss" in a:
        assert a["rec_loss"] == b["rec_loss"]
        for k in a["rec_grad"]:
            assert np.array_equal(a["rec_grad"][k], b["rec_grad"][k]), k


@pytest.mark.parametrize("kind", [None, "global", "local"])
def test_oracle_is_invariant_to_pad_rows(kind):
    """Losses, hidden states and every gradient of a batch with 31 target rows against the same captions padded to 61 rows, bit
    for bit, train mode with dropout.  The decoder and the local reconstructor never read caption_max_len beyond the loop
    bound: they are compared across caption_max_len 30 / 60.  The global reconstructor scales its pooled input by
    caption_max_len / T (global_reconstructor.py:37), a property of the model and not of the padding: it is compared at
    one caption_max_len for both row counts, and its decoder half across 30 / 60 as well."""
    dims = [6, 3, 32, 61, 8, 32, 16, 16]
    B, F, D, V, E, H, A, RA = dims
    lens = [30, 4, 0, 11, 2, 9]
    decP = GU.formula_params(GU.decoder_shapes(V, E, H, A, D), 3)
    recP = GU.formula_params(GU.rec_shapes(kind, H, D, RA), 4) if kind else None
    enc, t31 = GU.make_batch(B, F, D, V, lens, 9)
    enc61, t61 = GU.make_batch(B, F, D, V, lens, 9, Tm=61)
    assert torch.equal(enc, enc61) and torch.equal(t61[:31], t31) and not bool(t61[31:].any())
    a = oracle_grads(decP, recP, kind, enc, t31, True, 5, caption_max_len=30)
    assert a["hiddens"].shape[0] == 31
    if kind == "global":
        _equal(a, oracle_grads(decP, recP, kind, enc, t61, True, 5, caption_max_len=30))
        b = oracle_grads(decP, recP, kind, enc, t61, True, 5, caption_max_len=60)
        assert a["dec_loss"] == b["dec_loss"] and np.array_equal(a["hiddens"], b["hiddens"])
        assert a["rec_loss"] != b["rec_loss"]           # the rescale is there: 30 / T against 60 / T
    else:
        _equal(a, oracle_grads(decP, recP, kind, enc, t61, True, 5, caption_max_len=60))
    # a short batch as well: the loop leaves at the first all-<PAD> row, far from either bound
    _, s31 = GU.make_batch(B, F, D, V, [5, 2, 0, 3, 1, 4], 9)
    _, s61 = GU.make_batch(B, F, D, V, [5, 2, 0, 3, 1, 4], 9, Tm=61)
    c = oracle_grads(decP, recP, kind, enc, s31, True, 5, caption_max_len=30)
    assert c["hiddens"].shape[0] == 6
    _equal(c, oracle_grads(decP, recP, kind, enc, s61, True, 5, caption_max_len=30 if kind == "global" else 60))
    assert O.decode_len(s61 > 0, 60) == 6 and O.decode_len(t61 > 0, 60) == 31
