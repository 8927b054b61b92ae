"""On-device greedy / beam search (recnet_greedy_search / recnet_beam_search through the Python mirror of
eval.py's signatures) against the reference's own outputs (tests/golden/search_*.npz) — exact token match in the
fp32 path; the bf16 path is checked for agreement on the tokens whose decision margin exceeds bf16 rounding."""
import numpy as np
import pytest
import torch

import recnet_amd as R
from tests.golden_util import CASES, load_search_case
from tests.search_kit import Cfg, decoder_for, rows_engine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", CASES)
def test_greedy_search_fp32_exact(name):
    g, P, enc = load_search_case(name)
    dec, cfg, inp, hid = decoder_for(g, P, "f32")
    out = R.greedy_search(cfg, dec, inp, hid, enc.cuda())
    assert np.array_equal(np.array(out, dtype=np.int64), g["greedy"])


@pytest.mark.parametrize("bw", [1, 3, 5])
@pytest.mark.parametrize("name", CASES)
def test_beam_search_fp32_exact(name, bw):
    g, P, enc = load_search_case(name)
    dec, cfg, inp, hid = decoder_for(g, P, "f32")
    out = R.beam_search(cfg, bw, None, dec, inp, hid, enc.cuda())
    assert np.array_equal(np.array(out, dtype=np.int64), g["beam%d" % bw])


@pytest.mark.parametrize("name", CASES)
def test_step_api_loop_equals_device_loop(name):
    """eval.py's own greedy loop driven through Decoder.forward (the per-step API, invariants cached) gives the
    same tokens as the fused device-side loop."""
    g, P, enc = load_search_case(name)
    dec, cfg, inp, hid = decoder_for(g, P, "f32")
    encd = enc.cuda()
    toks, tok, h = [], inp, hid
    with torch.no_grad():
        for t in range(31):
            logits, h = dec(tok, h, encd)
            top = logits.argmax(dim=1)
            tok = top.view(1, -1)
            toks.append(top.cpu().numpy())
            if t == 30 or bool((tok == 0).all()):
                break
    assert np.array_equal(np.stack(toks), g["greedy"])


def test_bf16_search_mostly_agrees():
    """bf16 MFMA operands flip near-tie argmax decisions (and everything downstream of a flip), so only the
    first two steps are compared and a minority of captions may differ."""
    g, P, enc = load_search_case("search_small")
    dec, cfg, inp, hid = decoder_for(g, P, "bf16")
    out = np.array(R.greedy_search(cfg, dec, inp, hid, enc.cuda()), dtype=np.int64)
    assert out.shape == g["greedy"].shape
    agree = (out[:2] == g["greedy"][:2]).mean()
    assert agree >= 0.75, agree


def test_device_feeder_delivers_batches_and_normalisers():
    """DeviceFeeder: pinned double-buffered H2D on a side stream; T and step weights from the host."""
    from recnet_amd import feed
    rng = np.random.RandomState(1)
    batches = []
    for i in range(5):
        lens = rng.randint(2, 12, size=6)
        caps = [feed.pad_caption(rng.randint(3, 50, size=L), 30) for L in lens]
        vids = [rng.randn(28, 16).astype(np.float32) for _ in lens]
        batches.append(feed.collate_batch(vids, caps, 6))
    n = 0
    for (enc, tg), (e, t, T, w) in zip(batches, feed.DeviceFeeder(iter(batches), "cuda", 30)):
        n += 1                                           # the device buffers are recycled: check while iterating
        assert np.array_equal(e.cpu().numpy(), enc) and np.array_equal(t.cpu().numpy(), tg)
        masks = tg > 0
        assert T == R.decode_len(masks) and np.allclose(w.cpu().numpy(), R.step_weights(masks, T))
    assert n == 5
    # rank shard: only captions [2,5) on the device, normalisers still global
    e, t, T, w = next(iter(feed.DeviceFeeder(iter(batches[:1]), "cuda", 30, shard=(2, 5))))
    assert tuple(e.shape) == (3, 28, 16) and np.array_equal(t.cpu().numpy(), batches[0][1][:, 2:5])
    assert np.allclose(w.cpu().numpy(), R.step_weights(batches[0][1] > 0, T))


# ids with equal output rows (weight and bias): 7 / 199 meet in different waves of a row's 256-thread workgroup, 9 / 265 = 9 + 256
# in one thread's strided walk
TIE_PAIRS = [(7, 199), (9, 265)]


@pytest.mark.parametrize("pair", TIE_PAIRS, ids=["waves", "thread"])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("cell", ["LSTM", "GRU"])
def test_equal_maxima_go_to_the_lowest_index(cell, prec, pair):
    """The tie rule of the searches' arg-max (block_argmax256) and of the beam selections: among equal values the lowest index wins.
    A random decoder whose output rows lo / hi are equal and lifted by +50 has the two as its row maximum at every step, bit-equal
    (the premise, asserted through the step API).  The greedy search and the reference beam search then emit lo everywhere.  In the
    N-best search the tie is exact across beams as well — every step's log-probability is 0 - logf(2): the other 298 terms vanish
    in the fp32 sum — so the order is the flat index beam * V + token: the step-0 selection keeps (lo, hi) in that order with equal
    values (beam_select_rows on the step-0 logits), and from step 1 on both survivors continue beam 0, so rank 0 is lo everywhere and
    rank 1 differs from it in its last token alone, hi, at the same cum."""
    B, F, D, E, H, A, V = 4, 5, 64, 16, 32, 16, 300
    lo, hi = pair
    torch.manual_seed(11)
    dec = R.Decoder(cell, 1, D, E, 1, H, A, V, 0.5, 0.5, 0.5, precision=prec)
    with torch.no_grad():
        for a, b in TIE_PAIRS:
            dec.out.weight[b] = dec.out.weight[a]
            dec.out.bias[b] = dec.out.bias[a]
        dec.out.bias[lo] += 50.0
        dec.out.bias[hi] += 50.0
    dec = dec.cuda().eval()
    cfg = Cfg()
    cfg.batch_size, cfg.decoder_model, cfg.caption_max_len = B, cell, 7
    enc = torch.randn(B, F, D, device="cuda")
    inp = torch.full((1, B), 1, dtype=torch.long, device="cuda")
    hid = torch.zeros(1, B, H, device="cuda")
    hid = hid if cell == "GRU" else (hid, hid.clone())
    # the premise: two steps of the step API, the second fed lo
    with torch.no_grad():
        logits0, h1 = dec(inp, hid, enc)
        logits1, _ = dec(torch.full((1, B), lo, dtype=torch.long, device="cuda"), h1, enc)
    for lg in (logits0, logits1):
        assert torch.equal(lg[:, lo].view(torch.int32), lg[:, hi].view(torch.int32))
        assert bool((lg.argmax(dim=1) == lo).all() | (lg.argmax(dim=1) == hi).all()) and float(lg[:, lo].min()) > 40.0
    # the rule
    greedy = np.array(R.greedy_search(cfg, dec, inp, hid, enc), dtype=np.int64)
    assert greedy.shape == (31, B) and (greedy == lo).all(), greedy
    best = np.array(R.beam_search(cfg, 2, None, dec, inp, hid, enc), dtype=np.int64)
    assert best.shape == (B, 31) and (best == lo).all(), best
    vals, idx = rows_engine().beam_select_rows(logits0[None].contiguous(), torch.zeros(1, B, device="cuda"),
                                               torch.zeros(1, B, dtype=torch.int32, device="cuda"), 2)
    assert torch.equal(vals[:, 0].view(torch.int32), vals[:, 1].view(torch.int32)), vals
    assert idx.cpu().tolist() == [[lo, hi]] * B, idx
    nbest = R.beam_search_nbest(cfg, dec, inp, hid, enc, 2)
    print(cell, prec, pair, "step-0 vals", vals[0].tolist(), "n-best of caption 0", nbest[0])
    for b in range(B):
        (t0, c0, l0, _), (t1, c1, l1, _) = nbest[b]
        assert t0 == [lo] * 8 and t1 == [lo] * 7 + [hi] and l0 == l1 == 8, nbest[b]
        assert np.float32(c0).tobytes() == np.float32(c1).tobytes(), (c0, c1)
