"""Times the consensus (minimum-Bayes-risk) reranking: recnet_consensus_rows alone on random caption sets at
the (N, T, B) of --shapes (self-consensus; lengths uniform in [T / 2, T], words from a 40-word vocabulary), the width-8 N-best
search without and with the rerank launched behind it (device time), search.best_of_beam without and with consensus_weight (host
wall time: it ends in read-backs), and the same candidates through the host restatement tests/consensus_ref.py with their
read-back included, at the benchmark's decoder shape, bf16.  HIP events around `reps` back-to-back calls after `warmup` calls of
each; the calls are alternated over `rounds` rounds so that drift hits them alike; the median and the spread over rounds are
printed as one JSON line.  Read the rerank against the search of the same run.

    python tools/consensus_time.py [--B 100 --F 28 --D 1536 --V 4188 --width 8 --shapes 8:31,16:31,32:64 --reps 10 --warmup 3 --rounds 5]
"""
import json
import time

import torch

import _timing


def random_captions(N, T, B, gen):
    """[N, T, B] int64: words 3..42, an <EOS> at a length uniform in [T / 2, T] (none at T), words and <EOS> behind it."""
    x = torch.randint(3, 43, (N, T, B), generator=gen)
    L = torch.randint(T // 2, T + 1, (N, 1, B), generator=gen)
    t = torch.arange(T).view(1, T, 1)
    return torch.where(t == L, torch.full_like(x, 2), x)


def main():
    ap = _timing.parser(reps=10, warmup=3, width=8, host_runs=3)
    ap.add_argument("--shapes", default="8:31,16:31,32:64")
    ap.add_argument("--length_alpha", type=float, default=0.7)
    ap.add_argument("--consensus_weight", type=float, default=0.5)
    a = ap.parse_args()
    import recnet_amd as R
    from recnet_amd import search
    from tests import consensus_ref as CR
    dec = _timing.decoder(a, "consensus_time.py")
    gen = torch.Generator().manual_seed(0)

    class Cfg:
        caption_max_len, decoder_model, batch_size = 30, "LSTM", a.B
    enc = torch.randn(a.B, a.F, a.D, device="cuda")
    inp = torch.full((1, a.B), 1, dtype=torch.long, device="cuda")
    hid = (torch.zeros(1, a.B, a.H, device="cuda"), torch.zeros(1, a.B, a.H, device="cuda"))
    eng = search._consensus_engine(enc.device)
    eng_s = search._nbest_engine(Cfg, dec, enc)          # the searches' own engine: its call does not wait for n_steps
    nbest = lambda: eng_s.beam_search_nbest(enc, a.width, a.length_alpha)[0]
    calls = {}
    for N, T in ([int(x) for x in s.split(":")] for s in a.shapes.split(",")):
        caps = random_captions(N, T, a.B, gen).cuda()
        calls["consensus_rows_N%d_T%d" % (N, T)] = lambda caps=caps: eng.consensus_rows(caps)
    calls["beam_search_nbest_w%d" % a.width] = nbest
    calls["beam_search_nbest_w%d_then_consensus_rows" % a.width] = lambda: eng.consensus_rows(nbest())
    ms = _timing.time_calls(a, calls, lambda k: 20 if k.startswith("consensus_rows") else 1)
    # the public call, host wall time (it ends in read-backs and builds Python lists)
    wall = {"best_of_beam_w%d" % a.width: 0.0, "best_of_beam_w%d_consensus" % a.width: a.consensus_weight}
    for k, cw in list(wall.items()):
        runs = []
        for i in range(a.warmup + a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            R.best_of_beam(Cfg, dec, inp, hid, enc, a.width, a.length_alpha, consensus_weight=cw)
            runs.append((time.perf_counter() - t0) * 1e3)
        wall[k] = runs[a.warmup:]
    # the host restatement on the search's own candidates, their read-back included
    toks = nbest()
    torch.cuda.synchronize()
    host = []
    for _ in range(a.host_runs):
        t0 = time.perf_counter()
        ref = CR.consensus(toks.cpu().numpy())["util"]
        host.append((time.perf_counter() - t0) * 1e3)
    dev_util = eng.consensus_rows(toks).cpu().numpy()
    out = {"shape": _timing.shape(a), "precision": a.precision, "width": a.width,
           "length_alpha": a.length_alpha, "reps": a.reps, "rounds": a.rounds, "search_steps": int(toks.shape[1]),
           "device_minus_host_max_abs": float(abs(dev_util - ref).max())}
    out.update(ms)
    for k, v in [(k + "_wall", v) for k, v in wall.items()] + [("host_restatement_with_readback_wall", host)]:
        out[k + "_ms"] = _timing.summary(v)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
