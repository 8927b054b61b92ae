"""Times caption scoring against the greedy search on one handle: score_captions with features, with
enc = NULL (invariants reused), and greedy_search, at the benchmark's decoder shape, bf16.  HIP events around `reps` back-to-back
calls after `warmup` calls of each; the three are alternated over `rounds` rounds so that drift hits them alike; the median and the
spread over rounds are printed as one JSON line.

    python tools/score_time.py [--B 100 --F 28 --D 1536 --V 4188 --T 31 --reps 20 --warmup 5 --rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    for k, v in (("B", 100), ("F", 28), ("D", 1536), ("E", 468), ("H", 512), ("A", 128), ("V", 4188), ("T", 31), ("reps", 20),
                 ("warmup", 5), ("rounds", 5)):
        ap.add_argument("--" + k, type=int, default=v)
    ap.add_argument("--precision", default="bf16")
    a = ap.parse_args()
    import recnet_amd as R
    from recnet_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("score_time.py needs a GPU: a CPU run says nothing about these times")
    torch.manual_seed(0)
    dec = R.Decoder("LSTM", 1, a.D, a.E, 1, a.H, a.A, a.V, 0.5, 0.5, 0.5, precision=a.precision).cuda().eval()
    eng = Engine(dec.dims(a.B, a.F), None, a.precision, dec.hyper(), device="cuda")
    eng.bind_decoder({k: v.data for k, v in dec.named_tensors().items()})
    eng.pack_weights()
    enc = torch.randn(a.B, a.F, a.D, device="cuda")
    toks = torch.randint(3, a.V, (a.T, a.B), device="cuda")
    calls = {"score_captions": lambda: eng.score_captions(enc, toks),
             "score_captions_enc_null": lambda: eng.score_captions(None, toks),
             "greedy_search": lambda: eng.greedy_search(enc)}
    n_chain = eng.profile_site(9, calls["score_captions"], 1)[0]
    for fn in calls.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.reps)
    assert eng.chain_status() == 0
    out = {"shape": {k: getattr(a, k) for k in ("B", "F", "D", "E", "H", "A", "V", "T")}, "precision": a.precision,
           "persistent_chain_launches_per_score": n_chain, "reps": a.reps, "rounds": a.rounds}
    for k, v in ms.items():
        out[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
