"""Times the sampling search with and without a nucleus cut, and the greedy search beside them, on one handle (DESIGN.md sections 8
and 13): recnet_sample_search at top_k 0 and 50, recnet_sample_search_nucleus at top_p 0.9 (alone and behind top_k 50) and at top_p 1
(the nucleus kernel with its select skipped), at the benchmark's decoder shape, bf16, and the row kernel alone on random logits.
HIP events around `reps` back-to-back calls after `warmup` calls of each; the calls are alternated over `rounds` rounds so that drift
hits them alike; the median and the spread over rounds are printed as one JSON line.

    python tools/sample_time.py [--B 100 --F 28 --D 1536 --V 4188 --reps 10 --warmup 3 --rounds 5 --nucleus 1]
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
    for k, v in (("B", 100), ("F", 28), ("D", 1536), ("E", 468), ("H", 512), ("A", 128), ("V", 4188), ("reps", 10), ("warmup", 3),
                 ("rounds", 5), ("nucleus", 1)):
        ap.add_argument("--" + k, type=int, default=v)
    ap.add_argument("--precision", default="bf16")
    a = ap.parse_args()
    import recnet_amd as R
    from recnet_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("sample_time.py needs a GPU: a CPU run says nothing about these times")
    torch.manual_seed(0)
    dec = R.Decoder("LSTM", 1, a.D, a.E, 1, a.H, a.A, a.V, 0.5, 0.5, 0.5, precision=a.precision).cuda().eval()
    eng = Engine(dec.dims(a.B, a.F), None, a.precision, dec.hyper(), device="cuda")
    eng.bind_decoder({k: v.data for k, v in dec.named_tensors().items()})
    eng.pack_weights()
    enc = torch.randn(a.B, a.F, a.D, device="cuda")
    logits = torch.randn(a.B, a.V, device="cuda") * 2.0
    calls = {"greedy_search": lambda: eng.greedy_search(enc),
             "sample_search": lambda: eng.sample_search(enc, 1.0, 0, 1),
             "sample_search_k50": lambda: eng.sample_search(enc, 1.0, 50, 1),
             "sample_rows": lambda: eng.sample_rows(logits, 1.0, 0, 1, 3),
             "sample_rows_k50": lambda: eng.sample_rows(logits, 1.0, 50, 1, 3)}
    if a.nucleus:                        # (--nucleus 0: the call set of section 8, for a like-for-like run against an older commit)
        calls.update({"sample_search_p0.9": lambda: eng.sample_search_nucleus(enc, 1.0, 0, 0.9, 1),
                      "sample_search_k50_p0.9": lambda: eng.sample_search_nucleus(enc, 1.0, 50, 0.9, 1),
                      "sample_search_nucleus_p1": lambda: eng.sample_search_nucleus(enc, 1.0, 0, 1.0, 1),
                      "sample_rows_p0.9": lambda: eng.sample_rows_nucleus(logits, 1.0, 0, 0.9, 1, 3),
                      "sample_rows_k50_p0.9": lambda: eng.sample_rows_nucleus(logits, 1.0, 50, 0.9, 1, 3)})
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
    out = {"shape": {k: getattr(a, k) for k in ("B", "F", "D", "E", "H", "A", "V")}, "precision": a.precision, "reps": a.reps,
           "rounds": a.rounds}
    if a.nucleus:
        out["mean_n_allowed_p0.9"] = float(eng.sample_rows_nucleus(logits, 1.0, 0, 0.9, 1, 3)[2].float().mean().item())
    for k, v in ms.items():
        out[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
