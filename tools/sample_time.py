"""Times the sampling search with and without a nucleus cut, and the greedy search beside them, on one handle (DESIGN.md sections 8
and 13): recnet_sample_search at top_k 0 and 50, recnet_sample_search_nucleus at top_p 0.9 (alone and behind top_k 50) and at top_p 1
(the nucleus kernel with its select skipped), at the benchmark's decoder shape, bf16, and the row kernel alone on random logits.
HIP events around `reps` back-to-back calls after `warmup` calls of each; the calls are alternated over `rounds` rounds so that drift
hits them alike; the median and the spread over rounds are printed as one JSON line.

    python tools/sample_time.py [--B 100 --F 28 --D 1536 --V 4188 --reps 10 --warmup 3 --rounds 5 --nucleus 1]
"""
import json

import torch

import _timing


def main():
    a = _timing.parser(reps=10, warmup=3, nucleus=1).parse_args()
    eng = _timing.bound_engine(a, _timing.decoder(a, "sample_time.py"))
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
    ms = _timing.time_calls(a, calls)
    out = {"shape": _timing.shape(a), "precision": a.precision, "reps": a.reps, "rounds": a.rounds}
    if a.nucleus:
        out["mean_n_allowed_p0.9"] = float(eng.sample_rows_nucleus(logits, 1.0, 0, 0.9, 1, 3)[2].float().mean().item())
    print(json.dumps(dict(out, **ms)))


if __name__ == "__main__":
    main()
