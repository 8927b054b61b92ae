"""Times caption scoring against the greedy search on one handle: score_captions with features, with
enc = NULL (invariants reused), and greedy_search, at the benchmark's decoder shape, bf16.  HIP events around `reps` back-to-back
calls after `warmup` calls of each; the three are alternated over `rounds` rounds so that drift hits them alike; the median and the
spread over rounds are printed as one JSON line.

    python tools/score_time.py [--B 100 --F 28 --D 1536 --V 4188 --T 31 --reps 20 --warmup 5 --rounds 5]
"""
import json

import torch

import _timing


def main():
    a = _timing.parser(reps=20, warmup=5, T=31).parse_args()
    eng = _timing.bound_engine(a, _timing.decoder(a, "score_time.py"))
    enc = torch.randn(a.B, a.F, a.D, device="cuda")
    toks = torch.randint(3, a.V, (a.T, a.B), device="cuda")
    calls = {"score_captions": lambda: eng.score_captions(enc, toks),
             "score_captions_enc_null": lambda: eng.score_captions(None, toks),
             "greedy_search": lambda: eng.greedy_search(enc)}
    n_chain = eng.profile_site(9, calls["score_captions"], 1)[0]
    ms = _timing.time_calls(a, calls)
    assert eng.chain_status() == 0
    out = {"shape": _timing.shape(a, "T"), "precision": a.precision,
           "persistent_chain_launches_per_score": n_chain, "reps": a.reps, "rounds": a.rounds}
    print(json.dumps(dict(out, **ms)))


if __name__ == "__main__":
    main()
