"""Times the two beam searches and the greedy search on one handle: recnet_beam_search (the reference's
search: one decode step per beam, a score array, one arg-max pass per winner) against recnet_beam_search_nbest (all beams in one
batched step, the fused selection) at each width, greedy_search beside width 1, and the selection kernel alone at nb = 8 on
random logits, at the benchmark's decoder shape, bf16.  HIP events around `reps` back-to-back calls after `warmup` calls of each;
the calls are alternated over `rounds` rounds so that drift hits them alike; the median and the spread over rounds are printed as
one JSON line.  The selection kernel reads each logit three times (maximum, sum of exponentials, candidates): `select_bytes_read`
counts all three passes, `select_bytes_unique` the array once.  The `_constrained` rows are the same calls
with no_repeat_ngram = 2, min_length = 3 and two banned ids, the kernel alone at the last step (t = T - 1) on random histories over
a 4-letter alphabet: read them against the unconstrained rows of the same run.  --groups 8:2,8:4 adds the diverse form (DESIGN.md
section 14) at those (width, groups): the search and the grouped selection kernel alone at nb = width, penalty --penalty, beside
the plain selection at the same nb = width: read them against the plain rows of the same width.

    python tools/beam_time.py [--B 100 --F 28 --D 1536 --V 4188 --widths 1,5,8 --reps 10 --warmup 3 --rounds 5 --groups 8:2,8:4]
"""
import json

import torch

import _timing


def main():
    ap = _timing.parser(reps=10, warmup=3, constrained=1)
    ap.add_argument("--widths", default="1,5,8")
    ap.add_argument("--groups", default="")
    ap.add_argument("--penalty", type=float, default=0.5)
    ap.add_argument("--length_alpha", type=float, default=0.7)
    a = ap.parse_args()
    widths = [int(w) for w in a.widths.split(",")]
    eng = _timing.bound_engine(a, _timing.decoder(a, "beam_time.py"))
    enc = torch.randn(a.B, a.F, a.D, device="cuda")
    nb = 8
    logits = torch.randn(nb, a.B, a.V, device="cuda") * 2.0
    cum = -torch.rand(nb, a.B, device="cuda") * 6.0
    fin = torch.zeros(nb, a.B, dtype=torch.int32, device="cuda")
    Tm = eng.hyper["caption_max_len"] + 1
    hist = torch.randint(3, 7, (nb, a.B, Tm), device="cuda")
    con = dict(no_repeat_ngram=2, min_length=3, banned_tokens=(5, 9))
    calls = {"greedy_search": lambda: eng.greedy_search(enc)}
    for w in widths:
        calls["beam_search_w%d" % w] = lambda w=w: eng.beam_search(enc, w)
        calls["beam_search_nbest_w%d" % w] = lambda w=w: eng.beam_search_nbest(enc, w, a.length_alpha)
        if not a.constrained:            # (--constrained 0: the call set of section 11, for a like-for-like run against an older commit)
            calls["beam_select_rows_nb8_w%d" % w] = lambda w=w: eng.beam_select_rows(logits, cum, fin, w)
            continue
        calls["beam_search_nbest_constrained_w%d" % w] = lambda w=w: eng.beam_search_nbest(enc, w, a.length_alpha, **con)
        calls["beam_select_rows_nb8_w%d" % w] = lambda w=w: eng.beam_select_rows(logits, cum, fin, w)
        calls["beam_select_rows_constrained_nb8_w%d" % w] = lambda w=w: eng.beam_select_rows(logits, cum, fin, w, hist=hist, t=Tm - 1, **con)
    for w, G in ([int(x) for x in wg.split(":")] for wg in a.groups.split(",") if wg):
        calls["beam_search_nbest_diverse_w%d_g%d" % (w, G)] = lambda w=w, G=G: eng.beam_search_nbest_diverse(enc, w, a.length_alpha, G, a.penalty)
        calls["beam_select_rows_diverse_nb%d_w%d_g%d" % (w, w, G)] = lambda w=w, G=G: eng.beam_select_rows_diverse(logits[:w], cum[:w], fin[:w], w, G, a.penalty)
        calls["beam_select_rows_nb%d_w%d" % (w, w)] = lambda w=w: eng.beam_select_rows(logits[:w], cum[:w], fin[:w], w)
    ms = _timing.time_calls(a, calls, lambda k: 20 if k.startswith("beam_select") else 1)
    assert eng.chain_status() == 0
    out = {"shape": _timing.shape(a), "T": Tm, "constraints": {k: list(v) if isinstance(v, tuple) else v for k, v in con.items()},
           "precision": a.precision, "length_alpha": a.length_alpha, "reps": a.reps, "rounds": a.rounds, "groups": a.groups, "penalty": a.penalty,
           "select_bytes_unique": nb * a.B * a.V * 4, "select_bytes_read": 3 * nb * a.B * a.V * 4}
    print(json.dumps(dict(out, **ms)))


if __name__ == "__main__":
    main()
