"""Times the stochastic beam search on one handle, beside what it is read against: at each width
recnet_stochastic_beam_search, recnet_beam_search_nbest (the same loop with the deterministic selection) and one recnet_sample_search
rollout (`width` of them give as many candidates); the selection kernel alone at nb = 8 on random logits beside beam_select_kernel; and
the reranker, search.best_of_n(n) as n rollouts and n scoring passes against best_of_n(n, distinct=True), one search of width n, each
with its read-backs (wall time of the host call: that is what a user of best_of_n waits for).  At the benchmark's decoder shape, bf16.
The method of tools/beam_time.py: HIP events around `reps` back-to-back calls after `warmup` calls of each, alternated over `rounds`
rounds, the median and the spread over rounds, one JSON line.  --distinct 1 also counts, on the parameters of the shape case
eval_msvd (tests/search_shapes.py), the different captions per video among the n candidates of the two rerankers.
A commit without the stochastic search (--sbs 0) runs the rows that exist there, for the parent's side of the comparison.

    python tools/sbs_time.py [--B 100 --F 28 --D 1536 --V 4188 --widths 1,5,8 --n 8 --reps 10 --warmup 3 --rounds 5 --distinct 1]
"""
import json
import statistics
import time

import torch

import _timing


class _Cfg:
    caption_max_len = 30
    decoder_model = "LSTM"


def _wall_ms(fn, warmup, rounds):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def _distinct_counts(n, temperature, seed, sbs):
    """Mean / min different captions per video among n candidates on eval_msvd's parameters: n rollouts, and one search of width n."""
    import recnet_amd as R
    from tests.golden_util import load_search_case
    from tests.search_kit import decoder_for
    g, P, enc = load_search_case("eval_msvd")
    dec, cfg, inp, hid = decoder_for(g, P, "bf16")
    encd = enc.cuda()
    B = enc.shape[0]

    def cut(col):
        return tuple(col[:col.index(2) + 1]) if 2 in col else tuple(col)
    rolls = [R.sample_search(cfg, dec, inp, hid, encd, temperature, 0, seed + k)[0] for k in range(n)]
    per = [len({cut([step[b] for step in r]) for r in rolls}) for b in range(B)]
    out = {"rollouts": {"mean": statistics.mean(per), "min": min(per)}}
    if sbs:
        hyps = R.stochastic_beam_search(cfg, dec, inp, hid, encd, n, temperature, seed)
        per = [len({tuple(h[0]) for h in hb}) for hb in hyps]
        out["stochastic_beam"] = {"mean": statistics.mean(per), "min": min(per)}
    return out


def main():
    ap = _timing.parser(reps=10, warmup=3, n=8, distinct=0, sbs=1, seed=1)
    ap.add_argument("--widths", default="1,5,8")
    ap.add_argument("--temperature", type=float, default=1.0)
    a = ap.parse_args()
    import recnet_amd as R
    widths = [int(w) for w in a.widths.split(",")]
    dec = _timing.decoder(a, "sbs_time.py")
    eng = _timing.bound_engine(a, dec)
    enc = torch.randn(a.B, a.F, a.D, device="cuda")
    nb = 8
    logits = torch.randn(nb, a.B, a.V, device="cuda") * 2.0
    cum = -torch.rand(nb, a.B, device="cuda") * 6.0
    gum = -torch.sort(torch.rand(nb, a.B, device="cuda") * 8.0, dim=0)[0]
    fin = torch.zeros(nb, a.B, dtype=torch.int32, device="cuda")
    calls = {"sample_search": lambda: eng.sample_search(enc, a.temperature, 0, a.seed)}
    for w in widths:
        calls["beam_search_nbest_w%d" % w] = lambda w=w: eng.beam_search_nbest(enc, w, 0.0)
        calls["beam_select_rows_nb8_w%d" % w] = lambda w=w: eng.beam_select_rows(logits, cum, fin, w)
        if a.sbs:
            calls["stochastic_beam_search_w%d" % w] = lambda w=w: eng.stochastic_beam_search(enc, w, a.temperature, a.seed)
            calls["sbs_select_rows_nb8_w%d" % w] = lambda w=w: eng.sbs_select_rows(logits, cum, gum, fin, w, a.temperature, a.seed, 3)
    ms = _timing.time_calls(a, calls, lambda k: 20 if "_select_rows" in k else 1)
    assert eng.chain_status() == 0
    # the rerankers through the public calls, read-backs included
    cfg = _Cfg()
    cfg.batch_size = a.B
    inp = torch.full((1, a.B), 1, dtype=torch.long, device="cuda")
    hid = (torch.zeros(1, a.B, a.H, device="cuda"), torch.zeros(1, a.B, a.H, device="cuda"))
    wall = {"best_of_n_n%d" % a.n: lambda: R.best_of_n(cfg, dec, inp, hid, enc, a.n, a.temperature, 0, a.seed)}
    if a.sbs:
        wall["best_of_n_distinct_n%d" % a.n] = lambda: R.best_of_n(cfg, dec, inp, hid, enc, a.n, a.temperature, 0, a.seed, distinct=True)
    samples = {k: [] for k in wall}
    for k, fn in wall.items():
        fn()
    for _ in range(a.rounds):
        for k, fn in wall.items():
            samples[k] += _wall_ms(fn, 0, 1)
    ms.update({k + "_wall_ms": _timing.summary(v) for k, v in samples.items()})
    out = {"shape": _timing.shape(a), "T": eng.hyper["caption_max_len"] + 1, "precision": a.precision, "temperature": a.temperature,
           "reps": a.reps, "rounds": a.rounds, "n": a.n}
    if a.distinct:
        out["distinct_per_video_eval_msvd_n%d" % a.n] = _distinct_counts(a.n, a.temperature, a.seed, a.sbs)
    print(json.dumps(dict(out, **ms)))


if __name__ == "__main__":
    main()
