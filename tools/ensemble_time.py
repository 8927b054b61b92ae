"""Times ensemble decoding at the benchmark's decoder shape, bf16: recnet_ensemble_mix_rows alone on random
rows at the (rows, M) of --shapes in both modes, with the bytes per second it achieves on its (M + 1) * rows * V * 4 bytes of
compulsory traffic; the width-8 N-best search of one model and of ensembles of --members models (LSTM decoders with different
seeds); scoring of 31-row captions by one model and by the ensembles.  HIP events around `reps` back-to-back calls after `warmup`
calls of each; the calls are alternated over `rounds` rounds so that drift hits them alike; the median and the spread over rounds
are printed as one JSON line.  Read an ensemble call against M times the single-model call of the same run, plus one mix per step
(per call, for the scorer) at the rate the kernel-alone rows show.

    python tools/ensemble_time.py [--B 100 --F 28 --D 1536 --V 4188 --width 8 --shapes 800:2,800:4,3100:2,3100:4 --members 2,4 --reps 5 --warmup 2 --rounds 5]
"""
import json

import torch

import _timing


def main():
    ap = _timing.parser(reps=5, warmup=2, width=8)
    ap.add_argument("--shapes", default="800:2,800:4,3100:2,3100:4")
    ap.add_argument("--members", default="2,4")
    ap.add_argument("--length_alpha", type=float, default=0.7)
    a = ap.parse_args()
    import recnet_amd as R
    from recnet_amd import search
    from recnet_amd.engine import Engine
    members = [int(x) for x in a.members.split(",")]
    decs = []
    for m in range(max(members)):
        dec = _timing.decoder(a, "ensemble_time.py")                      # (seeds torch with 0)
        if m:
            torch.manual_seed(m)
            for p in dec.parameters():
                if p.numel() > 1:
                    p.data.copy_(torch.randn_like(p) * p.data.std())
        decs.append(dec)

    class Cfg:
        caption_max_len, decoder_model, batch_size = 30, "LSTM", a.B
    gen = torch.Generator().manual_seed(0)
    enc = torch.randn(a.B, a.F, a.D, device="cuda")
    rows_eng = search._consensus_engine(enc.device)
    engs = [search._nbest_engine(Cfg, d, enc) for d in decs]
    calls, mix_bytes = {}, {}
    for rows, M in ([int(x) for x in s.split(":")] for s in a.shapes.split(",")):
        xs = [torch.randn(rows, a.V, generator=gen).mul_(3.0).cuda() for _ in range(M)]
        y = torch.empty_like(xs[0])
        for mode in ("arithmetic", "geometric"):
            k = "mix_rows_%d_M%d_%s" % (rows, M, mode)
            calls[k] = lambda xs=xs, mode=mode: rows_eng.ensemble_mix_rows(xs, None, mode)
            mix_bytes[k] = (M + 1) * rows * a.V * 4
    caps = torch.randint(3, a.V, (31, a.B), generator=gen).cuda()
    calls["beam_search_nbest_w%d" % a.width] = lambda: engs[0].beam_search_nbest(enc, a.width, a.length_alpha)
    calls["score_captions_T31"] = lambda: engs[0].score_captions(enc, caps)
    for M in members:
        for mode in ("arithmetic", "geometric"):
            calls["beam_search_nbest_ensemble_w%d_M%d_%s" % (a.width, M, mode)] = \
                lambda M=M, mode=mode: Engine.beam_search_nbest_ensemble(engs[:M], enc, a.width, a.length_alpha, None, mode)
        calls["score_captions_ensemble_T31_M%d" % M] = lambda M=M: Engine.score_captions_ensemble(engs[:M], enc, caps)
    ms = _timing.time_calls(a, calls, lambda k: 20 if k.startswith("mix_rows") else 1)
    out = {"shape": _timing.shape(a), "precision": a.precision, "width": a.width, "length_alpha": a.length_alpha, "reps": a.reps,
           "rounds": a.rounds,
           "search_steps": {"M1": int(engs[0].beam_search_nbest(enc, a.width, a.length_alpha)[4].item())}}
    for M in members:
        out["search_steps"]["M%d" % M] = int(Engine.beam_search_nbest_ensemble(engs[:M], enc, a.width, a.length_alpha)[5].item())
    out.update(ms)
    for k, b in mix_bytes.items():
        out[k + "_GBps"] = b / (ms[k + "_ms"]["median"] * 1e-3) / 1e9
    print(json.dumps(out))


if __name__ == "__main__":
    main()
