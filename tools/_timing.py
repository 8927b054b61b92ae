"""What the search timing tools (beam_time, sample_time, score_time, recon_time, consensus_time) share: the shape arguments, the
decoder at that shape with an engine bound to it, and the measurement — HIP events around `reps` back-to-back calls after `warmup`
calls of each, the calls alternated over `rounds` rounds so that drift hits them alike, the median and the spread over rounds."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPE = ("B", "F", "D", "E", "H", "A", "V")


def parser(reps, warmup, **more):
    """--B --F --D --E --H --A --V at the benchmark's decoder shape, --reps --warmup --rounds, the tool's own integers, --precision."""
    ap = argparse.ArgumentParser()
    for k, v in dict(B=100, F=28, D=1536, E=468, H=512, A=128, V=4188, reps=reps, warmup=warmup, rounds=5, **more).items():
        ap.add_argument("--" + k, type=int, default=v)
    ap.add_argument("--precision", default="bf16")
    return ap


def decoder(a, tool):
    """The seeded LSTM decoder of the arguments, in eval mode on the device."""
    import recnet_amd as R
    if not torch.cuda.is_available():
        raise SystemExit("%s needs a GPU: a CPU run says nothing about these times" % tool)
    torch.manual_seed(0)
    return R.Decoder("LSTM", 1, a.D, a.E, 1, a.H, a.A, a.V, 0.5, 0.5, 0.5, precision=a.precision).cuda().eval()


def bound_engine(a, dec, rec=None, **rec_dims):
    """An engine of its own with the decoder (and the reconstructor, rec_dims being its dims) bound and packed."""
    from recnet_amd.engine import Engine
    dims = dec.dims(a.B, a.F)
    dims.update(rec_dims)
    eng = Engine(dims, getattr(rec, "kind", None), a.precision, dec.hyper(), device="cuda")
    eng.bind_decoder({k: v.data for k, v in dec.named_tensors().items()})
    if rec is not None:
        eng.bind_reconstructor({k: v.data for k, v in rec.named_tensors().items()})
    eng.pack_weights()
    return eng


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def time_calls(a, calls, times=lambda name: 1):
    """{name + "_ms": summary over the rounds of the device time of one call}; a call runs a.reps * times(name) times per round
    (kernel-alone calls are too short for a.reps of them to be read off two events)."""
    for fn in calls.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():
            reps = a.reps * times(k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)
    return {k + "_ms": summary(v) for k, v in ms.items()}


def shape(a, *more):
    return {k: getattr(a, k) for k in SHAPE + more}
