"""Times the per-caption reconstruction error at the shapes of BASELINE.json configs[1] (global reconstructor)
and configs[2] (local reconstructor, attention 128): B = 100, 28 x 1536 features, T = 31, bf16.  Per kind, on one handle with decoder
and reconstructor bound: the call with `tokens` (teacher-forced decoder forward + reconstructor forward + row kernel), the call with
`hiddens` (reconstructor forward + row kernel), and the row kernel alone (hipEvents around its launches through the profile site
RECNET_SITE_RECON_ERR = 11, minus the cost of the two event records, measured with recnet_profile_null_launch) next to the bytes it has to move.
HIP events around `reps` back-to-back calls after `warmup` calls of each; the two calls are alternated over `rounds` rounds; medians
and spreads are printed as one JSON line per kind.

    python tools/recon_time.py [--B 100 --F 28 --D 1536 --V 4188 --T 31 --reps 20 --warmup 5 --rounds 5 --kinds global,local]
"""
import ctypes as C
import json

import torch

import _timing


def kernel_bytes(kind, B, F, D, want_recon):
    """What the row kernel has to read and write once: the reconstruction, the features, the errors (+ the public reconstruction)."""
    out = B * D if kind == "global" else B * F * D
    return 4 * (out + B * F * D + B + (out if want_recon else 0))


def main():
    ap = _timing.parser(reps=20, warmup=5, RA=128, T=31)
    ap.add_argument("--kinds", default="global,local")
    a = ap.parse_args()
    import recnet_amd as R
    from recnet_amd import _lib
    for kind in a.kinds.split(","):
        dec = _timing.decoder(a, "recon_time.py")
        rec = (R.GlobalReconstructor("LSTM", 1, a.H, a.D, 0.5, 0.5, 30, precision=a.precision) if kind == "global"
               else R.LocalReconstructor("LSTM", 1, a.H, a.D, 0.5, 0.5, a.RA, precision=a.precision)).cuda().eval()
        eng = _timing.bound_engine(a, dec, rec, R=a.D, RA=a.RA if kind == "local" else 0, rec_cell="LSTM")
        enc = torch.randn(a.B, a.F, a.D, device="cuda")
        toks = torch.randint(3, a.V, (a.T, a.B), device="cuda")
        hid = torch.tanh(torch.randn(a.T, 1, a.B, a.H, device="cuda"))
        calls = {"tokens": lambda: eng.reconstruction_error(enc, tokens=toks),
                 "hiddens": lambda: eng.reconstruction_error(enc, hiddens=hid),
                 "hiddens_with_recon": lambda: eng.reconstruction_error(enc, hiddens=hid, want_recon=True)}
        n_dec = eng.profile_site(9, calls["tokens"], 1)[0]
        n_rec = eng.profile_site(7, calls["hiddens"], 1)[0]
        ms = _timing.time_calls(a, calls)
        # the row kernel alone: its bracket minus E, what the two event records add to every bracket — from empty brackets of one and
        # of two empty kernels, bracket(count) = E + count * f (include/recnet_hip.h: recnet_profile_null_launch)
        def empty_bracket(count):
            _lib.check(eng.lib.recnet_profile_begin(eng.handle, 11), "recnet_profile_begin")
            for _ in range(a.reps):
                eng.profile_null_launch(count)
            nn, tot = C.c_int32(0), C.c_double(0.0)
            _lib.check(eng.lib.recnet_profile_end(eng.handle, C.byref(nn), C.byref(tot)), "recnet_profile_end")
            return tot.value / max(nn.value, 1)
        b1, b2 = empty_bracket(1), empty_bracket(2)
        E = max(2 * b1 - b2, 0.0)
        kern = {"event_pair_us": E * 1e3, "empty_kernel_us": (b2 - b1) * 1e3}
        for k in ("hiddens", "hiddens_with_recon"):
            n, per = eng.profile_site(11, calls[k], a.reps)
            nbytes = kernel_bytes(kind, a.B, a.F, a.D, k.endswith("recon"))
            us = (per - E) * 1e3
            kern[k] = {"brackets": n, "bracket_us": per * 1e3, "kernel_us": us, "bytes": nbytes, "GB_per_s": nbytes / max(us, 1e-3) / 1e3}
        assert eng.chain_status() == 0
        out = {"kind": kind, "shape": {k: getattr(a, k) for k in ("B", "F", "D", "E", "H", "A", "RA", "V", "T")}, "precision": a.precision,
               "decoder_chain_launches_per_call": n_dec, "reconstructor_chain_launches_per_call": n_rec, "reps": a.reps, "rounds": a.rounds}
        print(json.dumps(dict(out, **ms, error_kernel=kern)))


if __name__ == "__main__":
    main()
