"""TEST INFRASTRUCTURE ONLY — float64 restatement of the stochastic beam search (Kool, van Hoof, Welling 2019; DESIGN.md section 21;
csrc/kernels_search.hpp: sbs_select_kernel, csrc/abi_search.inc: recnet_stochastic_beam_search) on the CPU oracle's decoder step, in the
style of tests/beam_ref.py.

Start: <SOS>, zero state, one hypothesis per caption with phi = 0 (its log-probability) and G = 0 (its perturbed score).  At step t a
caption has nb hypotheses (1 at t = 0, else bw) in slots i, on rows = B captions.  With s_v = logit_v / temperature (float32):
  a live hypothesis i, every v:
    phi_v  = phi_i + log_softmax(s)[v]                           float64 (the maximum subtracted before the exponentials)
    idx    = ((t * bw * rows + i * rows + r) * V + v) mod 2^32   r: the caption row; bw: the search's width, at t = 0 too
    g_v    = the float32 Gumbel of sample_ref.gumbel on idx (site SITE_SAMPLE, the seed)
    Gt_v   = phi_v + g_v
    Z_i    = max_v Gt_v
    Ghat_v = -log(exp(-G_i) - exp(-Z_i) + exp(-Gt_v)), evaluated as
             a = Gt_v - Z_i <= 0;  l = log(-expm1(a)) if a > -ln 2 else log1p(-exp(a))   (a = 0: l = -inf)
             w = G_i - Gt_v + l;   Ghat_v = G_i - max(0, w) - log1p(exp(-|w|))           (w = -inf: Ghat_v = G_i)
  a finished hypothesis i (it holds <EOS>): one candidate, v = <PAD>, phi = phi_i, Ghat = G_i, no noise; -inf at every other v
  the bw largest Ghat of the nb * V candidates become the new hypotheses, in descending order, the lowest flat index i * V + v first
  among equals; each carries (phi_v, Ghat_v).
Per parent the maximum of the children's perturbed scores is conditioned to be the parent's: its best child inherits G_i exactly, and
G never increases along a hypothesis.  Only <EOS> finishes a hypothesis; the loop ends after the first step at which every hypothesis
is finished, or after caption_max_len + 1 steps.  Rank = slot: G descending, the lowest slot among equals.

Near-ties.  The transform can stretch differences: its first-order sensitivities to G_i, Gt_v, Z_i are exp(Ghat - G_i),
exp(Ghat - Gt_v), exp(Ghat - Z_i).  Every candidate reports amp, their sum (1 for the candidate of a finished hypothesis and for a parent's best
child: there a = 0 exactly on every machine, Z_i being one of the Gt_v, and Ghat = G_i does not depend on Gt_v = Z_i at all — the sum
would charge it exp(G_i - Z_i) twice, for two errors that cancel; 1 is the smaller figure and so asks more of the device); every
decision reports the smallest non-zero gap among its top bw + 1 Ghat divided by the larger amp of the two neighbours.  A decision
whose quotient is below sample_ref.NEAR_TIE is left out of token comparisons, and the caption with it from that step on — a condition
for exclusion, not a tolerance on results.  tests/test_sbs_ref.py holds the cap: at least 3/4 of the (step, caption) decisions of
every run below are compared.  RUN_SHARES at the end of the file records the shares (python -m tests.sbs_ref prints them)."""
import numpy as np
import torch

from oracle import recnet_oracle as O
from tests import sample_ref as SR
from tests.beam_ref import log_softmax64
from tests.sample_ref import NEAR_TIE

EOS, PAD = 2, 0


def condition(G, Gt, Z):
    """Ghat of (G_i, Gt_v, Z_i), float64 arrays that broadcast; Gt <= Z."""
    G, Gt, Z = np.broadcast_arrays(np.asarray(G, dtype=np.float64), np.asarray(Gt, dtype=np.float64), np.asarray(Z, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = Gt - Z
        l = np.where(a > -np.log(2.0), np.log(-np.expm1(a)), np.log1p(-np.exp(a)))
        w = G - Gt + l
        out = G - np.maximum(0.0, w) - np.log1p(np.exp(-np.abs(w)))
    return np.where(np.isneginf(w), G, out)


def noise(seed, t, bw, rows, i, V):
    """float32 [rows, V]: the Gumbels of slot i at step t of a search of width bw on `rows` captions."""
    counters = [(t * bw * rows + i * rows + r) for r in range(rows)]
    return SR.gumbel(seed, 0, 1, V, rows=counters)


def candidates(logits, cum, gum, finished, bw, temperature, seed, t):
    """Every candidate of one step: (phi, Ghat, amp) float64 [rows, nb * V], flat index i * V + v."""
    logits = np.asarray(logits, dtype=np.float32)
    nb, rows, V = logits.shape
    cum, gum = np.asarray(cum).astype(np.float64), np.asarray(gum).astype(np.float64)
    fin = np.asarray(finished) != 0
    s = logits / np.float32(temperature)
    phi = cum[:, :, None] + log_softmax64(s)
    g = np.stack([noise(seed, t, bw, rows, i, V) for i in range(nb)]).astype(np.float64)
    Gt = phi + g
    Z = Gt.max(axis=2, keepdims=True)
    Gp = gum[:, :, None]
    Gh = condition(Gp, Gt, Z)
    with np.errstate(over="ignore", invalid="ignore"):
        amp = np.exp(Gh - Gp) + np.exp(Gh - Gt) + np.exp(Gh - Z)
    amp = np.where(Gt == Z, 1.0, amp)                                   # the parent's best child: Ghat = G_i whatever Gt = Z is
    pad_phi = np.full((nb, rows, V), -np.inf); pad_phi[:, :, PAD] = cum
    pad_G = np.full((nb, rows, V), -np.inf); pad_G[:, :, PAD] = gum
    f = fin[:, :, None]
    phi, Gh, amp = np.where(f, pad_phi, phi), np.where(f, pad_G, Gh), np.where(f, 1.0, amp)
    flat = lambda a: np.transpose(a, (1, 0, 2)).reshape(rows, nb * V)
    return flat(phi), flat(Gh), flat(amp)


def select_rows(logits, cum, gum, finished, bw, temperature=1.0, seed=0, t=0):
    """One selection step.  logits float32 [nb, rows, V]; cum, gum, finished [nb, rows].  Returns a dict: vals (phi) and gum (Ghat)
    float64 [rows, bw], idx int64 [rows, bw] = i * V + v, amp float64 [rows, bw], margin float64 [rows] (the near-tie quotient)."""
    phi, Gh, amp = candidates(logits, cum, gum, finished, bw, temperature, seed, t)
    order = np.argsort(-Gh, axis=1, kind="stable")                       # equal values keep index order
    k = min(bw + 1, Gh.shape[1])
    top = order[:, :k]
    tG, tA = np.take_along_axis(Gh, top, axis=1), np.take_along_axis(amp, top, axis=1)
    if k >= 2:
        with np.errstate(invalid="ignore"):
            gaps = tG[:, :-1] - tG[:, 1:]
            q = gaps / np.maximum(tA[:, :-1], tA[:, 1:])
        q = np.where(np.isnan(gaps) | (gaps == 0) | np.isnan(q), np.inf, q)  # exact ties, (-inf) - (-inf): the index rule decides
        margin = q.min(axis=1)
    else:
        margin = np.full(Gh.shape[0], np.inf)
    sel = order[:, :bw]
    return dict(vals=np.take_along_axis(phi, sel, axis=1), gum=np.take_along_axis(Gh, sel, axis=1), idx=sel.astype(np.int64),
                amp=np.take_along_axis(amp, sel, axis=1), margin=margin)


def stochastic_beam_search(P, enc, bw, temperature=1.0, seed=0, caption_max_len=30, cell="LSTM"):
    """Returns a dict: tokens int64 [bw][n_steps][B] rank-major (canonical), cum / gum float64 [bw][B], len int64 [bw][B], n_steps,
    margins float64 [n_steps][B], amp float64 [bw][B]: the largest amp along each returned hypothesis (for the bar of gum), amax
    [n_steps] (max |logit| of the step), and trace: per step a dict of what the step left, in slot order: tok, fin, cum, gum [bw][B],
    hist [bw][B][t + 1], src [bw][B] (the parent slot), and the parents' fin / cum / gum [nb][B] before it."""
    B = enc.shape[0]
    H = P["rnn.weight_hh_l0"].shape[1]
    Tm = caption_max_len + 1
    toks = [torch.full((1, B), O.SOS, dtype=torch.long)]
    hids = [O.zero_hidden(B, H, cell)]
    cum, gum = np.zeros((1, B)), np.zeros((1, B))
    fin = np.zeros((1, B), dtype=np.int64)
    hist = np.zeros((1, B, Tm), dtype=np.int64)
    amp_max = np.ones((1, B))
    margins, amax, trace = [], [], []
    n_steps = Tm
    ar = np.arange(B)
    with torch.no_grad():
        for t in range(Tm):
            nb = len(toks)
            steps = [O.decoder_step(P, toks[i], hids[i], enc, cell=cell, t=t) for i in range(nb)]
            lg = np.stack([s[0].numpy() for s in steps])                 # [nb, B, V]
            V = lg.shape[2]
            r = select_rows(lg, cum, gum, fin, bw, temperature, seed, t)
            src, tok = r["idx"] // V, r["idx"] % V                       # [B, bw]
            new_hids = []
            for k in range(bw):
                if cell == "GRU":
                    new_hids.append(torch.stack([steps[src[b, k]][1][:, b] for b in range(B)], dim=1))
                else:
                    new_hids.append(tuple(torch.stack([steps[src[b, k]][1][j][:, b] for b in range(B)], dim=1) for j in range(2)))
            new_hist = np.stack([hist[src[:, k], ar] for k in range(bw)])
            new_hist[:, :, t] = tok.T
            old_fin = np.stack([fin[src[:, k], ar] for k in range(bw)])
            before = dict(pfin=fin.copy(), pcum=cum.copy(), pgum=gum.copy())
            amp_max = np.maximum(np.stack([amp_max[src[:, k], ar] for k in range(bw)]), r["amp"].T)
            fin = np.where(old_fin > 0, old_fin, np.where(tok.T == EOS, t + 1, 0))
            cum, gum, hist, hids = r["vals"].T.copy(), r["gum"].T.copy(), new_hist, new_hids
            toks = [torch.from_numpy(tok[:, k].copy()).view(1, -1) for k in range(bw)]
            margins.append(r["margin"]); amax.append(float(np.abs(lg).max()))
            trace.append(dict(tok=tok.T.copy(), fin=fin.copy(), cum=cum.copy(), gum=gum.copy(), hist=hist[:, :, :t + 1].copy(),
                              src=src.T.copy(), **before))
            if (fin > 0).all():
                n_steps = t + 1
                break
    ln = np.where(fin > 0, fin, n_steps)
    tokens = np.transpose(hist, (0, 2, 1))[:, :n_steps]
    return dict(tokens=tokens, cum=cum, gum=gum, len=ln, n_steps=n_steps, margins=np.stack(margins), amp=amp_max, amax=np.array(amax),
                trace=trace)


def comparable_steps(margins):
    """bool [n][B]: True for the decisions of a caption before its first near-tie one."""
    near = margins < NEAR_TIE
    return ~(np.cumsum(near, axis=0) > 0)


def comparable_captions(res):
    """bool [B]: no decision of the caption is a near-tie: its returned hypotheses compare in full."""
    return comparable_steps(res["margins"]).all(axis=0)


def compared_share(res):
    return float(comparable_steps(res["margins"]).mean())


def weights(cum, gum, normalize=True):
    """The importance weights of search.sbs_weights, restated by plain quadrature: cum, gum float64 [bw][B] in rank order.  Rank
    k < bw - 1: w = int_0^inf p / (1 - exp(-p (c + e))) exp(-e) de with p = exp(cum), c = exp(-gum[bw - 1]) - 1 (the mean of p / q over
    the Exp(1) variable the search pinned to 1 by starting from G = 0); rank bw - 1: 0; width 1: 1.  The integrand is 1 / (c + e)
    plus a smooth bounded part: the first goes by t = (c + e) = c exp(s), Simpson on int exp(c - c exp(s)) ds over the range where it
    is above 1e-300, the second by Simpson on e in [0, 60]."""
    cum, gum = np.asarray(cum, dtype=np.float64), np.asarray(gum, dtype=np.float64)
    bw = cum.shape[0]
    if bw == 1:
        return np.ones_like(cum)
    p = np.exp(cum)
    with np.errstate(over="ignore"):
        c = np.clip(np.expm1(-gum[bw - 1]), 1e-300, 1e300)               # [B]
    n = 20001
    simpson = np.ones(n); simpson[1:-1:2] = 4.0; simpson[2:-1:2] = 2.0
    S = np.log((c + 800.0) / c)
    s = np.linspace(0.0, 1.0, n)[:, None] * S[None, :]
    first = (np.exp(c - c * np.exp(s)) * simpson[:, None]).sum(axis=0) * (S / (n - 1)) / 3.0
    e = np.linspace(0.0, 60.0, n)                                        # (exp(-60) is below the last place of the sum)
    x = p[:, :, None] * (c[None, :, None] + e)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        smooth = np.where(x < 1e-3, 0.5 + x / 12.0, 1.0 / -np.expm1(-x) - 1.0 / x)
    wu = simpson * np.exp(-e) * (60.0 / (n - 1)) / 3.0
    w = first[None, :] + p * (smooth * wu).sum(axis=2)
    w[bw - 1] = 0.0
    return w / w.sum(axis=0, keepdims=True) if normalize else w


# ---------------------------------------------------------------------------------- cases shared by the CPU and GPU tests
CAP = 0.75
# (case, beam width, caption_max_len, temperature, seed): the seven search goldens and the shape case rows160.  Seeds from 1..8, the
# first for which the restatement compares at least CAP of the run's decisions.
SEARCH_RUNS = [("search_small", 3, 7, 1.0, 1), ("search_stop", 3, 7, 1.0, 1),
               ("search_small_b", 3, 7, 1.0, 1), ("search_small_b", 8, 7, 0.5, 2), ("search_eos", 3, 7, 1.0, 1), ("search_eos", 8, 7, 0.5, 1),
               ("search_gru", 3, 7, 1.0, 1), ("search_gru", 8, 7, 0.5, 1), ("search_gru_stop", 3, 7, 1.0, 1), ("search_gru_stop", 8, 7, 0.5, 1),
               ("search_gru_b", 5, 30, 1.0, 1),
               ("rows160", 3, 7, 1.0, 1), ("rows160", 5, 7, 0.5, 1), ("rows160", 8, 7, 1.0, 1)]
# the runs the device test adds at the benchmark's decoder (no CPU test walks them: the restatement of one takes seconds)
DEVICE_RUNS = [("eval_msvd", 8, 7, 1.0, 1)]
# width 1 against sample_ref.sample_search: (case, temperature, seed)
WIDTH1_RUNS = [("search_small", 1.0, 4), ("search_small_b", 1.0, 3), ("search_eos", 1.0, 4), ("search_stop", 1.0, 2), ("search_gru", 1.0, 7),
               ("search_gru_b", 1.0, 2), ("search_gru_stop", 1.0, 2), ("search_small", 0.5, 5), ("rows160", 1.0, 2)]

# Kernel-alone cases: beam_ref.row_case's inputs plus a column of perturbed scores descending in the slot
ROW_T = (3, 200000)           # the second one wraps the counter past 2^32 at the large vocabularies
ROW_TEMPS = (1.0, 0.5)


def row_gum(nb, rows, V):
    """float32 [nb, rows]: perturbed scores of the hypotheses, descending in the slot i as a search leaves them."""
    rng = np.random.RandomState(7000 + 10 * V + nb)
    return (-np.sort(rng.rand(nb, rows) * 8.0, axis=0) - 0.5).astype(np.float32)


_RUNS = {}


def run(name, bw, cml, temperature, seed):
    """stochastic_beam_search of a run, computed once per process and left unchanged."""
    key = (name, bw, cml, temperature, seed)
    if key not in _RUNS:
        from tests.golden_util import load_search_case
        g, P, enc = load_search_case(name)
        torch.set_num_threads(min(16, torch.get_num_threads()))
        _RUNS[key] = stochastic_beam_search(P, enc, bw, temperature, seed, cml, g["_cell"])
    return _RUNS[key]


# share of compared (step, caption) decisions per run, measured by this restatement
RUN_SHARES = {("search_small", 3, 7, 1.0, 1): 0.833, ("search_stop", 3, 7, 1.0, 1): 1.000, ("search_small_b", 3, 7, 1.0, 1): 0.781,
              ("search_small_b", 8, 7, 0.5, 2): 1.000, ("search_eos", 3, 7, 1.0, 1): 0.833, ("search_eos", 8, 7, 0.5, 1): 0.833,
              ("search_gru", 3, 7, 1.0, 1): 0.854, ("search_gru", 8, 7, 0.5, 1): 0.833, ("search_gru_stop", 3, 7, 1.0, 1): 1.000,
              ("search_gru_stop", 8, 7, 0.5, 1): 1.000, ("search_gru_b", 5, 30, 1.0, 1): 1.000, ("rows160", 3, 7, 1.0, 1): 0.956,
              ("rows160", 5, 7, 0.5, 1): 0.969, ("rows160", 8, 7, 1.0, 1): 0.794, ("eval_msvd", 8, 7, 1.0, 1): 0.949}


if __name__ == "__main__":
    shares = []
    for name, bw, cml, temp, seed in SEARCH_RUNS + DEVICE_RUNS:
        r = run(name, bw, cml, temp, seed)
        print(name, bw, cml, temp, "seed", seed, "steps", r["n_steps"], "share %.3f" % compared_share(r), "captions in full",
              int(comparable_captions(r).sum()), "of", r["cum"].shape[1], "max amp %.2f" % r["amp"].max())
        shares.append('("%s", %d, %d, %s, %d): %.3f' % (name, bw, cml, temp, seed, compared_share(r)))
    print("RUN_SHARES = {" + ", ".join(shares) + "}")
