"""TEST INFRASTRUCTURE ONLY — numpy restatement of caption scoring (csrc/kernels_search.hpp: logprob_rows_kernel,
caption_logprob_kernel) on top of the CPU oracle's decoder step.

For a row of logits x [V], a token k and a temperature:
  s_v = x_v / temperature                       float32, like the kernel
  lp  = s_k - logsumexp_v s_v                   float64 log-softmax; k outside [0, V): -inf
For captions tokens [T][B] (time-major): step 0 is fed <SOS> and the zero state, step t > 0 is fed tokens[t - 1] (the
reference's teacher-forced loop, train.py:25,45, in eval mode);
  e_b = first t with tokens[t][b] == <EOS>, else T - 1 ;  length[b] = e_b + 1 ;  caption_logprob[b] = sum_{t <= e_b} lp[t][b]
(rows behind e_b never enter the sum: the rule of search.sequence_logprob)."""
import numpy as np
import torch

from oracle import recnet_oracle as O
from tests.gpu_util import TOL

EOS = 2


def row_bar(prec, amax, temperature):
    """Error bar of one log-probability: a logit minus a log-sum-exp of logits, each within the per-step logits bar of
    tests/test_gpu_parity.py (TOL[prec]["hid"] * 4 * max(1, max |logit|)), divided by the temperature.  The lp_bar of
    tests/search_kit.py."""
    return 2.0 * TOL[prec]["hid"] * 4 * max(1.0, float(amax)) / temperature


def logprob_rows(x, tokens, temperature):
    """x float32 [rows, V], tokens int64 [rows].  Returns float64 [rows]."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    tokens = np.asarray(tokens, dtype=np.int64)
    rows, V = x.shape
    s = (x / np.float32(temperature)).astype(np.float64)
    mx = s.max(axis=1)
    lse = mx + np.log(np.exp(s - mx[:, None]).sum(axis=1))
    ok = (tokens >= 0) & (tokens < V)
    lp = np.full(rows, -np.inf)
    r = np.nonzero(ok)[0]
    lp[r] = s[r, tokens[r]] - lse[r]
    return lp


def score_captions(P, enc, captions, temperature, cell="LSTM"):
    """captions int64 [T][B].  Returns (logprobs float64 [T][B], logit_abs_max [T]: max |logit| of the step, for the bars)."""
    captions = np.asarray(captions, dtype=np.int64)
    T, B = captions.shape
    H = P["rnn.weight_hh_l0"].shape[1]
    tok = torch.full((1, B), O.SOS, dtype=torch.long)
    hid = O.zero_hidden(B, H, cell)
    lps, amax = [], []
    with torch.no_grad():
        for t in range(T):
            logits, hid = O.decoder_step(P, tok, hid, enc, cell=cell, t=t)          # drop=None: eval mode
            lg = logits.numpy()
            lps.append(logprob_rows(lg, captions[t], temperature))
            amax.append(float(np.abs(lg).max()))
            tok = torch.from_numpy(captions[t]).view(1, -1)
    return np.stack(lps), np.array(amax)


def golden_logprobs(step_logits, tokens):
    """float64 log_softmax(step_logits)[tokens]: step_logits [T][B][V] as the reference produced them, tokens [T][B]."""
    x = np.asarray(step_logits).astype(np.float64)
    tokens = np.asarray(tokens, dtype=np.int64)
    mx = x.max(axis=2, keepdims=True)
    ls = x - mx - np.log(np.exp(x - mx).sum(axis=2, keepdims=True))
    return np.take_along_axis(ls, tokens[:, :, None], axis=2)[:, :, 0]


def caption_sums(lp, tokens):
    """lp [T][B], tokens [T][B].  Returns (caption_logprob float64 [B], length int64 [B])."""
    lp = np.asarray(lp, dtype=np.float64)
    tokens = np.asarray(tokens, dtype=np.int64)
    T, B = tokens.shape
    sums, lens = np.zeros(B), np.zeros(B, dtype=np.int64)
    for b in range(B):
        hit = np.nonzero(tokens[:, b] == EOS)[0]
        e = int(hit[0]) if hit.size else T - 1
        lens[b] = e + 1
        sums[b] = lp[:e + 1, b].sum()
    return sums, lens


# ---------------------------------------------------------------------------------- cases shared by the CPU and GPU tests
EVAL_GOLDENS = ("dec_eval", "global_eval", "local_eval", "gru_global_eval")
ROW_VS = (1, 61, 255, 256, 257, 4188, 12500)          # 4188: the row stays in registers; 12500: it is read twice
ROW_TEMPS = (0.5, 1.0, 2.0)
ROW_KINDS = ("gauss", "gauss60", "quantised")         # gauss60: |logit| in the hundreds, exp overflows without the max subtraction


def row_logits(V, rows, kind):
    rng = np.random.RandomState(7000 + 100 * V + 10 * rows + ROW_KINDS.index(kind))
    x = rng.randn(rows, V).astype(np.float32)
    if kind == "gauss60":
        x = x * np.float32(60.0)
    elif kind == "quantised":
        x = (np.round(x * 8) / 4).astype(np.float32)
    return x


def row_cases(V):
    """(rows, kind, temperature, shift): shift rotates row_case_tokens' cycle so that the single-row cases cover every kind of token."""
    out = []
    for rows in (1, 7):
        for kind in ROW_KINDS:
            for temperature in ROW_TEMPS:
                out.append((rows, kind, temperature, len(out) % 5))
    return out


def row_case_tokens(x, shift):
    """One token per row, cycling through 0, V - 1, the arg-max, -1 and V (the last two are out of range)."""
    rows, V = x.shape
    picks = [0, V - 1, None, -1, V]
    return np.array([int(x[r].argmax()) if picks[(r + shift) % 5] is None else picks[(r + shift) % 5] for r in range(rows)],
                    dtype=np.int64)
