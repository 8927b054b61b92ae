"""TEST INFRASTRUCTURE ONLY — float64 restatement of the per-caption reconstruction error (csrc/kernels_reconstructor.hpp:
recon_err_kernel) on top of the CPU oracle's reconstructor step functions.

Both reconstructors are separable per caption (models/global_reconstructor.py:30-46, models/local_reconstructor.py:37-55).  In
eval mode, for hidden states [T,1,B,H] and features enc [B,F,D]:
  global: recon[b, :] = mean_t out_t[b, :]      (train.py:96-98)     err[b] = (1 / R) sum_r (recon[b, r] - mean_f enc[b, f, r])^2 / T   (train.py:99-102)
  local:  recon[b, f, :] = out_f[b, :]          (train.py:125-127)   err[b] = (1 / (F D)) sum_{f, d} (recon[b, f, d] - enc[b, f, d])^2   (train.py:128)
so mean_b err[b] is the reference's MSE term at the same hidden states (tests/test_recon_ref.py pins that to the goldens).

Bar of one err[b] (the issue's derivation): the project's output bar tau = TOL[prec]["hid"] on every reconstructed value moves a mean
of squares e by at most 2 tau sqrt(e) + tau^2 (Cauchy-Schwarz); the global error is that mean divided by T."""
import numpy as np
import torch

from oracle import recnet_oracle as O
from tests.gpu_util import TOL

PAD, EOS = 0, 2
MUTATIONS = ("no_div_T", "sum_not_mean", "no_rescale", "frame0")


def _f64(P):
    return {k: v.detach().double() for k, v in P.items()}


def per_caption_error(recP, kind, hiddens, enc, cell="LSTM", caption_max_len=30, mutation=None):
    """hiddens [T,1,B,H], enc [B,F,D] (tensors or arrays).  Returns (err float64 [B], recon float64: global [B,R], local [B,F,D]).
    mutation: one of MUTATIONS — a deliberately wrong definition, for the tests that show the golden pin can tell them apart."""
    assert mutation is None or mutation in MUTATIONS
    P = _f64(recP)
    hid = torch.as_tensor(np.asarray(hiddens)).double()
    enc = torch.as_tensor(np.asarray(enc)).double()
    T, B, F = hid.shape[0], enc.shape[0], enc.shape[1]
    R = P["rnn.weight_hh_l0"].shape[1]
    state = O.zero_hidden(B, R, cell, torch.float64)
    outs = []
    with torch.no_grad():
        if kind == "global":
            cml = T if mutation == "no_rescale" else caption_max_len          # mp / T * T: the plain mean over the steps
            for t in range(T):
                o, state = O.global_rec_step(P, hid[t], state, hid, cell=cell, caption_max_len=cml, t=t)      # drop=None: eval mode
                outs.append(o)
            recon = torch.stack(outs).mean(0)                                                   # train.py:96-98
            ref = enc[:, 0] if mutation == "frame0" else enc.mean(1)                            # train.py:99
            sq = (recon - ref) ** 2
            err = sq.sum(1) if mutation == "sum_not_mean" else sq.mean(1)                       # train.py:101
            if mutation != "no_div_T":
                err = err / T                                                                   # train.py:102
        else:
            for f in range(F):
                o, state = O.local_rec_step(P, state, hid, cell=cell, t=f)
                outs.append(o)
            recon = torch.stack(outs).transpose(0, 1)                                           # train.py:125-127
            sq = (recon - enc) ** 2
            err = sq.sum((1, 2)) if mutation == "sum_not_mean" else sq.mean((1, 2))             # train.py:128
    return err.numpy(), recon.numpy()


def decoder_hiddens(decP, enc, captions, cell="LSTM"):
    """The teacher-forced eval-mode loop of tests/score_ref.py: score_captions (step 0 fed <SOS> and the zero state, step t > 0
    fed captions[t - 1]), returning the hidden states [T,1,B,H] it passes through."""
    captions = np.asarray(captions, dtype=np.int64)
    T, B = captions.shape
    H = decP["rnn.weight_hh_l0"].shape[1]
    tok = torch.full((1, B), O.SOS, dtype=torch.long)
    hid = O.zero_hidden(B, H, cell)
    out = []
    with torch.no_grad():
        for t in range(T):
            _, hid = O.decoder_step(decP, tok, hid, enc, cell=cell, t=t)
            out.append(hid[0] if cell == "LSTM" else hid)
            tok = torch.from_numpy(captions[t]).view(1, -1)
    return torch.stack(out)


def err_bar(prec, kind, e, T):
    """Bar of one err[b] whose restated value is e (array or scalar)."""
    tau = TOL[prec]["hid"]
    e = np.asarray(e, dtype=np.float64)
    if kind == "local":
        return 2 * tau * np.sqrt(e) + tau * tau
    return (2 * tau * np.sqrt(T * e) + tau * tau) / T


def canonical(captions, T=None, eos=EOS, pad=PAD):
    """Every token behind a caption's first <EOS> becomes <PAD>; <PAD> rows are appended up to T.  Plain loops."""
    cap = np.array(captions, dtype=np.int64)
    T0, B = cap.shape
    out = np.full((T0 if T is None else T, B), pad, dtype=np.int64)
    for b in range(B):
        for t in range(T0):
            out[t, b] = cap[t, b]
            if cap[t, b] == eos:
                break
    return out


def pick(caption_logprobs, lengths, rec_errors, recon_weight):
    """Brute-force arg-max of logprob / length - recon_weight * rec_error per caption, ties to the lowest k."""
    lp, ln, er = (np.asarray(x, dtype=np.float64) for x in (caption_logprobs, lengths, rec_errors))
    score = lp / ln - recon_weight * er
    ks = [int(np.flatnonzero(score[:, b] == score[:, b].max())[0]) for b in range(score.shape[1])]
    return ks, [float(score[k, b]) for b, k in enumerate(ks)]


GOLDENS = ("global_eval", "local_eval", "gru_global_eval")
