"""TEST INFRASTRUCTURE ONLY — the operand-rounded restatement of the train step.

oracle/recnet_oracle.py states the step as the reference writes it and rounds nothing.  The product's bf16 path
keeps its state in fp32 and rounds every GEMM operand to bf16; the persistent chain kernels exist in that path only.  This module
states what the BF16 PATH computes in real arithmetic: the factoring of DESIGN.md §2 (it decides WHAT is rounded) with a rounding at
every place where the product stores a bf16 (or fp16) value that something reads later.  It runs in float64 (the reference for the
device) or in float32 with every product's contraction summed in chunks of 32 in reversed order (the floor of
tests/test_rounded_ref.py: what a different summation order alone moves).  With the rounding switched off it computes the oracle's
CE, MSE, hidden states and gradients (same test).  No regulariser on either side (cells_kit.oracle_grads_no_reg).  Teacher forcing only.

Nothing in the product package imports this file.

Scope: the persistent chains and the batched products around them.  The per-step bf16 kernels round at other points (the BPTT's
per-step kernel sums four bf16 frame-chunk partials of dWh, the local per-step backward rounds dWhr per chunk of decoder steps:
DESIGN.md §18, §20) and are not restated; where a shape leaves one chain to them the difference stays inside the bars of
tests/gpu_util.TOL["bf16_rounded"] (the global family's H = 24 shapes: 2e-3 in the decoder's attention gradients).
`mistake`: the named local mistakes of tests/rounded_kit.MISTAKES, for the power test of tests/test_rounded_ref.py only.

The primitives
    mm(a, w)      a . w^T with both operands rounded (w [n, k] as the state_dict holds it).  Backward: the incoming gradient is
                  rounded ONCE and both operand gradients are formed from it and the saved rounded operands — the product keeps one
                  bf16 copy of every d-pre-activation and every deferred product reads that copy.
    ground(x)     identity whose backward rounds: marks the tensor whose GRADIENT the product stores in bf16 when more than products
                  read it (the bias gradients are column sums of the bf16 rows; da of the decoder's attention is formed from them).
    store16(x)    round with a straight-through gradient: a RESULT stored in bf16 and consumed later (P).
    The rounded weights are cached per call (mode()): W_hh at R = 2560 has 26 M elements.

The rounding contract of the bf16 path — site, buffer (csrc/api.hip), producer.  State (h, c, gate activations, losses, every
gradient tensor, every accumulator over t / s / frames) is fp32 unless listed.

  decoder forward
    enc                    enc_lp         prologue_pack_kernel                     operand of Uv and P
    drop(scale * emb_t)    emb_lp         prologue_pack_kernel / embed_fwd         operand of Xe = emb . W_ih[:, :E]^T + b_ih + b_hh (ONE product, fp32 out)
    Uv = enc . U^T         Uv (fp32)      grouped GEMM                             not rounded
    P = enc . W_ih[:,E:]^T P (bf16)       grouped GEMM                             a stored RESULT; the forward never forms a context vector:
                                                                                   gates += (1/F) sum_f a_t[f] P[b, f, :]
    a_t[f]                 registers      dec_chain_kernel                         the A operand of the context MFMA is bf16(a) + bf16(a - bf16(a)): 16 bits of a
    h_{t-1}                Hs_lp, dc_pan  dec_chain_kernel (hl)                    operand of h . [W_hh ; attn_W]^T, of logits, d W_hh, d attn_W, d W_o;
                                                                                   of the global reconstructor's input and the local one's Ud
    every weight           weight images  adam_chunk_kernel / pack_chunk_kernel    csrc/weight_images.hpp: Wcomb = [W_hh ; attn_W], We_w, Wc_w, U_w, Wo_w, the
                                                                                   reconstructor's Wih_f / Whh_w / Wor_w / Ur_w / Wr_w / Wihh_w and their transposes
    attention energies, tanh, cell pointwise: fp32 from fp32 (Wh + attn_b + Uv; w . tanh)
  decoder loss and backward
    d logits               dlog_lp        ce_kernel                                (softmax - onehot) * mask * 1/(n_t N), rounded; d hiddens, d W_o read it and
                                                                                   d b_o is ITS column sum
    [dgates_t | dWh_t]     dGx, dc_pan2   dec_chain_bwd_kernel (srow)              dh_{t-1}, da_t[f] = (1/F) P . dgates (from the bf16 row), d W_ih (both windows),
                                                                                   d W_hh, d attn_W, d emb read it; d b_ih, d b_hh, d attn_b are ITS column sums
    ctx_t = (1/F) sum a enc ctx_lp        ctx_all_kernel                           rebuilt in the backward from fp32 a and fp32 enc, rounded once:
                                                                                   d W_ih[:, E:] = dgates^T . ctx  (the forward never rounded a context vector)
    dUv = sum_t dz_t       dUv_lp         dec_chain_bwd_kernel                     accumulated over t in fp32, rounded once; d attn_U = dUv^T . enc
    d attn_w               dwacc (fp32)   dec_chain_bwd_kernel                     not rounded
  global reconstructor
    [h_t ; drop_t(mp)]     Xcat_g         dec_chain_kernel / xcat_global_kernel    ONE concatenated operand; mp = (cml / T^2) sum_t h_t from the fp32 h
    hr_{t-1}               Hr_lp, Hr_pan  rec_chain_kernel                         operand of hr . W_hh^T and of d W_hh
    mean_t hr_t            hrmean_lp      rec_chain_kernel (epilogue)              fp32 mean, rounded once; the output layer runs ONCE on it
    lambda * d out         dout_lp        rec_chain_kernel epilogue / mse_vec      d mean hr, d W_o read it; d b_o is its column sum
    dgates_t               dGr, dG_pan    rec_chain_bwd_kernel                     dhr_{t-1}, d W_hh, d W_ih, d [h_t ; mp] read it; the bias gradients are its
                                                                                   column sums.  d hiddens: fp32 product folded through masks and pooling in fp32
  local reconstructor
    Ud = h . U_r^T         Ud (fp32)      GEMM over Hs_lp                          not rounded
    Whr_s                  lc_pw (FP16)   loc_chain_kernel                         hr_{s-1} . W_r^T as R / 16 rank-16 partial products, each stored in fp16, summed in fp32
    x_s                    Xcat_r, panx   loc_chain_kernel (xl)                    drop((1/T) sum_t beta[t] h_t) from the fp32 h, rounded once
    hr_{s-1}               Hr_lp, panh    loc_chain_kernel                         operand of the gates, of out, d W_hh, d attn_W, d W_o
    lambda * d out         dout_lp        output layer's epilogue                  as the global one's
    dgates_s               dGr, lc_pang   loc_chain_bwd_kernel / lcbig_bwd_kernel  as the global one's; [dx | dhr] = dgates . [W_ih | W_hh] in fp32
    dWhr_s = sum_t dz      dWhrs, panw    loc_chain_bwd_kernel (swl)               dhr_{s-1} and d attn_W read it
    dUd = sum_s dz         dUd_lp         loc_chain_bwd_kernel                     accumulated over s in fp32, rounded once: d attn_U and d hiddens read it;
                                                                                   d attn_b is the column sum of the FP32 dUd
"""
import contextlib

import torch

from . import dropmask
from . import recnet_oracle as O

SOS = O.SOS


class _State:
    round = True      # round where the product rounds
    chunk = False     # sum every product's contraction in chunks of 32, last chunk first (the float32 floor)
    cache = None


_S = _State()


@contextlib.contextmanager
def mode(round=True, chunk=False):
    old = (_S.round, _S.chunk, _S.cache)
    _S.round, _S.chunk, _S.cache = round, chunk, {}
    try:
        yield
    finally:
        _S.round, _S.chunk, _S.cache = old


def bf16(x):
    """Round to nearest even to bf16, in the tensor's own dtype."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype) if _S.round else x


def fp16(x):
    return x.to(torch.float32).to(torch.float16).to(x.dtype) if _S.round else x


def _weight(w):
    if _S.cache is None:
        return bf16(w.detach())
    key = (id(w), w.data_ptr(), tuple(w.shape), tuple(w.stride()))
    hit = _S.cache.get(key)
    if hit is None:
        hit = _S.cache[key] = (w, bf16(w.detach()))      # (keeps w alive: its id stays its own)
    return hit[1]


def _dot(a, b):
    """a [m, k] . b [k, n]."""
    if not _S.chunk or a.shape[1] <= 32:
        return a @ b
    out = None
    for k0 in reversed(range(0, a.shape[1], 32)):
        part = a[:, k0:k0 + 32] @ b[k0:k0 + 32]
        out = part if out is None else out + part
    return out


class _MM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, w):
        ar, wr = bf16(a).reshape(-1, a.shape[-1]), _weight(w)
        ctx.save_for_backward(ar, wr)
        ctx.lead = a.shape[:-1]
        return _dot(ar, wr.t()).reshape(*a.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, g):
        ar, wr = ctx.saved_tensors
        gr = bf16(g).reshape(-1, g.shape[-1])
        return _dot(gr, wr).reshape(*ctx.lead, wr.shape[1]), _dot(gr.t(), ar)


def mm(a, w):
    return _MM.apply(a, w)


class _GRound(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return bf16(g)


def ground(x):
    return _GRound.apply(x)


class _Store16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return bf16(x)

    @staticmethod
    def backward(ctx, g):
        return g


def store16(x):
    return _Store16.apply(x)


class _Context(torch.autograd.Function):
    """The context's share of the gates, (1/F) sum_f a[f] P[b, f, :], P = store16(enc . Wc^T): forward from the stored P with a
    split into two bf16 parts; backward da = (1/F) P . g and d Wc = g^T . bf16((1/F) sum_f a[f] enc[b, f, :])."""

    @staticmethod
    def forward(ctx, a, enc, Wc, Pm):
        ctx.save_for_backward(a, enc, Pm)
        hi = bf16(a)
        a2 = hi + bf16(a - hi)
        return torch.einsum("bf,bfn->bn", a2, Pm) / a.shape[1]

    @staticmethod
    def backward(ctx, g):
        a, enc, Pm = ctx.saved_tensors
        gr = bf16(g)
        F = a.shape[1]
        da = torch.einsum("bn,bfn->bf", gr, Pm) / F
        c = bf16(torch.einsum("bf,bfd->bd", a, enc) / F)
        return da, None, _dot(gr.t(), c), None


class _WhrGroups(torch.autograd.Function):
    """hr . W_r^T of the local forward chain: rank-16 partial products by unit group, each stored in fp16, summed in fp32."""

    @staticmethod
    def forward(ctx, hr, Wr):
        hb, wb = bf16(hr), _weight(Wr)
        ctx.save_for_backward(hb, wb)
        B, R = hb.shape
        if not _S.round or R % 16:
            return _dot(hb, wb.t())
        part = torch.einsum("bgu,agu->bga", hb.reshape(B, R // 16, 16), wb.reshape(-1, R // 16, 16))
        return fp16(part).sum(1)

    @staticmethod
    def backward(ctx, g):
        hb, wb = ctx.saved_tensors
        gr = bf16(g)
        return _dot(gr, wb), _dot(gr.t(), hb)


# ----------------------------------------------------------------------------- cells: one pointwise function each
def lstm_point(pre, c):
    i, f, g, o = pre.chunk(4, dim=1)
    c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c2), c2


def gru_point(gi, gh, h):
    ir, iz, in_ = gi.chunk(3, dim=1)
    hr, hz, hn = gh.chunk(3, dim=1)
    r = torch.sigmoid(ir + hr)
    z = torch.sigmoid(iz + hz)
    n = torch.tanh(in_ + r * hn)
    return (1.0 - z) * n + z * h


def _cell(cell, xin, hh, P, state, biased):
    """xin: the input part of the gates (biased: with b_ih — and b_hh for an LSTM — already inside); hh = h_{t-1} . W_hh^T.  The
    product stores d(gates) once per gate block in bf16; a GRU's four blocks (r, z, input n, recurrent n) are the two ground()s."""
    if cell == "LSTM":
        h, c = state
        pre = xin + hh if biased else xin + hh + P["rnn.bias_ih_l0"] + P["rnn.bias_hh_l0"]
        h2, c2 = lstm_point(ground(pre), c)
        return h2, (h2, c2)
    h = state[0]
    gi = xin if biased else xin + P["rnn.bias_ih_l0"]
    h2 = gru_point(ground(gi), ground(hh + P["rnn.bias_hh_l0"]), h)
    return h2, (h2, None)


def _zero_state(B, H, like):
    z = torch.zeros(B, H, dtype=like.dtype)
    return (z, z.clone())


def _nomist(kind, **kw):
    return False


# ----------------------------------------------------------------------------- decoder
def forward_decoder(P, enc, targets, target_masks, *, cell="LSTM", caption_max_len=30, emb_scale=1.0, p_emb=0.5, p_out=0.5, drop=None,
                    mistake=None):
    """CE (train.py:68 without the regulariser) and hiddens [T, B, H].  mistake(kind, **where) -> bool: tests/rounded_kit.MISTAKES."""
    drop = drop or O.Dropper("eval")
    mist = mistake or _nomist
    B, F, D = enc.shape
    H = P["rnn.weight_hh_l0"].shape[1]
    E = P["embedding.weight"].shape[1]
    T = O.decode_len(target_masks, caption_max_len)
    W_ih = P["rnn.weight_ih_l0"]
    We, Wc = W_ih[:, :E], W_ih[:, E:]
    toks = torch.cat((torch.full((1, B), SOS, dtype=torch.long), targets[:T - 1]), 0)                    # train.py:25,45
    emb = torch.stack([drop(P["embedding.weight"][toks[t]] * emb_scale, p_emb, dropmask.SITE_DEC_EMBED, t) for t in range(T)])
    Xe = mm(emb, We) + P["rnn.bias_ih_l0"]
    if cell == "LSTM":
        Xe = Xe + P["rnn.bias_hh_l0"]
    Uv = mm(enc, P["attn_U.weight"])                                                                     # [B, F, A]
    Pm = bf16(_dot(bf16(enc.detach()).reshape(B * F, D), _weight(Wc).t())).reshape(B, F, -1)
    state = _zero_state(B, H, enc)
    hs = []
    for t in range(T):
        h = state[0]
        if t >= 2 and mist("hand_over_slip", t=t):
            h = h.clone()
            b = mist("hand_over_slip", t=t)[1]
            h[b] = hs[t - 2][b]
        Wh = ground(mm(h, P["attn_W.weight"]) + P["attn_b"])
        al = (torch.tanh(Wh.unsqueeze(1) + Uv) @ P["attn_w.weight"].t()).squeeze(2)                     # [B, F], no softmax
        if mist("frame_left_out", t=t):
            keep = torch.ones_like(al)
            keep[mist("frame_left_out", t=t)[1], F - 1] = 0.0
            al = al * keep
        if t >= 1 and mist("stale_frame_weight", t=t):
            row = torch.zeros(B, F, dtype=torch.bool)
            row[mist("stale_frame_weight", t=t)[1], F - 1] = True
            al = torch.where(row, al_prev, al)
        al_prev = al
        hh = mm(h, P["rnn.weight_hh_l0"])
        if t >= 1 and mist("dwhh_row_missing", t=t):
            row = torch.zeros(B, 1, dtype=torch.bool)
            row[mist("dwhh_row_missing", t=t)[1]] = True
            with torch.no_grad():
                wdet = P["rnn.weight_hh_l0"].detach().clone()
            hh = torch.where(row, mm(h, wdet), hh)
        xe = Xe[t]
        if t >= 1 and mist("stale_input_row", t=t):
            row = torch.zeros(B, 1, dtype=torch.bool)
            row[mist("stale_input_row", t=t)[1]] = True
            xe = torch.where(row, Xe[t - 1], xe)
        out, state = _cell(cell, xe + _Context.apply(al, enc, Wc, Pm), hh, P, state, True)
        hs.append(out)
    hiddens = torch.stack(hs)
    logits = ground(mm(hiddens, P["out.weight"]) + P["out.bias"])
    ce_sum, n_totals = 0.0, 0
    for t in range(T):
        lg = drop(logits[t], p_out, dropmask.SITE_DEC_LOGIT, t)
        m = target_masks[t]
        if bool(m.any()):
            ce_sum = ce_sum + torch.nn.functional.cross_entropy(lg[m], targets[t][m])                    # train.py:54-56
        n_totals += int(m.sum())
    return ce_sum / n_totals, hiddens


# ----------------------------------------------------------------------------- reconstructors
def forward_global_reconstructor(P, hiddens, enc, *, cell="LSTM", caption_max_len=30, p_drop=0.5, drop=None, mistake=None):
    """MSE / T (train.py:101-102).  hiddens [T, B, H]."""
    drop = drop or O.Dropper("eval")
    mist = mistake or _nomist
    T, B, H = hiddens.shape
    R = P["rnn.weight_hh_l0"].shape[1]
    src = hiddens
    if mist("rec_reads_zero"):
        keep = torch.ones_like(hiddens)
        keep[T - 1, 0, mist("rec_reads_zero")[1]] = 0.0
        src = hiddens * keep
    mp = src.sum(0) * (caption_max_len / float(T * T))
    xs = []
    for t in range(T):
        m = drop(mp, p_drop, dropmask.SITE_REC_INPUT, t)
        if t + 1 < T and mist("mask_t_plus_1", t=t):
            b = mist("mask_t_plus_1", t=t)[1]
            row = torch.zeros(B, 1, dtype=torch.bool)
            row[b] = True
            m = torch.where(row, drop(mp, p_drop, dropmask.SITE_REC_INPUT, t + 1), m)
        xs.append(torch.cat((src[t], m), dim=1))
    Xg = mm(torch.stack(xs), P["rnn.weight_ih_l0"]) + P["rnn.bias_ih_l0"]
    if cell == "LSTM":
        Xg = Xg + P["rnn.bias_hh_l0"]
    state = _zero_state(B, R, enc)
    hsum, hrs = 0.0, []
    for t in range(T):
        hr = state[0]
        if t >= 2 and mist("rec_hand_over_slip", t=t):
            hr = hr.clone()
            b = mist("rec_hand_over_slip", t=t)[1]
            hr[b] = hrs[t - 2][b]
        out, state = _cell(cell, Xg[t], mm(hr, P["rnn.weight_hh_l0"]), P, state, True)
        hrs.append(out)
        hsum = hsum + out
    outm = ground(mm(hsum / T, P["out.weight"]) + P["out.bias"])
    return torch.nn.functional.mse_loss(outm, enc.mean(1)) / T


def forward_local_reconstructor(P, hiddens, enc, *, cell="LSTM", p_drop=0.5, drop=None, mistake=None):
    """MSE (train.py:128).  hiddens [T, B, H]."""
    drop = drop or O.Dropper("eval")
    mist = mistake or _nomist
    T, B, H = hiddens.shape
    F = enc.shape[1]
    R = P["rnn.weight_hh_l0"].shape[1]
    src = hiddens
    if mist("rec_reads_zero"):
        keep = torch.ones_like(hiddens)
        keep[T - 1, 0, mist("rec_reads_zero")[1]] = 0.0
        src = hiddens * keep
    Ud = mm(src, P["attn_U.weight"])                                                                     # [T, B, A]
    state = _zero_state(B, R, enc)
    outs = []
    for s in range(F):
        hr = state[0]
        Whr = _WhrGroups.apply(hr, P["attn_W.weight"])
        be = torch.tanh(Whr.unsqueeze(0) + Ud + P["attn_b"]) @ P["attn_w.weight"].t()                    # [T, B, 1]
        x = (be * src).sum(0) / T
        xd = drop(x, p_drop, dropmask.SITE_REC_INPUT, s)
        if s + 1 < F and mist("mask_t_plus_1", t=s):
            row = torch.zeros(B, 1, dtype=torch.bool)
            row[mist("mask_t_plus_1", t=s)[1]] = True
            xd = torch.where(row, drop(x, p_drop, dropmask.SITE_REC_INPUT, s + 1), xd)
        out, state = _cell(cell, mm(xd, P["rnn.weight_ih_l0"]), mm(hr, P["rnn.weight_hh_l0"]), P, state, False)
        outs.append(out)
    out = ground(mm(torch.stack(outs), P["out.weight"]) + P["out.bias"])                                 # [F, B, R]
    return torch.nn.functional.mse_loss(out.transpose(0, 1), enc)


# ----------------------------------------------------------------------------- the step
def step_grads(decP, recP, kind, enc, targets, cells=("LSTM", "LSTM"), seed=6, *, round=True, dtype=torch.float64, chunk=False,
               caption_max_len=30, mistake=None):
    """CE, MSE, hidden states and every gradient of CE + MSE, as numpy float64 — the layout of cells_kit.oracle_grads_no_reg plus
    `hiddens` [T, B, H]."""
    dec = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in decP.items()}
    rec = None if recP is None else {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in recP.items()}
    enc = enc.to(dtype)
    masks = targets > 0
    drop = O.Dropper("hash", seed=seed)
    with mode(round=round, chunk=chunk):
        ce, hid = forward_decoder(dec, enc, targets, masks, cell=cells[0], caption_max_len=caption_max_len, drop=drop, mistake=mistake)
        loss, mse = ce, None
        if kind == "global":
            mse = forward_global_reconstructor(rec, hid, enc, cell=cells[1], caption_max_len=caption_max_len, drop=drop, mistake=mistake)
        elif kind == "local":
            mse = forward_local_reconstructor(rec, hid, enc, cell=cells[1], drop=drop, mistake=mistake)
        if mse is not None:
            loss = ce + mse
        loss.backward()
    f64 = lambda t: t.detach().to(torch.float64).numpy().copy()
    out = dict(dec_ce=float(ce.detach()), hiddens=f64(hid), dec_grad={k: f64(v.grad) for k, v in dec.items()})
    if mse is not None:
        out.update(rec_mse=float(mse.detach()), rec_grad={k: f64(v.grad) for k, v in rec.items()})
    return out
