"""The float64 restatement of the consensus (minimum-Bayes-risk) scores, written from the definition with
Counters, and the case generator of the tests.  Nothing here knows how the kernel counts.

The words of a caption, a column t_0 .. t_{T-1}, are its tokens before the first <EOS> (2), at most T; every other id is a word,
<PAD> (0) included.  c_n(g): the occurrences of n-gram g (n = 1..4).  For a hypothesis h and a reference r
    M_n(h, r) = sum_g min(h_n(g), r_n(g)) r_n(g)        Q_n(c) = sum_g c_n(g)^2
    sim(h, r) = 1/4 sum_n [M_n / sqrt(Q_n(h) Q_n(r)) if both Q > 0 else 0] * exp(-(L_h - L_r)^2 / (2 sigma^2))
    U_i = (sum_j sim(i, j)) / N_r,  or  sum_j w_j sim(i, j) with weights;  summed over j ascending, one term after the other."""
import math
from collections import Counter

import numpy as np

EOS = 2
ORDERS = (1, 2, 3, 4)
# every value lies in [0, 1]; at most 32 terms of about 10 roundings at 1.1e-16 each stay below 1e-13: the bar is one order above
BAR = 1e-12


def words(column):
    """The tokens before the first <EOS>, as a tuple of ints."""
    out = []
    for t in column:
        if int(t) == EOS:
            break
        out.append(int(t))
    return tuple(out)


def ngram_counts(w):
    """[Counter of the n-grams of the word tuple w for n = 1..4]."""
    return [Counter(w[p:p + n] for p in range(len(w) - n + 1)) for n in ORDERS]


def overlap(hc, rc):
    """M_n for n = 1..4 of two ngram_counts."""
    return [sum(min(h[g], c) * c for g, c in r.items()) for h, r in zip(hc, rc)]


def squares(cc):
    """Q_n for n = 1..4 of one ngram_counts."""
    return [sum(c * c for c in cn.values()) for cn in cc]


def sim_from_counts(M, Qh, Qr, Lh, Lr, sigma=6.0):
    s = 0.0
    for m, qh, qr in zip(M, Qh, Qr):
        if qh > 0 and qr > 0:
            s += m / math.sqrt(qh * qr)
    return 0.25 * s * math.exp(-float(Lh - Lr) ** 2 / (2.0 * sigma * sigma))


def sim(h, r, sigma=6.0):
    """sim of two token columns (anything behind their first <EOS> is ignored)."""
    wh, wr = words(h), words(r)
    ch, cr = ngram_counts(wh), ngram_counts(wr)
    return sim_from_counts(overlap(ch, cr), squares(ch), squares(cr), len(wh), len(wr), sigma)


def utilities(sims, weights=None):
    """U of one hypothesis from its sims over the references, in the contract's order: ascending, one term after the other."""
    u = 0.0
    for j, s in enumerate(sims):
        u += s if weights is None else float(weights[j]) * s
    return u if weights is not None else u / len(sims)


def consensus(hyp, ref=None, weights=None, sigma=6.0):
    """hyp [N_h, T_h, B], ref [N_r, T_r, B] or None (the hypotheses are their own references, j = i included), weights [N_r, B] or
    None.  Returns a dict: util [N_h, B], sim [N_h, N_r, B] float64; counts [N_h, N_r, B, 4], q_hyp [N_h, B, 4], q_ref [N_r, B, 4],
    len_hyp [N_h, B], len_ref [N_r, B] int64."""
    hyp = np.asarray(hyp)
    ref = hyp if ref is None else np.asarray(ref)
    Nh, _, B = hyp.shape
    Nr = ref.shape[0]
    out = dict(util=np.zeros((Nh, B)), sim=np.zeros((Nh, Nr, B)), counts=np.zeros((Nh, Nr, B, 4), np.int64),
               q_hyp=np.zeros((Nh, B, 4), np.int64), q_ref=np.zeros((Nr, B, 4), np.int64), len_hyp=np.zeros((Nh, B), np.int64),
               len_ref=np.zeros((Nr, B), np.int64))
    for b in range(B):
        wh = [words(hyp[i, :, b]) for i in range(Nh)]
        wr = [words(ref[j, :, b]) for j in range(Nr)]
        ch, cr = [ngram_counts(w) for w in wh], [ngram_counts(w) for w in wr]
        qh, qr = [squares(c) for c in ch], [squares(c) for c in cr]
        out["q_hyp"][:, b], out["q_ref"][:, b] = qh, qr
        out["len_hyp"][:, b], out["len_ref"][:, b] = [len(w) for w in wh], [len(w) for w in wr]
        for i in range(Nh):
            sims = []
            for j in range(Nr):
                M = overlap(ch[i], cr[j])
                out["counts"][i, j, b] = M
                sims.append(sim_from_counts(M, qh[i], qr[j], len(wh[i]), len(wr[j]), sigma))
            out["sim"][i, :, b] = sims
            out["util"][i, b] = utilities(sims, None if weights is None else np.asarray(weights)[:, b])
    return out


# ---- the hand case of the contract
HAND_H, HAND_R = (5, 6, 5, 6, 7, EOS), (5, 6, 7, 8, EOS)
HAND = dict(M=[3, 2, 1, 0], Qh=[9, 6, 3, 2], Qr=[4, 3, 2, 1], sim_hr=0.34015585527383213, sim_rh=0.4804525933278298, sim_hh=1.0,
            sim_one_word=0.25, util=(0.7800519517579442, 0.6536350622185533, 0.7800519517579442))


# ---- the cases of the GPU test
# (N_h, N_r or None: the hypotheses are their own references, T_h, T_r, B)
SHAPES = [(1, 1, 1, 1, 1), (2, None, 4, None, 3), (3, 5, 5, 7, 2), (8, None, 31, None, 5), (16, None, 12, None, 101), (32, 32, 64, 64, 2)]
VOCABS = {
    "three": [3, 4, 5],                                        # heavy repetition: the clipping matters
    "forty": list(range(3, 43)),
    "high_bits": [7, 7 + 2 ** 16, 7 + 2 ** 17, 2 ** 31 - 1],   # differ only above bit 15
}


def _caption_set(N, T, B, vocab, rng):
    """[N, T, B] int64 with the columns every case must hold, as far as the shape has room, and the list of (k1, k2, b): column
    (k2, b) is a copy of column (k1, b)."""
    vocab = np.asarray(vocab, np.int64)
    x = np.zeros((N, T, B), np.int64)
    for k in range(N):
        for b in range(B):
            L = int(rng.integers(0, T + 1))
            col = vocab[rng.integers(0, len(vocab), T)]
            if L < T:
                col[L] = EOS
                tail = T - L - 1                      # behind the <EOS>: words and further <EOS>, all to be ignored
                col[L + 1:] = np.where(rng.random(tail) < 0.3, EOS, vocab[rng.integers(0, len(vocab), tail)])
            x[k, :, b] = col
    slots = [(k, b) for b in range(B) for k in range(N)]
    specials = []
    specials.append(lambda T: [EOS] + [vocab[0]] * (T - 1))                                        # <EOS> at position 0
    specials.append(lambda T: list(vocab[rng.integers(0, len(vocab), T)]))                         # no <EOS> at all
    specials.append(lambda T: [vocab[-1]] * T)                                                     # one word T times (T = 64: Q_1 = 4096)
    for L in (1, 2, 3, 4, 5):                                                                      # each order's first existing n-gram
        specials.append(lambda T, L=L: (list(vocab[rng.integers(0, len(vocab), min(L, T))]) + [EOS] * T)[:T])
    specials.append(lambda T: ([vocab[0], EOS, vocab[-1], vocab[0], EOS, vocab[0]] + [vocab[-1]] * T)[:T])   # garbage and a second <EOS>
    for (k, b), make in zip(slots, specials):
        x[k, :, b] = make(T)
    copies = []
    if N >= 2:
        for b in range(min(B, 2)):
            x[N - 1, :, b] = x[0, :, b]
            copies.append((0, N - 1, b))
    return x, copies


def make_case(shape, vocab_name, seed=0):
    """dict(hyp, ref or None, copies: copied hypothesis columns, weights [N_r, B] float32 for the weighted call)."""
    Nh, Nr, Th, Tr, B = shape
    rng = np.random.default_rng([seed, Nh, Th, B, sorted(VOCABS).index(vocab_name)])
    hyp, copies = _caption_set(Nh, Th, B, VOCABS[vocab_name], rng)
    ref = None
    if Nr is not None:
        ref, _ = _caption_set(Nr, Tr, B, VOCABS[vocab_name], rng)
        n = min(Nr, Nh)
        ref[:n, :min(Th, Tr), 0] = hyp[:n, :min(Th, Tr), 0]            # column 0: the references share words with the hypotheses
    w = rng.random((Nr if Nr is not None else Nh, B)).astype(np.float32)
    w[rng.random(w.shape) < 0.25] = 0.0
    return dict(hyp=hyp, ref=ref, copies=copies, weights=w)


def case_id(shape):
    return "Nh%d_Nr%s_Th%d_Tr%s_B%d" % (shape[0], shape[1] or "self", shape[2], shape[3] or "-", shape[4])
