"""Inference search with the reference's signatures (eval.py:19-33 greedy_search, eval.py:36-120 beam_search),
run as device-side loops in the HIP library (recnet_greedy_search / recnet_beam_search): no per-sample Python
list building, no host synchronisation per step — one read-back at the end.  sample_search (no counterpart in the
reference) is greedy_search's loop with a temperature / top-k draw in place of the arg-max (recnet_sample_search).
score_captions answers the opposite question — how probable are these captions under the model — with the teacher-forced
forward in eval mode (recnet_score_captions); best_of_n ranks sampled candidates by it.

Differences from the reference that a caller can observe: `input` / `hidden` must be the start state the
reference's own `evaluate()` builds (<SOS> tokens, zero hidden state, eval.py:131-141) — that is the only
state the reference ever passes; beam_width <= 8."""
import math

import torch

from . import _ops
from .engine import Engine


def _engine(decoder, encoder_outputs):
    B, F = encoder_outputs.shape[0], encoder_outputs.shape[1]
    key = (B, F, encoder_outputs.device)
    eng = decoder._step_engines.get(key)
    if eng is None:
        eng = Engine(decoder.dims(B, F), None, decoder.precision, decoder.hyper(), device=encoder_outputs.device)
        eng.bind_decoder({k: v.data for k, v in decoder.named_tensors().items()})
        decoder._step_engines[key] = eng
    # The HIP optimiser updates the parameters through raw pointers (no torch `_version` bump), so a cached "packed"
    # flag can go stale between two evaluations of a training run.  Re-packing costs a few microseconds next to a
    # 31-step search: always do it.
    eng.pack_weights()
    eng._pver = decoder.weights_signature()
    eng._inv_sig = None          # the search recomputes the invariants itself
    return eng


def _check_start(config, input, hidden):
    if not bool((input == 1).all()):
        raise NotImplementedError("search starts from <SOS> (eval.py:131)")
    h = hidden[0] if isinstance(hidden, (tuple, list)) else hidden
    if bool((h != 0).any()):
        raise NotImplementedError("search starts from the zero hidden state (eval.py:134-141)")


def greedy_search(config, decoder, input, hidden, encoder_outputs):
    """eval.py:19-33.  Returns output_indices: list over steps of lists over the batch (python ints), like the
    reference's list of lists of 0-d tensors."""
    _check_start(config, input, hidden)
    eng = _engine(decoder, encoder_outputs)
    toks, n = _ops.load().greedy_search(int(eng.handle.value), encoder_outputs.contiguous())
    n = int(n.item())
    return toks[:n].cpu().tolist()


def beam_search(config, beam_width, vocab, decoder, input, hidden, encoder_outputs):
    """eval.py:36-120.  Returns top1_output_list: one token list per caption."""
    _check_start(config, input, hidden)
    eng = _engine(decoder, encoder_outputs)
    best, n = _ops.load().beam_search(int(eng.handle.value), encoder_outputs.contiguous(), int(beam_width))
    n = int(n.item())
    return best[:n].t().cpu().tolist()


def sample_search(config, decoder, input, hidden, encoder_outputs, temperature=1.0, top_k=0, seed=0):
    """greedy_search's loop (eval.py:19-33) with one draw per caption and step from softmax(logits / temperature) restricted
    to the top_k largest logits (0: no restriction; 1: the arg-max) — the reference has no counterpart.  The draw is a pure
    function of (seed, step, caption, vocabulary index): the same seed gives the same captions.  Returns (tokens, logprobs),
    both [n_steps][B] lists like greedy_search's; logprobs[t][b] is the log-probability of tokens[t][b] under the
    distribution it was drawn from.  Like the reference's loop this one goes on after a caption's <EOS> (see
    sequence_logprob)."""
    _check_temperature(temperature)
    if int(top_k) != top_k or not 0 <= top_k <= decoder.output_size:
        raise ValueError("top_k must be an integer in [0, %d] (got %r)" % (decoder.output_size, top_k))
    _check_start(config, input, hidden)
    eng = _engine(decoder, encoder_outputs)
    toks, lps, n = _ops.load().sample_search(int(eng.handle.value), encoder_outputs.contiguous(), float(temperature), int(top_k),
                                             int(seed) & 0xFFFFFFFF)
    n = int(n.item())
    return toks[:n].cpu().tolist(), lps[:n].cpu().tolist()


def sequence_logprob(tokens, logprobs, eos=2):
    """Per-caption sum of `logprobs` ([n_steps][B], as sample_search returns them) up to and including the caption's first
    <EOS>, or over all steps when it has none: the log-probability of the caption as the scorers read it."""
    B = len(tokens[0]) if tokens else 0
    out = []
    for b in range(B):
        total = 0.0
        for t in range(len(tokens)):
            total += logprobs[t][b]
            if tokens[t][b] == eos:
                break
        out.append(total)
    return out


def _check_temperature(temperature):
    if not (isinstance(temperature, (int, float)) and math.isfinite(temperature) and temperature > 0):
        raise ValueError("temperature must be a positive finite number (got %r)" % (temperature,))


def _caption_tensor(config, decoder, B, captions):
    """The checks of score_captions on `captions`; returns them as a [T, B] LongTensor (where they already live, if a tensor)."""
    V, Tmax = decoder.output_size, config.caption_max_len + 1
    if isinstance(captions, torch.Tensor):
        if captions.dim() != 2 or captions.dtype != torch.long:
            raise ValueError("captions must be a [T, B] LongTensor (got %s %s)" % (captions.dtype, tuple(captions.shape)))
        T = captions.shape[0]
        if captions.shape[1] != B:
            raise ValueError("captions hold %d captions per step, encoder_outputs %d" % (captions.shape[1], B))
        rows = None
    else:
        rows = [list(r) for r in captions]
        T = len(rows)
        for t, r in enumerate(rows):
            if len(r) != B:
                raise ValueError("captions[%d] holds %d tokens, encoder_outputs %d captions" % (t, len(r), B))
    if not 1 <= T <= Tmax:
        raise ValueError("captions must have between 1 and caption_max_len + 1 = %d steps (got %d)" % (Tmax, T))
    if rows is not None:
        for t, r in enumerate(rows):
            for b, k in enumerate(r):
                if int(k) != k or not 0 <= k < V:
                    raise ValueError("captions[%d][%d] = %r is not a token in [0, %d)" % (t, b, k, V))
        return torch.tensor(rows, dtype=torch.long)
    if B > 0:
        lo, hi = (int(x) for x in torch.stack([captions.min(), captions.max()]).tolist())      # one read-back
        if lo < 0 or hi >= V:
            raise ValueError("captions hold the token %d, outside [0, %d)" % (lo if lo < 0 else hi, V))
    return captions


def _score(decoder, encoder_outputs, tokens, temperature, reuse_features):
    """Device tensors (logprobs [T, B], caption_logprob [B], lengths [B]) of checked tokens [T, B]."""
    eng = _engine(decoder, encoder_outputs)
    enc = None if reuse_features else encoder_outputs.contiguous()
    return _ops.load().score_captions(int(eng.handle.value), enc, tokens.to(encoder_outputs.device).contiguous(), float(temperature))


def score_captions(config, decoder, encoder_outputs, captions, temperature=1.0, reuse_features=False):
    """How probable are `captions` under the model: the reference's teacher-forced loop (train.py:25,45) in eval mode — step 0
    is fed <SOS> and the zero state, step t > 0 is fed captions[t - 1] — on the device (recnet_score_captions).  captions:
    a [n_steps][B] list of lists, exactly what greedy_search / sample_search return, or a [T, B] LongTensor; tokens in [0, V).
    Returns (logprobs [T][B], caption_logprob [B], lengths [B]) as Python lists: logprobs[t][b] is the log-probability of
    captions[t][b] under softmax(logits_t / temperature), every row; lengths[b] = the position of the caption's first <EOS>
    + 1 (T when it has none); caption_logprob[b] = the sum of the first lengths[b] rows (the rule of sequence_logprob).
    reuse_features=True: the caller asserts that the previous call on this decoder used the same encoder_outputs and
    parameters — the loop invariants (Uv, P) are not recomputed.  Arguments are checked before anything is launched."""
    _check_temperature(temperature)
    if encoder_outputs.dim() != 3:
        raise ValueError("encoder_outputs must be [B, F, D] (got %s)" % (tuple(encoder_outputs.shape),))
    tokens = _caption_tensor(config, decoder, encoder_outputs.shape[0], captions)
    lps, cap, ln = _score(decoder, encoder_outputs, tokens, temperature, reuse_features)
    return lps.cpu().tolist(), cap.cpu().tolist(), ln.cpu().tolist()


def pick_best_of_n(caption_logprobs, lengths):
    """The selection rule of best_of_n on host tables [n][B]: for each caption the candidate k with the largest
    caption_logprobs[k][b] / lengths[k][b], the lowest k among equals.  Returns (chosen k [B], normalised score [B])."""
    n = len(caption_logprobs)
    B = len(caption_logprobs[0]) if n else 0
    ks, scores = [], []
    for b in range(B):
        best_k, best = 0, caption_logprobs[0][b] / lengths[0][b]
        for k in range(1, n):
            s = caption_logprobs[k][b] / lengths[k][b]
            if s > best:
                best_k, best = k, s
        ks.append(best_k); scores.append(best)
    return ks, scores


def best_of_n(config, decoder, input, hidden, encoder_outputs, n, temperature=1.0, top_k=0, seed=0):
    """n sampled candidates per video, ranked by the model's own length-normalised log-probability.  Candidate k is
    sample_search's rollout with seed (seed + k) & 0xFFFFFFFF; every candidate set is scored by score_captions at temperature
    1 (the sampler's own log-probabilities are under the tempered / cut distribution), the invariants of the features computed
    once and reused for k >= 1; per video the candidate with the largest caption_logprob / length wins, the lowest k among
    equals.  Returns (captions: [B] token lists cut after their <EOS>, chosen k [B], normalised score [B])."""
    if int(n) != n or n < 1:
        raise ValueError("n must be a positive integer (got %r)" % (n,))
    cands = [sample_search(config, decoder, input, hidden, encoder_outputs, temperature, top_k, (seed + k) & 0xFFFFFFFF)[0]
             for k in range(int(n))]
    caps, lens = [], []
    for k, toks in enumerate(cands):
        tokens = _caption_tensor(config, decoder, encoder_outputs.shape[0], toks)
        _, cap, ln = _score(decoder, encoder_outputs, tokens, 1.0, k > 0)
        caps.append(cap); lens.append(ln)
    caps = torch.stack(caps).cpu().tolist()          # one read-back each for the n x B sums and lengths
    lens = torch.stack(lens).cpu().tolist()
    ks, scores = pick_best_of_n(caps, lens)
    out = [[cands[k][t][b] for t in range(lens[k][b])] for b, k in enumerate(ks)]
    return out, ks, scores
