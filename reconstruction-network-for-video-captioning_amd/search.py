"""Inference search with the reference's signatures (eval.py:19-33 greedy_search, eval.py:36-120 beam_search),
run as device-side loops in the HIP library (recnet_greedy_search / recnet_beam_search): no per-sample Python
list building, no host synchronisation per step — one read-back at the end.  sample_search (no counterpart in the
reference) is greedy_search's loop with a temperature / top-k draw in place of the arg-max (recnet_sample_search).

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
    if not (isinstance(temperature, (int, float)) and math.isfinite(temperature) and temperature > 0):
        raise ValueError("temperature must be a positive finite number (got %r)" % (temperature,))
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
