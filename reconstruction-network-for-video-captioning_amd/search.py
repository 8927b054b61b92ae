"""Inference search with the reference's signatures (eval.py:19-33 greedy_search, eval.py:36-120 beam_search),
run as device-side loops in the HIP library (recnet_greedy_search / recnet_beam_search): no per-sample Python
list building, no host synchronisation per step — one read-back at the end.  sample_search (no counterpart in the
reference) is greedy_search's loop with a temperature / top-k draw in place of the arg-max (recnet_sample_search).
score_captions answers the opposite question — how probable are these captions under the model — with the teacher-forced
forward in eval mode (recnet_score_captions); best_of_n ranks sampled candidates by it.  reconstruction_errors asks the
question the model was built around — how well does the reconstructor recover a video's features from the decoder states of
a caption (recnet_reconstruction_error) — and best_of_n can rank by that as well.  beam_search_nbest is a second beam search,
standard in its scoring (sums of log-softmax, recnet_beam_search_nbest): it returns all beam_width hypotheses with scores that
compare with score_captions / sequence_logprob, and best_of_beam reranks them by the reconstructor.  consensus_scores ranks candidates
by their n-gram overlap with one another (minimum-Bayes-risk selection, recnet_consensus_rows): best_of_n and best_of_beam add it to
their score on request, on the candidates where the searches leave them.  stochastic_beam_search draws beam_width DIFFERENT captions
per video, a sample without replacement from the model's distribution, in one search (recnet_stochastic_beam_search); sbs_weights
gives their importance weights, and best_of_n(distinct=True) reranks them in place of n rollouts.

Differences from the reference that a caller can observe: `input` / `hidden` must be the start state the
reference's own `evaluate()` builds (<SOS> tokens, zero hidden state, eval.py:131-141) — that is the only
state the reference ever passes; beam_width <= 8."""
import math
import numbers

import numpy as np
import torch

from . import _lib, _ops
from .engine import Engine


class Ensemble:
    """Several decoders that are decoded together, passed where the calls of this module take `decoder`:
    beam_search_nbest, best_of_beam (with consensus_weight), score_captions, loop.evaluate's "beam_nbest" / "beam_consensus" and
    loop.perplexity.  decoders: 1 to 8 different Decoder objects that share the vocabulary and the feature size; embedding, hidden
    and attention sizes, the cell and the precision may differ.  weights: one positive finite number per member (None: uniform),
    normalised to sum 1.  mode "arithmetic": the ensemble's distribution is the weighted mean of the members' probabilities;
    "geometric": the renormalised weighted mean of their log-probabilities.  At every step every member is fed the ensemble's
    token and keeps its own state.  Arguments are checked here; no library is loaded.  An ensemble of one is that decoder, bit for
    bit."""

    def __init__(self, decoders, weights=None, mode="arithmetic"):
        members = list(decoders)
        if not 1 <= len(members) <= _lib.ENS_MAX_M:
            raise ValueError("an ensemble has between 1 and %d members (got %d)" % (_lib.ENS_MAX_M, len(members)))
        if len({id(d) for d in members}) != len(members):
            raise ValueError("the members of an ensemble must be different objects: each keeps its own state (build a second decoder with "
                             "the same parameters to use one twice)")
        w = [1.0] * len(members) if weights is None else list(weights)
        if len(w) != len(members):
            raise ValueError("%d weights for %d members" % (len(w), len(members)))
        for x in w:
            if not (isinstance(x, numbers.Real) and math.isfinite(x) and x > 0):
                raise ValueError("ensemble weights must be positive finite numbers (got %r)" % (x,))
        if mode not in _lib.ENS_MODES:
            raise ValueError('mode must be "arithmetic" or "geometric" (got %r)' % (mode,))
        for k, d in enumerate(members):
            if d.output_size != members[0].output_size or d.encoder_size != members[0].encoder_size:
                raise ValueError("member %d has vocabulary %d and feature size %d, member 0 has %d and %d"
                                 % (k, d.output_size, d.encoder_size, members[0].output_size, members[0].encoder_size))
        total = math.fsum(float(x) for x in w)
        self.members, self.mode = members, mode
        self.weights = [float(x) / total for x in w]

    # what loop.evaluate / loop.perplexity and the checks of this module ask a decoder for: member 0's
    hidden_size = property(lambda self: self.members[0].hidden_size)
    output_size = property(lambda self: self.members[0].output_size)
    encoder_size = property(lambda self: self.members[0].encoder_size)

    def eval(self):
        for d in self.members:
            d.eval()
        return self

    def parameters(self):
        for d in self.members:
            yield from d.parameters()

    def _call_args(self, engines):
        """The leading arguments of the ensemble ops: member 0's handle, the other members' handles, weights, mode."""
        hs = [int(e.handle.value) for e in engines]
        return hs[0], hs[1:], self.weights, _lib.ENS_MODES[self.mode]


def _no_ensemble(decoder, call):
    if isinstance(decoder, Ensemble):
        raise NotImplementedError("%s does not take an Ensemble: ensembles are decoded by beam_search_nbest / best_of_beam (with "
                                  "consensus_weight) and scored by score_captions" % call)


def _cached_engine(decoder, encoder_outputs, reconstructor=None, caption_max_len=None):
    """The engine the calls of this module run on, cached on the decoder.  Without the optional arguments: the decoder alone, under
    the key Decoder.forward uses — the two share one engine.  caption_max_len: that caption length instead of the engine's default
    (Tm is baked into the handle), under a key of its own.  reconstructor (with caption_max_len: the cml / T^2 rescale is baked in
    as well): decoder AND reconstructor bound, keyed by the reconstructor's kind and rebuilt for another reconstructor object."""
    B, F, dev = encoder_outputs.shape[0], encoder_outputs.shape[1], encoder_outputs.device
    shared = reconstructor is None and caption_max_len is None
    if reconstructor is not None:
        key = ("rec", reconstructor.kind, B, F, dev, int(caption_max_len))
    else:
        key = (B, F, dev) if shared else ("nbest", B, F, dev, int(caption_max_len))
    eng = decoder._step_engines.get(key)
    if reconstructor is not None and eng is not None:
        eng = eng[0] if eng[1] is reconstructor else None
    if eng is None:
        dims, hy = decoder.dims(B, F), decoder.hyper()
        if caption_max_len is not None:
            hy.update(caption_max_len=int(caption_max_len))
        if reconstructor is not None:
            dims.update(R=reconstructor.hidden_size, RA=getattr(reconstructor, "attn_size", 0), rec_cell=reconstructor.model_name)
            hy.update(reconstructor_decoder_dropout=reconstructor.decoder_dropout_p)
        eng = Engine(dims, getattr(reconstructor, "kind", None), decoder.precision, hy, device=dev)
        eng.bind_decoder({k: v.data for k, v in decoder.named_tensors().items()})
        if reconstructor is not None:
            eng.bind_reconstructor({k: v.data for k, v in reconstructor.named_tensors().items()})
        decoder._step_engines[key] = eng if reconstructor is None else (eng, reconstructor)
    # The HIP optimiser updates the parameters through raw pointers (no torch `_version` bump), so a cached "packed"
    # flag can go stale between two evaluations of a training run.  Re-packing costs a few microseconds next to a
    # 31-step search: always do it.
    eng.pack_weights()
    if shared:
        eng._pver = decoder.weights_signature()
        eng._inv_sig = None          # the search recomputes the invariants itself
    return eng


# The two named forms of _cached_engine: the points at which the tests put a poisoned engine in, to show that the argument checks
# come before any engine is asked for.
def _rec_engine(config, decoder, reconstructor, encoder_outputs):
    return _cached_engine(decoder, encoder_outputs, reconstructor, config.caption_max_len)


def _nbest_engine(config, decoder, encoder_outputs):
    return _cached_engine(decoder, encoder_outputs, caption_max_len=config.caption_max_len)


def _check_start(config, input, hidden):
    if not bool((input == 1).all()):
        raise NotImplementedError("search starts from <SOS> (eval.py:131)")
    h = hidden[0] if isinstance(hidden, (tuple, list)) else hidden
    if bool((h != 0).any()):
        raise NotImplementedError("search starts from the zero hidden state (eval.py:134-141)")


def greedy_search(config, decoder, input, hidden, encoder_outputs):
    """eval.py:19-33.  Returns output_indices: list over steps of lists over the batch (python ints), like the
    reference's list of lists of 0-d tensors."""
    _no_ensemble(decoder, "greedy_search")
    _check_start(config, input, hidden)
    eng = _cached_engine(decoder, encoder_outputs)
    toks, n = _ops.load().greedy_search(int(eng.handle.value), encoder_outputs.contiguous())
    n = int(n.item())
    return toks[:n].cpu().tolist()


def beam_search(config, beam_width, vocab, decoder, input, hidden, encoder_outputs):
    """eval.py:36-120.  Returns top1_output_list: one token list per caption."""
    _no_ensemble(decoder, "beam_search")
    _check_start(config, input, hidden)
    eng = _cached_engine(decoder, encoder_outputs)
    best, n = _ops.load().beam_search(int(eng.handle.value), encoder_outputs.contiguous(), int(beam_width))
    n = int(n.item())
    return best[:n].t().cpu().tolist()


def sample_search(config, decoder, input, hidden, encoder_outputs, temperature=1.0, top_k=0, seed=0, top_p=1.0):
    """greedy_search's loop (eval.py:19-33) with one draw per caption and step from softmax(logits / temperature) restricted
    to the top_k largest logits (0: no restriction; 1: the arg-max) — the reference has no counterpart.  The draw is a pure
    function of (seed, step, caption, vocabulary index): the same seed gives the same captions.  Returns (tokens, logprobs),
    both [n_steps][B] lists like greedy_search's; logprobs[t][b] is the log-probability of tokens[t][b] under the
    distribution it was drawn from.  Like the reference's loop this one goes on after a caption's <EOS> (see
    sequence_logprob).  top_p < 1 adds a nucleus cut behind the top_k cut (recnet_sample_search_nucleus):
    of the entries top_k leaves, only the most probable ones whose mass reaches top_p are drawn from, and logprobs are under
    that set; top_p = 1.0 is the call without it."""
    _no_ensemble(decoder, "sample_search")
    _check_temperature(temperature)
    if int(top_k) != top_k or not 0 <= top_k <= decoder.output_size:
        raise ValueError("top_k must be an integer in [0, %d] (got %r)" % (decoder.output_size, top_k))
    _check_top_p(top_p)
    _check_start(config, input, hidden)
    eng = _cached_engine(decoder, encoder_outputs)
    if top_p == 1.0:
        toks, lps, n = _ops.load().sample_search(int(eng.handle.value), encoder_outputs.contiguous(), float(temperature), int(top_k),
                                                 int(seed) & 0xFFFFFFFF)
    else:
        toks, lps, _, n = _ops.load().sample_search_nucleus(int(eng.handle.value), encoder_outputs.contiguous(), float(temperature),
                                                            int(top_k), float(top_p), int(seed) & 0xFFFFFFFF)
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


def _check_top_p(top_p):
    if not (isinstance(top_p, numbers.Real) and 0 < top_p <= 1):            # (refuses NaN too)
        raise ValueError("top_p must be a number in (0, 1] (got %r)" % (top_p,))


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


_SHARED_CML = 30          # Engine's default caption_max_len: the shared engine (Decoder.forward's) takes up to 31 caption rows


def _score(decoder, encoder_outputs, tokens, temperature, reuse_features, caption_max_len=None):
    """Device tensors (logprobs [T, B], caption_logprob [B], lengths [B]) of checked tokens [T, B].  caption_max_len: the config's —
    another one than the shared engine's runs on the engine keyed by it (_nbest_engine's), whose Tm admits the caption_max_len + 1
    rows _caption_tensor lets through (the shared engine refused captions of more than 31 rows: T out of range).  decoder an
    Ensemble: the same engine of every member, recnet_score_captions_ensemble; temperature 1 only."""
    def engine_of(dec):
        if caption_max_len is None or int(caption_max_len) == _SHARED_CML:
            return _cached_engine(dec, encoder_outputs)
        return _cached_engine(dec, encoder_outputs, caption_max_len=caption_max_len)
    enc = None if reuse_features else encoder_outputs.contiguous()
    tokens = tokens.to(encoder_outputs.device).contiguous()
    if isinstance(decoder, Ensemble):
        if temperature != 1.0:
            raise NotImplementedError("score_captions with an Ensemble scores at temperature 1 (got %r)" % (temperature,))
        return _ops.load().score_captions_ensemble(*decoder._call_args([engine_of(d) for d in decoder.members]), enc, tokens)
    return _ops.load().score_captions(int(engine_of(decoder).handle.value), enc, tokens, float(temperature))


def score_captions(config, decoder, encoder_outputs, captions, temperature=1.0, reuse_features=False):
    """How probable are `captions` under the model: the reference's teacher-forced loop (train.py:25,45) in eval mode — step 0
    is fed <SOS> and the zero state, step t > 0 is fed captions[t - 1] — on the device (recnet_score_captions).  captions:
    a [n_steps][B] list of lists, exactly what greedy_search / sample_search return, or a [T, B] LongTensor; tokens in [0, V).
    Returns (logprobs [T][B], caption_logprob [B], lengths [B]) as Python lists: logprobs[t][b] is the log-probability of
    captions[t][b] under softmax(logits_t / temperature), every row; lengths[b] = the position of the caption's first <EOS>
    + 1 (T when it has none); caption_logprob[b] = the sum of the first lengths[b] rows (the rule of sequence_logprob).
    reuse_features=True: the caller asserts that the previous call on this decoder used the same encoder_outputs and
    parameters — the loop invariants (Uv, P) are not recomputed.  Arguments are checked before anything is launched.
    decoder may be an Ensemble (temperature 1): the log-probabilities are the ensemble's, the ones its beam search sums."""
    _check_temperature(temperature)
    if encoder_outputs.dim() != 3:
        raise ValueError("encoder_outputs must be [B, F, D] (got %s)" % (tuple(encoder_outputs.shape),))
    tokens = _caption_tensor(config, decoder, encoder_outputs.shape[0], captions)
    lps, cap, ln = _score(decoder, encoder_outputs, tokens, temperature, reuse_features, config.caption_max_len)
    return lps.cpu().tolist(), cap.cpu().tolist(), ln.cpu().tolist()


def canonical_captions(captions, T=None, eos=2, pad=0):
    """Captions as the model saw them in training, where targets are padded: every token behind a caption's first <EOS>
    becomes <PAD>, and <PAD> rows are appended up to T steps (T None: no rows are added).  captions: a [T0, B] LongTensor or a
    [T0][B] list of lists (search loops go on feeding a caption its own tokens after its <EOS>: sample_search).  A pure tensor
    function: a device tensor stays on its device and nothing is read back.  Returns a [max(T0, T), B] LongTensor."""
    cap = captions if isinstance(captions, torch.Tensor) else torch.tensor([list(r) for r in captions], dtype=torch.long)
    if cap.dim() != 2 or cap.dtype != torch.long:
        raise ValueError("captions must be a [T, B] LongTensor (got %s %s)" % (cap.dtype, tuple(cap.shape)))
    T0, B = cap.shape
    if T is not None and (int(T) != T or T < T0):
        raise ValueError("T must be an integer >= the %d steps of the captions (got %r)" % (T0, T))
    is_eos = (cap == eos).long()
    behind = (is_eos.cumsum(0) - is_eos) > 0                 # strictly behind the caption's first <EOS>
    out = cap.masked_fill(behind, pad)
    if T is not None and T > T0:
        out = torch.cat([out, out.new_full((int(T) - T0, B), pad)], dim=0)
    return out


def _check_reconstructor(config, decoder, reconstructor, encoder_outputs):
    if getattr(reconstructor, "kind", None) not in ("global", "local"):
        raise ValueError("reconstructor must be a GlobalReconstructor or a LocalReconstructor (got %r)" % (type(reconstructor).__name__,))
    if encoder_outputs.dim() != 3:
        raise ValueError("encoder_outputs must be [B, F, D] (got %s)" % (tuple(encoder_outputs.shape),))
    if reconstructor.decoder_hidden_size != decoder.hidden_size:
        raise ValueError("the reconstructor reads decoder states of size %d, the decoder's are %d"
                         % (reconstructor.decoder_hidden_size, decoder.hidden_size))
    if reconstructor.hidden_size != encoder_outputs.shape[2] or decoder.encoder_size != encoder_outputs.shape[2]:
        raise ValueError("encoder_outputs have %d features per frame, the decoder expects %d and the reconstructor rebuilds %d"
                         % (encoder_outputs.shape[2], decoder.encoder_size, reconstructor.hidden_size))
    if reconstructor.kind == "global" and reconstructor.caption_max_len != config.caption_max_len:
        raise ValueError("the global reconstructor was built for caption_max_len %d, the config says %d"
                         % (reconstructor.caption_max_len, config.caption_max_len))
    if reconstructor.precision != decoder.precision:
        raise ValueError("decoder (%s) and reconstructor (%s) must share one precision" % (decoder.precision, reconstructor.precision))


def _check_recon_weight(config, decoder, reconstructor, encoder_outputs, recon_weight):
    """The checks of best_of_n / best_of_beam on their reranking arguments; returns (the reconstructor takes part, the weight)."""
    if reconstructor is None and recon_weight != 0:
        raise ValueError("recon_weight = %r needs a reconstructor" % (recon_weight,))
    if reconstructor is None or recon_weight == 0:
        return False, 0.0
    if not (isinstance(recon_weight, numbers.Real) and math.isfinite(recon_weight)):   # (numpy scalars are numbers.Real too)
        raise ValueError("recon_weight must be a finite number (got %r)" % (recon_weight,))
    _check_reconstructor(config, decoder, reconstructor, encoder_outputs)
    return True, float(recon_weight)


def _rec_errors(config, decoder, reconstructor, encoder_outputs, tokens, want_recon=False):
    """Device tensors (err [B], recon or an empty tensor) of checked, canonical tokens [T, B]."""
    eng = _rec_engine(config, decoder, reconstructor, encoder_outputs)
    return _ops.load().reconstruction_error(int(eng.handle.value), encoder_outputs.contiguous(),
                                            tokens.to(encoder_outputs.device).contiguous(), None, bool(want_recon))


def reconstruction_errors(config, decoder, reconstructor, encoder_outputs, captions, T=None, want_recon=False):
    """How well does the reconstructor recover each video's features from the decoder states of its caption
    (recnet_reconstruction_error): the teacher-forced decoder forward of score_captions in eval mode, the reconstructor's
    forward in eval mode on the states it leaves, and per caption the mean squared error the reference only ever averages over
    the batch (train.py:99-102 global, divided by T; train.py:128 local) — the mean of the returned values is the reference's
    MSE term.  captions as for score_captions; they are canonicalised first (canonical_captions: <PAD> behind the first <EOS>,
    <PAD> rows up to T).  The global error depends on T: compare errors of one video only at a common T.  Returns err [B] as a
    list, or (err, reconstruction) with want_recon: a device tensor, global [B, R] = mean_t out_t, local [B, F, D].
    Arguments are checked before anything is launched."""
    _no_ensemble(decoder, "reconstruction_errors")
    _check_reconstructor(config, decoder, reconstructor, encoder_outputs)
    tokens = _caption_tensor(config, decoder, encoder_outputs.shape[0], captions)
    if T is not None and (int(T) != T or not tokens.shape[0] <= T <= config.caption_max_len + 1):
        raise ValueError("T must be an integer between the %d steps of the captions and caption_max_len + 1 = %d (got %r)"
                         % (tokens.shape[0], config.caption_max_len + 1, T))
    err, recon = _rec_errors(config, decoder, reconstructor, encoder_outputs, canonical_captions(tokens, T), want_recon)
    return (err.cpu().tolist(), recon) if want_recon else err.cpu().tolist()


# ---- consensus (minimum-Bayes-risk) reranking by n-gram overlap (recnet_consensus_rows)
CONSENSUS_MAX_N, CONSENSUS_MAX_T = 32, 64
_DEVICE_ENGINES = {}


def _consensus_engine(device):
    """A handle that supplies the device only (no decoder is bound), cached per device: recnet_consensus_rows takes its shapes as
    arguments.  Like _rec_engine / _nbest_engine the point at which the tests put a poisoned engine in."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None and torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev not in _DEVICE_ENGINES:
        _DEVICE_ENGINES[dev] = Engine.device_only(dev)
    return _DEVICE_ENGINES[dev]


def _pad_eos(tokens, T, eos=2):
    """tokens [T0, B] continued to T >= T0 rows with <EOS>: the words of every caption stay what they are (<PAD> rows would add
    words to a caption without an <EOS>: to the consensus <PAD> is a word like any other)."""
    T0, B = tokens.shape
    return tokens if T == T0 else torch.cat([tokens, tokens.new_full((T - T0, B), eos)], dim=0)


def _consensus_utilities(hyp, weights=None):
    """Host table [N][B] of the self-consensus utilities of checked device captions hyp [N, T, B]: one launch, one read-back.
    weights: None (the uniform mean), or a host table [N][B] of finite numbers >= 0, one per candidate as a reference: they reach
    the kernel as consensus_scores(weights=) passes them, in float32."""
    eng = _consensus_engine(hyp.device)
    w = None if weights is None else torch.tensor(weights, dtype=torch.float64).to(hyp.device, torch.float32).contiguous()
    return _ops.load().consensus_rows(int(eng.handle.value), hyp, None, w, 6.0, False, False)[0].cpu().tolist()


def _check_consensus_weight(config, consensus_weight, n):
    """The checks of best_of_n / best_of_beam on consensus_weight; returns it as a float (0.0: the consensus takes no part)."""
    if not (isinstance(consensus_weight, numbers.Real) and math.isfinite(consensus_weight)):
        raise ValueError("consensus_weight must be a finite number (got %r)" % (consensus_weight,))
    if consensus_weight == 0:
        return 0.0
    if n > CONSENSUS_MAX_N:
        raise ValueError("consensus_weight != 0 takes at most %d candidates (got n = %r)" % (CONSENSUS_MAX_N, n))
    if config.caption_max_len + 1 > CONSENSUS_MAX_T:
        raise ValueError("consensus_weight != 0 needs caption_max_len + 1 <= %d (got %d)" % (CONSENSUS_MAX_T, config.caption_max_len + 1))
    return float(consensus_weight)


def _consensus_set(captions, name):
    """The checks of consensus_scores on one caption set; returns it as a [N, T, B] LongTensor (where it lives, if a tensor)."""
    if isinstance(captions, torch.Tensor):
        if captions.dim() != 3 or captions.dtype != torch.long:
            raise ValueError("%s must be a [N, T, B] LongTensor (got %s %s)" % (name, captions.dtype, tuple(captions.shape)))
        N, T, B = captions.shape
        sets = None
    else:
        sets = [[list(r) for r in c] for c in captions]
        N = len(sets)
        T = max((len(c) for c in sets), default=0)
        B = len(sets[0][0]) if N and sets[0] else 0
    if not 1 <= N <= CONSENSUS_MAX_N:
        raise ValueError("%s must hold between 1 and %d caption sets (got %d)" % (name, CONSENSUS_MAX_N, N))
    if sets is not None:
        for k, c in enumerate(sets):
            if not 1 <= len(c) <= CONSENSUS_MAX_T:
                raise ValueError("%s[%d] must have between 1 and %d steps (got %d)" % (name, k, CONSENSUS_MAX_T, len(c)))
            for t, r in enumerate(c):
                if len(r) != B:
                    raise ValueError("%s[%d][%d] holds %d tokens, %s[0][0] %d" % (name, k, t, len(r), name, B))
                for b, v in enumerate(r):
                    if int(v) != v or not 0 <= v < 2 ** 31:
                        raise ValueError("%s[%d][%d][%d] = %r is not a token in [0, 2^31)" % (name, k, t, b, v))
    if not 1 <= T <= CONSENSUS_MAX_T:
        raise ValueError("%s must have between 1 and %d steps (got %d)" % (name, CONSENSUS_MAX_T, T))
    if B < 1:
        raise ValueError("%s must hold at least one caption per step (got B = %d)" % (name, B))
    if sets is not None:
        return torch.stack([_pad_eos(torch.tensor(c, dtype=torch.long), T) for c in sets])
    lo, hi = (int(x) for x in torch.stack([captions.min(), captions.max()]).tolist())      # one read-back
    if lo < 0 or hi >= 2 ** 31:
        raise ValueError("%s holds the token %d, outside [0, 2^31)" % (name, lo if lo < 0 else hi))
    return captions


def consensus_scores(captions, refs=None, weights=None, sigma=6.0, want_sim=False, device=None):
    """Consensus (minimum-Bayes-risk) utilities by n-gram overlap, on the device (recnet_consensus_rows).
    The words of a caption column are its tokens before the first <EOS> (2); every other id, <PAD> included, is a word.  With
    c_n(g) the occurrences of n-gram g (n = 1..4), M_n(h, r) = sum_g min(h_n(g), r_n(g)) r_n(g) and Q_n(c) = sum_g c_n(g)^2,
        sim(h, r) = 1/4 sum_n [M_n / sqrt(Q_n(h) Q_n(r)), 0 where a Q is 0] * exp(-(L_h - L_r)^2 / (2 sigma^2))
    — coco CIDEr's clipped cosine and length penalty with a uniform idf.  U_i = (sum_j sim(i, j)) / N_r, or sum_j w_j sim(i, j)
    with weights [N_r][B] (finite, >= 0), summed in float64 over j ascending.  refs None: the captions are their own references,
    the term j = i included; candidates with the same words then get bit-equal utilities.
    captions / refs: a [N, T, B] LongTensor, or a list of N caption sets [T_k][B] (what the searches return; the T_k may differ: a
    shorter set is continued with <EOS> rows, which leaves its words as they are).  N <= 32, T <= 64, tokens in [0, 2^31).  The call
    needs a device, not a decoder: the tensor's, or `device` (for lists and CPU tensors; default: the current HIP device).  Returns
    U [N][B] as Python floats, or (U, sim [N][N_r][B]) with want_sim.  Arguments are checked before any engine is asked for."""
    if not (isinstance(sigma, numbers.Real) and math.isfinite(sigma) and sigma > 0):
        raise ValueError("sigma must be a positive finite number (got %r)" % (sigma,))
    hyp = _consensus_set(captions, "captions")
    ref = None if refs is None else _consensus_set(refs, "refs")
    if ref is not None and ref.shape[2] != hyp.shape[2]:
        raise ValueError("refs hold %d captions per step, captions %d" % (ref.shape[2], hyp.shape[2]))
    Nr, B = (hyp if ref is None else ref).shape[0], hyp.shape[2]
    w = None
    if weights is not None:
        w = weights.detach().to("cpu", torch.float64) if isinstance(weights, torch.Tensor) else None
        if w is None:
            rows = [list(r) for r in weights]
            if len(rows) != Nr or any(len(r) != B for r in rows):
                raise ValueError("weights must be [N_r = %d][B = %d]" % (Nr, B))
            w = torch.tensor(rows, dtype=torch.float64)
        if tuple(w.shape) != (Nr, B):
            raise ValueError("weights must be [N_r = %d][B = %d] (got %s)" % (Nr, B, tuple(w.shape)))
        if not bool((torch.isfinite(w) & (w >= 0)).all()):
            raise ValueError("weights must be finite and >= 0")
    if device is not None:
        dev = torch.device(device)
    else:
        dev = hyp.device if hyp.is_cuda else (ref.device if ref is not None and ref.is_cuda else torch.device("cuda"))
    eng = _consensus_engine(dev)
    dev = eng.device
    out = _ops.load().consensus_rows(int(eng.handle.value), hyp.to(dev).contiguous(), None if ref is None else ref.to(dev).contiguous(),
                                     None if w is None else w.to(dev, torch.float32).contiguous(), float(sigma), bool(want_sim), False)
    util = out[0].cpu().tolist()
    return (util, out[1].cpu().tolist()) if want_sim else util


def pick_best_of_n(caption_logprobs, lengths, rec_errors=None, recon_weight=0.0, consensus=None, consensus_weight=0.0):
    """The selection rule of best_of_n on host tables [n][B]: for each caption the candidate k with the largest score
    caption_logprobs[k][b] / lengths[k][b] - recon_weight * rec_errors[k][b] + consensus_weight * consensus[k][b], the lowest k
    among equals (rec_errors None: without the second term; consensus None: without the third — the call without the two new
    arguments computes what it always did).  consensus: the utilities of consensus_scores; candidates with the same words carry
    the same bits there, so duplicates are decided by k on every run.  Returns (chosen k [B], score [B])."""
    n = len(caption_logprobs)
    B = len(caption_logprobs[0]) if n else 0

    def score(k, b):
        s = caption_logprobs[k][b] / lengths[k][b]
        if rec_errors is not None:
            s = s - recon_weight * rec_errors[k][b]
        return s if consensus is None else s + consensus_weight * consensus[k][b]
    ks, scores = [], []
    for b in range(B):
        best_k, best = 0, score(0, b)
        for k in range(1, n):
            s = score(k, b)
            if s > best:
                best_k, best = k, s
        ks.append(best_k); scores.append(best)
    return ks, scores


def _rerank(caption_logprobs, lengths, recon_weight, rec_args, rec_tokens, consensus_weight, hyp, consensus_ref_weights=None):
    """The tail of best_of_n / best_of_beam on host tables [n][B] of sums and lengths.  rec_tokens: the n candidate sets as
    _rec_errors takes them behind its leading arguments rec_args (checked, canonical, one common T), or None: no reconstruction
    error; the n x B errors are read back once.  hyp: the candidates stacked [n, T, B] on the device, or None: no consensus.
    consensus_ref_weights: _consensus_utilities' weights (None: the uniform mean, what every caller but best_of_n(distinct=True)
    passes)."""
    errs = None if rec_tokens is None else torch.stack([_rec_errors(*rec_args, tokens)[0] for tokens in rec_tokens]).cpu().tolist()
    util = None if hyp is None else _consensus_utilities(hyp, consensus_ref_weights)
    return pick_best_of_n(caption_logprobs, lengths, errs, recon_weight, util, consensus_weight)


def _cut_winners(tokens, ks, lengths):
    """Per caption b the tokens[k][t][b] of its winner k = ks[b], cut after their <EOS> (at lengths[k][b])."""
    return [[tokens[k][t][b] for t in range(lengths[k][b])] for b, k in enumerate(ks)]


def best_of_n(config, decoder, input, hidden, encoder_outputs, n, temperature=1.0, top_k=0, seed=0, reconstructor=None,
              recon_weight=0.0, top_p=1.0, consensus_weight=0.0, distinct=False):
    """n sampled candidates per video, ranked by the model's own length-normalised log-probability.  Candidate k is
    sample_search's rollout with seed (seed + k) & 0xFFFFFFFF; every candidate set is scored by score_captions at temperature
    1 (the sampler's own log-probabilities are under the tempered / cut distribution), the invariants of the features computed
    once and reused for k >= 1; per video the candidate with the largest caption_logprob / length wins, the lowest k among
    equals.  With a reconstructor and recon_weight != 0 the score is caption_logprob / length - recon_weight * rec_error
    (pick_best_of_n): all n candidate sets are canonicalised to the common T* = the longest rollout (the global error depends
    on T, so the candidates of one video must share it) and passed to the reconstruction error; the n x B errors are read back
    once.  That costs one more decoder chain pass per candidate set — the reconstruction error runs its own teacher-forced
    forward instead of reusing the scorer's states — which keeps the log-probability half bit for bit what it is without a
    reconstructor.  top_p is sample_search's nucleus cut on the rollouts; like temperature and top_k it shapes the candidates
    only, the scores stay those of the full distribution at temperature 1.  consensus_weight != 0 adds consensus_weight * U_k to
    the score, U the consensus utilities of the n candidates among themselves (consensus_scores): the
    candidate sets are stacked on the device at the common length of the longest rollout, one more launch, and the n x B utilities
    are one more read-back; it needs n <= 32 and caption_max_len + 1 <= 64.  consensus_weight = 0 launches nothing new.  Returns
    (captions: [B] token lists cut after their <EOS>, chosen k [B], score [B]).
    distinct=True (needs n <= 8, top_k = 0, top_p = 1): the n candidates are the ranks of ONE
    stochastic_beam_search of width n at (temperature, seed) — n different captions per video, sampled without replacement — instead
    of n rollouts that repeat one another.  caption_logprob / length come from the search; they are re-scored by score_captions at
    temperature 1 only when temperature != 1 (the rule above: scores are those of the full distribution at temperature 1).  The
    tail is the same, except that the consensus utilities weigh reference k by sbs_weights (its normalised importance weight: the
    candidates are no longer an i.i.d. sample whose plain mean estimates the expectation).  distinct=False is the call as it was."""
    _no_ensemble(decoder, "best_of_n")
    if int(n) != n or n < 1:
        raise ValueError("n must be a positive integer (got %r)" % (n,))
    _check_top_p(top_p)
    if distinct:
        if n > 8:
            raise ValueError("distinct=True takes at most 8 candidates, the widest stochastic beam search (got n = %r)" % (n,))
        if top_k != 0 or top_p != 1.0:
            raise ValueError("distinct=True samples from the full distribution: top_k must be 0 and top_p 1 (got %r, %r); the cuts "
                             "change the distribution the stochastic beam search conditions on" % (top_k, top_p))
        _check_sbs(decoder, n, temperature)
    use_rec, recon_weight = _check_recon_weight(config, decoder, reconstructor, encoder_outputs, recon_weight)
    consensus_weight = _check_consensus_weight(config, consensus_weight, n)
    if distinct:
        toks, cum, ln, gum = _sbs(config, decoder, input, hidden, encoder_outputs, int(n), temperature, seed)
        weights = sbs_weights(cum.cpu().tolist(), gum.cpu().tolist()) if consensus_weight != 0 else None
        if temperature != 1.0:
            cum = torch.stack([_score(decoder, encoder_outputs, toks[k].contiguous(), 1.0, k > 0, config.caption_max_len)[1]
                               for k in range(int(n))])
        lens = ln.cpu().tolist()
        ks, scores = _rerank(cum.cpu().tolist(), lens, recon_weight, (config, decoder, reconstructor, encoder_outputs),
                             [toks[k] for k in range(int(n))] if use_rec else None, consensus_weight,
                             toks.contiguous() if consensus_weight != 0 else None, weights)
        return _cut_winners(toks.cpu().tolist(), ks, lens), ks, scores
    cands =[sample_search(config, decoder, input, hidden, encoder_outputs, temperature, top_k, (seed + k) & 0xFFFFFFFF, top_p)[0]
             for k in range(int(n))]
    caps, lens, checked = [], [], []
    for k, toks in enumerate(cands):
        tokens = _caption_tensor(config, decoder, encoder_outputs.shape[0], toks)
        _, cap, ln = _score(decoder, encoder_outputs, tokens, 1.0, k > 0, config.caption_max_len)
        caps.append(cap); lens.append(ln); checked.append(tokens)
    caps, lens = (torch.stack(x).cpu().tolist() for x in (caps, lens))      # one read-back each for the n x B sums and lengths
    t_star = max(tokens.shape[0] for tokens in checked)
    rec_tokens = [canonical_captions(tokens, t_star) for tokens in checked] if use_rec else None
    hyp = torch.stack([_pad_eos(tokens.to(encoder_outputs.device), t_star) for tokens in checked]) if consensus_weight != 0 else None
    ks, scores = _rerank(caps, lens, recon_weight, (config, decoder, reconstructor, encoder_outputs), rec_tokens, consensus_weight, hyp)
    return _cut_winners(cands, ks, lens), ks, scores


def _check_beam(decoder, beam_width, length_alpha):
    if int(beam_width) != beam_width or not 1 <= beam_width <= min(8, decoder.output_size):
        raise ValueError("beam_width must be an integer in [1, %d] (got %r)" % (min(8, decoder.output_size), beam_width))
    if not (isinstance(length_alpha, numbers.Real) and math.isfinite(length_alpha) and length_alpha >= 0):
        raise ValueError("length_alpha must be a finite number >= 0 (got %r)" % (length_alpha,))


def _check_constraints(config, decoder, beam_width, no_repeat_ngram, min_length, banned_tokens):
    """The checks of the constrained search; returns the banned ids as a list of ints."""
    cml, V = int(config.caption_max_len), decoder.output_size
    for name, v in (("no_repeat_ngram", no_repeat_ngram), ("min_length", min_length)):
        if not isinstance(v, numbers.Real) or int(v) != v or not 0 <= v <= cml:
            raise ValueError("%s must be an integer in [0, caption_max_len = %d] (got %r)" % (name, cml, v))
    try:
        ids = list(banned_tokens)
    except TypeError:
        raise ValueError("banned_tokens must be a sequence of token ids (got %r)" % (banned_tokens,))
    if len(ids) > 16:
        raise ValueError("at most 16 tokens can be banned (got %d)" % len(ids))
    for v in ids:
        if not isinstance(v, numbers.Real) or int(v) != v or not 0 <= v < V:
            raise ValueError("banned_tokens must be token ids in [0, %d) (got %r)" % (V, v))
        if v == 2:
            raise ValueError("<EOS> (2) cannot be banned: no hypothesis could finish")
    ids = [int(v) for v in ids]
    if len(set(ids)) != len(ids):
        raise ValueError("banned_tokens must be distinct (got %r)" % (ids,))
    if (no_repeat_ngram or min_length or ids) and beam_width + len(ids) + cml + 1 > V:
        raise ValueError("the vocabulary (%d) is too small for these constraints: beam_width + banned tokens + caption_max_len + 1 = %d "
                         "must not exceed it" % (V, beam_width + len(ids) + cml + 1))
    return ids


def _check_groups(beam_width, n_groups, diversity_penalty):
    """The checks of the diverse search on a checked beam_width."""
    if not isinstance(n_groups, numbers.Real) or int(n_groups) != n_groups or n_groups < 1 or beam_width % int(n_groups) != 0:
        raise ValueError("n_groups must be an integer >= 1 that divides beam_width = %d (got %r)" % (beam_width, n_groups))
    if not (isinstance(diversity_penalty, numbers.Real) and math.isfinite(diversity_penalty) and diversity_penalty >= 0):
        raise ValueError("diversity_penalty must be a finite number >= 0 (got %r)" % (diversity_penalty,))


def _beam_nbest(config, decoder, input, hidden, encoder_outputs, beam_width, length_alpha, no_repeat_ngram=0, min_length=0,
                banned_tokens=(), n_groups=1, diversity_penalty=0.0, want_groups=False):
    """Device tensors (tokens [bw, n_steps, B], cum [bw, B], len [bw, B], score [bw, B]) of the checked search; want_groups: and
    group [bw, B], the group of each rank."""
    _check_beam(decoder, beam_width, length_alpha)
    ids = _check_constraints(config, decoder, beam_width, no_repeat_ngram, min_length, banned_tokens)
    _check_groups(beam_width, n_groups, diversity_penalty)
    _check_start(config, input, hidden)
    if isinstance(decoder, Ensemble):    # (one member: the library launches the single-model search)
        engines = [_nbest_engine(config, d, encoder_outputs) for d in decoder.members]
        toks, cum, ln, score, group, n = _ops.load().beam_search_nbest_ensemble(*decoder._call_args(engines), encoder_outputs.contiguous(),
                                                                                int(beam_width), float(length_alpha), int(n_groups),
                                                                                float(diversity_penalty), int(no_repeat_ngram),
                                                                                int(min_length), ids)
        out = (toks[:, :int(n.item())], cum, ln, score)
        return out + (group,) if want_groups else out
    eng = _nbest_engine(config, decoder, encoder_outputs)
    if int(n_groups) == 1:
        # (constraints all off: the library launches the unconstrained selection, recnet_beam_search_nbest's own path)
        toks, cum, ln, score, n = _ops.load().beam_search_nbest_constrained(int(eng.handle.value), encoder_outputs.contiguous(),
                                                                            int(beam_width), float(length_alpha), int(no_repeat_ngram),
                                                                            int(min_length), ids)
        group = torch.zeros_like(ln) if want_groups else None
    else:
        toks, cum, ln, score, group, n = _ops.load().beam_search_nbest_diverse(int(eng.handle.value), encoder_outputs.contiguous(),
                                                                               int(beam_width), float(length_alpha), int(n_groups),
                                                                               float(diversity_penalty), int(no_repeat_ngram),
                                                                               int(min_length), ids)
    out = (toks[:, :int(n.item())], cum, ln, score)
    return out + (group,) if want_groups else out


def beam_search_nbest(config, decoder, input, hidden, encoder_outputs, beam_width, length_alpha=0.0, no_repeat_ngram=0, min_length=0,
                      banned_tokens=(), n_groups=1, diversity_penalty=0.0, return_groups=False):
    """Beam search on the model's own log-probabilities (the reference has no counterpart: its beam_search scores by
    log(sigmoid(logit))).  A hypothesis' value is the sum of log_softmax(logits_t)[token_t] over its steps — what score_captions
    and sequence_logprob return for it; a hypothesis with <EOS> is finished and carried with <PAD>; at every step the beam_width
    best continuations of all hypotheses of a caption are kept, the lowest (beam, token) among equals; the search ends when every
    hypothesis is finished or after caption_max_len + 1 steps.  The final order is by cum / length^length_alpha (0: the raw
    sum).  All beams of a step run as one batched decode step on the device (recnet_beam_search_nbest).  Returns, per caption, a
    list of beam_width tuples (tokens cut after <EOS>, cum, length, score) in rank order.  Arguments are checked before anything
    is launched.
    Three controls on what a hypothesis may emit, all off by default (recnet_beam_search_nbest_constrained):
    no_repeat_ngram = n > 0: no n-gram occurs twice in a hypothesis; min_length = m: no <EOS> before m tokens; banned_tokens: at
    most 16 ids that are never emitted (not <EOS>).  They remove candidates inside the selection, so the beam keeps its width; the
    values are not renormalised: cum is still the model's log-probability of the hypothesis, the one score_captions returns.  They
    need beam_width + len(banned_tokens) + caption_max_len + 1 <= V.
    n_groups = G > 1 (a divisor of beam_width) is diverse beam search (recnet_beam_search_nbest_diverse): the
    beam is G groups of beam_width / G hypotheses that are extended separately; inside a step the groups are decided one after the
    other, and a candidate pays diversity_penalty for every hypothesis of an earlier group that chose its token at this step.  The
    penalty steers the selection only: cum, length and score are as above, and the final order runs over all groups.  Different
    groups may still return the same caption (nbest_diversity counts).  return_groups: the tuples get the group of the hypothesis
    as a fifth field.  n_groups = 1 is the search above for any penalty.
    decoder may be an Ensemble (recnet_beam_search_nbest_ensemble): the search runs on the ensemble's
    distribution, every member on the ensemble's tokens with its own state; everything above holds, with score_captions on the
    Ensemble in place of the model's."""
    out = _beam_nbest(config, decoder, input, hidden, encoder_outputs, beam_width, length_alpha, no_repeat_ngram, min_length,
                      banned_tokens, n_groups, diversity_penalty, bool(return_groups))
    toks, cum, ln, score = (x.cpu().tolist() for x in out[:4])
    B = encoder_outputs.shape[0]
    hyps = [[([toks[r][t][b] for t in range(ln[r][b])], cum[r][b], ln[r][b], score[r][b]) for r in range(int(beam_width))]
            for b in range(B)]
    if return_groups:
        group = out[4].cpu().tolist()
        hyps = [[h + (group[r][b],) for r, h in enumerate(hb)] for b, hb in enumerate(hyps)]
    return hyps


def nbest_diversity(hyps):
    """How different the hypotheses of each caption are: hyps as beam_search_nbest returns them (per caption a list of tuples whose
    first field is the token list; bare token lists are taken as well).  Returns per caption (distinct captions, distinct-1,
    distinct-2): the number of different token lists, and the distinct unigrams / bigrams of the list divided by their total (0.0
    when there is none).  Host only."""
    out = []
    for hb in hyps:
        caps = [tuple(h[0]) if isinstance(h, tuple) else tuple(h) for h in hb]
        uni = [x for c in caps for x in c]
        bi = [c[j:j + 2] for c in caps for j in range(len(c) - 1)]
        out.append((len(set(caps)), len(set(uni)) / len(uni) if uni else 0.0, len(set(bi)) / len(bi) if bi else 0.0))
    return out


def best_of_beam(config, decoder, input, hidden, encoder_outputs, beam_width, length_alpha=0.0, reconstructor=None,
                 recon_weight=0.0, no_repeat_ngram=0, min_length=0, banned_tokens=(), n_groups=1, diversity_penalty=0.0,
                 consensus_weight=0.0):
    """The beam_width hypotheses of beam_search_nbest, reranked like best_of_n's candidates: per video the rank k with the largest
    cum / length - recon_weight * rec_error (pick_best_of_n, the lowest k among equals; without a reconstructor or with
    recon_weight = 0 the first term alone).  Every rank of the search is a canonical [n_steps, B] caption set already, so it goes to
    the reconstruction error as it is, all ranks at the common T = n_steps (the global error depends on T).  no_repeat_ngram /
    min_length / banned_tokens / n_groups / diversity_penalty are beam_search_nbest's: with groups the reconstructor is given
    hypotheses that differ.  consensus_weight != 0 adds consensus_weight * U_k, the consensus utilities of the ranks among
    themselves (consensus_scores) on the search's own device tensor: one more launch and one more read-back,
    of the beam_width x B utilities; it needs caption_max_len + 1 <= 64, and 0 launches nothing new.  Returns what best_of_n
    returns: (captions: [B] token lists cut after their <EOS>, chosen k [B], score [B]).  decoder may be an Ensemble, without a
    reconstructor: reranking an ensemble's beams by one member's reconstructor is not defined."""
    if isinstance(decoder, Ensemble) and reconstructor is not None:
        raise NotImplementedError("best_of_beam(reconstructor=) does not take an Ensemble: the reconstructor reads one decoder's states")
    use_rec, recon_weight = _check_recon_weight(config, decoder, reconstructor, encoder_outputs, recon_weight)
    consensus_weight = _check_consensus_weight(config, consensus_weight, 1)
    toks, cum, ln, _ = _beam_nbest(config, decoder, input, hidden, encoder_outputs, beam_width, length_alpha, no_repeat_ngram,
                                   min_length, banned_tokens, n_groups, diversity_penalty)
    lens = ln.cpu().tolist()
    ks, scores = _rerank(cum.cpu().tolist(), lens, recon_weight, (config, decoder, reconstructor, encoder_outputs),
                         [toks[r] for r in range(int(beam_width))] if use_rec else None, consensus_weight,
                         toks.contiguous() if consensus_weight != 0 else None)
    return _cut_winners(toks.cpu().tolist(), ks, lens), ks, scores


# ---- stochastic beam search (recnet_stochastic_beam_search)
def _check_sbs(decoder, beam_width, temperature):
    if not isinstance(beam_width, numbers.Real) or int(beam_width) != beam_width or not 1 <= beam_width <= min(8, decoder.output_size):
        raise ValueError("beam_width must be an integer in [1, %d] (got %r)" % (min(8, decoder.output_size), beam_width))
    _check_temperature(temperature)
    if isinstance(decoder, Ensemble) and temperature != 1.0:
        raise NotImplementedError("stochastic_beam_search with an Ensemble samples at temperature 1 (got %r): score_captions on an "
                                  "Ensemble has no temperature to hold the result to" % (temperature,))


def _sbs(config, decoder, input, hidden, encoder_outputs, beam_width, temperature, seed):
    """Device tensors (tokens [bw, n_steps, B], cum [bw, B], len [bw, B], gum [bw, B]) of the checked search."""
    _check_sbs(decoder, beam_width, temperature)
    _check_start(config, input, hidden)
    if isinstance(decoder, Ensemble):    # (one member: the library launches the single-model search)
        engines = [_nbest_engine(config, d, encoder_outputs) for d in decoder.members]
        toks, cum, ln, gum, n = _ops.load().stochastic_beam_search_ensemble(*decoder._call_args(engines), encoder_outputs.contiguous(),
                                                                            int(beam_width), float(temperature), int(seed) & 0xFFFFFFFF)
    else:
        eng = _nbest_engine(config, decoder, encoder_outputs)
        toks, cum, ln, gum, n = _ops.load().stochastic_beam_search(int(eng.handle.value), encoder_outputs.contiguous(), int(beam_width),
                                                                   float(temperature), int(seed) & 0xFFFFFFFF)
    return toks[:, :int(n.item())], cum, ln, gum


def stochastic_beam_search(config, decoder, input, hidden, encoder_outputs, beam_width, temperature=1.0, seed=0):
    """beam_width DIFFERENT captions per video, sampled without replacement from the model's sequence distribution at `temperature`
    (Kool, van Hoof, Welling 2019; recnet_stochastic_beam_search): Gumbel-top-k over whole captions, done lazily
    inside one beam search of that width on the batched decode step of beam_search_nbest.  Every hypothesis carries its
    log-probability cum and a perturbed score G = cum + Gumbel noise, conditioned at every step so that the best child of a
    hypothesis inherits its G; the beam keeps the beam_width largest G.  Rank 0 is an exact sample from the model (with beam_width
    = 1 the search draws sample_search(temperature, seed=seed)'s tokens, up to near-ties), ranks 0 .. beam_width - 1 are a sample
    without replacement, in descending G.  The draw is a pure function of (seed, step, slot, caption, vocabulary index).  Returns,
    per caption, a list of beam_width tuples (tokens cut after <EOS>, cum, length, G) in rank order; cum and length are what
    score_captions(temperature=temperature) returns for the tokens.  A hypothesis that reaches caption_max_len + 1 tokens without
    <EOS> is a prefix: its cum is the probability of all captions that begin with it.  sbs_weights turns (cum, G) into importance
    weights.  There are no top-k / top-p cuts, constraints or groups here: they change the distribution the conditioning assumes.
    decoder may be an Ensemble (recnet_stochastic_beam_search_ensemble), at temperature 1.  Arguments are checked before anything
    is launched."""
    toks, cum, ln, gum = (x.cpu().tolist() for x in _sbs(config, decoder, input, hidden, encoder_outputs, beam_width, temperature, seed))
    return [[([toks[r][t][b] for t in range(ln[r][b])], cum[r][b], ln[r][b], gum[r][b]) for r in range(int(beam_width))]
            for b in range(encoder_outputs.shape[0])]


def _exp_e1(c):
    """exp(c) E1(c) for float64 c > 0 (E1 the exponential integral): the power series up to 1, the continued fraction above."""
    c = np.asarray(c, dtype=np.float64)
    lo = np.minimum(c, 1.0)
    term, series = np.ones_like(lo), np.zeros_like(lo)
    for k in range(1, 40):
        term = term * -lo / k
        series = series - term / k
    small = np.exp(lo) * (-0.5772156649015329 - np.log(lo) + series)
    hi = np.maximum(c, 1.0)
    f = np.zeros_like(hi)
    for k in range(80, 0, -1):                        # 1 / (c + 1 - 1 / (c + 3 - 4 / (c + 5 - ...)))
        f = k * k / (hi + 2 * k + 1 - f)
    return np.where(c <= 1.0, small, 1.0 / (hi + 1 - f))


_LAGUERRE = np.polynomial.laguerre.laggauss(48)


def sbs_weights(cum, gum, normalize=True):
    """Importance weights of the ranks of a stochastic beam search (Kool et al. 2019, section 4.2), host only, float64.  cum, gum:
    tables [bw][B] (lists or tensors) of log-probabilities and perturbed scores in rank order.  With kappa the smallest perturbed
    score kept, rank k < bw - 1 gets w = p / q, p = exp(cum) and q = P(G > kappa) = 1 - exp(-exp(cum - kappa)) = -expm1(-exp(cum -
    kappa)), its probability of being among the first bw - 1; rank bw - 1, which sets the threshold, gets 0; width 1 gets [1].
    sum_k w_k f(y_k) then estimates E f without bias — for a kappa of Gumbels whose maximum is free.  The search pins the maximum: its
    start hypothesis has G = 0 where a free one has a Gumbel(0) draw g0, and with it exp(-kappa_free) = exp(-gum[bw - 1]) - 1 +
    exp(-g0), exp(-g0) an Exp(1) variable independent of everything the search returns (the conditioning of section 21 is a shift of
    exp(-G)).  Plugging gum[bw - 1] in for kappa is biased low; the weight returned is the mean of p / q over that variable,
        w = int_0^inf p / (1 - exp(-p (c + e))) exp(-e) de,   c = exp(-gum[bw - 1]) - 1 >= 0,
    which is unbiased (tests/test_sbs_ref.py holds it to that) and has no more variance than a weight from one draw of g0.  Evaluated
    as exp(c) E1(c), the integral of 1 / (c + e), plus a 48-point Gauss-Laguerre sum of the smooth remainder.  normalize=True divides
    by the sum over the ranks (the lower-variance, slightly biased estimator, and what a reference set's weights should be).  Returns
    [bw][B] Python floats."""
    c = torch.as_tensor(cum, dtype=torch.float64).cpu().numpy()
    g = torch.as_tensor(gum, dtype=torch.float64).cpu().numpy()
    if c.ndim != 2 or c.shape != g.shape or c.shape[0] < 1:
        raise ValueError("cum and gum must be tables [bw][B] of one shape (got %s, %s)" % (tuple(c.shape), tuple(g.shape)))
    bw = c.shape[0]
    if bw == 1:
        return np.ones_like(c).tolist()
    p = np.exp(c)
    with np.errstate(over="ignore"):
        shift = np.maximum(np.expm1(-g[bw - 1:bw]), 1e-300)              # c of the docstring (kappa <= 0; 0 only at an exact tie)
    nodes, wts = _LAGUERRE
    x = p[..., None] * (shift[..., None] + nodes)                        # [bw, B, nodes]
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        smooth = np.where(x < 1e-3, 0.5 + x / 12.0, 1.0 / -np.expm1(-x) - 1.0 / x)     # 1 / (1 - exp(-x)) - 1 / x, in [1/2, 1)
    w = np.broadcast_to(_exp_e1(shift), c.shape) + p * (smooth * wts).sum(axis=-1)
    w[bw - 1] = 0.0
    if normalize:
        w = w / w.sum(axis=0, keepdims=True)
    return w.tolist()


def ensemble_logits(ens, rows_of_logits, device=None):
    """The ensemble's logits of given rows (recnet_ensemble_mix_rows): rows_of_logits holds one [rows, V] array of logits per member
    of `ens` (tensors or anything torch.as_tensor takes).  Returns y [rows, V] float32 on the device: log of the weighted mean of
    the members' softmax (arithmetic) or the weighted mean of their log_softmax (geometric, not renormalised: log_softmax(y) is the
    ensemble's distribution in both modes).  device: for inputs that do not live on one (default: the current HIP device)."""
    if not isinstance(ens, Ensemble):
        raise ValueError("ens must be an Ensemble (got %r)" % (type(ens).__name__,))
    xs = [torch.as_tensor(x, dtype=torch.float32) for x in rows_of_logits]
    if len(xs) != len(ens.members):
        raise ValueError("%d rows of logits for %d members" % (len(xs), len(ens.members)))
    for x in xs:
        if x.dim() != 2 or x.shape != xs[0].shape or x.shape[0] < 1 or x.shape[1] != ens.output_size:
            raise ValueError("every member's logits must be [rows, V = %d] of one shape (got %s)" % (ens.output_size, tuple(x.shape)))
    dev = torch.device(device) if device is not None else next((x.device for x in xs if x.is_cuda), torch.device("cuda"))
    eng = _consensus_engine(dev)
    return _ops.load().ensemble_mix_rows(int(eng.handle.value), [x.to(eng.device).contiguous() for x in xs], ens.weights,
                                         _lib.ENS_MODES[ens.mode], False)
