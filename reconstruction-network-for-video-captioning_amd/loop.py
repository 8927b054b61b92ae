"""The shell around the train step: what train.py:227-420 and eval.py:123-169 do around the hot
path — iterate batches, log the three losses, run the validation pass, score captions with a search method, write
checkpoints — with the device work routed through this package:

  train step        feed.DeviceFeeder (H2D one batch ahead) -> hipGraph replay of the fused step, one graph per T
  validation        forward_decoder (free running, on-device arg-max feedback) + reconstructor forward, eval mode
  scoring           search.greedy_search / beam_search on the device, metrics.score_all (BLEU / CIDEr / ROUGE-L)
  checkpoints       checkpoint.save_checkpoint (the reference's dict layout)

Losses are read back only when they are logged (`log_every`), not three `.item()` syncs per iteration (train.py:275-277).
Out of scope here as in the tier: tensorboard, the MSVD files, vocabulary building.
"""
import os

import torch

from . import metrics
from .api import (GraphedStep, build_decoder, build_reconstructor, forward_decoder, forward_global_reconstructor,
                  forward_local_reconstructor)
from .checkpoint import load_checkpoint, save_checkpoint
from .dp import DataParallelTrainStep
from .feed import DeviceFeeder
from .search import (_caption_tensor, _score, beam_search, beam_search_nbest, best_of_beam, best_of_n, greedy_search,
                     sample_search, stochastic_beam_search)


class Trainer:
    """decoder / reconstructor dicts as train.py:222-225 builds them, plus the step machinery."""

    def __init__(self, C, n_vocabs, rank=0, world_size=1, group=None, use_graphs=True, eager_steps=2,
                 defer_reconstructor_update=False, plateau=None):
        """plateau: None, or dict(factor=, patience=, min_scale=, which=(0, 1)) — reduce-on-plateau on fit's validation loss: after
        `patience` validations in a row without a new best, the lr scale of the named optimisers (0 decoder, 1 reconstructor) is
        multiplied by `factor`, never below `min_scale` (FusedAdam.scale_lr: device-resident, the captured graphs follow it).
        Every rank has to see the same validation losses for the ranks to stay in step: fit validates on rank 0 only, so under
        data parallelism call plateau_step on every rank with the broadcast loss instead."""
        self.C, self.rank, self.world = C, rank, world_size
        self._plateau_init(plateau)
        self.decoder = build_decoder(n_vocabs, C)
        self.reconstructor = build_reconstructor(C) if C.use_recon else None
        self.global_batch = C.batch_size
        self.dp = DataParallelTrainStep(self.decoder, self.reconstructor, self.global_batch, rank, world_size, group=group)
        self.use_graphs, self.eager_steps = use_graphs, eager_steps
        # opt-in (measured slower at the benchmark shape): graph steps on one rank leave the
        # reconstructor's update pending for the next step to run under its decoder forward chain (api.GraphedStep);
        # flush() completes it wherever the parameters are read (validation, checkpoints, the end of fit)
        # (True: the whole update, global reconstructor; "recurrent": the split update of round 4 — d W_hh and its Adam step only)
        self.defer = defer_reconstructor_update if (defer_reconstructor_update and world_size == 1 and use_graphs and self.reconstructor is not None) else False
        self._graphs, self._static = {}, None
        self.iteration = 0
        self._eager_until = eager_steps       # optimiser step count up to which steps are launched eagerly

    # ------------------------------------------------------------------ reduce-on-plateau (host logic only)
    def _plateau_init(self, plateau):
        self.plateau = None
        if plateau is not None:
            p = dict(factor=0.5, patience=2, min_scale=0.0, which=(0, 1))
            unknown = sorted(set(plateau) - set(p))
            if unknown:
                raise ValueError("unknown plateau field(s) %s: the fields are factor, patience, min_scale, which" % unknown)
            p.update(plateau)
            p["which"] = tuple(int(w) for w in p["which"])
            if not (0.0 < float(p["factor"]) < 1.0) or int(p["patience"]) < 1 or not (0.0 <= float(p["min_scale"]) <= 1.0) \
                    or any(w not in (0, 1) for w in p["which"]):
                raise ValueError("plateau: 0 < factor < 1, patience >= 1, 0 <= min_scale <= 1, which a subset of (0, 1); got %r" % (plateau,))
            self.plateau = p
        self._plateau_best, self._plateau_bad = None, 0

    def _plateau_optimizers(self):
        models = (self.decoder, self.reconstructor)
        return [models[w]["optimizer"] for w in self.plateau["which"] if models[w] is not None]

    def plateau_step(self, val_loss):
        """One validation result: a new best resets the count; the `patience`-th result in a row without one multiplies the lr
        scale of the named optimisers by `factor`, floored at `min_scale`, and starts the count again.  Returns True when it scaled."""
        if self.plateau is None:
            return False
        val_loss = float(val_loss)
        if self._plateau_best is None or val_loss < self._plateau_best:
            self._plateau_best, self._plateau_bad = val_loss, 0
            return False
        self._plateau_bad += 1
        if self._plateau_bad < int(self.plateau["patience"]):
            return False
        self._plateau_bad = 0
        factor, floor = float(self.plateau["factor"]), float(self.plateau["min_scale"])
        scaled = False
        for opt in self._plateau_optimizers():
            cur = opt.lr_scale
            if cur * factor >= floor:
                opt.scale_lr(factor)
                scaled = True
            elif cur > floor:                 # the floor itself, once; at the floor nothing is sent
                opt.lr_scale = floor
                scaled = True
        return scaled

    def flush(self):
        """Completes a pending deferred reconstructor update (stream-ordered; a no-op when there is none)."""
        self.dp.step_impl.engine.flush()

    def resume(self, path):
        """Continue a run from a checkpoint written by `fit` (or by the reference's train.py:398-420): parameters, Adam
        state, step count and iteration are restored, the packed operand images of every bound engine are refreshed
        (checkpoint.load_checkpoint), captured graphs are dropped and the next `eager_steps` steps run eagerly again
        (module loading, RCCL set-up) before a graph is captured."""
        self.flush()
        ckpt = load_checkpoint(path, self.decoder, self.reconstructor)
        self.iteration = int(ckpt.get("iteration", self.decoder["_state"].step))
        self._graphs.clear()
        self._eager_until = self.decoder["_state"].step + self.eager_steps
        return ckpt

    def check_health(self, scalars=None):
        """Raises if a persistent chain kernel gave up a bounded wait (the step's gradients were garbage; the optimiser
        kernels skipped the update) or the loss is not finite.  Before raising, the handle is switched to the per-step
        kernels and the captured graphs are dropped, so a caller that catches the error can keep training.

        Data parallel: a collective — every rank calls it at the same iterations (fit does) and the status words are
        MAX-reduced first, so all ranks raise (and fall back) together instead of the healthy ones blocking in the next
        all-reduce.  The update itself was already skipped on EVERY rank: the affected rank marks the last gradient
        bucket with a NaN before the all-reduce (csrc/kernels_util.hpp: poison_mark_kernel / poison_collect_kernel)."""
        eng = self.dp.step_impl.engine
        st = eng.chain_status()
        bad_loss = scalars is not None and not bool(torch.isfinite(scalars[6]))
        where = ""
        if self.world > 1:
            import torch.distributed as dist
            # gloo has no bitwise OR: one MAX per status bit (9 bits) + the loss flag
            word = torch.tensor([float((st >> k) & 1) for k in range(9)] + [float(bad_loss)], device=scalars.device if scalars is not None
                                else next(self.decoder["model"].parameters()).device)
            mine = (st, bad_loss)
            dist.all_reduce(word, op=dist.ReduceOp.MAX, group=self.dp.group)
            w = word.cpu().tolist()
            st = sum(1 << k for k in range(9) if w[k] > 0)
            bad_loss = w[9] > 0
            if (st & 0xFF) and not (mine[0] & 0xFF):
                where = " (raised by another rank)"
        if st or bad_loss:
            eng.chain_reset(disable_persistent=True)
            self._graphs.clear()
            raise RuntimeError("train step %d: %s%s; the optimiser updates of the affected steps were skipped on every rank, the "
                               "engine now uses the per-step kernels" % (self.iteration, "persistent chain kernel gave up waiting "
                               "(status 0x%x: another kernel held the CUs it needs)" % st if st else "non-finite loss", where))

    def global_scalars(self, acc):
        """acc: device scalars summed over steps on THIS rank.  Under data parallelism the CE / MSE parts ([0], [3]) are
        per-rank partial sums (dp.py): all-reduce them (a collective: every rank must call this) and rebuild the derived
        values.  Returns a host list in _lib.SCALAR_NAMES order."""
        a = acc.clone()
        if self.world > 1:
            import torch.distributed as dist
            part = torch.stack([a[0], a[3]])
            dist.all_reduce(part, op=dist.ReduceOp.SUM, group=self.dp.group)
            a[0], a[3] = part[0], part[1]
        v = a.cpu().tolist()
        hy = self.decoder["_hyper"]
        v[2] = v[0] + hy["decoder_lambda_reg"] * v[1]
        v[5] = v[3] + hy["reconstructor_lambda_reg"] * v[4] if self.reconstructor else 0.0
        v[6] = v[2] + (hy["lambda_recon"] * v[5] if self.reconstructor else 0.0)
        return v

    # ------------------------------------------------------------------ one optimiser step
    def step(self, enc, targets, T, w):
        """enc [B_local,F,D], targets [31,B_local] on the device; T / w from the GLOBAL batch (feed.DeviceFeeder)."""
        self.iteration += 1
        # (decoder_teacher_forcing_ratio < 1: the draw of train.py:38 is made on the host in every iteration — eager steps only)
        if not self.use_graphs or self.dp.step_impl.teacher_forcing_ratio < 1.0 or self.decoder["_state"].step < self._eager_until:
            return self.dp(enc, targets, T, w)         # first steps eagerly: module loading, RCCL set-up
        if self._static is None:
            self._static = (torch.empty_like(enc), torch.empty_like(targets))
        senc, stg = self._static
        senc.copy_(enc); stg.copy_(targets)
        g = self._graphs.get(T)
        if g is None:                                  # one graph per loop length T (<= 31 of them)
            g = self._graphs[T] = (GraphedStep(self.dp, senc, stg, T, torch.empty_like(w), warmup=0,
                                               defer_reconstructor_update=self.defer))
        g.w.copy_(w)
        return g()

    # ------------------------------------------------------------------ validation pass, train.py:310-372
    @torch.no_grad()
    def validate(self, batches, idx2word=None):
        """batches: host (enc, targets) pairs of the GLOBAL batch size; single-rank evaluation of full batches."""
        C, dec, rec = self.C, self.decoder, self.reconstructor
        self.flush()
        dec["model"].eval()
        if rec:
            rec["model"].eval()
        tot = {"loss": 0.0, "dec": 0.0, "rec": 0.0}
        n, gt, pd = 0, [], []
        dev = next(dec["model"].parameters()).device
        for enc, targets in batches:
            enc = torch.as_tensor(enc, dtype=torch.float32).to(dev)
            targets = torch.as_tensor(targets).long().to(dev)
            dl, hid, idx = forward_decoder(dec, enc, targets, targets > 0)            # default ratio 0: free running
            rl = None
            if rec:
                fwd = forward_global_reconstructor if C.reconstructor_type == "global" else forward_local_reconstructor
                rl = fwd(hid, enc, rec)
            loss = dl + C.lambda_recon * rl if rec else dl
            tot["loss"] += float(loss) * C.batch_size
            tot["dec"] += float(dl) * C.batch_size
            tot["rec"] += (float(rl) * C.batch_size) if rec else 0.0
            n += C.batch_size
            if idx2word is not None:
                gt += [metrics.indices_to_sentence(c, idx2word) for c in targets.t().cpu().tolist()]
                pd += [metrics.indices_to_sentence(c, idx2word) for c in idx.t().cpu().tolist()]
        dec["model"].train()
        if rec:
            rec["model"].train()
        out = {k: v / max(n, 1) for k, v in tot.items()}
        out["captions"] = list(zip(gt, pd))
        return out

    # ------------------------------------------------------------------ the loop, train.py:227-420
    def fit(self, batches, n_iterations, log_every=None, val_batches=None, validate_every=None, save_every=None,
            save_dpath=None, idx2word=None, log=print, health_every=200):
        C = self.C
        lo, hi = self.dp.lo, self.dp.hi
        dev = next(self.decoder["model"].parameters()).device
        feeder = DeviceFeeder(batches, dev, C.caption_max_len, shard=(lo, hi))
        hist = []
        acc = torch.zeros(8, device=dev)
        n_acc = 0
        for enc, targets, T, w in feeder:
            sc = self.step(enc, targets, T, w)
            acc += sc                                   # stays on the device; read at log time only
            n_acc += 1
            it = self.iteration
            checked = False
            if log_every and it % log_every == 0:
                self.check_health(sc); checked = True
                # the reference divides its running sums by log_every * batch_size (train.py:282-286)
                a = [x / (n_acc * C.batch_size) for x in self.global_scalars(acc)]
                rec = {"iteration": it, "loss": a[6], "dec": a[2], "rec": a[5]}
                hist.append(rec)
                msg = "Iter {} / {} ({:.1f}%): loss {:.5f}".format(it, n_iterations, it / n_iterations * 100, a[6])
                if C.use_recon:
                    msg += " (dec {:.5f} + rec {:.5f})".format(a[2], a[5])
                log(msg)
                acc.zero_()
                n_acc = 0
            if validate_every and val_batches is not None and it % validate_every == 0 and self.rank == 0:
                v = self.validate(val_batches() if callable(val_batches) else val_batches, idx2word)
                hist.append({"iteration": it, "val_loss": v["loss"], "val_dec": v["dec"], "val_rec": v["rec"]})
                log("[Validation] Iter {} / {}: loss {:.5f} (dec {:.5f} + rec {:.5f})".format(it, n_iterations, v["loss"],
                                                                                            v["dec"], v["rec"]))
                if self.plateau_step(v["loss"]):
                    log("[Plateau] Iter {}: lr scale {}".format(it, [o.lr_scale for o in self._plateau_optimizers()]))
            if save_every and save_dpath and it % save_every == 0:
                if not checked:
                    self.check_health(sc); checked = True   # never write weights of a step that went wrong
                gl = self.global_scalars(sc)           # collective under data parallelism: every rank
                self.flush()
                if self.rank == 0:
                    os.makedirs(save_dpath, exist_ok=True)
                    save_checkpoint(os.path.join(save_dpath, "{}_checkpoint.tar".format(it)), it, self.decoder,
                                    self.reconstructor, loss=torch.tensor(gl[6]), config=C)
            # health is checked even when nothing is logged or saved (one stream sync + a 40-byte read every health_every steps)
            if not checked and health_every and (it % health_every == 0 or it >= n_iterations):
                self.check_health(sc)
            if it >= n_iterations:
                break
        self.flush()
        return hist


# ---------------------------------------------------------------------- scoring, eval.py:123-169
_CONSTRAINT_KEYS = ("no_repeat_ngram", "min_length", "banned_tokens", "n_groups", "diversity_penalty")


def _split_constraints(search_method, n):
    """(the first n fields of a beam method tuple, its optional trailing dict of constraints); anything else is refused."""
    search_method = tuple(search_method)
    if len(search_method) == n:
        return search_method, {}
    if len(search_method) != n + 1 or not isinstance(search_method[n], dict):
        raise ValueError("the %r method takes %d fields and an optional dict of constraints (got %r)" % (search_method[0], n, search_method))
    unknown = sorted(set(search_method[n]) - set(_CONSTRAINT_KEYS))
    if unknown:
        raise ValueError("unknown constraint %s: the keys are %s" % (", ".join(map(repr, unknown)), ", ".join(_CONSTRAINT_KEYS)))
    return search_method[:n], dict(search_method[n])


def _split_top_p(search_method, n):
    """A sampling search method is its n fields, optionally followed by top_p; returns (the n fields, top_p or 1.0)."""
    if len(search_method) == n:
        return search_method, 1.0
    if len(search_method) != n + 1:
        raise ValueError("the %r method takes %d fields and an optional top_p (got %r)" % (search_method[0], n, search_method))
    return search_method[:n], search_method[n]


def _arity(name, fields, n):
    """The fields of a method without a tail, which nothing else counts."""
    if len(fields) != n:
        raise ValueError("the %r method takes %d fields (got %r)" % (name, n, tuple(fields)))
    return fields


def _by_caption(steps):
    """[n_steps][B] token lists (greedy_search, sample_search) as one token list per caption."""
    return list(map(list, zip(*steps)))


# The search methods evaluate() takes besides "greedy": name -> (the fields behind the name, the optional trailing field, whether
# `reconstructor` is needed, the call).  A method is (name, *fields) or (name, *fields, tail).  The tail "top_p" is the nucleus cut
# of search.sample_search (default 1.0: none); the tail "constraints" is a dict with keys of _CONSTRAINT_KEYS, the constraints and
# groups of search.beam_search_nbest (default: none).  The call gets the five leading arguments of every runner, the fields, the tail
# and the reconstructor, and returns one token list per caption; it looks its runner up in the module's globals when it runs.
_TAILS = {"top_p": _split_top_p, "constraints": _split_constraints}
_METHODS = {
    # the reference's beam search; read by position, without an arity check: fields behind the width are ignored
    "beam": (("width",), None, False, lambda a, f, _, rec: beam_search(a[0], f[0], None, *a[1:])),
    # one sampled rollout
    "sample": (("temperature", "top_k", "seed"), "top_p", False, lambda a, f, top_p, rec: _by_caption(sample_search(*a, *f, top_p)[0])),
    # search.best_of_n: the best of n sampled candidates by the model's length-normalised log-probability, ...
    "best_of": (("n", "temperature", "top_k", "seed"), "top_p", False, lambda a, f, top_p, rec: best_of_n(*a, *f, top_p=top_p)[0]),
    # ... with recon_weight times the reconstruction error of `reconstructor` subtracted from the score, ...
    "best_of_recon": (("n", "temperature", "top_k", "seed", "recon_weight"), "top_p", True,
                      lambda a, f, top_p, rec: best_of_n(*a, *f[:4], rec, f[4], top_p)[0]),
    # ... with consensus_weight times the consensus utility of each candidate among the n added to it (search.consensus_scores:
    # n-gram overlap with the other candidates, no reconstructor and no references needed)
    "best_of_consensus": (("n", "temperature", "top_k", "seed", "consensus_weight"), "top_p", False,
                          lambda a, f, top_p, rec: best_of_n(*a, *f[:4], top_p=top_p, consensus_weight=f[4])[0]),
    # search.beam_search_nbest: the first-ranked hypothesis of the beam search on log-probabilities
    "beam_nbest": (("width", "length_alpha"), "constraints", False,
                   lambda a, f, con, rec: [hyps[0][0] for hyps in beam_search_nbest(*a, *f, **con)]),
    # search.best_of_beam: its hypotheses reranked with the reconstruction error of `reconstructor`, ...
    "beam_recon": (("width", "length_alpha", "recon_weight"), "constraints", True,
                   lambda a, f, con, rec: best_of_beam(*a, *f[:2], rec, f[2], **con)[0]),
    # ... or with their consensus utility (groups are the natural partner)
    "beam_consensus": (("width", "length_alpha", "consensus_weight"), "constraints", False,
                       lambda a, f, con, rec: best_of_beam(*a, *f[:2], consensus_weight=f[2], **con)[0]),
    # search.stochastic_beam_search: rank 0 of `width` captions sampled without replacement, an exact sample from the model
    "sbs": (("width", "temperature", "seed"), None, False,
            lambda a, f, _, rec: [hyps[0][0] for hyps in stochastic_beam_search(*a, *_arity("sbs", f, 3))]),
    # search.best_of_n(distinct=True): the best of n DIFFERENT sampled candidates (one stochastic beam search of width n) by the
    # model's length-normalised log-probability, ...
    "best_of_distinct": (("n", "temperature", "seed"), None, False,
                         lambda a, f, _, rec: best_of_n(*a, *_arity("best_of_distinct", f, 3)[:2], seed=f[2], distinct=True)[0]),
    # ... with consensus_weight times their importance-weighted consensus utility added to it
    "best_of_distinct_consensus": (("n", "temperature", "seed", "consensus_weight"), None, False,
                                   lambda a, f, _, rec: best_of_n(*a, *_arity("best_of_distinct_consensus", f, 4)[:2], seed=f[2],
                                                                  consensus_weight=f[3], distinct=True)[0]),
}


@torch.no_grad()
def evaluate(config, score_batches, decoder, search_method, idx2word, references, reconstructor=None):
    """score_batches: iterable of (vids, enc [B,F,D]) with B == config.batch_size (the score loader repeats its last
    sample to fill the batch, dataset/MSVD.py:76-93; "PAD" ids are dropped like eval.py:145).  search_method: "greedy", or a
    tuple or list in one of the forms of _METHODS, such as ("beam", 5) or ("beam_nbest", 5, 0.7, {"min_length": 3}); it is
    parsed again for every batch.  reconstructor: for the methods that rerank by it.  references: {vid: [caption strings]}.
    Returns the score dict of metrics.score_all."""
    decoder.eval()
    dev = next(decoder.parameters()).device
    B, H = config.batch_size, decoder.hidden_size
    res = {}
    for vids, enc in score_batches:
        enc = torch.as_tensor(enc, dtype=torch.float32).to(dev)
        inp = torch.full((1, B), 1, dtype=torch.long, device=dev)                      # eval.py:131
        hid = torch.zeros(1, B, H, device=dev)
        if config.decoder_model == "LSTM":
            hid = (hid, torch.zeros(1, B, H, device=dev))
        if isinstance(search_method, str):
            if search_method != "greedy":
                raise NotImplementedError("Unknown search method: {}".format(search_method))
            caps = _by_caption(greedy_search(config, decoder, inp, hid, enc))
        else:
            name = search_method[0]
            if not isinstance(name, str) or name not in _METHODS:
                raise NotImplementedError("Unknown search method: {}".format(name))
            fields, tail, needs_reconstructor, run = _METHODS[name]
            head, extra = _TAILS[tail](search_method, 1 + len(fields)) if tail else (search_method, None)
            if needs_reconstructor:
                if reconstructor is None:
                    raise ValueError('the "%s" method needs a reconstructor' % name)
                reconstructor.eval()
            caps = run((config, decoder, inp, hid, enc), head[1:], extra, reconstructor)
        for vid, c in zip(vids, caps):
            if vid != "PAD" and vid not in res:
                res[vid] = [metrics.indices_to_sentence(c, idx2word)]
    gts = {v: references[v] for v in res}
    return metrics.score_all(gts, res)


@torch.no_grad()
def perplexity(config, decoder, batches):
    """Teacher-forced per-token perplexity (the reference's validation pass, train.py:310-372, is free-running only):
    exp(-sum caption_logprob / sum length) over all captions of `batches`, (enc [B,F,D], targets [31,B]) pairs as in
    Trainer.validate; a caption counts up to and including its <EOS> (search.score_captions)."""
    decoder.eval()
    dev = next(decoder.parameters()).device
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    for enc, targets in batches:
        enc = torch.as_tensor(enc, dtype=torch.float32).to(dev)
        targets = torch.as_tensor(targets).long().to(dev)
        _, cap, ln = _score(decoder, enc, _caption_tensor(config, decoder, enc.shape[0], targets), 1.0, False, config.caption_max_len)
        total += cap.double().sum()
        count += ln.sum()
    return float(torch.exp(-total / count).item())
