"""Engine: one recnet_handle (C ABI) plus the device memory it works in.

PyTorch is used here for what the task allows it for — device allocations, the current stream
and (in dp.py) torch.distributed.  Every computation is a call into librecnet_hip.so.
"""
import ctypes as C
import weakref

import torch

from . import _lib
from ._lib import DECODER_KEYS, REC_KEYS

_KIND = {None: _lib.REC_NONE, "none": _lib.REC_NONE, "global": _lib.REC_GLOBAL, "local": _lib.REC_LOCAL}
_CELL = {"LSTM": 0, "GRU": 1}
_PREC = {"f32": _lib.PREC_F32, "fp32": _lib.PREC_F32, "bf16": _lib.PREC_BF16}


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk_tensor(t, shape, dtype, name):
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA (HIP) tensor — the RecNet HIP path has no CPU fallback" % name)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise RuntimeError("%s: expected contiguous %s %s, got %s %s" % (name, dtype, tuple(shape), t.dtype,
                                                                          tuple(t.shape)))


class FlatState:
    """A set of named fp32 tensors carved out of ONE flat device buffer (so a data-parallel
    all-reduce is a single collective over `flat`)."""

    def __init__(self, shapes, device):
        self.shapes = dict(shapes)
        n = 0
        self.offsets = {}
        for k, s in self.shapes.items():
            self.offsets[k] = n
            cnt = 1
            for d in s:
                cnt *= d
            n += (cnt + 3) // 4 * 4          # keep every tensor 16-byte aligned
        self.flat = torch.zeros(n, dtype=torch.float32, device=device)
        self.views = {}
        for k, s in self.shapes.items():
            cnt = 1
            for d in s:
                cnt *= d
            self.views[k] = self.flat[self.offsets[k]:self.offsets[k] + cnt].view(s)

    def struct(self, cls, keys):
        st = cls()
        for k in keys:
            setattr(st, k.replace(".", "_"), self.views[k].data_ptr() if k in self.views else None)
        return st


def _struct_from(cls, keys, tensors):
    st = cls()
    for k in keys:
        t = tensors.get(k)
        setattr(st, k.replace(".", "_"), None if t is None else t.data_ptr())
    return st


class Engine:
    """dims: dict with B,F,D,E,H,A,V and (optional) R, RA.  kind: None | 'global' | 'local'."""

    def __init__(self, dims, kind=None, precision="bf16", hyper=None, device=None, global_batch=None,
                 batch_offset=0):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("RecNet HIP engine needs a GPU (torch.cuda.is_available() is False)")
        self.device = torch.device(device if device is not None else "cuda")
        hy = dict(embedding_scale=1.0, embedding_dropout=0.5, decoder_out_dropout=0.5,
                  reconstructor_decoder_dropout=0.5, decoder_learning_rate=1e-5, reconstructor_learning_rate=1e-6,
                  decoder_weight_decay=1e-5, reconstructor_weight_decay=1e-5, decoder_use_amsgrad=True,
                  reconstructor_use_amsgrad=False, gradient_clip=50.0, decoder_lambda_reg=1e-3,
                  reconstructor_lambda_reg=1e-2, lambda_recon=1.0, adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-8,
                  caption_max_len=30)
        hy.update(hyper or {})
        self.hyper = hy
        self.dims = dict(dims)
        self.kind = kind if kind not in ("none",) else None
        self.precision = precision
        c = _lib.Config()
        c.batch_size = dims["B"]; c.encoder_output_len = dims["F"]; c.encoder_output_size = dims["D"]
        c.embedding_size = dims["E"]; c.decoder_hidden_size = dims["H"]; c.decoder_attn_size = dims["A"]
        c.n_vocabs = dims["V"]
        c.reconstructor_hidden_size = dims.get("R", dims["D"]) if self.kind else 0
        c.reconstructor_attn_size = dims.get("RA", 0) if self.kind == "local" else 0
        c.caption_max_len = hy["caption_max_len"]
        c.reconstructor_type = _KIND[self.kind]
        c.precision = _PREC[precision]
        c.global_batch_size = global_batch if global_batch else dims["B"]
        c.batch_offset = batch_offset
        c.decoder_cell = _CELL[dims.get("dec_cell", "LSTM")]
        c.reconstructor_cell = _CELL[dims.get("rec_cell", "LSTM")]
        c.decoder_attn_normalize = {"none": 0, "softmax": 1}[dims.get("attn_normalize", "none")]
        c.decoder_use_amsgrad = int(bool(hy["decoder_use_amsgrad"]))
        c.reconstructor_use_amsgrad = int(bool(hy["reconstructor_use_amsgrad"]))
        for k in ("embedding_scale", "embedding_dropout", "decoder_out_dropout", "reconstructor_decoder_dropout",
                  "decoder_lambda_reg", "reconstructor_lambda_reg", "lambda_recon", "decoder_learning_rate",
                  "reconstructor_learning_rate", "decoder_weight_decay", "reconstructor_weight_decay", "adam_beta1",
                  "adam_beta2", "adam_eps"):
            setattr(c, k, float(hy[k]))
        c.gradient_clip = float(hy["gradient_clip"] or 0.0)
        self.cfg = c
        self.handle = C.c_void_p()
        _lib.check(self.lib.recnet_create(C.byref(c), C.byref(self.handle)), "recnet_create")
        nbytes = self.lib.recnet_workspace_bytes(self.handle)
        with torch.cuda.device(self.device):
            self.workspace = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
            off = (-self.workspace.data_ptr()) % 256
            self._ws_ptr = self.workspace.data_ptr() + off
            _lib.check(self.lib.recnet_bind_workspace(self.handle, C.c_void_p(self._ws_ptr), C.c_size_t(nbytes)),
                       "recnet_bind_workspace")
            self.scalars = torch.zeros(8, dtype=torch.float32, device=self.device)
        self._keep = []
        self.T = None
        # what the handle steps each model with (lr, weight decay, beta1, beta2, eps): set_optimizer_hyper keeps it current
        self.opt_hyper = {w: (float(hy[n + "_learning_rate"]), float(hy[n + "_weight_decay"]), float(hy["adam_beta1"]),
                              float(hy["adam_beta2"]), float(hy["adam_eps"])) for w, n in ((0, "decoder"), (1, "reconstructor"))}
        self.captured_steps = weakref.WeakSet()      # live api.GraphedStep objects: their graphs hold opt_hyper as kernel arguments
        # the lr schedule the handle holds for each model: (LRSchedule.to_dict()'s dict or None, scale); set_lr_schedule keeps it
        # current.  Device-resident, so unlike opt_hyper it may change under a live GraphedStep.
        self.lr_sched = {0: (None, 1.0), 1: (None, 1.0)}

    @classmethod
    def device_only(cls, device=None, precision="f32"):
        """A handle that supplies a device and nothing else, for the entries that take their shapes as arguments (the row kernels
        of the searches, recnet_consensus_rows, the GEMM hooks; precision is what the `gemm` hook dispatches on)."""
        # Any handle will do, so the dims are placeholders: those entries ask the handle for a bound workspace (REQUIRE_WS in
        # csrc/host_common.inc) and for nothing else — no dims, no weights.
        return cls(dict(B=2, F=2, D=8, E=4, H=8, A=4, V=8), None, precision, device=device)

    def __del__(self):
        try:
            if getattr(self, "handle", None) is not None and self.handle.value:
                self.lib.recnet_destroy(self.handle)
                self.handle = C.c_void_p()
        except Exception:
            pass

    # ------------------------------------------------------------------ binding
    def decoder_shapes(self):
        d = self.dims
        G = 3 if d.get("dec_cell", "LSTM") == "GRU" else 4
        return {"attn_b": (d["A"],), "embedding.weight": (d["V"], d["E"]), "attn_W.weight": (d["A"], d["H"]),
                "attn_U.weight": (d["A"], d["D"]), "attn_w.weight": (1, d["A"]),
                "rnn.weight_ih_l0": (G * d["H"], d["E"] + d["D"]), "rnn.weight_hh_l0": (G * d["H"], d["H"]),
                "rnn.bias_ih_l0": (G * d["H"],), "rnn.bias_hh_l0": (G * d["H"],),
                "out.weight": (d["V"], d["H"]), "out.bias": (d["V"],)}

    def rec_shapes(self):
        d = self.dims
        R, H = d.get("R", d["D"]), d["H"]
        G = 3 if d.get("rec_cell", "LSTM") == "GRU" else 4
        s = {}
        if self.kind == "local":
            RA = d["RA"]
            s.update({"attn_b": (RA,), "attn_W.weight": (RA, R), "attn_U.weight": (RA, H), "attn_w.weight": (1, RA)})
        s.update({"rnn.weight_ih_l0": (G * R, H if self.kind == "local" else 2 * H), "rnn.weight_hh_l0": (G * R, R),
                  "rnn.bias_ih_l0": (G * R,), "rnn.bias_hh_l0": (G * R,), "out.weight": (R, R), "out.bias": (R,)})
        return s

    def bind_decoder(self, params, grads=None, exp_avg=None, exp_avg_sq=None, max_exp_avg_sq=None):
        """params etc.: dict key -> CUDA fp32 tensor (state_dict names)."""
        shp = self.decoder_shapes()
        for k in DECODER_KEYS:
            _chk_tensor(params[k], shp[k], torch.float32, "decoder." + k)
        sts = [_struct_from(_lib.DecoderTensors, DECODER_KEYS, params)]
        for grp in (grads, exp_avg, exp_avg_sq, max_exp_avg_sq):
            if grp is not None:
                for k in DECODER_KEYS:
                    _chk_tensor(grp[k], shp[k], torch.float32, "decoder state " + k)
            sts.append(None if grp is None else _struct_from(_lib.DecoderTensors, DECODER_KEYS, grp))
        self._keep.append((params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq))
        args = [C.byref(s) if s is not None else None for s in sts]
        with torch.cuda.device(self.device):
            _lib.check(self.lib.recnet_bind_decoder(self.handle, *args), "recnet_bind_decoder")

    def bind_reconstructor(self, params, grads=None, exp_avg=None, exp_avg_sq=None, max_exp_avg_sq=None):
        shp = self.rec_shapes()
        for k in shp:
            _chk_tensor(params[k], shp[k], torch.float32, "reconstructor." + k)
        sts = [_struct_from(_lib.ReconstructorTensors, REC_KEYS, params)]
        for grp in (grads, exp_avg, exp_avg_sq, max_exp_avg_sq):
            if grp is not None:
                for k in shp:
                    _chk_tensor(grp[k], shp[k], torch.float32, "reconstructor state " + k)
            sts.append(None if grp is None else _struct_from(_lib.ReconstructorTensors, REC_KEYS, grp))
        self._keep.append((params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq))
        args = [C.byref(s) if s is not None else None for s in sts]
        with torch.cuda.device(self.device):
            _lib.check(self.lib.recnet_bind_reconstructor(self.handle, *args), "recnet_bind_reconstructor")

    def set_shard(self, global_batch, batch_offset):
        _lib.check(self.lib.recnet_set_shard(self.handle, global_batch, batch_offset), "recnet_set_shard")

    def set_optimizer_hyper(self, which, lr, weight_decay, beta1, beta2, eps):
        """Adam hyper-parameters of one model (0 decoder, 1 reconstructor) for the optimiser launches enqueued from now on
        (recnet_set_optimizer_hyper; host fields only).  A graph captured earlier keeps the values it was captured with."""
        hp = (float(lr), float(weight_decay), float(beta1), float(beta2), float(eps))
        _lib.check(self.lib.recnet_set_optimizer_hyper(self.handle, int(which), *hp), "recnet_set_optimizer_hyper")
        self.opt_hyper[int(which)] = hp

    def set_lr_schedule(self, which, fields, scale=1.0):
        """The learning-rate schedule of one model's optimiser (recnet_set_lr_schedule): `fields` is LRSchedule.to_dict()'s dict or
        None (no schedule), `scale` the host-driven multiplier.  Written to the device in stream order; a live GraphedStep
        follows it from its next replay on.  A pending deferred reconstructor update is completed first, with the old schedule."""
        d = _lib.lr_desc(fields, scale)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.recnet_set_lr_schedule(self.handle, int(which), C.byref(d), _stream()), "recnet_set_lr_schedule")
        self.lr_sched[int(which)] = (dict(fields) if fields else None, float(scale))

    def get_lr_schedule(self, which):
        """The handle's host copy of the descriptor (recnet_get_lr_schedule) as a _lib.LRScheduleDesc."""
        d = _lib.LRScheduleDesc()
        _lib.check(self.lib.recnet_get_lr_schedule(self.handle, int(which), C.byref(d)), "recnet_get_lr_schedule")
        return d

    def read_lr(self):
        """(decoder lr, reconstructor lr): what the most recent Adam launch of each model stepped with, as the launch wrote it
        (recnet_read_lr; 0.0 before the first).  Synchronises the stream."""
        out = (C.c_double * 2)()
        _lib.check(self.lib.recnet_read_lr(self.handle, out, _stream()), "recnet_read_lr")
        return float(out[0]), float(out[1])

    # ------------------------------------------------------------------ hot path
    def pack_weights(self):
        _lib.check(self.lib.recnet_pack_weights(self.handle, _stream()), "recnet_pack_weights")

    def decoder_prepare(self, enc):
        d = self.dims
        _chk_tensor(enc, (d["B"], d["F"], d["D"]), torch.float32, "encoder_outputs")
        _lib.check(self.lib.recnet_decoder_prepare(self.handle, _ptr(enc), _stream()), "recnet_decoder_prepare")

    def greedy_search(self, enc):
        """eval.py:19-33 on the device.  Returns (tokens [Tm, B] int64, n_steps int32[1]) device tensors."""
        d = self.dims
        _chk_tensor(enc, (d["B"], d["F"], d["D"]), torch.float32, "encoder_outputs")
        Tm = self.hyper["caption_max_len"] + 1
        toks = torch.zeros(Tm, d["B"], dtype=torch.int64, device=self.device)
        n = torch.zeros(1, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.recnet_greedy_search(self.handle, _ptr(enc), _ptr(toks), _ptr(n), _stream()),
                   "recnet_greedy_search")
        return toks, n

    def beam_search(self, enc, beam_width):
        """eval.py:36-120 on the device.  Returns (best [Tm, B] int64, n_steps int32[1])."""
        d = self.dims
        _chk_tensor(enc, (d["B"], d["F"], d["D"]), torch.float32, "encoder_outputs")
        Tm = self.hyper["caption_max_len"] + 1
        best = torch.zeros(Tm, d["B"], dtype=torch.int64, device=self.device)
        n = torch.zeros(1, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.recnet_beam_search(self.handle, _ptr(enc), int(beam_width), _ptr(best), _ptr(n), _stream()),
                   "recnet_beam_search")
        return best, n

    @staticmethod
    def _ban_array(banned_tokens):
        """The ids as the int32 host array the constrained entries read during the call (None when there are none)."""
        ids = [int(v) for v in banned_tokens]
        if any(not -2 ** 31 <= v < 2 ** 31 for v in ids):
            raise RuntimeError("banned_tokens: ids must fit an int32 (got %r)" % (ids,))
        return ((C.c_int32 * len(ids))(*ids) if ids else None), len(ids)

    def _nbest_outputs(self, enc, beam_width, with_group=False):
        """The check of enc and the zeroed output set of the N-best searches (for a width outside [1, 8] with one rank):
        (tokens [bw, Tm, B] int64, cum, len, score [bw, B], group [bw, B] int32 or None, n_steps int32[1])."""
        d = self.dims
        _chk_tensor(enc, (d["B"], d["F"], d["D"]), torch.float32, "encoder_outputs")
        Tm, B, bw = self.hyper["caption_max_len"] + 1, d["B"], (int(beam_width) if 1 <= int(beam_width) <= 8 else 1)
        toks = torch.zeros(bw, Tm, B, dtype=torch.int64, device=self.device)
        cum = torch.zeros(bw, B, dtype=torch.float32, device=self.device)
        ln = torch.zeros(bw, B, dtype=torch.int32, device=self.device)
        score = torch.zeros(bw, B, dtype=torch.float32, device=self.device)
        group = torch.zeros(bw, B, dtype=torch.int32, device=self.device) if with_group else None
        n = torch.zeros(1, dtype=torch.int32, device=self.device)
        return toks, cum, ln, score, group, n

    @staticmethod
    def _select_rows_args(logits, cum, finished, beam_width, hist):
        """The checks of the selection inputs (logits [nb, rows, V] float32, cum [nb, rows] float32, finished [nb, rows] int32, hist
        None or [nb, rows, Tm] int64) and the outputs: (nb, rows, V, Tm, vals [rows, bw] float32, idx [rows, bw] int32)."""
        if logits.dim() != 3:
            raise RuntimeError("logits: expected [nb, rows, V], got %s" % (tuple(logits.shape),))
        nb, rows, V = logits.shape
        _chk_tensor(logits, (nb, rows, V), torch.float32, "logits")
        _chk_tensor(cum, (nb, rows), torch.float32, "cum")
        _chk_tensor(finished, (nb, rows), torch.int32, "finished")
        bw = max(int(beam_width), 1)
        vals = torch.empty(rows, bw, dtype=torch.float32, device=logits.device)
        idx = torch.empty(rows, bw, dtype=torch.int32, device=logits.device)
        Tm = 0x7FFFFFFF              # (no hist: only min_length / the static bans can be on, and they read no history)
        if hist is not None:
            if hist.dim() != 3:
                raise RuntimeError("hist: expected [nb, rows, Tm], got %s" % (tuple(hist.shape),))
            Tm = hist.shape[2]
            _chk_tensor(hist, (nb, rows, Tm), torch.int64, "hist")
        return int(nb), int(rows), int(V), int(Tm), vals, idx

    def beam_search_nbest(self, enc, beam_width, length_alpha=0.0, no_repeat_ngram=0, min_length=0, banned_tokens=()):
        """N-best beam search on log-probabilities (recnet_beam_search_nbest; the reference has none).
        no_repeat_ngram / min_length / banned_tokens (all off by default, and then the call is
        recnet_beam_search_nbest's as before): no n-gram twice in a hypothesis, no <EOS> before min_length tokens, ids that are never
        emitted; any of them on: recnet_beam_search_nbest_constrained, which checks their ranges and that the vocabulary leaves
        every live hypothesis beam_width offered tokens.
        Returns device tensors (tokens [bw, Tm, B] int64 rank-major, each rank canonical: <PAD> behind <EOS>; cum [bw, B]
        float32; len [bw, B] int32; score [bw, B] float32 = cum / len^length_alpha; n_steps int32[1]).  The library checks
        beam_width in [1, min(8, V)] and length_alpha finite and >= 0 before any launch of its own; the output tensors are
        allocated and zeroed here first (for a width outside [1, 8] with one rank), so a refused call has still run those fills:
        search.beam_search_nbest checks its arguments before anything at all."""
        toks, cum, ln, score, _, n = self._nbest_outputs(enc, beam_width)
        if no_repeat_ngram == 0 and min_length == 0 and len(banned_tokens) == 0:
            _lib.check(self.lib.recnet_beam_search_nbest(self.handle, _ptr(enc), int(beam_width), float(length_alpha), _ptr(toks),
                                                         _ptr(cum), _ptr(ln), _ptr(score), _ptr(n), _stream()),
                       "recnet_beam_search_nbest")
        else:
            ban, n_ban = self._ban_array(banned_tokens)
            _lib.check(self.lib.recnet_beam_search_nbest_constrained(self.handle, _ptr(enc), int(beam_width), float(length_alpha),
                                                                     int(no_repeat_ngram), int(min_length), ban, n_ban, _ptr(toks),
                                                                     _ptr(cum), _ptr(ln), _ptr(score), _ptr(n), _stream()),
                       "recnet_beam_search_nbest_constrained")
        return toks, cum, ln, score, n

    def beam_select_rows(self, logits, cum, finished, beam_width, hist=None, t=None, no_repeat_ngram=0, min_length=0,
                         banned_tokens=()):
        """One selection step of the N-best beam search on caller-supplied device arrays (recnet_beam_select_rows; no decoder
        needed): logits [nb, rows, V] float32 (only read), cum [nb, rows] float32, finished [nb, rows] int32.  Returns
        (vals [rows, bw] float32, idx [rows, bw] int32): the bw largest of cum_i + log_softmax(logits_i)[v] (a finished
        hypothesis offers <PAD> at cum_i alone) in descending order, idx = i * V + v, the lowest idx first among equals.
        With t given (the step, and hist [nb, rows, Tm] int64: the tokens generated so far in entries [0, t); needed for
        no_repeat_ngram only) the call is recnet_beam_select_rows_constrained's: what a live hypothesis does not offer is
        DESIGN.md section 12's."""
        # (without the step, hist is refused below, unread)
        nb, rows, V, Tm, vals, idx = self._select_rows_args(logits, cum, finished, beam_width, hist if t is not None else None)
        if t is None:
            if hist is not None or no_repeat_ngram != 0 or min_length != 0 or len(banned_tokens) != 0:
                raise RuntimeError("the constrained selection needs the step t")
            _lib.check(self.lib.recnet_beam_select_rows(self.handle, _ptr(logits), _ptr(cum), _ptr(finished), nb, rows, V,
                                                        int(beam_width), _ptr(vals), _ptr(idx), _stream()), "recnet_beam_select_rows")
            return vals, idx
        ban, n_ban = self._ban_array(banned_tokens)
        _lib.check(self.lib.recnet_beam_select_rows_constrained(self.handle, _ptr(logits), _ptr(cum), _ptr(finished), _ptr(hist), nb,
                                                                rows, V, Tm, int(t), int(beam_width), int(no_repeat_ngram),
                                                                int(min_length), ban, n_ban, _ptr(vals), _ptr(idx), _stream()),
                   "recnet_beam_select_rows_constrained")
        return vals, idx

    def beam_search_nbest_diverse(self, enc, beam_width, length_alpha=0.0, n_groups=1, diversity_penalty=0.0, no_repeat_ngram=0,
                                  min_length=0, banned_tokens=()):
        """Diverse (group) N-best beam search (recnet_beam_search_nbest_diverse): beam_search_nbest with the
        beam in n_groups groups of beam_width / n_groups slots, decided one after the other inside every step; a live candidate pays
        diversity_penalty for each slot of an earlier group that chose its token at this step.  cum stays the un-penalised
        log-probability.  Returns beam_search_nbest's tensors with group [bw, B] int32 (the group of each returned rank) before
        n_steps: (tokens, cum, len, score, group, n_steps).  The library checks the arguments before any launch of its own."""
        toks, cum, ln, score, group, n = self._nbest_outputs(enc, beam_width, with_group=True)
        ban, n_ban = self._ban_array(banned_tokens)
        _lib.check(self.lib.recnet_beam_search_nbest_diverse(self.handle, _ptr(enc), int(beam_width), float(length_alpha), int(n_groups),
                                                             float(diversity_penalty), int(no_repeat_ngram), int(min_length), ban, n_ban,
                                                             _ptr(toks), _ptr(cum), _ptr(ln), _ptr(score), _ptr(group), _ptr(n), _stream()),
                   "recnet_beam_search_nbest_diverse")
        return toks, cum, ln, score, group, n

    def beam_select_rows_diverse(self, logits, cum, finished, beam_width, n_groups, diversity_penalty, hist=None, t=0, no_repeat_ngram=0,
                                 min_length=0, banned_tokens=()):
        """One grouped selection step on caller-supplied device arrays (recnet_beam_select_rows_diverse): the
        arguments of beam_select_rows with nb = 1 (every group selects from hypothesis 0) or nb = beam_width (group g selects from
        hypotheses g * w .. g * w + w - 1, w = beam_width / n_groups).  Returns (vals [rows, bw] float32, idx [rows, bw] int32):
        slot g * w + j holds the j-th of group g by its penalised value, vals its UN-penalised value, idx = i * V + v."""
        nb, rows, V, Tm, vals, idx = self._select_rows_args(logits, cum, finished, beam_width, hist)
        ban, n_ban = self._ban_array(banned_tokens)
        _lib.check(self.lib.recnet_beam_select_rows_diverse(self.handle, _ptr(logits), _ptr(cum), _ptr(finished), _ptr(hist), nb,
                                                            rows, V, Tm, int(t), int(beam_width), int(n_groups),
                                                            float(diversity_penalty), int(no_repeat_ngram), int(min_length), ban, n_ban,
                                                            _ptr(vals), _ptr(idx), _stream()), "recnet_beam_select_rows_diverse")
        return vals, idx

    def _sample_search_outputs(self, enc, nucleus):
        """The check of enc and the zeroed outputs of the sampling searches: (tokens [Tm, B] int64, logprobs [Tm, B] float32,
        n_allowed [Tm, B] int32 or None, n_steps int32[1])."""
        d = self.dims
        _chk_tensor(enc, (d["B"], d["F"], d["D"]), torch.float32, "encoder_outputs")
        Tm = self.hyper["caption_max_len"] + 1
        toks = torch.zeros(Tm, d["B"], dtype=torch.int64, device=self.device)
        lps = torch.zeros(Tm, d["B"], dtype=torch.float32, device=self.device)
        na = torch.zeros(Tm, d["B"], dtype=torch.int32, device=self.device) if nucleus else None
        n = torch.zeros(1, dtype=torch.int32, device=self.device)
        return toks, lps, na, n

    @staticmethod
    def _sample_rows_outputs(logits, nucleus):
        """The check of logits [rows, V] float32 and the outputs of one draw per row: (rows, V, tokens [rows] int64, logprobs [rows]
        float32, n_allowed [rows] int32 or None)."""
        if logits.dim() != 2:
            raise RuntimeError("logits: expected [rows, V], got %s" % (tuple(logits.shape),))
        rows, V = logits.shape
        _chk_tensor(logits, (rows, V), torch.float32, "logits")
        toks = torch.empty(rows, dtype=torch.int64, device=logits.device)
        lps = torch.empty(rows, dtype=torch.float32, device=logits.device)
        na = torch.empty(rows, dtype=torch.int32, device=logits.device) if nucleus else None
        return int(rows), int(V), toks, lps, na

    def sample_search(self, enc, temperature=1.0, top_k=0, seed=0, top_p=1.0):
        """The loop of greedy_search with a draw from softmax(logits / temperature) over the top_k largest logits in place of
        the arg-max (recnet_sample_search; the reference has none).  Returns (tokens [Tm, B] int64, logprobs [Tm, B] float32,
        n_steps int32[1]) device tensors; only rows [:n_steps] are meaningful.  The library checks temperature / top_k.
        top_p other than 1.0: the nucleus cut of sample_search_nucleus, without its n_allowed."""
        if top_p != 1.0:
            toks, lps, _, n = self.sample_search_nucleus(enc, temperature, top_k, top_p, seed)
            return toks, lps, n
        toks, lps, _, n = self._sample_search_outputs(enc, False)
        _lib.check(self.lib.recnet_sample_search(self.handle, _ptr(enc), float(temperature), int(top_k), seed & 0xFFFFFFFF,
                                                 _ptr(toks), _ptr(lps), _ptr(n), _stream()), "recnet_sample_search")
        return toks, lps, n

    def sample_search_nucleus(self, enc, temperature=1.0, top_k=0, top_p=1.0, seed=0):
        """sample_search with a nucleus cut behind the top_k cut (recnet_sample_search_nucleus): every draw is
        from the shortest prefix of the allowed entries whose mass reaches top_p.  Returns (tokens [Tm, B] int64, logprobs [Tm, B]
        float32, n_allowed [Tm, B] int32: the size of the set each token was drawn from, n_steps int32[1]).  The library checks
        temperature / top_k / top_p (0 < top_p <= 1; 1 = no nucleus cut)."""
        toks, lps, na, n = self._sample_search_outputs(enc, True)
        _lib.check(self.lib.recnet_sample_search_nucleus(self.handle, _ptr(enc), float(temperature), int(top_k), float(top_p),
                                                         seed & 0xFFFFFFFF, _ptr(toks), _ptr(lps), _ptr(na), _ptr(n), _stream()),
                   "recnet_sample_search_nucleus")
        return toks, lps, na, n

    def sample_rows_nucleus(self, logits, temperature=1.0, top_k=0, top_p=1.0, seed=0, t=0):
        """sample_rows with the nucleus cut (recnet_sample_rows_nucleus).  Returns (tokens [rows] int64, logprobs [rows] float32,
        n_allowed [rows] int32); `logits` is only read."""
        rows, V, toks, lps, na = self._sample_rows_outputs(logits, True)
        _lib.check(self.lib.recnet_sample_rows_nucleus(self.handle, _ptr(logits), rows, V, float(temperature), int(top_k),
                                                       float(top_p), seed & 0xFFFFFFFF, int(t), _ptr(toks), _ptr(lps), _ptr(na),
                                                       _stream()), "recnet_sample_rows_nucleus")
        return toks, lps, na

    def sample_rows(self, logits, temperature=1.0, top_k=0, seed=0, t=0, top_p=1.0):
        """One draw per row of caller-supplied device logits [rows, V] (recnet_sample_rows; no decoder needed).  Returns
        (tokens [rows] int64, logprobs [rows] float32); `logits` is only read.  top_p other than 1.0: the nucleus cut of
        sample_rows_nucleus, without its n_allowed."""
        if top_p != 1.0:
            return self.sample_rows_nucleus(logits, temperature, top_k, top_p, seed, t)[:2]
        rows, V, toks, lps, _ = self._sample_rows_outputs(logits, False)
        _lib.check(self.lib.recnet_sample_rows(self.handle, _ptr(logits), rows, V, float(temperature), int(top_k),
                                               seed & 0xFFFFFFFF, int(t), _ptr(toks), _ptr(lps), _stream()),
                   "recnet_sample_rows")
        return toks, lps

    def logprob_rows(self, logits, tokens, temperature=1.0):
        """Log-probability of tokens[r] under softmax(logits[r] / temperature) for caller-supplied device logits [rows, V]
        (recnet_logprob_rows; no decoder needed).  tokens [rows] int64; one outside [0, V) gives -inf.  Returns logprobs [rows]
        float32; `logits` is only read."""
        if logits.dim() != 2:
            raise RuntimeError("logits: expected [rows, V], got %s" % (tuple(logits.shape),))
        rows, V = logits.shape
        _chk_tensor(logits, (rows, V), torch.float32, "logits")
        _chk_tensor(tokens, (rows,), torch.int64, "tokens")
        lps = torch.empty(rows, dtype=torch.float32, device=logits.device)
        _lib.check(self.lib.recnet_logprob_rows(self.handle, _ptr(logits), _ptr(tokens), int(rows), int(V), float(temperature),
                                                _ptr(lps), _stream()), "recnet_logprob_rows")
        return lps

    def consensus_rows(self, hyp, ref=None, weights=None, sigma=6.0, want_sim=False, want_counts=False):
        """Consensus (minimum-Bayes-risk) utilities of hypotheses against a reference set by n-gram overlap (recnet_consensus_rows;
        DESIGN.md section 16; no decoder needed, and B is the tensors', not the engine's).  hyp [N_h, T_h, B] int64 as
        beam_search_nbest leaves its tokens; ref [N_r, T_r, B] int64, or None: the hypotheses are their own references, the term
        j = i included; weights [N_r, B] float32 or None (uniform 1 / N_r).  Tokens in [0, 2^31): the caller's duty
        (search.consensus_scores checks).  Returns util [N_h, B] float64; with want_sim (util, sim [N_h, N_r, B] float64); with
        want_counts a dict of int32 tensors follows: counts [N_h, N_r, B, 4] (M_n), q_hyp [N_h, B, 4], q_ref [N_r, B, 4], len_hyp
        [N_h, B], len_ref [N_r, B].  The library checks the ranges of N, T and sigma; the inputs are only read."""
        if hyp.dim() != 3:
            raise RuntimeError("hyp: expected [N_h, T_h, B], got %s" % (tuple(hyp.shape),))
        Nh, Th, B = hyp.shape
        _chk_tensor(hyp, (Nh, Th, B), torch.int64, "hyp")
        Nr, Tr = Nh, Th
        if ref is not None:
            if ref.dim() != 3:
                raise RuntimeError("ref: expected [N_r, T_r, B], got %s" % (tuple(ref.shape),))
            Nr, Tr = ref.shape[:2]
            _chk_tensor(ref, (Nr, Tr, B), torch.int64, "ref")
        if weights is not None:
            _chk_tensor(weights, (Nr, B), torch.float32, "weights")
        dev = hyp.device
        util = torch.empty(Nh, B, dtype=torch.float64, device=dev)
        sim = torch.empty(Nh, Nr, B, dtype=torch.float64, device=dev) if want_sim else None
        ints = None
        if want_counts:
            ints = {k: torch.empty(*s, dtype=torch.int32, device=dev) for k, s in
                    (("counts", (Nh, Nr, B, 4)), ("q_hyp", (Nh, B, 4)), ("q_ref", (Nr, B, 4)), ("len_hyp", (Nh, B)), ("len_ref", (Nr, B)))}
        ip = [_ptr(ints[k] if ints else None) for k in ("counts", "q_hyp", "q_ref", "len_hyp", "len_ref")]
        _lib.check(self.lib.recnet_consensus_rows(self.handle, _ptr(hyp), int(Nh), int(Th), _ptr(ref), int(Nr), int(Tr), int(B),
                                                  _ptr(weights), float(sigma), _ptr(util), _ptr(sim), *ip, _stream()),
                   "recnet_consensus_rows")
        out = (util,) + ((sim,) if want_sim else ()) + ((ints,) if want_counts else ())
        return out[0] if len(out) == 1 else out

    # ------------------------------------------------------------------ ensemble decoding
    @staticmethod
    def _ens_args(n, weights, mode):
        """(weights as the host float array the ensemble entries read during the call, the mode's number); weights None: uniform.
        The library checks the values."""
        w = [1.0] * n if weights is None else [float(x) for x in weights]
        if len(w) != n:
            raise RuntimeError("%d weights for %d ensemble members" % (len(w), n))
        return (C.c_float * n)(*w), (_lib.ENS_MODES[mode] if isinstance(mode, str) else int(mode))

    def ensemble_mix_rows(self, logits, weights=None, mode="arithmetic", in_place=False):
        """The ensemble's logits of caller-supplied device rows (recnet_ensemble_mix_rows; no decoder needed): logits a list of M
        tensors [rows, V] float32, one per member.  Returns y [rows, V] float32: the log of the weighted mean of the members'
        probabilities (arithmetic) or the weighted mean of their log-probabilities (geometric); in_place: written over logits[0],
        which is returned.  The library checks M, the weights and the mode."""
        logits = list(logits)
        if not logits or logits[0].dim() != 2:
            raise RuntimeError("logits: expected a list of [rows, V] tensors")
        rows, V = logits[0].shape
        for x in logits:
            _chk_tensor(x, (rows, V), torch.float32, "logits")
        w, md = self._ens_args(len(logits), weights, mode)
        y = logits[0] if in_place else torch.empty_like(logits[0])
        ptrs = (C.c_void_p * len(logits))(*[x.data_ptr() for x in logits])
        _lib.check(self.lib.recnet_ensemble_mix_rows(self.handle, ptrs, len(logits), w, md, int(rows), int(V), _ptr(y), _stream()),
                   "recnet_ensemble_mix_rows")
        return y

    @staticmethod
    def beam_search_nbest_ensemble(engines, enc, beam_width, length_alpha=0.0, weights=None, mode="arithmetic", n_groups=1,
                                   diversity_penalty=0.0, no_repeat_ngram=0, min_length=0, banned_tokens=()):
        """beam_search_nbest_diverse over the engines of an ensemble (recnet_beam_search_nbest_ensemble; member 0 first): every
        step mixes the members' rows into the ensemble's logits, every member keeps its own state.  Returns that call's tensors
        (tokens, cum, len, score, group, n_steps).  The library checks the members, the weights, the mode and the search's own
        arguments before any launch of its own."""
        engines = list(engines)
        e0 = engines[0]
        toks, cum, ln, score, group, n = e0._nbest_outputs(enc, beam_width, with_group=True)
        w, md = Engine._ens_args(len(engines), weights, mode)
        hs = (C.c_void_p * len(engines))(*[e.handle.value for e in engines])
        ban, n_ban = Engine._ban_array(banned_tokens)
        _lib.check(e0.lib.recnet_beam_search_nbest_ensemble(hs, len(engines), w, md, _ptr(enc), int(beam_width), float(length_alpha),
                                                            int(n_groups), float(diversity_penalty), int(no_repeat_ngram), int(min_length),
                                                            ban, n_ban, _ptr(toks), _ptr(cum), _ptr(ln), _ptr(score), _ptr(group), _ptr(n),
                                                            _stream()), "recnet_beam_search_nbest_ensemble")
        return toks, cum, ln, score, group, n

    @staticmethod
    def score_captions_ensemble(engines, enc, tokens, weights=None, mode="arithmetic"):
        """score_captions at temperature 1 under the ensemble (recnet_score_captions_ensemble): the teacher-forced forward of every
        member, one mix of the T * B rows.  Returns (logprobs [T, B], caption_logprob [B], lengths [B]) like score_captions."""
        engines = list(engines)
        e0, d = engines[0], engines[0].dims
        if enc is not None:
            _chk_tensor(enc, (d["B"], d["F"], d["D"]), torch.float32, "encoder_outputs")
        if tokens.dim() != 2:
            raise RuntimeError("tokens: expected [T, B], got %s" % (tuple(tokens.shape),))
        T = tokens.shape[0]
        _chk_tensor(tokens, (T, d["B"]), torch.int64, "tokens")
        lps = torch.zeros(T, d["B"], dtype=torch.float32, device=e0.device)
        cap = torch.zeros(d["B"], dtype=torch.float32, device=e0.device)
        ln = torch.zeros(d["B"], dtype=torch.int32, device=e0.device)
        w, md = Engine._ens_args(len(engines), weights, mode)
        hs = (C.c_void_p * len(engines))(*[e.handle.value for e in engines])
        _lib.check(e0.lib.recnet_score_captions_ensemble(hs, len(engines), w, md, _ptr(enc), _ptr(tokens), int(T), _ptr(lps), _ptr(cap),
                                                         _ptr(ln), _stream()), "recnet_score_captions_ensemble")
        return lps, cap, ln

    # ------------------------------------------------------------------ stochastic beam search
    def sbs_select_rows(self, logits, cum, gum, finished, beam_width, temperature=1.0, seed=0, t=0):
        """One selection step of the stochastic beam search on caller-supplied device arrays (recnet_sbs_select_rows; no decoder
        needed): logits [nb, rows, V] float32 (only read), cum / gum [nb, rows] float32 (the log-probability phi and the perturbed
        score G of each hypothesis), finished [nb, rows] int32.  Returns (vals [rows, bw] float32 = phi, gum [rows, bw] float32 = G,
        idx [rows, bw] int32 = i * V + v) of the bw largest conditioned perturbed scores, descending, the lowest idx first among
        equals.  The library checks the width, the temperature and t."""
        nb, rows, V, _, vals, idx = self._select_rows_args(logits, cum, finished, beam_width, None)
        _chk_tensor(gum, (nb, rows), torch.float32, "gum")
        gout = torch.empty_like(vals)
        _lib.check(self.lib.recnet_sbs_select_rows(self.handle, _ptr(logits), _ptr(cum), _ptr(gum), _ptr(finished), nb, rows, V,
                                                   int(beam_width), float(temperature), seed & 0xFFFFFFFF, int(t), _ptr(vals), _ptr(gout),
                                                   _ptr(idx), _stream()), "recnet_sbs_select_rows")
        return vals, gout, idx

    def stochastic_beam_search(self, enc, beam_width, temperature=1.0, seed=0):
        """Stochastic beam search (recnet_stochastic_beam_search): beam_width captions per video drawn without replacement from the
        model's sequence distribution at `temperature`.  Returns device tensors (tokens [bw, Tm, B] int64 rank-major and canonical,
        cum [bw, B] float32: the log-probability, len [bw, B] int32, gum [bw, B] float32: the perturbed score the ranks descend in,
        n_steps int32[1]).  The library checks the width and the temperature before any launch of its own."""
        return Engine.stochastic_beam_search_ensemble([self], enc, beam_width, temperature, seed)

    @staticmethod
    def stochastic_beam_search_ensemble(engines, enc, beam_width, temperature=1.0, seed=0, weights=None, mode="arithmetic"):
        """stochastic_beam_search over the engines of an ensemble (recnet_stochastic_beam_search_ensemble; member 0 first); a list of
        one engine without weights calls the single-model entry.  Returns that call's tensors."""
        engines = list(engines)
        e0 = engines[0]
        toks, cum, ln, gum, _, n = e0._nbest_outputs(enc, beam_width)
        if len(engines) == 1 and weights is None:
            _lib.check(e0.lib.recnet_stochastic_beam_search(e0.handle, _ptr(enc), int(beam_width), float(temperature), seed & 0xFFFFFFFF,
                                                            _ptr(toks), _ptr(cum), _ptr(ln), _ptr(gum), _ptr(n), _stream()),
                       "recnet_stochastic_beam_search")
            return toks, cum, ln, gum, n
        w, md = Engine._ens_args(len(engines), weights, mode)
        hs = (C.c_void_p * len(engines))(*[e.handle.value for e in engines])
        _lib.check(e0.lib.recnet_stochastic_beam_search_ensemble(hs, len(engines), w, md, _ptr(enc), int(beam_width), float(temperature),
                                                                 seed & 0xFFFFFFFF, _ptr(toks), _ptr(cum), _ptr(ln), _ptr(gum), _ptr(n),
                                                                 _stream()), "recnet_stochastic_beam_search_ensemble")
        return toks, cum, ln, gum, n

    def score_captions(self, enc, tokens, temperature=1.0):
        """Teacher-forced log-probabilities of given captions, eval mode (recnet_score_captions).  tokens [T, B] int64 with every
        entry in [0, V) (the caller's duty: search.score_captions checks); enc None reuses the invariants of the previous call.
        Returns (logprobs [T, B] float32, caption_logprob [B] float32, lengths [B] int32) device tensors.  The library checks T
        and temperature."""
        d = self.dims
        if enc is not None:
            _chk_tensor(enc, (d["B"], d["F"], d["D"]), torch.float32, "encoder_outputs")
        if tokens.dim() != 2:
            raise RuntimeError("tokens: expected [T, B], got %s" % (tuple(tokens.shape),))
        T = tokens.shape[0]
        _chk_tensor(tokens, (T, d["B"]), torch.int64, "tokens")
        lps = torch.zeros(T, d["B"], dtype=torch.float32, device=self.device)
        cap = torch.zeros(d["B"], dtype=torch.float32, device=self.device)
        ln = torch.zeros(d["B"], dtype=torch.int32, device=self.device)
        _lib.check(self.lib.recnet_score_captions(self.handle, _ptr(enc), _ptr(tokens), int(T), float(temperature), _ptr(lps),
                                                  _ptr(cap), _ptr(ln), _stream()), "recnet_score_captions")
        return lps, cap, ln

    def reconstruction_error(self, enc, tokens=None, hiddens=None, want_recon=False):
        """Per-caption reconstruction error in eval mode (recnet_reconstruction_error): how well the reconstructor recovers
        enc [B, F, D] from the decoder states of the given captions.  Exactly one of tokens [T, B] int64 (every entry in [0, V):
        the caller's duty, search.reconstruction_errors checks; the teacher-forced decoder forward of score_captions runs first)
        and hiddens [T, 1, B, H] (states handed in).  Returns (err [B] float32, recon) device tensors; recon is None unless
        want_recon, else the reconstruction itself, global [B, R] = mean_t out_t, local [B, F, D].  mean(err) is the rec_mse of
        forward_reconstructor(train=False) at the same states.  The library checks T and the bound models."""
        d = self.dims
        B = d["B"]
        _chk_tensor(enc, (B, d["F"], d["D"]), torch.float32, "encoder_outputs")
        if (tokens is None) == (hiddens is None):
            raise RuntimeError("exactly one of tokens / hiddens must be given")
        if tokens is not None:
            if tokens.dim() != 2:
                raise RuntimeError("tokens: expected [T, B], got %s" % (tuple(tokens.shape),))
            T = tokens.shape[0]
            _chk_tensor(tokens, (T, B), torch.int64, "tokens")
        else:
            if hiddens.dim() != 4:
                raise RuntimeError("decoder_hiddens: expected [T, 1, B, H], got %s" % (tuple(hiddens.shape),))
            T = hiddens.shape[0]
            _chk_tensor(hiddens, (T, 1, B, d["H"]), torch.float32, "decoder_hiddens")
        err = torch.zeros(B, dtype=torch.float32, device=self.device)
        recon = None
        if want_recon:
            shape = (B, d["F"], d["D"]) if self.kind == "local" else (B, d.get("R", d["D"]))
            recon = torch.zeros(shape, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.recnet_reconstruction_error(self.handle, _ptr(enc), _ptr(tokens), _ptr(hiddens), int(T), _ptr(err),
                                                        _ptr(recon), _stream()), "recnet_reconstruction_error")
        return err, recon

    def decoder_step(self, tokens, h_in, c_in, enc, train=False, seed=0, t=0):
        d = self.dims
        B = d["B"]
        _chk_tensor(tokens, (B,), torch.int64, "tokens")
        for nm, st in (("h", h_in), ("c", c_in)):
            if st is not None:
                _chk_tensor(st, (B, d["H"]), torch.float32, "hidden state " + nm)
        if enc is not None:
            _chk_tensor(enc, (B, d["F"], d["D"]), torch.float32, "encoder_outputs")
        logits = torch.empty(B, d["V"], dtype=torch.float32, device=self.device)
        h_out = torch.empty(B, d["H"], dtype=torch.float32, device=self.device)
        c_out = torch.empty_like(h_out)
        _lib.check(self.lib.recnet_decoder_step(self.handle, _ptr(tokens), _ptr(h_in), _ptr(c_in), _ptr(enc),
                                                _ptr(logits), _ptr(h_out), _ptr(c_out), int(train), seed & 0xFFFFFFFF,
                                                int(t), _stream()), "recnet_decoder_step")
        return logits, h_out, c_out

    def reconstructor_step(self, inp, hr_in, cr_in, decoder_hiddens, T, train=False, seed=0, t=0):
        """One step of GlobalReconstructor.forward / LocalReconstructor.forward (global_reconstructor.py:30-46,
        local_reconstructor.py:37-55).  inp [B,H] (global only), hr_in / cr_in [B,R] or None (zero state),
        decoder_hiddens [T,1,B,H] or None (reuse the previous call's loop invariants) -> (out [B,R], hr', cr')."""
        d = self.dims
        B, R = d["B"], d.get("R", d["D"])
        for nm, x in (("hr", hr_in), ("cr", cr_in)):
            if x is not None:
                _chk_tensor(x, (B, R), torch.float32, "reconstructor state " + nm)
        if inp is not None:
            _chk_tensor(inp, (B, d["H"]), torch.float32, "input")
        if decoder_hiddens is not None:
            _chk_tensor(decoder_hiddens, (T, 1, B, d["H"]), torch.float32, "decoder_hiddens")
        out = torch.empty(B, R, dtype=torch.float32, device=self.device)
        hr = torch.empty_like(out)
        cr = torch.empty_like(out)
        _lib.check(self.lib.recnet_reconstructor_step(self.handle, _ptr(inp), _ptr(hr_in), _ptr(cr_in),
                                                      _ptr(decoder_hiddens), int(T), _ptr(out), _ptr(hr), _ptr(cr),
                                                      int(train), seed & 0xFFFFFFFF, int(t), _stream()),
                   "recnet_reconstructor_step")
        return out, hr, cr

    def poison_lds(self):
        """Test hook: NaN patterns into the LDS of every CU (uninitialised-LDS reads then show up in the parity tests)."""
        _lib.check(self.lib.recnet_debug_poison_lds(self.handle, _stream()), "recnet_debug_poison_lds")

    def chain_status(self):
        """Bit mask of persistent chain kernels that gave up a bounded wait (0 = healthy).  Synchronises the stream."""
        s = C.c_int32(0)
        _lib.check(self.lib.recnet_chain_status(self.handle, C.byref(s), _stream()), "recnet_chain_status")
        return s.value

    def debug_raise_give_up(self, chain_bit=1):
        """Test hook: raise chain `chain_bit`'s sticky word and the poison word the way a chain kernel that gives up does."""
        _lib.check(self.lib.recnet_debug_raise_give_up(self.handle, int(chain_bit), _stream()), "recnet_debug_raise_give_up")

    def set_deferred_reconstructor_update(self, on):
        """Opt in to / out of the deferred reconstructor update of the fused step (include/recnet_hip.h); completes a
        pending update first."""
        mode = 2 if on in (2, "recurrent") else int(bool(on))      # 2: only the recurrent weights' update is deferred
        _lib.check(self.lib.recnet_set_deferred_reconstructor_update(self.handle, mode, _stream()), "recnet_set_deferred_reconstructor_update")

    def set_dp_overlap(self, on):
        _lib.check(self.lib.recnet_set_dp_overlap(self.handle, int(bool(on))), "recnet_set_dp_overlap")

    def step_ring(self):
        """[(start, end)] of the last (up to seven) replayed steps in microseconds, oldest first (recnet_read_step_ring)."""
        buf = (C.c_uint64 * 16)()
        _lib.check(self.lib.recnet_read_step_ring(self.handle, buf, _stream()), "recnet_read_step_ring")
        ns, ne = int(buf[0]), int(buf[8])
        k = min(ns, ne, 7)
        out = []
        for i in range(k):
            a, b = ns - k + i, ne - k + i
            out.append((buf[1 + a % 7] * 0.01, buf[9 + b % 7] * 0.01))
        return out

    def abort_step(self):
        """After an abandoned stream capture: the handle's enqueue-time bookkeeping back to "between two steps" (recnet_abort_step)."""
        _lib.check(self.lib.recnet_abort_step(self.handle), "recnet_abort_step")

    def join_side(self):
        """The current stream waits for the library's side stream (recnet_join_side)."""
        _lib.check(self.lib.recnet_join_side(self.handle, _stream()), "recnet_join_side")

    def mark_pending(self):
        _lib.check(self.lib.recnet_mark_pending(self.handle), "recnet_mark_pending")

    def flush(self):
        """Completes a pending deferred reconstructor update on the current stream (stream-ordered; no host sync)."""
        _lib.check(self.lib.recnet_flush(self.handle, _stream()), "recnet_flush")

    def debug_tensor(self, which, n):
        """Test hook: n floats of a saved tensor of the local reconstructor's forward pass (recnet_debug_offset)."""
        off = self.lib.recnet_debug_offset(self.handle, int(which))
        assert off >= 0
        base = (self._ws_ptr - self.workspace.data_ptr()) + off
        return self.workspace[base:base + 4 * n].view(torch.float32).clone()

    def poison_dlogits_padding(self, T):
        """Test hook: NaN into the padding columns [V, ldV) of the first T * B rows of the dlogits operand (recnet_debug_offset 4) —
        the cross-entropy kernel of a T-step forward owns them, and the output layer's backward products read whole ldV-wide
        rows.  Returns the number of padding columns per row (0: V is a multiple of 8, nothing to poison)."""
        V, B, Tm = self.dims["V"], self.dims["B"], self.hyper["caption_max_len"] + 1
        ldV = (V + 7) // 8 * 8
        if ldV == V:
            return 0
        off = self.lib.recnet_debug_offset(self.handle, 4)
        assert off >= 0
        esz = 2 if self.precision == "bf16" else 4
        base = (self._ws_ptr - self.workspace.data_ptr()) + off
        rows = self.workspace[base:base + Tm * B * ldV * esz].view(torch.int16 if esz == 2 else torch.int32).view(Tm * B, ldV)
        assert 1 <= T <= Tm
        rows[:T * B, V:] = -1     # all bits set: a NaN in either format
        return ldV - V

    def images_stale(self):
        """Test hook: number of 16-bit words in which the packed operand images differ from a fresh re-pack of the master
        parameters (recnet_debug_images_stale); completes a pending update and synchronises."""
        nb = int(self.lib.recnet_debug_images_bytes(self.handle))
        assert nb > 0
        scratch = torch.empty(nb + 256, dtype=torch.uint8, device=self.device)      # (the caller's allocator, like every other buffer)
        base = (scratch.data_ptr() + 255) // 256 * 256
        n = C.c_int64(-1)
        _lib.check(self.lib.recnet_debug_images_stale(self.handle, C.c_void_p(base), nb, C.byref(n), _stream()), "recnet_debug_images_stale")
        return int(n.value)

    def debug_occupy(self, n_workgroups, microseconds, stream=None):
        """Test hook: n_workgroups CU-filling workgroups spinning for `microseconds` on `stream` (a torch stream; default: the current one)."""
        st = C.c_void_p(stream.cuda_stream) if stream is not None else _stream()
        _lib.check(self.lib.recnet_debug_occupy(self.handle, int(n_workgroups), int(microseconds), st), "recnet_debug_occupy")

    def chain_reset(self, disable_persistent=True):
        _lib.check(self.lib.recnet_chain_reset(self.handle, int(bool(disable_persistent)), _stream()), "recnet_chain_reset")

    def forward_decoder(self, enc, targets, T, step_weight, train=True, seed=0, want_hiddens=True):
        d = self.dims
        B = d["B"]
        _chk_tensor(enc, (B, d["F"], d["D"]), torch.float32, "encoder_outputs")
        _chk_tensor(targets, (self.hyper["caption_max_len"] + 1, B), torch.int64, "targets")
        _chk_tensor(step_weight, (T,), torch.float32, "step_weight")
        hid = torch.empty(T, 1, B, d["H"], dtype=torch.float32, device=self.device) if want_hiddens else None
        _lib.check(self.lib.recnet_forward_decoder(self.handle, _ptr(enc), _ptr(targets), int(T), _ptr(step_weight),
                                                   int(train), seed & 0xFFFFFFFF, _ptr(hid), _ptr(self.scalars),
                                                   _stream()), "recnet_forward_decoder")
        self.T = T
        return hid

    def forward_decoder_free(self, enc, targets, T, step_weight, train=False, seed=0):
        """Free-running pass (train.py:46-51): returns (hiddens [T,1,B,H], output_indices [T,B] int64).  Forward only."""
        d = self.dims
        B = d["B"]
        _chk_tensor(enc, (B, d["F"], d["D"]), torch.float32, "encoder_outputs")
        _chk_tensor(targets, (self.hyper["caption_max_len"] + 1, B), torch.int64, "targets")
        _chk_tensor(step_weight, (T,), torch.float32, "step_weight")
        hid = torch.empty(T, 1, B, d["H"], dtype=torch.float32, device=self.device)
        out = torch.empty(T, B, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.recnet_forward_decoder_free(self.handle, _ptr(enc), _ptr(targets), int(T), _ptr(step_weight),
                                                        int(train), seed & 0xFFFFFFFF, _ptr(hid), _ptr(out),
                                                        _ptr(self.scalars), _stream()), "recnet_forward_decoder_free")
        self.T = T
        return hid, out

    def forward_reconstructor(self, enc, hiddens, T, train=True, seed=0):
        d = self.dims
        _chk_tensor(enc, (d["B"], d["F"], d["D"]), torch.float32, "encoder_outputs")
        if hiddens is not None:
            _chk_tensor(hiddens, (T, 1, d["B"], d["H"]), torch.float32, "decoder_hiddens")
        _lib.check(self.lib.recnet_forward_reconstructor(self.handle, _ptr(enc), _ptr(hiddens), int(T), int(train),
                                                         seed & 0xFFFFFFFF, _ptr(self.scalars), _stream()),
                   "recnet_forward_reconstructor")
        self.T = T

    def backward_reconstructor(self, enc, grad_scale=1.0, want_dhiddens=True):
        d = self.dims
        _chk_tensor(enc, (d["B"], d["F"], d["D"]), torch.float32, "encoder_outputs")
        dh = torch.empty(self.T, 1, d["B"], d["H"], dtype=torch.float32, device=self.device) if want_dhiddens else None
        _lib.check(self.lib.recnet_backward_reconstructor(self.handle, _ptr(enc), float(grad_scale), _ptr(dh),
                                                          _stream()), "recnet_backward_reconstructor")
        return dh

    def backward_decoder(self, enc, targets, dhiddens=None, grad_scale=1.0):
        d = self.dims
        _chk_tensor(enc, (d["B"], d["F"], d["D"]), torch.float32, "encoder_outputs")
        _chk_tensor(targets, (self.hyper["caption_max_len"] + 1, d["B"]), torch.int64, "targets")
        if dhiddens is not None:
            _chk_tensor(dhiddens, (self.T, 1, d["B"], d["H"]), torch.float32, "dhiddens")
        _lib.check(self.lib.recnet_backward_decoder(self.handle, _ptr(enc), _ptr(targets), _ptr(dhiddens),
                                                    float(grad_scale), _stream()), "recnet_backward_decoder")

    def add_reg_grad(self, which, grad_scale=1.0):
        _lib.check(self.lib.recnet_add_reg_grad(self.handle, int(which), float(grad_scale), _stream()),
                   "recnet_add_reg_grad")

    def clip_grad_norm(self, which, max_norm):
        out = torch.empty(1, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.recnet_clip_grad_norm(self.handle, int(which), float(max_norm), _ptr(out), _stream()),
                   "recnet_clip_grad_norm")
        return out

    def optimizer_step(self, step, flags):
        _lib.check(self.lib.recnet_optimizer_step(self.handle, int(step), int(flags), _ptr(self.scalars), _stream()),
                   "recnet_optimizer_step")

    def _chk_step(self, enc, targets, T, step_weight):
        """The raw pointers go straight to the device: shapes, dtypes and residency are checked here."""
        d = self.dims
        _chk_tensor(enc, (d["B"], d["F"], d["D"]), torch.float32, "encoder_outputs")
        _chk_tensor(targets, (self.hyper["caption_max_len"] + 1, d["B"]), torch.int64, "targets")
        _chk_tensor(step_weight, (int(T),), torch.float32, "step_weight")

    def _chk_rec(self, enc, hiddens, T):
        from ._lib import RecNetError  # noqa: F401
        d = self.dims
        _chk_tensor(enc, (d["B"], d["F"], d["D"]), torch.float32, "encoder_outputs")
        if hiddens is not None:
            _chk_tensor(hiddens, (int(T), 1, d["B"], d["H"]), torch.float32, "decoder_hiddens")

    def train_step_fwd_bwd(self, enc, targets, T, step_weight, seed):
        self._chk_step(enc, targets, T, step_weight)
        _lib.check(self.lib.recnet_train_step_fwd_bwd(self.handle, _ptr(enc), _ptr(targets), int(T),
                                                      _ptr(step_weight), seed & 0xFFFFFFFF, _ptr(self.scalars),
                                                      _stream()), "recnet_train_step_fwd_bwd")
        self.T = T

    def train_step(self, enc, targets, T, step_weight, seed, step):
        self._chk_step(enc, targets, T, step_weight)
        _lib.check(self.lib.recnet_train_step(self.handle, _ptr(enc), _ptr(targets), int(T), _ptr(step_weight),
                                              seed & 0xFFFFFFFF, int(step), _ptr(self.scalars), _stream()),
                   "recnet_train_step")
        self.T = T

    # ---- hipGraph-replay-friendly forms (step counter and dropout seed live on the device)
    def set_step(self, step):
        _lib.check(self.lib.recnet_set_step(self.handle, int(step), _stream()), "recnet_set_step")

    def train_step_fwd_bwd_dev(self, enc, targets, T, step_weight, seed_base):
        self._chk_step(enc, targets, T, step_weight)
        _lib.check(self.lib.recnet_train_step_fwd_bwd_dev(self.handle, _ptr(enc), _ptr(targets), int(T),
                                                          _ptr(step_weight), seed_base & 0xFFFFFFFF,
                                                          _ptr(self.scalars), _stream()),
                   "recnet_train_step_fwd_bwd_dev")
        self.T = T

    def train_step_dev(self, enc, targets, T, step_weight, seed_base, flags):
        """Fused forward + backward + optimiser, step count / seed on the device (graph replay, single rank)."""
        self._chk_step(enc, targets, T, step_weight)
        _lib.check(self.lib.recnet_train_step_dev(self.handle, _ptr(enc), _ptr(targets), int(T), _ptr(step_weight),
                                                  seed_base & 0xFFFFFFFF, int(flags), _ptr(self.scalars), _stream()),
                   "recnet_train_step_dev")
        self.T = T

    def train_step_part_dev(self, part, enc, targets, T, step_weight, seed_base):
        self._chk_step(enc, targets, T, step_weight)
        _lib.check(self.lib.recnet_train_step_part_dev(self.handle, int(part), _ptr(enc), _ptr(targets), int(T),
                                                       _ptr(step_weight), seed_base & 0xFFFFFFFF, _ptr(self.scalars),
                                                       _stream()), "recnet_train_step_part_dev")
        self.T = T

    def optimizer_step_dev(self, flags):
        _lib.check(self.lib.recnet_optimizer_step_dev(self.handle, int(flags), _ptr(self.scalars), _stream()),
                   "recnet_optimizer_step_dev")

    # ---- live measurement of one recurrent-step GEMM site with HIP events on its own stream
    def profile_site(self, site, fn, iters=3):
        """Runs fn() `iters` times with hipEvents around every launch of `site` (1 dec fwd, 2 dec bwd, 3 rec
        fwd, 4 rec bwd, 5 local-attention, 7-10 the chain kernels, 11 the reconstruction-error kernel); returns (launches, average ms per launch).  fn() launches
        EAGERLY: on a capturing stream no bracket is taken (csrc/host_common.inc: prof_take)."""
        _lib.check(self.lib.recnet_profile_begin(self.handle, int(site)), "recnet_profile_begin")
        for _ in range(iters):
            fn()
        n, ms = C.c_int32(0), C.c_double(0.0)
        _lib.check(self.lib.recnet_profile_end(self.handle, C.byref(n), C.byref(ms)), "recnet_profile_end")
        return n.value, (ms.value / n.value if n.value else 0.0)

    def profile_null_launch(self, count=1):
        _lib.check(self.lib.recnet_profile_null_launch(self.handle, int(count), _stream()), "recnet_profile_null_launch")

    def read_stamps(self):
        """Phase stamps of the last train step (recnet_read_stamps): dict of microsecond offsets from the step's start —
        `chains[name] = (begin, end)` for the chain kernels that ran inside it, `end` = the step's last kernel.  Written by the
        step's own kernels, so it describes a REPLAYED graph with no tracer attached.  Synchronises."""
        buf = (C.c_uint64 * 30)()
        _lib.check(self.lib.recnet_read_stamps(self.handle, buf, 30, _stream()), "recnet_read_stamps")
        t0, t1 = buf[0], buf[13]
        names = ("decoder_forward", "decoder_bptt", "global_forward", "global_backward", "local_forward", "local_backward")
        chains = {}
        for k, nm in enumerate(names):
            b, e = buf[1 + 2 * k], buf[2 + 2 * k]
            if t0 <= b <= e <= t1:                       # ran inside this step
                chains[nm] = ((b - t0) / 100.0, (e - t0) / 100.0)
        groups = {}
        for j, nm in enumerate(("prologue_products", "reconstructor_weight_gradients", "pending_recurrent_update", "decoder_weight_gradients")):
            b, e = buf[14 + 2 * j], buf[15 + 2 * j]
            if t0 <= b <= e <= t1:
                groups[nm] = ((b - t0) / 100.0, (e - t0) / 100.0)
        return {"end": (t1 - t0) / 100.0 if t1 >= t0 else None, "chains": chains, "groups": groups}

    def recurrent_step_bytes(self, which):
        return float(self.lib.recnet_recurrent_step_bytes(self.handle, int(which)))

    def chain_exchange_bytes(self, which):
        return float(self.lib.recnet_chain_exchange_bytes(self.handle, int(which)))

    def scalar_dict(self):
        """Host copy of the device scalars (synchronises)."""
        v = self.scalars.tolist()
        return dict(zip(_lib.SCALAR_NAMES, v))

    def gemm_bf16(self, A, B, a_col=False, b_col=False, bias=None, alpha=1.0, C_out=None, accumulate=False, splitk=1,
                  M=None, N=None, K=None, tag=0):
        """Test hook for the DMA-staged bf16 kernel: A, B are torch.bfloat16."""
        if M is None:
            M = A.shape[1] if a_col else A.shape[0]
            K = A.shape[0] if a_col else A.shape[1]
            N = B.shape[1] if b_col else B.shape[0]
        if C_out is None:
            C_out = torch.zeros(M, N, dtype=torch.float32, device=A.device)
        ws = torch.empty(max(1, splitk) * M * N, dtype=torch.float32, device=A.device) if splitk > 1 else None
        _lib.check(self.lib.recnet_gemm_bf16(_ptr(A), int(a_col), A.stride(0), _ptr(B), int(b_col), B.stride(0),
                                             _ptr(C_out), C_out.stride(0), _ptr(bias), M, N, K, float(alpha),
                                             int(accumulate), int(splitk), _ptr(ws), int(tag), _stream()),
                   "recnet_gemm_bf16")
        return C_out

    def gemm_group_bf16(self, As, Bs, a_col=False, b_col=False, biases=None, alphas=None, C_outs=None, accumulate=None, split=True):
        """Test hook for the grouped launch (recnet_gemm_group_bf16): lists of torch.bfloat16 operands of one layout; returns the
        fp32 results.  split=False: no slab workspace, i.e. no product is split along K."""
        n = len(As)
        Ms = [A.shape[1] if a_col else A.shape[0] for A in As]
        Ks = [A.shape[0] if a_col else A.shape[1] for A in As]
        Ns = [B.shape[1] if b_col else B.shape[0] for B in Bs]
        dev = As[0].device
        if C_outs is None:
            C_outs = [torch.zeros(m, nn_, dtype=torch.float32, device=dev) for m, nn_ in zip(Ms, Ns)]
        ws = torch.empty(16 * max(m * nn_ for m, nn_ in zip(Ms, Ns)) * n, dtype=torch.float32, device=dev) if split else None
        if not hasattr(self, "_gg_cnt"):
            self._gg_cnt = torch.zeros(1 << 16, dtype=torch.int32, device=dev)
        vp = lambda ts: (C.c_void_p * n)(*[C.c_void_p(t.data_ptr()) if t is not None else None for t in ts])
        ia = lambda xs: (C.c_int32 * n)(*[int(x) for x in xs])
        bl = biases if biases is not None else [None] * n
        _lib.check(self.lib.recnet_gemm_group_bf16(int(a_col), int(b_col), n, vp(As), ia([A.stride(0) for A in As]), vp(Bs),
                                                   ia([B.stride(0) for B in Bs]), vp(C_outs), ia([c.stride(0) for c in C_outs]), vp(bl),
                                                   ia(Ms), ia(Ns), ia(Ks), (C.c_float * n)(*[float(x) for x in (alphas or [1.0] * n)]),
                                                   ia(accumulate or [0] * n), _ptr(ws), ws.numel() if ws is not None else 0,
                                                   _ptr(self._gg_cnt) if split else None, (1 << 16) if split else 0, _stream()),
                   "recnet_gemm_group_bf16")
        return C_outs

    def gemm(self, A, B, a_col=False, b_col=False, bias=None, alpha=1.0, C_out=None, accumulate=False, splitk=1,
             M=None, N=None, K=None):
        """Test hook: C[M,N] (+)= alpha * op(A) op(B)^T + bias through the MFMA GEMM."""
        if M is None:
            M = A.shape[1] if a_col else A.shape[0]
            K = A.shape[0] if a_col else A.shape[1]
            N = B.shape[1] if b_col else B.shape[0]
        if C_out is None:
            C_out = torch.zeros(M, N, dtype=torch.float32, device=A.device)
        ws = torch.empty(max(1, splitk) * M * N, dtype=torch.float32, device=A.device) if splitk > 1 else None
        _lib.check(self.lib.recnet_gemm(_PREC[self.precision], _ptr(A), int(a_col), A.stride(0), _ptr(B), int(b_col),
                                        B.stride(0), _ptr(C_out), C_out.stride(0), _ptr(bias), M, N, K, float(alpha),
                                        int(accumulate), int(splitk), _ptr(ws), _stream()), "recnet_gemm")
        return C_out
