"""MI355X-native RecNet train-step path (gfx950 HIP kernels behind the reference's Python API).

Host-side mirror of the reference interface for the hot path:
  models/decoder.py  Decoder                 -> modules.Decoder
  models/global_reconstructor.py             -> modules.GlobalReconstructor
  models/local_reconstructor.py              -> modules.LocalReconstructor
  train.py forward_decoder / forward_*_reconstructor / build_decoder / build_reconstructor
                                             -> api.*
  train.py:248-273 (the step body)           -> api.TrainStep (single stream, hipGraph-capturable)
  eval.py greedy_search / beam_search        -> search.* (device-side loops)
  (no counterpart) temperature / top-k draws -> search.sample_search, search.sequence_logprob
  (no counterpart) scoring given captions    -> search.score_captions, search.best_of_n, loop.perplexity
  (no counterpart) reconstruction error      -> search.reconstruction_errors, search.canonical_captions
  (no counterpart) N-best beam search        -> search.beam_search_nbest, search.best_of_beam
  (no counterpart) diverse (group) beams     -> the same two with n_groups / diversity_penalty, search.nbest_diversity
  (no counterpart) consensus (MBR) reranking -> search.consensus_scores, best_of_n / best_of_beam with consensus_weight
  (no counterpart) ensemble decoding         -> search.Ensemble in place of the decoder, search.ensemble_logits
  (no counterpart) stochastic beam search    -> search.stochastic_beam_search, search.sbs_weights, best_of_n(distinct=True)
  (no counterpart) lr schedules under replay -> api.LRSchedule, FusedAdam.set_lr_schedule / scale_lr, Trainer(plateau=...)
All compute goes through csrc/librecnet_hip.so (C ABI: include/recnet_hip.h).
"""
from .config import TrainConfig, make_config  # noqa: F401
from .modules import Decoder, GlobalReconstructor, LocalReconstructor  # noqa: F401
from .api import (build_decoder, build_reconstructor, forward_decoder, forward_global_reconstructor,  # noqa: F401
                  forward_local_reconstructor, clip_grad_norm_, TrainStep, GraphedStep, FusedAdam, decode_len,
                  step_weights, LRSchedule)
from .dp import DataParallelTrainStep, shard_bounds  # noqa: F401
from .search import (greedy_search, beam_search, sample_search, sequence_logprob, score_captions, best_of_n,  # noqa: F401
                     pick_best_of_n, canonical_captions, reconstruction_errors, beam_search_nbest, best_of_beam, nbest_diversity,
                     consensus_scores, Ensemble, ensemble_logits, stochastic_beam_search, sbs_weights)
from .loop import Trainer, evaluate, perplexity  # noqa: F401
from .checkpoint import save_checkpoint, load_checkpoint, read_checkpoint  # noqa: F401
