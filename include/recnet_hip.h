/* recnet_hip.h — C ABI of the MI355X (gfx950) RecNet train-step library (librecnet_hip.so).
 *
 * The reference (hobincar/reconstruction-network-for-video-captioning) has no FFI layer: its hot
 * path sits behind Python callables that dispatch to stock PyTorch kernels.  This header is the
 * boundary a maintainer would bind instead (ctypes stub: INTEGRATION.md).  Every entry point names
 * the reference interface it replaces.  All pointers are raw DEVICE pointers unless a parameter is
 * documented "host"; `stream` is a hipStream_t passed as void*; every function only enqueues work
 * on that stream (no allocation, no synchronisation => hipGraph-capturable) and returns 0 on
 * success or a negative RECNET_E* code (recnet_last_error() gives the message).
 *
 * Tensors are fp32, row-major, with the reference's shapes and state_dict names;
 * token ids are int64 like the reference's LongTensors.
 */
#ifndef RECNET_HIP_H
#define RECNET_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 12 still: recnet_beam_select_rows_constrained / recnet_beam_search_nbest_constrained, and after them
 * recnet_beam_select_rows_diverse / recnet_beam_search_nbest_diverse, and recnet_consensus_rows, and the three ensemble entries (recnet_ensemble_mix_rows, recnet_beam_search_nbest_ensemble, recnet_score_captions_ensemble), and the three stochastic beam search entries (recnet_sbs_select_rows, recnet_stochastic_beam_search, recnet_stochastic_beam_search_ensemble), and the four learning-rate schedule entries (recnet_set_lr_schedule, recnet_get_lr_schedule, recnet_lr_at, recnet_read_lr, with the struct recnet_lr_schedule), were added without changing any existing entry.  A library built before them is still caught: a binding that resolves every declared symbol fails on the first one missing. */
#define RECNET_ABI_VERSION 12
#define RECNET_ATTN_NONE 0
#define RECNET_ATTN_SOFTMAX 1
#define RECNET_OK 0
#define RECNET_EINVAL (-1)      /* bad dimension / null pointer / unsupported variant */
#define RECNET_ESTATE (-2)      /* call order violated (e.g. backward before forward) */
#define RECNET_EHIP (-3)        /* a HIP runtime call failed */

#define RECNET_REC_NONE 0
#define RECNET_REC_GLOBAL 1     /* models/global_reconstructor.py */
#define RECNET_REC_LOCAL 2      /* models/local_reconstructor.py  */
#define RECNET_CELL_LSTM 0      /* torch.nn.LSTM, gate rows (i, f, g, o) */
#define RECNET_CELL_GRU 1       /* torch.nn.GRU, gate rows (r, z, n); the hidden state is a single tensor (train.py:33-35) */
#define RECNET_PREC_F32 0       /* exact fp32 MFMA (v_mfma_f32_16x16x4_f32) */
#define RECNET_PREC_BF16 1      /* bf16 MFMA operands, fp32 accumulate / state / losses */

/* Shapes + hyper-parameters.  Field names follow config.py:27-93 (TrainConfig). */
typedef struct recnet_config {
  int32_t batch_size;                 /* B: captions on THIS rank                       config.py:51  */
  int32_t encoder_output_len;         /* F                                              config.py:63  */
  int32_t encoder_output_size;        /* D                                              config.py:62  */
  int32_t embedding_size;             /* E                                              config.py:57  */
  int32_t decoder_hidden_size;        /* H                                              config.py:67  */
  int32_t decoder_attn_size;          /* A                                              config.py:68  */
  int32_t n_vocabs;                   /* V                                              train.py:222  */
  int32_t reconstructor_hidden_size;  /* R (local reconstructor requires R == D)        config.py:78  */
  int32_t reconstructor_attn_size;    /* local reconstructor only                       config.py:82  */
  int32_t caption_max_len;            /* decoder runs <= caption_max_len + 1 steps      config.py:50  */
  int32_t reconstructor_type;         /* RECNET_REC_*                                   config.py:76  */
  int32_t precision;                  /* RECNET_PREC_*                                                */
  int32_t global_batch_size;          /* data parallel: B summed over ranks (== B single GPU)         */
  int32_t batch_offset;               /* data parallel: global index of this rank's first caption     */
  int32_t decoder_use_amsgrad, reconstructor_use_amsgrad;       /* config.py:90-91 */
  int32_t decoder_cell;               /* RECNET_CELL_*: decoder_model                    config.py:31  */
  int32_t reconstructor_cell;         /* RECNET_CELL_*: reconstructor_model              config.py:77  */
  int32_t decoder_attn_normalize;     /* RECNET_ATTN_NONE (the reference: decoder.py:30's softmax is constructed but never
                                         called, decoder.py:55-61) | RECNET_ATTN_SOFTMAX: softmax over the frames of the
                                         attention energies before the weighted mean (opt-in; north_star's wording) */
  float embedding_scale;              /*                                                config.py:59  */
  float embedding_dropout;            /*                                                config.py:58  */
  float decoder_out_dropout;          /* dropout applied to the logits, decoder.py:69   config.py:70  */
  float reconstructor_decoder_dropout;/*                                                config.py:79  */
  float gradient_clip;                /* <= 0 disables clipping                         config.py:92-93 */
  float decoder_lambda_reg;           /* train.py:151 (1e-3) */
  float reconstructor_lambda_reg;     /* train.py:188 (1e-2) */
  float lambda_recon;                 /* train.py:225 (1.0)  */
  /* optimiser hyper-parameters are doubles, like the Python floats torch.optim.Adam receives */
  double decoder_learning_rate, reconstructor_learning_rate;    /* config.py:86-87 */
  double decoder_weight_decay, reconstructor_weight_decay;      /* config.py:88-89 */
  double adam_beta1, adam_beta2, adam_eps;                      /* torch.optim.Adam defaults 0.9 / 0.999 / 1e-8 */
} recnet_config;

/* Decoder parameter set — state_dict keys of models/decoder.py:22-42 (LSTM, 1 layer). */
typedef struct recnet_decoder_tensors {
  float* attn_b;           /* [A]          */
  float* embedding_weight; /* [V, E]       */
  float* attn_W_weight;    /* [A, H]       */
  float* attn_U_weight;    /* [A, D]       */
  float* attn_w_weight;    /* [1, A]       */
  float* rnn_weight_ih_l0; /* [4H, E + D]  */
  float* rnn_weight_hh_l0; /* [4H, H]      */
  float* rnn_bias_ih_l0;   /* [4H]         */
  float* rnn_bias_hh_l0;   /* [4H]         */
  float* out_weight;       /* [V, H]       */
  float* out_bias;         /* [V]          */
} recnet_decoder_tensors;

/* Reconstructor parameter set — models/global_reconstructor.py:17-28 / local_reconstructor.py:17-35.
 * attn_* are NULL for the global reconstructor. */
typedef struct recnet_reconstructor_tensors {
  float* attn_b;           /* [RA]                              (local) */
  float* attn_W_weight;    /* [RA, R]                           (local) */
  float* attn_U_weight;    /* [RA, H]                           (local) */
  float* attn_w_weight;    /* [1, RA]                           (local) */
  float* rnn_weight_ih_l0; /* [4R, 2H] global | [4R, H] local           */
  float* rnn_weight_hh_l0; /* [4R, R]   */
  float* rnn_bias_ih_l0;   /* [4R]      */
  float* rnn_bias_hh_l0;   /* [4R]      */
  float* out_weight;       /* [R, R]    */
  float* out_bias;         /* [R]       */
} recnet_reconstructor_tensors;

/* Scalars produced on the device by the forward / optimiser calls (one float each). */
typedef struct recnet_scalars {
  float dec_ce;        /* sum_t mean_b CE / sum_t n_t            train.py:56-68  */
  float dec_reg;       /* sum_p ||p||_2 over decoder tensors     train.py:69     */
  float dec_loss;      /* dec_ce + lambda_reg * dec_reg          train.py:70     */
  float rec_mse;       /* MSE term (global: already / T)         train.py:101-102 / :128 */
  float rec_reg;       /*                                        train.py:103 / :129 */
  float rec_loss;      /*                                        train.py:104 / :130 */
  float total_loss;    /* dec_loss + lambda_recon * rec_loss     train.py:260    */
  float dec_grad_norm; /* total decoder grad norm before clipping, clip_grad_norm_ train.py:270 */
} recnet_scalars;

typedef struct recnet_handle recnet_handle;

int recnet_abi_version(void);
const char* recnet_last_error(void);

/* Host-only object describing one (config) problem; owns no device memory. */
int recnet_create(const recnet_config* cfg, recnet_handle** out);
void recnet_destroy(recnet_handle* h);
/* Update the data-parallel placement / learning rates without re-creating (host fields only). */
int recnet_set_shard(recnet_handle* h, int32_t global_batch_size, int32_t batch_offset);
/* Replace the Adam hyper-parameters of one model (which: 0 decoder, 1 reconstructor) — what an edit of torch.optim.Adam's
 * param_groups or a load_state_dict changes: lr, weight decay, betas, eps.  recnet_create takes them from the config
 * (adam_beta1 / adam_beta2 / adam_eps for both models); this call gives each model its own.  Host fields only: it takes effect
 * for launches enqueued afterwards, so a captured graph keeps the values it was captured with and has to be captured again.
 * Whether a model runs AMSGrad is fixed by the config and the state bound to it.  Ranges are torch.optim.Adam's
 * (lr, weight decay, eps >= 0; 0 <= beta < 1), else RECNET_EINVAL. */
int recnet_set_optimizer_hyper(recnet_handle* h, int32_t which, double lr, double weight_decay, double beta1, double beta2,
                               double eps);

/* Learning-rate schedules that a captured step follows.  The lr above is the BASE lr; every Adam launch
 * multiplies it, on the device and in double, by scale * warm(n) * decay(n) for the 1-based optimiser step n it belongs to (the
 * device's step counter, so a graph captured at any time follows a schedule installed later).  With W = warmup_steps,
 * m = max(0, n - W), M = total_steps - W:
 *   warm(n)  = n / W for n < W, else 1
 *   decay(n) = CONSTANT 1 | LINEAR 1 - (1 - min_factor) min(m, M) / M | COSINE min_factor + (1 - min_factor) (1 + cos(pi min(m, M) / M)) / 2
 *            | INVSQRT max(min_factor, sqrt(W' / max(n, W'))), W' = max(W, 1) | STEP max(min_factor, gamma ^ floor(m / period))
 * NONE, every handle's state at creation, is the factor 1 exactly; scale (host-driven, e.g. reduce-on-plateau) applies under every
 * kind.  Weight decay, betas and eps stay captured values. */
#define RECNET_LR_NONE 0
#define RECNET_LR_CONSTANT 1
#define RECNET_LR_LINEAR 2
#define RECNET_LR_COSINE 3
#define RECNET_LR_INVSQRT 4
#define RECNET_LR_STEP 5
typedef struct recnet_lr_schedule {
  int32_t kind, warmup_steps, total_steps, period;      /* RECNET_LR_*; total_steps: LINEAR / COSINE; period: STEP */
  double min_factor, gamma, scale;                      /* in [0, 1]; in (0, 1]; > 0 */
} recnet_lr_schedule;
/* Installs the schedule of one optimiser (which: 0 decoder, 1 reconstructor).  Checked on the host, RECNET_EINVAL for: which outside
 * {0, 1}; an unknown kind; negative warmup_steps / total_steps; total_steps <= warmup_steps (LINEAR, COSINE); period <= 0 (STEP);
 * min_factor outside [0, 1]; gamma outside (0, 1]; scale <= 0 or infinite; any NaN.  A pending deferred reconstructor update is
 * completed first, as by recnet_flush (it belongs to a step of the old schedule); then the descriptor is written stream-ordered by
 * a one-thread kernel: no copy from pageable memory, no host synchronisation.  Legal while captured graphs of the handle are alive —
 * their next replay steps with the new schedule; RECNET_ESTATE when `stream` itself is being captured.  Before a workspace is bound
 * only the host copy is set (recnet_bind_workspace uploads it). */
int recnet_set_lr_schedule(recnet_handle* h, int32_t which, const recnet_lr_schedule* sched, void* stream);
/* The host copy of what the last recnet_set_lr_schedule installed (kind NONE, scale 1 after recnet_create). */
int recnet_get_lr_schedule(const recnet_handle* h, int32_t which, recnet_lr_schedule* out);
/* lr(step) = base_lr * scale * warm * decay on the host: no handle, no GPU; the same inline function the kernels call.  The
 * descriptor is checked like recnet_set_lr_schedule's; step >= 1. */
int recnet_lr_at(const recnet_lr_schedule* sched, double base_lr, int64_t step, double* out);
/* out[0] / out[1]: the lr the decoder's / reconstructor's most recent Adam launch used, as that launch wrote it (0 before the
 * first).  Synchronises `stream`, like recnet_read_step_ring. */
int recnet_read_lr(recnet_handle* h, double* out2, void* stream);

/* Bytes of device scratch the caller must provide (activations saved for backward, split-K slabs,
 * packed weights).  Must stay alive and untouched between a forward and its backward. */
size_t recnet_workspace_bytes(const recnet_handle* h);
int recnet_bind_workspace(recnet_handle* h, void* workspace, size_t bytes);

/* Parameters, gradients and Adam state.  `grad` tensors are overwritten (not accumulated) by the
 * backward calls — the reference zero_grad()s before every backward (train.py:265-267).
 * exp_avg / exp_avg_sq / max_exp_avg_sq mirror torch.optim.Adam's per-parameter state; max_* may be
 * NULL structs' pointers when amsgrad is off. */
int recnet_bind_decoder(recnet_handle* h, const recnet_decoder_tensors* param, const recnet_decoder_tensors* grad,
                        const recnet_decoder_tensors* exp_avg, const recnet_decoder_tensors* exp_avg_sq,
                        const recnet_decoder_tensors* max_exp_avg_sq);
int recnet_bind_reconstructor(recnet_handle* h, const recnet_reconstructor_tensors* param,
                              const recnet_reconstructor_tensors* grad,
                              const recnet_reconstructor_tensors* exp_avg,
                              const recnet_reconstructor_tensors* exp_avg_sq,
                              const recnet_reconstructor_tensors* max_exp_avg_sq);

/* Re-derive the packed (concatenated / bf16) weight images after the fp32 parameters changed
 * (optimiser step, load_state_dict).  recnet_optimizer_step does this itself. */
int recnet_pack_weights(recnet_handle* h, void* stream);

/* ---- Decoder.forward, models/decoder.py:45-70: ONE decode step (the API eval.py's greedy / beam
 * search drive, eval.py:22,48).  tokens [B] int64; h_in/c_in/h_out/c_out [B,H]; enc [B,F,D];
 * logits [B,V].  `train` != 0 applies the embedding / logits dropout with (seed, t).  enc == NULL reuses the invariants
 * of the previous call / of recnet_decoder_prepare. */
int recnet_decoder_step(recnet_handle* h, const int64_t* tokens, const float* h_in, const float* c_in,
                        const float* enc, float* logits, float* h_out, float* c_out, int32_t train,
                        uint32_t seed, int32_t t, void* stream);

/* Compute the loop invariants of `enc` once (Uv = enc . U^T, P = enc . W_ih[:, E:]^T); later recnet_decoder_step calls
 * with enc == NULL reuse them (the search loops of eval.py call the step 31 x beam times on the same features). */
int recnet_decoder_prepare(recnet_handle* h, const float* enc, void* stream);

/* ---- greedy_search, eval.py:19-33, as one device-side loop (no per-sample Python, no host sync): start from <SOS> and
 * zero state (eval.py:131-141), argmax feedback.  tokens_out [caption_max_len+1][B] int64 (time-major);
 * n_steps_out (device int32) = number of steps the reference's loop produces (it stops after the first step whose
 * tokens are all <PAD>, eval.py:30): rows >= n_steps are to be ignored. */
int recnet_greedy_search(recnet_handle* h, const float* enc, int64_t* tokens_out, int32_t* n_steps_out, void* stream);
/* ---- beam_search, eval.py:36-120: log(sigmoid(logit)) scores (eval.py:61), cumulative score divided by
 * length^0.7 at every step (eval.py:53-59, length = position of the hypothesis' last <EOS>, else t+1), top beam_width of
 * beam_width * V continuations (eval.py:64).  best_out [caption_max_len+1][B] = the top-1 hypothesis (eval.py:119),
 * n_steps_out as above (eval.py:116).  beam_width <= 8. */
int recnet_beam_search(recnet_handle* h, const float* enc, int32_t beam_width, int64_t* best_out, int32_t* n_steps_out,
                       void* stream);
/* ---- sampling: one token per row drawn from softmax(logits / temperature) restricted to the top_k largest logits (the
 * reference has no counterpart: eval.py only has the two deterministic searches).  Gumbel-max on the counter-based hash of the
 * dropout masks: token = argmax_v (logit_v / temperature - log(-log u_v)), u_v a function of (seed, t, row, v) alone, so a call is
 * reproducible and a CPU restatement pins it (DESIGN.md "Sampling search").  logits [rows, V] contiguous, read only;
 * tokens_out [rows] int64; logprobs_out [rows] = log-probability of the token under the distribution sampled from (temperature
 * and top_k applied).  temperature > 0 and finite; 0 <= top_k <= V, 0 and V = no restriction, ties at the cut admitted lowest
 * index first, top_k = 1 = arg-max.  The handle supplies the device only: no decoder needs to be bound. */
int recnet_sample_rows(recnet_handle* h, const float* logits, int32_t rows, int32_t V, float temperature, int32_t top_k,
                       uint32_t seed, int32_t t, int64_t* tokens_out, float* logprobs_out, void* stream);
/* ---- sampling search (the reference has no counterpart; the loop is greedy_search's, eval.py:19-33, with the draw above in
 * place of the arg-max): same start state, eval mode, same stop rule, one device-side loop with no host sync; like the
 * reference's loop it keeps feeding a caption's own tokens after its <EOS>.  tokens_out [caption_max_len+1][B] int64,
 * logprobs_out [caption_max_len+1][B] float (row t drawn with step index t), n_steps_out as for recnet_greedy_search: only
 * rows [0, n_steps) are meaningful, later rows hold what the fixed-length loop went on to draw. */
int recnet_sample_search(recnet_handle* h, const float* enc, float temperature, int32_t top_k, uint32_t seed,
                         int64_t* tokens_out, float* logprobs_out, int32_t* n_steps_out, void* stream);
/* ---- nucleus (top-p) sampling, composed with top_k (the reference has no counterpart).  The two calls above
 * with one more cut: after the top_k cut, only the shortest prefix of the allowed entries (value descending, index ascending) whose
 * mass reaches top_p of the allowed mass is drawn from.  Masses are integers, floor(exp(s_v - max s) * 2^32) in fp32, summed exactly:
 * the set is a pure function of the logits, the same on every call.  Entries equal to the cut value are admitted lowest index first,
 * only as many as the target needs.  0 < top_p <= 1; top_p = 1 is no nucleus cut (tokens and log-probabilities of the calls above,
 * bit for bit); top_p < 1 needs V < 2^21.  n_allowed_out (int32, [rows] resp. [caption_max_len+1][B], may be NULL) = the size of the
 * set each token was drawn from, always >= 1; logprobs_out is the log-probability under that set. */
int recnet_sample_rows_nucleus(recnet_handle* h, const float* logits, int32_t rows, int32_t V, float temperature, int32_t top_k,
                               float top_p, uint32_t seed, int32_t t, int64_t* tokens_out, float* logprobs_out, int32_t* n_allowed_out,
                               void* stream);
int recnet_sample_search_nucleus(recnet_handle* h, const float* enc, float temperature, int32_t top_k, float top_p, uint32_t seed,
                                 int64_t* tokens_out, float* logprobs_out, int32_t* n_allowed_out, int32_t* n_steps_out, void* stream);

/* ---- scoring: how probable is a GIVEN token / caption under the model (the reference has no counterpart).
 * recnet_logprob_rows: logprobs_out[r] = s_k - logsumexp_v s_v with s_v = logits[r, v] / temperature and k = tokens[r] (the maximum
 * is subtracted before the exponentials); a token outside [0, V) gives -inf and is never used as an index.  logits [rows, V]
 * contiguous, read only; tokens [rows] int64; temperature > 0 and finite.  The handle supplies the device only, as for
 * recnet_sample_rows. */
int recnet_logprob_rows(recnet_handle* h, const float* logits, const int64_t* tokens, int32_t rows, int32_t V, float temperature,
                        float* logprobs_out, void* stream);
/* recnet_score_captions: the teacher-forced loop of train.py:25,45 in eval mode (no dropout) over tokens [T][B] int64, time-major,
 * 1 <= T <= caption_max_len + 1: step 0 is fed <SOS> and the zero state, step t > 0 is fed tokens[t - 1].
 * logprobs_out [T][B] = log-probability of tokens[t][b] under softmax(logits_t / temperature), every row, unmasked;
 * caption_logprob_out [B] = sum of rows 0 .. e_b in ascending t, e_b = the first t with tokens[t][b] == <EOS> (2) or T - 1 when
 * there is none (later rows never enter the sum); length_out [B] int32 = e_b + 1.  enc == NULL reuses the invariants of the previous
 * call / of recnet_decoder_prepare, like recnet_decoder_step.  PRECONDITION: every token lies in [0, V) (the embedding gather
 * indexes by them; the Python layer checks).  One stream-ordered sequence, no host synchronisation.  The call overwrites the saved
 * state of a decoder forward (hidden states, gate activations, logits): a following recnet_backward_decoder /
 * recnet_forward_reconstructor(hiddens = NULL) is refused with their state error until the next forward. */
int recnet_score_captions(recnet_handle* h, const float* enc, const int64_t* tokens, int32_t T, float temperature,
                          float* logprobs_out, float* caption_logprob_out, int32_t* length_out, void* stream);

/* ---- reconstruction error of GIVEN captions (the reference has no counterpart: it only ever forms the batch mean, as a training
 * loss).  How well does the reconstructor recover this video's features from the decoder states of this
 * caption?  Both reconstructors are separable per caption (models/global_reconstructor.py:30-46, models/local_reconstructor.py:37-55);
 * in eval mode (no dropout), for hidden states [T,1,B,H] and features enc [B,F,D]:
 *   global: recon[b, :] = mean_t out_t[b, :]  (train.py:96-98);   err[b] = (1 / R) sum_r (recon[b, r] - mean_f enc[b, f, r])^2 / T  (train.py:99-102)
 *   local:  recon[b, f, :] = out_f[b, :]      (train.py:125-127); err[b] = (1 / (F D)) sum_{f, d} (recon[b, f, d] - enc[b, f, d])^2  (train.py:128)
 * so mean_b err[b] is the reference's MSE term (rec_mse) at the same hidden states; the normaliser never involves the batch
 * (global_batch_size / batch_offset play no part).  Exactly one of tokens / hiddens is non-NULL: tokens [T][B] int64 = the
 * teacher-forced decoder forward in eval mode exactly as recnet_score_captions runs it (step 0 fed <SOS>; the same PRECONDITION:
 * every token in [0, V)), the reconstructor then runs on the states it leaves; hiddens [T,1,B,H] = states handed in, as
 * recnet_forward_reconstructor takes them.  1 <= T <= caption_max_len + 1; the global error depends on T, so errors of one video
 * are comparable only at a common T.  err_out [B]; recon_out NULL or the reconstruction itself, global [B,R], local [B,F,D].  One
 * fixed summation order per caption and no atomics: two calls on the same inputs return the same bits.  One stream-ordered
 * sequence, no host synchronisation, no allocation; a pending deferred update is completed first.  The call runs the
 * reconstructor's forward without its regulariser norms, loss epilogues and loss scalars (no recnet_scalars are written) and leaves
 * the handle between two steps: a following recnet_backward_reconstructor / recnet_backward_decoder /
 * recnet_forward_reconstructor(hiddens = NULL) is refused with their state error until the next forward.  RECNET_ESTATE: no
 * reconstructor (or, with tokens, no decoder) bound; RECNET_EINVAL: both or neither of tokens / hiddens, NULL enc / err_out, T out
 * of range. */
int recnet_reconstruction_error(recnet_handle* h, const float* enc, const int64_t* tokens, const float* hiddens, int32_t T,
                                float* err_out, float* recon_out, void* stream);

/* ---- N-best beam search on log-probabilities (the reference has no counterpart: recnet_beam_search above restates eval.py:36-120,
 * whose log(sigmoid) scores compare with nothing else here; DESIGN.md section 11 states the definitions).
 * recnet_beam_select_rows: one selection step on caller-supplied device arrays.  logits [nb][rows][V] contiguous, read only;
 * cum [nb][rows]; finished [nb][rows] int32.  A live hypothesis i of row r offers cum[i][r] + log_softmax(logits[i][r])[v] for every
 * v (the maximum is subtracted before the exponentials; the formulas of recnet_logprob_rows at temperature 1, bit for bit); a
 * finished one (finished != 0) offers v = <PAD> (0) at cum[i][r] and -inf at every other v.  vals_out / idx_out [rows][beam_width]:
 * the beam_width largest of the nb * V candidates in descending order, idx = i * V + v, the lowest idx first among equal values.
 * 1 <= nb <= 8, 1 <= beam_width <= min(8, V).  One launch, no score array, no atomics: two calls give the same bits.  The handle
 * supplies the device only, as for recnet_sample_rows. */
int recnet_beam_select_rows(recnet_handle* h, const float* logits, const float* cum, const int32_t* finished, int32_t nb,
                            int32_t rows, int32_t V, int32_t beam_width, float* vals_out, int32_t* idx_out, void* stream);
/* recnet_beam_search_nbest: start from <SOS>, the zero state and one hypothesis with cum = 0; at every step the selection above
 * over the hypotheses of a caption (1 at step 0, then beam_width), all of them advanced by ONE batched decode step; only <EOS> (2)
 * finishes a hypothesis, len = position of its <EOS> + 1, or the number of steps run when it has none.  n_steps_out (device int32)
 * = the first step after which every hypothesis of every caption is finished, + 1, else caption_max_len + 1; the device loop has a
 * fixed trip count and carries the hypotheses over unchanged with <PAD> appended.  Final rank per caption: score = cum /
 * len^length_alpha descending, lowest beam index among equals (length_alpha = 0: the raw sum).  tokens_out
 * [beam_width][caption_max_len+1][B] int64, rank-major: each rank is a time-major caption tensor with <PAD> behind <EOS>, which
 * recnet_score_captions / recnet_reconstruction_error take as it is (rows >= n_steps are <PAD>); cum_out / score_out
 * [beam_width][B] float, len_out [beam_width][B] int32.  RECNET_EINVAL before any launch: beam_width outside [1, min(8, V)],
 * length_alpha negative or not finite, a NULL pointer; RECNET_ESTATE: decoder not bound.  Like the other searches the call
 * overwrites the decoder's loop invariants and clears the saved forward. */
int recnet_beam_search_nbest(recnet_handle* h, const float* enc, int32_t beam_width, float length_alpha, int64_t* tokens_out,
                             float* cum_out, int32_t* len_out, float* score_out, int32_t* n_steps_out, void* stream);

/* ---- Constrained N-best beam search (no counterpart in the reference).  Three controls on what a LIVE
 * hypothesis offers at step t, given its generated history w_0 .. w_{t-1} (<SOS> is not part of it).  Token v is not offered if
 *   v is one of the n_banned ids of `banned`;  or  v = <EOS> (2) and t < min_length;  or  no_repeat_ngram = n >= 1, t >= n - 1 and
 *   (w_{t-n+1} .. w_{t-1}, v) already occurs in the history as an n-gram (n = 1: every token of the history).
 * Tokens compare as ids (<PAD> emitted by a live hypothesis is a token like any other).  Finished hypotheses are untouched: <PAD>
 * at cum and nothing else.  There is no renormalisation: an offered candidate keeps cum + log_softmax(logits)[v] over all V
 * entries, so cum remains the model's log-probability of the hypothesis and recnet_score_captions reproduces it as before.
 * Ranges: 0 <= no_repeat_ngram, min_length <= caption_max_len (0 = off), 0 <= n_banned <= 16, the ids distinct, in [0, V) and
 * not <EOS>.  `banned` is a HOST pointer, read during the call (the ids travel as kernel arguments: no device array, no copy, the
 * call stays capturable); it may be NULL when n_banned = 0.  With any constraint on, the call is refused unless every live
 * hypothesis is left at least beam_width offered tokens: beam_width + n_banned + caption_max_len + 1 <= V for the search,
 * beam_width + n_banned + t + 1 <= V for the kernel alone; -inf is then never selected from a live hypothesis.  With all three off
 * both entries launch the kernels of the unconstrained entries above and return the same bits.
 * recnet_beam_select_rows_constrained: recnet_beam_select_rows plus hist [nb][rows][Tm] int64 (device; entries [0, t) are read; may
 * be NULL when no_repeat_ngram = 0) and the step 0 <= t < Tm.  recnet_beam_search_nbest_constrained: recnet_beam_search_nbest with
 * the constrained selection at every step; recnet_beam_search_nbest is this entry with the constraints off.  RECNET_EINVAL before
 * any launch for everything above. */
int recnet_beam_select_rows_constrained(recnet_handle* h, const float* logits, const float* cum, const int32_t* finished,
                                        const int64_t* hist, int32_t nb, int32_t rows, int32_t V, int32_t Tm, int32_t t,
                                        int32_t beam_width, int32_t no_repeat_ngram, int32_t min_length, const int32_t* banned,
                                        int32_t n_banned, float* vals_out, int32_t* idx_out, void* stream);
int recnet_beam_search_nbest_constrained(recnet_handle* h, const float* enc, int32_t beam_width, float length_alpha,
                                         int32_t no_repeat_ngram, int32_t min_length, const int32_t* banned, int32_t n_banned,
                                         int64_t* tokens_out, float* cum_out, int32_t* len_out, float* score_out, int32_t* n_steps_out,
                                         void* stream);

/* ---- Diverse (group) N-best beam search (Vijayakumar et al., "Diverse Beam Search"; no counterpart in the reference; DESIGN.md
 * section 14).  beam_width = n_groups * w: slot k of a caption belongs to group k / w.  At step 0 every group selects from the one
 * start hypothesis; from step 1 on group g selects only from its own w hypotheses.  The groups of a step are decided in the order
 * g = 0, 1, ..: a live candidate (i, v) of group g is ordered by cum_i + log_softmax(logits_i)[v] - diversity_penalty * c, c = the
 * number of slots of the groups before g whose candidate selected at this step carries token v and came from a live hypothesis
 * (the <PAD> of a finished one is not counted; a finished hypothesis is never penalised).  The group keeps its w largest, the
 * lowest idx = i * V + v among equals (i: the slot), and the j-th becomes slot g * w + j.  The value a hypothesis carries is the
 * UN-penalised one: cum stays the model's log-probability, recnet_score_captions reproduces it, and inside a group the slots are
 * ordered by the penalised value, not by cum.  The constraints of section 12 apply as they do there.  The final rank runs over all
 * beam_width slots as in recnet_beam_search_nbest; different groups may return the same caption.  n_groups = 1 launches the kernels
 * of the entries above and returns their bits, for any penalty; group 0 is never penalised.
 * recnet_beam_select_rows_diverse: one grouped selection on caller-supplied arrays, the arguments of
 * recnet_beam_select_rows_constrained; nb must be 1 (every group selects from hypothesis 0) or beam_width; vals_out holds the
 * un-penalised values.  recnet_beam_search_nbest_diverse: recnet_beam_search_nbest_constrained with the grouped selection at every
 * step; group_out [beam_width][B] int32 (may be NULL): the group of each returned rank.  RECNET_EINVAL before any launch: everything
 * the constrained entries refuse, n_groups < 1 or not a divisor of beam_width, diversity_penalty negative or not finite. */
int recnet_beam_select_rows_diverse(recnet_handle* h, const float* logits, const float* cum, const int32_t* finished,
                                    const int64_t* hist, int32_t nb, int32_t rows, int32_t V, int32_t Tm, int32_t t, int32_t beam_width,
                                    int32_t n_groups, float diversity_penalty, int32_t no_repeat_ngram, int32_t min_length,
                                    const int32_t* banned, int32_t n_banned, float* vals_out, int32_t* idx_out, void* stream);
int recnet_beam_search_nbest_diverse(recnet_handle* h, const float* enc, int32_t beam_width, float length_alpha, int32_t n_groups,
                                     float diversity_penalty, int32_t no_repeat_ngram, int32_t min_length, const int32_t* banned,
                                     int32_t n_banned, int64_t* tokens_out, float* cum_out, int32_t* len_out, float* score_out,
                                     int32_t* group_out, int32_t* n_steps_out, void* stream);

/* ---- Ensemble decoding: beam search and scoring over M decoders (no counterpart in the reference; added at
 * version 12 without changing any existing entry).  An ensemble is M handles (1 <= M <= 8, all different) with a bound workspace
 * and a bound decoder, on one device, that agree on B, F, D, V and caption_max_len; E, H, A, the cell, the attention normalisation
 * and the precision may differ.  weights: a HOST array of M positive finite floats (NULL: uniform), normalised by the library in
 * float64 to w_m, sum 1.  For one row, with x_m [V] the logits of member m and l_m = log_softmax(x_m) (the formulas of
 * recnet_logprob_rows at temperature 1):
 *   RECNET_ENS_ARITHMETIC  y[v] = a + log sum_m exp(log w_m + l_m[v] - a),  a = max_m (log w_m + l_m[v])    (log of the mean probability)
 *   RECNET_ENS_GEOMETRIC   y[v] = sum_m w_m l_m[v]                                                          (mean log-probability)
 * summed over m ASCENDING by the one thread that owns v: no atomics, two calls give the same bits, equal rows get equal bits.  y
 * are the ensemble's LOGITS: the selection and the scorer form cum + (y[v] - logsumexp(y)) from them as from one model's (the usual
 * renormalisation in the geometric mode; logsumexp(y) = 0 up to rounding in the arithmetic one), so constraints, groups, the ranking
 * and "recnet_score_captions reproduces cum" hold for the ensemble entries as they do for the single-model ones. */
#define RECNET_ENS_ARITHMETIC 0
#define RECNET_ENS_GEOMETRIC 1
/* recnet_ensemble_mix_rows: the mix alone on caller-supplied rows.  logits: a HOST array of M device pointers, each [rows][V] float,
 * read only; y_out [rows][V] may be logits[0] itself (in place) and must overlap no other input.  It runs for M = 1 too
 * (y = log_softmax(x_0)).  The handle supplies the device only.  RECNET_EINVAL before any launch: a NULL pointer, M outside [1, 8],
 * a weight that is not positive and finite, an unknown mode, rows or V below 1, an overlap other than the one allowed. */
int recnet_ensemble_mix_rows(recnet_handle* h, const float* const* logits, int32_t M, const float* weights, int32_t mode, int32_t rows,
                             int32_t V, float* y_out, void* stream);
/* recnet_beam_search_nbest_ensemble: recnet_beam_search_nbest_diverse on the ensemble's logits; the arguments from beam_width on are
 * that entry's.  hs: a HOST array of M handles.  Every step runs the decode step of every member on the tokens member 0 holds,
 * mixes the nb * B rows, selects as before, and applies the regather (src = idx / V) to every member's own recurrent state;
 * history, cum, lengths and tokens exist once.  M = 1 launches what recnet_beam_search_nbest_diverse launches and returns its bits.
 * RECNET_EINVAL / RECNET_ESTATE before any launch: hs NULL, M outside [1, 8], a NULL or repeated member, a member without workspace
 * or bound decoder, members on different devices or with unequal B, F, D, V or caption_max_len, a bad weight or mode, and
 * everything recnet_beam_search_nbest_diverse refuses. */
int recnet_beam_search_nbest_ensemble(recnet_handle* const* hs, int32_t M, const float* weights, int32_t mode, const float* enc,
                                      int32_t beam_width, float length_alpha, int32_t n_groups, float diversity_penalty,
                                      int32_t no_repeat_ngram, int32_t min_length, const int32_t* banned, int32_t n_banned,
                                      int64_t* tokens_out, float* cum_out, int32_t* len_out, float* score_out, int32_t* group_out,
                                      int32_t* n_steps_out, void* stream);
/* recnet_score_captions_ensemble: recnet_score_captions at temperature 1 on the ensemble's logits: the teacher-forced forward and
 * the vocabulary product of every member, one mix over the T * B rows, then the row kernel and the per-caption sums.  It reproduces
 * the cum of recnet_beam_search_nbest_ensemble as recnet_score_captions does for one model.  enc NULL: every member reuses its own
 * invariants.  M = 1 launches what recnet_score_captions launches.  Refusals: those of the ensemble search on hs / M / weights /
 * mode, and those of recnet_score_captions. */
int recnet_score_captions_ensemble(recnet_handle* const* hs, int32_t M, const float* weights, int32_t mode, const float* enc,
                                   const int64_t* tokens, int32_t T, float* logprobs_out, float* caption_logprob_out, int32_t* length_out,
                                   void* stream);

/* ---- Stochastic beam search (Kool, van Hoof, Welling 2019; no counterpart in the reference; added at
 * version 12 without changing any existing entry): beam_width captions per video drawn WITHOUT replacement from the model's
 * sequence distribution at the given temperature, in one search of that width.  A hypothesis carries phi, its log-probability (the
 * cum of recnet_beam_search_nbest), and G, its perturbed score; the start hypothesis has phi = G = 0.
 * recnet_sbs_select_rows: one selection step on caller-supplied device arrays.  logits [nb][rows][V] contiguous, read only; cum,
 * gum [nb][rows] float (phi and G); finished [nb][rows] int32.  A live hypothesis i of row r offers every v with
 *   phi_v = cum[i][r] + log_softmax(logits[i][r] / temperature)[v]     (the formulas of recnet_logprob_rows, bit for bit)
 *   Gt_v  = phi_v + g_v, g_v the Gumbel of recnet_sample_rows on the counter ((t * beam_width * rows + i * rows + r) * V + v) mod 2^32
 *   Ghat_v = -log(exp(-gum[i][r]) - exp(-max_v Gt_v) + exp(-Gt_v))     (in double from the fp32 inputs, rounded to fp32)
 * so that the largest Ghat of a parent is the parent's G exactly; a finished one (finished != 0) offers v = <PAD> (0) at
 * (cum[i][r], gum[i][r]) without noise and -inf at every other v.  vals_out / gum_out / idx_out [rows][beam_width]: phi, Ghat and
 * idx = i * V + v of the beam_width largest Ghat in descending order, the lowest idx first among equal values.  1 <= nb <= 8,
 * 1 <= beam_width <= min(8, V), temperature positive and finite, t >= 0.  One launch, no score array, no atomics: two calls give
 * the same bits.  The handle supplies the device only, as for recnet_beam_select_rows.
 * recnet_stochastic_beam_search: the loop of recnet_beam_search_nbest (one batched decode step for all hypotheses, only <EOS>
 * finishes, the same n_steps_out and fixed trip count) with the selection above at every step t, beam_width the search's width in
 * the counter at step 0 too.  Rank = slot: G descending, the lowest slot among equals.  Rank 0 is an exact sample from the model,
 * ranks 0 .. beam_width - 1 a sample without replacement; with beam_width = 1 the counters are those of
 * recnet_sample_search(temperature, top_k = 0, seed).  tokens_out [beam_width][caption_max_len+1][B] int64, rank-major and canonical
 * like recnet_beam_search_nbest's; cum_out (phi) / gum_out (G) [beam_width][B] float; len_out [beam_width][B] int32.  A hypothesis
 * that reaches caption_max_len + 1 tokens without <EOS> is a PREFIX: its cum is the probability of the prefix, not of a caption.
 * recnet_score_captions at the same temperature reproduces cum and len.  No top-k / top-p cut, constraints or groups: they change
 * the distribution the conditioning assumes.
 * recnet_stochastic_beam_search_ensemble: the same search on the ensemble's logits (hs, M, weights, mode as for
 * recnet_beam_search_nbest_ensemble; M = 1 launches what the single-model entry launches and returns its bits).
 * RECNET_EINVAL before any launch: a NULL pointer, beam_width outside [1, min(8, V)], temperature not positive and finite, the
 * refusals of the ensemble entries; RECNET_ESTATE: decoder not bound. */
int recnet_sbs_select_rows(recnet_handle* h, const float* logits, const float* cum, const float* gum, const int32_t* finished, int32_t nb,
                           int32_t rows, int32_t V, int32_t beam_width, float temperature, uint32_t seed, int32_t t, float* vals_out,
                           float* gum_out, int32_t* idx_out, void* stream);
int recnet_stochastic_beam_search(recnet_handle* h, const float* enc, int32_t beam_width, float temperature, uint32_t seed,
                                  int64_t* tokens_out, float* cum_out, int32_t* len_out, float* gum_out, int32_t* n_steps_out, void* stream);
int recnet_stochastic_beam_search_ensemble(recnet_handle* const* hs, int32_t M, const float* weights, int32_t mode, const float* enc,
                                           int32_t beam_width, float temperature, uint32_t seed, int64_t* tokens_out, float* cum_out,
                                           int32_t* len_out, float* gum_out, int32_t* n_steps_out, void* stream);

/* ---- Consensus (minimum-Bayes-risk) scoring of hypotheses against a reference set by n-gram overlap (no counterpart in the
 * reference; added at version 12 without changing any existing entry).
 * The WORDS of a caption, a column t_0 .. t_{T-1} of tokens, are the tokens before its first <EOS> (2), at most T; every other id
 * is an ordinary word, <PAD> (0) included; whatever stands behind the first <EOS> is ignored.  L = the number of words.  For
 * n = 1..4 let c_n(g) be the occurrences of n-gram g in the caption.  For a hypothesis h and a reference r, exact integers:
 *   M_n(h, r) = sum_g min(h_n(g), r_n(g)) * r_n(g)        Q_n(c) = sum_g c_n(g)^2
 *   sim(h, r) = 1/4 * sum_{n=1..4} [ M_n / sqrt(Q_n(h) * Q_n(r)) if Q_n(h) > 0 and Q_n(r) > 0, else 0 ] * exp(-(L_h - L_r)^2 / (2 sigma^2))
 * (coco CIDEr's clipped cosine and Gaussian length penalty with a uniform idf).  The utility of hypothesis i is
 *   util_i = (sum_j sim(i, j)) / N_r   without weights,     util_i = sum_j w_j * sim(i, j)   with weights (widened to double),
 * summed in float64 over j ASCENDING, one term after the other from 0.0: two hypotheses with the same words get the same bits.
 * n-grams are equal when their tokens are; nothing is hashed.  hyp [N_h][T_h][B] int64, B innermost (what
 * recnet_beam_search_nbest leaves); ref [N_r][T_r][B], or NULL: the hypotheses are their own references, the term j = i included
 * (N_r and T_r are then ignored).  weights [N_r][B] float or NULL.  util_out [N_h][B] double; optional (NULL: not written)
 * sim_out [N_h][N_r][B] double, counts_out [N_h][N_r][B][4] int32 (M_n), q_hyp_out [N_h][B][4], q_ref_out [N_r][B][4],
 * len_hyp_out [N_h][B], len_ref_out [N_r][B] int32.  One launch, integer counting, no atomics: two calls give the same bits.
 * RECNET_EINVAL before any launch: N_h / N_r outside [1, 32], T_h / T_r outside [1, 64], B < 1, sigma not positive and finite, a
 * NULL hyp or util_out.  Tokens must lie in [0, 2^31): the caller's duty (they are compared as 32-bit ids).  The handle supplies
 * the device only: no decoder needs to be bound, and B is the argument, not the handle's. */
int recnet_consensus_rows(recnet_handle* h, const int64_t* hyp, int32_t N_h, int32_t T_h, const int64_t* ref, int32_t N_r, int32_t T_r,
                          int32_t B, const float* weights, double sigma, double* util_out, double* sim_out, int32_t* counts_out,
                          int32_t* q_hyp_out, int32_t* q_ref_out, int32_t* len_hyp_out, int32_t* len_ref_out, void* stream);

/* ---- forward_decoder, train.py:17-75 (teacher forcing, train.py:38,45).
 * enc [B,F,D]; targets [caption_max_len+1, B] int64 (time-major, <PAD>=0, <EOS>=2);
 * T = number of steps the reference's loop would run (train.py:66), computed by the caller from the
 * caption lengths (host) — no device sync; step_weight [T] = 1 / (n_t * sum_t n_t) with GLOBAL counts
 * (SURVEY.md §8e); hiddens_out [T,1,B,H] (may be NULL: they stay in the workspace for the
 * reconstructor either way); scalars: dec_ce / dec_reg / dec_loss are written. */
int recnet_forward_decoder(recnet_handle* h, const float* enc, const int64_t* targets, int32_t T,
                           const float* step_weight, int32_t train, uint32_t seed, float* hiddens_out,
                           recnet_scalars* scalars, void* stream);

/* ---- forward_decoder without teacher forcing, train.py:46-51 — the validation pass (train.py:327 calls
 * forward_decoder with the default teacher_forcing_ratio = 0): the input of step t+1 is the arg-max of the logits
 * Decoder.forward returned at step t.  Same arguments and loss as recnet_forward_decoder (targets / masks only enter the
 * loss and T); output_indices [T,B] int64 receives the fed-back tokens (train.py:50, `output_indices`).  A following
 * recnet_backward_decoder differentiates this pass (the arg-max passes no gradient; the embedding gradient is scattered to
 * the rows of the tokens that were fed); the hidden states feed recnet_forward_reconstructor as usual. */
int recnet_forward_decoder_free(recnet_handle* h, const float* enc, const int64_t* targets, int32_t T,
                                const float* step_weight, int32_t train, uint32_t seed, float* hiddens_out,
                                int64_t* output_indices, recnet_scalars* scalars, void* stream);

/* ---- forward_global_reconstructor (train.py:78-105) / forward_local_reconstructor (train.py:108-131),
 * selected by cfg.reconstructor_type.  Consumes the hidden states left by recnet_forward_decoder
 * (or `hiddens` [T,1,B,H] when not NULL).  mse_count = GLOBAL element count of the MSE mean
 * (global: B_global*R, local: B_global*F*D).  Writes rec_mse / rec_reg / rec_loss / total_loss. */
int recnet_forward_reconstructor(recnet_handle* h, const float* enc, const float* hiddens, int32_t T,
                                 int32_t train, uint32_t seed, recnet_scalars* scalars, void* stream);

/* ---- loss.backward(), train.py:268, for loss = dec_loss + lambda_recon * rec_loss (train.py:260).
 * Reconstructor first (produces d loss / d hiddens), then the decoder BPTT.  grad_scale multiplies
 * the incoming gradient (1.0 in the reference).  The norm-regulariser gradient lambda * p/||p|| is
 * NOT included here (it is rank-independent; recnet_optimizer_step / recnet_add_reg_grad add it
 * once, after the data-parallel all-reduce — SURVEY.md §8e). */
int recnet_backward_reconstructor(recnet_handle* h, const float* enc, float grad_scale, float* dhiddens_out,
                                  void* stream);
int recnet_backward_decoder(recnet_handle* h, const float* enc, const int64_t* targets, const float* dhiddens,
                            float grad_scale, void* stream);
/* grad += lambda_reg * grad_scale * p / ||p||  for every tensor of the model (autograd-compatible path). */
int recnet_add_reg_grad(recnet_handle* h, int32_t which /*0 decoder, 1 reconstructor*/, float grad_scale,
                        void* stream);

/* ---- train.py:269-273: clip_grad_norm_(decoder, gradient_clip) + decoder Adam(amsgrad) step +
 * reconstructor Adam step (torch.optim.Adam semantics, coupled weight decay); then re-packs the
 * weights.  `step` is the 1-based optimiser step count.  flags: */
#define RECNET_OPT_REG 1                 /* fold the regulariser gradient lambda * p/||p|| in        */
#define RECNET_OPT_CLIP 2                /* clip the decoder gradient to cfg.gradient_clip first      */
#define RECNET_OPT_SKIP_DECODER 4
#define RECNET_OPT_SKIP_RECONSTRUCTOR 8
int recnet_optimizer_step(recnet_handle* h, int32_t step, int32_t flags, recnet_scalars* scalars, void* stream);
/* torch.nn.utils.clip_grad_norm_ (train.py:270) on the bound gradients of one model, in place;
 * total_norm_out: device float or NULL. */
int recnet_clip_grad_norm(recnet_handle* h, int32_t which, float max_norm, float* total_norm_out, void* stream);

/* ---- The whole train-step body, train.py:248-273, on one stream: forward decoder, forward
 * reconstructor, backward, clip, both optimiser steps.  With world size > 1 the caller instead runs
 * recnet_train_step_fwd_bwd, all-reduces (SUM) the gradient tensors, then recnet_optimizer_step. */
int recnet_train_step_fwd_bwd(recnet_handle* h, const float* enc, const int64_t* targets, int32_t T,
                              const float* step_weight, uint32_t seed, recnet_scalars* scalars, void* stream);
int recnet_train_step(recnet_handle* h, const float* enc, const int64_t* targets, int32_t T,
                      const float* step_weight, uint32_t seed, int32_t step, recnet_scalars* scalars,
                      void* stream);

/* The fused step for graph replay (single rank): recnet_train_step with the step count and the dropout seed taken from
 * device memory (advanced by the call itself, seed = seed_base + step) — forward, backward, then the optimiser with
 * `flags`.  The reconstructor's optimiser step is issued as soon as its gradients are complete, under the decoder's
 * backward chain; the decoder's follows the clip (train.py:265-273 as one capturable sequence). */
int recnet_train_step_dev(recnet_handle* h, const float* enc, const int64_t* targets, int32_t T, const float* step_weight,
                          uint32_t seed_base, int32_t flags, recnet_scalars* scalars, void* stream);

/* hipGraph-replay-friendly forms: the optimiser step count and the dropout seed live in device memory.
 * recnet_set_step initialises the counter; *_fwd_bwd_dev first does step += 1, seed = seed_base + step
 * on the device, so replaying a captured graph advances both; *_optimizer_step_dev reads the counter. */
int recnet_set_step(recnet_handle* h, int32_t step, void* stream);
int recnet_train_step_fwd_bwd_dev(recnet_handle* h, const float* enc, const int64_t* targets, int32_t T,
                                  const float* step_weight, uint32_t seed_base, recnet_scalars* scalars, void* stream);
/* The same forward + backward in two launches, so that a data-parallel caller can all-reduce the reconstructor's
 * gradient bucket while the decoder's backward is still running: part 1 = step += 1, decoder forward, loss,
 * reconstructor forward + complete backward (all reconstructor gradients final, d loss / d hiddens kept);
 * part 2 = decoder BPTT + deferred decoder gradients. */
int recnet_train_step_part_dev(recnet_handle* h, int32_t part, const float* enc, const int64_t* targets, int32_t T,
                               const float* step_weight, uint32_t seed_base, recnet_scalars* scalars, void* stream);
int recnet_optimizer_step_dev(recnet_handle* h, int32_t flags, recnet_scalars* scalars, void* stream);
/* Deferred reconstructor update (opt-in; the fused single-rank step recnet_train_step[_dev] only).  train.py:272-273 steps
 * the two optimisers one after the other at the end of an iteration; nothing reads the reconstructor's parameters again
 * before the NEXT iteration's reconstructor forward (train.py:256).  With on != 0 a fused step therefore leaves the
 * reconstructor's weight-gradient products + Adam update PENDING (its gate gradients and saved activations stay in the
 * workspace), and the next fused step runs them on a third stream under its decoder forward chain — CUs that chain leaves
 * idle — instead of under / behind this step's decoder BPTT.  Same arithmetic in the same order: parameters after
 * recnet_flush are bit-identical to the non-deferred step's.  recnet_flush completes a pending update on `stream` (a no-op
 * on the device when nothing is pending); every other entry point of the handle that reads the reconstructor's parameters,
 * gradients or Adam state flushes first, callers that read them through their own pointers (state_dict, checkpoints)
 * call recnet_flush themselves.
 * on == 2 (global reconstructor): SPLIT update — only the recurrent weights (rnn.weight_hh_l0: 60 % of the reconstructor's
 * weight-gradient work) are left pending; the input-side weights, the output layer and the biases are updated inside the step,
 * beside the decoder's BPTT chain.  The pending product then fits under the next step's decoder forward chain (137 workgroups,
 * 119 CUs idle) without delaying that step's reconstructor, and this step's BPTT window is not overfilled. */
int recnet_set_deferred_reconstructor_update(recnet_handle* h, int32_t on, void* stream);
int recnet_flush(recnet_handle* h, void* stream);
/* A hipGraph that captured a fused step was replayed (replays run no host code): tells the handle that — with the deferred
 * update on — an update may be pending, so that its other entry points catch up before they touch the reconstructor. */
int recnet_mark_pending(recnet_handle* h);

/* Data-parallel step inside ONE stream-ordered sequence (or one captured graph): with on != 0, part 1 of
 * recnet_train_step_part_dev returns with the reconstructor's weight-gradient products still running on the library's side
 * stream; recnet_join_side makes `stream` — the stream the caller launches the all-reduce of the reconstructor bucket from — wait
 * for them, while the caller's main stream goes straight on to part 2 (the decoder's BPTT).  Without it part 1 waits for those
 * products itself (+0.2 ms in front of the BPTT at the benchmark shape).  train.py:264-273; SURVEY.md section 8e. */
int recnet_set_dp_overlap(recnet_handle* h, int32_t on);
int recnet_join_side(recnet_handle* h, void* stream);
/* A stream capture that contained calls of this library was abandoned (e.g. api.GraphedStep: a collective could not be captured,
 * train.py:264-273 under data parallelism): the enqueue-time bookkeeping of the step those calls were part of — open side
 * branches, recorded-but-unjoined fork events, the data-parallel overlap switch — is put back to "between two steps".  No device
 * work, no effect on parameters, gradients or a pending deferred update. */
int recnet_abort_step(recnet_handle* h);

/* ---- plumbing exposed for tests and profiling */
/* Between begin and end every recurrent-step GEMM launch of one site (the dependent-chain kernels: one
 * per decoder / reconstructor time step) is bracketed by hipEvents on its stream; end() synchronises and
 * returns the launch count and summed duration.  Not for use under graph capture. */
#define RECNET_SITE_DEC_FWD 1   /* gates_t   = [ctx_t, h_{t-1}] . [W_ih[:,E:] | W_hh]^T       */
#define RECNET_SITE_DEC_BWD 2   /* d[ctx, h] = dgates_t . [W_ih[:,E:] | W_hh]                   */
#define RECNET_SITE_REC_FWD 3   /* reconstructor gates (global: hr . W_hh^T; local: [x, hr] . [W_ih | W_hh]^T) */
#define RECNET_SITE_REC_BWD 4
#define RECNET_SITE_REC_ATT 5   /* local reconstructor: hr . attn_W^T                           */
#define RECNET_SITE_REC_ATT_BWD 6
#define RECNET_SITE_REC_CHAIN_FWD 7   /* global reconstructor, bf16: the whole forward chain as one persistent launch */
#define RECNET_SITE_REC_CHAIN_BWD 8   /* ... and the whole backward chain                                              */
#define RECNET_SITE_DEC_CHAIN_FWD 9   /* decoder, bf16, teacher-forced: the whole forward chain as one persistent launch */
#define RECNET_SITE_DEC_CHAIN_BWD 10  /* ... and the whole BPTT chain                                                    */
#define RECNET_SITE_RECON_ERR 11      /* recnet_reconstruction_error: the row kernel (and the sum of its parts) alone          */
int recnet_profile_begin(recnet_handle* h, int32_t site);
int recnet_profile_end(recnet_handle* h, int32_t* n_launches, double* total_ms);
/* Same read-out without leaving profiling mode.  Brackets are taken around EAGER launches only: on a capturing stream the
 * launches of the site are not bracketed (round 4: event-record nodes read back after every replay aborted inside the HIP
 * runtime in about 1 of 100 bench runs; a replayed graph is described by recnet_read_stamps instead). */
int recnet_profile_read(recnet_handle* h, int32_t* n_launches, double* total_ms);
/* Phase stamps of the LAST train step, written by the step's own kernels (no tracer, no extra launch, also in a replayed
 * hipGraph): 14 values of the device's 100 MHz wall clock (10 ns units) —
 *   [0] step start (the step-counter kernel of recnet_train_step[_fwd_bwd]_dev)
 *   [1 + 2k], [2 + 2k] workgroup 0 of chain kernel k started running / left, k = 0 decoder forward chain, 1 decoder BPTT chain,
 *                      2 global reconstructor forward, 3 global reconstructor backward, 4 local reconstructor forward, 5 local backward
 *                      (the last launch of that chain; a chain that did not run keeps its old stamps)
 *   [13] step end (the kernel that exports the step's scalars)
 *   n >= 30: [14 + 2j], [15 + 2j] first workgroup started / last workgroup left of the grouped GEMM launch of site j:
 *            0 decoder prologue (Xe, Uv, P), 1 reconstructor weight gradients inside the step, 2 the pending half of a split
 *            reconstructor update (mode 2), 3 decoder weight gradients.
 * Synchronises `stream`.  train.py:248-273 is the span between [0] and [13]. */
int recnet_read_stamps(recnet_handle* h, uint64_t* out, int32_t n, void* stream);
/* Calibration of the bracket itself: `count` launches of an empty kernel bracketed by the same two event records (call
 * between recnet_profile_begin and _read/_end, in the same eager / captured mode as the measurement).  bracket(count) =
 * E + count * f: E is what the two event records add to every bracketed duration, f the dispatch-to-completion time of
 * an empty kernel; a bracketed kernel's own dispatch-to-completion time is its bracket minus E. */
int recnet_profile_null_launch(recnet_handle* h, int32_t count, void* stream);
/* C[M,N] (+)= alpha * op(A) op(B)^T + bias.  a_col / b_col: operand stored with the contraction index
 * as the ROW index (see csrc/gemm.hpp).  All fp32 device pointers. */
int recnet_gemm(int32_t precision, const float* A, int32_t a_col, int32_t lda, const float* B, int32_t b_col,
                int32_t ldb, float* C, int32_t ldc, const float* bias, int32_t M, int32_t N, int32_t K,
                float alpha, int32_t accumulate, int32_t splitk, float* splitk_ws, void* stream);
/* Same with bf16 operands in memory (the production kernel of the bf16 path, csrc/gemm_lds.hpp): needs 16-byte
 * aligned bases and leading dimensions that are multiples of 8.  tag 0 = batched form, 1..5 = chain-site forms. */
int recnet_gemm_bf16(const void* A, int32_t a_col, int32_t lda, const void* B, int32_t b_col, int32_t ldb, float* C,
                     int32_t ldc, const float* bias, int32_t M, int32_t N, int32_t K, float alpha, int32_t accumulate,
                     int32_t splitk, float* splitk_ws, int32_t tag, void* stream);
/* Grouped form: the tiles of n <= 8 products of one operand layout in ONE launch (csrc/gemm_lds.hpp: gemm_group_kernel); a
 * product the scheduler splits along K is summed inside the launch by its last-arriving slice.  Arrays of n entries; splitk_ws:
 * fp32 slabs (may be null: no splitting), counters: zero-initialised words the launch leaves zeroed (null: no splitting).
 * The batched products of train.py:258-273 (the decoder's and reconstructor's weight gradients) are issued this way. */
int recnet_gemm_group_bf16(int32_t a_col, int32_t b_col, int32_t n, const void* const* A, const int32_t* lda, const void* const* B,
                           const int32_t* ldb, float* const* C, const int32_t* ldc, const float* const* bias, const int32_t* M,
                           const int32_t* N, const int32_t* K, const float* alpha, const int32_t* accumulate, float* splitk_ws,
                           int64_t ws_floats, uint32_t* counters, int32_t n_counters, void* stream);
/* Probe builds only (csrc: make probe): in-kernel wall-clock stamps of the local chain kernels' last launch,
 * [role][step][8] uint64 ticks; RECNET_ESTATE in the product build. */
int recnet_probe_read(recnet_handle* h, uint64_t* out, int32_t n);
/* Test hook: fills the LDS of every CU with NaN patterns, so that a kernel reading LDS it never wrote fails the parity
 * tests deterministically. */
int recnet_debug_poison_lds(recnet_handle* h, void* stream);
/* Dimensions a handle was created with (the torch.ops layer sizes its outputs from these). */
#define RECNET_DIM_B 0
#define RECNET_DIM_F 1
#define RECNET_DIM_D 2
#define RECNET_DIM_E 3
#define RECNET_DIM_H 4
#define RECNET_DIM_A 5
#define RECNET_DIM_V 6
#define RECNET_DIM_R 7
#define RECNET_DIM_RA 8
#define RECNET_DIM_TM 9      /* caption_max_len + 1: rows of `targets` */
#define RECNET_DIM_SPLIT_FITS 10   /* 1: mode 2 of recnet_set_deferred_reconstructor_update is applied at this shape (the pending
                                    * product fits beside the decoder's forward chain); 0: the step updates immediately */
int32_t recnet_dim(const recnet_handle* h, int32_t which);
/* One reconstructor step with the reference's per-step semantics — GlobalReconstructor.forward(input, hidden,
 * decoder_hiddens) (models/global_reconstructor.py:30-46, called at train.py:94) and LocalReconstructor.forward(hidden,
 * decoder_hiddens) (models/local_reconstructor.py:37-55, called at train.py:123).  input [B][H] (global only: the layer-0
 * slice of decoder_hiddens[t]); hr_in / cr_in [B][R] or NULL for the zero state (GRU: cr_* unused); decoder_hiddens
 * [T][B][H] fp32, or NULL to reuse the loop invariants of the previous call; out [B][R] = out(h'), hr_out / cr_out
 * [B][R].  t indexes the dropout mask of this call (the reference draws a fresh mask per call).  Forward only. */
int recnet_reconstructor_step(recnet_handle* h, const float* input, const float* hr_in, const float* cr_in,
                              const float* decoder_hiddens, int32_t T, float* out, float* hr_out, float* cr_out,
                              int32_t train, uint32_t seed, int32_t t, void* stream);
/* Health of the persistent chain kernels (bounded waits): status bits 1/2 reconstructor fwd/bwd chain, 4/8 decoder
 * fwd/BPTT chain, 32/64 local reconstructor fwd/bwd chain gave up a wait; 256 the step's loss was poisoned (NaN) and the
 * optimiser kernels skip their updates.  Synchronises `stream`.  recnet_chain_reset clears the sticky words;
 * disable_persistent != 0 switches the handle to the per-step kernels for every later call. */
/* Gradient transport of the data-parallel step in its direct form (one reduce-scatter message per peer, i.e. per xGMI link, then an
 * all-gather: SURVEY.md section 8e; train.py:264-273 under data parallelism).  The collectives themselves are RCCL's; these are
 * the staging kernels around them, on `stream`, no handle needed:
 *   recnet_dp_cast    dst[i] = (dst type) src[i], n elements; *_bf16 = 0: fp32, 1: bf16 (fp32 -> wire type before the reduce-scatter,
 *                     wire type -> the fp32 gradient buffer after the all-gather)
 *   recnet_dp_reduce  red[j] = (wire type) sum_{r = 0 .. world-1, in rank order} (float) recv[r * chunk + j]: fp32 accumulation at the
 *                     destination, one rounding of the sum (world <= 16) */
int recnet_dp_cast(const void* src, int32_t src_bf16, void* dst, int32_t dst_bf16, int64_t n, void* stream);
int recnet_dp_reduce(const void* recv, int32_t world, int64_t chunk, void* red, int32_t wire_bf16, void* stream);
/* Measurement hook: the last seven step-start stamps (out16[1..7], written by the step's first kernel; out16[0] = how many steps ever
 * started) and step-end stamps (out16[9..15] / out16[8]) of recnet_train_step_dev, 100 MHz wall clock, slot of step n = 1 + (n - 1) % 7
 * counting from the handle's first step: the idle time between back-to-back replays of a captured step, read directly.
 * Synchronises the stream. */
int recnet_read_step_ring(recnet_handle* h, uint64_t* out16, void* stream);
int recnet_chain_status(recnet_handle* h, int32_t* status_out, void* stream);
int recnet_chain_reset(recnet_handle* h, int32_t disable_persistent, void* stream);
/* Test hook: what a chain kernel does when it gives up a bounded wait (chain_sync.hpp: rc_give_up) — raises the sticky word
 * of chain `chain_bit` (one of 1, 2, 4, 8, 32, 64) and the poison word, stream-ordered. */
int recnet_debug_raise_give_up(recnet_handle* h, int32_t chain_bit, void* stream);
/* Test hook: a kernel of `n_workgroups` workgroups that each take a whole CU (160 KB of LDS) and spin for `microseconds` —
 * what a resident collective (RCCL) kernel looks like to the persistent chain kernels.  Launch it on another stream. */
int recnet_debug_occupy(recnet_handle* h, int32_t n_workgroups, int32_t microseconds, void* stream);
/* Test hook: the packed operand images of the weights (bf16 / fp32 copies, transposes, streamed fragments — what the kernels
 * read instead of the master parameters; rewritten by the optimiser kernels, by the Adam epilogue of the pending d W_hh product
 * and by recnet_pack_weights) are copied aside, re-packed from the master parameters, and compared: *n_diff_out = number of
 * 16-bit words that differ (0 = every image was up to date).  Completes a pending deferred update first; synchronises the
 * stream; leaves the images freshly packed.  Holds train.py:271-273 "the next forward uses the updated weights" for the images. */
int64_t recnet_debug_images_bytes(recnet_handle* h);       /* bytes of device scratch recnet_debug_images_stale needs (256-byte aligned) */
int recnet_debug_images_stale(recnet_handle* h, void* scratch_dev, int64_t scratch_bytes, int64_t* n_diff_out, void* stream);
/* Test hook: byte offset inside the bound workspace of a saved tensor of the local reconstructor's forward pass
 * (0: Whr [F][B][RA], 1: beta [F][B][T], 2: Hr [F][B][R], 3: acts [F][B][4R]), or of the dlogits operand of the output layer's
 * backward products (4: [Tm][B][ldV], ldV = V rounded up to 8, bf16 or fp32 by the precision); -1 if unknown. */
int64_t recnet_debug_offset(const recnet_handle* h, int32_t which);
/* Name / start / duration of the dominant kernel's launches inside the last train step are measured
 * by the caller with hipEvents; this returns the ALGORITHMIC bytes of one launch: loop invariants once, every input /
 * saved tensor once.  The step-to-step exchange blocks of a persistent chain kernel are not part of it. */
double recnet_recurrent_step_bytes(const recnet_handle* h, int32_t which /*0 decoder fwd step, 1 reconstructor fwd step,
    2 reconstructor bwd step, 3 / 4 one launch of the persistent reconstructor fwd / bwd chain over the last T,
    5 / 6 one launch of the persistent decoder fwd / BPTT chain*/);
/* Bytes of the exchange blocks (h_t / dgates_t panels, stamped words) one launch of chain kernel `which` (3..6) writes
 * and reads back: implementation traffic, reported beside the algorithmic bytes. */
double recnet_chain_exchange_bytes(const recnet_handle* h, int32_t which);

#ifdef __cplusplus
}
#endif
#endif /* RECNET_HIP_H */
