// torch.ops.recnet.* — PyTorch-ROCm custom-op registration of the RecNet hot path (BASELINE
// north_star: "called from Python via PyTorch-ROCm custom ops").  A thin layer over the C ABI of librecnet_hip.so
// (include/recnet_hip.h): every op validates its tensors (TORCH_CHECK -> RuntimeError: dtype, shape, contiguity,
// residency), allocates its outputs through torch's caching allocator, takes the current HIP stream and makes exactly
// one C-ABI call.  No arithmetic happens here.  The engine handle (recnet_create) travels as an int.
//
// Paired forward / backward ops (autograd is wired in api.py with torch.autograd.Function over these ops):
//   forward_decoder / backward_decoder                  train.py:17-75 and its BPTT
//   forward_decoder_free                                train.py:46-51 (validation pass)
//   forward_reconstructor / backward_reconstructor      train.py:78-131 and its BPTT
//   train_step_fwd_bwd, train_step, optimizer_step      train.py:248-273
//   decoder_step, reconstructor_step                    Decoder.forward / *Reconstructor.forward (per-step API)
//   greedy_search, beam_search                          eval.py:19-120
//   beam_search_nbest, beam_select_rows                 N-best beam search on log-probabilities (no counterpart)
//   beam_search_nbest_constrained, beam_select_rows_constrained   the same with no-repeat n-grams, a minimum length, banned ids (section 12)
//   beam_search_nbest_diverse, beam_select_rows_diverse  the same in groups with a Hamming penalty between them (section 14)
//   sample_search, sample_rows                          sampling (no counterpart in the reference; loop shape of eval.py:19-33)
//   sample_search_nucleus, sample_rows_nucleus          the same with a nucleus (top-p) cut behind the top-k cut
//   score_captions                                      teacher-forced log-probabilities of given captions (train.py:25,45, eval mode)
//   reconstruction_error                                per-caption reconstruction error and the reconstruction (train.py:96-102 / :125-128, eval mode)
//   consensus_rows                                      n-gram consensus (minimum-Bayes-risk) utilities of hypotheses against a reference set (no counterpart; section 16)
//   ensemble_mix_rows, beam_search_nbest_ensemble, score_captions_ensemble   N-best beam search and scoring over several decoders (no counterpart; section 19)
//   sbs_select_rows, stochastic_beam_search, stochastic_beam_search_ensemble   stochastic beam search: sampled captions without replacement (no counterpart; section 21)
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <cmath>

#include "../../include/recnet_hip.h"

namespace {

recnet_handle* H(int64_t h) {
  TORCH_CHECK(h != 0, "recnet: null engine handle");
  return reinterpret_cast<recnet_handle*>(static_cast<intptr_t>(h));
}
void* stream() { return (void*)c10::hip::getCurrentHIPStream().stream(); }
void ok(int rc, const char* what) { TORCH_CHECK(rc == 0, "recnet::", what, " failed (code ", rc, "): ", recnet_last_error()); }
void chk(const at::Tensor& t, at::ScalarType ty, const char* name) {
  TORCH_CHECK(t.is_cuda(), "recnet: ", name, " must be a CUDA (HIP) tensor — there is no CPU fallback");
  TORCH_CHECK(t.scalar_type() == ty, "recnet: ", name, " has dtype ", t.scalar_type(), ", expected ", ty);
  TORCH_CHECK(t.is_contiguous(), "recnet: ", name, " must be contiguous");
}
const float* fptr(const c10::optional<at::Tensor>& t, const char* name) {
  if (!t.has_value() || !t->defined()) return nullptr;
  chk(*t, at::kFloat, name);
  return t->data_ptr<float>();
}
at::Tensor scalars_like(const at::Tensor& ref) { return at::zeros({8}, ref.options().dtype(at::kFloat)); }
int64_t dim(int64_t h, int which) { return recnet_dim(H(h), which); }
// Shapes come from the handle (recnet_dim), never from the caller's tensors: a wrong-shaped tensor is a RuntimeError,
// not an out-of-bounds device write.
void shape(const at::Tensor& t, std::initializer_list<int64_t> want, const char* name) {
  int64_t n = 1;
  for (auto w : want) n *= w;
  TORCH_CHECK(t.numel() == n, "recnet: ", name, " has ", t.numel(), " elements (sizes ", t.sizes(), "), the engine expects ",
              at::IntArrayRef(want.begin(), want.size()));
}
void chk_enc(int64_t h, const at::Tensor& enc) {
  chk(enc, at::kFloat, "encoder_outputs");
  TORCH_CHECK(enc.dim() == 3 && enc.size(0) == dim(h, RECNET_DIM_B) && enc.size(1) == dim(h, RECNET_DIM_F) && enc.size(2) == dim(h, RECNET_DIM_D),
              "recnet: encoder_outputs has sizes ", enc.sizes(), ", the engine expects [", dim(h, RECNET_DIM_B), ", ", dim(h, RECNET_DIM_F), ", ",
              dim(h, RECNET_DIM_D), "]");
}
void chk_targets(int64_t h, const at::Tensor& targets, int64_t T) {
  chk(targets, at::kLong, "targets");
  TORCH_CHECK(targets.dim() == 2 && targets.size(1) == dim(h, RECNET_DIM_B) && targets.size(0) >= T && T >= 1 && T <= dim(h, RECNET_DIM_TM),
              "recnet: targets has sizes ", targets.sizes(), ", the engine expects [>= T = ", T, " (<= ", dim(h, RECNET_DIM_TM), "), ",
              dim(h, RECNET_DIM_B), "]");
}
void chk_T(int64_t h, int64_t T) { TORCH_CHECK(T >= 1 && T <= dim(h, RECNET_DIM_TM), "recnet: T = ", T, " outside [1, ", dim(h, RECNET_DIM_TM), "]"); }

// ---------------------------------------------------------------- sequence level
std::tuple<at::Tensor, at::Tensor, at::Tensor> forward_decoder(int64_t h, const at::Tensor& enc, const at::Tensor& targets, int64_t T,
                                                               const at::Tensor& step_weight, bool train, int64_t seed) {
  chk_enc(h, enc); chk_targets(h, targets, T); chk(step_weight, at::kFloat, "step_weight");
  TORCH_CHECK(step_weight.numel() == T, "recnet: step_weight must have T entries");
  auto sc = scalars_like(enc);
  auto hid = at::empty({T, 1, enc.size(0), recnet_dim(H(h), RECNET_DIM_H)}, enc.options());
  ok(recnet_forward_decoder(H(h), enc.data_ptr<float>(), targets.data_ptr<int64_t>(), (int32_t)T, step_weight.data_ptr<float>(),
                            train, (uint32_t)seed, hid.data_ptr<float>(), (recnet_scalars*)sc.data_ptr<float>(), stream()), "forward_decoder");
  return {sc.select(0, 2).clone(), hid, sc};
}
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> forward_decoder_free(int64_t h, const at::Tensor& enc, const at::Tensor& targets,
                                                                                int64_t T, const at::Tensor& step_weight, bool train,
                                                                                int64_t seed) {
  chk_enc(h, enc); chk_targets(h, targets, T); chk(step_weight, at::kFloat, "step_weight");
  TORCH_CHECK(step_weight.numel() == T, "recnet: step_weight must have T entries");
  auto sc = scalars_like(enc);
  auto hid = at::empty({T, 1, enc.size(0), recnet_dim(H(h), RECNET_DIM_H)}, enc.options());
  auto idx = at::empty({T, enc.size(0)}, targets.options());
  ok(recnet_forward_decoder_free(H(h), enc.data_ptr<float>(), targets.data_ptr<int64_t>(), (int32_t)T, step_weight.data_ptr<float>(),
                                 train, (uint32_t)seed, hid.data_ptr<float>(), idx.data_ptr<int64_t>(),
                                 (recnet_scalars*)sc.data_ptr<float>(), stream()), "forward_decoder_free");
  return {sc.select(0, 2).clone(), hid, idx, sc};
}
void backward_decoder(int64_t h, const at::Tensor& enc, const at::Tensor& targets, const c10::optional<at::Tensor>& dhiddens,
                      double grad_scale) {
  chk_enc(h, enc); chk(targets, at::kLong, "targets");
  TORCH_CHECK(targets.dim() == 2 && targets.size(1) == dim(h, RECNET_DIM_B), "recnet: targets must be [Tm, B]");
  if (dhiddens.has_value() && dhiddens->defined())
    TORCH_CHECK(dhiddens->numel() % (dim(h, RECNET_DIM_B) * dim(h, RECNET_DIM_H)) == 0 && dhiddens->numel() > 0 &&
                    dhiddens->numel() / (dim(h, RECNET_DIM_B) * dim(h, RECNET_DIM_H)) <= dim(h, RECNET_DIM_TM),
                "recnet: dhiddens must be [T,1,B,H] of the forward pass, got ", dhiddens->sizes());
  ok(recnet_backward_decoder(H(h), enc.data_ptr<float>(), targets.data_ptr<int64_t>(), fptr(dhiddens, "dhiddens"), (float)grad_scale,
                             stream()), "backward_decoder");
}
std::tuple<at::Tensor, at::Tensor> forward_reconstructor(int64_t h, const at::Tensor& enc, const c10::optional<at::Tensor>& hiddens,
                                                         int64_t T, bool train, int64_t seed) {
  chk_enc(h, enc); chk_T(h, T);
  if (hiddens.has_value() && hiddens->defined()) shape(*hiddens, {T, 1, dim(h, RECNET_DIM_B), dim(h, RECNET_DIM_H)}, "decoder_hiddens");
  auto sc = scalars_like(enc);
  ok(recnet_forward_reconstructor(H(h), enc.data_ptr<float>(), fptr(hiddens, "decoder_hiddens"), (int32_t)T, train, (uint32_t)seed,
                                  (recnet_scalars*)sc.data_ptr<float>(), stream()), "forward_reconstructor");
  return {sc.select(0, 5).clone(), sc};
}
at::Tensor backward_reconstructor(int64_t h, const at::Tensor& enc, int64_t T, double grad_scale) {
  chk_enc(h, enc); chk_T(h, T);
  auto dh = at::empty({T, 1, dim(h, RECNET_DIM_B), dim(h, RECNET_DIM_H)}, enc.options());
  ok(recnet_backward_reconstructor(H(h), enc.data_ptr<float>(), (float)grad_scale, dh.data_ptr<float>(), stream()), "backward_reconstructor");
  return dh;
}
void add_reg_grad(int64_t h, int64_t which, double grad_scale) { ok(recnet_add_reg_grad(H(h), (int32_t)which, (float)grad_scale, stream()), "add_reg_grad"); }

// ---------------------------------------------------------------- fused step (train.py:248-273)
at::Tensor train_step_fwd_bwd(int64_t h, const at::Tensor& enc, const at::Tensor& targets, int64_t T, const at::Tensor& step_weight,
                              int64_t seed) {
  chk_enc(h, enc); chk_targets(h, targets, T); chk(step_weight, at::kFloat, "step_weight");
  TORCH_CHECK(step_weight.numel() == T, "recnet: step_weight must have T entries");
  auto sc = scalars_like(enc);
  ok(recnet_train_step_fwd_bwd(H(h), enc.data_ptr<float>(), targets.data_ptr<int64_t>(), (int32_t)T, step_weight.data_ptr<float>(),
                               (uint32_t)seed, (recnet_scalars*)sc.data_ptr<float>(), stream()), "train_step_fwd_bwd");
  return sc;
}
at::Tensor train_step(int64_t h, const at::Tensor& enc, const at::Tensor& targets, int64_t T, const at::Tensor& step_weight, int64_t seed,
                      int64_t step) {
  chk_enc(h, enc); chk_targets(h, targets, T); chk(step_weight, at::kFloat, "step_weight");
  TORCH_CHECK(step_weight.numel() == T, "recnet: step_weight must have T entries");
  auto sc = scalars_like(enc);
  ok(recnet_train_step(H(h), enc.data_ptr<float>(), targets.data_ptr<int64_t>(), (int32_t)T, step_weight.data_ptr<float>(), (uint32_t)seed,
                       (int32_t)step, (recnet_scalars*)sc.data_ptr<float>(), stream()), "train_step");
  return sc;
}
void optimizer_step(int64_t h, int64_t step, int64_t flags) { ok(recnet_optimizer_step(H(h), (int32_t)step, (int32_t)flags, nullptr, stream()), "optimizer_step"); }
at::Tensor clip_grad_norm(int64_t h, int64_t which, double max_norm, const at::Tensor& like) {
  auto out = at::empty({1}, like.options().dtype(at::kFloat));
  ok(recnet_clip_grad_norm(H(h), (int32_t)which, (float)max_norm, out.data_ptr<float>(), stream()), "clip_grad_norm");
  return out;
}

// ---------------------------------------------------------------- per-step API
std::tuple<at::Tensor, at::Tensor, at::Tensor> decoder_step(int64_t h, const at::Tensor& tokens, const c10::optional<at::Tensor>& h_in,
                                                            const c10::optional<at::Tensor>& c_in, const c10::optional<at::Tensor>& enc,
                                                            bool train, int64_t seed, int64_t t) {
  chk(tokens, at::kLong, "input");
  const int64_t B = dim(h, RECNET_DIM_B), Hd = dim(h, RECNET_DIM_H);
  shape(tokens, {1, B}, "input");
  if (h_in.has_value() && h_in->defined()) shape(*h_in, {B, Hd}, "hidden h");
  if (c_in.has_value() && c_in->defined()) shape(*c_in, {B, Hd}, "hidden c");
  if (enc.has_value() && enc->defined()) chk_enc(h, *enc);
  auto opt = tokens.options().dtype(at::kFloat);
  auto logits = at::empty({B, recnet_dim(H(h), RECNET_DIM_V)}, opt);
  auto ho = at::empty({B, recnet_dim(H(h), RECNET_DIM_H)}, opt), co = at::empty_like(ho);
  ok(recnet_decoder_step(H(h), tokens.data_ptr<int64_t>(), fptr(h_in, "hidden h"), fptr(c_in, "hidden c"), fptr(enc, "encoder_outputs"),
                         logits.data_ptr<float>(), ho.data_ptr<float>(), co.data_ptr<float>(), train, (uint32_t)seed, (int32_t)t, stream()),
     "decoder_step");
  return {logits, ho, co};
}
std::tuple<at::Tensor, at::Tensor, at::Tensor> reconstructor_step(int64_t h, const c10::optional<at::Tensor>& input, const at::Tensor& hr_in,
                                                                  const c10::optional<at::Tensor>& cr_in,
                                                                  const c10::optional<at::Tensor>& decoder_hiddens, int64_t T, bool train,
                                                                  int64_t seed, int64_t t) {
  chk(hr_in, at::kFloat, "hidden hr");
  const int64_t B = dim(h, RECNET_DIM_B), R = dim(h, RECNET_DIM_R), Hd = dim(h, RECNET_DIM_H);
  chk_T(h, T);
  shape(hr_in, {B, R}, "hidden hr");
  if (cr_in.has_value() && cr_in->defined()) shape(*cr_in, {B, R}, "hidden cr");
  if (input.has_value() && input->defined()) shape(*input, {B, Hd}, "input");
  if (decoder_hiddens.has_value() && decoder_hiddens->defined()) shape(*decoder_hiddens, {T, 1, B, Hd}, "decoder_hiddens");
  auto out = at::empty({B, R}, hr_in.options()), ho = at::empty({B, R}, hr_in.options()), co = at::empty({B, R}, hr_in.options());
  ok(recnet_reconstructor_step(H(h), fptr(input, "input"), hr_in.data_ptr<float>(), fptr(cr_in, "hidden cr"),
                               fptr(decoder_hiddens, "decoder_hiddens"), (int32_t)T, out.data_ptr<float>(), ho.data_ptr<float>(),
                               co.data_ptr<float>(), train, (uint32_t)seed, (int32_t)t, stream()), "reconstructor_step");
  return {out, ho, co};
}

// ---------------------------------------------------------------- search (eval.py:19-120)
std::tuple<at::Tensor, at::Tensor> greedy_search(int64_t h, const at::Tensor& enc) {
  chk_enc(h, enc);
  auto toks = at::zeros({recnet_dim(H(h), RECNET_DIM_TM), enc.size(0)}, enc.options().dtype(at::kLong));
  auto n = at::zeros({1}, enc.options().dtype(at::kInt));
  ok(recnet_greedy_search(H(h), enc.data_ptr<float>(), toks.data_ptr<int64_t>(), n.data_ptr<int32_t>(), stream()), "greedy_search");
  return {toks, n};
}
std::tuple<at::Tensor, at::Tensor> beam_search(int64_t h, const at::Tensor& enc, int64_t beam_width) {
  chk_enc(h, enc);
  auto best = at::zeros({recnet_dim(H(h), RECNET_DIM_TM), enc.size(0)}, enc.options().dtype(at::kLong));
  auto n = at::zeros({1}, enc.options().dtype(at::kInt));
  ok(recnet_beam_search(H(h), enc.data_ptr<float>(), (int32_t)beam_width, best.data_ptr<int64_t>(), n.data_ptr<int32_t>(), stream()), "beam_search");
  return {best, n};
}
// ---- sampling: one implementation per shape of call; top_p null: the form without a nucleus, which launches the kernels it always
// had (n_allowed comes back undefined), else the nucleus form: one more cut and one more output, the size of the set every token
// was drawn from
static std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> sample_search_impl(int64_t h, const at::Tensor& enc, double temperature,
                                                                                     int64_t top_k, const double* top_p, int64_t seed) {
  chk_enc(h, enc);
  const int64_t Tm = recnet_dim(H(h), RECNET_DIM_TM), B = enc.size(0);
  auto toks = at::zeros({Tm, B}, enc.options().dtype(at::kLong));
  auto lps = at::zeros({Tm, B}, enc.options());
  at::Tensor na;
  if (top_p) na = at::zeros({Tm, B}, enc.options().dtype(at::kInt));
  auto n = at::zeros({1}, enc.options().dtype(at::kInt));
  TORCH_CHECK(top_k >= INT32_MIN && top_k <= INT32_MAX, "recnet: top_k out of range");
  if (top_p)
    ok(recnet_sample_search_nucleus(H(h), enc.data_ptr<float>(), (float)temperature, (int32_t)top_k, (float)*top_p, (uint32_t)seed,
                                    toks.data_ptr<int64_t>(), lps.data_ptr<float>(), na.data_ptr<int32_t>(), n.data_ptr<int32_t>(), stream()), "sample_search_nucleus");
  else
    ok(recnet_sample_search(H(h), enc.data_ptr<float>(), (float)temperature, (int32_t)top_k, (uint32_t)seed, toks.data_ptr<int64_t>(),
                            lps.data_ptr<float>(), n.data_ptr<int32_t>(), stream()), "sample_search");
  return {toks, lps, na, n};
}
static std::tuple<at::Tensor, at::Tensor, at::Tensor> sample_rows_impl(int64_t h, const at::Tensor& logits, double temperature, int64_t top_k,
                                                                       const double* top_p, int64_t seed, int64_t t) {
  chk(logits, at::kFloat, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.size(0) >= 1 && logits.size(1) >= 1 && logits.size(0) <= INT32_MAX && logits.size(1) <= INT32_MAX,
              "recnet: logits must be [rows, V], got ", logits.sizes());
  TORCH_CHECK(top_k >= INT32_MIN && top_k <= INT32_MAX && t >= 0 && t <= INT32_MAX, "recnet: top_k / t out of range");
  const int32_t rows = (int32_t)logits.size(0), V = (int32_t)logits.size(1);
  auto toks = at::empty({rows}, logits.options().dtype(at::kLong));
  auto lps = at::empty({rows}, logits.options());
  at::Tensor na;
  if (top_p) na = at::empty({rows}, logits.options().dtype(at::kInt));
  if (top_p)
    ok(recnet_sample_rows_nucleus(H(h), logits.data_ptr<float>(), rows, V, (float)temperature, (int32_t)top_k, (float)*top_p, (uint32_t)seed,
                                  (int32_t)t, toks.data_ptr<int64_t>(), lps.data_ptr<float>(), na.data_ptr<int32_t>(), stream()), "sample_rows_nucleus");
  else
    ok(recnet_sample_rows(H(h), logits.data_ptr<float>(), rows, V, (float)temperature, (int32_t)top_k, (uint32_t)seed, (int32_t)t,
                          toks.data_ptr<int64_t>(), lps.data_ptr<float>(), stream()), "sample_rows");
  return {toks, lps, na};
}
std::tuple<at::Tensor, at::Tensor, at::Tensor> sample_search(int64_t h, const at::Tensor& enc, double temperature, int64_t top_k, int64_t seed) {
  auto [toks, lps, na, n] = sample_search_impl(h, enc, temperature, top_k, nullptr, seed);
  return {toks, lps, n};
}
std::tuple<at::Tensor, at::Tensor> sample_rows(int64_t h, const at::Tensor& logits, double temperature, int64_t top_k, int64_t seed, int64_t t) {
  auto [toks, lps, na] = sample_rows_impl(h, logits, temperature, top_k, nullptr, seed, t);
  return {toks, lps};
}
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> sample_search_nucleus(int64_t h, const at::Tensor& enc, double temperature, int64_t top_k,
                                                                                 double top_p, int64_t seed) {
  return sample_search_impl(h, enc, temperature, top_k, &top_p, seed);
}
std::tuple<at::Tensor, at::Tensor, at::Tensor> sample_rows_nucleus(int64_t h, const at::Tensor& logits, double temperature, int64_t top_k,
                                                                   double top_p, int64_t seed, int64_t t) {
  return sample_rows_impl(h, logits, temperature, top_k, &top_p, seed, t);
}
// ---- N-best beam search on log-probabilities, its constrained forms (section 12: no-repeat n-grams, a minimum
// length, banned ids, which travel to the library as a host array) and its diverse forms (section 14: the constrained forms in
// n_groups groups with a penalty between them).  One implementation of the selection and one of the search; bans / groups null: the
// form without them, which makes the library call of its own name.
struct Bans { int64_t no_repeat_ngram, min_length; at::IntArrayRef banned; };
struct Groups { int64_t n; double penalty; };
static std::vector<int32_t> ban_ids(const Bans* b) {
  std::vector<int32_t> ids;
  if (!b) return ids;
  TORCH_CHECK(b->no_repeat_ngram >= 0 && b->no_repeat_ngram <= INT32_MAX && b->min_length >= 0 && b->min_length <= INT32_MAX,
              "recnet: no_repeat_ngram / min_length out of range");
  TORCH_CHECK(b->banned.size() <= 16, "recnet: at most 16 banned tokens, got ", b->banned.size());
  for (const int64_t v : b->banned) {
    TORCH_CHECK(v >= 0 && v <= INT32_MAX, "recnet: banned token out of range: ", v);
    ids.push_back((int32_t)v);
  }
  return ids;
}
static void chk_groups(int64_t beam_width, const Groups* g) {
  if (!g) return;
  TORCH_CHECK(g->n >= 1 && beam_width % g->n == 0, "recnet: n_groups must be at least 1 and divide beam_width, got ", g->n);
  TORCH_CHECK(std::isfinite(g->penalty) && g->penalty >= 0.0, "recnet: diversity_penalty must be finite and >= 0, got ", g->penalty);
}
// logits [nb, rows, V], cum [nb, rows] float, finished [nb, rows] int32 -> vals [rows, beam_width], idx [rows, beam_width] int32;
// with bans: hist [nb, rows, Tm] int64 (undefined: allowed when no_repeat_ngram = 0: null, and a Tm no step reaches) and the step t
static std::tuple<at::Tensor, at::Tensor> select_rows_impl(int64_t h, const at::Tensor& logits, const at::Tensor& cum, const at::Tensor& finished,
                                                           int64_t beam_width, const c10::optional<at::Tensor>* hist, int64_t t,
                                                           const Bans* b, const Groups* g) {
  chk(logits, at::kFloat, "logits"); chk(cum, at::kFloat, "cum"); chk(finished, at::kInt, "finished");
  TORCH_CHECK(logits.dim() == 3 && logits.size(0) >= 1 && logits.size(1) >= 1 && logits.size(2) >= 1 && logits.size(1) <= INT32_MAX &&
              logits.size(2) <= INT32_MAX && logits.size(0) <= 8, "recnet: logits must be [nb <= 8, rows, V], got ", logits.sizes());
  shape(cum, {logits.size(0), logits.size(1)}, "cum"); shape(finished, {logits.size(0), logits.size(1)}, "finished");
  TORCH_CHECK(beam_width >= 1 && beam_width <= 8 && beam_width <= logits.size(2), "recnet: beam_width must be in [1, min(8, V)], got ", beam_width);
  chk_groups(beam_width, g);
  if (g) TORCH_CHECK(logits.size(0) == 1 || logits.size(0) == beam_width, "recnet: nb must be 1 or beam_width, got ", logits.size(0));
  if (b) TORCH_CHECK(t >= 0 && t < INT32_MAX, "recnet: t out of range");
  const auto ids = ban_ids(b);
  int64_t Tm = INT32_MAX;            // (no hist: only min_length / the static bans can be on, and they read no history)
  const int64_t* hp = nullptr;
  if (b && hist->has_value() && (*hist)->defined()) {
    const at::Tensor& hs = **hist;
    chk(hs, at::kLong, "hist");
    TORCH_CHECK(hs.dim() == 3 && hs.size(0) == logits.size(0) && hs.size(1) == logits.size(1) && hs.size(2) >= 1 && hs.size(2) <= INT32_MAX,
                "recnet: hist must be [nb, rows, Tm], got ", hs.sizes());
    Tm = hs.size(2); hp = hs.data_ptr<int64_t>();
  }
  auto vals = at::empty({logits.size(1), beam_width}, logits.options());
  auto idx = at::empty({logits.size(1), beam_width}, logits.options().dtype(at::kInt));
  const float* x = logits.data_ptr<float>(); const float* c = cum.data_ptr<float>(); const int32_t* f = finished.data_ptr<int32_t>();
  const int32_t nb = (int32_t)logits.size(0), rows = (int32_t)logits.size(1), V = (int32_t)logits.size(2), bw = (int32_t)beam_width;
  if (g)
    ok(recnet_beam_select_rows_diverse(H(h), x, c, f, hp, nb, rows, V, (int32_t)Tm, (int32_t)t, bw, (int32_t)g->n, (float)g->penalty,
                                       (int32_t)b->no_repeat_ngram, (int32_t)b->min_length, ids.data(), (int32_t)ids.size(),
                                       vals.data_ptr<float>(), idx.data_ptr<int32_t>(), stream()), "beam_select_rows_diverse");
  else if (b)
    ok(recnet_beam_select_rows_constrained(H(h), x, c, f, hp, nb, rows, V, (int32_t)Tm, (int32_t)t, bw, (int32_t)b->no_repeat_ngram,
                                           (int32_t)b->min_length, ids.data(), (int32_t)ids.size(), vals.data_ptr<float>(),
                                           idx.data_ptr<int32_t>(), stream()), "beam_select_rows_constrained");
  else
    ok(recnet_beam_select_rows(H(h), x, c, f, nb, rows, V, bw, vals.data_ptr<float>(), idx.data_ptr<int32_t>(), stream()), "beam_select_rows");
  return {vals, idx};
}
// tokens [beam_width, Tm, B] rank-major, cum / score [beam_width, B] float, len [beam_width, B] int32, n_steps [1] int32 and, with
// groups, group [beam_width, B] int32, the group of each returned rank (undefined without)
// (the width is checked here before the outputs are allocated and zeroed; length_alpha by the library, behind those fills)
using NbestOut = std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor>;
using NbestGroupOut = std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor>;
static NbestGroupOut nbest_impl(int64_t h, const at::Tensor& enc, int64_t beam_width, double length_alpha, const Bans* b, const Groups* g) {
  chk_enc(h, enc);
  TORCH_CHECK(beam_width >= 1 && beam_width <= 8 && beam_width <= dim(h, RECNET_DIM_V), "recnet: beam_width must be in [1, min(8, V)], got ", beam_width);
  chk_groups(beam_width, g);
  const auto ids = ban_ids(b);
  const int64_t B = enc.size(0);
  auto toks = at::zeros({beam_width, recnet_dim(H(h), RECNET_DIM_TM), B}, enc.options().dtype(at::kLong));
  auto cum = at::zeros({beam_width, B}, enc.options()), score = at::zeros({beam_width, B}, enc.options());
  auto len = at::zeros({beam_width, B}, enc.options().dtype(at::kInt));
  auto n = at::zeros({1}, enc.options().dtype(at::kInt));
  at::Tensor group;
  if (g) group = at::zeros({beam_width, B}, enc.options().dtype(at::kInt));
  const float* e = enc.data_ptr<float>(); const int32_t bw = (int32_t)beam_width; const float la = (float)length_alpha;
  int64_t* tp = toks.data_ptr<int64_t>(); float* cp = cum.data_ptr<float>(); int32_t* lp = len.data_ptr<int32_t>();
  float* sp = score.data_ptr<float>(); int32_t* np = n.data_ptr<int32_t>();
  if (g)
    ok(recnet_beam_search_nbest_diverse(H(h), e, bw, la, (int32_t)g->n, (float)g->penalty, (int32_t)b->no_repeat_ngram, (int32_t)b->min_length,
                                        ids.data(), (int32_t)ids.size(), tp, cp, lp, sp, group.data_ptr<int32_t>(), np, stream()), "beam_search_nbest_diverse");
  else if (b)
    ok(recnet_beam_search_nbest_constrained(H(h), e, bw, la, (int32_t)b->no_repeat_ngram, (int32_t)b->min_length, ids.data(), (int32_t)ids.size(),
                                            tp, cp, lp, sp, np, stream()), "beam_search_nbest_constrained");
  else
    ok(recnet_beam_search_nbest(H(h), e, bw, la, tp, cp, lp, sp, np, stream()), "beam_search_nbest");
  return {toks, cum, len, score, group, n};
}
static NbestOut without_group(const NbestGroupOut& o) {
  return {std::get<0>(o), std::get<1>(o), std::get<2>(o), std::get<3>(o), std::get<5>(o)};
}
std::tuple<at::Tensor, at::Tensor> beam_select_rows(int64_t h, const at::Tensor& logits, const at::Tensor& cum, const at::Tensor& finished,
                                                    int64_t beam_width) {
  return select_rows_impl(h, logits, cum, finished, beam_width, nullptr, 0, nullptr, nullptr);
}
std::tuple<at::Tensor, at::Tensor> beam_select_rows_constrained(int64_t h, const at::Tensor& logits, const at::Tensor& cum,
                                                                const at::Tensor& finished, const c10::optional<at::Tensor>& hist, int64_t t,
                                                                int64_t beam_width, int64_t no_repeat_ngram, int64_t min_length,
                                                                at::IntArrayRef banned) {
  const Bans b{no_repeat_ngram, min_length, banned};
  return select_rows_impl(h, logits, cum, finished, beam_width, &hist, t, &b, nullptr);
}
std::tuple<at::Tensor, at::Tensor> beam_select_rows_diverse(int64_t h, const at::Tensor& logits, const at::Tensor& cum,
                                                            const at::Tensor& finished, const c10::optional<at::Tensor>& hist, int64_t t,
                                                            int64_t beam_width, int64_t n_groups, double diversity_penalty,
                                                            int64_t no_repeat_ngram, int64_t min_length, at::IntArrayRef banned) {
  const Bans b{no_repeat_ngram, min_length, banned};
  const Groups g{n_groups, diversity_penalty};
  return select_rows_impl(h, logits, cum, finished, beam_width, &hist, t, &b, &g);
}
NbestOut beam_search_nbest(int64_t h, const at::Tensor& enc, int64_t beam_width, double length_alpha) {
  return without_group(nbest_impl(h, enc, beam_width, length_alpha, nullptr, nullptr));
}
NbestOut beam_search_nbest_constrained(int64_t h, const at::Tensor& enc, int64_t beam_width, double length_alpha, int64_t no_repeat_ngram,
                                       int64_t min_length, at::IntArrayRef banned) {
  const Bans b{no_repeat_ngram, min_length, banned};
  return without_group(nbest_impl(h, enc, beam_width, length_alpha, &b, nullptr));
}
NbestGroupOut beam_search_nbest_diverse(
    int64_t h, const at::Tensor& enc, int64_t beam_width, double length_alpha, int64_t n_groups, double diversity_penalty,
    int64_t no_repeat_ngram, int64_t min_length, at::IntArrayRef banned) {
  const Bans b{no_repeat_ngram, min_length, banned};
  const Groups g{n_groups, diversity_penalty};
  return nbest_impl(h, enc, beam_width, length_alpha, &b, &g);
}
// tokens [T, B] with every entry in [0, V): the caller's duty (search.score_captions checks it)
std::tuple<at::Tensor, at::Tensor, at::Tensor> score_captions(int64_t h, const c10::optional<at::Tensor>& enc, const at::Tensor& tokens,
                                                              double temperature) {
  if (enc.has_value() && enc->defined()) chk_enc(h, *enc);
  chk(tokens, at::kLong, "tokens");
  TORCH_CHECK(tokens.dim() == 2 && tokens.size(1) == dim(h, RECNET_DIM_B), "recnet: tokens has sizes ", tokens.sizes(), ", the engine expects [T, ",
              dim(h, RECNET_DIM_B), "]");
  const int64_t T = tokens.size(0), B = tokens.size(1);
  TORCH_CHECK(T <= INT32_MAX, "recnet: T out of range");
  auto lps = at::zeros({T, B}, tokens.options().dtype(at::kFloat));
  auto cap = at::zeros({B}, tokens.options().dtype(at::kFloat));
  auto len = at::zeros({B}, tokens.options().dtype(at::kInt));
  ok(recnet_score_captions(H(h), fptr(enc, "encoder_outputs"), tokens.data_ptr<int64_t>(), (int32_t)T, (float)temperature,
                           lps.data_ptr<float>(), cap.data_ptr<float>(), len.data_ptr<int32_t>(), stream()), "score_captions");
  return {lps, cap, len};
}
// Exactly one of tokens [T, B] (every entry in [0, V): the caller's duty, search.reconstruction_errors checks it) and hiddens
// [T, 1, B, H].  recon: global [B, R], local [B, F, D]; an empty tensor when it is not asked for.
std::tuple<at::Tensor, at::Tensor> reconstruction_error(int64_t h, const at::Tensor& enc, const c10::optional<at::Tensor>& tokens,
                                                        const c10::optional<at::Tensor>& hiddens, bool want_recon) {
  chk_enc(h, enc);
  const bool has_t = tokens.has_value() && tokens->defined(), has_h = hiddens.has_value() && hiddens->defined();
  TORCH_CHECK(has_t != has_h, "recnet: exactly one of tokens / hiddens must be given");
  const int64_t B = dim(h, RECNET_DIM_B), Hd = dim(h, RECNET_DIM_H), R = dim(h, RECNET_DIM_R);
  TORCH_CHECK(R > 0, "recnet: the engine was created without a reconstructor");
  int64_t T = 0;
  if (has_t) {
    chk(*tokens, at::kLong, "tokens");
    TORCH_CHECK(tokens->dim() == 2 && tokens->size(1) == B, "recnet: tokens has sizes ", tokens->sizes(), ", the engine expects [T, ", B, "]");
    T = tokens->size(0);
  } else {
    chk(*hiddens, at::kFloat, "decoder_hiddens");
    TORCH_CHECK(hiddens->dim() == 4 && hiddens->size(1) == 1 && hiddens->size(2) == B && hiddens->size(3) == Hd,
                "recnet: decoder_hiddens has sizes ", hiddens->sizes(), ", the engine expects [T, 1, ", B, ", ", Hd, "]");
    T = hiddens->size(0);
  }
  chk_T(h, T);
  auto err = at::zeros({B}, enc.options());
  const bool local = dim(h, RECNET_DIM_RA) > 0;      // recnet_create: a local reconstructor needs RA > 0, every other kind holds RA = 0
  at::Tensor recon = !want_recon ? at::empty({0}, enc.options())
                                 : (local ? at::zeros({B, dim(h, RECNET_DIM_F), dim(h, RECNET_DIM_D)}, enc.options()) : at::zeros({B, R}, enc.options()));
  ok(recnet_reconstruction_error(H(h), enc.data_ptr<float>(), has_t ? tokens->data_ptr<int64_t>() : nullptr,
                                 has_h ? hiddens->data_ptr<float>() : nullptr, (int32_t)T, err.data_ptr<float>(),
                                 want_recon ? recon.data_ptr<float>() : nullptr, stream()), "reconstruction_error");
  return {err, recon};
}
// ---- ensemble decoding.  handle: the engine handle of member 0, like every op's leading argument;
// more_handles: those of members 1 .. M - 1 (M <= 8; empty: an ensemble of one); weights: one positive finite number per member,
// member 0 first (the library normalises them); mode: RECNET_ENS_ARITHMETIC / RECNET_ENS_GEOMETRIC.  Shapes come from member 0;
// that the members agree is the library's check.
static std::vector<recnet_handle*> ens_handles(int64_t handle, at::IntArrayRef more_handles) {
  TORCH_CHECK(more_handles.size() <= 7, "recnet: an ensemble has between 1 and 8 members, got ", more_handles.size() + 1);
  std::vector<recnet_handle*> hs{H(handle)};
  for (const int64_t h : more_handles) hs.push_back(H(h));
  return hs;
}
static std::vector<float> ens_weights(at::ArrayRef<double> weights, size_t M) {
  TORCH_CHECK(weights.size() == M, "recnet: ", weights.size(), " weights for ", M, " ensemble members");
  return std::vector<float>(weights.begin(), weights.end());
}
// logits: M tensors [rows, V] float -> y [rows, V]; in_place: y is logits[0] itself (it is returned)
at::Tensor ensemble_mix_rows(int64_t h, at::TensorList logits, at::ArrayRef<double> weights, int64_t mode, bool in_place) {
  TORCH_CHECK(logits.size() >= 1 && logits.size() <= 8, "recnet: an ensemble has between 1 and 8 members, got ", logits.size());
  const auto w = ens_weights(weights, logits.size());
  std::vector<const float*> xs;
  for (const at::Tensor& x : logits) {
    chk(x, at::kFloat, "logits");
    TORCH_CHECK(x.dim() == 2 && x.sizes() == logits[0].sizes() && x.size(0) >= 1 && x.size(1) >= 1 && x.size(0) <= INT32_MAX && x.size(1) <= INT32_MAX,
                "recnet: logits must be M tensors [rows, V] of one shape, got ", x.sizes());
    xs.push_back(x.data_ptr<float>());
  }
  at::Tensor y = in_place ? logits[0] : at::empty_like(logits[0]);
  ok(recnet_ensemble_mix_rows(H(h), xs.data(), (int32_t)xs.size(), w.data(), (int32_t)mode, (int32_t)logits[0].size(0), (int32_t)logits[0].size(1),
                              y.data_ptr<float>(), stream()), "ensemble_mix_rows");
  return y;
}
NbestGroupOut beam_search_nbest_ensemble(int64_t h, at::IntArrayRef more_handles, at::ArrayRef<double> weights, int64_t mode, const at::Tensor& enc,
                                         int64_t beam_width, double length_alpha, int64_t n_groups, double diversity_penalty,
                                         int64_t no_repeat_ngram, int64_t min_length, at::IntArrayRef banned) {
  const auto hs = ens_handles(h, more_handles);
  const auto w = ens_weights(weights, hs.size());
  chk_enc(h, enc);
  TORCH_CHECK(beam_width >= 1 && beam_width <= 8 && beam_width <= dim(h, RECNET_DIM_V), "recnet: beam_width must be in [1, min(8, V)], got ", beam_width);
  const Bans b{no_repeat_ngram, min_length, banned};
  const Groups g{n_groups, diversity_penalty};
  chk_groups(beam_width, &g);
  const auto ids = ban_ids(&b);
  const int64_t B = enc.size(0);
  auto toks = at::zeros({beam_width, dim(h, RECNET_DIM_TM), B}, enc.options().dtype(at::kLong));
  auto cum = at::zeros({beam_width, B}, enc.options()), score = at::zeros({beam_width, B}, enc.options());
  auto len = at::zeros({beam_width, B}, enc.options().dtype(at::kInt)), group = at::zeros({beam_width, B}, enc.options().dtype(at::kInt));
  auto n = at::zeros({1}, enc.options().dtype(at::kInt));
  ok(recnet_beam_search_nbest_ensemble(hs.data(), (int32_t)hs.size(), w.data(), (int32_t)mode, enc.data_ptr<float>(), (int32_t)beam_width,
                                       (float)length_alpha, (int32_t)n_groups, (float)diversity_penalty, (int32_t)no_repeat_ngram,
                                       (int32_t)min_length, ids.data(), (int32_t)ids.size(), toks.data_ptr<int64_t>(), cum.data_ptr<float>(),
                                       len.data_ptr<int32_t>(), score.data_ptr<float>(), group.data_ptr<int32_t>(), n.data_ptr<int32_t>(), stream()),
     "beam_search_nbest_ensemble");
  return {toks, cum, len, score, group, n};
}
std::tuple<at::Tensor, at::Tensor, at::Tensor> score_captions_ensemble(int64_t h, at::IntArrayRef more_handles, at::ArrayRef<double> weights, int64_t mode,
                                                                       const c10::optional<at::Tensor>& enc, const at::Tensor& tokens) {
  const auto hs = ens_handles(h, more_handles);
  const auto w = ens_weights(weights, hs.size());
  if (enc.has_value() && enc->defined()) chk_enc(h, *enc);
  chk(tokens, at::kLong, "tokens");
  TORCH_CHECK(tokens.dim() == 2 && tokens.size(1) == dim(h, RECNET_DIM_B), "recnet: tokens has sizes ", tokens.sizes(), ", the engine expects [T, ",
              dim(h, RECNET_DIM_B), "]");
  const int64_t T = tokens.size(0), B = tokens.size(1);
  TORCH_CHECK(T <= INT32_MAX, "recnet: T out of range");
  auto lps = at::zeros({T, B}, tokens.options().dtype(at::kFloat));
  auto cap = at::zeros({B}, tokens.options().dtype(at::kFloat));
  auto len = at::zeros({B}, tokens.options().dtype(at::kInt));
  ok(recnet_score_captions_ensemble(hs.data(), (int32_t)hs.size(), w.data(), (int32_t)mode, fptr(enc, "encoder_outputs"),
                                    tokens.data_ptr<int64_t>(), (int32_t)T, lps.data_ptr<float>(), cap.data_ptr<float>(), len.data_ptr<int32_t>(),
                                    stream()), "score_captions_ensemble");
  return {lps, cap, len};
}
// ---- stochastic beam search.  logits [nb, rows, V], cum / gum [nb, rows] float, finished [nb, rows] int32 ->
// vals (phi), gum_out (G) [rows, beam_width] float, idx [rows, beam_width] int32
std::tuple<at::Tensor, at::Tensor, at::Tensor> sbs_select_rows(int64_t h, const at::Tensor& logits, const at::Tensor& cum, const at::Tensor& gum,
                                                               const at::Tensor& finished, int64_t beam_width, double temperature, int64_t seed,
                                                               int64_t t) {
  chk(logits, at::kFloat, "logits"); chk(cum, at::kFloat, "cum"); chk(gum, at::kFloat, "gum"); chk(finished, at::kInt, "finished");
  TORCH_CHECK(logits.dim() == 3 && logits.size(0) >= 1 && logits.size(1) >= 1 && logits.size(2) >= 1 && logits.size(1) <= INT32_MAX &&
              logits.size(2) <= INT32_MAX && logits.size(0) <= 8, "recnet: logits must be [nb <= 8, rows, V], got ", logits.sizes());
  shape(cum, {logits.size(0), logits.size(1)}, "cum"); shape(gum, {logits.size(0), logits.size(1)}, "gum");
  shape(finished, {logits.size(0), logits.size(1)}, "finished");
  TORCH_CHECK(beam_width >= 1 && beam_width <= 8 && beam_width <= logits.size(2), "recnet: beam_width must be in [1, min(8, V)], got ", beam_width);
  TORCH_CHECK(t >= 0 && t <= INT32_MAX, "recnet: t out of range");
  auto vals = at::empty({logits.size(1), beam_width}, logits.options()), gout = at::empty({logits.size(1), beam_width}, logits.options());
  auto idx = at::empty({logits.size(1), beam_width}, logits.options().dtype(at::kInt));
  ok(recnet_sbs_select_rows(H(h), logits.data_ptr<float>(), cum.data_ptr<float>(), gum.data_ptr<float>(), finished.data_ptr<int32_t>(),
                            (int32_t)logits.size(0), (int32_t)logits.size(1), (int32_t)logits.size(2), (int32_t)beam_width, (float)temperature,
                            (uint32_t)seed, (int32_t)t, vals.data_ptr<float>(), gout.data_ptr<float>(), idx.data_ptr<int32_t>(), stream()),
     "sbs_select_rows");
  return {vals, gout, idx};
}
// tokens [beam_width, Tm, B] rank-major, cum / gum [beam_width, B] float, len [beam_width, B] int32, n_steps [1] int32; hs empty:
// the single-model entry (the width is checked here before the outputs are allocated and zeroed; the temperature by the library)
using SbsOut = std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor>;
static SbsOut sbs_impl(int64_t h, const std::vector<recnet_handle*>& hs, const std::vector<float>& w, int64_t mode, const at::Tensor& enc,
                       int64_t beam_width, double temperature, int64_t seed) {
  chk_enc(h, enc);
  TORCH_CHECK(beam_width >= 1 && beam_width <= 8 && beam_width <= dim(h, RECNET_DIM_V), "recnet: beam_width must be in [1, min(8, V)], got ", beam_width);
  const int64_t B = enc.size(0);
  auto toks = at::zeros({beam_width, dim(h, RECNET_DIM_TM), B}, enc.options().dtype(at::kLong));
  auto cum = at::zeros({beam_width, B}, enc.options()), gum = at::zeros({beam_width, B}, enc.options());
  auto len = at::zeros({beam_width, B}, enc.options().dtype(at::kInt));
  auto n = at::zeros({1}, enc.options().dtype(at::kInt));
  if (hs.empty())
    ok(recnet_stochastic_beam_search(H(h), enc.data_ptr<float>(), (int32_t)beam_width, (float)temperature, (uint32_t)seed, toks.data_ptr<int64_t>(),
                                     cum.data_ptr<float>(), len.data_ptr<int32_t>(), gum.data_ptr<float>(), n.data_ptr<int32_t>(), stream()),
       "stochastic_beam_search");
  else
    ok(recnet_stochastic_beam_search_ensemble(hs.data(), (int32_t)hs.size(), w.data(), (int32_t)mode, enc.data_ptr<float>(), (int32_t)beam_width,
                                              (float)temperature, (uint32_t)seed, toks.data_ptr<int64_t>(), cum.data_ptr<float>(),
                                              len.data_ptr<int32_t>(), gum.data_ptr<float>(), n.data_ptr<int32_t>(), stream()),
       "stochastic_beam_search_ensemble");
  return {toks, cum, len, gum, n};
}
SbsOut stochastic_beam_search(int64_t h, const at::Tensor& enc, int64_t beam_width, double temperature, int64_t seed) {
  return sbs_impl(h, {}, {}, 0, enc, beam_width, temperature, seed);
}
SbsOut stochastic_beam_search_ensemble(int64_t h, at::IntArrayRef more_handles, at::ArrayRef<double> weights, int64_t mode, const at::Tensor& enc,
                                       int64_t beam_width, double temperature, int64_t seed) {
  const auto hs = ens_handles(h, more_handles);
  return sbs_impl(h, hs, ens_weights(weights, hs.size()), mode, enc, beam_width, temperature, seed);
}
// ---- consensus scoring by n-gram overlap.  hyp [N_h, T_h, B] int64, ref [N_r, T_r, B] int64 or undefined
// (the hypotheses are their own references), weights [N_r, B] float or undefined.  Returns util [N_h, B] double, sim [N_h, N_r, B]
// double (want_sim) and counts [N_h, N_r, B, 4], q_hyp [N_h, B, 4], q_ref [N_r, B, 4], len_hyp [N_h, B], len_ref [N_r, B] int32
// (want_counts); what is not asked for comes back as an empty tensor.  Tokens in [0, 2^31): the caller's duty.
using ConsensusOut = std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor>;
ConsensusOut consensus_rows(int64_t h, const at::Tensor& hyp, const c10::optional<at::Tensor>& ref, const c10::optional<at::Tensor>& weights,
                            double sigma, bool want_sim, bool want_counts) {
  chk(hyp, at::kLong, "hyp");
  TORCH_CHECK(hyp.dim() == 3 && hyp.size(0) >= 1 && hyp.size(0) <= 32 && hyp.size(1) >= 1 && hyp.size(1) <= 64 && hyp.size(2) >= 1 &&
              hyp.size(2) <= INT32_MAX, "recnet: hyp must be [N_h in [1, 32], T_h in [1, 64], B >= 1], got ", hyp.sizes());
  const int64_t Nh = hyp.size(0), Th = hyp.size(1), B = hyp.size(2);
  int64_t Nr = Nh, Tr = Th;
  const int64_t* rp = nullptr;
  if (ref.has_value() && ref->defined()) {
    chk(*ref, at::kLong, "ref");
    TORCH_CHECK(ref->dim() == 3 && ref->size(0) >= 1 && ref->size(0) <= 32 && ref->size(1) >= 1 && ref->size(1) <= 64 && ref->size(2) == B,
                "recnet: ref must be [N_r in [1, 32], T_r in [1, 64], B = ", B, "], got ", ref->sizes());
    Nr = ref->size(0); Tr = ref->size(1); rp = ref->data_ptr<int64_t>();
  }
  if (weights.has_value() && weights->defined())
    TORCH_CHECK(weights->dim() == 2 && weights->size(0) == Nr && weights->size(1) == B, "recnet: weights must be [N_r = ", Nr, ", B = ", B,
                "], got ", weights->sizes());
  const auto f64 = hyp.options().dtype(at::kDouble), i32 = hyp.options().dtype(at::kInt);
  auto util = at::empty({Nh, B}, f64);
  auto sim = want_sim ? at::empty({Nh, Nr, B}, f64) : at::empty({0}, f64);
  auto counts = at::empty({0}, i32), qh = at::empty({0}, i32), qr = at::empty({0}, i32), lh = at::empty({0}, i32), lr = at::empty({0}, i32);
  if (want_counts) {
    counts = at::empty({Nh, Nr, B, 4}, i32); qh = at::empty({Nh, B, 4}, i32); qr = at::empty({Nr, B, 4}, i32);
    lh = at::empty({Nh, B}, i32); lr = at::empty({Nr, B}, i32);
  }
  auto ip = [&](at::Tensor& t) { return want_counts ? t.data_ptr<int32_t>() : nullptr; };
  ok(recnet_consensus_rows(H(h), hyp.data_ptr<int64_t>(), (int32_t)Nh, (int32_t)Th, rp, (int32_t)Nr, (int32_t)Tr, (int32_t)B,
                           fptr(weights, "weights"), sigma, util.data_ptr<double>(), want_sim ? sim.data_ptr<double>() : nullptr, ip(counts),
                           ip(qh), ip(qr), ip(lh), ip(lr), stream()), "consensus_rows");
  return {util, sim, counts, qh, qr, lh, lr};
}

}  // namespace

TORCH_LIBRARY(recnet, m) {
  m.def("forward_decoder(int handle, Tensor encoder_outputs, Tensor targets, int T, Tensor step_weight, bool train, int seed) -> (Tensor loss, Tensor hiddens, Tensor scalars)");
  m.def("forward_decoder_free(int handle, Tensor encoder_outputs, Tensor targets, int T, Tensor step_weight, bool train, int seed) -> (Tensor loss, Tensor hiddens, Tensor output_indices, Tensor scalars)");
  m.def("backward_decoder(int handle, Tensor encoder_outputs, Tensor targets, Tensor? dhiddens, float grad_scale) -> ()");
  m.def("forward_reconstructor(int handle, Tensor encoder_outputs, Tensor? decoder_hiddens, int T, bool train, int seed) -> (Tensor loss, Tensor scalars)");
  m.def("backward_reconstructor(int handle, Tensor encoder_outputs, int T, float grad_scale) -> Tensor dhiddens");
  m.def("add_reg_grad(int handle, int which, float grad_scale) -> ()");
  m.def("train_step_fwd_bwd(int handle, Tensor encoder_outputs, Tensor targets, int T, Tensor step_weight, int seed) -> Tensor scalars");
  m.def("train_step(int handle, Tensor encoder_outputs, Tensor targets, int T, Tensor step_weight, int seed, int step) -> Tensor scalars");
  m.def("optimizer_step(int handle, int step, int flags) -> ()");
  m.def("clip_grad_norm(int handle, int which, float max_norm, Tensor like) -> Tensor total_norm");
  m.def("decoder_step(int handle, Tensor input, Tensor? h, Tensor? c, Tensor? encoder_outputs, bool train, int seed, int t) -> (Tensor logits, Tensor h, Tensor c)");
  m.def("reconstructor_step(int handle, Tensor? input, Tensor hr, Tensor? cr, Tensor? decoder_hiddens, int T, bool train, int seed, int t) -> (Tensor output, Tensor hr, Tensor cr)");
  m.def("greedy_search(int handle, Tensor encoder_outputs) -> (Tensor tokens, Tensor n_steps)");
  m.def("beam_search(int handle, Tensor encoder_outputs, int beam_width) -> (Tensor tokens, Tensor n_steps)");
  m.def("sample_search(int handle, Tensor encoder_outputs, float temperature, int top_k, int seed) -> (Tensor tokens, Tensor logprobs, Tensor n_steps)");
  m.def("sample_rows(int handle, Tensor logits, float temperature, int top_k, int seed, int t) -> (Tensor tokens, Tensor logprobs)");
  m.def("sample_search_nucleus(int handle, Tensor encoder_outputs, float temperature, int top_k, float top_p, int seed) -> (Tensor tokens, Tensor logprobs, Tensor n_allowed, Tensor n_steps)");
  m.def("sample_rows_nucleus(int handle, Tensor logits, float temperature, int top_k, float top_p, int seed, int t) -> (Tensor tokens, Tensor logprobs, Tensor n_allowed)");
  m.def("beam_select_rows(int handle, Tensor logits, Tensor cum, Tensor finished, int beam_width) -> (Tensor vals, Tensor idx)");
  m.def("beam_search_nbest(int handle, Tensor encoder_outputs, int beam_width, float length_alpha) -> (Tensor tokens, Tensor cum, Tensor lengths, Tensor score, Tensor n_steps)");
  m.def("beam_select_rows_constrained(int handle, Tensor logits, Tensor cum, Tensor finished, Tensor? hist, int t, int beam_width, int no_repeat_ngram, int min_length, int[] banned) -> (Tensor vals, Tensor idx)");
  m.def("beam_search_nbest_constrained(int handle, Tensor encoder_outputs, int beam_width, float length_alpha, int no_repeat_ngram, int min_length, int[] banned) -> (Tensor tokens, Tensor cum, Tensor lengths, Tensor score, Tensor n_steps)");
  m.def("beam_select_rows_diverse(int handle, Tensor logits, Tensor cum, Tensor finished, Tensor? hist, int t, int beam_width, int n_groups, float diversity_penalty, int no_repeat_ngram, int min_length, int[] banned) -> (Tensor vals, Tensor idx)");
  m.def("beam_search_nbest_diverse(int handle, Tensor encoder_outputs, int beam_width, float length_alpha, int n_groups, float diversity_penalty, int no_repeat_ngram, int min_length, int[] banned) -> (Tensor tokens, Tensor cum, Tensor lengths, Tensor score, Tensor group, Tensor n_steps)");
  m.def("score_captions(int handle, Tensor? encoder_outputs, Tensor tokens, float temperature) -> (Tensor logprobs, Tensor caption_logprob, Tensor lengths)");
  m.def("reconstruction_error(int handle, Tensor encoder_outputs, Tensor? tokens, Tensor? decoder_hiddens, bool want_recon) -> (Tensor err, Tensor recon)");
  m.def("ensemble_mix_rows(int handle, Tensor[] logits, float[] weights, int mode, bool in_place) -> Tensor y");
  m.def("beam_search_nbest_ensemble(int handle, int[] more_handles, float[] weights, int mode, Tensor encoder_outputs, int beam_width, float length_alpha, int n_groups, float diversity_penalty, int no_repeat_ngram, int min_length, int[] banned) -> (Tensor tokens, Tensor cum, Tensor lengths, Tensor score, Tensor group, Tensor n_steps)");
  m.def("score_captions_ensemble(int handle, int[] more_handles, float[] weights, int mode, Tensor? encoder_outputs, Tensor tokens) -> (Tensor logprobs, Tensor caption_logprob, Tensor lengths)");
  m.def("sbs_select_rows(int handle, Tensor logits, Tensor cum, Tensor gum, Tensor finished, int beam_width, float temperature, int seed, int t) -> (Tensor vals, Tensor gum_out, Tensor idx)");
  m.def("stochastic_beam_search(int handle, Tensor encoder_outputs, int beam_width, float temperature, int seed) -> (Tensor tokens, Tensor cum, Tensor lengths, Tensor gum, Tensor n_steps)");
  m.def("stochastic_beam_search_ensemble(int handle, int[] more_handles, float[] weights, int mode, Tensor encoder_outputs, int beam_width, float temperature, int seed) -> (Tensor tokens, Tensor cum, Tensor lengths, Tensor gum, Tensor n_steps)");
  m.def("consensus_rows(int handle, Tensor hyp, Tensor? ref, Tensor? weights, float sigma, bool want_sim, bool want_counts) -> (Tensor util, Tensor sim, Tensor counts, Tensor q_hyp, Tensor q_ref, Tensor len_hyp, Tensor len_ref)");
}

// The handle is an int, so dispatch cannot key on a tensor for every op: ops with tensor arguments are registered for the
// CUDA (= HIP on ROCm) key — a CPU tensor then fails with "no kernel for CPU backend", loudly — and the tensor-free ones
// as CompositeExplicitAutograd.
TORCH_LIBRARY_IMPL(recnet, CUDA, m) {
  m.impl("forward_decoder", forward_decoder);
  m.impl("forward_decoder_free", forward_decoder_free);
  m.impl("backward_decoder", backward_decoder);
  m.impl("forward_reconstructor", forward_reconstructor);
  m.impl("backward_reconstructor", backward_reconstructor);
  m.impl("train_step_fwd_bwd", train_step_fwd_bwd);
  m.impl("train_step", train_step);
  m.impl("clip_grad_norm", clip_grad_norm);
  m.impl("decoder_step", decoder_step);
  m.impl("reconstructor_step", reconstructor_step);
  m.impl("greedy_search", greedy_search);
  m.impl("beam_search", beam_search);
  m.impl("sample_search", sample_search);
  m.impl("sample_rows", sample_rows);
  m.impl("sample_search_nucleus", sample_search_nucleus);
  m.impl("sample_rows_nucleus", sample_rows_nucleus);
  m.impl("beam_select_rows", beam_select_rows);
  m.impl("beam_search_nbest", beam_search_nbest);
  m.impl("beam_select_rows_constrained", beam_select_rows_constrained);
  m.impl("beam_search_nbest_constrained", beam_search_nbest_constrained);
  m.impl("beam_select_rows_diverse", beam_select_rows_diverse);
  m.impl("beam_search_nbest_diverse", beam_search_nbest_diverse);
  m.impl("score_captions", score_captions);
  m.impl("reconstruction_error", reconstruction_error);
  m.impl("consensus_rows", consensus_rows);
  m.impl("ensemble_mix_rows", ensemble_mix_rows);
  m.impl("beam_search_nbest_ensemble", beam_search_nbest_ensemble);
  m.impl("score_captions_ensemble", score_captions_ensemble);
  m.impl("sbs_select_rows", sbs_select_rows);
  m.impl("stochastic_beam_search", stochastic_beam_search);
  m.impl("stochastic_beam_search_ensemble", stochastic_beam_search_ensemble);
}
TORCH_LIBRARY_IMPL(recnet, CompositeExplicitAutograd, m) {
  m.impl("add_reg_grad", add_reg_grad);
  m.impl("optimizer_step", optimizer_step);
}
