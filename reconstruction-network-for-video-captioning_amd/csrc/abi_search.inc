// C ABI: the decoder's per-step API, the device-side inference search (eval.py:19-120), greedy / beam / sampling, the scoring of
// given captions and their per-caption reconstruction error (train.py:96-102 / :125-128 in eval mode).
// Part of api.hip (one translation unit; see the include list there).
// The operand rows a decode step works on: the embedding rows, their input product, the operand copy of the incoming hidden
// states and of the outgoing ones (the vocabulary product reads those).
struct DecStepRows { void* emb; float* Xe; void* h_lp_in; void* h_lp_out; };
// B rows on the training operand buffers: rows [0,B) / [B,2B) of Hs_lp are scratch
static DecStepRows dec_rows_batch(recnet_handle* h) { return {h->emb_lp, h->Xe, h->Hs_lp, at_off(h, h->Hs_lp, (size_t)h->B * h->ldH)}; }
// up to 8 * B rows ordered [beam][caption] on the N-best search's own operand rows
static DecStepRows dec_rows_beams(recnet_handle* h) { return {h->bs_emb, h->bs_Xe, h->bs_hlp, at_off(h, h->bs_hlp, (size_t)8 * h->B * h->ldH)}; }
// One decode step of `rows` rows on already prepared loop invariants (Uv, P, bias sum): embedding, input projection,
// h . [W_hh ; attn_W]^T, cell kernel, vocabulary projection, each launch once for all rows.  nc = 0: one row per caption; nc = B:
// [beam][caption] rows that share the captions' Uv / P (DecCellArgs::nc).  h_in null: the zero state, no recurrent product.
static void dec_step(recnet_handle* h, int rows, int nc, const DecStepRows& r, const int64_t* tokens, const float* h_in,
                     const float* c_in, float* logits, float* h_out, float* c_out, int train, int t, hipStream_t st) {
  const int F = h->F, E = h->E, H = h->H, A = h->A, V = h->V;
  // (the kernel's B places a row in (t, b) for the dropout mask and picks tokens[row % B]: one step of `rows` tokens)
  embed_fwd(h, nullptr, tokens, r.emb, rows, rows, train, t, st);
  gemm(h, r.emb, 0, h->ldE, h->We_w, 0, h->ldE, r.Xe, 4 * H, h->bsum_d, rows, 4 * H, E, 1.f, 0, st);
  int S = 0;
  if (h_in) {   // operand copy of the incoming hidden state, then h . [W_hh ; attn_W]^T
    pack_block(h, r.h_lp_in, h->ldH, h_in, H, rows, H, 1.f, st);
    S = gemm_slabs(h, RN_TAG_DEC_FWD, r.h_lp_in, h->ldH, h->Wcomb, 0, h->ldH, rows, 4 * H + A, H, st);
  }
  DecCellArgs a;
  a.t = t; a.B = rows; a.F = F; a.H = H; a.A = A; a.S = S; a.slab = h_in ? h->slab : nullptr; a.nc = nc;
  a.Xe = r.Xe; a.P = h->P; a.ldp = h->ld4H; a.Uv = h->Uv; a.ab = h->dP.attn_b; a.w = h->dP.attn_w_weight;
  a.gru = h->dgru; a.c_prev = h->dgru ? h_in : c_in; a.h_out = h_out; a.c_out = c_out; a.acts = nullptr; a.Wh_out = nullptr; a.att_out = nullptr; a.softmax = h->c.decoder_attn_normalize == RECNET_ATTN_SOFTMAX;
  a.h_lp = r.h_lp_out; a.ld_hlp = h->ldH;
  launch_dec_cell(h, a, rows, st);
  gemm(h, r.h_lp_out, 0, h->ldH, h->Wo_w, 0, h->ldH, logits, V, h->dP.out_bias, rows, V, H, 1.f, 0, st);
  if (train && h->c.decoder_out_dropout > 0.f)
    hipLaunchKernelGGL(logits_drop_kernel, dim3(ew_blocks((size_t)rows * V)), dim3(256), 0, st, logits, rows, V,
                       mkdrop(h, RN_SITE_DEC_LOGIT, h->c.decoder_out_dropout, train), t);
  h->fwd_dec_done = 0;
}

int recnet_decoder_prepare(recnet_handle* h, const float* enc, void* stream) {
  REQUIRE_WS(h);
  if (!h->dec_bound) return fail(RECNET_ESTATE, "decoder not bound");
  if (!enc) return fail(RECNET_EINVAL, "null argument");
  dec_invariants(h, enc, (hipStream_t)stream);
  h->fwd_dec_done = 0;
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_decoder_step(recnet_handle* h, const int64_t* tokens, const float* h_in, const float* c_in,
                        const float* enc, float* logits, float* h_out, float* c_out, int32_t train,
                        uint32_t seed, int32_t t, void* stream) {
  REQUIRE_WS(h);
  if (!h->dec_bound) return fail(RECNET_ESTATE, "decoder not bound");
  if (!tokens || !logits || !h_out || (!c_out && !h->dgru)) return fail(RECNET_EINVAL, "null argument");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, st, h->ctrl, seed);
  if (enc) dec_invariants(h, enc, st);   // enc == NULL: reuse what recnet_decoder_prepare / the last call computed
  dec_step(h, h->B, 0, dec_rows_batch(h), tokens, h_in, c_in, logits, h_out, c_out, train, t, st);
  LAUNCH_OK();
  return RECNET_OK;
}

// One reconstructor step with the reference's per-step semantics (GlobalReconstructor.forward, global_reconstructor.py:30-46;
// LocalReconstructor.forward, local_reconstructor.py:37-55) on the single-step kernels.  decoder_hiddens == NULL reuses
// the loop invariants of the previous call (the mean-pooled states / Ud = hiddens . U_r^T): the reference's loops
// (train.py:93-94,122-123) pass the same decoder_hiddens T or F times.  Row block 0 of the operand buffers is scratch.
int recnet_reconstructor_step(recnet_handle* h, const float* input, const float* hr_in, const float* cr_in,
                              const float* decoder_hiddens, int32_t T, float* out, float* hr_out, float* cr_out,
                              int32_t train, uint32_t seed, int32_t t, void* stream) {
  REQUIRE_WS(h);
  FLUSH_PENDING(h, stream);
  if (h->kind == RECNET_REC_NONE || !h->rec_bound) return fail(RECNET_ESTATE, "reconstructor not bound");
  if (!out || !hr_out || (!cr_out && !h->rgru)) return fail(RECNET_EINVAL, "null argument");
  if (h->kind == RECNET_REC_GLOBAL && !input) return fail(RECNET_EINVAL, "the global reconstructor step needs `input` (= decoder_hiddens[t])");
  if (check_T(h, T)) return fail(RECNET_EINVAL, "T out of range");
  hipStream_t st = (hipStream_t)stream;
  const int B = h->B, H = h->H, R = h->R, RA = h->RA;
  hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, st, h->ctrl, seed);
  gate_bias(h->rP.rnn_bias_ih_l0, h->rP.rnn_bias_hh_l0, h->bsum_r, R, h->rgru, st);
  const float* c_prev = h->rgru ? hr_in : cr_in;
  if (hr_in) pack_block(h, h->Hr_lp, h->ldR, hr_in, R, B, R, 1.f, st);
  h->fwd_dec_done = h->fwd_rec_done = 0; h->ss.mp_done = 0;     // Hs / Hs_lp / Hr_lp no longer hold a sequence-level forward
  const DropDesc dd = mkdrop(h, RN_SITE_REC_INPUT, h->c.reconstructor_decoder_dropout, train);
  if (h->kind == RECNET_REC_GLOBAL) {
    if (decoder_hiddens)   // (caption_max_len / T^2) sum_t h_t: mean over T and L, rescaled (global_reconstructor.py:33-37)
      mean_over_t(h, decoder_hiddens, T, H, (float)h->cml / ((float)T * (float)T), h->mp, nullptr, 0, st);
    pack_block(h, h->Hs_lp, h->ldH, input, H, B, H, 1.f, st);
    const size_t n = (size_t)B * h->ld2H;
    if (h->lp) hipLaunchKernelGGL(xcat_global_kernel<bf16_t>, dim3(ew_blocks(n)), dim3(256), 0, st, (const bf16_t*)h->Hs_lp, h->ldH, h->mp, (bf16_t*)h->Xcat_g, h->ld2H, 1, B, H, dd, t);
    else hipLaunchKernelGGL(xcat_global_kernel<float>, dim3(ew_blocks(n)), dim3(256), 0, st, (const float*)h->Hs_lp, h->ldH, h->mp, (float*)h->Xcat_g, h->ld2H, 1, B, H, dd, t);
    gemm(h, h->Xcat_g, 0, h->ld2H, h->Wih_f, 0, h->ld2H, h->Xg, 4 * R, h->bsum_r, B, 4 * R, 2 * H, 1.f, 0, st);
    int S = 0;
    if (hr_in) S = gemm_slabs(h, RN_TAG_REC_FWD, h->Hr_lp, h->ldR, h->Whh_w, 0, h->ldR, B, 4 * R, R, st);
    lstm_pw(h, R, S, 4 * R, h->Xg, 4 * R, nullptr, nullptr, c_prev, hr_out, h->Hr_lp, h->ldR, nullptr, 0, cr_out ? cr_out : h->Cr, h->acts_r, st);
  } else {
    const size_t esz = h->lp ? 2 : 4;
    if (decoder_hiddens) {   // Ud = hiddens . U_r^T (local_reconstructor.py:42)
      copyf(decoder_hiddens, h->Hs, (size_t)T * B * H, st);
      pack_block(h, h->Hs_lp, h->ldH, decoder_hiddens, H, T * B, H, 1.f, st);
      gemm(h, h->Hs_lp, 0, h->ldH, h->Ur_w, 0, h->ldH, h->Ud, RA, nullptr, T * B, RA, H, 1.f, 0, st);
    }
    hipMemsetAsync(h->Xcat_r, 0, (size_t)B * h->ldHR * esz, st);
    int Sa = 0;
    if (hr_in) {
      const size_t n = (size_t)B * R;
      if (h->lp) hipLaunchKernelGGL(pack_cols_kernel<bf16_t>, dim3(ew_blocks(n)), dim3(256), 0, st, (bf16_t*)h->Xcat_r + H, h->ldHR, hr_in, R, B, R);
      else hipLaunchKernelGGL(pack_cols_kernel<float>, dim3(ew_blocks(n)), dim3(256), 0, st, (float*)h->Xcat_r + H, h->ldHR, hr_in, R, B, R);
      Sa = gemm_slabs(h, RN_TAG_REC_ATT, h->Hr_lp, h->ldR, h->Wr_w, 0, h->ldR, B, RA, R, st);
    }
    LocAttnArgs a;
    a.B = B; a.T = T; a.H = H; a.A = RA; a.Ud = h->Ud; a.ab = h->rP.attn_b; a.w = h->rP.attn_w_weight; a.Hs = h->Hs;
    a.xcat_ld = h->ldHR; a.dd = dd; a.s = t; a.S = Sa; a.slab = hr_in ? h->slab : nullptr;
    a.Whr_out = h->Whr; a.beta_out = h->beta; a.xcat = h->Xcat_r;
    const size_t sm = (size_t)(RA + T + 16) * 4;
    LAUNCH_AT(h, loc_attn_fwd_kernel, dim3(B, cdiv(H, 256)), dim3(256), sm, st, a);
    const int Sb = gemm_slabs(h, RN_TAG_REC_FWD, h->Xcat_r, h->ldHR, h->Wihh_w, 0, h->ldHR, B, 4 * R, H + R, st);
    lstm_pw(h, R, Sb, 4 * R, nullptr, 0, h->bsum_r, nullptr, c_prev, hr_out, h->Hr_lp, h->ldR, nullptr, 0, cr_out ? cr_out : h->Cr, h->acts_r, st);
  }
  gemm(h, h->Hr_lp, 0, h->ldR, h->Wor_w, 0, h->ldR, out, R, h->rP.out_bias, B, R, R, 1.f, 0, st);   // out(h) (:45 / :54)
  LAUNCH_OK();
  return RECNET_OK;
}

// ---- the skeleton of the device-side searches: every entry opens with search_check, its own argument checks follow, then
// search_begin, its loop of Tm steps (a fixed trip count, no host synchronisation) and search_end
static int search_check(const recnet_handle* h, bool args_given) {
  REQUIRE_WS(h);
  if (!h->dec_bound) return fail(RECNET_ESTATE, "decoder not bound");
  if (!args_given) return fail(RECNET_EINVAL, "null argument");
  return RECNET_OK;
}
// The invariants, n_steps = 0 and one initial hypothesis per caption in slot 0 of the sr_* pairs: <SOS> = 1 (eval.py:131), the zero
// state; beam_eos_fill >= 0 (the two beam searches): also log-prob 0, an empty history and the <EOS> words filled with that byte
// (eval.py:37-42: 0xFF = -1, no <EOS> yet; the N-best search: 0, not finished).
static void search_begin(recnet_handle* h, const float* enc, int32_t* n_steps_out, int beam_eos_fill, hipStream_t st) {
  const int B = h->B, H = h->H, Tm = h->Tm;
  dec_invariants(h, enc, st);
  hipMemsetAsync(n_steps_out, 0, 4, st);
  hipMemsetAsync(h->sr_h[0], 0, (size_t)B * H * 4, st);
  hipMemsetAsync(h->sr_c[0], 0, (size_t)B * H * 4, st);
  if (beam_eos_fill >= 0) {
    hipMemsetAsync(h->sr_cum[0], 0, (size_t)B * 4, st);
    hipMemsetAsync(h->sr_hist[0], 0, (size_t)B * Tm * 8, st);
    hipMemsetAsync(h->sr_eos[0], beam_eos_fill, (size_t)B * 4, st);
  }
  hipLaunchKernelGGL(fill_i64_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, h->sr_tok[0], (int64_t)1, B);
}
// a search that never stopped ran all Tm steps
static void search_end(recnet_handle* h, int32_t* n_steps_out, hipStream_t st) {
  hipLaunchKernelGGL(search_finish_kernel, dim3(1), dim3(1), 0, st, n_steps_out, h->Tm);
}
// One hypothesis per caption (eval.py:19-33): pick(t, out_t) launches what turns h->sr_logits [B][V] into the step's tokens out_t [B]
static void search_one_per_caption(recnet_handle* h, const float* enc, int64_t* tokens_out, int32_t* n_steps_out, hipStream_t st,
                                   const std::function<void(int, int64_t*)>& pick) {
  const int B = h->B;
  search_begin(h, enc, n_steps_out, -1, st);
  const DecStepRows rows = dec_rows_batch(h);
  const int64_t* tok = h->sr_tok[0];
  int cur = 0;
  for (int t = 0; t < h->Tm; ++t) {
    dec_step(h, B, 0, rows, tok, h->sr_h[cur], h->sr_c[cur], h->sr_logits, h->sr_h[cur ^ 1], h->sr_c[cur ^ 1], 0, t, st);
    int64_t* out_t = tokens_out + (size_t)t * B;
    pick(t, out_t);
    hipLaunchKernelGGL(search_stop_kernel, dim3(1), dim3(256), 0, st, out_t, (const int32_t*)nullptr, B, t, n_steps_out);
    tok = out_t; cur ^= 1;
  }
  search_end(h, n_steps_out, st);
}

int recnet_greedy_search(recnet_handle* h, const float* enc, int64_t* tokens_out, int32_t* n_steps_out, void* stream) {
  int r = search_check(h, enc && tokens_out && n_steps_out); if (r) return r;
  hipStream_t st = (hipStream_t)stream;
  search_one_per_caption(h, enc, tokens_out, n_steps_out, st, [&](int, int64_t* out_t) {
    hipLaunchKernelGGL(argmax_rows_kernel, dim3(h->B), dim3(256), 0, st, h->sr_logits, h->V, h->V, out_t);
  });
  LAUNCH_OK();
  return RECNET_OK;
}

// ---- sampling (the reference has no counterpart; the loop shape is eval.py:19-33) and, top_p given, nucleus (top-p) sampling on
// what the top-k cut leaves (DESIGN.md section 13).  One launcher and one body per shape of entry; the exports without top_p pass
// null and keep their kernels, the nucleus exports launch the nucleus kernels at top_p = 1 too (they count n_allowed).
static int check_sample(float temperature, int top_k, int V, const float* top_p = nullptr) {
  if (!(temperature > 0.f) || !std::isfinite(temperature)) return fail(RECNET_EINVAL, "temperature must be positive and finite");
  if (top_k < 0 || top_k > V) return fail(RECNET_EINVAL, "top_k must be in [0, V]");
  if (!top_p) return RECNET_OK;
  if (!(*top_p > 0.f) || !(*top_p <= 1.f)) return fail(RECNET_EINVAL, "top_p must be in (0, 1]");    // (refuses NaN too)
  if (*top_p < 1.f && V >= (1 << 21)) return fail(RECNET_EINVAL, "top_p < 1 needs V < 2^21 (the integer masses sum in 53 bits)");
  return RECNET_OK;
}
// one draw per row of logits [rows][V]; (B, t) place the rows in the counter space of the draw; n_allowed [rows] may be null
static void launch_sample_rows(const float* logits, int rows, int V, int B, float temperature, int top_k, const float* top_p, uint32_t seed,
                               int t, int64_t* tokens, float* logprobs, int32_t* n_allowed, hipStream_t st) {
  SampleNucArgs a;
  a.x = logits; a.V = V; a.k = top_k == V ? 0 : top_k; a.B = B; a.t = t;
  a.temp = temperature; a.key = rn_site_key(seed, RN_SITE_SAMPLE); a.tok = tokens; a.lp = logprobs;
  a.top_p = top_p ? *top_p : 1.f; a.n_allowed = n_allowed;
  const SampleArgs& u = a;
  const bool res = V <= SR_ROW_LDS_MAX;
  const size_t sm = res ? (size_t)V * 4 : 0;
  if (top_p) {
    if (res) hipLaunchKernelGGL((sample_rows_kernel<true, true>), dim3(rows), dim3(256), sm, st, a);
    else hipLaunchKernelGGL((sample_rows_kernel<false, true>), dim3(rows), dim3(256), sm, st, a);
  } else {
    if (res) hipLaunchKernelGGL((sample_rows_kernel<true>), dim3(rows), dim3(256), sm, st, u);
    else hipLaunchKernelGGL((sample_rows_kernel<false>), dim3(rows), dim3(256), sm, st, u);
  }
}
static int sample_rows_run(recnet_handle* h, const float* logits, int rows, int V, float temperature, int top_k, const float* top_p,
                           uint32_t seed, int t, int64_t* tokens_out, float* logprobs_out, int32_t* n_allowed_out, void* stream) {
  REQUIRE_WS(h);
  if (!logits || !tokens_out || !logprobs_out) return fail(RECNET_EINVAL, "null argument");
  if (rows < 1 || V < 1 || t < 0) return fail(RECNET_EINVAL, "rows and V must be positive, t non-negative");
  int r = check_sample(temperature, top_k, V, top_p); if (r) return r;
  launch_sample_rows(logits, rows, V, rows, temperature, top_k, top_p, seed, t, tokens_out, logprobs_out, n_allowed_out, (hipStream_t)stream);
  LAUNCH_OK();
  return RECNET_OK;
}
static int sample_search_run(recnet_handle* h, const float* enc, float temperature, int top_k, const float* top_p, uint32_t seed,
                             int64_t* tokens_out, float* logprobs_out, int32_t* n_allowed_out, int32_t* n_steps_out, void* stream) {
  int r = search_check(h, enc && tokens_out && logprobs_out && n_steps_out); if (r) return r;
  r = check_sample(temperature, top_k, h->V, top_p); if (r) return r;
  hipStream_t st = (hipStream_t)stream;
  search_one_per_caption(h, enc, tokens_out, n_steps_out, st, [&](int t, int64_t* out_t) {
    launch_sample_rows(h->sr_logits, h->B, h->V, h->B, temperature, top_k, top_p, seed, t, out_t, logprobs_out + (size_t)t * h->B,
                       n_allowed_out ? n_allowed_out + (size_t)t * h->B : nullptr, st);
  });
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_sample_rows(recnet_handle* h, const float* logits, int32_t rows, int32_t V, float temperature, int32_t top_k,
                       uint32_t seed, int32_t t, int64_t* tokens_out, float* logprobs_out, void* stream) {
  return sample_rows_run(h, logits, rows, V, temperature, top_k, nullptr, seed, t, tokens_out, logprobs_out, nullptr, stream);
}
int recnet_sample_rows_nucleus(recnet_handle* h, const float* logits, int32_t rows, int32_t V, float temperature, int32_t top_k,
                               float top_p, uint32_t seed, int32_t t, int64_t* tokens_out, float* logprobs_out, int32_t* n_allowed_out,
                               void* stream) {
  return sample_rows_run(h, logits, rows, V, temperature, top_k, &top_p, seed, t, tokens_out, logprobs_out, n_allowed_out, stream);
}
int recnet_sample_search(recnet_handle* h, const float* enc, float temperature, int32_t top_k, uint32_t seed,
                         int64_t* tokens_out, float* logprobs_out, int32_t* n_steps_out, void* stream) {
  return sample_search_run(h, enc, temperature, top_k, nullptr, seed, tokens_out, logprobs_out, nullptr, n_steps_out, stream);
}
int recnet_sample_search_nucleus(recnet_handle* h, const float* enc, float temperature, int32_t top_k, float top_p, uint32_t seed,
                                 int64_t* tokens_out, float* logprobs_out, int32_t* n_allowed_out, int32_t* n_steps_out, void* stream) {
  return sample_search_run(h, enc, temperature, top_k, &top_p, seed, tokens_out, logprobs_out, n_allowed_out, n_steps_out, stream);
}

// ---- scoring given captions (the reference has no counterpart; the loop is train.py:25,45 in eval mode)
static void launch_logprob_rows(const float* logits, const int64_t* tokens, int rows, int V, float temperature, float* logprobs,
                                hipStream_t st) {
  LogprobArgs a;
  a.x = logits; a.V = V; a.temp = temperature; a.tok = tokens; a.lp = logprobs;
  if (V <= LP_NV * 256) hipLaunchKernelGGL((logprob_rows_kernel<true>), dim3(rows), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((logprob_rows_kernel<false>), dim3(rows), dim3(256), 0, st, a);
}

int recnet_logprob_rows(recnet_handle* h, const float* logits, const int64_t* tokens, int32_t rows, int32_t V, float temperature,
                        float* logprobs_out, void* stream) {
  REQUIRE_WS(h);
  if (!logits || !tokens || !logprobs_out) return fail(RECNET_EINVAL, "null argument");
  if (rows < 1 || V < 1) return fail(RECNET_EINVAL, "rows and V must be positive");
  int r = check_sample(temperature, 0, V); if (r) return r;
  launch_logprob_rows(logits, tokens, rows, V, temperature, logprobs_out, (hipStream_t)stream);
  LAUNCH_OK();
  return RECNET_OK;
}

// The teacher-forced forward in eval mode (the persistent chain where the handle runs it, the per-step kernels otherwise) and the
// batched vocabulary product into h->logits [T * B][V].  Hs / acts / logits no longer hold a training forward afterwards: a backward
// call is refused until the next forward.
static int score_logits(recnet_handle* h, const float* enc, const int64_t* tokens, int T, hipStream_t st) {
  // step 0 is fed <SOS>, step t > 0 tokens[t - 1] (embed_fwd_kernel's teacher-forcing rule); enc == NULL: the invariants of the
  // previous call / of recnet_decoder_prepare
  int r = dec_fwd_chain(h, enc, tokens, T, 0, st, nullptr, nullptr, DFC_NO_REG_NORM | (enc ? 0 : DFC_REUSE_INVARIANTS)); if (r) return r;
  h->fwd_dec_done = h->fwd_rec_done = 0; h->ss.mp_done = 0; h->ss.xcat_done = 0;
  gemm(h, h->Hs_lp, 0, h->ldH, h->Wo_w, 0, h->ldH, h->logits, h->V, h->dP.out_bias, T * h->B, h->V, h->H, 1.f, 0, st);
  return RECNET_OK;
}
// score_logits, the row kernel, the per-caption sums.
int recnet_score_captions(recnet_handle* h, const float* enc, const int64_t* tokens, int32_t T, float temperature,
                          float* logprobs_out, float* caption_logprob_out, int32_t* length_out, void* stream) {
  REQUIRE_WS(h);
  FLUSH_PENDING(h, stream);      // (a pending reconstructor update reads the operands of the step it belongs to: Hs_lp is overwritten here)
  if (!h->dec_bound) return fail(RECNET_ESTATE, "decoder not bound");
  if (check_T(h, T)) return fail(RECNET_EINVAL, "T out of range");
  if (!tokens || !logprobs_out || !caption_logprob_out || !length_out) return fail(RECNET_EINVAL, "null argument");
  int r = check_sample(temperature, 0, h->V); if (r) return r;
  hipStream_t st = (hipStream_t)stream;
  r = score_logits(h, enc, tokens, T, st); if (r) return r;
  launch_logprob_rows(h->logits, tokens, T * h->B, h->V, temperature, logprobs_out, st);
  hipLaunchKernelGGL(caption_logprob_kernel, dim3(cdiv(h->B, 256)), dim3(256), 0, st, logprobs_out, tokens, T, h->B, caption_logprob_out, length_out);
  LAUNCH_OK();
  return RECNET_OK;
}

// ---- reconstruction error of given captions (the reference has no counterpart: train.py:99-102 / :128 only form the batch mean)
// The row kernel over the reconstruction the outputs-only forward left in h->outm / h->outl.  Grid: the caption's items cut into NP
// parts so that B * NP workgroups cover the chip about twice (B = 100 on 256 CUs: 6 parts of a global caption and 6 of a local one), a part never
// below one wave's worth of items; the partial sums [B][NP] go through h->rowloss (NP <= caption_max_len + 1 keeps them inside it;
// the decoder forward that owns it is invalidated by the call anyway).
static void launch_recon_err(recnet_handle* h, const float* enc, int T, float* err_out, float* recon_out, hipStream_t st) {
  const int B = h->B, F = h->F, R = h->R;
  const bool local = h->kind == RECNET_REC_LOCAL;
  ReconErrArgs a;
  a.out = local ? h->outl : h->outm; a.enc = enc; a.recon = recon_out; a.B = B; a.F = F; a.R = R;
  a.scale = local ? (float)(1.0 / ((double)F * R)) : (float)(1.0 / ((double)R * T));
  const bool vec = (R & 3) == 0 && (((uintptr_t)a.out) & 15) == 0 && (((uintptr_t)enc) & 15) == 0 && (((uintptr_t)recon_out) & 15) == 0;
  const long n = (long)(local ? F : 1) * (vec ? R >> 2 : R);
  const int want = cdiv(2L * (h->ncu > 0 ? h->ncu : 256), B), most = cdiv(n, 64);
  int NP = want < most ? want : most;
  if (NP > h->Tm) NP = h->Tm;
  if (NP < 1) NP = 1;
  a.NP = NP; a.dst = NP == 1 ? err_out : h->rowloss;
  const dim3 g(B, NP);
  hipEvent_t pe = prof_bracket_begin(h, RN_SITE_RECON_ERR, st);
  if (local) {
    if (vec) hipLaunchKernelGGL((recon_err_kernel<true, 4>), g, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((recon_err_kernel<true, 1>), g, dim3(256), 0, st, a);
  } else {
    if (vec) hipLaunchKernelGGL((recon_err_kernel<false, 4>), g, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((recon_err_kernel<false, 1>), g, dim3(256), 0, st, a);
  }
  if (NP > 1) hipLaunchKernelGGL(recon_err_finalize_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, (const float*)h->rowloss, NP, B, a.scale, err_out);
  if (pe) hipEventRecord(pe, st);
}

// The decoder's teacher-forced forward in eval mode as recnet_score_captions runs it (tokens), or hidden states handed in as
// recnet_forward_reconstructor takes them (hiddens); then the reconstructor's forward in eval mode with outputs only (fwd_rec:
// the same chains, row groups and per-step fall-backs as recnet_forward_reconstructor(train = 0), without norms, loss epilogues and
// loss scalars), then the row kernel.  The handle is left between two steps: no saved forward a backward could follow.
int recnet_reconstruction_error(recnet_handle* h, const float* enc, const int64_t* tokens, const float* hiddens, int32_t T,
                                float* err_out, float* recon_out, void* stream) {
  REQUIRE_WS(h);
  FLUSH_PENDING(h, stream);
  if (h->kind == RECNET_REC_NONE || !h->rec_bound) return fail(RECNET_ESTATE, "reconstructor not bound");
  if (!enc || !err_out) return fail(RECNET_EINVAL, "null argument");
  if ((tokens != nullptr) == (hiddens != nullptr)) return fail(RECNET_EINVAL, "exactly one of tokens / hiddens must be given");
  if (check_T(h, T)) return fail(RECNET_EINVAL, "T out of range");
  if (tokens && !h->dec_bound) return fail(RECNET_ESTATE, "decoder not bound");
  hipStream_t st = (hipStream_t)stream;
  int r;
  if (tokens) {
    r = dec_fwd_chain(h, enc, tokens, T, 0, st, nullptr, nullptr, DFC_NO_REG_NORM); if (r) return r;
  } else {   // hidden states handed in by the caller: refresh the fp32 image and its operand copy
    copyf(hiddens, h->Hs, (size_t)T * h->B * h->H, st);
    pack_block(h, h->Hs_lp, h->ldH, hiddens, h->H, T * h->B, h->H, 1.f, st);
    h->ss.mp_done = 0;
  }
  h->fwd_dec_done = h->fwd_rec_done = 0;
  h->ss.xcat_done = 0;          // (as recnet_forward_reconstructor: the operand is formed here, in eval mode)
  r = fwd_rec(h, enc, T, 0, st, false, false, nullptr, /*outputs_only*/ true); if (r) return r;
  launch_recon_err(h, enc, T, err_out, recon_out, st);
  h->fwd_dec_done = h->fwd_rec_done = 0;
  h->ss.mp_done = 0; h->ss.xcat_done = 0; h->ss.dout_ready = 0; h->ss.dhr_done = 0; h->ss.encmean_hoisted = 0;
  LAUNCH_OK();
  return RECNET_OK;
}

// the regather of both beam searches on the sr_* pairs: slot `cur` and the step's states sr_hn / sr_cn into slot cur ^ 1
static BeamUpdArgs beam_update_args(recnet_handle* h, int bw, int t, int cur, const int32_t* n_steps) {
  BeamUpdArgs u;
  u.B = h->B; u.H = h->H; u.V = h->V; u.Tm = h->Tm; u.bw = bw; u.t = t;
  u.vals = h->sr_vals; u.idx = h->sr_idx; u.h_next = h->sr_hn; u.c_next = h->dgru ? nullptr : h->sr_cn;
  u.eos_old = h->sr_eos[cur]; u.hist_old = h->sr_hist[cur];
  u.h_new = h->sr_h[cur ^ 1]; u.c_new = h->sr_c[cur ^ 1]; u.cum_new = h->sr_cum[cur ^ 1];
  u.eos_new = h->sr_eos[cur ^ 1]; u.hist_new = h->sr_hist[cur ^ 1]; u.tok_new = h->sr_tok[cur ^ 1];
  u.n_steps = n_steps;
  return u;
}

int recnet_beam_search(recnet_handle* h, const float* enc, int32_t beam_width, int64_t* best_out, int32_t* n_steps_out,
                       void* stream) {
  int r = search_check(h, enc && best_out && n_steps_out); if (r) return r;
  if (beam_width < 1 || beam_width > 8) return fail(RECNET_EINVAL, "beam_width must be in [1, 8]");
  hipStream_t st = (hipStream_t)stream;
  const int B = h->B, H = h->H, V = h->V, Tm = h->Tm, bw = beam_width;
  search_begin(h, enc, n_steps_out, 0xFF, st);
  const DecStepRows rows = dec_rows_batch(h);
  int cur = 0, nb = 1;
  for (int t = 0; t < Tm; ++t) {
    for (int i = 0; i < nb; ++i) {   // the reference's search: one decode step of B rows per beam
      dec_step(h, B, 0, rows, h->sr_tok[cur] + (size_t)i * B, h->sr_h[cur] + (size_t)i * B * H, h->sr_c[cur] + (size_t)i * B * H,
               h->sr_logits, h->sr_hn + (size_t)i * B * H, h->sr_cn + (size_t)i * B * H, 0, t, st);
      hipLaunchKernelGGL(beam_score_kernel, dim3(B), dim3(256), 0, st, h->sr_logits, h->sr_cum[cur], h->sr_eos[cur], h->sr_scores,
                         B, V, nb, i, t);
    }
    hipLaunchKernelGGL(topk_rows_kernel, dim3(B), dim3(256), 0, st, h->sr_scores, nb * V, bw, h->sr_vals, h->sr_idx);
    hipLaunchKernelGGL(beam_update_kernel<false>, dim3(bw, B), dim3(128), 0, st, beam_update_args(h, bw, t, cur, n_steps_out));
    hipLaunchKernelGGL(search_stop_kernel, dim3(1), dim3(256), 0, st, h->sr_tok[cur ^ 1], (const int32_t*)nullptr, bw * B, t, n_steps_out);
    cur ^= 1; nb = bw;
  }
  search_end(h, n_steps_out, st);
  hipLaunchKernelGGL(beam_gather_kernel, dim3(cdiv(B * Tm, 256)), dim3(256), 0, st, h->sr_hist[cur], (const int32_t*)nullptr, best_out, B, Tm, 1);
  LAUNCH_OK();
  return RECNET_OK;
}

// ---- N-best beam search on log-probabilities (the reference has no counterpart; DESIGN.md section 11)
static int check_beam(int beam_width, int V, float length_alpha) {
  if (beam_width < 1 || beam_width > 8 || beam_width > V) return fail(RECNET_EINVAL, "beam_width must be in [1, min(8, V)]");
  if (!std::isfinite(length_alpha) || length_alpha < 0.f) return fail(RECNET_EINVAL, "length_alpha must be finite and >= 0");
  return RECNET_OK;
}
// the constraints of the constrained form (DESIGN.md section 12), checked: all off = the unconstrained kernel is launched
struct BeamBans {
  int ngram = 0, min_len = 0, n_banned = 0;
  int32_t banned[16] = {};
  bool on() const { return ngram > 0 || min_len > 0 || n_banned > 0; }
};
// ranges (Tm = caption_max_len + 1), distinct ids in [0, V) without <EOS>, and room for beam_width offered tokens on every live
// hypothesis: it bans at most n_banned + t_max + 1 tokens (t_max: the last step the call runs)
static int check_beam_bans(int no_repeat_ngram, int min_length, const int32_t* banned, int n_banned, int beam_width, int V, int Tm,
                           int t_max, BeamBans* out) {
  if (no_repeat_ngram < 0 || no_repeat_ngram > Tm - 1) return fail(RECNET_EINVAL, "no_repeat_ngram must be in [0, caption_max_len]");
  if (min_length < 0 || min_length > Tm - 1) return fail(RECNET_EINVAL, "min_length must be in [0, caption_max_len]");
  if (n_banned < 0 || n_banned > 16) return fail(RECNET_EINVAL, "n_banned must be in [0, 16]");
  if (n_banned > 0 && !banned) return fail(RECNET_EINVAL, "null argument");
  out->ngram = no_repeat_ngram; out->min_len = min_length; out->n_banned = n_banned;
  for (int k = 0; k < n_banned; ++k) {
    if (banned[k] < 0 || banned[k] >= V) return fail(RECNET_EINVAL, "banned tokens must be in [0, V)");
    if (banned[k] == 2) return fail(RECNET_EINVAL, "<EOS> cannot be banned");
    for (int j = 0; j < k; ++j)
      if (banned[j] == banned[k]) return fail(RECNET_EINVAL, "banned tokens must be distinct");
    out->banned[k] = banned[k];
  }
  if (out->on() && (long)beam_width + n_banned + t_max + 1 > (long)V)
    return fail(RECNET_EINVAL, "the vocabulary is too small for these constraints: beam_width + n_banned + steps + 1 must not exceed V");
  if (out->on() && (size_t)(8 + 8 * bs_ban_stride(t_max)) * 4 > 48 * 1024) return fail(RECNET_EINVAL, "caption_max_len too large for the ban lists");
  return RECNET_OK;
}
// bans == nullptr or all off: the unconstrained instantiation; else the constrained one on hist [nb][rows][Tm] at step t
// n_groups > 1 (it divides bw, nb is 1 or bw): the grouped selection of DESIGN.md section 14 at group width bw / n_groups
static void launch_beam_select(const float* logits, const float* cum, const int32_t* fin, int nb, int rows, int V, int bw, float* vals,
                               int32_t* idx, hipStream_t st, const BeamBans* bans = nullptr, const int64_t* hist = nullptr, int Tm = 0,
                               int t = 0, int n_groups = 1, float diversity_penalty = 0.f) {
  BeamSelCArgs a;
  a.x = logits; a.cum = cum; a.fin = fin; a.nb = nb; a.rows = rows; a.V = V; a.vals = vals; a.idx = idx;
  const bool con = bans && bans->on();
  size_t sm = 0;
  if (con) {
    a.hist = hist; a.Tm = Tm; a.t = t; a.ngram = bans->ngram; a.min_len = bans->min_len; a.n_banned = bans->n_banned;
    for (int k = 0; k < 16; ++k) a.banned[k] = bans->banned[k];
    sm = (size_t)(8 + nb * bs_ban_stride(t)) * 4;
  }
  const BeamSelArgs& u = a;            // (the unconstrained kernels take the base part)
  BeamGrpArgs q;
  q.G = n_groups; q.lam = diversity_penalty;
#define RN_BSEL(W, KERNEL, ...) case W:                                                                       \
    if (con) hipLaunchKernelGGL((KERNEL<W, true>), dim3(rows), dim3(256), sm, st, a, ##__VA_ARGS__);          \
    else hipLaunchKernelGGL((KERNEL<W>), dim3(rows), dim3(256), 0, st, u, ##__VA_ARGS__);                     \
    break;
  if (n_groups > 1) {
    switch (bw / n_groups) {
      RN_BSEL(1, beam_select_groups_kernel, q) RN_BSEL(2, beam_select_groups_kernel, q) RN_BSEL(3, beam_select_groups_kernel, q)
      RN_BSEL(4, beam_select_groups_kernel, q)
    }
  } else {
    switch (bw) {
      RN_BSEL(1, beam_select_kernel) RN_BSEL(2, beam_select_kernel) RN_BSEL(3, beam_select_kernel) RN_BSEL(4, beam_select_kernel)
      RN_BSEL(5, beam_select_kernel) RN_BSEL(6, beam_select_kernel) RN_BSEL(7, beam_select_kernel) RN_BSEL(8, beam_select_kernel)
    }
  }
#undef RN_BSEL
}

static int check_select_rows(const float* logits, const float* cum, const int32_t* finished, int nb, int rows, int V, int beam_width,
                             const float* vals_out, const int32_t* idx_out) {
  if (!logits || !cum || !finished || !vals_out || !idx_out) return fail(RECNET_EINVAL, "null argument");
  if (rows < 1 || V < 1 || nb < 1 || nb > 8) return fail(RECNET_EINVAL, "rows and V must be positive, nb in [1, 8]");
  if ((long)nb * V > 0x7fffffffL) return fail(RECNET_EINVAL, "nb * V must fit an int32 index");
  return check_beam(beam_width, V, 0.f);
}

// the groups of the diverse form (DESIGN.md section 14), checked: one group = the selection as it was
static int check_beam_groups(int beam_width, int n_groups, float diversity_penalty) {
  if (n_groups < 1 || beam_width % n_groups != 0) return fail(RECNET_EINVAL, "n_groups must be at least 1 and divide beam_width");
  if (!std::isfinite(diversity_penalty) || diversity_penalty < 0.f) return fail(RECNET_EINVAL, "diversity_penalty must be finite and >= 0");
  return RECNET_OK;
}

// The one body of the three selection exports below, which differ in what they hand in; diverse: the diverse export, the only one
// that checks the groups and ties nb to the width (the other two pass one group and any nb in [1, 8]).
static int beam_select_rows_run(recnet_handle* h, const float* logits, const float* cum, const int32_t* finished, const int64_t* hist,
                                int nb, int rows, int V, int Tm, int t, int beam_width, bool diverse, int n_groups, float diversity_penalty,
                                int no_repeat_ngram, int min_length, const int32_t* banned, int n_banned, float* vals_out, int32_t* idx_out,
                                void* stream) {
  REQUIRE_WS(h);
  int r = check_select_rows(logits, cum, finished, nb, rows, V, beam_width, vals_out, idx_out); if (r) return r;
  if (diverse) {
    r = check_beam_groups(beam_width, n_groups, diversity_penalty); if (r) return r;
    if (nb != 1 && nb != beam_width) return fail(RECNET_EINVAL, "nb must be 1 or beam_width");
  }
  if (Tm < 1 || t < 0 || t >= Tm) return fail(RECNET_EINVAL, "Tm must be positive and t in [0, Tm)");
  BeamBans bans;
  r = check_beam_bans(no_repeat_ngram, min_length, banned, n_banned, beam_width, V, Tm, t, &bans); if (r) return r;
  if (no_repeat_ngram > 0 && !hist) return fail(RECNET_EINVAL, "null argument");
  launch_beam_select(logits, cum, finished, nb, rows, V, beam_width, vals_out, idx_out, (hipStream_t)stream, &bans, hist, Tm, t, n_groups,
                     diversity_penalty);
  LAUNCH_OK();
  return RECNET_OK;
}

// (all constraints off and a step inside a history of one: the unconstrained kernel, as recnet_beam_search_nbest forwards below)
int recnet_beam_select_rows(recnet_handle* h, const float* logits, const float* cum, const int32_t* finished, int32_t nb,
                            int32_t rows, int32_t V, int32_t beam_width, float* vals_out, int32_t* idx_out, void* stream) {
  return beam_select_rows_run(h, logits, cum, finished, nullptr, nb, rows, V, 1, 0, beam_width, false, 1, 0.f, 0, 0, nullptr, 0, vals_out,
                              idx_out, stream);
}
int recnet_beam_select_rows_constrained(recnet_handle* h, const float* logits, const float* cum, const int32_t* finished,
                                        const int64_t* hist, int32_t nb, int32_t rows, int32_t V, int32_t Tm, int32_t t,
                                        int32_t beam_width, int32_t no_repeat_ngram, int32_t min_length, const int32_t* banned,
                                        int32_t n_banned, float* vals_out, int32_t* idx_out, void* stream) {
  return beam_select_rows_run(h, logits, cum, finished, hist, nb, rows, V, Tm, t, beam_width, false, 1, 0.f, no_repeat_ngram, min_length,
                              banned, n_banned, vals_out, idx_out, stream);
}
int recnet_beam_select_rows_diverse(recnet_handle* h, const float* logits, const float* cum, const int32_t* finished,
                                    const int64_t* hist, int32_t nb, int32_t rows, int32_t V, int32_t Tm, int32_t t, int32_t beam_width,
                                    int32_t n_groups, float diversity_penalty, int32_t no_repeat_ngram, int32_t min_length,
                                    const int32_t* banned, int32_t n_banned, float* vals_out, int32_t* idx_out, void* stream) {
  return beam_select_rows_run(h, logits, cum, finished, hist, nb, rows, V, Tm, t, beam_width, true, n_groups, diversity_penalty,
                              no_repeat_ngram, min_length, banned, n_banned, vals_out, idx_out, stream);
}

// ---- ensemble decoding (the reference has no counterpart; DESIGN.md section 19): M decoders, their rows mixed into one row of logits
// the checked weights of an ensemble: normalised to sum 1 in float64, and their logs
struct EnsMix { int M = 1, geo = 0; float w[ENS_MAX_M] = {}, lw[ENS_MAX_M] = {}; };
static int check_ens_mix(int M, const float* weights, int mode, EnsMix* e) {
  if (M < 1 || M > ENS_MAX_M) return fail(RECNET_EINVAL, "an ensemble has between 1 and 8 members");
  if (mode != RECNET_ENS_ARITHMETIC && mode != RECNET_ENS_GEOMETRIC) return fail(RECNET_EINVAL, "unknown ensemble mode");
  double sum = 0.0;
  for (int m = 0; m < M; ++m) {
    const float w = weights ? weights[m] : 1.f;
    if (!(w > 0.f) || !std::isfinite(w)) return fail(RECNET_EINVAL, "ensemble weights must be positive and finite");
    sum += (double)w;
  }
  e->M = M; e->geo = mode == RECNET_ENS_GEOMETRIC;
  for (int m = 0; m < M; ++m) {
    const double w = (double)(weights ? weights[m] : 1.f) / sum;
    e->w[m] = (float)w; e->lw[m] = (float)std::log(w);
  }
  return RECNET_OK;
}
// the members: distinct handles with a workspace and a bound decoder, on one device, that agree on B, F, D, V and Tm
static int check_ens_members(recnet_handle* const* hs, int M) {
  if (!hs) return fail(RECNET_EINVAL, "null argument");
  if (M < 1 || M > ENS_MAX_M) return fail(RECNET_EINVAL, "an ensemble has between 1 and 8 members");
  int dev0 = -1;
  for (int m = 0; m < M; ++m) {
    recnet_handle* h = hs[m];
    if (!h) return fail(RECNET_EINVAL, "null ensemble member");
    REQUIRE_WS(h);
    if (!h->dec_bound) return fail(RECNET_ESTATE, "decoder not bound");
    for (int j = 0; j < m; ++j)
      if (hs[j] == h) return fail(RECNET_EINVAL, "ensemble members must be distinct handles (each keeps its own state)");
    if (h->B != hs[0]->B || h->F != hs[0]->F || h->D != hs[0]->D || h->V != hs[0]->V || h->Tm != hs[0]->Tm)
      return fail(RECNET_EINVAL, "ensemble members must agree on B, F, D, V and caption_max_len");
    if (M > 1) {
      hipPointerAttribute_t at;
      if (hipPointerGetAttributes(&at, h->ws) != hipSuccess) { (void)hipGetLastError(); return fail(RECNET_EINVAL, "ensemble member: workspace is not device memory"); }
      if (m == 0) dev0 = at.device;
      else if (at.device != dev0) return fail(RECNET_EINVAL, "ensemble members must live on one device");
    }
  }
  return RECNET_OK;
}
// y [rows][V] from the members' rows x[m] [rows][V]; y may be x[0]
static void launch_ensemble_mix(const EnsMix& e, const float* const* x, int rows, int V, float* y, hipStream_t st) {
  EnsMixArgs a;
  a.M = e.M; a.V = V; a.geo = e.geo; a.y = y;
  bool vec = (V & 3) == 0 && (((uintptr_t)y) & 15) == 0;
  for (int m = 0; m < ENS_MAX_M; ++m) {
    a.x[m] = m < e.M ? x[m] : nullptr; a.w[m] = m < e.M ? e.w[m] : 0.f; a.lw[m] = m < e.M ? e.lw[m] : 0.f;
    vec = vec && (((uintptr_t)a.x[m]) & 15) == 0;
  }
  const size_t floats = (size_t)e.M * ens_row_stride(V);
  const bool res = floats <= ENS_LDS_FLOATS;
  const size_t sm = res ? floats * 4 : 0;
#define RN_ENS(RES, VEC) do {                                                                                             \
    static bool attr_done = false;                                                                                        \
    if (RES && !attr_done) {                                                                                              \
      hipFuncSetAttribute(reinterpret_cast<const void*>(ensemble_mix_rows_kernel<RES, VEC>), hipFuncAttributeMaxDynamicSharedMemorySize, ENS_LDS_FLOATS * 4); \
      attr_done = true;                                                                                                   \
    }                                                                                                                     \
    hipLaunchKernelGGL((ensemble_mix_rows_kernel<RES, VEC>), dim3(rows), dim3(256), sm, st, a);                           \
  } while (0)
  if (res) { if (vec) RN_ENS(true, 4); else RN_ENS(true, 1); }
  else { if (vec) RN_ENS(false, 4); else RN_ENS(false, 1); }
#undef RN_ENS
}

int recnet_ensemble_mix_rows(recnet_handle* h, const float* const* logits, int32_t M, const float* weights, int32_t mode, int32_t rows,
                             int32_t V, float* y_out, void* stream) {
  REQUIRE_WS(h);
  if (!logits || !y_out) return fail(RECNET_EINVAL, "null argument");
  EnsMix e;
  int r = check_ens_mix(M, weights, mode, &e); if (r) return r;
  if (rows < 1 || V < 1) return fail(RECNET_EINVAL, "rows and V must be positive");
  const size_t n = (size_t)rows * V;
  for (int m = 0; m < M; ++m) {
    if (!logits[m]) return fail(RECNET_EINVAL, "null argument");
    const bool apart = logits[m] + n <= y_out || y_out + n <= logits[m];
    if (!apart && !(m == 0 && logits[0] == y_out)) return fail(RECNET_EINVAL, "y_out may be the rows of member 0 or overlap none");
  }
  launch_ensemble_mix(e, logits, rows, V, y_out, (hipStream_t)stream);
  LAUNCH_OK();
  return RECNET_OK;
}

// The loop of the N-best searches on checked arguments.  group_out (may be null): the group of each returned rank.  hs[0 .. mix.M):
// the members (one: the single-model search, which launches what it always did).  Every member runs the step on the tokens of
// member 0 and keeps its own state; their rows are mixed into member 0's, the selection and member 0's regather are unchanged, the
// other members regather their states by member 0's decisions.
static void beam_search_nbest_run(recnet_handle* const* hs, const EnsMix& mix, const float* enc, int bw, float length_alpha,
                                  const BeamBans& bans, int n_groups, float diversity_penalty, int64_t* tokens_out, float* cum_out,
                                  int32_t* len_out, float* score_out, int32_t* group_out, int32_t* n_steps_out, hipStream_t st) {
  recnet_handle* h = hs[0];
  const int B = h->B, V = h->V, Tm = h->Tm, M = mix.M;
  const float* x[ENS_MAX_M];
  for (int m = 0; m < M; ++m) { search_begin(hs[m], enc, n_steps_out, m == 0 ? 0 : -1, st); x[m] = hs[m]->sr_scores; }
  int cur = 0, nb = 1;
  for (int t = 0; t < Tm; ++t) {   // all nb * B hypotheses in one decode step, the captions' Uv / P shared by their beams
    for (int m = 0; m < M; ++m) {
      recnet_handle* g = hs[m];
      dec_step(g, nb * B, B, dec_rows_beams(g), h->sr_tok[cur], g->sr_h[cur], g->sr_c[cur], g->sr_scores, g->sr_hn, g->sr_cn, 0, t, st);
    }
    if (M > 1) launch_ensemble_mix(mix, x, nb * B, V, h->sr_scores, st);
    launch_beam_select(h->sr_scores, h->sr_cum[cur], h->sr_eos[cur], nb, B, V, bw, h->sr_vals, h->sr_idx, st, &bans, h->sr_hist[cur], Tm, t,
                       n_groups, diversity_penalty);
    hipLaunchKernelGGL(beam_update_kernel<true>, dim3(bw, B), dim3(128), 0, st, beam_update_args(h, bw, t, cur, nullptr));
    for (int m = 1; m < M; ++m) {
      recnet_handle* g = hs[m];
      hipLaunchKernelGGL(beam_regather_state_kernel, dim3(bw, B), dim3(128), 0, st, (const int32_t*)h->sr_idx, B, g->H, V, bw,
                         (const float*)g->sr_hn, (const float*)(g->dgru ? nullptr : g->sr_cn), g->sr_h[cur ^ 1], g->sr_c[cur ^ 1]);
    }
    hipLaunchKernelGGL(search_stop_kernel, dim3(1), dim3(256), 0, st, (const int64_t*)nullptr, h->sr_eos[cur ^ 1], bw * B, t, n_steps_out);
    cur ^= 1; nb = bw;
  }
  search_end(h, n_steps_out, st);
  hipLaunchKernelGGL(beam_nbest_rank_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, h->sr_cum[cur], h->sr_eos[cur], n_steps_out, B, bw,
                     length_alpha, cum_out, len_out, score_out, h->bs_order);
  hipLaunchKernelGGL(beam_gather_kernel, dim3(cdiv(bw * Tm * B, 256)), dim3(256), 0, st, h->sr_hist[cur], h->bs_order, tokens_out,
                     B, Tm, bw);
  if (group_out)
    hipLaunchKernelGGL(beam_group_kernel, dim3(cdiv(bw * B, 256)), dim3(256), 0, st, (const int32_t*)h->bs_order, bw / n_groups, bw * B, group_out);
}

// the checks every N-best search makes on its arguments behind those on its handle(s)
static int check_nbest_args(const recnet_handle* h, const float* enc, int beam_width, float length_alpha, int n_groups, float diversity_penalty,
                            int no_repeat_ngram, int min_length, const int32_t* banned, int n_banned, const void* tokens_out,
                            const void* cum_out, const void* len_out, const void* score_out, const void* n_steps_out, BeamBans* bans) {
  if (!(enc && tokens_out && cum_out && len_out && score_out && n_steps_out)) return fail(RECNET_EINVAL, "null argument");
  int r = check_beam(beam_width, h->V, length_alpha); if (r) return r;
  r = check_beam_groups(beam_width, n_groups, diversity_penalty); if (r) return r;
  return check_beam_bans(no_repeat_ngram, min_length, banned, n_banned, beam_width, h->V, h->Tm, h->Tm - 1, bans);
}

int recnet_beam_search_nbest_ensemble(recnet_handle* const* hs, int32_t M, const float* weights, int32_t mode, const float* enc,
                                      int32_t beam_width, float length_alpha, int32_t n_groups, float diversity_penalty,
                                      int32_t no_repeat_ngram, int32_t min_length, const int32_t* banned, int32_t n_banned,
                                      int64_t* tokens_out, float* cum_out, int32_t* len_out, float* score_out, int32_t* group_out,
                                      int32_t* n_steps_out, void* stream) {
  int r = check_ens_members(hs, M); if (r) return r;
  EnsMix mix;
  r = check_ens_mix(M, weights, mode, &mix); if (r) return r;
  BeamBans bans;
  r = check_nbest_args(hs[0], enc, beam_width, length_alpha, n_groups, diversity_penalty, no_repeat_ngram, min_length, banned, n_banned,
                       tokens_out, cum_out, len_out, score_out, n_steps_out, &bans); if (r) return r;
  beam_search_nbest_run(hs, mix, enc, beam_width, length_alpha, bans, n_groups, diversity_penalty, tokens_out, cum_out, len_out, score_out,
                        group_out, n_steps_out, (hipStream_t)stream);
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_beam_search_nbest_diverse(recnet_handle* h, const float* enc, int32_t beam_width, float length_alpha, int32_t n_groups,
                                     float diversity_penalty, int32_t no_repeat_ngram, int32_t min_length, const int32_t* banned,
                                     int32_t n_banned, int64_t* tokens_out, float* cum_out, int32_t* len_out, float* score_out,
                                     int32_t* group_out, int32_t* n_steps_out, void* stream) {
  int r = search_check(h, enc && tokens_out && cum_out && len_out && score_out && n_steps_out); if (r) return r;
  BeamBans bans;
  r = check_nbest_args(h, enc, beam_width, length_alpha, n_groups, diversity_penalty, no_repeat_ngram, min_length, banned, n_banned,
                       tokens_out, cum_out, len_out, score_out, n_steps_out, &bans); if (r) return r;
  beam_search_nbest_run(&h, EnsMix(), enc, beam_width, length_alpha, bans, n_groups, diversity_penalty, tokens_out, cum_out, len_out, score_out,
                        group_out, n_steps_out, (hipStream_t)stream);
  LAUNCH_OK();
  return RECNET_OK;
}

// (one group, which every width passes, and no group output: the search as it was)
int recnet_beam_search_nbest_constrained(recnet_handle* h, const float* enc, int32_t beam_width, float length_alpha,
                                         int32_t no_repeat_ngram, int32_t min_length, const int32_t* banned, int32_t n_banned,
                                         int64_t* tokens_out, float* cum_out, int32_t* len_out, float* score_out, int32_t* n_steps_out,
                                         void* stream) {
  return recnet_beam_search_nbest_diverse(h, enc, beam_width, length_alpha, 1, 0.f, no_repeat_ngram, min_length, banned, n_banned, tokens_out,
                                          cum_out, len_out, score_out, nullptr, n_steps_out, stream);
}

int recnet_beam_search_nbest(recnet_handle* h, const float* enc, int32_t beam_width, float length_alpha, int64_t* tokens_out,
                             float* cum_out, int32_t* len_out, float* score_out, int32_t* n_steps_out, void* stream) {
  return recnet_beam_search_nbest_constrained(h, enc, beam_width, length_alpha, 0, 0, nullptr, 0, tokens_out, cum_out, len_out, score_out,
                                              n_steps_out, stream);
}

// ---- stochastic beam search (the reference has no counterpart; DESIGN.md section 21): bw captions per video drawn without
// replacement from the model's sequence distribution, in one search of width bw
static int check_sbs(int beam_width, int V, float temperature) {
  if (beam_width < 1 || beam_width > 8 || beam_width > V) return fail(RECNET_EINVAL, "beam_width must be in [1, min(8, V)]");
  if (!(temperature > 0.f) || !std::isfinite(temperature)) return fail(RECNET_EINVAL, "temperature must be positive and finite");
  return RECNET_OK;
}
// one selection step: (phi, G, finished) [nb][rows] and logits [nb][rows][V] into vals = phi, gum_out = G, idx [rows][bw]
static void launch_sbs_select(const float* logits, const float* cum, const float* gum, const int32_t* fin, int nb, int rows, int V, int bw,
                              float temperature, uint32_t seed, int t, float* vals, float* gum_out, int32_t* idx, hipStream_t st) {
  SbsSelArgs a;
  a.x = logits; a.cum = cum; a.gum = gum; a.fin = fin; a.nb = nb; a.rows = rows; a.V = V; a.t = t;
  a.temp = temperature; a.key = rn_site_key(seed, RN_SITE_SAMPLE); a.vals = vals; a.gum_out = gum_out; a.idx = idx;
#define RN_SBS(W) case W: hipLaunchKernelGGL((sbs_select_kernel<W>), dim3(rows), dim3(256), 0, st, a); break;
  switch (bw) { RN_SBS(1) RN_SBS(2) RN_SBS(3) RN_SBS(4) RN_SBS(5) RN_SBS(6) RN_SBS(7) RN_SBS(8) }
#undef RN_SBS
}

int recnet_sbs_select_rows(recnet_handle* h, const float* logits, const float* cum, const float* gum, const int32_t* finished, int32_t nb,
                           int32_t rows, int32_t V, int32_t beam_width, float temperature, uint32_t seed, int32_t t, float* vals_out,
                           float* gum_out, int32_t* idx_out, void* stream) {
  REQUIRE_WS(h);
  if (!logits || !cum || !gum || !finished || !vals_out || !gum_out || !idx_out) return fail(RECNET_EINVAL, "null argument");
  if (rows < 1 || V < 1 || nb < 1 || nb > 8 || t < 0) return fail(RECNET_EINVAL, "rows and V must be positive, nb in [1, 8], t non-negative");
  if ((long)nb * V > 0x7fffffffL) return fail(RECNET_EINVAL, "nb * V must fit an int32 index");
  int r = check_sbs(beam_width, V, temperature); if (r) return r;
  launch_sbs_select(logits, cum, gum, finished, nb, rows, V, beam_width, temperature, seed, t, vals_out, gum_out, idx_out, (hipStream_t)stream);
  LAUNCH_OK();
  return RECNET_OK;
}

// beam_search_nbest_run's loop with the stochastic selection: the same batched step, regather (which carries G beside phi), member
// regathers and stop rule; no constraints, no groups.  The slots leave every step in rank order, so the outputs are the slots.
static void sbs_run(recnet_handle* const* hs, const EnsMix& mix, const float* enc, int bw, float temperature, uint32_t seed,
                    int64_t* tokens_out, float* cum_out, int32_t* len_out, float* gum_out, int32_t* n_steps_out, hipStream_t st) {
  recnet_handle* h = hs[0];
  const int B = h->B, V = h->V, Tm = h->Tm, M = mix.M;
  const float* x[ENS_MAX_M];
  for (int m = 0; m < M; ++m) { search_begin(hs[m], enc, n_steps_out, m == 0 ? 0 : -1, st); x[m] = hs[m]->sr_scores; }
  hipMemsetAsync(h->sr_gum[0], 0, (size_t)B * 4, st);
  int cur = 0, nb = 1;
  for (int t = 0; t < Tm; ++t) {
    for (int m = 0; m < M; ++m) {
      recnet_handle* g = hs[m];
      dec_step(g, nb * B, B, dec_rows_beams(g), h->sr_tok[cur], g->sr_h[cur], g->sr_c[cur], g->sr_scores, g->sr_hn, g->sr_cn, 0, t, st);
    }
    if (M > 1) launch_ensemble_mix(mix, x, nb * B, V, h->sr_scores, st);
    launch_sbs_select(h->sr_scores, h->sr_cum[cur], h->sr_gum[cur], h->sr_eos[cur], nb, B, V, bw, temperature, seed, t, h->sr_vals,
                      h->sr_gvals, h->sr_idx, st);
    BeamUpdArgs u = beam_update_args(h, bw, t, cur, nullptr);
    u.gum_vals = h->sr_gvals; u.gum_new = h->sr_gum[cur ^ 1];
    hipLaunchKernelGGL(beam_update_kernel<true>, dim3(bw, B), dim3(128), 0, st, u);
    for (int m = 1; m < M; ++m) {
      recnet_handle* g = hs[m];
      hipLaunchKernelGGL(beam_regather_state_kernel, dim3(bw, B), dim3(128), 0, st, (const int32_t*)h->sr_idx, B, g->H, V, bw,
                         (const float*)g->sr_hn, (const float*)(g->dgru ? nullptr : g->sr_cn), g->sr_h[cur ^ 1], g->sr_c[cur ^ 1]);
    }
    hipLaunchKernelGGL(search_stop_kernel, dim3(1), dim3(256), 0, st, (const int64_t*)nullptr, h->sr_eos[cur ^ 1], bw * B, t, n_steps_out);
    cur ^= 1; nb = bw;
  }
  search_end(h, n_steps_out, st);
  hipLaunchKernelGGL(sbs_finish_kernel, dim3(cdiv(bw * B, 256)), dim3(256), 0, st, (const float*)h->sr_cum[cur], (const float*)h->sr_gum[cur],
                     (const int32_t*)h->sr_eos[cur], (const int32_t*)n_steps_out, B, bw, cum_out, len_out, gum_out, h->bs_order);
  hipLaunchKernelGGL(beam_gather_kernel, dim3(cdiv(bw * Tm * B, 256)), dim3(256), 0, st, h->sr_hist[cur], h->bs_order, tokens_out,
                     B, Tm, bw);
}

int recnet_stochastic_beam_search(recnet_handle* h, const float* enc, int32_t beam_width, float temperature, uint32_t seed,
                                  int64_t* tokens_out, float* cum_out, int32_t* len_out, float* gum_out, int32_t* n_steps_out, void* stream) {
  int r = search_check(h, enc && tokens_out && cum_out && len_out && gum_out && n_steps_out); if (r) return r;
  r = check_sbs(beam_width, h->V, temperature); if (r) return r;
  sbs_run(&h, EnsMix(), enc, beam_width, temperature, seed, tokens_out, cum_out, len_out, gum_out, n_steps_out, (hipStream_t)stream);
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_stochastic_beam_search_ensemble(recnet_handle* const* hs, int32_t M, const float* weights, int32_t mode, const float* enc,
                                           int32_t beam_width, float temperature, uint32_t seed, int64_t* tokens_out, float* cum_out,
                                           int32_t* len_out, float* gum_out, int32_t* n_steps_out, void* stream) {
  int r = check_ens_members(hs, M); if (r) return r;
  EnsMix mix;
  r = check_ens_mix(M, weights, mode, &mix); if (r) return r;
  if (!(enc && tokens_out && cum_out && len_out && gum_out && n_steps_out)) return fail(RECNET_EINVAL, "null argument");
  r = check_sbs(beam_width, hs[0]->V, temperature); if (r) return r;
  sbs_run(hs, mix, enc, beam_width, temperature, seed, tokens_out, cum_out, len_out, gum_out, n_steps_out, (hipStream_t)stream);
  LAUNCH_OK();
  return RECNET_OK;
}

// recnet_score_captions over the members: score_logits of each, one mix over the T * B rows into member 0's, then the row kernel at
// temperature 1 and the per-caption sums, unchanged.  One member: the kernels of recnet_score_captions at temperature 1.
int recnet_score_captions_ensemble(recnet_handle* const* hs, int32_t M, const float* weights, int32_t mode, const float* enc,
                                   const int64_t* tokens, int32_t T, float* logprobs_out, float* caption_logprob_out, int32_t* length_out,
                                   void* stream) {
  int r = check_ens_members(hs, M); if (r) return r;
  EnsMix mix;
  r = check_ens_mix(M, weights, mode, &mix); if (r) return r;
  if (check_T(hs[0], T)) return fail(RECNET_EINVAL, "T out of range");
  if (!tokens || !logprobs_out || !caption_logprob_out || !length_out) return fail(RECNET_EINVAL, "null argument");
  for (int m = 0; m < M; ++m) FLUSH_PENDING(hs[m], stream);
  hipStream_t st = (hipStream_t)stream;
  recnet_handle* h = hs[0];
  const float* x[ENS_MAX_M];
  for (int m = 0; m < M; ++m) {
    r = score_logits(hs[m], enc, tokens, T, st); if (r) return r;
    x[m] = hs[m]->logits;
  }
  if (M > 1) launch_ensemble_mix(mix, x, T * h->B, h->V, h->logits, st);
  launch_logprob_rows(h->logits, tokens, T * h->B, h->V, 1.f, logprobs_out, st);
  hipLaunchKernelGGL(caption_logprob_kernel, dim3(cdiv(h->B, 256)), dim3(256), 0, st, logprobs_out, tokens, T, h->B, caption_logprob_out, length_out);
  LAUNCH_OK();
  return RECNET_OK;
}

// ---- consensus (minimum-Bayes-risk) scoring by n-gram overlap (the reference has no counterpart; DESIGN.md section 16)
// One launch.  Grid: the caption columns times tiles of HT hypotheses, HT chosen so that about two workgroups per CU exist (B = 100
// alone would leave most of the chip idle); the integers do not depend on the tiling, so neither do the outputs.
int recnet_consensus_rows(recnet_handle* h, const int64_t* hyp, int32_t N_h, int32_t T_h, const int64_t* ref, int32_t N_r, int32_t T_r,
                          int32_t B, const float* weights, double sigma, double* util_out, double* sim_out, int32_t* counts_out,
                          int32_t* q_hyp_out, int32_t* q_ref_out, int32_t* len_hyp_out, int32_t* len_ref_out, void* stream) {
  REQUIRE_WS(h);
  if (!hyp || !util_out) return fail(RECNET_EINVAL, "null argument");
  if (!ref) { N_r = N_h; T_r = T_h; }
  if (N_h < 1 || N_h > 32 || N_r < 1 || N_r > 32) return fail(RECNET_EINVAL, "N_h and N_r must be in [1, 32]");
  if (T_h < 1 || T_h > 64 || T_r < 1 || T_r > 64) return fail(RECNET_EINVAL, "T_h and T_r must be in [1, 64]");
  if (B < 1) return fail(RECNET_EINVAL, "B must be positive");
  if (!(sigma > 0.0) || !std::isfinite(sigma)) return fail(RECNET_EINVAL, "sigma must be positive and finite");
  ConsensusArgs a;
  a.hyp = hyp; a.ref = ref; a.w = weights; a.sigma = sigma; a.Nh = N_h; a.Nr = N_r; a.Th = T_h; a.Tr = T_r; a.B = B;
  a.util = util_out; a.sim = sim_out; a.counts = counts_out; a.q_hyp = q_hyp_out; a.q_ref = q_ref_out; a.len_hyp = len_hyp_out;
  a.len_ref = len_ref_out;
  int tiles = cdiv(2L * (h->ncu > 0 ? h->ncu : 256), B);
  if (tiles > N_h) tiles = N_h;
  a.HT = cdiv(N_h, tiles);
  tiles = cdiv(N_h, a.HT);
  const size_t sm = (size_t)cs_lds_words(N_r, T_r, T_h, a.HT) * 4;
  hipLaunchKernelGGL(consensus_rows_kernel, dim3(B, tiles), dim3(256), sm, (hipStream_t)stream, a);
  LAUNCH_OK();
  return RECNET_OK;
}
