// C ABI: sequence-level forward / backward, optimiser, and the fused train step with its stream orchestration.
// Part of api.hip (one translation unit; see the include list there).

int recnet_set_deferred_reconstructor_update(recnet_handle* h, int32_t on, void* stream) {
  REQUIRE_WS(h);
  FLUSH_PENDING(h, stream);
  h->defer_rec = on ? (on == 2 ? 2 : 1) : 0;      // 2: only the recurrent weights' update is deferred (include/recnet_hip.h)
  LAUNCH_OK();
  return RECNET_OK;
}
int recnet_flush(recnet_handle* h, void* stream) {
  REQUIRE_WS(h);
  int r = flush_pending(h, (hipStream_t)stream, 1); if (r) return r;
  LAUNCH_OK();
  return RECNET_OK;
}
int recnet_set_dp_overlap(recnet_handle* h, int32_t on) {
  if (!h) return fail(RECNET_EINVAL, "null handle");
  h->ss.dp_overlap = on ? 1 : 0;
  return RECNET_OK;
}
int recnet_join_side(recnet_handle* h, void* stream) {
  REQUIRE_WS(h);
  if (h->ss.side_open && h->s2) { hipEventRecord(h->ev[EV_REC_DW_JOIN], h->s2); hipStreamWaitEvent((hipStream_t)stream, h->ev[EV_REC_DW_JOIN], 0); }
  h->ss.side_open = 0;
  LAUNCH_OK();
  return RECNET_OK;
}
int recnet_abort_step(recnet_handle* h) {
  if (!h) return fail(RECNET_EINVAL, "null handle");
  sched_reset(h);
  return RECNET_OK;
}
int recnet_mark_pending(recnet_handle* h) {
  if (!h) return fail(RECNET_EINVAL, "null handle");
  if (h->defer_rec) { h->maybe_pending = 1; h->images_maybe_stale = 1; }
  return RECNET_OK;
}

int recnet_forward_decoder(recnet_handle* h, const float* enc, const int64_t* targets, int32_t T,
                           const float* step_weight, int32_t train, uint32_t seed, float* hiddens_out,
                           recnet_scalars* scalars, void* stream) {
  REQUIRE_WS(h);
  if (!h->dec_bound) return fail(RECNET_ESTATE, "decoder not bound");
  if (!enc || !targets || !step_weight) return fail(RECNET_EINVAL, "null argument");
  if (check_T(h, T)) return fail(RECNET_EINVAL, "T out of range");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, st, h->ctrl, seed);
  int r = fwd_decoder(h, enc, targets, T, step_weight, train, hiddens_out, st); if (r) return r;
  if (scalars) hipLaunchKernelGGL(export_scalars_kernel, dim3(1), dim3(1), 0, st, h->scal, scalars);
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_forward_decoder_free(recnet_handle* h, const float* enc, const int64_t* targets, int32_t T,
                                const float* step_weight, int32_t train, uint32_t seed, float* hiddens_out,
                                int64_t* output_indices, recnet_scalars* scalars, void* stream) {
  REQUIRE_WS(h);
  if (!h->dec_bound) return fail(RECNET_ESTATE, "decoder not bound");
  if (!enc || !targets || !step_weight || !output_indices) return fail(RECNET_EINVAL, "null argument");
  if (check_T(h, T)) return fail(RECNET_EINVAL, "T out of range");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, st, h->ctrl, seed);
  int r = fwd_decoder(h, enc, targets, T, step_weight, train, hiddens_out, st, output_indices); if (r) return r;
  if (scalars) hipLaunchKernelGGL(export_scalars_kernel, dim3(1), dim3(1), 0, st, h->scal, scalars);
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_forward_reconstructor(recnet_handle* h, const float* enc, const float* hiddens, int32_t T,
                                 int32_t train, uint32_t seed, recnet_scalars* scalars, void* stream) {
  REQUIRE_WS(h);
  FLUSH_PENDING(h, stream);
  if (h->kind == RECNET_REC_NONE || !h->rec_bound) return fail(RECNET_ESTATE, "reconstructor not bound");
  if (!enc) return fail(RECNET_EINVAL, "null argument");
  if (check_T(h, T)) return fail(RECNET_EINVAL, "T out of range");
  if (!hiddens && (!h->fwd_dec_done || h->T_last != T)) return fail(RECNET_ESTATE, "no decoder hidden states for this T");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, st, h->ctrl, seed);
  h->ss.xcat_done = 0;          // (this entry point sets its own dropout seed: an operand the decoder chain wrote carries the masks of ITS seed)
  if (hiddens) {   // hidden states handed in by the caller: refresh the fp32 image and its operand copy
    copyf(hiddens, h->Hs, (size_t)T * h->B * h->H, st);
    pack_block(h, h->Hs_lp, h->ldH, hiddens, h->H, T * h->B, h->H, 1.f, st);
    h->ss.mp_done = 0;
  }
  int r = fwd_rec(h, enc, T, train, st); if (r) return r;
  if (scalars) hipLaunchKernelGGL(export_scalars_kernel, dim3(1), dim3(1), 0, st, h->scal, scalars);
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_backward_reconstructor(recnet_handle* h, const float* enc, float grad_scale, float* dhiddens_out, void* stream) {
  REQUIRE_WS(h);
  FLUSH_PENDING(h, stream);
  h->ss.prezeroed = 0;
  if (!h->fwd_rec_done) return fail(RECNET_ESTATE, "backward_reconstructor before forward_reconstructor");
  if (!h->rG.out_weight) return fail(RECNET_ESTATE, "reconstructor gradients not bound");
  hipStream_t st = (hipStream_t)stream;
  float* dh = dhiddens_out ? dhiddens_out : h->dHsrec;
  int r = bwd_rec(h, grad_scale, dh, st);
  if (r) return r;
  if (dhiddens_out) copyf(dhiddens_out, h->dHsrec, (size_t)h->T_last * h->B * h->H, st);
  h->rec_bwd_done = 1;
  (void)enc;
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_backward_decoder(recnet_handle* h, const float* enc, const int64_t* targets, const float* dhiddens,
                            float grad_scale, void* stream) {
  REQUIRE_WS(h);
  h->ss.prezeroed = 0;
  if (!h->fwd_dec_done) return fail(RECNET_ESTATE, "backward_decoder before forward_decoder");
  if (!h->dGd.out_weight) return fail(RECNET_ESTATE, "decoder gradients not bound");
  if (!enc || !targets) return fail(RECNET_EINVAL, "null argument");
  int r = bwd_decoder(h, enc, targets, dhiddens, grad_scale, (hipStream_t)stream); if (r) return r;
  h->fwd_dec_done = 0;   // dlogits were consumed in place
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_add_reg_grad(recnet_handle* h, int32_t which, float grad_scale, void* stream) {
  REQUIRE_WS(h);
  FLUSH_PENDING(h, stream);
  if (which < 0 || which > 1 || !h->og[which].bound) return fail(RECNET_EINVAL, "model not bound");
  OptGroup& o = h->og[which];
  const float lam = which == 0 ? h->c.decoder_lambda_reg : h->c.reconstructor_lambda_reg;
  hipLaunchKernelGGL(add_reg_grad_kernel, dim3(o.nchunks), dim3(256), 0, (hipStream_t)stream, o.d_tab, o.d_chunks, o.d_pnorm, lam * grad_scale);
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_clip_grad_norm(recnet_handle* h, int32_t which, float max_norm, float* total_norm_out, void* stream) {
  REQUIRE_WS(h);
  FLUSH_PENDING(h, stream);
  if (which < 0 || which > 1 || !h->og[which].bound || !h->og[which].tab[0].g) return fail(RECNET_EINVAL, "gradients not bound");
  OptGroup& o = h->og[which];
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sumsq_chunk_kernel, dim3(o.nchunks), dim3(256), 0, st, o.d_tab, o.d_chunks, 1, o.d_pnorm, 0.f, o.d_partial);
  hipLaunchKernelGGL(tensor_norm_kernel, dim3(o.ntens), dim3(256), 0, st, o.d_tab, o.d_partial, o.d_gnorm);
  hipLaunchKernelGGL(norm_finalize_kernel, dim3(1), dim3(64), 0, st, o.d_gnorm, o.ntens, max_norm, h->scal + RN_SCAL_GNORM, h->scal + RN_SCAL_CLIP, (float*)nullptr);
  hipLaunchKernelGGL(scale_grads_kernel, dim3(o.nchunks), dim3(256), 0, st, o.d_tab, o.d_chunks, h->scal + RN_SCAL_CLIP);
  if (total_norm_out) copyf(h->scal + RN_SCAL_GNORM, total_norm_out, 1, st);
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_optimizer_step(recnet_handle* h, int32_t step, int32_t flags, recnet_scalars* scalars, void* stream) {
  REQUIRE_WS(h);
  FLUSH_PENDING(h, stream);
  if (step < 1) return fail(RECNET_EINVAL, "step must be >= 1");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, st, h->ctrl + RN_CTRL_STEP, (uint32_t)step);
  if (h->og[0].bound && h->og[0].tab[0].g) hipLaunchKernelGGL(poison_collect_kernel, dim3(1), dim3(1), 0, st, (const float*)h->og[0].tab[0].g, h->scal + RN_SCAL_POISON);
  int r = optimizer_step(h, flags, st); if (r) return r;
  if (scalars) hipLaunchKernelGGL(export_scalars_kernel, dim3(1), dim3(1), 0, st, h->scal, scalars);
  LAUNCH_OK();
  return RECNET_OK;
}

// Batch-independent work of a step: parameter norms (regulariser values; the optimiser needs them again at the end), the
// reconstructor's gate bias, the zeroing of this step's atomic targets, the frame mean of the features (global
// reconstructor's target).  On the side stream when there is one; EV_HOIST_DONE marks its end.
// The reconstructor's share of the hoisted work: its parameter norms, gate bias and the zeroing of its atomic targets.
// With a deferred reconstructor update they have to follow that update (stream s3, see fwd_bwd_impl).
static void hoist_rec_parts(recnet_handle* h, hipStream_t sn) {
  param_norms(h, 1, h->scal + RN_SCAL_REC_REG, sn);
  gate_bias(h->rP.rnn_bias_ih_l0, h->rP.rnn_bias_hh_l0, h->bsum_r, h->R, h->rgru, sn);
  ZeroList z; z.cnt = 0;
  z.p[z.cnt] = h->rG.out_bias; z.n[z.cnt] = h->R; ++z.cnt;
  z.p[z.cnt] = h->bsum4r; z.n[z.cnt] = (size_t)4 * h->R; ++z.cnt;
  hipLaunchKernelGGL(zero_list_kernel, dim3(64), dim3(256), 0, sn, z);
}
// fork_recorded: the caller (dec_fwd_chain) recorded the fork events EV_HOIST_FORK / EV_S3_FORK itself, in front of its chain launch.
// Returns what the pending reconstructor update returned.
static int hoist_side_work(recnet_handle* h, const HoistWork& w, hipStream_t st, bool fork_recorded) {
  RN_RANGE("recnet: hoisted side work (parameter norms, zeroing, frame mean)");
  const bool split_upd = h->ss.defer_now && h->defer_rec == 2;
  int r = RECNET_OK;
  if (h->ss.defer_now) {
    // forked HERE, i.e. after the decoder prologue has been enqueued: forked at the start of the step the replayed graph
    // ran the whole update in front of the prologue (the prologue's first kernel started 0.5 ms late)
    if (fork_recorded) hipStreamWaitEvent(h->s3, h->ev[EV_S3_FORK], 0); else fork_to(h, EV_S3_FORK, st, h->s3);
    if (h->persist_dec) wait_chain(h, 0, h->s3);      // the pending products start once the decoder chain is resident (wait_chain_kernel)
    r = rec_pending_update(h, h->s3, -1, h->defer_flags);
    // mode 2: only W_hh changes here — its norm (the regulariser's value) follows the update; the gate bias and the zeroing do not
    // depend on it and stay with the ordinary hoisted work below, so that the input-side product of the reconstructor's forward
    // (which needs the bias sum) does not wait for this branch: only the recurrent chain does (fwd_rec_global)
    // (the recurrent chain waits for the UPDATE only, EV_PENDING_DONE; the norm — 35 us of launches behind it — is read by the loss scalars
    // after the chain: EV_WHH_NORM, fwd_rec)
    if (split_upd) { hipEventRecord(h->ev[EV_PENDING_DONE], h->s3); param_norms(h, 1, h->scal + RN_SCAL_REC_REG, h->s3); hipEventRecord(h->ev[EV_WHH_NORM], h->s3); h->ss.rec_norm_late = 1; }
    else { hoist_rec_parts(h, h->s3); hipEventRecord(h->ev[EV_PENDING_DONE], h->s3); }
  }
  if (h->ss.img_defer_now && !h->ss.defer_now) {
    // deferred image refresh (api.hip: img_defer_now): the transposes / fragment packs the previous fused step left out, on the third
    // stream beside the decoder's chain; EV_PENDING_DONE = done (the reconstructor's chains wait for it, fwd_rec_*: rec_wait_pending)
    if (fork_recorded) hipStreamWaitEvent(h->s3, h->ev[EV_S3_FORK], 0); else fork_to(h, EV_S3_FORK, st, h->s3);
    if (h->persist_dec) wait_chain(h, 0, h->s3);
    refresh_images(h, 1, h->s3);
    hipEventRecord(h->ev[EV_PENDING_DONE], h->s3);
  }
  const bool rec = h->kind != RECNET_REC_NONE && !h->ss.defer_now;
  hipStream_t sd = h->s2;
  hipStream_t sn = w.par ? sd : st;
  if (sn != st) { if (fork_recorded) hipStreamWaitEvent(sd, h->ev[EV_HOIST_FORK], 0); else fork_to(h, EV_HOIST_FORK, st, sd); }
  if (sn != st && h->persist_dec) wait_chain(h, 0, sn);      // nothing of this branch before the decoder chain is resident
  param_norms(h, 0, h->scal + RN_SCAL_DEC_REG, sn);
  if (rec) { param_norms(h, 1, h->scal + RN_SCAL_REC_REG, sn); gate_bias(h->rP.rnn_bias_ih_l0, h->rP.rnn_bias_hh_l0, h->bsum_r, h->R, h->rgru, sn); }
  if (split_upd) gate_bias(h->rP.rnn_bias_ih_l0, h->rP.rnn_bias_hh_l0, h->bsum_r, h->R, h->rgru, sn);
  {   // the targets of this step's atomic column sums and of the embedding scatter-add, zeroed in one launch
    ZeroList z; z.cnt = 0;
    auto add = [&](float* p, size_t n) { if (p && n) { z.p[z.cnt] = p; z.n[z.cnt] = n; ++z.cnt; } };
    add(h->dGd.embedding_weight, (size_t)h->V * h->E); add(h->dGd.out_bias, h->V); add(h->bsum4, (size_t)4 * h->H);
    add(h->dGd.attn_b, h->A); add(h->dGd.attn_w_weight, h->A);
    if (rec || split_upd) { add(h->rG.out_bias, h->R); add(h->bsum4r, (size_t)4 * h->R); }
    hipLaunchKernelGGL(zero_list_kernel, dim3(512), dim3(256), 0, sn, z);
    h->ss.prezeroed = 1;
  }
  if (h->kind == RECNET_REC_GLOBAL) {
    hipLaunchKernelGGL(mean_over_f_kernel, dim3(ew_blocks((size_t)h->B * h->D)), dim3(256), 0, sn, w.enc, h->B, h->F, h->D, h->encmean);
    h->ss.encmean_hoisted = 1;
  }
  if (sn != st) hipEventRecord(h->ev[EV_HOIST_DONE], sd);
  return r;
}

// What only needs the decoder's forward pass: vocabulary projection + CE + output-layer gradients (+ the attended
// features for the deferred dW_ih), on the side stream when there is one.
static int side_after_decoder_fwd(recnet_handle* h, const SideWork& w, hipStream_t st, bool fork_recorded) {
  hipStream_t sd = h->overlap ? h->s2 : st;
  const bool par = sd != st;
  // (fork_recorded: the caller — fwd_rec_global — recorded the fork event EV_SIDE_FORK itself, IN FRONT of a chain launch it then enqueued — the side
  // work is enqueued behind that launch on the host but depends only on what preceded it)
  if (par) {
    if (fork_recorded) {
      hipStreamWaitEvent(sd, h->ev[EV_SIDE_FORK], 0);
      // the fork point lies in front of the reconstructor's forward chain, which may still be waiting for something else (mode 2
      // of the deferred update: W_hh's pending update) when this branch becomes runnable: hold it until the chain is resident
      if (h->kind == RECNET_REC_GLOBAL && h->persist_rec) wait_chain(h, 2, sd);
    } else fork_to(h, EV_SIDE_FORK, st, sd);
  }
  h->ss.join_pending = par; h->ss.join_recorded = 0; h->ss.side_tail_open = 0;
  int r = dec_fwd_loss(h, w.targets, w.T, w.stepw, 1, sd);
  // (measured and rejected, round 4: the output layer's own gradients and the attended features beside the BPTT chain instead of
  // here, with the split reconstructor update — the products the BPTT waits for come 17 us earlier, but that window is full
  // and the tail grows by 67 us: C2 1.773 against 1.724 ms)
  if (!r) r = dec_bwd_out(h, 1.0f, sd, 3, w.phase == 0);
  if (!r && par && w.phase != 2) { dec_ctx_rows(h, w.enc, 0, w.T, sd); h->ss.ctx_done = 1; }   // off the tail
  if (h->ss.side_tail_open) hipEventRecord(h->ev[EV_SIDE_TAIL], sd);      // (dec_bwd_out recorded the join the BPTT waits for in front of this branch's rest)
  return r;
}

// The whole forward + backward.  The four dependent chains (decoder fwd, reconstructor fwd, reconstructor bwd,
// decoder bwd) stay on `st`; work that no chain waits for runs on the side stream beside them: the vocabulary
// projection + CE + output-layer gradients while the reconstructor runs, the reconstructor's deferred weight
// gradients while the decoder BPTT runs.  The chains are latency-bound (~1 workgroup per CU), so the batched
// GEMMs fill CUs that would otherwise idle.
// phase 0: everything.  phase 1: up to and including every reconstructor gradient (so a data-parallel caller can
// start all-reducing the reconstructor bucket).  phase 2: the decoder BPTT + its deferred gradients.
// early_opt >= 0 (single-rank fused step): the reconstructor's optimiser step (flags = early_opt) is issued on the side
// stream as soon as its gradients are complete, i.e. it runs under the decoder BPTT; the caller then steps the decoder only.
static int fwd_bwd_impl(recnet_handle* h, const float* enc, const int64_t* targets, int T, const float* stepw, hipStream_t st,
                        int phase, int early_opt) {
  const bool rec = h->kind != RECNET_REC_NONE;
  hipStream_t sd = h->overlap ? h->s2 : st;
  const bool par = sd != st;
  int r;
  bool s3_join = false;
  // total = dec_loss + lambda_recon * rec_loss, and the reconstructor's loss scalars in front of it: scalars only the export at the
  // step's end reads — on the side stream behind the BPTT's fork when there is one (one launch less between the reconstructor's
  // backward and the decoder's BPTT)
  const bool total_late = rec && phase == 0 && par;
  const float* dh = rec ? h->dHsrec : nullptr;
  h->ss.early_opt_done = 0;
  if (phase != 2) h->free_fwd = 0;                 // the fused step is teacher-forced
  if (phase != 2) h->ss.ctx_done = 0;
  // Deferred reconstructor update (opt-in, global reconstructor): the step before left its weight-gradient products and Adam
  // step pending; they run on a third stream under this step's decoder forward chain, followed by the reconstructor's share
  // of the hoisted work (its norms are those of the UPDATED parameters).  EV_PENDING_DONE = all of that done.
  // MEASURED AND NOT THE DEFAULT (round 3, C2): 2.34 ms against 1.95 ms.  The chain kernels need whole CUs (512 registers per
  // lane); a stream of ordinary workgroups that is already running when a chain launches keeps every CU partly occupied and
  // the chain's workgroups wait for hundreds of microseconds to become resident (decoder chain start 125 -> 644 us in the
  // replayed graph), and batched products beside a RUNNING chain cost it +46 us of hand-over latency.  Under the BPTT the
  // same products start after the chain is resident, which is why the immediate form wins.
  // (mode 1 — the whole update — exists for the global reconstructor; mode 2 — the recurrent weights only — for both)
  // (defer_static: everything but the decode length — a property of the handle and of the entry point)
  const bool defer_static = h->defer_rec && (h->kind == RECNET_REC_GLOBAL || (h->defer_rec == 2 && h->kind == RECNET_REC_LOCAL)) && phase == 0 && early_opt >= 0 && par && h->s3 &&
                            (h->defer_rec != 2 || h->split_ok);
  const bool defer = defer_static && (h->defer_rec != 2 || T >= 2);
  // A step that cannot defer completes what the one before it left.  Where the only reason is its decode length (T < 2) the flush is
  // enqueued UNCONDITIONALLY — a captured graph of such a step may be replayed behind a graph that left an update pending, and the
  // device's pending word (RN_CTRL_PENDING) decides inside the kernels whether the update happens (ADVICE r4).  A handle that never defers at
  // its shape (the split does not fit: 28 x 3584, row groups, the fp32 path) leaves nothing pending: only the host's flag counts there
  // (round 5 first enqueued it for those too: +0.4 ms per step at 28 x 3584, +0.7 ms on the fp32 path — products nobody reads).
  if (!defer && h->defer_rec && phase != 2) {
    if (defer_static) { const int fr = flush_pending(h, st, 1); if (fr) return fr; }
    else if (h->maybe_pending) { const int fr = flush_pending(h, st, 0); if (fr) return fr; }
  }
  h->ss.defer_now = defer ? 1 : 0;
  // (deferred image refresh: see api.hip.  Static per handle and entry point, like defer_static.)
  h->ss.img_defer_now = (!defer_static && h->defer_rec && rec && h->lp && phase == 0 && early_opt >= 0 && par && h->s3 &&
                      (h->persist_rec_bwd || h->persist_loc_bwd || h->persist_big_bwd || (h->persist_loc && h->lc_steps))) ? 1 : 0;
  if (defer) h->defer_flags = early_opt;       // (forked from hoist_side_work: behind the decoder prologue, like the hoisted work)
  if (phase != 2) {
    // Work that does not depend on the batch's forward pass (hoist_side_work below) goes to the side stream.  It is forked
    // from inside dec_fwd_chain, after the decoder's prologue has been enqueued: forked at the very start of the step it
    // ran before the prologue instead of beside it (80 us on the critical path in the kernel trace).
    const HoistWork hoist = {par ? 1 : 0, enc};
    r = dec_fwd_chain(h, enc, targets, T, 1, st, nullptr, &hoist); if (r) return r;
    const SideWork side = {targets, stepw, enc, T, phase};
    // global reconstructor: the side work is forked from inside fwd_rec_global, behind the batched input GEMM (so that
    // GEMM does not share the chip with the vocabulary projection; the persistent chain that follows leaves CUs free)
    const bool side_in_rec = par && h->kind == RECNET_REC_GLOBAL;
    if (!side_in_rec) { r = side_after_decoder_fwd(h, side, st, false); if (r) return r; }
    if (rec) {
      // bsum_r and the reconstructor's norm.  (Joining the hoisted branch through the pending-update branch instead — one
      // cross-stream edge in front of the reconstructor's chain instead of two, with the reconstructor's gate bias formed by
      // prologue_pack_kernel — was measured in round 4 and removed: the replayed graph then ran the pending update BEHIND the
      // decoder's chain instead of beside it at C3, 2.27 against 2.15 ms, and the prologue grew by 7 us.)
      if (par) hipStreamWaitEvent(st, h->ev[EV_HOIST_DONE], 0);
      if (defer && h->defer_rec != 2) hipStreamWaitEvent(st, h->ev[EV_PENDING_DONE], 0);          // ... and the updated parameters (deferred update)
      else if (defer) h->ss.rec_wait_pending = 1;                  // (mode 2: only the recurrent chain waits, see fwd_rec_global)
      if (h->ss.img_defer_now) h->ss.rec_wait_pending = 1;            // (deferred image refresh: the chains wait for the third stream's EV_PENDING_DONE)
      r = fwd_rec(h, enc, T, 1, st, /*norms_hoisted*/ true, /*loss_late*/ total_late, side_in_rec ? &side : nullptr); if (r) return r;      // (the loss scalars go where the total goes)
      // (measured and rejected in the fused step: the deferred gradients forked right behind the chain share the chip with the
      // d hiddens products the BPTT waits for, C2 2.06 -> 2.10 ms, C5 5.04 -> 5.44 ms)
      h->ss.deferred_done = 0;
      // phase 1 (data parallel, graph A): there is no decoder BPTT in this graph to hide the deferred products behind; forked
      // here they at least run beside the d hiddens products that follow the chain instead of after them
      r = bwd_rec_chain(h, h->c.lambda_recon, h->dHsrec, st, par && !defer && phase == 1, early_opt >= 0 ? early_opt : -1); if (r) return r;
      if (h->ss.join_pending) {                         // the decoder BPTT needs dHs_out; RN_SCAL_DEC_LOSS is final
        if (h->ss.join_recorded) hipStreamWaitEvent(st, h->ev[EV_SIDE_JOIN], 0); else join_from(h, EV_SIDE_JOIN, st, sd);
        h->ss.join_pending = 0; h->ss.join_recorded = 0;
      }
      if (!total_late) hipLaunchKernelGGL(axpb_kernel, dim3(1), dim3(1), 0, st, h->scal + RN_SCAL_DEC_LOSS, h->scal + RN_SCAL_REC_LOSS, h->c.lambda_recon, h->scal + RN_SCAL_TOTAL);
      if (phase == 1) {
        // (dp_overlap: the caller makes the stream of its early all-reduce wait for the side stream itself — recnet_join_side —
        // so that this stream can go on with the decoder's BPTT while the reconstructor's weight gradients are still being formed)
        if (h->ss.deferred_done && h->ss.dp_overlap) { h->ss.side_open = 1; h->ss.deferred_done = 0; }
        else if (h->ss.deferred_done) { join_from(h, EV_REC_DW_JOIN, st, sd); h->ss.deferred_done = 0; }      // forked behind the chain (above)
        else { r = bwd_rec_deferred(h, st, 0); if (r) return r; }
      }
    } else if (par) {
      if (h->ss.join_recorded) hipStreamWaitEvent(st, h->ev[EV_SIDE_JOIN], 0); else join_from(h, EV_SIDE_JOIN, st, sd);      // dHs_out of the vocabulary projection
      h->ss.join_pending = 0; h->ss.join_recorded = 0;
    }
    if (phase == 1) return RECNET_OK;
  }
  // (measured without effect: the BPTT chain enqueued in front of this fork, C2 1.906 / 1.906 ms, C3 2.32 / 2.32 ms)
  if (par) fork_to(h, EV_BPTT_FORK, st, sd);
  if (total_late) {      // (see above; sd is ordered behind the reconstructor's chains by the fork, and joined at the step's end)
    rec_loss_scalars(h, sd);
    hipLaunchKernelGGL(axpb_kernel, dim3(1), dim3(1), 0, sd, h->scal + RN_SCAL_DEC_LOSS, h->scal + RN_SCAL_REC_LOSS, h->c.lambda_recon, h->scal + RN_SCAL_TOTAL);
  }
  if (defer) {
    // this step's update stays pending: only what its deferred products could not read later is done now — the product
    // with the decoder's hidden states (local) and the zeroing of the gate gradients of the steps that did not run (global:
    // the deferred products always cover caption_max_len + 1 steps)
    if (h->defer_rec == 2) {
      // mode 2: everything but the recurrent weights is updated NOW, beside the decoder's BPTT chain (input-side and output-layer
      // products, bias sums, their Adam step); d W_hh = dG^T . h_{t-1} — 60 % of the reconstructor's weight-gradient work — and
      // its Adam step run under the NEXT step's decoder forward chain, whose 137 workgroups leave 119 CUs idle for 0.3 ms
      if (h->persist_dec_bwd) wait_chain(h, 1, sd);
      r = bwd_rec_deferred(h, sd, 0, 2);
      if (!r) r = optimizer_step(h, early_opt, sd, 1, 0, 0, 1u << RN_REC_T_WHH(h));      // (refreshes W_o^T / the W_ih rows of [W_ih | W_hh]^T; W_hh^T follows its own update in the next step)
    } else {
      r = bwd_rec_deferred(h, sd, 1);
    }
    if (r) { h->ss.defer_now = 0; return r; }
    if (h->kind == RECNET_REC_GLOBAL && T < h->Tm)
      hipMemsetAsync(at_off(h, h->dGr, (size_t)T * h->B * h->ld4R), 0, (size_t)(h->Tm - T) * h->B * h->ld4R * (h->lp ? 2 : 4), sd);
    hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, sd, h->ctrl + RN_CTRL_PENDING, 1u);
    h->maybe_pending = 1; h->ss.early_opt_done = 1; h->ss.deferred_done = 1;
  }
  if (phase == 0 && rec && !h->ss.deferred_done) {
    if (par && h->persist_dec_bwd) wait_chain(h, 1, sd);      // (the BPTT chain is launched on `st` below; this branch waits for its residency)
    r = bwd_rec_deferred(h, sd, 0); if (r) return r;
    if (early_opt >= 0 && par) {
      // The reconstructor's Adam step + re-transpose on a third stream behind its deferred products, so that the side stream is free for its half of the decoder's deferred gradients the moment the BPTT chain ends (the update
      // streams 0.5 GB and holds the side stream for ~130 us past the end of the chain).  Measured and rejected (round 3):
      // C2 1.993 against 1.931 ms, C3 2.322 against 2.295 ms — a third branch in the replayed graph costs more than it returns.
      // At R = 3584 (C5) the update streams 2 GB (367 us) and the decoder's second tail branch queues behind it on the side
      // stream: there the third stream wins (3.645 against 3.693 ms), so it is the default from R = 2560 up.
      const int f_s3 = h->R >= 2560 ? 1 : 0;
      hipStream_t so = (f_s3 && h->s3) ? h->s3 : sd;
      if (so != sd) fork_to(h, EV_OPT_FORK, sd, so);
      r = optimizer_step(h, early_opt, so, 1); if (r) return r;
      h->ss.early_opt_done = 1;
      s3_join = so != sd;
    }
  }
  h->ss.deferred_done = 0;
  // Issuing the decoder's deferred GEMMs for finished parts of the chain while it is still running was measured and
  // is a loss (+0.22 ms): the batched GEMMs occupy the CUs the latency-bound chain kernels need at every step.
  // (So is splitting the deferred gradients over two streams after the chain, +0.11 ms: in a replayed graph every extra
  // fork / join costs more than the concurrency returns.)
  r = dec_bwd_chain(h, dh, st); if (r) return r;
  // the decoder's deferred weight gradients: two independent halves on the two streams (the side stream's earlier
  // work — the reconstructor's deferred gradients and optimiser step — ends about when the chain does)
  if (par) fork_to(h, EV_DEC_DW_FORK, st, sd);
  r = dec_bwd_deferred(h, enc, targets, st, par ? sd : nullptr, (par && h->s3 && !s3_join) ? h->s3 : nullptr);
  h->ss.ctx_done = 0;
  if (r) return r;
  if (par) join_from(h, EV_TAIL_JOIN, st, sd);
  // (fused step: the decoder's optimiser step does not depend on the third stream's reconstructor update — the caller joins it behind
  // its own optimiser step: at 28 x 3584 the two overlap instead of 140 us of decoder update behind 600 us of reconstructor update)
  if (s3_join) { if (h->ss.in_fused) h->ss.s3_late = 1; else join_from(h, EV_S3_JOIN, st, h->s3); }
  h->fwd_dec_done = 0;
  h->ss.prezeroed = 0;
  return RECNET_OK;
}

static int fwd_bwd(recnet_handle* h, const float* enc, const int64_t* targets, int T, const float* stepw, hipStream_t st,
                   int phase = 0, int early_opt = -1) {
  const int r = fwd_bwd_impl(h, enc, targets, T, stepw, st, phase, early_opt);
  // the optimiser step is a separate call (a data-parallel caller all-reduces in between): carry the poison word across
  if (!r && phase != 1 && early_opt < 0 && h->og[0].bound && h->og[0].tab[0].g)
    hipLaunchKernelGGL(poison_mark_kernel, dim3(1), dim3(1), 0, st, h->og[0].tab[0].g, (const float*)(h->scal + RN_SCAL_POISON));
  h->ss.defer_now = 0;
  if (r) sched_reset(h);
  return r;
}

// the argument checks every step entry point makes, in this order
static int check_step_args(recnet_handle* h, const float* enc, const int64_t* targets, int T, const float* step_weight) {
  if (!h->dec_bound || (h->kind != RECNET_REC_NONE && !h->rec_bound)) return fail(RECNET_ESTATE, "models not bound");
  if (!h->dGd.out_weight || (h->kind != RECNET_REC_NONE && !h->rG.out_weight)) return fail(RECNET_ESTATE, "gradients not bound");
  if (!enc || !targets || !step_weight) return fail(RECNET_EINVAL, "null argument");
  if (check_T(h, T)) return fail(RECNET_EINVAL, "T out of range");
  return RECNET_OK;
}

int recnet_train_step_fwd_bwd(recnet_handle* h, const float* enc, const int64_t* targets, int32_t T,
                              const float* step_weight, uint32_t seed, recnet_scalars* scalars, void* stream) {
  REQUIRE_WS(h);
  FLUSH_PENDING(h, stream);
  { const int cr = check_step_args(h, enc, targets, T, step_weight); if (cr) return cr; }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, st, h->ctrl, seed);
  int r = fwd_bwd(h, enc, targets, T, step_weight, st); if (r) return r;
  if (scalars) hipLaunchKernelGGL(export_scalars_kernel, dim3(1), dim3(1), 0, st, h->scal, scalars);
  h->fwd_dec_done = 0;
  LAUNCH_OK();
  return RECNET_OK;
}

// A failing optimizer_step inside the fused step (ADVICE r5): the side streams the step opened are joined back into the caller's stream
// and the enqueue-time bookkeeping goes back to "between two steps" (recnet_abort_step's reset) — otherwise the third stream stayed
// unjoined and a later non-fused optimizer_step saw img_defer_now set and skipped the refresh of the derived weight images.
static void step_fail_cleanup(recnet_handle* h, hipStream_t st) {
  if (h->ss.s3_late && h->s3) join_from(h, EV_S3_JOIN, st, h->s3);
  recnet_abort_step(h);
  if (h->defer_rec) { h->maybe_pending = 1; h->images_maybe_stale = 1; }      // (what the step left pending is flushed / refreshed by the next call)
}

// The fused step behind its first kernel (which sets the seed and the step counter and writes the step-start stamp): forward + backward with
// the reconstructor's optimiser step issued inside, under the decoder BPTT, then the decoder's.
static int fused_step(recnet_handle* h, const float* enc, const int64_t* targets, int T, const float* step_weight, int flags,
                      recnet_scalars* scalars, hipStream_t st) {
  h->ss.in_fused = 1;
  int r = fwd_bwd(h, enc, targets, T, step_weight, st, 0, flags); if (r) { h->ss.in_fused = 0; return r; }
  r = optimizer_step(h, flags, st, h->ss.early_opt_done ? 0 : -1); h->ss.in_fused = 0;
  if (r) { step_fail_cleanup(h, st); return r; }
  if (h->ss.s3_late) { join_from(h, EV_S3_JOIN, st, h->s3); h->ss.s3_late = 0; }
  h->ss.img_defer_now = 0;
  if (scalars) hipLaunchKernelGGL(export_scalars_kernel, dim3(1), dim3(1), 0, st, h->scal, scalars);
  h->fwd_dec_done = 0;
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_train_step(recnet_handle* h, const float* enc, const int64_t* targets, int32_t T,
                      const float* step_weight, uint32_t seed, int32_t step, recnet_scalars* scalars, void* stream) {
  REQUIRE_WS(h);
  if (!h->defer_rec) { const int fr_ = flush_pending(h, (hipStream_t)stream); if (fr_) return fr_; }
  int r = check_step_args(h, enc, targets, T, step_weight); if (r) return r;
  if (step < 1) return fail(RECNET_EINVAL, "step must be >= 1");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, st, h->ctrl, seed);
  hipLaunchKernelGGL(set_step_kernel, dim3(1), dim3(1), 0, st, (int32_t*)(h->ctrl + RN_CTRL_STEP), step);      // (+ the step-start stamp)
  return fused_step(h, enc, targets, T, step_weight, RECNET_OPT_REG | RECNET_OPT_CLIP, scalars, st);
}

int recnet_train_step_dev(recnet_handle* h, const float* enc, const int64_t* targets, int32_t T, const float* step_weight,
                          uint32_t seed_base, int32_t flags, recnet_scalars* scalars, void* stream) {
  REQUIRE_WS(h);
  if (!h->defer_rec) { const int fr_ = flush_pending(h, (hipStream_t)stream); if (fr_) return fr_; }
  int r = check_step_args(h, enc, targets, T, step_weight); if (r) return r;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(advance_step_kernel, dim3(1), dim3(1), 0, st, (int32_t*)(h->ctrl + RN_CTRL_STEP), h->ctrl, seed_base);
  return fused_step(h, enc, targets, T, step_weight, flags, scalars, st);
}

int recnet_set_step(recnet_handle* h, int32_t step, void* stream) {
  REQUIRE_WS(h);
  hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, h->ctrl + RN_CTRL_STEP, (uint32_t)step);
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_train_step_fwd_bwd_dev(recnet_handle* h, const float* enc, const int64_t* targets, int32_t T,
                                  const float* step_weight, uint32_t seed_base, recnet_scalars* scalars, void* stream) {
  REQUIRE_WS(h);
  FLUSH_PENDING(h, stream);
  { const int cr = check_step_args(h, enc, targets, T, step_weight); if (cr) return cr; }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(advance_step_kernel, dim3(1), dim3(1), 0, st, (int32_t*)(h->ctrl + RN_CTRL_STEP), h->ctrl, seed_base);
  int r = fwd_bwd(h, enc, targets, T, step_weight, st); if (r) return r;
  if (scalars) hipLaunchKernelGGL(export_scalars_kernel, dim3(1), dim3(1), 0, st, h->scal, scalars);
  h->fwd_dec_done = 0;
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_train_step_part_dev(recnet_handle* h, int32_t part, const float* enc, const int64_t* targets, int32_t T,
                               const float* step_weight, uint32_t seed_base, recnet_scalars* scalars, void* stream) {
  REQUIRE_WS(h);
  FLUSH_PENDING(h, stream);
  if (part != 1 && part != 2) return fail(RECNET_EINVAL, "part must be 1 or 2");
  { const int cr = check_step_args(h, enc, targets, T, step_weight); if (cr) return cr; }
  hipStream_t st = (hipStream_t)stream;
  if (part == 1) hipLaunchKernelGGL(advance_step_kernel, dim3(1), dim3(1), 0, st, (int32_t*)(h->ctrl + RN_CTRL_STEP), h->ctrl, seed_base);
  else if (h->T_last != T) return fail(RECNET_ESTATE, "part 2 without a matching part 1");
  int r = fwd_bwd(h, enc, targets, T, step_weight, st, part); if (r) return r;
  if (scalars) hipLaunchKernelGGL(export_scalars_kernel, dim3(1), dim3(1), 0, st, h->scal, scalars);
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_optimizer_step_dev(recnet_handle* h, int32_t flags, recnet_scalars* scalars, void* stream) {
  REQUIRE_WS(h);
  FLUSH_PENDING(h, stream);
  hipStream_t st = (hipStream_t)stream;
  // (the poison marker travels with the decoder's LAST bucket: a call that steps the reconstructor only — early, beside the BPTT —
  // must not read the decoder's gradients, which are still being formed)
  if (!(flags & RECNET_OPT_SKIP_DECODER) && h->og[0].bound && h->og[0].tab[0].g)
    hipLaunchKernelGGL(poison_collect_kernel, dim3(1), dim3(1), 0, st, (const float*)h->og[0].tab[0].g, h->scal + RN_SCAL_POISON);
  int r = optimizer_step(h, flags, st); if (r) return r;
  if (scalars && !(flags & RECNET_OPT_SKIP_DECODER)) hipLaunchKernelGGL(export_scalars_kernel, dim3(1), dim3(1), 0, st, h->scal, scalars);
  LAUNCH_OK();
  return RECNET_OK;
}

