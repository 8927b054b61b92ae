// Decoder sequences (train.py:17-75): forward chain + loss, backward chain + deferred weight gradients.
// Part of api.hip (one translation unit; see the include list there).
// ---------------------------------------------------------------------------------------------- decoder forward
// the dependent chain: invariants, embeddings, T x (GEMM + cell kernel)
// free_tokens != nullptr: free-running decoding (train.py:46-51) — the input of step t+1 is the argmax of step t's
// (dropped-out) logits, written to free_tokens [T][B]; the per-step embedding / input projection / vocabulary projection
// then sit inside the chain.  Forward only.
// hoist != nullptr (fused step): the step's hoisted work is forked from here and forms the parameter norms (hoist_side_work).
// flags (recnet_score_captions): DFC_REUSE_INVARIANTS — Uv / P / the gate bias are what the previous call left (enc is not read);
// DFC_NO_REG_NORM — the regulariser's parameter norms are not formed (a pass that has no loss).
enum { DFC_REUSE_INVARIANTS = 1, DFC_NO_REG_NORM = 2 };
static int dec_fwd_chain(recnet_handle* h, const float* enc, const int64_t* targets, int T, int train, hipStream_t st,
                         int64_t* free_tokens = nullptr, const HoistWork* hoist = nullptr, unsigned flags = 0) {
  RN_RANGE("recnet: decoder forward chain (decoder.py:45-70 x T)");
  const int B = h->B, F = h->F, E = h->E, H = h->H, A = h->A, V = h->V;
  h->ss.mp_done = 0;
  if (!hoist && !(flags & DFC_NO_REG_NORM)) param_norms(h, 0, h->scal + RN_SCAL_DEC_REG, st);
  // The input part of the gates (embeddings -> Xe) does not depend on the features: in the fused step it runs on the side
  // stream beside the feature products Uv / P (EV_XE_FORK joins it in front of the chain)
  const bool fork_xe = !free_tokens && h->overlap && h->s2 && hoist && hoist->par;
  // bf16 path, round 4: the three products of the prologue — Xe, Uv, P — are ONE grouped launch (774 tiles in one hardware
  // queue instead of launches of 400, 22 and 352 workgroups): only the embedding gather runs beside the feature cast
  const bool pro_group = fork_xe && h->lp;
  if (pro_group) {
    // gate bias, embedding gather and feature cast in one launch (kernels_util.hpp: prologue_pack_kernel)
    // (measured and rejected: the three as separate kernels on the step's own stream, 1.748 against 1.720 ms at C2)
    ProPackArgs a;
    a.enc_lp = (bf16_t*)h->enc_lp; a.ld_enc = h->ldD; a.enc = enc; a.rowsE = B * F; a.D = h->D;
    a.Emb = h->dP.embedding_weight; a.targets = targets; a.emb = (bf16_t*)h->emb_lp; a.ld_emb = h->ldE; a.B = B; a.E = E; a.V = V;
    a.scale = h->c.embedding_scale; a.dd = mkdrop(h, RN_SITE_DEC_EMBED, h->c.embedding_dropout, train); a.rowsT = T * B;
    a.bih = h->dP.rnn_bias_ih_l0; a.bhh = h->dP.rnn_bias_hh_l0; a.bsum = h->bsum_d; a.Hd = H; a.gru = h->dgru;
    a.nb_pack = 2 * (h->ncu > 0 ? h->ncu : 256);
    hipLaunchKernelGGL(prologue_pack_kernel, dim3(a.nb_pack + (T * B + 1) / 2 + 1), dim3(256), 0, st, a);
  }
  if (pro_group) {
    GemmGroup g = gg_begin(0, 0);
    gg_add(h, g, h->emb_lp, h->ldE, h->We_w, h->ldE, h->Xe, 4 * H, h->bsum_d, T * B, 4 * H, E, 1.f, 0, st);
    gg_add(h, g, h->enc_lp, h->ldD, h->U_w, h->ldD, h->Uv, A, nullptr, B * F, A, h->D, 1.f, 0, st);
    gg_add(h, g, h->enc_lp, h->ldD, h->Wc_w, h->ldD, (float*)h->P, h->ld4H, nullptr, B * F, 4 * H, h->D, 1.f, 0, st, 1);
    gg_run(h, g, st, stamp_site(1));
  } else if (fork_xe) {
    fork_to(h, EV_XE_FORK, st, h->s2);
    gate_bias(h->dP.rnn_bias_ih_l0, h->dP.rnn_bias_hh_l0, h->bsum_d, H, h->dgru, h->s2);   // Xe's bias
    embed_fwd(h, targets, nullptr, h->emb_lp, T * B, B, train, 0, h->s2);
    gemm(h, h->emb_lp, 0, h->ldE, h->We_w, 0, h->ldE, h->Xe, 4 * H, h->bsum_d, T * B, 4 * H, E, 1.f, 0, h->s2);
    hipEventRecord(h->ev[EV_XE_JOIN], h->s2);
  }
  if (!pro_group && !(flags & DFC_REUSE_INVARIANTS)) dec_invariants(h, enc, st, !fork_xe);   // (Uv on the side stream as well: measured +10 us, the two products share the chip anyway)
  if (pro_group) {
  } else if (fork_xe) {
    hipStreamWaitEvent(st, h->ev[EV_XE_JOIN], 0);
  } else if (!free_tokens) {
    // all T teacher-forced input embeddings at once    (decoder.py:46-48, train.py:25,45)
    embed_fwd(h, targets, nullptr, h->emb_lp, T * B, B, train, 0, st);
    // Xe = emb . W_ih[:, :E]^T + b_ih + b_hh
    gemm(h, h->emb_lp, 0, h->ldE, h->We_w, 0, h->ldE, h->Xe, 4 * H, h->bsum_d, T * B, 4 * H, E, 1.f, 0, st);
  } else {
    hipLaunchKernelGGL(fill_i64_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, h->sr_tok[0], (int64_t)1, B);   // <SOS>, train.py:25
  }
  // The side branches of the step's start (hoisted work, a pending reconstructor update) fork from HERE — behind the prologue — but,
  // when the chain is one persistent launch, they are enqueued BEHIND that launch with their fork events recorded in front of it:
  // captured in this order the chain stays on the prologue's hardware queue (the first-captured successor of a graph node does)
  // instead of paying a cross-queue hand-over of ~20 us on the critical path; the branches wait for the chain's residency anyway
  // (wait_chain_kernel)
  const bool hoist_late = hoist && h->persist_dec && !free_tokens && (h->ld4H & 7) == 0 && h->overlap && h->s2;
  int hoist_r = RECNET_OK;
  if (hoist_late) { hipEventRecord(h->ev[EV_HOIST_FORK], st); hipEventRecord(h->ev[EV_S3_FORK], st); }
  else if (hoist) hoist_r = hoist_side_work(h, *hoist, st, false);     // forked here: beside the chain, behind the prologue (fwd_bwd_impl)
  if (h->persist_dec && !free_tokens && (h->ld4H & 7) == 0) {
   hipEvent_t pe = prof_bracket_begin(h, RN_SITE_DEC_CHAIN_FWD, st);
   // batches above RC_PAN_ROWS captions: one launch per row group of h->bgrp captions (csrc/api.hip) — a group is an
   // independent batch for the chain: its own rows of every [T][B][.] tensor (row stride Bs = B), the same weights
   for (int b0 = 0; b0 < B; b0 += h->bgrp) {
    const int nb = B - b0 < h->bgrp ? B - b0 : h->bgrp;
    DecChainArgs c;
    c.T = T; c.B = nb; c.Bs = B; c.F = F; c.H = H; c.A = A; c.gru = h->dgru;
    c.W = (const bf16_t*)h->Wcomb; c.ldw = h->ldH;
    c.P = (const bf16_t*)h->P + (size_t)b0 * F * h->ld4H; c.ldp = h->ld4H; c.Uv = h->Uv + (size_t)b0 * F * A; c.ab = h->dP.attn_b; c.w = h->dP.attn_w_weight;
    c.Xe = h->Xe + (size_t)b0 * 4 * H; c.G1 = h->dc_G1; c.Pan = (bf16_t*)h->dc_pan;
    c.Hs = h->Hs + (size_t)b0 * H; c.Cs = h->Cs + (size_t)b0 * H; c.acts = h->acts + (size_t)b0 * 4 * H; c.Hlp = (bf16_t*)h->Hs_lp + (size_t)b0 * h->ldH; c.ld_hlp = h->ldH;
    c.Wh = h->Wh + (size_t)b0 * A; c.att = h->att + (size_t)b0 * F; c.bar = cs_ws_bar(h->gbar, CS_DEC_FWD); c.ts = h->lc_ts + 4096; c.softmax = h->c.decoder_attn_normalize == RECNET_ATTN_SOFTMAX;
    c.epoch = cs_ws_epoch(h->gbar, CS_DEC_FWD); c.rep = h->gbar + CS_WS_REP_DEC_FWD; c.poison = h->scal + RN_SCAL_POISON;
    c.mp = h->kind == RECNET_REC_GLOBAL ? h->mp + (size_t)b0 * H : nullptr; c.mp_scale = (float)h->cml / ((float)T * (float)T);   // global_reconstructor.py:33-37
    h->ss.mp_done = c.mp ? 1 : 0;
    // dec_xcat: the chain also writes the global reconstructor's input operand [h_t ; drop_t(mp)] (no xcat_global_kernel behind it)
    const int f_xcat = h->sw.dec_xcat;
    c.Xcat = nullptr; c.ld_xcat = 0; c.xdd = mkdrop(h, RN_SITE_REC_INPUT, h->c.reconstructor_decoder_dropout, train);
    // (not with the deferred reconstructor update: its pending weight-gradient products read the PREVIOUS step's operand while this chain runs)
    if (f_xcat && c.mp && h->lp && h->ld2H == 2 * H && h->Xcat_g && h->defer_rec != 1) {
      c.Xcat = (bf16_t*)h->Xcat_g + (size_t)b0 * h->ld2H; c.ld_xcat = h->ld2H; c.xdd.boff += b0;
      h->ss.xcat_done = 1;
    }
    // LW (F <= 32): the attention projection is formed by the caption's own workgroup from an LDS-resident attn_W (dec_chain.hpp)
    const bool lw = h->sw.dec_lw && A <= 128 && H <= 512 && (H & 31) == 0 && F <= 32;
    const int NAx = DCF_NA(lw ? 4 * H : 4 * H + A);
    const dim3 grid(NAx > nb ? NAx : nb);
    if (F > 32) {      // frames 32 .. 47 from LDS
      const size_t dyn = (size_t)DC_XF * 2048 * 2 + (size_t)DC_XF * 128 * 4;
      hipFuncSetAttribute(reinterpret_cast<const void*>(dec_chain_kernel<true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
      hipLaunchKernelGGL((dec_chain_kernel<true, false>), grid, dim3(256), dyn, st, c);
    } else if (lw) {
      const size_t dyn = (size_t)128 * 512 * 2;
      hipFuncSetAttribute(reinterpret_cast<const void*>(dec_chain_kernel<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
      hipLaunchKernelGGL((dec_chain_kernel<false, true>), grid, dim3(256), dyn, st, c);
    } else {
      hipLaunchKernelGGL((dec_chain_kernel<false, false>), grid, dim3(256), 0, st, c);
    }
   }
    if (pe) hipEventRecord(pe, st);
    if (hoist_late) hoist_r = hoist_side_work(h, *hoist, st, true);
    h->T_last = T; h->train_last = train;
    return hoist_r;
  }
  DecCellArgs a;
  a.B = B; a.F = F; a.H = H; a.A = A;
  a.P = h->P; a.ldp = h->ld4H; a.Uv = h->Uv; a.ab = h->dP.attn_b; a.w = h->dP.attn_w_weight;
  a.ld_hlp = h->ldH; a.gru = h->dgru; a.nc = 0;
  const float* prev_state = h->dgru ? h->Hs : h->Cs;   // what the pointwise part carries: h_{t-1} (GRU) / c_{t-1}
  for (int t = 0; t < T; ++t) {
    if (free_tokens) {
      const int64_t* fed = t == 0 ? h->sr_tok[0] : free_tokens + (size_t)(t - 1) * B;
      hipMemcpyAsync(h->in_tok + (size_t)t * B, fed, (size_t)B * 8, hipMemcpyDeviceToDevice, st);
      embed_fwd(h, nullptr, fed, at_off(h, h->emb_lp, (size_t)t * B * h->ldE), B, B, train, t, st);
      gemm(h, at_off(h, h->emb_lp, (size_t)t * B * h->ldE), 0, h->ldE, h->We_w, 0, h->ldE, h->Xe + (size_t)t * B * 4 * H, 4 * H,
           h->bsum_d, B, 4 * H, E, 1.f, 0, st);
    }
    int S = 0;
    if (t > 0)   // h_{t-1} . [W_hh ; attn_W]^T  -> recurrent gate part + Wh of the attention
      S = gemm_slabs(h, RN_TAG_DEC_FWD, at_off(h, h->Hs_lp, (size_t)(t - 1) * B * h->ldH), h->ldH, h->Wcomb, 0, h->ldH, B, 4 * H + A, H, st);
    a.t = t; a.S = S; a.slab = t > 0 ? h->slab : nullptr;
    a.Xe = h->Xe + (size_t)t * B * 4 * H;
    a.c_prev = t > 0 ? prev_state + (size_t)(t - 1) * B * H : nullptr;
    a.h_out = h->Hs + (size_t)t * B * H; a.c_out = h->Cs + (size_t)t * B * H;
    a.h_lp = at_off(h, h->Hs_lp, (size_t)t * B * h->ldH);
    a.acts = h->acts + (size_t)t * B * 4 * H;
    a.Wh_out = h->Wh + (size_t)t * B * A; a.att_out = h->att + (size_t)t * B * F; a.softmax = h->c.decoder_attn_normalize == RECNET_ATTN_SOFTMAX;
    launch_dec_cell(h, a, B, st);
    if (free_tokens) {   // logits_t, then argmax of what Decoder.forward returns (the dropped-out logits, decoder.py:68-69)
      float* lg = h->logits + (size_t)t * B * V;
      gemm(h, at_off(h, h->Hs_lp, (size_t)t * B * h->ldH), 0, h->ldH, h->Wo_w, 0, h->ldH, lg, V, h->dP.out_bias, B, V, H, 1.f, 0, st);
      const float* pick = lg;
      if (train && h->c.decoder_out_dropout > 0.f) {
        copyf(lg, h->sr_logits, (size_t)B * V, st);
        hipLaunchKernelGGL(logits_drop_kernel, dim3(ew_blocks((size_t)B * V)), dim3(256), 0, st, h->sr_logits, B, V,
                           mkdrop(h, RN_SITE_DEC_LOGIT, h->c.decoder_out_dropout, train), t);
        pick = h->sr_logits;
      }
      hipLaunchKernelGGL(argmax_rows_kernel, dim3(B), dim3(256), 0, st, pick, V, V, free_tokens + (size_t)t * B);
    }
  }
  h->T_last = T; h->train_last = train;
  return hoist_r;
}
// vocabulary projection + loss for all steps (decoder.py:68-69, train.py:54-68); independent of the reconstructor
static int dec_fwd_loss(recnet_handle* h, const int64_t* targets, int T, const float* stepw, int train, hipStream_t st,
                        int have_logits = 0) {
  RN_RANGE("recnet: vocabulary projection + masked CE (train.py:56-68)");
  const int B = h->B, H = h->H, V = h->V;
  if (!have_logits) gemm(h, h->Hs_lp, 0, h->ldH, h->Wo_w, 0, h->ldH, h->logits, V, h->dP.out_bias, T * B, V, H, 1.f, 0, st);
  {
    // (the step weights are read where the caller keeps them: a copy into the workspace first was one more launch on this branch)
    const DropDesc dd = mkdrop(h, RN_SITE_DEC_LOGIT, h->c.decoder_out_dropout, train);
    if (h->lp) hipLaunchKernelGGL(ce_kernel<bf16_t>, dim3(T * B), dim3(256), 0, st, h->logits, targets, stepw, h->rowloss, (bf16_t*)h->dlog_lp, h->ldV, B, V, dd);
    else hipLaunchKernelGGL(ce_kernel<float>, dim3(T * B), dim3(256), 0, st, h->logits, targets, stepw, h->rowloss, (float*)h->dlog_lp, h->ldV, B, V, dd);
  }
  hipLaunchKernelGGL(dec_loss_finalize_kernel, dim3(1), dim3(256), 0, st, h->rowloss, T * B, h->scal, h->c.decoder_lambda_reg);
  return RECNET_OK;
}
static int fwd_decoder(recnet_handle* h, const float* enc, const int64_t* targets, int T, const float* stepw,
                       int train, float* hiddens_out, hipStream_t st, int64_t* free_tokens = nullptr) {
  int r = dec_fwd_chain(h, enc, targets, T, train, st, free_tokens); if (r) return r;
  r = dec_fwd_loss(h, targets, T, stepw, train, st, free_tokens != nullptr); if (r) return r;
  if (hiddens_out) copyf(h->Hs, hiddens_out, (size_t)T * h->B * h->H, st);
  // free_fwd: the backward scatters the embedding gradient by the tokens that were fed (in_tok), not by the targets
  h->fwd_dec_done = 1; h->free_fwd = free_tokens ? 1 : 0; h->fwd_rec_done = 0; h->rec_bwd_done = 0;
  return RECNET_OK;
}

// ---------------------------------------------------------------------------------------------- decoder backward
// output layer: dHs_out = dlogits . W_o, dW_o, db_o — needs only the decoder forward
// part: bit 0 = d hiddens (what the BPTT chain needs), bit 1 = the layer's own gradients dW_o, db_o (needed by the optimiser only)
// early_join: the caller is the whole fused step's side branch (side_after_decoder_fwd, phase 0), whose join the BPTT waits for
static int dec_bwd_out(recnet_handle* h, float gscale, hipStream_t st, int part = 3, bool early_join = false) {
  RN_RANGE("recnet: output layer backward");
  const int B = h->B, H = h->H, V = h->V, T = h->T_last, TB = T * B;
  if (gscale != 1.0f && (part & 1)) {
    const size_t n = (size_t)TB * h->ldV;
    if (h->lp) hipLaunchKernelGGL(scale_kernel<bf16_t>, dim3(ew_blocks(n)), dim3(256), 0, st, (bf16_t*)h->dlog_lp, n, gscale);
    else hipLaunchKernelGGL(scale_kernel<float>, dim3(ew_blocks(n)), dim3(256), 0, st, (float*)h->dlog_lp, n, gscale);
  }
  if (part & 1) gemm(h, h->dlog_lp, 0, h->ldV, h->Wo_w, 1, h->ldH, h->dHs, H, nullptr, TB, H, V, 1.f, 0, st);
  // Decoder-only step: the BPTT waits for this branch only up to here (d hiddens of the output layer, and the CE loss in front of
  // it) — the output layer's own gradients and the attended features that follow run beside the BPTT chain, whose 129 workgroups
  // leave half the chip idle and which nothing else shares in this configuration (EV_SIDE_TAIL covers them for the step's tail).  With a
  // reconstructor the same was measured in round 4 and is off: there the BPTT waits for the reconstructor's d-hiddens product.
  if ((part & 1) && h->kind == RECNET_REC_NONE && h->ss.join_pending && !h->ss.join_recorded && st == h->s2 && early_join) {
    hipEventRecord(h->ev[EV_SIDE_JOIN], st); h->ss.join_recorded = 1; h->ss.side_tail_open = 1;
  }
  if (!(part & 2)) return RECNET_OK;
  // dW_o = dlogits^T . Hs ; db_o = colsum(dlogits)
  gemm(h, h->dlog_lp, 1, h->ldV, h->Hs_lp, 1, h->ldH, h->dGd.out_weight, H, nullptr, V, H, TB, 1.f, 0, st);
  colsum_at(h, h->dlog_lp, TB, V, h->ldV, h->dGd.out_bias, st, h->ss.prezeroed);
  return RECNET_OK;
}
// BPTT chain; dh_t (direct) = dHs_out[t] + dhid[t] (the reconstructor's gradient w.r.t. the hidden states)
static int dec_bwd_chain(recnet_handle* h, const float* dhid, hipStream_t st) {
  RN_RANGE("recnet: decoder BPTT chain");
  const int B = h->B, F = h->F, H = h->H, A = h->A, T = h->T_last;
  const int ldWS = h->ldWS, KW = 4 * H + RN_FCH * A;
  if (h->persist_dec_bwd) {
   hipEvent_t pe = prof_bracket_begin(h, RN_SITE_DEC_CHAIN_BWD, st);
   for (int b0 = 0; b0 < B; b0 += h->bgrp) {      // one launch per row group (see dec_fwd_chain)
    const int nb = B - b0 < h->bgrp ? B - b0 : h->bgrp;
    DecChainBwdArgs c;
    c.T = T; c.B = nb; c.Bs = B; c.F = F; c.H = H; c.A = A; c.gru = h->dgru;
    c.Wt = (const bf16_t*)h->WcombT; c.ldwt = h->ldKW;
    c.P = (const bf16_t*)h->P + (size_t)b0 * F * h->ld4H; c.ldp = h->ld4H; c.Uv = h->Uv + (size_t)b0 * F * A; c.ab = h->dP.attn_b; c.w = h->dP.attn_w_weight;
    c.dHs = h->dHs + (size_t)b0 * H; c.dHs2 = dhid ? dhid + (size_t)b0 * H : nullptr; c.acts = h->acts + (size_t)b0 * 4 * H; c.Cs = h->Cs + (size_t)b0 * H; c.Hs = h->Hs + (size_t)b0 * H;
    c.Wh = h->Wh + (size_t)b0 * A; c.att = h->att + (size_t)b0 * F; c.softmax = h->c.decoder_attn_normalize == RECNET_ATTN_SOFTMAX;
    c.G2 = h->dc_G2; c.Pan = (bf16_t*)h->dc_pan2; c.dGx = (bf16_t*)h->dGx + (size_t)b0 * ldWS; c.ld_dgx = ldWS;
    c.dUv = h->dUv + (size_t)b0 * F * A; c.dUv_lp = (bf16_t*)h->dUv_lp + (size_t)b0 * F * h->ldA; c.ld_dUv = h->ldA; c.dwacc = h->dwacc + (size_t)b0 * A;
    c.bar = cs_ws_bar(h->gbar, CS_DEC_BWD); c.ts = h->lc_ts + 4096 + 512;
    // the B' -> A' hand-over (dec_chain.hpp): the arrival flags of a row part polled by the part's own unit owners
    c.epoch = cs_ws_epoch(h->gbar, CS_DEC_BWD); c.rep = h->gbar + CS_WS_REP_DEC_BWD; c.poison = h->scal + RN_SCAL_POISON;
    const int NAb = DCB_NA(H);
    const dim3 grid(NAb > nb ? NAb : nb);
    if (F > 32) {
      const size_t dyn = (size_t)DC_XF * DCB_PLD * 2 + (size_t)2 * DC_XF * 128 * 4;
      hipFuncSetAttribute(reinterpret_cast<const void*>(dec_chain_bwd_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
      hipLaunchKernelGGL(dec_chain_bwd_kernel<true>, grid, dim3(256), dyn, st, c);
    } else {
      hipLaunchKernelGGL(dec_chain_bwd_kernel<false>, grid, dim3(256), 0, st, c);
    }
   }
    if (pe) hipEventRecord(pe, st);
    return RECNET_OK;
  }
  // per step one fused kernel over (caption, frame chunk) + one split-K GEMM (dgates_t | dWh_t chunks) . [W_hh ; W x4]
  DecCellBwdArgs a;
  a.B = B; a.F = F; a.H = H; a.A = A;
  a.P = h->P; a.ldp = h->ld4H; a.Uv = h->Uv; a.ab = h->dP.attn_b; a.w = h->dP.attn_w_weight;
  a.dUv = h->dUv; a.dwacc = h->dwacc; a.ld_dgx = ldWS; a.dUv_lp = h->dUv_lp; a.ld_dUv = h->ldA; a.gru = h->dgru;
  const float* prev_state = h->dgru ? h->Hs : h->Cs;
  const int Asz = A <= 256 ? 256 : A;
  const size_t sm = (size_t)(4 * H + F + 2 * Asz + 16) * 4;
  int S = 0;
  for (int t = T - 1; t >= 0; --t) {
    a.t = t; a.S = S; a.slab = (t < T - 1) ? h->slab : nullptr; a.first = (t == T - 1); a.last = (t == 0);
    a.dHs = h->dHs + (size_t)t * B * H; a.dHs2 = dhid ? dhid + (size_t)t * B * H : nullptr;
    a.acts = h->acts + (size_t)t * B * 4 * H;
    a.c = h->Cs + (size_t)t * B * H;
    a.c_prev = t > 0 ? prev_state + (size_t)(t - 1) * B * H : nullptr;
    a.dc_in = h->dc_carry + (size_t)((t + 1) & 1) * B * H; a.dc_out = h->dc_carry + (size_t)(t & 1) * B * H;
    a.dGx = at_off(h, h->dGx, (size_t)t * B * ldWS);
    a.Wh = h->Wh + (size_t)t * B * A; a.att = h->att + (size_t)t * B * F; a.softmax = h->c.decoder_attn_normalize == RECNET_ATTN_SOFTMAX;
    LAUNCH_AT(h, dec_cell_bwd_kernel, dim3(B, RN_FCH), dim3(256), sm, st, a);
    if (t > 0)
      S = h->use_wcomb_t ? gemm_slabs(h, RN_TAG_DEC_BWD, at_off(h, h->dGx, (size_t)t * B * ldWS), ldWS, h->WcombT, 0, h->ldKW, B, H, KW, st)
                         : gemm_slabs(h, RN_TAG_DEC_BWD, at_off(h, h->dGx, (size_t)t * B * ldWS), ldWS, h->Wcomb, 1, h->ldH, B, H, KW, st);
  }
  return RECNET_OK;
}
// the attended features of the steps [t0, t1): needs only the forward pass (att), so a caller may run it early
static void dec_ctx_rows(recnet_handle* h, const float* enc, int t0, int t1, hipStream_t st) {
  const int B = h->B, F = h->F, D = h->D;
  const size_t r0 = (size_t)t0 * B;
  dim3 grid(B, cdiv(h->ldD, h->Tm <= 32 ? 512 : 256));      // (ctx_all_kernel: two columns per thread)
  const float* att = h->att + r0 * F;
  void* ctx = at_off(h, h->ctx_lp, r0 * h->ldD);
  const int Tn = t1 - t0;
  if (h->Tm <= 32) {
    if (h->lp) hipLaunchKernelGGL(ctx_all_kernel<bf16_t>, grid, dim3(256), (size_t)32 * F * 4, st, att, enc, (bf16_t*)ctx, h->ldD, Tn, B, F, D);
    else hipLaunchKernelGGL(ctx_all_kernel<float>, grid, dim3(256), (size_t)32 * F * 4, st, att, enc, (float*)ctx, h->ldD, Tn, B, F, D);
  } else {
    if (h->lp) hipLaunchKernelGGL(ctx_all_slow_kernel<bf16_t>, grid, dim3(256), 0, st, att, enc, (bf16_t*)ctx, h->ldD, Tn, B, F, D);
    else hipLaunchKernelGGL(ctx_all_slow_kernel<float>, grid, dim3(256), 0, st, att, enc, (float*)ctx, h->ldD, Tn, B, F, D);
  }
}
// Deferred weight gradients of the decoder for the time steps [t0, t1) (rows [t0 B, t1 B) of dGx): every product whose
// contraction runs over (t, b).  acc = 0 for the first range processed (it also zeroes dEmb), 1 afterwards.  Ranges can be
// issued as soon as the BPTT chain has produced their rows, on another stream, while the chain goes on.
static int dec_bwd_deferred_rows(recnet_handle* h, const float* enc, const int64_t* targets, int t0, int t1, int acc, hipStream_t st,
                                 hipStream_t st2 = nullptr) {
  const int B = h->B, D = h->D, E = h->E, H = h->H, A = h->A, V = h->V;
  const int train = h->train_last, ldWS = h->ldWS, nrow = (t1 - t0) * B;
  const size_t r0 = (size_t)t0 * B;
  const int GH = (h->dgru ? 3 : 4) * H;   // rows of the master W_ih / W_hh: gate blocks (r, z, n) or (i, f, g, o)
  void* dG = at_off(h, h->dGx, r0 * ldWS);
  // dgates live in columns [0,4H) of dGx, dWh chunks behind them
  // the embedding branch: d emb product + the two scatter kernels (measured and rejected, round 3: on the second stream's half,
  // C2 1.979 against 1.931 ms — the side stream is still busy with the reconstructor's Adam step when the chain ends)
  gemm(h, dG, 0, ldWS, h->We_w, 1, h->ldE, h->demb + r0 * E, E, nullptr, nrow, E, 4 * H, 1.f, 0, st);
  if (!acc && !h->ss.prezeroed) hipMemsetAsync(h->dGd.embedding_weight, 0, (size_t)V * E * 4, st);
  hipLaunchKernelGGL(embed_bwd_kernel, dim3(nrow), dim3(128), 0, st, h->dGd.embedding_weight, targets, h->demb, B, E, V,
                     h->c.embedding_scale, mkdrop(h, RN_SITE_DEC_EMBED, h->c.embedding_dropout, train), (int)r0,
                     (const int64_t*)(h->free_fwd ? h->in_tok : nullptr));
  hipLaunchKernelGGL(embed_bwd_hot_kernel, dim3(cdiv(E, 128), cdiv(nrow, RN_HOT_ROWS)), dim3(128), 0, st, h->dGd.embedding_weight, targets, h->demb, B, E, V,
                     h->c.embedding_scale, mkdrop(h, RN_SITE_DEC_EMBED, h->c.embedding_dropout, train), (int)r0, nrow,
                     (const int64_t*)(h->free_fwd ? h->in_tok : nullptr));
  gemm(h, dG, 1, ldWS, at_off(h, h->emb_lp, r0 * h->ldE), 1, h->ldE, h->dGd.rnn_weight_ih_l0, E + D, nullptr, GH, E, nrow, 1.f, acc, st);
  // ctx_t = (1/F) sum_f a_t[f] enc[b,f] for these steps (only needed here), then dW_ih[:, E:] (+)= dgates^T . ctx
  {
    if (!h->ss.ctx_done) dec_ctx_rows(h, enc, t0, t1, st);
    void* ctx = at_off(h, h->ctx_lp, r0 * h->ldD);
    gemm(h, dG, 1, ldWS, ctx, 1, h->ldD, h->dGd.rnn_weight_ih_l0 + E, E + D, nullptr, GH, D, nrow, 1.f, acc, st);
  }
  // the rest touches other gradient tensors: on a second stream when the caller has one
  if (st2 && st2 != st) st = st2;
  // dWh_t = sum of its RN_FCH frame-chunk partials (operand of dW_attn and source of d attn_b)
  {
    const size_t n = (size_t)nrow * h->ldA;
    void* dst = at_off(h, h->dWhs, r0 * h->ldA);
    if (h->lp) hipLaunchKernelGGL(sum_chunks_kernel<bf16_t>, dim3(ew_blocks(n)), dim3(256), 0, st, (bf16_t*)dst, h->ldA, (const bf16_t*)dG + 4 * H, ldWS, nrow, A, RN_FCH);
    else hipLaunchKernelGGL(sum_chunks_kernel<float>, dim3(ew_blocks(n)), dim3(256), 0, st, (float*)dst, h->ldA, (const float*)dG + 4 * H, ldWS, nrow, A, RN_FCH);
  }
  // dW_hh (+)= sum_{t>=1} dgates_t^T h_{t-1} ; dW_attn (+)= sum_{t>=1} dWh_t^T h_{t-1}   (h_{-1} = 0)
  const int ta = t0 > 1 ? t0 : 1;
  if (t1 > ta) {
    const int nr = (t1 - ta) * B;
    const void* hp = at_off(h, h->Hs_lp, (size_t)(ta - 1) * B * h->ldH);
    dW_hh(h, h->dgru, H, at_off(h, h->dGx, (size_t)ta * B * ldWS), ldWS, hp, h->ldH, h->dGd.rnn_weight_hh_l0, nr, acc, st);
    gemm(h, at_off(h, h->dWhs, (size_t)ta * B * h->ldA), 1, h->ldA, hp, 1, h->ldH, h->dGd.attn_W_weight, H, nullptr, A, H, nr, 1.f, acc, st);
  } else if (!acc) {
    hipMemsetAsync(h->dGd.rnn_weight_hh_l0, 0, (size_t)GH * H * 4, st);
    hipMemsetAsync(h->dGd.attn_W_weight, 0, (size_t)A * H * 4, st);
  }
  return RECNET_OK;
}
// what needs the whole chain: bias gradients (column sums over all rows), d attn_U (dUv is complete after step 0), d attn_w
static int dec_bwd_deferred_tail(recnet_handle* h, hipStream_t st) {
  const int B = h->B, F = h->F, D = h->D, H = h->H, A = h->A, T = h->T_last, TB = T * B, ldWS = h->ldWS;
  gate_bias_grad(h, h->dGx, TB, H, ldWS, h->dGd.rnn_bias_ih_l0, h->dGd.rnn_bias_hh_l0, h->dgru, st);
  gemm(h, h->dUv_lp, 1, h->ldA, h->enc_lp, 1, h->ldD, h->dGd.attn_U_weight, D, nullptr, A, D, B * F, 1.f, 0, st);
  colsum_t<float>(h->dwacc, RN_FCH * B, A, A, h->dGd.attn_w_weight, st, h->ss.prezeroed);
  colsum_at(h, h->dWhs, TB, A, h->ldA, h->dGd.attn_b, st, h->ss.prezeroed);
  return RECNET_OK;
}
// bf16 path, round 4: the five weight-gradient products (dW_ih[:, :E], dW_ih[:, E:], dW_hh, dW_att, dU — every one dY^T . X) are
// ONE grouped launch on `st`, the embedding branch (d emb product + scatter) and the column sums run beside it on `st2`.
static int dec_bwd_deferred_grouped(recnet_handle* h, const float* enc, const int64_t* targets, hipStream_t st, hipStream_t st2, hipStream_t st3) {
  const int B = h->B, F = h->F, D = h->D, E = h->E, H = h->H, A = h->A, V = h->V, T = h->T_last, TB = T * B;
  const int train = h->train_last, ldWS = h->ldWS;
  const int GH = (h->dgru ? 3 : 4) * H;
  void* dG = h->dGx;
  // dWh_t: with the persistent BPTT chain the rows are [dgates | dWh | 0 ...] (dec_chain.hpp): the sum of the frame-chunk
  // partials IS the first chunk, read in place; the per-step kernels leave RN_FCH partials that sum_chunks adds up
  const void* dWh = at_off(h, dG, (size_t)4 * H); int ld_dwh = ldWS;
  if (!h->persist_dec_bwd) {
    const size_t n = (size_t)TB * h->ldA;
    hipLaunchKernelGGL(sum_chunks_kernel<bf16_t>, dim3(ew_blocks(n)), dim3(256), 0, st, (bf16_t*)h->dWhs, h->ldA, (const bf16_t*)dG + 4 * H, ldWS, TB, A, RN_FCH);
    dWh = h->dWhs; ld_dwh = h->ldA;
  }
  if (!h->ss.ctx_done) dec_ctx_rows(h, enc, 0, T, st);
  if (h->ss.side_tail_open) { hipStreamWaitEvent(st, h->ev[EV_SIDE_TAIL], 0); h->ss.side_tail_open = 0; }      // (the side branch's output-layer gradients and attended features)
  const bool two = st2 && st2 != st;
  if (two) fork_to(h, EV_TAIL2_FORK, st, st2);      // (behind sum_chunks: the column sum of dWh on st2 reads its output)
  // the bias gradients (column sums of dG / dWh / the attention vector's partials: four short launches that read only what the
  // BPTT left) on a third stream beside both branches — behind the embedding branch they were the last 40 us before the norms
  const bool three = two && st3 && st3 != st && st3 != st2;
  if (three) fork_to(h, EV_TAIL3_FORK, st, st3);
  GemmGroup g = gg_begin(1, 1);
  gg_add(h, g, dG, ldWS, h->ctx_lp, h->ldD, h->dGd.rnn_weight_ih_l0 + E, E + D, nullptr, GH, D, TB, 1.f, 0, st);
  gg_add(h, g, dG, ldWS, h->emb_lp, h->ldE, h->dGd.rnn_weight_ih_l0, E + D, nullptr, GH, E, TB, 1.f, 0, st);
  if (T > 1) {
    const int nr = (T - 1) * B;
    const void* hp = h->Hs_lp;                                            // h_{t-1} for the rows of step t >= 1
    const void* dG1 = at_off(h, dG, (size_t)B * ldWS);
    if (!h->dgru) gg_add(h, g, dG1, ldWS, hp, h->ldH, h->dGd.rnn_weight_hh_l0, H, nullptr, 4 * H, H, nr, 1.f, 0, st);
    else {
      gg_add(h, g, dG1, ldWS, hp, h->ldH, h->dGd.rnn_weight_hh_l0, H, nullptr, 2 * H, H, nr, 1.f, 0, st);
      gg_add(h, g, at_off(h, (void*)dG1, (size_t)3 * H), ldWS, hp, h->ldH, h->dGd.rnn_weight_hh_l0 + (size_t)2 * H * H, H, nullptr, H, H, nr, 1.f, 0, st);
    }
    gg_add(h, g, at_off(h, (void*)dWh, (size_t)B * ld_dwh), ld_dwh, hp, h->ldH, h->dGd.attn_W_weight, H, nullptr, A, H, nr, 1.f, 0, st);
  } else {
    hipMemsetAsync(h->dGd.rnn_weight_hh_l0, 0, (size_t)GH * H * 4, st);
    hipMemsetAsync(h->dGd.attn_W_weight, 0, (size_t)A * H * 4, st);
  }
  gg_add(h, g, h->dUv_lp, h->ldA, h->enc_lp, h->ldD, h->dGd.attn_U_weight, D, nullptr, A, D, B * F, 1.f, 0, st);
  gg_run(h, g, st, stamp_site(4));
  // ---- beside it: embedding branch + column sums.  With three streams the embedding branch (d emb product + two scatter kernels: the
  // longest thing beside the grouped launch) takes the THIRD one, which is idle when the BPTT ends — the second still runs the
  // reconstructor's in-step optimiser for ~20 us then —, and the short column sums queue behind that
  hipStream_t sb = three ? st3 : (two ? st2 : st);
  GemmOpts eo;
  eo.sum_in_launch = 1;      // (no reduction launch in front of the embedding scatter)
  if (two) eo.slots = h->ncu > 0 ? h->ncu / 2 : 128;      // (beside the grouped launch above)
  gemm(h, dG, 0, ldWS, h->We_w, 1, h->ldE, h->demb, E, nullptr, TB, E, 4 * H, 1.f, 0, sb, eo);
  if (!h->ss.prezeroed) hipMemsetAsync(h->dGd.embedding_weight, 0, (size_t)V * E * 4, sb);
  hipLaunchKernelGGL(embed_bwd_kernel, dim3(TB), dim3(128), 0, sb, h->dGd.embedding_weight, targets, h->demb, B, E, V,
                     h->c.embedding_scale, mkdrop(h, RN_SITE_DEC_EMBED, h->c.embedding_dropout, train), 0,
                     (const int64_t*)(h->free_fwd ? h->in_tok : nullptr));
  hipLaunchKernelGGL(embed_bwd_hot_kernel, dim3(cdiv(E, 128), cdiv(TB, RN_HOT_ROWS)), dim3(128), 0, sb, h->dGd.embedding_weight, targets, h->demb, B, E, V,
                     h->c.embedding_scale, mkdrop(h, RN_SITE_DEC_EMBED, h->c.embedding_dropout, train), 0, TB,
                     (const int64_t*)(h->free_fwd ? h->in_tok : nullptr));
  hipStream_t sc = three ? st2 : sb;
  gate_bias_grad(h, dG, TB, H, ldWS, h->dGd.rnn_bias_ih_l0, h->dGd.rnn_bias_hh_l0, h->dgru, sc);
  colsum_t<float>(h->dwacc, RN_FCH * B, A, A, h->dGd.attn_w_weight, sc, h->ss.prezeroed);
  colsum_at(h, dWh, TB, A, ld_dwh, h->dGd.attn_b, sc, h->ss.prezeroed);
  if (three) join_from(h, EV_TAIL3_JOIN, st, st3);
  return RECNET_OK;
}
static int dec_bwd_deferred(recnet_handle* h, const float* enc, const int64_t* targets, hipStream_t st, hipStream_t st2 = nullptr, hipStream_t st3 = nullptr) {
  RN_RANGE("recnet: decoder deferred weight gradients");
  if (h->lp) return dec_bwd_deferred_grouped(h, enc, targets, st, st2, st3);
  int r = dec_bwd_deferred_rows(h, enc, targets, 0, h->T_last, 0, st, st2); if (r) return r;
  return dec_bwd_deferred_tail(h, (st2 && st2 != st) ? st2 : st);
}
static int bwd_decoder(recnet_handle* h, const float* enc, const int64_t* targets, const float* dhid, float gscale,
                       hipStream_t st) {
  int r = dec_bwd_out(h, gscale, st); if (r) return r;
  r = dec_bwd_chain(h, dhid, st); if (r) return r;
  return dec_bwd_deferred(h, enc, targets, st);
}

