// Reconstructor sequences (train.py:78-131), global and local, and the optimiser step.
// Part of api.hip (one translation unit; see the include list there).
// ---------------------------------------------------------------------------------------------- global reconstructor
static void lstm_pw(recnet_handle* h, int Hd, int S, int slab_ld, const float* X, int x_ld, const float* b1, const float* b2,
                    const float* c_prev, float* h_out, void* h_lp, int hlp_ld, void* h_lp2, int hlp2_ld, float* c_out,
                    float* acts, hipStream_t st) {
  LstmPwArgs p;
  p.B = h->B; p.Hd = Hd; p.S = S; p.gru = h->rgru; p.slab = h->slab; p.slab_stride = (size_t)h->B * slab_ld; p.slab_ld = slab_ld;
  p.X = X; p.x_ld = x_ld; p.b1 = b1; p.b2 = b2; p.c_prev = c_prev; p.h_out = h_out; p.h_ld = Hd;
  p.h_lp = h_lp; p.hlp_ld = hlp_ld; p.hlp_pad_from = Hd; p.h_lp2 = h_lp2; p.hlp2_ld = hlp2_ld; p.c_out = c_out; p.acts = acts;
  auto al16 = [](const void* q) { return (((uintptr_t)q) & 15) == 0; };
  const bool vec = (Hd & 3) == 0 && (slab_ld & 3) == 0 && (x_ld & 3) == 0 && (hlp_ld & 3) == 0 && (hlp2_ld & 3) == 0 &&
                   al16(p.slab) && al16(X) && al16(b1) && al16(b2) && al16(c_prev) && al16(h_out) && al16(c_out) && al16(acts) &&
                   (((uintptr_t)h_lp) & 7) == 0 && (((uintptr_t)h_lp2) & 7) == 0;
  if (vec) LAUNCH_AT(h, lstm_pw_vec_kernel, dim3(cdiv((long)h->B * (Hd >> 2), 256)), dim3(256), 0, st, p);
  else LAUNCH_AT(h, lstm_pw_kernel, dim3(cdiv((long)h->B * Hd, 256)), dim3(256), 0, st, p);
}
static void mean_over_t(recnet_handle* h, const float* X, int T, int Cn, float scale, float* out, void* out_lp, int ld_lp, hipStream_t st) {
  const size_t n = (size_t)h->B * (out_lp ? ld_lp : Cn);
  if (h->lp) hipLaunchKernelGGL(mean_over_t_kernel<bf16_t>, dim3(ew_blocks(n)), dim3(256), 0, st, X, T, h->B, Cn, scale, out, (bf16_t*)out_lp, ld_lp);
  else hipLaunchKernelGGL(mean_over_t_kernel<float>, dim3(ew_blocks(n)), dim3(256), 0, st, X, T, h->B, Cn, scale, out, (float*)out_lp, ld_lp);
}

template <typename K, typename Args>
static void rc_launch(recnet_handle* h, int site, K kern, dim3 grid, size_t smem, hipStream_t st, const Args& a) {
  if (smem > 64 * 1024) hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  hipEvent_t e1 = nullptr;
  if (h->prof_on == site) {
    hipEvent_t e0 = nullptr;
    if (prof_take(h, st, &e0, &e1)) hipEventRecord(e0, st);
  }
  hipLaunchKernelGGL(kern, grid, dim3(256), smem, st, a);
  if (e1) hipEventRecord(e1, st);
}
// MSE against `ref` + d loss / d out in place (fp32) and, when the layout allows, as the scaled operand copy the
// backward's GEMMs read (scale = lambda_recon: what the fused step passes to the backward)
static void mse_and_dout(recnet_handle* h, float* out, const float* ref, int Sn, int rows_b, int R, size_t bstride, size_t sstride,
                         float gcoef, int nb, hipStream_t st) {
  const bool vec = (R & 3) == 0 && (((uintptr_t)out) & 15) == 0 && (((uintptr_t)ref) & 15) == 0 && (bstride & 3) == 0 && (sstride & 3) == 0;
  h->ss.dout_ready = 0;
  if (!vec) { hipLaunchKernelGGL(mse_kernel, dim3(nb), dim3(256), 0, st, out, ref, Sn, rows_b, R, bstride, sstride, gcoef, h->msep); return; }
  const bool lp = h->ldR == R;          // no padding columns to zero
  h->dout_scale = h->c.lambda_recon; h->ss.dout_ready = lp;
  if (h->lp) hipLaunchKernelGGL(mse_vec_kernel<bf16_t>, dim3(nb), dim3(256), 0, st, out, ref, Sn, rows_b, R, bstride, sstride, gcoef, h->msep,
                                lp ? (bf16_t*)h->dout_lp : (bf16_t*)nullptr, h->c.lambda_recon);
  else hipLaunchKernelGGL(mse_vec_kernel<float>, dim3(nb), dim3(256), 0, st, out, ref, Sn, rows_b, R, bstride, sstride, gcoef, h->msep,
                          lp ? (float*)h->dout_lp : (float*)nullptr, h->c.lambda_recon);
}
// norms_hoisted: the parameter norms and the gate bias come from hoist_side_work.  side != nullptr: the fused step's side work
// is forked from here, behind the batched input product.
// outputs_only (recnet_reconstruction_error): no regulariser norms, no loss epilogue, no MSE pass — h->outm is left holding the
// reconstruction mean_t out_t itself instead of d loss / d out, and h->scal is not written.
static int fwd_rec_global(recnet_handle* h, const float* enc, int T, int train, hipStream_t st, bool norms_hoisted, const SideWork* side,
                          bool outputs_only = false) {
  const int B = h->B, F = h->F, D = h->D, H = h->H, R = h->R;
  if (!norms_hoisted) {
    if (!outputs_only) param_norms(h, 1, h->scal + RN_SCAL_REC_REG, st);
    gate_bias(h->rP.rnn_bias_ih_l0, h->rP.rnn_bias_hh_l0, h->bsum_r, R, h->rgru, st);
  }
  // mean-pooled decoder states, rescaled by caption_max_len / T (global_reconstructor.py:33-37): (cml / T^2) sum_t h_t
  if (!h->ss.mp_done) mean_over_t(h, h->Hs, T, H, (float)h->cml / ((float)T * (float)T), h->mp, nullptr, 0, st);   // else: accumulated by dec_chain_kernel
  if (h->ss.xcat_done && h->ss.mp_done) {
    h->ss.xcat_done = 0;          // (dec_chain_kernel wrote the operand)
  } else {
    h->ss.xcat_done = 0;
    const size_t n = (size_t)T * B * h->ld2H;
    const DropDesc dd = mkdrop(h, RN_SITE_REC_INPUT, h->c.reconstructor_decoder_dropout, train);
    if (h->lp) hipLaunchKernelGGL(xcat_global_kernel<bf16_t>, dim3(ew_blocks(n)), dim3(256), 0, st, (const bf16_t*)h->Hs_lp, h->ldH, h->mp, (bf16_t*)h->Xcat_g, h->ld2H, T, B, H, dd, 0);
    else hipLaunchKernelGGL(xcat_global_kernel<float>, dim3(ew_blocks(n)), dim3(256), 0, st, (const float*)h->Hs_lp, h->ldH, h->mp, (float*)h->Xcat_g, h->ld2H, T, B, H, dd, 0);
  }
  // Xg = [h_t ; drop_t(mp)] . W_ih^T + b_ih + b_hh, batched over T (only h_r . W_hh^T is recurrent)
  gemm(h, h->Xcat_g, 0, h->ld2H, h->Wih_f, 0, h->ld2H, h->Xg, 4 * R, h->bsum_r, T * B, 4 * R, 2 * H, 1.f, 0, st);
  // The side work (vocabulary projection, CE, ...) is enqueued BEHIND the chain launch, with its fork event recorded in front of
  // it — so that the chain's workgroups, which need whole CUs, are dispatched before the projection's workgroups start filling
  // every CU partly (C2: 1.926 -> 1.913 ms)
  // (one-graph step only: in the data-parallel three-graph form it costs 0.17 ms — 2.31 against 2.14 ms at one rank)
  const bool side_late = h->ss.in_fused && side && h->overlap && h->s2 && h->persist_rec;
  int side_r = RECNET_OK;
  if (side_late) hipEventRecord(h->ev[EV_SIDE_FORK], st);
  else if (side) side_r = side_after_decoder_fwd(h, *side, st, false);       // see fwd_bwd_impl
  if (h->ss.rec_wait_pending) { hipStreamWaitEvent(st, h->ev[EV_PENDING_DONE], 0); h->ss.rec_wait_pending = 0; }      // W_hh's pending update (mode 2)
  // batches above RC_PAN_ROWS captions run the chain once per row group (h->bgrp rows each, csrc/api.hip): a group is an
  // independent batch for the chain — same weights, its own rows of every [T][B][.] tensor (row stride Bs = B)
  bool epi_done = false;
  for (int b0 = 0; b0 < B && h->persist_rec; b0 += h->bgrp) {
    const int nb = B - b0 < h->bgrp ? B - b0 : h->bgrp;
    RecChainArgs a;
    a.T = T; a.B = nb; a.Bs = B; a.R = R; a.gru = h->rgru;
    a.W = (const bf16_t*)h->Whh_w; a.ldw = h->ldR;
    a.Hlp = (bf16_t*)h->Hr_lp + (size_t)b0 * h->ldR; a.ld_hlp = h->ldR; a.Pan = (bf16_t*)h->Hr_pan;
    a.Xg = h->Xg + (size_t)b0 * 4 * R; a.H = h->Hr + (size_t)b0 * R; a.C = h->Cr + (size_t)b0 * R; a.acts = h->acts_r + (size_t)b0 * 4 * R;
    a.hmean = h->hrmean + (size_t)b0 * R; a.hmean_lp = (bf16_t*)h->hrmean_lp + (size_t)b0 * h->ldR; a.ld_hmean = h->ldR;
    a.bar = cs_ws_bar(h->gbar, CS_REC_FWD); a.epoch = cs_ws_epoch(h->gbar, CS_REC_FWD);
    a.master = R / 8 + 1 <= h->ncu;      // the master needs a CU of its own
    a.poison = h->scal + RN_SCAL_POISON;
    const int steps = (R + 127) / 128;
    a.epi = 0;
    // <4, 4>: two row halves x 16 units (less L2 -> L1 traffic per CU), when the batch has rows in both halves
    const int f_ms = h->sw.persist_ms;
    const bool split = f_ms ? f_ms == 2 : (nb > RC_PAN_ROWS / 2);
    if (split && (R & 15) == 0) {
      const dim3 g(R / 16 + a.master, 2);
      const size_t sm = rc_smem_bytes<4, 4>();
      // rec_epi 1: output layer + MSE + d out as an epilogue of the chain (rec_chain.hpp) instead of a split-K GEMM, its
      // reduction and the MSE kernel between the two chains (C2: 1.837 -> 1.815 ms)
      const int f_epi = h->sw.rec_epi;
      if (f_epi && !outputs_only && a.master && h->lp && h->ldR == R && nb == B && h->hm_pan) {
        if (!h->ss.encmean_hoisted) hipLaunchKernelGGL(mean_over_f_kernel, dim3(ew_blocks((size_t)B * D)), dim3(256), 0, st, enc, B, F, D, h->encmean);
        h->ss.encmean_hoisted = 1;
        const double cnt = (double)h->c.global_batch_size * R;
        a.epi = 1; a.Wo = (const bf16_t*)h->Wor_w; a.ldwo = h->ldR; a.obias = h->rP.out_bias; a.target = h->encmean;
        a.dout = h->outm; a.dout_lp = (bf16_t*)h->dout_lp; a.PanM = (bf16_t*)h->hm_pan; a.mse_part = h->msep;
        a.gcoef = (float)(2.0 / (cnt * T)); a.lp_scale = h->c.lambda_recon;
        // rec_epi 2: + d loss / d mean_t h_t = dout . W_o behind one more barrier phase (no product between the two chains)
        a.WoT = nullptr; a.ldwot = 0; a.PanD = nullptr; a.dhr = nullptr;
        if (f_epi > 1 && h->WoT && h->hd_pan && h->persist_rec_bwd) {
          a.epi = 2; a.WoT = (const bf16_t*)h->WoT; a.ldwot = h->ldR; a.PanD = (bf16_t*)h->hd_pan; a.dhr = h->dhrmean;
          h->ss.dhr_done = 1;
        }
        epi_done = true;
      }
      if (steps <= 4) rc_launch(h, RN_SITE_REC_CHAIN_FWD, (rec_chain_kernel<4, 2, 4, 4>), g, sm, st, a);
      else if (steps <= 8) rc_launch(h, RN_SITE_REC_CHAIN_FWD, (rec_chain_kernel<8, 3, 4, 4>), g, sm, st, a);
      else if (steps <= 12) rc_launch(h, RN_SITE_REC_CHAIN_FWD, (rec_chain_kernel<12, 2, 4, 4>), g, sm, st, a);
      else rc_launch(h, RN_SITE_REC_CHAIN_FWD, (rec_chain_kernel<16, 2, 4, 4>), g, sm, st, a);
    } else {
      const dim3 g(R / 8 + a.master, 1);
      const size_t sm = rc_smem_bytes<7, 2>();
      if (steps <= 4) rc_launch(h, RN_SITE_REC_CHAIN_FWD, (rec_chain_kernel<4, 2, 7, 2>), g, sm, st, a);
      else if (steps <= 8) rc_launch(h, RN_SITE_REC_CHAIN_FWD, (rec_chain_kernel<8, 3, 7, 2>), g, sm, st, a);
      else if (steps <= 12) rc_launch(h, RN_SITE_REC_CHAIN_FWD, (rec_chain_kernel<12, 2, 7, 2>), g, sm, st, a);
      else rc_launch(h, RN_SITE_REC_CHAIN_FWD, (rec_chain_kernel<16, 2, 7, 2>), g, sm, st, a);
    }
  }
  if (side_late) side_r = side_after_decoder_fwd(h, *side, st, true);
  for (int t = 0; t < T && !h->persist_rec; ++t) {
    int S = 0;
    if (t > 0) S = gemm_slabs(h, RN_TAG_REC_FWD, at_off(h, h->Hr_lp, (size_t)(t - 1) * B * h->ldR), h->ldR, h->Whh_w, 0, h->ldR, B, 4 * R, R, st);
    lstm_pw(h, R, S, 4 * R, h->Xg + (size_t)t * B * 4 * R, 4 * R, nullptr, nullptr,
            t > 0 ? (h->rgru ? h->Hr : h->Cr) + (size_t)(t - 1) * B * R : nullptr, h->Hr + (size_t)t * B * R,
            at_off(h, h->Hr_lp, (size_t)t * B * h->ldR), h->ldR, nullptr, 0, h->Cr + (size_t)t * B * R,
            h->acts_r + (size_t)t * B * 4 * R, st);
  }
  // mean_t out_t = (mean_t hr_t) . W_o^T + b_o  (train.py:96-98; `out` is linear so the mean commutes)
  if (!h->persist_rec) mean_over_t(h, h->Hr, T, R, 1.0f / (float)T, h->hrmean, h->hrmean_lp, h->ldR, st);   // (the chain kernel accumulates it)
  const double cnt = (double)h->c.global_batch_size * R;
  if (epi_done) {      // the chain's epilogue has done all of it
    h->ss.encmean_hoisted = 0;
    h->dout_scale = h->c.lambda_recon; h->ss.dout_ready = 1;
    h->mse_nb = (R / 16) * 2; h->mse_scale = (float)(1.0 / (cnt * T));
    return side_r;
  }
  gemm(h, h->hrmean_lp, 0, h->ldR, h->Wor_w, 0, h->ldR, h->outm, R, h->rP.out_bias, B, R, R, 1.f, 0, st);
  if (outputs_only) { h->ss.dout_ready = 0; return side_r; }
  if (!h->ss.encmean_hoisted) hipLaunchKernelGGL(mean_over_f_kernel, dim3(ew_blocks((size_t)B * D)), dim3(256), 0, st, enc, B, F, D, h->encmean);
  h->ss.encmean_hoisted = 0;
  const int nb = 256;
  mse_and_dout(h, h->outm, h->encmean, 1, B, R, (size_t)R, (size_t)0, (float)(2.0 / (cnt * T)), nb, st);
  h->mse_nb = nb; h->mse_scale = (float)(1.0 / (cnt * T));
  return side_r;
}

static void lstm_bwd(recnet_handle* h, int Hd, int S, int slab_ld, int slab_col0, const float* dh_direct, int dhd_ld,
                     float dh_scale, const float* acts, const float* c, const float* c_prev, float* dc_carry, int first,
                     void* dG, int ld_dg, hipStream_t st, const float* slab2 = nullptr, int S2 = 0) {
  LstmBwdArgs p;
  p.B = h->B; p.Hd = Hd; p.S = S; p.gru = h->rgru; p.dh_direct = dh_direct; p.dhd_ld = dhd_ld; p.dh_scale = dh_scale;
  p.slab = h->slab; p.slab_stride = (size_t)h->B * slab_ld; p.slab_ld = slab_ld; p.slab_col0 = slab_col0;
  p.slab2 = slab2; p.slab2_stride = (size_t)h->B * Hd; p.S2 = S2;
  p.acts = acts; p.c = c; p.c_prev = c_prev; p.dc_carry = dc_carry; p.first = first; p.dG = dG; p.ld_dg = ld_dg;
  auto al16 = [](const void* q) { return (((uintptr_t)q) & 15) == 0; };
  const bool vec = (Hd & 3) == 0 && (slab_ld & 3) == 0 && (slab_col0 & 3) == 0 && (dhd_ld & 3) == 0 && (ld_dg & 3) == 0 &&
                   al16(p.slab) && al16(slab2) && al16(dh_direct) && al16(acts) && al16(c) && al16(c_prev) && al16(dc_carry) &&
                   (((uintptr_t)dG) & 7) == 0;
  if (vec) LAUNCH_AT(h, lstm_bwd_vec_kernel, dim3(cdiv((long)h->B * (Hd >> 2), 256)), dim3(256), 0, st, p);
  else LAUNCH_AT(h, lstm_bwd_kernel, dim3(cdiv((long)h->B * Hd, 256)), dim3(256), 0, st, p);
}

static int bwd_rec_deferred(recnet_handle* h, hipStream_t st, int part, int which = 3);
static int optimizer_step(recnet_handle* h, int flags, hipStream_t st, int only_group = -1, int deferred = 0, int step_off = 0, unsigned skip_mask = 0u);
static bool rec_pending_hh_fused(recnet_handle* h, hipStream_t s, int step_off, int flags);
// Fused single-rank step: the reconstructor's deferred weight gradients and its optimiser step only need the backward CHAIN
// (the gate gradients), not the batched d hiddens products behind it: forked to the side stream right after the chain launch
// they get a head start of ~130 us over forking them in front of the decoder's BPTT, which is what the side stream was
// still busy with when the BPTT ended.  The join the BPTT needs (vocabulary-projection side work) is recorded first.
// Called by the backward chains for a caller that asked for it (bwd_rec_chain: fork_deferred); opt_flags >= 0: the optimiser step too.
static int rec_deferred_fork(recnet_handle* h, hipStream_t st, int opt_flags) {
  hipStream_t sd = h->s2;
  if (h->ss.join_pending) { hipEventRecord(h->ev[EV_SIDE_JOIN], sd); h->ss.join_recorded = 1; }
  fork_to(h, EV_REC_DW_FORK, st, sd);
  int r = bwd_rec_deferred(h, sd, 0); if (r) return r;
  h->ss.deferred_done = 1;
  if (opt_flags >= 0) {
    r = optimizer_step(h, opt_flags, sd, 1); if (r) return r;
    h->ss.early_opt_done = 1;
  }
  return RECNET_OK;
}

// fork_deferred: the deferred weight gradients are forked to the side stream right behind the chain (rec_deferred_fork)
static int bwd_rec_global(recnet_handle* h, float gscale, float* dhid_out, hipStream_t st, bool fork_deferred, int opt_flags) {
  const int B = h->B, H = h->H, R = h->R, T = h->T_last, TB = T * B, ld4R = h->ld4R;
  const int train = h->train_last;
  // dout (operand copy) = gscale * d loss / d out_mean
  // (the output layer's own gradients do not feed the chain: bwd_rec_global_deferred)
  const bool had_dout = h->ss.dout_ready && h->dout_scale == gscale;      // (else the epilogue's dhrmean carries another scale)
  if (!had_dout) pack_block(h, h->dout_lp, h->ldR, h->outm, R, B, R, gscale, st);
  h->ss.dout_ready = 0;
  if (!(h->ss.dhr_done && had_dout)) gemm(h, h->dout_lp, 0, h->ldR, h->Wor_w, 1, h->ldR, h->dhrmean, R, nullptr, B, R, R, 1.f, 0, st);
  h->ss.dhr_done = 0;
  int S = 0;
  for (int b0 = 0; b0 < B && h->persist_rec_bwd; b0 += h->bgrp) {      // one launch per row group (see fwd_rec_global)
    const int nb = B - b0 < h->bgrp ? B - b0 : h->bgrp;
    RecChainBwdArgs a;
    a.T = T; a.B = nb; a.Bs = B; a.R = R; a.gru = h->rgru;
    a.Wt = (const bf16_t*)h->WhhT; a.ldwt = ld4R;
    a.Pan = (bf16_t*)h->dG_pan; a.dG = (bf16_t*)h->dGr + (size_t)b0 * ld4R; a.ld_dg = ld4R;
    a.dh_direct = h->dhrmean + (size_t)b0 * R; a.dh_scale = 1.0f / (float)T;
    a.acts = h->acts_r + (size_t)b0 * 4 * R; a.C = h->Cr + (size_t)b0 * R; a.H = h->Hr + (size_t)b0 * R;
    a.bar = cs_ws_bar(h->gbar, CS_REC_BWD); a.epoch = cs_ws_epoch(h->gbar, CS_REC_BWD);
    a.master = (R / 16) * (nb > 64 ? 2 : 1) + 1 <= h->ncu;
    a.poison = h->scal + RN_SCAL_POISON;
    const int steps = (4 * R + 127) / 128;
    // above 64 captions and up to R = 1536: 32 units x 32 rows per workgroup (a third of its weights in LDS), four row parts
    const int f_wide = h->sw.rec_wide;
    const bool wide = f_wide && nb > 64 && (R & 31) == 0 && steps > 32 && steps <= 48 && (R / 32) * 4 + 1 <= h->ncu;
    if (wide) a.master = 1;
    const dim3 g((wide ? R / 32 : R / 16) + a.master, wide ? 4 : (nb > 64 ? 2 : 1));
    const size_t sm = rc_bwd_smem_bytes<4, 1>();
    if (wide) {
      constexpr size_t smw = rc_bwd_smem_bytes<2, 2, 16>();
      rc_launch(h, RN_SITE_REC_CHAIN_BWD, (rec_chain_bwd_kernel<48, 3, 2, 2, 16>), g, smw, st, a);
    } else if (steps <= 8) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (rec_chain_bwd_kernel<8, 3, 4, 1>), g, sm, st, a);
    else if (steps <= 16) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (rec_chain_bwd_kernel<16, 3, 4, 1>), g, sm, st, a);
    else if (steps <= 32) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (rec_chain_bwd_kernel<32, 3, 4, 1>), g, sm, st, a);
    else if (steps <= 48) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (rec_chain_bwd_kernel<48, 3, 4, 1>), g, sm, st, a);
    else rc_launch(h, RN_SITE_REC_CHAIN_BWD, (rec_chain_bwd_kernel<64, 2, 4, 1>), g, sm, st, a);
  }
  for (int t = T - 1; t >= 0 && !h->persist_rec_bwd; --t) {
    lstm_bwd(h, R, S, R, 0, h->dhrmean, R, 1.0f / (float)T, h->acts_r + (size_t)t * B * 4 * R, h->Cr + (size_t)t * B * R,
             t > 0 ? (h->rgru ? h->Hr : h->Cr) + (size_t)(t - 1) * B * R : nullptr, h->dcr_carry, t == T - 1, at_off(h, h->dGr, (size_t)t * B * ld4R), ld4R, st);
    if (t > 0) S = gemm_slabs(h, RN_TAG_REC_BWD, at_off(h, h->dGr, (size_t)t * B * ld4R), ld4R, h->Whh_w, 1, h->ldR, B, R, 4 * R, st);
  }
  if (fork_deferred) { const int rr = rec_deferred_fork(h, st, opt_flags); if (rr) return rr; }
  // input-side gradients, batched: ONE product over both halves of W_ih (the h_t half and the pooled-states half), then one
  // kernel that folds the pooled half through its dropout masks and the 1 / T^2 pooling back onto every step
  // (Leaving the K slices of this product in their slabs for global_dhid_kernel to add up — one launch less in front of the
  // decoder's BPTT — was measured in round 4: no change, 1.699 against 1.683 ms within the box's spread; not kept.)
  // (a group of one: the K slices are summed inside the launch by the last-arriving slice — the separate reduction kernel was 17 us of the
  //  gap in front of the decoder's BPTT, where the side stream's weight-gradient products still run)
  GemmOpts go;
  go.sum_in_launch = 1;
  gemm(h, h->dGr, 0, ld4R, h->Wih_f, 1, h->ld2H, h->dmpd, 2 * H, nullptr, TB, 2 * H, 4 * R, 1.f, 0, st, go);
  hipLaunchKernelGGL(global_dhid_kernel, dim3((unsigned)(((size_t)B * H + 63) / 64)), dim3(256), 0, st, h->dmpd, dhid_out, T, B, H,
                     (float)h->cml / ((float)T * (float)T), mkdrop(h, RN_SITE_REC_INPUT, h->c.reconstructor_decoder_dropout, train));
  return RECNET_OK;
}
// which: bit 0 = the recurrent weights' product (dW_hh), bit 1 = everything else (dW_ih, the output layer, the bias sums) — the
// split reconstructor update (recnet_set_deferred_reconstructor_update, mode 2) runs the two halves in different steps
static int bwd_rec_global_deferred(recnet_handle* h, hipStream_t st, int which = 3) {
  // (deferred update: the products always run over caption_max_len + 1 steps — the graph that runs them was captured
  // without knowing the length of the step before; the step itself zeroed the gate gradients of the steps it did not run)
  const int B = h->B, H = h->H, R = h->R, T = h->def_rows ? h->Tm : h->T_last, TB = T * B, ld4R = h->ld4R;
  const int GR = (h->rgru ? 3 : 4) * R;
  // (bf16 path: the three products dY^T . X are one grouped launch, gemm_lds.hpp; the fp32 path runs them one by one)
  GemmGroup g = gg_begin(1, 1);
  if (!(which & 1)) {
  } else if (T > 1) {
    const void* dG1 = at_off(h, h->dGr, (size_t)B * ld4R);
    const int nr = (T - 1) * B;
    if (!h->rgru) gg_add(h, g, dG1, ld4R, h->Hr_lp, h->ldR, h->rG.rnn_weight_hh_l0, R, nullptr, 4 * R, R, nr, 1.f, 0, st);
    else {
      gg_add(h, g, dG1, ld4R, h->Hr_lp, h->ldR, h->rG.rnn_weight_hh_l0, R, nullptr, 2 * R, R, nr, 1.f, 0, st);
      gg_add(h, g, at_off(h, (void*)dG1, (size_t)3 * R), ld4R, h->Hr_lp, h->ldR, h->rG.rnn_weight_hh_l0 + (size_t)2 * R * R, R, nullptr, R, R, nr, 1.f, 0, st);
    }
  } else {
    hipMemsetAsync(h->rG.rnn_weight_hh_l0, 0, (size_t)GR * R * 4, st);
  }
  if (!(which & 2)) { gg_run(h, g, st, stamp_site(3)); return RECNET_OK; }
  gg_add(h, g, h->dGr, ld4R, h->Xcat_g, h->ld2H, h->rG.rnn_weight_ih_l0, 2 * H, nullptr, GR, 2 * H, TB, 1.f, 0, st);   // d W_ih = dG^T . [h_t ; drop(mp)]
  gg_add(h, g, h->dout_lp, h->ldR, h->hrmean_lp, h->ldR, h->rG.out_weight, R, nullptr, R, R, B, 1.f, 0, st);            // d W_o = dout^T . mean_t hr_t
  // the column sums first: in the fused step this stream runs beside the decoder's BPTT chain, whose whole-CU workgroups must
  // be resident before the grouped launch's ~1000 workgroups start filling every CU (they were 480 instead of 325 us otherwise)
  colsum_at(h, h->dout_lp, B, R, h->ldR, h->rG.out_bias, st, h->ss.prezeroed);
  gate_bias_grad(h, h->dGr, TB, R, ld4R, h->rG.rnn_bias_ih_l0, h->rG.rnn_bias_hh_l0, h->rgru, st);
  gg_run(h, g, st, stamp_site(2));
  return RECNET_OK;
}

// ---------------------------------------------------------------------------------------------- local reconstructor
// outputs_only: see fwd_rec_global — h->outl [F][B][R] is left holding the reconstruction out_f itself.
static int fwd_rec_local(recnet_handle* h, const float* enc, int T, int train, hipStream_t st, bool norms_hoisted, bool outputs_only = false) {
  const int B = h->B, F = h->F, D = h->D, H = h->H, R = h->R, RA = h->RA, ldHR = h->ldHR;
  const size_t esz = h->lp ? 2 : 4;
  if (!norms_hoisted) {
    if (!outputs_only) param_norms(h, 1, h->scal + RN_SCAL_REC_REG, st);
    gate_bias(h->rP.rnn_bias_ih_l0, h->rP.rnn_bias_hh_l0, h->bsum_r, R, h->rgru, st);
  }
  // Ud = hiddens . U_r^T   (local_reconstructor.py:42, hoisted)
  gemm(h, h->Hs_lp, 0, h->ldH, h->Ur_w, 0, h->ldH, h->Ud, RA, nullptr, T * B, RA, H, 1.f, 0, st);
  if (h->ss.rec_wait_pending) { hipStreamWaitEvent(st, h->ev[EV_PENDING_DONE], 0); h->ss.rec_wait_pending = 0; }      // W_hh's pending update (mode 2)
  if (h->persist_loc) for (int b0 = 0; b0 < B; b0 += h->bgrp_loc) {      // one launch per row group (see fwd_rec_global; bgrp_loc: recnet_create)
    const int nb = B - b0 < h->bgrp_loc ? B - b0 : h->bgrp_loc;
    LocChainArgs a;
    a.F = F; a.T = T; a.B = nb; a.Bs = B; a.R = R; a.H = H; a.A = RA; a.gru = h->rgru;
    a.NG = h->lc_ng; a.MS = h->lc_ms; a.NU = a.NG * a.MS; a.NC = (nb + LC_CPW - 1) / LC_CPW;
    a.relay = a.NU + a.NC + 1 <= h->ncu;     // else: no CU left for the relay workgroup, every waiter polls the flags
    a.W = (const bf16_t*)h->Wihh_w; a.ldw = ldHR; a.Wr = (const bf16_t*)h->Wr_w; a.ldwr = h->ldR; a.bias = h->bsum_r; a.Wst = (const bf16_t*)h->Wst;
    a.Hs = h->Hs + (size_t)b0 * H; a.Ud = h->Ud + (size_t)b0 * RA; a.ab = h->rP.attn_b; a.w = h->rP.attn_w_weight;
    a.Hr = h->Hr + (size_t)b0 * R; a.Cr = h->Cr + (size_t)b0 * R; a.acts = h->acts_r + (size_t)b0 * 4 * R; a.Hlp = (bf16_t*)h->Hr_lp + (size_t)b0 * h->ldR; a.ld_hlp = h->ldR;
    a.Xcat = (bf16_t*)h->Xcat_r + (size_t)b0 * ldHR; a.ld_xcat = ldHR; a.beta = h->beta + (size_t)b0 * T; a.Whr = h->Whr + (size_t)b0 * RA;
    a.PanH = (bf16_t*)h->lc_panh; a.PanX = (bf16_t*)h->lc_panx; a.Pw = h->lc_pw;
    a.bar = cs_ws_bar(h->gbar, CS_LOC_FWD); a.epoch = cs_ws_epoch(h->gbar, CS_LOC_FWD); a.poison = h->scal + RN_SCAL_POISON;
    a.dd = mkdrop(h, RN_SITE_REC_INPUT, h->c.reconstructor_decoder_dropout, train); a.dd.boff += b0; a.ts = h->lc_ts;
    const dim3 g(a.NU + a.NC + a.relay);
    const int steps = (R + 127) / 128;
    if (steps > 16) {
      // R above 2048 (C5: R = 3584): hybrid — LC_HYB_SR k-steps per wave resident in registers, the rest streamed every step
      if (h->lc_rb == 2) {
        const size_t sm = lc_smem_bytes<2>();
        if (steps <= 28) rc_launch(h, RN_SITE_REC_CHAIN_FWD, (loc_chain_kernel<28, 2, 2, LC_HYB_SR(28), 64>), g, sm, st, a);
        else rc_launch(h, RN_SITE_REC_CHAIN_FWD, (loc_chain_kernel<32, 2, 2, LC_HYB_SR(32), 64>), g, sm, st, a);
      } else {
        const size_t sm = lc_smem_bytes<4>();
        if (steps <= 28) rc_launch(h, RN_SITE_REC_CHAIN_FWD, (loc_chain_kernel<28, 2, 4, LC_HYB_SR(28), 64>), g, sm, st, a);
        else rc_launch(h, RN_SITE_REC_CHAIN_FWD, (loc_chain_kernel<32, 2, 4, LC_HYB_SR(32), 64>), g, sm, st, a);
      }
    } else if (h->lc_rb == 2) {
      const size_t sm = lc_smem_bytes<2>();
      if (steps <= 4) rc_launch(h, RN_SITE_REC_CHAIN_FWD, (loc_chain_kernel<4, 2, 2>), g, sm, st, a);
      else if (steps <= 8) rc_launch(h, RN_SITE_REC_CHAIN_FWD, (loc_chain_kernel<8, 2, 2>), g, sm, st, a);
      else if (steps <= 12) rc_launch(h, RN_SITE_REC_CHAIN_FWD, (loc_chain_kernel<12, 2, 2>), g, sm, st, a);
      else rc_launch(h, RN_SITE_REC_CHAIN_FWD, (loc_chain_kernel<16, 2, 2>), g, sm, st, a);
    } else {
      const size_t sm = lc_smem_bytes<4>();
      if (steps <= 4) rc_launch(h, RN_SITE_REC_CHAIN_FWD, (loc_chain_kernel<4, 2, 4>), g, sm, st, a);
      else if (steps <= 8) rc_launch(h, RN_SITE_REC_CHAIN_FWD, (loc_chain_kernel<8, 2, 4>), g, sm, st, a);
      else if (steps <= 12) rc_launch(h, RN_SITE_REC_CHAIN_FWD, (loc_chain_kernel<12, 2, 4>), g, sm, st, a);
      else rc_launch(h, RN_SITE_REC_CHAIN_FWD, (loc_chain_kernel<16, 2, 4>), g, sm, st, a);
    }
  } else {
    hipMemsetAsync(h->Xcat_r, 0, (size_t)F * B * ldHR * esz, st);   // hr_{-1} = 0 and the zero padding of every row
    LocAttnArgs a;
    a.B = B; a.T = T; a.H = H; a.A = RA; a.Ud = h->Ud; a.ab = h->rP.attn_b; a.w = h->rP.attn_w_weight; a.Hs = h->Hs;
    a.xcat_ld = ldHR; a.dd = mkdrop(h, RN_SITE_REC_INPUT, h->c.reconstructor_decoder_dropout, train);
    const size_t sm = (size_t)(RA + T + 16) * 4;
    for (int s = 0; s < F; ++s) {
      int Sa = 0;
      if (s > 0) Sa = gemm_slabs(h, RN_TAG_REC_ATT, at_off(h, h->Hr_lp, (size_t)(s - 1) * B * h->ldR), h->ldR, h->Wr_w, 0, h->ldR, B, RA, R, st);
      a.s = s; a.S = Sa; a.slab = s > 0 ? h->slab : nullptr;
      a.Whr_out = h->Whr + (size_t)s * B * RA; a.beta_out = h->beta + (size_t)s * B * T;
      a.xcat = at_off(h, h->Xcat_r, (size_t)s * B * ldHR);
      LAUNCH_AT(h, loc_attn_fwd_kernel, dim3(B, cdiv(H, 256)), dim3(256), sm, st, a);
      const int Sb = gemm_slabs(h, RN_TAG_REC_FWD, at_off(h, h->Xcat_r, (size_t)s * B * ldHR), ldHR, h->Wihh_w, 0, ldHR, B, 4 * R, H + R, st);
      lstm_pw(h, R, Sb, 4 * R, nullptr, 0, h->bsum_r, nullptr,
              s > 0 ? (h->rgru ? h->Hr : h->Cr) + (size_t)(s - 1) * B * R : nullptr, h->Hr + (size_t)s * B * R,
              at_off(h, h->Hr_lp, (size_t)s * B * h->ldR), h->ldR,
              s + 1 < F ? at_off(h, h->Xcat_r, (size_t)(s + 1) * B * ldHR + H) : nullptr, ldHR, h->Cr + (size_t)s * B * R,
              h->acts_r + (size_t)s * B * 4 * R, st);
    }
  }
  // (264 tiles — one workgroup per CU; K slices summed inside a grouped launch instead was measured in round 4 for this product
  // and for the d-hiddens product of bwd_rec_local: no change, 2.087 / 2.095 against 2.084 ms)
  const double cnt = (double)h->c.global_batch_size * F * D;
  // bf16 path: MSE + d loss / d out in the output layer's own epilogue (one launch instead of product, MSE kernel and the 17 MB of
  // `out` in between); the partial sums are per output tile
  const int tiles = ((F * B + 127) / 128) * ((R + 127) / 128);      // (128 x 128 output tiles: gemm_lds.hpp)
  const int f_me = h->sw.mse_epi;
  if (f_me && !outputs_only && h->lp && h->ldR == R && (R & 3) == 0 && (D & 3) == 0 && tiles <= 1024 && (((uintptr_t)enc) & 15) == 0 && (((uintptr_t)h->outl) & 15) == 0) {
    RnMse m; m.ref = enc; m.part = h->msep; m.bstride = (size_t)F * D; m.sstride = (size_t)D; m.B = B; m.gcoef = (float)(2.0 / cnt); m.lp = h->c.lambda_recon;
    rn_launch_gemm(h->prec, h->Hr_lp, 1, 0, h->ldR, h->Wor_w, 1, 0, h->ldR, h->outl, R, h->rP.out_bias, F * B, R, R, 1.f, 0, 1, nullptr, 0, st, 0, 0,
                   h->dout_lp, h->ldR, &m);
    h->dout_scale = h->c.lambda_recon; h->ss.dout_ready = 1;
    h->mse_nb = tiles; h->mse_scale = (float)(1.0 / cnt);
    return RECNET_OK;
  }
  gemm(h, h->Hr_lp, 0, h->ldR, h->Wor_w, 0, h->ldR, h->outl, R, h->rP.out_bias, F * B, R, R, 1.f, 0, st);
  if (outputs_only) { h->ss.dout_ready = 0; return RECNET_OK; }
  const int nb = 512;
  mse_and_dout(h, h->outl, enc, F, B, R, (size_t)F * D, (size_t)D, (float)(2.0 / cnt), nb, st);
  h->mse_nb = nb; h->mse_scale = (float)(1.0 / cnt);
  return RECNET_OK;
}

static int bwd_rec_local(recnet_handle* h, float gscale, float* dhid_out, hipStream_t st, bool fork_deferred, int opt_flags) {
  const int B = h->B, F = h->F, H = h->H, R = h->R, RA = h->RA, T = h->T_last, TB = T * B, FB = F * B;
  const int train = h->train_last, ld4R = h->ld4R, ldHR = h->ldHR;
  // (the output layer's own gradients do not feed the chain: bwd_rec_local_deferred)
  if (!(h->ss.dout_ready && h->dout_scale == gscale)) pack_block(h, h->dout_lp, h->ldR, h->outl, R, FB, R, gscale, st);
  h->ss.dout_ready = 0;
  gemm(h, h->dout_lp, 0, h->ldR, h->Wor_w, 1, h->ldR, h->dHr, R, nullptr, FB, R, R, 1.f, 0, st);
  h->lc_bwd_done = 0;
  if (h->persist_big_bwd) {
    // R above 2048: the phased chain of loc_big.hpp, then the two kernels that rebuild the sums over s its caption phase leaves out
   for (int b0 = 0; b0 < B; b0 += h->bgrp_loc) {      // one launch per row group of <= 64 captions (round 6; see fwd_rec_global): every [s][B][.] tensor by the caption's row in the whole batch
    const int nb = B - b0 < h->bgrp_loc ? B - b0 : h->bgrp_loc;
    LocBigBwdArgs c;
    c.F = F; c.T = T; c.B = nb; c.Bs = B; c.R = R; c.H = H; c.A = RA; c.gru = h->rgru;
    c.NCB = h->lb_ncb; c.NWG = h->lb_ncb * 4;
    c.WT = (const bf16_t*)h->WihhT; c.ldwt = ld4R; c.WstT = (const bf16_t*)h->WstT; c.Wr = (const bf16_t*)h->Wr_w; c.ldwr = h->ldR;
    c.dHr = h->dHr + (size_t)b0 * R; c.acts = h->acts_r + (size_t)b0 * 4 * R; c.Cr = h->Cr + (size_t)b0 * R; c.Hr = h->Hr + (size_t)b0 * R;
    c.Hs = h->Hs + (size_t)b0 * H; c.Ud = h->Ud + (size_t)b0 * RA; c.ab = h->rP.attn_b; c.w = h->rP.attn_w_weight; c.Whr = h->Whr + (size_t)b0 * RA;
    c.dG = (bf16_t*)h->dGr + (size_t)b0 * ld4R; c.ld_dg = ld4R; c.dWhrs = (bf16_t*)h->dWhrs + (size_t)b0 * h->ldRA; c.ld_dwhr = h->ldRA;
    c.dxm = h->lb_dxm + (size_t)b0 * H; c.dbeta = h->lb_dbeta + (size_t)b0 * T;
    c.PanG = (bf16_t*)h->lc_pang; c.PanW = (bf16_t*)h->lc_panw; c.Part = h->lb_part;
    c.bar = cs_ws_bar(h->gbar, CS_LOC_BWD); c.epoch = cs_ws_epoch(h->gbar, CS_LOC_BWD); c.poison = h->scal + RN_SCAL_POISON;
    c.dd = mkdrop(h, RN_SITE_REC_INPUT, h->c.reconstructor_decoder_dropout, train); c.dd.boff += b0; c.ts = h->lc_ts;
    const dim3 g(c.NWG);
    // (round 4: every even R / 128 in 18 ... 32, i.e. R = 2304 ... 4096 in steps of 256 — round 3 had the benchmark's 24 / 28 / 32 only)
    if (h->lb_steps == 18) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (lcbig_bwd_kernel<18, LB_SR(18), LB_PF, LB_NL>), g, lcbig_smem_bytes<LB_NL>(), st, c);
    else if (h->lb_steps == 20) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (lcbig_bwd_kernel<20, LB_SR(20), LB_PF, LB_NL>), g, lcbig_smem_bytes<LB_NL>(), st, c);
    else if (h->lb_steps == 22) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (lcbig_bwd_kernel<22, LB_SR(22), LB_PF, LB_NL>), g, lcbig_smem_bytes<LB_NL>(), st, c);
    else if (h->lb_steps == 24) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (lcbig_bwd_kernel<24, LB_SR(24), LB_PF, LB_NL>), g, lcbig_smem_bytes<LB_NL>(), st, c);
    else if (h->lb_steps == 26) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (lcbig_bwd_kernel<26, LB_SR(26), LB_PF, LB_NL>), g, lcbig_smem_bytes<LB_NL>(), st, c);
    else if (h->lb_steps == 30) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (lcbig_bwd_kernel<30, LB_SR(30), LB_PF, LB_NL>), g, lcbig_smem_bytes<LB_NL>(), st, c);
    else if (h->lb_steps == 28) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (lcbig_bwd_kernel<28, LB_SR(28), LB_PF, LB_NL>), g, lcbig_smem_bytes<LB_NL>(), st, c);
    else rc_launch(h, RN_SITE_REC_CHAIN_BWD, (lcbig_bwd_kernel<32, LB_SR(32), LB_PF, LB_NL>), g, lcbig_smem_bytes<LB_NL>(), st, c);
   }
    hipLaunchKernelGGL(lcbig_dhs_kernel, dim3(B, cdiv(H, 256), 2), dim3(256), 0, st, (const float*)h->beta, (const float*)h->lb_dxm, dhid_out, F, T, B, H);
    static_assert(RN_TCH == 4, "lcbig_dud_kernel writes one dwacc chunk per quarter of the decoder steps");
    hipLaunchKernelGGL(lcbig_dud_kernel, dim3(B, 4), dim3(256), 0, st, (const float*)h->lb_dbeta, (const float*)h->Whr, (const float*)h->Ud,
                       (const float*)h->rP.attn_b, (const float*)h->rP.attn_w_weight, h->dUd, (bf16_t*)h->dUd_lp, h->ldRA, h->dwacc_r, RN_TCH, F, T, B, RA);
    h->lc_bwd_done = 1;
  } else if (h->persist_loc_bwd) {
   for (int b0 = 0; b0 < B; b0 += h->bgrp_loc) {      // one launch per row group (see fwd_rec_global)
    const int nb = B - b0 < h->bgrp_loc ? B - b0 : h->bgrp_loc;
    LocChainBwdArgs c;
    c.F = F; c.T = T; c.B = nb; c.Bs = B; c.R = R; c.H = H; c.A = RA; c.gru = h->rgru;
    c.NGU = h->lc_ng; c.MSU = 1; c.NGX = H / 16; c.MSX = h->lcb_msx; c.NC = (nb + LC_CPW - 1) / LC_CPW; c.KSX = 1;
    if (h->lcb_xs) { c.NGX = (H + 63) / 64; c.MSX = (nb + 31) / 32; c.KSX = (4 * R + h->lcb_xs * 128 - 1) / (h->lcb_xs * 128); }
    c.WT = (const bf16_t*)h->WihhT; c.ldwt = ld4R; c.Wr = (const bf16_t*)h->Wr_w; c.ldwr = h->ldR;
    c.dHr = h->dHr + (size_t)b0 * R; c.acts = h->acts_r + (size_t)b0 * 4 * R; c.Cr = h->Cr + (size_t)b0 * R; c.Hr = h->Hr + (size_t)b0 * R;
    c.Hs = h->Hs + (size_t)b0 * H; c.Ud = h->Ud + (size_t)b0 * RA; c.ab = h->rP.attn_b; c.w = h->rP.attn_w_weight; c.Whr = h->Whr + (size_t)b0 * RA; c.beta = h->beta + (size_t)b0 * T;
    c.dG = (bf16_t*)h->dGr + (size_t)b0 * ld4R; c.ld_dg = ld4R; c.dWhrs = (bf16_t*)h->dWhrs + (size_t)b0 * h->ldRA; c.ld_dwhr = h->ldRA;
    c.dHs = dhid_out + (size_t)b0 * H; c.dUd = h->dUd + (size_t)b0 * RA; c.dUd_lp = (bf16_t*)h->dUd_lp + (size_t)b0 * h->ldRA; c.ld_dUd = h->ldRA; c.dwacc = h->dwacc_r + (size_t)b0 * RA; c.nch = RN_TCH;
    c.PanG = (bf16_t*)h->lc_pang; c.PanW = (bf16_t*)h->lc_panw; c.Dx = h->lc_dx;
    c.bar = cs_ws_bar(h->gbar, CS_LOC_BWD); c.epoch = cs_ws_epoch(h->gbar, CS_LOC_BWD); c.poison = h->scal + RN_SCAL_POISON;
    c.dd = mkdrop(h, RN_SITE_REC_INPUT, h->c.reconstructor_decoder_dropout, train); c.dd.boff += b0; c.ts = h->lc_ts;
    // (measured and rejected: U' waiting for X' to publish dx before its recurrent product, +0.08 ms at B = 100 — X' is bound by its
    // own CU's L1 fill rate, not by U')
    const dim3 g(c.NGU * c.MSU + c.NGX * c.MSX * c.KSX + c.NC + 1);
    const int steps = (4 * R + 127) / 128;
    if (h->lcb_xs) {      // X' with the contraction split over workgroups (lcb_xsplit_role)
      if (h->lcb_rbu == 7) {
        if (steps <= 32) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<32, 2, 7, 4, 16>), g, lcb_smem_bytes<7, 4, 16>(), st, c);
        else rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<48, 2, 7, 4, 16>), g, lcb_smem_bytes<7, 4, 16>(), st, c);
      } else if (h->lcb_rbu == 2) {
        if (steps <= 32) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<32, 3, 2, 2, 16>), g, lcb_smem_bytes<2, 2, 16>(), st, c);
        else if (steps <= 48) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<48, 3, 2, 2, 16>), g, lcb_smem_bytes<2, 2, 16>(), st, c);
        else rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<64, 3, 2, 2, 16>), g, lcb_smem_bytes<2, 2, 16>(), st, c);
      } else {
        if (steps <= 32) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<32, 3, 4, 4, 16>), g, lcb_smem_bytes<4, 4, 16>(), st, c);
        else if (steps <= 48) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<48, 3, 4, 4, 16>), g, lcb_smem_bytes<4, 4, 16>(), st, c);
        else rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<64, 2, 4, 4, 16>), g, lcb_smem_bytes<4, 4, 16>(), st, c);
      }
    } else if (h->lcb_rbu == 7) {
      const size_t sm = lcb_smem_bytes<7, 4>();
      if (steps <= 8) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<8, 3, 7, 4>), g, sm, st, c);
      else if (steps <= 16) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<16, 3, 7, 4>), g, sm, st, c);
      else if (steps <= 32) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<32, 2, 7, 4>), g, sm, st, c);
      else rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<48, 2, 7, 4>), g, sm, st, c);
    } else if (h->lcb_rbu == 2) {    // at most 32 captions: one 32-row block per workgroup
      const size_t sm = lcb_smem_bytes<2, 2>();
      if (steps <= 8) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<8, 3, 2, 2>), g, sm, st, c);
      else if (steps <= 16) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<16, 3, 2, 2>), g, sm, st, c);
      else if (steps <= 32) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<32, 3, 2, 2>), g, sm, st, c);
      else if (steps <= 48) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<48, 3, 2, 2>), g, sm, st, c);
      else rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<64, 3, 2, 2>), g, sm, st, c);
    } else {
      const size_t sm = lcb_smem_bytes<4, 4>();
      if (steps <= 8) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<8, 3, 4, 4>), g, sm, st, c);
      else if (steps <= 16) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<16, 3, 4, 4>), g, sm, st, c);
      else if (steps <= 32) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<32, 3, 4, 4>), g, sm, st, c);
      else if (steps <= 48) rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<48, 3, 4, 4>), g, sm, st, c);
      else rc_launch(h, RN_SITE_REC_CHAIN_BWD, (loc_chain_bwd_kernel<64, 2, 4, 4>), g, sm, st, c);
    }
   }
    h->lc_bwd_done = 1;
  } else {
    LocBwdArgs a;
    a.B = B; a.T = T; a.H = H; a.R = R; a.A = RA;
    a.Hs = h->Hs; a.Ud = h->Ud; a.ab = h->rP.attn_b; a.w = h->rP.attn_w_weight;
    a.dHs = dhid_out; a.dUd = h->dUd; a.dwacc = h->dwacc_r; a.slab = h->slab;
    a.ld_dwhr = h->ldRA4; a.dUd_lp = h->dUd_lp; a.ld_dUd = h->ldRA;
    a.dd = mkdrop(h, RN_SITE_REC_INPUT, h->c.reconstructor_decoder_dropout, train);
    const int Asz = RA <= 256 ? 256 : RA;
    const size_t sm = (size_t)(H + 2 * T + 2 * Asz + 16) * 4;
    // per step: LSTM backward -> GEMM dGr_s . [W_ih | W_hh] -> attention backward -> GEMM dWhr_s . W_r
    // (measured and rejected, round 3, C5: the dx and dhr columns of the product on two streams, 4.31 against 4.21 ms)
    a.slab_w = 0;
    int S1 = 0, S2 = 0;
    for (int s = F - 1; s >= 0; --s) {
      lstm_bwd(h, R, S1, H + R, H, h->dHr + (size_t)s * B * R, R, 1.0f, h->acts_r + (size_t)s * B * 4 * R, h->Cr + (size_t)s * B * R,
               s > 0 ? (h->rgru ? h->Hr : h->Cr) + (size_t)(s - 1) * B * R : nullptr, h->dcr_carry, s == F - 1, at_off(h, h->dGr, (size_t)s * B * ld4R), ld4R, st,
               h->slab2, S2);
      S1 = gemm_slabs(h, RN_TAG_REC_BWD, at_off(h, h->dGr, (size_t)s * B * ld4R), ld4R, h->Wihh_w, 1, ldHR, B, H + R, 4 * R, st);
      a.s = s; a.S = S1; a.slab = h->slab; a.first = (s == F - 1); a.last = (s == 0);
      a.Whr = h->Whr + (size_t)s * B * RA; a.beta = h->beta + (size_t)s * B * T;
      a.dWhr = at_off(h, h->dWhr, (size_t)s * B * h->ldRA4);
      LAUNCH_AT(h, loc_attn_bwd_kernel, dim3(B, RN_TCH), dim3(256), sm, st, a);
      if (s > 0)   // d hr_{s-1} (attention path) = (dWhr_s chunk partials) . [W_r ; .. ; W_r]
        S2 = gemm_slabs(h, RN_TAG_REC_ATT_BWD, at_off(h, h->dWhr, (size_t)s * B * h->ldRA4), h->ldRA4, h->Wr4_w, 1, h->ldR, B, R, RN_TCH * RA, st, h->slab2);
    }
  }
  if (fork_deferred) { const int rr = rec_deferred_fork(h, st, opt_flags); if (rr) return rr; }
  gemm(h, h->dUd_lp, 0, h->ldRA, h->Ur_w, 1, h->ldH, dhid_out, H, nullptr, TB, H, RA, 1.f, 1, st);
  return RECNET_OK;
}
// part 0: everything; 1: only the product that reads the DECODER's hidden states (they are overwritten by the next step's
// decoder chain, so a deferred update runs it in its own step); 2: everything else
// which (mode 2 of the deferred update): bit 0 = the recurrent weights' product d W_hh, bit 1 = everything else
static int bwd_rec_local_deferred(recnet_handle* h, hipStream_t st, int part = 0, int which = 3) {
  const int B = h->B, F = h->F, H = h->H, R = h->R, RA = h->RA, T = h->T_last, TB = T * B, FB = F * B;
  const int ld4R = h->ld4R, ldHR = h->ldHR, GR = (h->rgru ? 3 : 4) * R;
  GemmGroup g = gg_begin(1, 1);      // (bf16 path: every product dY^T . X below in one grouped launch, gemm_lds.hpp)
  const bool rest = (which & 2) != 0, hh = (which & 1) != 0;
  if (part != 2 && rest) gg_add(h, g, h->dUd_lp, h->ldRA, h->Hs_lp, h->ldH, h->rG.attn_U_weight, H, nullptr, RA, H, TB, 1.f, 0, st);
  if (part == 1) { gg_run(h, g, st); return RECNET_OK; }
  if (!rest) {      // d W_hh alone (the pending half of a split update)
    if (F > 1 && hh) {
      const void* dG1 = at_off(h, h->dGr, (size_t)B * ld4R);
      const int nr = (F - 1) * B;
      if (!h->rgru) gg_add(h, g, dG1, ld4R, h->Hr_lp, h->ldR, h->rG.rnn_weight_hh_l0, R, nullptr, 4 * R, R, nr, 1.f, 0, st);
      else {
        gg_add(h, g, dG1, ld4R, h->Hr_lp, h->ldR, h->rG.rnn_weight_hh_l0, R, nullptr, 2 * R, R, nr, 1.f, 0, st);
        gg_add(h, g, at_off(h, (void*)dG1, (size_t)3 * R), ld4R, h->Hr_lp, h->ldR, h->rG.rnn_weight_hh_l0 + (size_t)2 * R * R, R, nullptr, R, R, nr, 1.f, 0, st);
      }
    } else if (hh) hipMemsetAsync(h->rG.rnn_weight_hh_l0, 0, (size_t)GR * R * 4, st);
    gg_run(h, g, st, stamp_site(3));
    return RECNET_OK;
  }
  gg_add(h, g, h->dout_lp, h->ldR, h->Hr_lp, h->ldR, h->rG.out_weight, R, nullptr, R, R, FB, 1.f, 0, st);              // d W_o = dout^T . hr
  colsum_at(h, h->dout_lp, FB, R, h->ldR, h->rG.out_bias, st, h->ss.prezeroed);
  if (!h->lc_bwd_done) {   // (loc_chain_bwd_kernel writes dWhrs itself)
    const size_t n = (size_t)FB * h->ldRA;
    if (h->lp) hipLaunchKernelGGL(sum_chunks_kernel<bf16_t>, dim3(ew_blocks(n)), dim3(256), 0, st, (bf16_t*)h->dWhrs, h->ldRA, (const bf16_t*)h->dWhr, h->ldRA4, FB, RA, RN_TCH);
    else hipLaunchKernelGGL(sum_chunks_kernel<float>, dim3(ew_blocks(n)), dim3(256), 0, st, (float*)h->dWhrs, h->ldRA, (const float*)h->dWhr, h->ldRA4, FB, RA, RN_TCH);
  }
  if (F > 1) {
    const void* dG1 = at_off(h, h->dGr, (size_t)B * ld4R);
    const int nr = (F - 1) * B;
    gg_add(h, g, at_off(h, h->dWhrs, (size_t)B * h->ldRA), h->ldRA, h->Hr_lp, h->ldR, h->rG.attn_W_weight, R, nullptr, RA, R, nr, 1.f, 0, st);
    if (!hh) {
    } else if (!h->rgru) gg_add(h, g, dG1, ld4R, h->Hr_lp, h->ldR, h->rG.rnn_weight_hh_l0, R, nullptr, 4 * R, R, nr, 1.f, 0, st);      // (through the vendor library beside the BPTT, R = 3584: 3.15 -> 3.24 ms)
    else {
      gg_add(h, g, dG1, ld4R, h->Hr_lp, h->ldR, h->rG.rnn_weight_hh_l0, R, nullptr, 2 * R, R, nr, 1.f, 0, st);
      gg_add(h, g, at_off(h, (void*)dG1, (size_t)3 * R), ld4R, h->Hr_lp, h->ldR, h->rG.rnn_weight_hh_l0 + (size_t)2 * R * R, R, nullptr, R, R, nr, 1.f, 0, st);
    }
  } else {
    hipMemsetAsync(h->rG.attn_W_weight, 0, (size_t)RA * R * 4, st);
    if (hh) hipMemsetAsync(h->rG.rnn_weight_hh_l0, 0, (size_t)GR * R * 4, st);
  }
  gg_add(h, g, h->dGr, ld4R, h->Xcat_r, ldHR, h->rG.rnn_weight_ih_l0, H, nullptr, GR, H, FB, 1.f, 0, st);
  // d attn_b = sum_{s,b,t} dz = the column sums of dUd (fp32, [T][B][RA], written whole by every backward form).  The same sum over dWhrs
  // would add bf16-rounded terms of a sum that nearly cancels (the softmax gradient sums to zero over t): the chain and the per-step
  // form round dWhr_s at different points and differed by 2.6e-3 of this gradient (tests/test_gpu_cells.py: test_gru_local_chain_variants)
  colsum_t<float>(h->dUd, TB, RA, RA, h->rG.attn_b, st);
  colsum_t<float>(h->dwacc_r, RN_TCH * B, RA, RA, h->rG.attn_w_weight, st);
  gate_bias_grad(h, h->dGr, FB, R, ld4R, h->rG.rnn_bias_ih_l0, h->rG.rnn_bias_hh_l0, h->rgru, st);
  gg_run(h, g, st, stamp_site(2));      // (behind the column sums: see bwd_rec_global_deferred)
  return RECNET_OK;
}

// rec_loss = mse + lambda_reg * reg from the chain's partial sums (and the norm of the pending-updated W_hh, hoist_side_work: EV_WHH_NORM)
static void rec_loss_scalars(recnet_handle* h, hipStream_t st) {
  if (h->ss.rec_norm_late) { hipStreamWaitEvent(st, h->ev[EV_WHH_NORM], 0); h->ss.rec_norm_late = 0; }
  hipLaunchKernelGGL(rec_loss_finalize_kernel, dim3(1), dim3(256), 0, st, h->msep, h->mse_nb, h->mse_scale, h->scal,
                     h->c.reconstructor_lambda_reg, h->c.lambda_recon);
}
// loss_late: the caller launches rec_loss_scalars itself (fused step: on the side stream behind the BPTT's fork, not between the
// two chains).  norms_hoisted, side: see fwd_rec_global (the local form takes no side work).  outputs_only: the reconstruction
// itself stays in h->outm / h->outl, no loss is formed, and the pass is not one a backward may follow.
static int fwd_rec(recnet_handle* h, const float* enc, int T, int train, hipStream_t st, bool norms_hoisted = false, bool loss_late = false,
                   const SideWork* side = nullptr, bool outputs_only = false) {
  RN_RANGE("recnet: reconstructor forward (train.py:78-131)");
  int r = h->kind == RECNET_REC_GLOBAL ? fwd_rec_global(h, enc, T, train, st, norms_hoisted, side, outputs_only)
                                       : fwd_rec_local(h, enc, T, train, st, norms_hoisted, outputs_only);
  if (r) return r;
  if (outputs_only) { h->T_last = T; h->train_last = train; h->fwd_rec_done = 0; return RECNET_OK; }
  // rec_loss = mse + lambda_reg * reg ; total = dec_loss + lambda_recon * rec_loss
  // (launching it on the fused step's side stream behind the BPTT's fork, like the total-loss scalar, was measured: no change)
  if (!loss_late) rec_loss_scalars(h, st);
  h->T_last = T; h->train_last = train; h->fwd_rec_done = 1;
  return RECNET_OK;
}
// chain part (ends with d loss / d hiddens, which the decoder backward needs) and the deferred weight gradients
static int bwd_rec_chain(recnet_handle* h, float gscale, float* dhid_out, hipStream_t st, bool fork_deferred = false, int opt_flags = -1) {
  RN_RANGE("recnet: reconstructor backward chain");
  return h->kind == RECNET_REC_GLOBAL ? bwd_rec_global(h, gscale, dhid_out, st, fork_deferred, opt_flags)
                                      : bwd_rec_local(h, gscale, dhid_out, st, fork_deferred, opt_flags);
}
static int bwd_rec_deferred(recnet_handle* h, hipStream_t st, int part, int which) {
  RN_RANGE("recnet: reconstructor deferred weight gradients");
  if (h->kind == RECNET_REC_GLOBAL) return part == 1 ? RECNET_OK : bwd_rec_global_deferred(h, st, which);
  return bwd_rec_local_deferred(h, st, part, which);
}
// Deferred reconstructor update (include/recnet_hip.h: recnet_set_deferred_reconstructor_update): the weight-gradient
// products of the step that left an update pending, its Adam step and the re-transposed weight images, on stream s.  The
// Adam kernel reads the device's pending word (RN_CTRL_PENDING) and does nothing when no step left one; the products then ran on
// stale operands into gradient buffers nobody reads.  step_off = -1 when the step counter was already advanced.
static int rec_pending_update(recnet_handle* h, hipStream_t s, int step_off, int flags) {
  const int pz = h->ss.prezeroed; h->ss.prezeroed = 0;          // the column sums' atomic targets: colsum_at zeroes them itself
  const bool split = h->defer_rec == 2;      // only the recurrent weights were left pending (mode 2)
  if (split && rec_pending_hh_fused(h, s, step_off, flags)) {
    // product + Adam update + both operand images of W_hh in one launch (W_o^T was refreshed inside the step that updated W_o)
    h->ss.prezeroed = pz;
    hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, s, h->ctrl + RN_CTRL_PENDING, 0u);
    return RECNET_OK;
  }
  h->def_rows = 1;
  int r = bwd_rec_deferred(h, s, 2, split ? 1 : 3);
  h->def_rows = 0; h->ss.prezeroed = pz;
  // (the derived weight images are refreshed right behind this update, on its stream)
  const int fused = h->ss.in_fused; h->ss.in_fused = 0;
  if (!r) r = optimizer_step(h, flags, s, 1, 1, step_off, split ? ~(1u << RN_REC_T_WHH(h)) : 0u);
  h->ss.in_fused = fused;
  if (r) return r;
  hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, s, h->ctrl + RN_CTRL_PENDING, 0u);
  return RECNET_OK;
}
static int bwd_rec(recnet_handle* h, float gscale, float* dhid_out, hipStream_t st) {
  int r = bwd_rec_chain(h, gscale, dhid_out, st); if (r) return r;
  return bwd_rec_deferred(h, st, 0);
}

static AdamHyper adam_hyper(const recnet_handle* h, int g, int flags) {
  const float lam = g == 0 ? h->c.decoder_lambda_reg : h->c.reconstructor_lambda_reg;
  AdamHyper hp;
  const recnet_handle::OptHyper& oh = h->oh[g];      // (the config's values until recnet_set_optimizer_hyper replaced them)
  hp.lr = oh.lr;
  hp.wd = (float)oh.wd;
  hp.beta1 = oh.beta1; hp.beta2 = oh.beta2; hp.eps = (float)oh.eps;
  hp.one_m_b1 = (float)(1.0 - oh.beta1); hp.beta2f = (float)oh.beta2; hp.one_m_b2 = (float)(1.0 - oh.beta2);
  hp.amsgrad = g == 0 ? h->c.decoder_use_amsgrad : h->c.reconstructor_use_amsgrad;
  hp.reg_coef = (flags & RECNET_OPT_REG) ? lam * (g == 0 ? 1.0f : h->c.lambda_recon) : 0.f;
  return hp;
}
// The split update's pending half (mode 2 of recnet_set_deferred_reconstructor_update), global reconstructor, bf16 path:
// d W_hh = dG^T . h_{t-1} as a grouped launch that applies the recurrent weights' Adam update in its epilogue and rewrites
// both of their operand images (Whh_w and its transpose): no optimiser kernel, no transposes.  false: not applicable here.
// (Measured and rejected, round 4: the last gate block of W_hh updated inside the step — beside the BPTT chain — and only three
// quarters pending.  It balanced the two windows while the epilogue cost 91 us; with the epilogue's loads issued up front (58 us)
// the whole product fits beside the decoder chain and the split only overfilled the BPTT window: C2 1.733 against 1.699 ms.)
// (a property of the handle, not of a launch: a captured step must know what the step BEFORE it left pending)
static bool rec_hh_fused_ok(const recnet_handle* h) {
  const int on = h->sw.adam_epi;
  const OptGroup& o = h->og[1];
  if (!on || !h->lp || h->kind == RECNET_REC_NONE || (h->R & 31) || (h->H & 7) || !o.bound || !o.tab[0].m || !o.tab[0].g) return false;
  const int amsgrad = h->c.reconstructor_use_amsgrad;
  return !(amsgrad && !o.tab[RN_REC_T_WHH(h)].vmax);
}
static bool rec_pending_hh_fused(recnet_handle* h, hipStream_t s, int step_off, int flags) {
  const bool local = h->kind == RECNET_REC_LOCAL;
  // contraction rows: the global form always covers caption_max_len + 1 steps (the step zeroed the gate gradients beyond its T),
  // the local form its F frame steps
  const int R = h->R, B = h->B, ld4R = h->ld4R, T = local ? h->F : h->Tm;
  OptGroup& o = h->og[1];
  if (!rec_hh_fused_ok(h) || T < 2) return false;
  const bool skip = (flags & RECNET_OPT_SKIP_RECONSTRUCTOR) != 0;      // gradient only
  const int ti = RN_REC_T_WHH(h);
  const TensorDesc& td = o.tab[ti];      // rnn.weight_hh_l0
  AdamShared sh;
  sh.hp = adam_hyper(h, 1, flags); sh.step_ptr = (const int32_t*)(h->ctrl + RN_CTRL_STEP); sh.poison = h->scal + RN_SCAL_POISON;
  sh.pending = (const uint32_t*)(h->ctrl + RN_CTRL_PENDING); sh.step_off = step_off; sh.pad = 0; sh.lrs = h->lrs + 1;
#ifdef RN_FAULT_INJECT
  sh.pad = getenv("RN_FAULT") ? atoi(getenv("RN_FAULT")) : 0;      // (fault-injection build only: gemm_lds.hpp)
#endif
  GemmGroup g = gg_begin(1, 1);
  const void* dG1 = at_off(h, h->dGr, (size_t)B * ld4R);
  const int nr = (T - 1) * B;
  auto add = [&](size_t row0, int rows, size_t img_row0, const void* dGcol) {
    gg_add(h, g, dGcol, ld4R, h->Hr_lp, h->ldR, td.g + row0 * R, R, nullptr, rows, R, nr, 1.f, 0, s);
    RnGemmDesc& e = g.d[g.n - 1];
    if (skip) return;
    e.ad_p = td.p + row0 * R; e.ad_m = td.m + row0 * R; e.ad_v = td.v + row0 * R; e.ad_vmax = td.vmax ? td.vmax + row0 * R : nullptr;
    if (!local) {
      e.ad_img = at_off(h, h->Whh_w, img_row0 * h->ldR); e.ad_ld_img = h->ldR;
      e.ad_imgt = h->persist_rec_bwd ? at_off(h, h->WhhT, img_row0) : nullptr; e.ad_ld_imgt = ld4R;
    } else {      // [W_ih | W_hh] image: W_hh behind the H columns of W_ih; its transpose: rows H .. H + R
      e.ad_img = at_off(h, h->Wihh_w, img_row0 * h->ldHR + h->H); e.ad_ld_img = h->ldHR;
      e.ad_imgt = (h->persist_loc_bwd || h->persist_big_bwd) ? at_off(h, h->WihhT, (size_t)h->H * ld4R + img_row0) : nullptr; e.ad_ld_imgt = ld4R;
    }
    e.ad_pnorm = o.d_pnorm + ti;
  };
  if (!h->rgru) add(0, 4 * R, 0, dG1);
  else { add(0, 2 * R, 0, dG1); add((size_t)2 * R, R, (size_t)3 * R, at_off(h, (void*)dG1, (size_t)3 * R)); }      // GRU: (r, z) in place, n -> packed block 3
  if (!gg_run(h, g, s, stamp_site(3), &sh)) return false;
  if (local) { refresh_image(h, WI_WST, s); refresh_image(h, WI_WSTT, s); }      // the streamed-fragment images of the R > 2048 chains follow the two images
  return true;
}
static int optimizer_step(recnet_handle* h, int flags, hipStream_t st, int only_group, int deferred, int step_off, unsigned skip_mask) {
  RN_RANGE("recnet: norms + clip + Adam (train.py:270-273)");
  // decoder: total grad norm (incl. the regulariser gradient), clip coefficient, AMSGrad step
  for (int g = 0; g < 2; ++g) {
    OptGroup& o = h->og[g];
    if (!o.bound) continue;
    if (only_group >= 0 && g != only_group) continue;
    if (g == 0 && (flags & RECNET_OPT_SKIP_DECODER)) continue;
    if (g == 1 && ((flags & RECNET_OPT_SKIP_RECONSTRUCTOR) || h->kind == RECNET_REC_NONE)) continue;
    if (!o.tab[0].m || !o.tab[0].g) return fail(RECNET_ESTATE, "gradients / Adam state not bound");
    AdamHyper hp = adam_hyper(h, g, flags);
    const float coef = hp.reg_coef;
    const float* clip = nullptr;
    if (g == 0 && (flags & RECNET_OPT_CLIP) && h->c.gradient_clip > 0.f) {
      hipLaunchKernelGGL(sumsq_chunk_kernel, dim3(o.nchunks), dim3(256), 0, st, o.d_tab, o.d_chunks, 1, o.d_pnorm, coef, o.d_partial);
      if (o.ntens <= 16) {
        hipLaunchKernelGGL(norm_all_kernel, dim3(1), dim3(256), 0, st, o.d_tab, o.d_partial, o.ntens, o.d_gnorm, h->c.gradient_clip, h->scal + RN_SCAL_GNORM, h->scal + RN_SCAL_CLIP, (float*)nullptr);
      } else {
        hipLaunchKernelGGL(tensor_norm_kernel, dim3(o.ntens), dim3(256), 0, st, o.d_tab, o.d_partial, o.d_gnorm);
        hipLaunchKernelGGL(norm_finalize_kernel, dim3(1), dim3(64), 0, st, o.d_gnorm, o.ntens, h->c.gradient_clip, h->scal + RN_SCAL_GNORM, h->scal + RN_SCAL_CLIP, (float*)nullptr);
      }
      clip = h->scal + RN_SCAL_CLIP;
    }
    // the kernel also writes the packed operand images of the tensors it updates (no separate re-pack pass)
    hipLaunchKernelGGL(adam_chunk_kernel, dim3(o.nchunks), dim3(256), 0, st, o.d_tab, o.d_chunks, hp, o.d_pnorm, clip,
                       (const int32_t*)(h->ctrl + RN_CTRL_STEP), (const PackDesc*)o.d_pack, h->lp, (const float*)(h->scal + RN_SCAL_POISON), h->lrs + g,
                       deferred ? (const uint32_t*)(h->ctrl + RN_CTRL_PENDING) : (const uint32_t*)nullptr, step_off, g == 1 ? skip_mask : 0u);
    if (g == 0) refresh_images(h, 0, st);
    if (g == 1) rec_images_after_update(h, st, (skip_mask >> RN_REC_T_WHH(h)) & 1u);
  }
  return RECNET_OK;
}

