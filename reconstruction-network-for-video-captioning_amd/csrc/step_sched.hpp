// Host-side schedule state of one train step: the stream events by name, and the enqueue-time flags the sequencing functions
// (abi_step.inc, host_decoder.inc, host_reconstructor.inc, host_common.inc) hand to one another.  Included by api.hip.
#pragma once
#include <stdint.h>

// Events of the handle (recnet_handle::ev).  st = the caller's stream, s2 / s3 = the handle's side streams.  A fork is recorded on
// the stream that goes on and the branch waits for it; a join is recorded on the branch.
//   idx name             recorded by; on                                                  waited for by
//   0   EV_SIDE_FORK     side_after_decoder_fwd, or fwd_rec_global in front of its chain; st   s2: vocabulary projection, CE, output-layer gradients
//   1   EV_SIDE_JOIN     fwd_bwd_impl, or early: rec_deferred_fork, dec_bwd_out; s2       st, in front of the decoder's BPTT
//   2   EV_BPTT_FORK     fwd_bwd_impl in front of the BPTT chain; st                      s2: total loss, the reconstructor's deferred gradients
//   3   EV_TAIL_JOIN     fwd_bwd_impl at the step's end; s2                               st
//   4   EV_HOIST_FORK    hoist_side_work, or dec_fwd_chain in front of its chain; st      s2: hoisted work (parameter norms, zeroing, frame mean)
//   5   EV_HOIST_DONE    hoist_side_work; s2                                              st, in front of the reconstructor's forward
//   6   EV_DEC_DW_FORK   fwd_bwd_impl behind the BPTT chain; st                           s2: its half of the decoder's deferred gradients
//   8   EV_XE_FORK       dec_fwd_chain (fp32 path); st                                    s2: embeddings -> Xe beside the feature products
//   9   EV_XE_JOIN       dec_fwd_chain; s2                                                st, in front of the decoder's chain
//   10  EV_REC_DW_FORK   rec_deferred_fork behind the reconstructor's backward chain; st  s2: its deferred gradients (part 1, data parallel)
//   11  EV_S3_FORK       hoist_side_work, or dec_fwd_chain with EV_HOIST_FORK; st         s3: the pending update / deferred image refresh
//   11  EV_S3_JOIN       fwd_bwd_impl, fused_step (s3_late), step_fail_cleanup; s3        st, at the step's end
//   12  EV_PENDING_DONE  hoist_side_work; s3                                              st: fwd_bwd_impl (mode 1), fwd_rec_* (rec_wait_pending)
//   13  EV_OPT_FORK      fwd_bwd_impl behind the deferred gradients; s2                   s3: the reconstructor's Adam step (R >= 2560)
//   14  EV_REC_DW_JOIN   fwd_bwd_impl (part 1), recnet_join_side; s2                      st / the stream handed to recnet_join_side
//   15  EV_TAIL2_FORK    dec_bwd_deferred_grouped; st                                     s2: second branch of the decoder's deferred gradients
//   16  EV_TAIL3_FORK    dec_bwd_deferred_grouped; st                                     s3: third branch
//   17  EV_TAIL3_JOIN    dec_bwd_deferred_grouped; s3                                     st
//   18  EV_SIDE_TAIL     side_after_decoder_fwd (side_tail_open); s2                      st: dec_bwd_deferred_grouped
//   21  EV_WHH_NORM      hoist_side_work (mode 2); s3                                     the stream of rec_loss_scalars (rec_norm_late)
// Free: 7, 19, 20, 22, 23.  Index 11 has two roles, ordered within a step: the fork to s3 belongs to the step's start (behind the
// decoder's prologue), the join from s3 to its end, and s3 itself runs the second's record behind the first's wait.
enum RnEvent {
  EV_SIDE_FORK = 0, EV_SIDE_JOIN = 1, EV_BPTT_FORK = 2, EV_TAIL_JOIN = 3, EV_HOIST_FORK = 4, EV_HOIST_DONE = 5, EV_DEC_DW_FORK = 6,
  EV_XE_FORK = 8, EV_XE_JOIN = 9, EV_REC_DW_FORK = 10, EV_S3_FORK = 11, EV_S3_JOIN = 11, EV_PENDING_DONE = 12, EV_OPT_FORK = 13,
  EV_REC_DW_JOIN = 14, EV_TAIL2_FORK = 15, EV_TAIL3_FORK = 16, EV_TAIL3_JOIN = 17, EV_SIDE_TAIL = 18, EV_WHH_NORM = 21,
  RN_EV_COUNT = 24
};

// The default member initialisers are the state between two steps (sched_reset, api.hip).  What persists across steps by design —
// maybe_pending, images_maybe_stale, defer_rec, defer_flags, split_ok, fwd_*_done, T_last, free_fwd — stays in the handle.  What one
// function hands to the next as an argument or a result is one: the GEMM options and lane (host_common.inc: GemmOpts, gemm_lane), the
// hoisted and side work of the fused step (HoistWork, SideWork), the parameters of dec_fwd_chain / fwd_rec / bwd_rec_chain / dec_bwd_out.
struct StepSched {
  // ---- within one entry-point call: ambient flags, written and consumed while one C-ABI call enqueues.  Each is either set by a callee
  // for a later sibling of its caller, or describes the whole call and is read at several depths below the function that sets it
  int encmean_hoisted = 0;       // the frame mean of the features is formed already.  Set: hoist_side_work, fwd_rec_global.  Read / cleared: fwd_rec_global
  int join_pending = 0;          // the side branch of side_after_decoder_fwd is not joined yet.  Set: side_after_decoder_fwd.  Read / cleared: fwd_bwd_impl; read: rec_deferred_fork, dec_bwd_out
  int join_recorded = 0;         // EV_SIDE_JOIN was recorded early.  Set: rec_deferred_fork, dec_bwd_out.  Read / cleared: fwd_bwd_impl
  int side_tail_open = 0;        // decoder-only: dec_bwd_out recorded the BPTT's join in front of the rest of the side branch (EV_SIDE_TAIL covers the rest).  Set: dec_bwd_out.  Read: side_after_decoder_fwd; cleared: dec_bwd_deferred
  int rec_norm_late = 0;         // mode 2: the norm of the pending-updated W_hh is joined in front of the loss scalars (EV_WHH_NORM), not in front of the chain.  Set: hoist_side_work.  Read / cleared: rec_loss_scalars
  int rec_wait_pending = 0;      // the reconstructor's recurrent chain waits for EV_PENDING_DONE (W_hh's pending update in mode 2, the deferred image refresh).  Set: fwd_bwd_impl.  Read / cleared: fwd_rec_global, fwd_rec_local
  int deferred_done = 0;         // the reconstructor's deferred gradients are enqueued already.  Set: rec_deferred_fork, the deferring branch of fwd_bwd_impl.  Read / cleared: fwd_bwd_impl
  int defer_now = 0;             // this step leaves its reconstructor update pending and completes the one before it on s3.  Set: fwd_bwd_impl.  Read: hoist_side_work; cleared: fwd_bwd
  // Deferred refresh of the reconstructor's DERIVED weight images (opt-in with the deferred-update modes, applies where the split update
  // does not — 28 x 3584, row groups): the fused step skips the transposes / fragment packs behind its reconstructor Adam step (183 us at
  // the end of the step at 28 x 3584) and runs them at the start of the NEXT fused step, on the third stream beside the decoder's forward
  // chain; the reconstructor's chains wait for them (EV_PENDING_DONE).  The refresh is idempotent, so a captured step is correct behind
  // any other; the handle's images_maybe_stale is the host's shadow for the non-fused entry points (flush_pending).
  int img_defer_now = 0;         // Set: fwd_bwd_impl.  Read: hoist_side_work, rec_images_after_update; cleared: fused_step
  int s3_late = 0;               // the third stream's reconstructor update is joined behind the decoder's optimiser step.  Set: fwd_bwd_impl.  Read / cleared: fused_step, step_fail_cleanup
  int in_fused = 0;              // the call is the one-graph fused step (its first kernel writes the step-start stamp).  Set / cleared: fused_step.  Read: wait_chain, fwd_rec_global, fwd_bwd_impl

  // ---- carried between the calls of one step: part 1 to part 2, forward to backward, a chain to its consumer
  int dp_overlap = 0;            // part 1 of the data-parallel step leaves the side stream's weight-gradient products unjoined.  Set: recnet_set_dp_overlap.  Read: fwd_bwd_impl (part 1)
  int side_open = 0;             // ... and it did.  Set: fwd_bwd_impl (part 1).  Read / cleared: recnet_join_side
  int prezeroed = 0;             // the step's atomic-sum targets were zeroed by one hoisted kernel.  Set: hoist_side_work.  Read: the column sums of both backward passes (part 2 included); cleared: fwd_bwd_impl at the step's end, the separate backward entry points
  int xcat_done = 0;             // dec_chain_kernel wrote the global reconstructor's input operand itself.  Set: dec_fwd_chain.  Read / cleared: fwd_rec_global; cleared: recnet_forward_reconstructor
  int mp_done = 0;               // h->mp holds the mean-pooled decoder states of the last decoder forward (dec_chain_kernel).  Set: dec_fwd_chain.  Read: fwd_rec_global; cleared: the entry points that overwrite Hs
  int dhr_done = 0;              // dhrmean was computed by rec_chain_kernel's epilogue.  Set: fwd_rec_global.  Read / cleared: bwd_rec_global
  int dout_ready = 0;            // dout_lp already holds dout_scale * d loss / d out (written by the MSE kernel or the chain's epilogue).  Set: mse_and_dout, fwd_rec_*.  Read / cleared: bwd_rec_global, bwd_rec_local
  int early_opt_done = 0;        // the reconstructor's optimiser step was issued inside fwd_bwd_impl.  Set: fwd_bwd_impl, rec_deferred_fork.  Read: fused_step
  int ctx_done = 0;              // the attended features of all steps were computed early.  Set: side_after_decoder_fwd.  Read: dec_bwd_deferred (part 2); cleared: fwd_bwd_impl
};
