// Host-side helpers shared by the sequences: GEMM wrappers, split-K slabs of the chain sites, column sums, streams,
// weight packing, the decoder's loop invariants and embeddings.
// Part of api.hip (one translation unit; see the include list there).
// A pair of hipEvents for one bracket of the site being profiled (recnet_profile_begin) — around EAGER launches only: on a
// capturing stream no bracket is taken (false).  Until round 4 the bench also captured the records as graph nodes and read them
// after each replay; that form died with a host abort / SIGSEGV inside the HIP runtime in about 1 of 100 bench runs (always in
// the second capture over the same events; tools/crash_hunt.sh found it), and fresh events per capture cannot be read at all
// (hipEventElapsedTime: invalid resource handle for events only ever recorded by graph nodes).
static bool prof_take(recnet_handle* h, hipStream_t st, hipEvent_t* e0, hipEvent_t* e1) {
  *e0 = *e1 = nullptr;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return false;
  if (h->prof_used + 2 > h->prof_ev.size()) {
    hipEvent_t a = nullptr, b = nullptr; hipEventCreate(&a); hipEventCreate(&b);
    h->prof_ev.push_back(a); h->prof_ev.push_back(b);
  }
  *e0 = h->prof_ev[h->prof_used++]; *e1 = h->prof_ev[h->prof_used++];
  return true;
}
// ================================================================================================
// internal helpers
// ================================================================================================
#define REQUIRE_WS(h) do { if (!(h) || !(h)->ws) return fail(RECNET_ESTATE, "workspace not bound"); } while (0)
// kernels that read / write operand copies are templated on the operand type AT (bf16 | float)
#define LAUNCH_AT(h, kern, grid, block, smem, st, ...)                                          \
  do { if ((h)->lp) hipLaunchKernelGGL((kern<bf16_t>), grid, block, smem, st, __VA_ARGS__);     \
       else hipLaunchKernelGGL((kern<float>), grid, block, smem, st, __VA_ARGS__); } while (0)

static int check_T(const recnet_handle* h, int T) { return (T >= 1 && T <= h->Tm) ? 0 : 1; }
inline void* at_off(const recnet_handle* h, void* p, size_t elems) {
  return (char*)p + elems * (h->lp ? 2 : 4);
}

// roctx ranges around the launch sites of the step (SURVEY.md section 5: tracing), so that a rocprofv3 --marker-trace
// timeline of an EAGER step is self-describing (a replayed hipGraph runs no host code: no ranges there).  The marker
// library (librocprofiler-sdk-roctx.so, else libroctx64.so) is looked up at run time when RN_ROCTX=1 — no link-time
// dependency, and nothing at all happens without the variable.
#include <dlfcn.h>
struct RnRange {
  typedef int (*push_t)(const char*);
  typedef int (*pop_t)();
  static push_t& push_fn() { static push_t f = nullptr; return f; }
  static pop_t& pop_fn() { static pop_t f = nullptr; return f; }
  static bool enabled() {
    static const int on = [] {
      const char* e = getenv("RN_ROCTX");
      if (!e || !atoi(e)) return 0;
      void* lib = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
      if (!lib) lib = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
      if (!lib) return 0;
      push_fn() = (push_t)dlsym(lib, "roctxRangePushA");
      pop_fn() = (pop_t)dlsym(lib, "roctxRangePop");
      return (push_fn() && pop_fn()) ? 1 : 0;
    }();
    return on != 0;
  }
  bool live;
  explicit RnRange(const char* name) : live(enabled()) { if (live) push_fn()(name); }
  ~RnRange() { if (live) pop_fn()(); }
};
#define RN_RANGE(name) RnRange rn_range_(name)

// ---- grouped launches (gemm_lds.hpp: gemm_group_kernel): the batched products of one phase that share an operand layout go out
// as ONE grid — their tiles share one hardware work queue, and a product split along K is summed inside the launch by its
// last-arriving slice (no reduction launch).  bf16 path only; the exact-fp32 path runs the members one by one.
struct GemmGroup { int a_col, b_col, n; RnGemmDesc d[GG_MAX]; };
static GemmGroup gg_begin(int a_col, int b_col) { GemmGroup g; g.a_col = a_col; g.b_col = b_col; g.n = 0; return g; }
// What a product's launch needs beyond its operands.  slots: workgroup slots it can expect (0: the whole chip) — for a launch beside
// a chain kernel or beside another grouped launch (launch.hpp: rn_launch_gemm_group).  sum_in_launch: gemm() runs its product as a
// group of one, whose K slices are summed inside the launch.  site (1..8, 0 = none): gg_run's launch stamps its start / end into
// this slot of the handle's group stamps.
struct GemmOpts { int slots = 0, sum_in_launch = 0, site = 0; };
static GemmOpts stamp_site(int site) { GemmOpts o; o.site = site; return o; }
static void gemm(recnet_handle* h, const void* A, int a_col, int lda, const void* Bm, int b_col, int ldb, float* C, int ldc,
                 const float* bias, int M, int N, int K, float alpha, int acc, hipStream_t st, GemmOpts o = GemmOpts());
static void gemm_to_at(recnet_handle* h, const void* A, int a_col, int lda, const void* Bm, int b_col, int ldb, void* C,
                       int ldc, int M, int N, int K, hipStream_t st);
// The split-K slabs and the tile counters (one block of RN_GCNT_WORDS per slab workspace) a product uses follow from the stream it is
// enqueued on: the handle's side streams have their own, so that launches on different streams never share.  (Only a side stream
// that exists is compared: a null s2 / s3 is not the caller's null stream.)
struct GemmLane { float* ws; unsigned* cnt; };
static GemmLane gemm_lane(const recnet_handle* h, hipStream_t st) {
  if (h->s3 && st == h->s3) return {h->gws3, h->gcnt + 2 * RN_GCNT_WORDS};
  if (h->s2 && st == h->s2) return {h->gws2, h->gcnt + RN_GCNT_WORDS};
  return {h->gws, h->gcnt};
}
// adam != null: members with ad_p set apply their Adam update in the epilogue (returns false if the launch did not qualify —
// nothing was enqueued then, and the caller runs the plain products and the optimiser kernel instead)
static bool gg_run(recnet_handle* h, GemmGroup& g, hipStream_t st, GemmOpts o = GemmOpts(), const AdamShared* adam = nullptr) {
  if (g.n == 0) return true;
  unsigned long long* stamp = o.site > 0 ? reinterpret_cast<unsigned long long*>(h->gbar + CS_WS_GROUP_STAMPS) + 2 * (o.site - 1) : nullptr;
  const GemmLane ln = gemm_lane(h, st);
  if (h->lp && h->sw.gemm_group && !rn_launch_gemm_group(g.a_col, g.b_col, g.d, g.n, ln.ws, h->gws_floats, ln.cnt, RN_GCNT_WORDS, st, o.slots, adam, stamp)) { g.n = 0; return true; }
  if (adam) { g.n = 0; return false; }
  for (int i = 0; i < g.n; ++i) {
    const RnGemmDesc& e = g.d[i];
    if (e.c_bf16) gemm_to_at(h, e.A, g.a_col, e.lda, e.B, g.b_col, e.ldb, e.C, e.ldc, e.M, e.N, e.K, st);
    else gemm(h, e.A, g.a_col, e.lda, e.B, g.b_col, e.ldb, e.C, e.ldc, e.bias, e.M, e.N, e.K, e.alpha, e.accumulate, st);
  }
  g.n = 0;
  return true;
}
static void gg_add(recnet_handle* h, GemmGroup& g, const void* A, int lda, const void* Bm, int ldb, float* C, int ldc, const float* bias,
                   int M, int N, int K, float alpha, int acc, hipStream_t st, int c_bf16 = 0) {
  if (M <= 0 || N <= 0 || K <= 0) return;
  if (g.n == GG_MAX) gg_run(h, g, st);
  RnGemmDesc& e = g.d[g.n++];
  e.A = A; e.lda = lda; e.B = Bm; e.ldb = ldb; e.C = C; e.ldc = ldc; e.bias = bias; e.M = M; e.N = N; e.K = K; e.alpha = alpha;
  e.accumulate = acc; e.c_bf16 = c_bf16; e.c2 = nullptr; e.ldc2 = 0; e.ad_p = nullptr;
}
// batched GEMM on operand buffers (AT) with automatic split-K; fp32 output
static void gemm(recnet_handle* h, const void* A, int a_col, int lda, const void* Bm, int b_col, int ldb, float* C, int ldc,
                 const float* bias, int M, int N, int K, float alpha, int acc, hipStream_t st, GemmOpts o) {
  const GemmLane ln = gemm_lane(h, st);
  if (h->lp && o.sum_in_launch) {      // a group of one: same kernel, split products summed inside the launch
    RnGemmDesc e;
    e.A = A; e.lda = lda; e.B = Bm; e.ldb = ldb; e.C = C; e.ldc = ldc; e.bias = bias; e.M = M; e.N = N; e.K = K; e.alpha = alpha;
    e.accumulate = acc; e.c_bf16 = 0; e.c2 = nullptr; e.ldc2 = 0; e.ad_p = nullptr;
    if (h->sw.gemm_group && !rn_launch_gemm_group(a_col, b_col, &e, 1, ln.ws, h->gws_floats, ln.cnt, RN_GCNT_WORDS, st, o.slots)) return;
  }
  int s = rn_pick_splitk(h->prec, M, N, K, 16, 0);
  while (s > 1 && (size_t)s * M * N > h->gws_floats) s >>= 1;
  rn_launch_gemm(h->prec, A, h->lp, a_col, lda, Bm, h->lp, b_col, ldb, C, ldc, bias, M, N, K, alpha, acc, s, ln.ws, 1, st);
}
// same, output written as an operand buffer (AT) — direct epilogue only
static void gemm_to_at(recnet_handle* h, const void* A, int a_col, int lda, const void* Bm, int b_col, int ldb, void* C,
                       int ldc, int M, int N, int K, hipStream_t st) {
  rn_launch_gemm(h->prec, A, h->lp, a_col, lda, Bm, h->lp, b_col, ldb, (float*)C, ldc, nullptr, M, N, K, 1.f, 0, 1, nullptr, 0,
                 st, 0, h->lp);
}
// recurrent-step GEMM: partial slabs only; returns the slab count the consumer must sum
static int gemm_slabs(recnet_handle* h, int tag, const void* A, int lda, const void* Bm, int b_col, int ldb, int M, int N,
                      int K, hipStream_t st, float* dst = nullptr) {
  float* slab = dst ? dst : h->slab;
  // split-K caps per site: more slices than this buy nothing for the GEMM (measured) and every slab is re-read by
  // the consumer kernel
  int cap = (tag == RN_TAG_DEC_FWD) ? 4 : ((tag == RN_TAG_DEC_BWD && b_col) ? 8 : 16);
  if (dst) cap = 8;
  int s = rn_pick_splitk(h->prec, M, N, K, cap, 1);
  while (s > 1 && (size_t)s * M * N > h->slab_floats) s >>= 1;
  if (s < 2) s = 2;  // always use the slab path so the consumer code is uniform
  s = rn_effective_splitk(h->prec, K, s);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (h->prof_on == tag) {
    if (prof_take(h, st, &e0, &e1)) hipEventRecord(e0, st);
  }
  if (s < 2) {   // K fits one tile: the single product goes to slab 0 through the direct epilogue
    rn_launch_gemm(h->prec, A, h->lp, 0, lda, Bm, h->lp, b_col, ldb, slab, N, nullptr, M, N, K, 1.f, 0, 1, nullptr, 0, st, tag);
    s = 1;
  } else {
    rn_launch_gemm(h->prec, A, h->lp, 0, lda, Bm, h->lp, b_col, ldb, nullptr, N, nullptr, M, N, K, 1.f, 0, s, slab, 0, st, tag);
  }
  if (e1) hipEventRecord(e1, st);
  return s;
}
template <typename ST>
static void colsum_t(const ST* X, int rows, int cols, int ld, float* out, hipStream_t st, int zeroed = 0) {
  if (rows >= 64 && (ld & 7) == 0 && (((uintptr_t)X) & 15) == 0) {
    int rs = rows / 96; rs = rs < 1 ? 1 : (rs > 64 ? 64 : rs);
    if (!zeroed) hipMemsetAsync(out, 0, (size_t)cols * 4, st);
    hipLaunchKernelGGL(colsum_vec_kernel<ST>, dim3(cdiv(cols, 512), rs), dim3(256), 0, st, X, rows, cols, ld, out);
    return;
  }
  int rs = rows >= 512 ? 8 : 1;
  if (rs > 1 && !zeroed) hipMemsetAsync(out, 0, (size_t)cols * 4, st);
  hipLaunchKernelGGL(colsum_kernel<ST>, dim3(cdiv(cols, 64), rs), dim3(256), 0, st, X, rows, cols, ld, out, rs > 1 ? 1 : 0);
}
// zeroed: `out` is one of the buffers the hoisted zero_list_kernel of this step cleared
static void colsum_at(recnet_handle* h, const void* X, int rows, int cols, int ld, float* out, hipStream_t st, int zeroed = 0) {
  if (h->lp) colsum_t<bf16_t>((const bf16_t*)X, rows, cols, ld, out, st, zeroed);
  else colsum_t<float>((const float*)X, rows, cols, ld, out, st, zeroed);
}
// fork: `side` continues after everything enqueued on `main` so far; join: `main` waits for `side`.  Under
// stream capture these become graph edges, so independent work runs in parallel branches of the hipGraph.
static void gate_bias_grad(recnet_handle* h, const void* dG, int rows, int Hd, int ld, float* dbih, float* dbhh, int gru, hipStream_t st) {
  float* tmp = (dbih == h->dGd.rnn_bias_ih_l0) ? h->bsum4 : h->bsum4r;      // decoder / reconstructor
  colsum_at(h, dG, rows, 4 * Hd, ld, tmp, st, h->ss.prezeroed);
  hipLaunchKernelGGL(gate_bias_grad_kernel, dim3(cdiv(4 * Hd, 256)), dim3(256), 0, st, tmp, dbih, dbhh, Hd, gru);
}
// dW_hh = dG^T . Hprev over `rows` rows.  LSTM: the 4 gate blocks as they are.  GRU: master blocks (r, z) come from
// packed blocks (0, 1) and master block n from packed block 3 (the hidden-side n pre-activation, see gru_point).
static void dW_hh(recnet_handle* h, int gru, int Hd, const void* dG, int ld_dg, const void* Hprev, int ld_h, float* dW, int rows,
                  int acc, hipStream_t st) {
  if (!gru) { gemm(h, dG, 1, ld_dg, Hprev, 1, ld_h, dW, Hd, nullptr, 4 * Hd, Hd, rows, 1.f, acc, st); return; }
  gemm(h, dG, 1, ld_dg, Hprev, 1, ld_h, dW, Hd, nullptr, 2 * Hd, Hd, rows, 1.f, acc, st);
  gemm(h, at_off(h, (void*)dG, (size_t)3 * Hd), 1, ld_dg, Hprev, 1, ld_h, dW + (size_t)2 * Hd * Hd, Hd, nullptr, Hd, Hd, rows, 1.f, acc, st);
}
static void fork_to(recnet_handle* h, RnEvent e, hipStream_t main, hipStream_t side) {
  hipEventRecord(h->ev[e], main); hipStreamWaitEvent(side, h->ev[e], 0);
}
static void join_from(recnet_handle* h, RnEvent e, hipStream_t main, hipStream_t side) {
  hipEventRecord(h->ev[e], side); hipStreamWaitEvent(main, h->ev[e], 0);
}
static void copyf(const float* x, float* y, size_t n, hipStream_t st) {
  hipMemcpyAsync(y, x, n * 4, hipMemcpyDeviceToDevice, st);
}
// dst (AT) [rows][ld_dst] <- scale * src fp32 [rows][.. ld_src], zero padded
static void pack_block(recnet_handle* h, void* dst, int ld_dst, const float* src, int ld_src, int rows, int cols, float scale,
                       hipStream_t st) {
  const size_t n = (size_t)rows * ld_dst;
  if (h->lp) hipLaunchKernelGGL(pack_block_kernel<bf16_t>, dim3(ew_blocks(n)), dim3(256), 0, st, (bf16_t*)dst, ld_dst, src, ld_src, rows, cols, scale);
  else hipLaunchKernelGGL(pack_block_kernel<float>, dim3(ew_blocks(n)), dim3(256), 0, st, (float*)dst, ld_dst, src, ld_src, rows, cols, scale);
}
static void param_norms(recnet_handle* h, int g, float* sum_out, hipStream_t st) {
  OptGroup& o = h->og[g];
  hipLaunchKernelGGL(sumsq_chunk_kernel, dim3(o.nchunks), dim3(256), 0, st, o.d_tab, o.d_chunks, 0, (const float*)nullptr, 0.f, o.d_partial);
  if (o.ntens <= 16) {
    hipLaunchKernelGGL(norm_all_kernel, dim3(1), dim3(256), 0, st, o.d_tab, o.d_partial, o.ntens, o.d_pnorm, 0.f, (float*)nullptr, (float*)nullptr, sum_out);
    return;
  }
  hipLaunchKernelGGL(tensor_norm_kernel, dim3(o.ntens), dim3(256), 0, st, o.d_tab, o.d_partial, o.d_pnorm);
  hipLaunchKernelGGL(norm_finalize_kernel, dim3(1), dim3(64), 0, st, o.d_pnorm, o.ntens, 0.f, (float*)nullptr, (float*)nullptr, sum_out);
}
__global__ void fill_i64_kernel(int64_t* p, int64_t v, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
// out = a + k * b
__global__ void axpb_kernel(const float* a, const float* b, float k, float* out) { *out = *a + k * *b; }
__global__ void export_scalars_kernel(const float* scal, recnet_scalars* out) {
  out->dec_ce = scal[RN_SCAL_DEC_CE]; out->dec_reg = scal[RN_SCAL_DEC_REG]; out->dec_loss = scal[RN_SCAL_DEC_LOSS]; out->rec_mse = scal[RN_SCAL_REC_MSE];
  out->rec_reg = scal[RN_SCAL_REC_REG]; out->rec_loss = scal[RN_SCAL_REC_LOSS]; out->total_loss = scal[RN_SCAL_TOTAL] + scal[RN_SCAL_POISON]; out->dec_grad_norm = scal[RN_SCAL_GNORM];   // the poison word: 0, or NaN after a chain kernel gave up waiting (chain_sync.hpp)
  const unsigned long long now = (unsigned long long)wall_clock64();
  reinterpret_cast<unsigned long long*>(const_cast<float*>(scal) + RN_SCAL_STAMP_END)[0] = now;      // phase stamp: step end (recnet_read_stamps)
  rn_ring_push(reinterpret_cast<unsigned long long*>(const_cast<float*>(scal) + RN_SCAL_RING), now);
}

static void gate_bias(const float* bih, const float* bhh, float* out, int Hd, int gru, hipStream_t st) {
  hipLaunchKernelGGL(gate_bias_kernel, dim3(cdiv(4 * Hd, 256)), dim3(256), 0, st, bih, bhh, out, Hd, gru);
}
// both bias gradients from the 4-block gate gradients dG [rows][4 Hd]
static void gate_bias_grad(recnet_handle* h, const void* dG, int rows, int Hd, int ld, float* dbih, float* dbhh, int gru, hipStream_t st);

// hipEvent bracket around one launch of a profile site (recnet_profile_begin): returns the end event to record, or null
static hipEvent_t prof_bracket_begin(recnet_handle* h, int site, hipStream_t st) {
  if (h->prof_on != site) return nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (prof_take(h, st, &e0, &e1)) hipEventRecord(e0, st);
  return e1;
}
// see wait_chain_kernel (rec_chain.hpp); k = the chain's CsChain (chain_sync.hpp): 0 decoder forward chain, 1 decoder BPTT, 2 / 3 global fwd / bwd, 4 / 5 local fwd / bwd
static void wait_chain(recnet_handle* h, int k, hipStream_t st) {
  const int on = h->sw.wait_chain;
  if (!on || !h->ss.in_fused) return;      // (the step-start stamp is written by the fused step's first kernel)
  const unsigned long long* stamps = reinterpret_cast<const unsigned long long*>(h->gbar + CS_WS_STAMPS);
  hipLaunchKernelGGL(wait_chain_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<const unsigned long long*>(h->ctrl + RN_CTRL_STAMP_START), stamps + 2 * k, 30000u);
}
// The two pieces of the fused step that a sequence may enqueue on fwd_bwd_impl's behalf, where the captured order wants them
// (abi_step.inc).  The callee that is handed one enqueues it and returns its error behind its own; null: nothing to enqueue.
struct HoistWork { int par; const float* enc; };      // hoist_side_work: on the side stream?; the features (frame mean)
struct SideWork { const int64_t* targets; const float* stepw; const float* enc; int T, phase; };      // side_after_decoder_fwd
static int hoist_side_work(recnet_handle* h, const HoistWork& w, hipStream_t st, bool fork_recorded);
static int side_after_decoder_fwd(recnet_handle* h, const SideWork& w, hipStream_t st, bool fork_recorded);
// ---- the images DERIVED from the packed weights (weight_images.hpp): shapes, sources and existence come from the handle's table.
// A transposed image = (its source image)^T, K contiguous (source rows beyond its extent read as zero -> the padding of the
// transposed rows); src_cols > 0: only the first src_cols columns of the source.  A fragment image: one 16-byte fragment per thread.
static void refresh_image(recnet_handle* h, int id, hipStream_t st, int src_cols = 0) {
  const WImage& d = h->wimg[id];
  if (!d.live || !(h->*d.field)) return;
  const WImage& s = h->wimg[d.from];
  const bf16_t* src = (const bf16_t*)(h->*s.field);
  bf16_t* dst = (bf16_t*)(h->*d.field);
  const int cols = src_cols ? src_cols : s.cols;
  const dim3 grid((unsigned)cdiv((long)d.rows, 256));
  if (d.how == WI_TRANSPOSE)
    hipLaunchKernelGGL(transpose_at_kernel<bf16_t>, dim3(cdiv(cols, 32), cdiv(d.ld, 32)), dim3(256), 0, st, src, s.ld, (int)s.rows, cols, dst, d.ld);
  else if (d.how == WI_STREAM_FWD)
    hipLaunchKernelGGL(lc_pack_stream_kernel, grid, dim3(256), 0, st, src, s.ld, h->R, h->H, h->lc_steps, h->lc_sr, dst, d.rows);
  else if (d.how == WI_STREAM_BWD)
    hipLaunchKernelGGL(lcbig_pack_stream_kernel, grid, dim3(256), 0, st, src, s.ld, h->R, h->lb_ncb, h->lb_steps, h->lb_sr, dst, d.rows);
}
// every derived image of one optimiser group's weights (table order: a source comes before what derives from it)
static void refresh_images(recnet_handle* h, int group, hipStream_t st) {
  for (int id = 0; id < WI_COUNT; ++id)
    if (h->wimg[id].how != WI_DIRECT && h->wimg[id].group == group) refresh_image(h, id, st);
}
// ... after the reconstructor's Adam step (a lazy refresh under the next step's decoder chain existed in rounds 3-4; the split
// update's epilogue, which writes both images itself, replaced it)
// whh_skipped: this Adam step left the recurrent weights alone (the in-step half of a split update): their transposed image is
// rewritten by the epilogue that updates them (gemm_lds.hpp), so only what follows the OTHER tensors is refreshed here — W_o^T
// (global), the W_ih rows of [W_ih | W_hh]^T (local).  (Round 4 transposed all of W_hh^T here as well, 30 us of the BPTT window
// at C2 for an image the next step's pending update overwrites, and W_o^T twice.)
static void rec_images_after_update(recnet_handle* h, hipStream_t st, bool whh_skipped = false) {
  if (h->ss.img_defer_now) { h->images_maybe_stale = 1; return; }      // the next fused step refreshes them beside its decoder chain (api.hip)
  if (!whh_skipped || h->persist_big_bwd) { refresh_images(h, 1, st); return; }
  if (h->kind == RECNET_REC_GLOBAL) { refresh_image(h, WI_WOT, st); return; }
  if (h->kind == RECNET_REC_LOCAL && h->persist_loc_bwd) refresh_image(h, WI_WIHHT, st, h->wimg[WI_WIHH_W].src[0].nc);      // the W_ih window of [W_ih | W_hh]
}

// Packed operand images of the weights (AT, zero padded leading dimensions) from the master parameters: one launch per bound
// group through the pack descriptors the Adam kernel also stores by, then the derived images.  Padding and a GRU's empty gate block
// stay zero from the workspace's memset: every writer (this kernel, Adam, the split update's GEMM epilogue) stays inside the windows.
static int pack_weights(recnet_handle* h, hipStream_t st) {
  for (int g = 0; g < 2; ++g) {
    const OptGroup& o = h->og[g];
    if (!o.bound) continue;
    hipLaunchKernelGGL(pack_chunk_kernel, dim3(o.nchunks), dim3(256), 0, st, (const TensorDesc*)o.d_tab, (const int2*)o.d_chunks, (const PackDesc*)o.d_pack, h->lp);
    refresh_images(h, g, st);
  }
  return RECNET_OK;
}

// rows: the captions of the batch, or [beam][caption] rows over args.nc captions (DecCellArgs).  The row count is taken from here
// alone: the kernels' B (the slab stride) is set to it, whatever the caller left in args.B.
static void launch_dec_cell(recnet_handle* h, const DecCellArgs& args, int rows, hipStream_t st) {
  DecCellArgs a = args;
  a.B = rows;
  // (A % 4: the kernel's LDS rows behind swh[A] are written with 16-byte stores, so A floats must keep them 16-byte aligned; the
  // persistent chain of host_decoder.inc asks for (4H + A) % 16 == 0 with H % 8 == 0, which implies A % 16 == 0)
  if (h->lp && (h->H & 7) == 0 && h->F <= 32 && h->A <= 128 && (h->A & 3) == 0 && (h->ld4H & 7) == 0) {
    const size_t smv = (size_t)(h->A + ((h->F + 3) & ~3) + 4 * 512 + 16) * 4;
    hipLaunchKernelGGL(dec_cell_vec_kernel<bf16_t>, dim3(rows, cdiv(h->H, 512)), dim3(256), smv, st, a);
    return;
  }
  // units per workgroup: 256 (1024 threads) when H allows, so a caption is covered by H/256 workgroups
  int uc = h->H >= 256 ? 256 : (h->H >= 128 ? 128 : 64);
  dim3 grid(rows, cdiv(h->H, uc));
  const size_t sm = (size_t)(h->A + h->F + 4 * uc + 16) * 4;
  LAUNCH_AT(h, dec_cell_kernel, grid, dim3(4 * uc), sm, st, a);
}
// loop-invariant products of the decoder: Uv = enc . U^T (decoder.py:54) and P = enc . W_ih[:, E:]^T
static void dec_invariants(recnet_handle* h, const float* enc, hipStream_t st, bool with_bias = true) {
  RN_RANGE("recnet: decoder prologue (enc -> bf16, Uv, P)");
  const int B = h->B, F = h->F, D = h->D, H = h->H, A = h->A;
  if (with_bias) gate_bias(h->dP.rnn_bias_ih_l0, h->dP.rnn_bias_hh_l0, h->bsum_d, H, h->dgru, st);
  pack_block(h, h->enc_lp, h->ldD, enc, D, B * F, D, 1.f, st);
  gemm(h, h->enc_lp, 0, h->ldD, h->U_w, 0, h->ldD, h->Uv, A, nullptr, B * F, A, D, 1.f, 0, st);
  gemm_to_at(h, h->enc_lp, 0, h->ldD, h->Wc_w, 0, h->ldD, h->P, h->ld4H, B * F, 4 * H, D, st);
}
// `rows` embedding rows into dst (operand type, row stride ldE); B: the kernel's rows per step (row = (t - t0) * B + b)
static void embed_fwd(recnet_handle* h, const int64_t* targets, const int64_t* tokens, void* dst, int rows, int B, int train, int t0,
                      hipStream_t st) {
  const DropDesc dd = mkdrop(h, RN_SITE_DEC_EMBED, h->c.embedding_dropout, train);
  if (h->lp) hipLaunchKernelGGL(embed_fwd_kernel<bf16_t>, dim3(rows), dim3(128), 0, st, h->dP.embedding_weight, targets, tokens, (bf16_t*)dst, h->ldE, B, h->E, h->V, h->c.embedding_scale, dd, t0);
  else hipLaunchKernelGGL(embed_fwd_kernel<float>, dim3(rows), dim3(128), 0, st, h->dP.embedding_weight, targets, tokens, (float*)dst, h->ldE, B, h->E, h->V, h->c.embedding_scale, dd, t0);
}

