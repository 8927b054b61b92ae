// C ABI: launch-site profiling hooks and the bare GEMM entry points.
// Part of api.hip (one translation unit; see the include list there).
int recnet_profile_begin(recnet_handle* h, int32_t site) {
  if (!h || site < 1 || site > 11) return fail(RECNET_EINVAL, "bad profile site");
  h->prof_on = site; h->prof_used = 0;
  return RECNET_OK;
}

int recnet_profile_null_launch(recnet_handle* h, int32_t count, void* stream) {
  if (!h || !h->ws) return fail(RECNET_ESTATE, "workspace not bound");
  if (!h->prof_on) return fail(RECNET_ESTATE, "not profiling");
  hipStream_t st = (hipStream_t)stream;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!prof_take(h, st, &e0, &e1)) return fail(RECNET_ESTATE, "profile brackets are taken around eager launches only (the stream is capturing)");
  HIPCHK(hipEventRecord(e0, st));
  for (int i = 0; i < count; ++i) hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, st, h->ctrl + RN_CTRL_SINK_LAUNCH, 0u);
  HIPCHK(hipEventRecord(e1, st));
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_profile_read(recnet_handle* h, int32_t* n_launches, double* total_ms) {
  if (!h || !n_launches || !total_ms) return fail(RECNET_EINVAL, "null argument");
  double tot = 0; int n = 0;
  for (size_t i = 0; i + 1 < h->prof_used; i += 2) {
    HIPCHK(hipEventSynchronize(h->prof_ev[i + 1]));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->prof_ev[i], h->prof_ev[i + 1]));
    tot += ms; ++n;
  }
  *n_launches = n; *total_ms = tot;
  return RECNET_OK;
}

int recnet_profile_end(recnet_handle* h, int32_t* n_launches, double* total_ms) {
  if (!h || !n_launches || !total_ms) return fail(RECNET_EINVAL, "null argument");
  h->prof_on = 0;
  double tot = 0; int n = 0;
  for (size_t i = 0; i + 1 < h->prof_used; i += 2) {
    HIPCHK(hipEventSynchronize(h->prof_ev[i + 1]));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->prof_ev[i], h->prof_ev[i + 1]));
    tot += ms; ++n;
  }
  *n_launches = n; *total_ms = tot;
  h->prof_used = 0;
  return RECNET_OK;
}

// Probe builds (make probe -> librecnet_hip_probe.so): the wall-clock stamps the local chain kernels recorded in
// their last launch, [role][step][8] 100 MHz ticks (roles 0-2 forward U / C / relay, 3-6 backward relay / U' / X' / C').
int recnet_probe_read(recnet_handle* h, uint64_t* out, int32_t n) {
  REQUIRE_WS(h);
#ifndef LC_PROBE
  (void)out; (void)n;
  return fail(RECNET_ESTATE, "not a probe build (make probe)");
#else
  if (!out || n <= 0 || n > 2 * 8 * 64 * 8) return fail(RECNET_EINVAL, "bad probe read");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, h->lc_ts, (size_t)n * 8, hipMemcpyDeviceToHost));
  return RECNET_OK;
#endif
}

// Test hook: fill the LDS of every CU with NaN bit patterns (one pass of 64 KB workgroups, several per CU).  A kernel that
// reads LDS it never wrote usually reads the finite left-overs of whatever ran before; after this it reads NaN, and the
// parity tests that call it (tests/test_gpu_parity.py) fail deterministically instead of once in two hundred launches.
__global__ __launch_bounds__(256) void lds_poison_kernel(unsigned* sink) {
  extern __shared__ unsigned lp_smem[];
  for (int i = threadIdx.x; i < 16384; i += 256) lp_smem[i] = 0x7fc00000u + (unsigned)i;
  __syncthreads();
  if (lp_smem[(threadIdx.x * 37 + blockIdx.x) & 16383] == 0u) *sink = 1u;     // keeps the stores alive
}
int recnet_debug_poison_lds(recnet_handle* h, void* stream) {
  REQUIRE_WS(h);
  hipFuncSetAttribute(reinterpret_cast<const void*>(lds_poison_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
  hipLaunchKernelGGL(lds_poison_kernel, dim3(h->ncu > 0 ? 8 * h->ncu : 2048), dim3(256), 65536, (hipStream_t)stream, h->ctrl + RN_CTRL_SINK_LDS);
  LAUNCH_OK();
  return RECNET_OK;
}

int32_t recnet_dim(const recnet_handle* h, int32_t which) {
  if (!h) return 0;
  const int v[11] = {h->B, h->F, h->D, h->E, h->H, h->A, h->V, h->R, h->RA, h->Tm, h->split_ok};
  return (which >= 0 && which < 11) ? v[which] : 0;
}

// Health of the persistent chain kernels.  Every wait inside them is bounded; a waiter that gives up raises a sticky word
// in its chain's barrier block and the step's total loss becomes NaN (chain_sync.hpp: rc_give_up / cs_finish), and the
// optimiser kernels leave the parameters alone from then on.  recnet_chain_status synchronises the stream and returns a
// bit per chain (1 reconstructor fwd, 2 reconstructor bwd, 4 decoder fwd, 8 decoder BPTT, 32 / 64 local reconstructor
// fwd / bwd, 256 the poisoned-loss word); recnet_chain_reset clears the words and, with disable_persistent != 0, makes
// every later launch sequence of this handle use the per-step kernels (graphs captured earlier must be re-captured).
int recnet_chain_status(recnet_handle* h, int32_t* status_out, void* stream) {
  REQUIRE_WS(h);
  if (!status_out) return fail(RECNET_EINVAL, "null argument");
  uint32_t w[CS_WS_BLOCKS]; float poison = 0.f;
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  for (int k = 0; k < CS_WS_BLOCKS; ++k) HIPCHK(hipMemcpy(&w[k], cs_ws_sticky(h->gbar, k), 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&poison, h->scal + RN_SCAL_POISON, 4, hipMemcpyDeviceToHost));
  int32_t s = 0;
  for (int k = 0; k < CS_WS_BLOCKS; ++k) if (w[k]) s |= 1 << k;
  if (poison != 0.f) s |= 256;      // NaN != 0
  *status_out = s;
  return RECNET_OK;
}
// Phase stamps of the last step (include/recnet_hip.h): 100 MHz wall-clock values written by the kernels themselves.
int recnet_read_stamps(recnet_handle* h, uint64_t* out, int32_t n, void* stream) {
  REQUIRE_WS(h);
  if (!out || n < 14) return fail(RECNET_EINVAL, "recnet_read_stamps needs room for 14 values");
  // (every copy BEHIND the synchronisation: the library's and torch's streams do not block on the null stream, so a blocking copy in
  // front of it could return the stamps of a step that has not finished)
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  if (n >= 30) HIPCHK(hipMemcpy(&out[14], h->gbar + CS_WS_GROUP_STAMPS, 16 * 8, hipMemcpyDeviceToHost));      // grouped launches: 8 x (start, end)
  HIPCHK(hipMemcpy(&out[0], h->ctrl + RN_CTRL_STAMP_START, 8, hipMemcpyDeviceToHost));                       // step start (advance_step_kernel)
  HIPCHK(hipMemcpy(&out[1], h->gbar + CS_WS_STAMPS, 12 * 8, hipMemcpyDeviceToHost));           // six chains x (begin, end): rc_stamp_slot
  HIPCHK(hipMemcpy(&out[13], h->scal + RN_SCAL_STAMP_END, 8, hipMemcpyDeviceToHost));                      // step end (export_scalars_kernel)
  return RECNET_OK;
}
// ---- staging kernels of the direct gradient transport (include/recnet_hip.h; kernels_util.hpp)
int recnet_dp_cast(const void* src, int32_t src_bf16, void* dst, int32_t dst_bf16, int64_t n, void* stream) {
  if (!src || !dst || n < 0) return fail(RECNET_EINVAL, "bad dp_cast argument");
  if (n == 0) return RECNET_OK;
  hipStream_t st = (hipStream_t)stream;
  long blocks = (n / 4 + 255) / 256; blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  if (!src_bf16 && dst_bf16) hipLaunchKernelGGL((dp_cast_kernel<bf16_t, float>), dim3((unsigned)blocks), dim3(256), 0, st, (const float*)src, (bf16_t*)dst, (long)n);
  else if (src_bf16 && !dst_bf16) hipLaunchKernelGGL((dp_cast_kernel<float, bf16_t>), dim3((unsigned)blocks), dim3(256), 0, st, (const bf16_t*)src, (float*)dst, (long)n);
  else if (!src_bf16 && !dst_bf16) hipLaunchKernelGGL((dp_cast_kernel<float, float>), dim3((unsigned)blocks), dim3(256), 0, st, (const float*)src, (float*)dst, (long)n);
  else return fail(RECNET_EINVAL, "dp_cast: bf16 -> bf16 is a plain copy");
  LAUNCH_OK();
  return RECNET_OK;
}
int recnet_dp_reduce(const void* recv, int32_t world, int64_t chunk, void* red, int32_t wire_bf16, void* stream) {
  if (!recv || !red || world < 1 || world > 16 || chunk < 0) return fail(RECNET_EINVAL, "bad dp_reduce argument (world <= 16)");
  if (chunk == 0) return RECNET_OK;
  hipStream_t st = (hipStream_t)stream;
  long blocks = (chunk + 255) / 256; blocks = blocks > 2048 ? 2048 : blocks;
  if (wire_bf16) hipLaunchKernelGGL(dp_reduce_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, st, (const bf16_t*)recv, world, (long)chunk, (bf16_t*)red);
  else hipLaunchKernelGGL(dp_reduce_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)recv, world, (long)chunk, (float*)red);
  LAUNCH_OK();
  return RECNET_OK;
}
// The last seven step-start and step-end stamps (100 MHz wall clock; out[0] / out[8] = how many were ever written): see rn_ring_push
int recnet_read_step_ring(recnet_handle* h, uint64_t* out16, void* stream) {
  REQUIRE_WS(h);
  if (!out16) return fail(RECNET_EINVAL, "null argument");
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  HIPCHK(hipMemcpy(&out16[0], h->ctrl + RN_CTRL_RING, 8 * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&out16[8], h->scal + RN_SCAL_RING, 8 * 8, hipMemcpyDeviceToHost));
  return RECNET_OK;
}
// ---- learning-rate schedules (include/recnet_hip.h; the formula: common.hpp, rn_lr_at)
static_assert(sizeof(recnet_lr_schedule) == sizeof(RnLrSched) && offsetof(recnet_lr_schedule, scale) == offsetof(RnLrSched, scale), "recnet_lr_schedule is RnLrSched's layout");
// nullptr, or what is wrong with the descriptor (every comparison is written so that a NaN fails it)
static const char* lr_sched_problem(const recnet_lr_schedule* s) {
  if (s->kind < RECNET_LR_NONE || s->kind > RECNET_LR_STEP) return "unknown kind";
  if (s->warmup_steps < 0 || s->total_steps < 0) return "negative warmup_steps / total_steps";
  if ((s->kind == RECNET_LR_LINEAR || s->kind == RECNET_LR_COSINE) && s->total_steps <= s->warmup_steps) return "total_steps must exceed warmup_steps (linear, cosine)";
  if (s->kind == RECNET_LR_STEP && s->period <= 0) return "period must be positive (step)";
  if (!(s->min_factor >= 0.0 && s->min_factor <= 1.0)) return "min_factor outside [0, 1]";
  if (!(s->gamma > 0.0 && s->gamma <= 1.0)) return "gamma outside (0, 1]";
  if (!(s->scale > 0.0 && s->scale <= 1.7976931348623157e308)) return "scale must be positive and finite";
  return nullptr;
}
int recnet_set_lr_schedule(recnet_handle* h, int32_t which, const recnet_lr_schedule* sched, void* stream) {
  if (!h || !sched) return fail(RECNET_EINVAL, "null argument");
  if (which < 0 || which > 1) return fail(RECNET_EINVAL, "bad model index");
  if (const char* bad = lr_sched_problem(sched)) return fail(RECNET_EINVAL, std::string("lr schedule: ") + bad);
  RnLrSched d;
  memcpy(&d, sched, sizeof(d));
  if (h->ws) {
    hipStream_t st = (hipStream_t)stream;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone)
      return fail(RECNET_ESTATE, "recnet_set_lr_schedule on a capturing stream: a captured graph reads the descriptor, it does not set it");
    FLUSH_PENDING(h, st);      // (a pending reconstructor update belongs to a step of the old schedule)
    hipLaunchKernelGGL(set_lr_sched_kernel, dim3(1), dim3(1), 0, st, h->lrs + which, d);
    LAUNCH_OK();
  }
  h->lr_sched[which] = d;
  return RECNET_OK;
}
int recnet_get_lr_schedule(const recnet_handle* h, int32_t which, recnet_lr_schedule* out) {
  if (!h || !out) return fail(RECNET_EINVAL, "null argument");
  if (which < 0 || which > 1) return fail(RECNET_EINVAL, "bad model index");
  memcpy(out, &h->lr_sched[which], sizeof(*out));
  return RECNET_OK;
}
int recnet_lr_at(const recnet_lr_schedule* sched, double base_lr, int64_t step, double* out) {
  if (!sched || !out) return fail(RECNET_EINVAL, "null argument");
  if (const char* bad = lr_sched_problem(sched)) return fail(RECNET_EINVAL, std::string("lr schedule: ") + bad);
  if (step < 1) return fail(RECNET_EINVAL, "step must be >= 1");
  RnLrSched d;
  memcpy(&d, sched, sizeof(d));
  *out = rn_lr_at(d, base_lr, (long long)step);
  return RECNET_OK;
}
int recnet_read_lr(recnet_handle* h, double* out2, void* stream) {
  REQUIRE_WS(h);
  if (!out2) return fail(RECNET_EINVAL, "null argument");
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  for (int g = 0; g < 2; ++g) HIPCHK(hipMemcpy(&out2[g], &h->lrs[g].last_lr, 8, hipMemcpyDeviceToHost));
  return RECNET_OK;
}
int recnet_chain_reset(recnet_handle* h, int32_t disable_persistent, void* stream) {
  REQUIRE_WS(h);
  hipStream_t st = (hipStream_t)stream;
  for (int k = 0; k < CS_WS_BLOCKS; ++k) HIPCHK(hipMemsetAsync(cs_ws_sticky(h->gbar, k), 0, 4, st));
  HIPCHK(hipMemsetAsync(h->scal + RN_SCAL_POISON, 0, 4, st));
  // a pending deferred reconstructor update belongs to a step whose results are void: drop it (the poison word that made its
  // Adam kernel a no-op is cleared above, so a later flush would otherwise apply the garbage step's gradients)
  HIPCHK(hipMemsetAsync(h->ctrl + RN_CTRL_PENDING, 0, 4, st));
  h->maybe_pending = 0;
  if (disable_persistent) {
    h->persist_rec = h->persist_rec_bwd = h->persist_dec = h->persist_dec_bwd = 0; h->persist_loc = h->persist_loc_bwd = 0;
    h->persist_big_bwd = 0;      // (lcbig_bwd_kernel, R > 2048; the hybrid forward chain follows persist_loc)
    build_weight_images(h);      // the derived images of those chains are no longer kept
  }
  return RECNET_OK;
}

int recnet_debug_raise_give_up(recnet_handle* h, int32_t chain_bit, void* stream) {
  REQUIRE_WS(h);
  int k = -1;
  for (int i = 0; i < CS_WS_BLOCKS; ++i) if (chain_bit == (1 << i)) k = i;
  if (k < 0) return fail(RECNET_EINVAL, "chain_bit must be one chain's status bit");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, st, cs_ws_sticky(h->gbar, k), 1u);
  hipLaunchKernelGGL(set_u32_kernel, dim3(1), dim3(1), 0, st, (uint32_t*)(h->scal + RN_SCAL_POISON), 0x7fc00000u);
  LAUNCH_OK();
  return RECNET_OK;
}

__global__ __launch_bounds__(256) void occupy_kernel(unsigned long long ticks, unsigned* sink) {
  extern __shared__ unsigned occ_lds[];
  const unsigned long long t0 = wall_clock64();
  occ_lds[threadIdx.x] = threadIdx.x;
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
  if (occ_lds[(threadIdx.x + 1) & 255] == 0xdeadbeefu) *sink = 1;   // keeps the LDS allocation alive
}
int64_t recnet_debug_offset(const recnet_handle* h, int32_t which) {
  if (!h || !h->ws) return -1;
  const void* p = which == 0 ? (const void*)h->Whr : which == 1 ? (const void*)h->beta : which == 2 ? (const void*)h->Hr : which == 3 ? (const void*)h->acts_r :
                  which == 4 ? (const void*)h->dlog_lp : nullptr;
  return p ? (int64_t)((const char*)p - h->ws) : -1;
}
// Test hook (include/recnet_hip.h): are the packed operand images what pack_weights would write from the master parameters?
__global__ void count_diff_u16_kernel(const uint16_t* a, const uint16_t* b, size_t n, unsigned long long* cnt) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned c = 0;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) c += a[i] != b[i];
  if (c) atomicAdd(cnt, (unsigned long long)c);
}
// (the scratch comes from the caller, like every other buffer of this library: a raw hipMalloc / hipFree pair here, between the
// captures and replays of the tests' graphs, coincided with rare segmentation faults inside hipGraphLaunch — three of eight runs of
// tests/test_gpu_deferred.py in round 5, never under the debugger)
struct RnImg { void* p; size_t bytes; };
// every live image of the bound groups, from the handle's table (weight_images.hpp)
static int rn_image_list(recnet_handle* h, RnImg* im) {
  int n = 0;
  for (const WImage& w : h->wimg)
    if (w.live && h->og[w.group].bound && h->*w.field) { im[n].p = h->*w.field; im[n].bytes = wimg_bytes(w, h->lp); ++n; }
  return n;
}
int64_t recnet_debug_images_bytes(recnet_handle* h) {
  if (!h || !h->ws) return -1;
  RnImg im[WI_COUNT];
  const int n = rn_image_list(h, im);
  size_t total = 0;
  for (int i = 0; i < n; ++i) total += (im[i].bytes + 255) & ~(size_t)255;
  return (int64_t)(total + 256);
}
int recnet_debug_images_stale(recnet_handle* h, void* scratch_dev, int64_t scratch_bytes, int64_t* n_diff_out, void* stream) {
  REQUIRE_WS(h);
  if (!n_diff_out || !scratch_dev) return fail(RECNET_EINVAL, "null argument");
  FLUSH_PENDING(h, stream);
  hipStream_t st = (hipStream_t)stream;
  RnImg im[WI_COUNT];
  const int n = rn_image_list(h, im);
  size_t total = 0;
  for (int i = 0; i < n; ++i) total += (im[i].bytes + 255) & ~(size_t)255;
  if ((int64_t)(total + 256) > scratch_bytes || (((uintptr_t)scratch_dev) & 255)) return fail(RECNET_EINVAL, "scratch too small or not 256-byte aligned (recnet_debug_images_bytes)");
  char* scratch = (char*)scratch_dev;
  unsigned long long* cnt = (unsigned long long*)(scratch + total);
  HIPCHK(hipMemsetAsync(cnt, 0, 8, st));
  size_t off = 0;
  for (int i = 0; i < n; ++i) { HIPCHK(hipMemcpyAsync(scratch + off, im[i].p, im[i].bytes, hipMemcpyDeviceToDevice, st)); off += (im[i].bytes + 255) & ~(size_t)255; }
  int r = pack_weights(h, st);
  off = 0;
  for (int i = 0; i < n && !r; ++i) {
    hipLaunchKernelGGL(count_diff_u16_kernel, dim3(256), dim3(256), 0, st, (const uint16_t*)(scratch + off), (const uint16_t*)im[i].p, im[i].bytes / 2, cnt);
    off += (im[i].bytes + 255) & ~(size_t)255;
  }
  unsigned long long c = 0;
  hipError_t e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipMemcpy(&c, cnt, 8, hipMemcpyDeviceToHost);
  if (r) return r;
  if (e != hipSuccess) return fail(RECNET_EHIP, hipGetErrorString(e));
  *n_diff_out = (int64_t)c;
  return RECNET_OK;
}
int recnet_debug_occupy(recnet_handle* h, int32_t n_workgroups, int32_t microseconds, void* stream) {
  REQUIRE_WS(h);
  if (n_workgroups < 1 || n_workgroups > 1024 || microseconds < 1 || microseconds > 100000) return fail(RECNET_EINVAL, "bad occupy argument");
  const int lds = 160 * 1024;     // the whole LDS of a CU: nothing else is co-resident with one of these workgroups
  hipFuncSetAttribute(reinterpret_cast<const void*>(occupy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  hipLaunchKernelGGL(occupy_kernel, dim3(n_workgroups), dim3(256), lds, (hipStream_t)stream, (unsigned long long)microseconds * 100ull, h->ctrl + RN_CTRL_SINK_OCCUPY);
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_gemm(int32_t precision, const float* A, int32_t a_col, int32_t lda, const float* B, int32_t b_col,
                int32_t ldb, float* C, int32_t ldc, const float* bias, int32_t M, int32_t N, int32_t K,
                float alpha, int32_t accumulate, int32_t splitk, float* splitk_ws, void* stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0) return fail(RECNET_EINVAL, "bad gemm argument");
  if (splitk > 1 && !splitk_ws) return fail(RECNET_EINVAL, "split-K needs a workspace");
  rn_launch_gemm(precision, A, 0, a_col, lda, B, 0, b_col, ldb, C, ldc, bias, M, N, K, alpha, accumulate, splitk, splitk_ws, 1,
                 (hipStream_t)stream);
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_gemm_bf16(const void* A, int32_t a_col, int32_t lda, const void* B, int32_t b_col, int32_t ldb, float* C,
                     int32_t ldc, const float* bias, int32_t M, int32_t N, int32_t K, float alpha, int32_t accumulate,
                     int32_t splitk, float* splitk_ws, int32_t tag, void* stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0) return fail(RECNET_EINVAL, "bad gemm argument");
  if (splitk > 1 && !splitk_ws) return fail(RECNET_EINVAL, "split-K needs a workspace");
  if (tag < 0 || tag > 5) return fail(RECNET_EINVAL, "bad tag");
  rn_launch_gemm(RN_PREC_BF16, A, 1, a_col, lda, B, 1, b_col, ldb, C, ldc, bias, M, N, K, alpha, accumulate, splitk, splitk_ws, 1,
                 (hipStream_t)stream, tag);
  LAUNCH_OK();
  return RECNET_OK;
}

int recnet_gemm_group_bf16(int32_t a_col, int32_t b_col, int32_t n, const void* const* A, const int32_t* lda, const void* const* B,
                           const int32_t* ldb, float* const* C, const int32_t* ldc, const float* const* bias, const int32_t* M,
                           const int32_t* N, const int32_t* K, const float* alpha, const int32_t* accumulate, float* splitk_ws,
                           int64_t ws_floats, uint32_t* counters, int32_t n_counters, void* stream) {
  if (n < 1 || n > 8 || !A || !B || !C || !lda || !ldb || !ldc || !M || !N || !K) return fail(RECNET_EINVAL, "bad gemm group argument");
  RnGemmDesc d[8];
  for (int i = 0; i < n; ++i) {
    if (!A[i] || !B[i] || !C[i] || M[i] <= 0 || N[i] <= 0 || K[i] <= 0) return fail(RECNET_EINVAL, "bad gemm group member");
    d[i].A = A[i]; d[i].lda = lda[i]; d[i].B = B[i]; d[i].ldb = ldb[i]; d[i].C = C[i]; d[i].ldc = ldc[i]; d[i].bias = bias ? bias[i] : nullptr;
    d[i].M = M[i]; d[i].N = N[i]; d[i].K = K[i]; d[i].alpha = alpha ? alpha[i] : 1.f; d[i].accumulate = accumulate ? accumulate[i] : 0;
    d[i].c_bf16 = 0; d[i].c2 = nullptr; d[i].ldc2 = 0; d[i].ad_p = nullptr;
  }
  if (rn_launch_gemm_group(a_col, b_col, d, n, splitk_ws, (size_t)(ws_floats > 0 ? ws_floats : 0), counters, n_counters, (hipStream_t)stream))
    return fail(RECNET_EINVAL, "gemm group: operands must be 16-byte aligned bf16 with leading dimensions that are multiples of 8");
  LAUNCH_OK();
  return RECNET_OK;
}

// Algorithmic bytes of one launch: every loop invariant once (the resident weights / feature products) and every input or
// saved tensor of the T steps once.  The exchange blocks a chain kernel hands from step to step (h_t / dgates_t panels,
// stamped pre-activations) are an artefact of the implementation, not of the algorithm: chain_bytes(.., exchange = 1)
// reports them separately (written once and read back once; the PMC traffic additionally sees one fetch per XCD L2).
static double chain_bytes(const recnet_handle* h, int32_t which, int exchange) {
  const double wb = h->prec == RN_PREC_BF16 ? 2.0 : 4.0;
  const double T = h->T_last > 0 ? h->T_last : h->Tm, H = h->H, A = h->A, F = h->F, R = h->R, RA = h->RA, N = 4 * H + A;
  // rows of ONE bracketed launch: the reconstructor's chains are bracketed per row group (bgrp / bgrp_loc rows, recnet_create), the
  // decoder's chains once around all their groups (every group re-reads the resident weights)
  const bool dec = which == 5 || which == 6, loc = h->kind == RECNET_REC_LOCAL;
  const int grp = dec ? h->bgrp : (loc ? h->bgrp_loc : h->bgrp);
  const double B = dec || grp <= 0 || grp > h->B ? h->B : grp;
  const double ngr = dec && h->bgrp > 0 ? (h->B + h->bgrp - 1) / h->bgrp : 1;
  if ((which == 3 || which == 4) && h->kind == RECNET_REC_GLOBAL) {
    // rec_chain.hpp: W_hh once + per step Xg, acts, h, c and the row-major operand copy (fwd); acts, c_t, c_t-1, dG (bwd)
    const double w = 4 * R * R * wb;
    if (which == 3) return exchange ? T * 2 * B * R * wb : w + T * (B * 4 * R * 4 + B * 4 * R * 4 + 2 * B * R * 4 + B * R * wb);
    return exchange ? T * 2 * B * 4 * R * wb : w + B * R * 4 + T * (B * 4 * R * 4 + 2 * B * R * 4 + B * 4 * R * wb);
  }
  if ((which == 3 || which == 4) && h->kind == RECNET_REC_LOCAL) {
    // loc_chain.hpp: [W_ih | W_hh], W_r once, the decoder states and their projections Ud once; per step the saved
    // tensors (acts, h, c, beta, Whr, the LSTM input x) and the bf16 operand copies
    const double w = 4 * R * (H + R) * wb + RA * R * wb, inv = T * B * (H * 4 + RA * 4);
    const double NG = R / 16;     // unit groups: each contributes a [B][RA] fp32 block to the next step's attention projection
    if (which == 3) return exchange ? F * (2 * B * R * wb /*hr panel*/ + 2 * B * NG * RA * 2 /*rank-16 contributions, fp16*/ + 2 * B * H * wb /*x panel*/)
                                    : w + inv + F * (B * 4 * R * 4 + 2 * B * R * 4 + B * T * 4 + B * RA * 4 + B * (H + R) * wb);
    return exchange ? F * (2 * B * 4 * R * wb /*dG panel*/ + 2 * B * H * 4 * (h->lcb_xs ? (4 * R + 2047) / 2048 : 1) /*dx, one per K part*/ + 2 * B * RA * wb /*dWhr panel*/)
                    : w + inv + 2 * T * B * (H + RA) * 4 + F * (B * R * 4 + B * 4 * R * 4 + 2 * B * R * 4 + B * T * 4 + B * RA * 4 + B * 4 * R * wb + B * RA * wb);
  }
  if (which == 5 || which == 6) {
    // dec_chain.hpp: residents (packed [W_hh ; attn_W], the P blocks, Uv) once; per step Xe, h, c, acts, the operand copy of
    // h, Wh, att (fwd); dHs, dhid, acts, c_t, c_t-1, Wh and the row-major [dgates | dWh] rows (bwd) + dUv (both forms) once
    const double res = ngr * N * H * wb + B * F * 4 * H * wb + B * F * A * 4;
    // (round 4, F <= 32: the attention projection is formed inside the caption's workgroup — phase A hands over the 4H gate
    // columns only; dec_chain.hpp LW, same conditions as the launch site in host_decoder.inc)
    const bool lw = h->F <= 32 && h->A <= 128 && h->H <= 512 && (h->H & 31) == 0 && h->sw.dec_lw;
    if (which == 5) return exchange ? T * (2 * B * (lw ? 4 * H : N) * 8 + 2 * B * H * wb)
                                    : res + T * (B * 4 * H * 4 + 2 * B * H * 4 + B * 4 * H * 4 + B * H * wb + B * A * 4 + B * F * 4);
    return exchange ? T * (2 * B * H * 8 * DCB_KS + 2 * B * N * wb)
                    : res + B * F * A * (4 + wb) + T * (2 * B * H * 4 + B * 4 * H * 4 + 2 * B * H * 4 + B * A * 4 + B * (4 * H + 4 * A) * wb);
  }
  return 0;
}

double recnet_recurrent_step_bytes(const recnet_handle* h, int32_t which) {
  if (!h) return 0;
  const double wb = h->prec == RN_PREC_BF16 ? 2.0 : 4.0;
  // per-step launches: weights streamed once + activation block read + fp32 partial results written
  if (which == 0) return (double)(4 * h->H + h->A) * h->H * wb + (double)h->B * h->H * wb + (double)h->B * (4 * h->H + h->A) * 4;
  if (which >= 3 && which <= 6) return chain_bytes(h, which, 0);
  // which == 2: the backward form (dgates . W_hh): weights + the [B x 4R] gate-gradient block + fp32 result
  if (which == 2 && h->kind == RECNET_REC_GLOBAL) return (double)4 * h->R * h->R * wb + (double)h->B * 4 * h->R * wb + (double)h->B * h->R * 4;
  if (which == 2 && h->kind == RECNET_REC_LOCAL) return (double)4 * h->R * (h->H + h->R) * wb + (double)h->B * 4 * h->R * wb + (double)h->B * (h->H + h->R) * 4;
  if (h->kind == RECNET_REC_GLOBAL) return (double)4 * h->R * h->R * wb + (double)h->B * h->R * wb + (double)h->B * 4 * h->R * 4;
  if (h->kind == RECNET_REC_LOCAL) return (double)4 * h->R * (h->H + h->R) * wb + (double)h->B * (h->H + h->R) * wb + (double)h->B * 4 * h->R * 4;
  return 0;
}

double recnet_chain_exchange_bytes(const recnet_handle* h, int32_t which) {
  if (!h || which < 3 || which > 6) return 0;
  return chain_bytes(h, which, 1);
}

}  // extern "C"

