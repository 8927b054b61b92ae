// Common device helpers for the RecNet gfx950 kernels (wave64, MFMA, LDS).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __bf16 bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));

#define RN_WAVE 64

// ---------------------------------------------------------------- scalar and control slots of a handle's workspace
// scal: RN_SCAL_WORDS floats.  The loss scalars of recnet_scalars in its order, the decoder's gradient norm and clip factor, the
// poison word (0, or NaN after a chain kernel gave up waiting: chain_sync.hpp), and behind them as 64-bit words the step-end stamp
// (export_scalars_kernel) and the ring of the last step-end stamps (rn_ring_push: a count + 7 stamps).
enum {
  RN_SCAL_DEC_CE = 0, RN_SCAL_DEC_REG = 1, RN_SCAL_DEC_LOSS = 2, RN_SCAL_REC_MSE = 3, RN_SCAL_REC_REG = 4, RN_SCAL_REC_LOSS = 5,
  RN_SCAL_TOTAL = 6, RN_SCAL_GNORM = 7, RN_SCAL_CLIP = 8, RN_SCAL_POISON = 15, RN_SCAL_STAMP_END = 32, RN_SCAL_RING = 34,
  RN_SCAL_WORDS = 64
};
// ctrl: RN_CTRL_WORDS 32-bit words.  The dropout seed, the step counter (int32), the device's "a deferred reconstructor update is
// pending" word, three words that the timing / debugging kernels of abi_misc.inc write to, and as 64-bit words the step-start stamp
// (advance_step_kernel, set_step_kernel; wait_chain_kernel reads it) and the ring of the last step-start stamps.
enum {
  RN_CTRL_SEED = 0, RN_CTRL_STEP = 1, RN_CTRL_PENDING = 2, RN_CTRL_SINK_LAUNCH = 8, RN_CTRL_SINK_LDS = 16, RN_CTRL_SINK_OCCUPY = 17,
  RN_CTRL_STAMP_START = 32, RN_CTRL_RING = 34, RN_CTRL_WORDS = 64
};
#define RN_RING_WORDS 16      // 32-bit words of one stamp ring: 8 x 64 bit
static_assert(RN_SCAL_RING + RN_RING_WORDS <= RN_SCAL_WORDS && RN_CTRL_RING + RN_RING_WORDS <= RN_CTRL_WORDS, "the stamp rings end inside the words carved for scal / ctrl");
static_assert(RN_SCAL_STAMP_END % 2 == 0 && RN_SCAL_RING % 2 == 0 && RN_CTRL_STAMP_START % 2 == 0 && RN_CTRL_RING % 2 == 0, "64-bit slots are 8-byte aligned");

// ---------------------------------------------------------------- dropout (counter-based)
// keep(seed, site, t, b, j): see oracle/dropmask.py (the numpy restatement used by the tests).
#define RN_SITE_DEC_EMBED 0u
#define RN_SITE_DEC_LOGIT 1u
#define RN_SITE_REC_INPUT 2u
#define RN_SITE_SAMPLE 3u      // Gumbel noise of the sampling search, tensor [B, V] at step t (kernels_search.hpp: sample_rows_kernel)

__host__ __device__ __forceinline__ uint32_t rn_fmix32(uint32_t x) {
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}
__host__ __device__ __forceinline__ uint32_t rn_site_key(uint32_t seed, uint32_t site) {
  return seed * 0x632BE5ABu + site * 0x7F4A7C15u + 0x1234567u;
}
// returns the multiplicative mask: 0 (dropped) or 1/(1-p) (kept).  thr = floor(p*2^32), thr==0 -> no dropout.
__device__ __forceinline__ float rn_drop_scale(uint32_t key, uint32_t thr, float inv_keep, uint32_t idx) {
  if (thr == 0u) return 1.0f;
  uint32_t h = rn_fmix32(idx * 0x9E3779B1u + key);
  return h >= thr ? inv_keep : 0.0f;
}
__host__ __forceinline__ uint32_t rn_drop_thr(float p) {
  if (p <= 0.f) return 0u;
  double v = (double)p * 4294967296.0;
  return v >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)v;
}

// ---------------------------------------------------------------- reductions
// Wave-wide reductions (all 64 lanes active; every lane gets the result).  Four DPP steps (quad swaps, half-row and row
// mirrors: ~10 clocks each) leave the sum of each 16-lane row in all of its lanes, four v_readlane fetch the row sums.
// (The __shfl_xor butterfly costs six dependent ds_bpermute round trips, ~700 clocks — measured: seven of them in a row
// were 2.5 us of a 16 us decoder step.)
template <int CTRL> __device__ __forceinline__ float rn_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float rn_readlane(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ float wave_sum(float v) {
  v += rn_dpp<0xB1>(v);     // quad_perm [1,0,3,2]
  v += rn_dpp<0x4E>(v);     // quad_perm [2,3,0,1]
  v += rn_dpp<0x141>(v);    // row_half_mirror
  v += rn_dpp<0x140>(v);    // row_mirror
  return (rn_readlane(v, 0) + rn_readlane(v, 16)) + (rn_readlane(v, 32) + rn_readlane(v, 48));
}
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, rn_dpp<0xB1>(v));
  v = fmaxf(v, rn_dpp<0x4E>(v));
  v = fmaxf(v, rn_dpp<0x141>(v));
  v = fmaxf(v, rn_dpp<0x140>(v));
  return fmaxf(fmaxf(rn_readlane(v, 0), rn_readlane(v, 16)), fmaxf(rn_readlane(v, 32), rn_readlane(v, 48)));
}
// block-wide sum for blockDim.x == 256 (4 waves); sm: >= 4 floats of LDS scratch. All threads get the result.
__device__ __forceinline__ float block_sum256(float v, float* sm) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return sm[0] + sm[1] + sm[2] + sm[3];
}
__device__ __forceinline__ float block_max256(float v, float* sm) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
}

// Transcendentals.  The recurrent-step kernels are VALU-issue bound on tanh / sigmoid (libm tanhf is ~80
// instructions); these forms are one v_exp_f32 + one v_rcp_f32 (~12 instructions) with absolute error
// <= 3e-7, far inside the fp32-path parity bar (2e-5 on hidden states).
__device__ __forceinline__ float rn_exp(float x) { return __expf(x); }
__device__ __forceinline__ float rn_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float rn_tanh(float x) {
  const float t = __expf(-2.0f * fabsf(x));
  const float r = (1.0f - t) * __builtin_amdgcn_rcpf(1.0f + t);
  return copysignf(r, x);
}

// ---------------------------------------------------------------- learning-rate schedule
// lr(n) = base_lr * scale * warm(n) * decay(n) for the 1-based optimiser step n, in double: the one definition, called by both Adam
// sites on the device (their first thread, beside the bias corrections) and by recnet_lr_at on the host.  With W = warmup_steps,
// m = max(0, n - W), M = total_steps - W:  warm = n / W below W, else 1;  decay = 1 (CONSTANT) | 1 - (1 - fmin) min(m, M) / M (LINEAR) |
// fmin + (1 - fmin) (1 + cos(pi min(m, M) / M)) / 2 (COSINE) | max(fmin, sqrt(W' / max(n, W'))), W' = max(W, 1) (INVSQRT) |
// max(fmin, gamma ^ floor(m / period)) (STEP).  NONE (a handle's state at creation) is the factor 1.0 exactly: base_lr * 1.0 * 1.0
// has base_lr's bits.  The ranges are checked where a descriptor is installed (recnet_set_lr_schedule).
enum { RN_LR_NONE = 0, RN_LR_CONSTANT = 1, RN_LR_LINEAR = 2, RN_LR_COSINE = 3, RN_LR_INVSQRT = 4, RN_LR_STEP = 5 };
struct RnLrSched { int32_t kind, warmup_steps, total_steps, period; double min_factor, gamma, scale; };      // (recnet_lr_schedule's layout)
// one optimiser's words in device memory: the descriptor the Adam launches read, and the lr the last of them used
struct RnLrSlot { RnLrSched s; double last_lr; };
__host__ __device__ inline double rn_lr_factor(const RnLrSched& s, long long n) {
  if (s.kind == RN_LR_NONE) return 1.0;
  const long long W = s.warmup_steps, m = n > W ? n - W : 0, M = (long long)s.total_steps - W;
  const double warm = n < W ? (double)n / (double)W : 1.0, fmin = s.min_factor;
  double decay = 1.0;
  if (s.kind == RN_LR_LINEAR) decay = 1.0 - (1.0 - fmin) * (double)(m < M ? m : M) / (double)M;
  else if (s.kind == RN_LR_COSINE) decay = fmin + (1.0 - fmin) * 0.5 * (1.0 + cos(3.14159265358979323846 * (double)(m < M ? m : M) / (double)M));
  else if (s.kind == RN_LR_INVSQRT) { const long long W1 = W > 1 ? W : 1; decay = sqrt((double)W1 / (double)(n > W1 ? n : W1)); decay = decay > fmin ? decay : fmin; }
  else if (s.kind == RN_LR_STEP) { decay = pow(s.gamma, (double)(m / s.period)); decay = decay > fmin ? decay : fmin; }
  return warm * decay;
}
__host__ __device__ inline double rn_lr_at(const RnLrSched& s, double base_lr, long long n) { return base_lr * s.scale * rn_lr_factor(s, n); }

// ---------------------------------------------------------------- Adam (shared by adam_chunk_kernel and the GEMM epilogue)
// torch.optim.Adam (single-tensor form of torch 2.10): g' = clip * (g + reg) + wd * p ; m <- lerp(m, g', 1-b1) ;
// v <- b2 v + (1-b2) g'^2 ; [vmax <- max(vmax, v)] ; p <- p - (lr / bc1) * m / (sqrt(v̂) / sqrt(bc2) + eps).
// One definition, contraction pinned per expression, so that the optimiser kernel and the weight-gradient product that applies
// the update in its epilogue (gemm_lds.hpp) round identically.
struct AdamHyper { double lr, beta1, beta2; float eps, wd, one_m_b1, beta2f, one_m_b2; int amsgrad; float reg_coef; };
// what the products of one grouped launch share when they apply Adam in their epilogue (gemm_lds.hpp)
// (lrs: the optimiser's schedule descriptor and last-lr word; hp.lr is the base lr)
struct AdamShared { AdamHyper hp; const int32_t* step_ptr; const float* poison; const uint32_t* pending; int step_off; int pad; RnLrSlot* lrs; };
__device__ __forceinline__ float rn_adam_update(float p, float gr, float& m, float& v, float& vmx, float k, float cl, const AdamHyper& hp,
                                                float step_size, float bc2s) {
#pragma clang fp contract(on)
  float g = (gr + k * p) * cl;
  g = g + hp.wd * p;
  m = m + hp.one_m_b1 * (g - m);
  v = v * hp.beta2f + hp.one_m_b2 * g * g;
  float vh = v;
  if (hp.amsgrad) { vh = fmaxf(vmx, v); vmx = vh; }
  const float denom = sqrtf(vh) / bc2s + hp.eps;
  return p - step_size * (m / denom);
}
