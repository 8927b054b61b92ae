// The hand-over protocol of the persistent chain kernels (rec_chain.hpp, dec_chain.hpp, loc_chain.hpp, loc_big.hpp), in one place:
// the layout of a chain's barrier block, launch epoch and phase stamps, the bounded waits and their sticky word, the flag polls,
// arrive / release / wait_release, the write-through stores and the panel helpers — and the table of the handle's barrier
// workspace that the host code carves those blocks from.
#pragma once
#include "common.hpp"

// ---------------------------------------------------------------- layout of one chain's barrier block (4-byte words)
//   [0, CS_FLAGS)                        arrival flags, one word per workgroup
//   CS_RELEASE + x * CS_LINE + slot      release words: one 128-byte line per XCD x, up to three words (slots) per line
//   CS_STICKY                            the sticky "a waiter gave up" word (word 1 of release line 0: no slot uses it)
#define CS_FLAGS 256
#define CS_RELEASE 256
#define CS_LINE 32
#define CS_STICKY (CS_RELEASE + 1)
#define CS_REL_A 0
#define CS_REL_B 8
#define CS_REL_C 16
#define CS_BLOCK (CS_RELEASE + 8 * CS_LINE)
// the decoder chains' partial hand-over (cs_wait_part): [8 XCDs][CS_PARTS row parts] lines of arrival words
#define CS_PARTS 4
#define CS_REP_WORDS (8 * CS_PARTS * CS_LINE)

// Acquire side of the barriers.  An agent-scope acquire fence is `buffer_inv sc1`: it drops every non-local line of the
// XCD's L2 — under all other workgroups of the chain and under the batched GEMMs of the side stream — 120-190 times
// per time step (measured: 0.12 ms of a 2.29 ms train step).  It is not needed here: (a) every exchange block has its own
// address per time step and nobody touches it before the barrier that publishes it, so no L1 / L2 can hold a line of it
// from an earlier step of this launch; (b) lines from an earlier LAUNCH are dropped by the acquire of the kernel dispatch
// itself (the same mechanism every producer -> consumer pair of kernels on different XCDs relies on); (c) producers write
// through (sc1 stores) and are acknowledged before they arrive at the barrier, so memory holds the data when the
// consumer's first — necessarily missing — load goes out; (d) flags, release words and stamped words are read with sc1
// loads.  RC_ACQUIRE_INV=1 compiles the fences back in (same results on every test; Makefile: acqinv).
#ifndef RC_ACQUIRE_INV
#define RC_ACQUIRE_INV 0
#endif

// ---------------------------------------------------------------- launch epoch and phase stamps
// Grid barrier, split in two so that the stores nobody waits for are issued between the halves.
//   arrive: the caller has already waited for its write-through stores of h_t (s_waitcnt vmcnt(0) + __syncthreads: cs_publish_arrive);
//           one agent-scope store of the step number into this workgroup's own flag — no read-modify-write, so the
//           arrivals of the R / 8 workgroups do not serialise on one address;
//   wait:   wave 0 polls all flags (one agent-scope load per 64 workgroups) until every one has reached the step, then
//           invalidates this CU's L1 and this XCD's L2 (acquire) so that the next loads of h_t come from memory.
// Launch epoch: one word per chain kernel in device memory, read by every workgroup at the start and incremented by
// workgroup 0 at the end (a workgroup that has passed a barrier knows every other one has started).  Barrier flags are
// epoch << 7 | phase and stamped words carry epoch << 6 | step, so neither needs clearing between launches — in a replayed
// hipGraph each clearing memset was a 6 us node on the critical path.
// Phase stamps (recnet_read_stamps): the launch-epoch words of the six chain kernels are consecutive words at the start of a
// 256-byte line; the line behind it holds one pair of 100 MHz wall-clock stamps per chain — written by workgroup 0 when it starts
// running and when it leaves — so that a REPLAYED hipGraph, which no tracer has to be attached to, reports where its step went
// (prologue / chains / gaps / tail) at the cost of two 8-byte stores per launch.
__device__ __forceinline__ unsigned long long* rc_stamp_slot(const unsigned* epoch) {
  const unsigned long long a = (unsigned long long)epoch;
  return reinterpret_cast<unsigned long long*>((a & ~255ull) + 256ull) + 2 * ((a >> 2) & 7ull);
}
__device__ __forceinline__ unsigned rc_epoch_read(const unsigned* epoch) {
  // (written through: wait_chain_kernel on another XCD polls it)
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) __hip_atomic_store(rc_stamp_slot(epoch), (unsigned long long)wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __hip_atomic_load(epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- bounded waiting
// Every wait in the chain kernels is bounded: a launch whose workgroups are not all resident (two such launches sharing
// the GPU) would otherwise spin forever and take the device with it.  After ~2^22 polls (seconds) a waiter raises the
// sticky word bar[CS_STICKY]; every wait of this and of later launches then falls through, and the kernel poisons the step's
// total loss with NaN (cs_finish) — wrong loudly instead of hung.
#define RC_SPIN_LIMIT (1u << 22)
__device__ __forceinline__ void cs_raise(unsigned* bar) { __hip_atomic_store(bar + CS_STICKY, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ bool rc_give_up(unsigned* bar, unsigned& spin) {
  if ((++spin & 0x3ffu) != 0) return false;
  if (spin <= RC_SPIN_LIMIT && __hip_atomic_load(bar + CS_STICKY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return false;
  cs_raise(bar);
  return true;
}
// The end of a launch, by ONE thread that knows every workgroup has read the epoch: bump the epoch, stamp the end, poison the
// loss if the sticky word is raised.
__device__ __forceinline__ void cs_finish(unsigned* epoch, unsigned e, unsigned* bar, float* poison) {
  __hip_atomic_store(epoch, e + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  rc_stamp_slot(epoch)[1] = wall_clock64();
  if (__hip_atomic_load(bar + CS_STICKY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) *poison = __builtin_nanf("");
}

// ---------------------------------------------------------------- polls (by one wave: lane = threadIdx.x < 64)
// all n <= CS_FLAGS flags have reached `target`.  Four loads per lane, all in flight together (a loop that folds each flag
// into a running minimum waits for every load before issuing the next one: three memory round trips per poll instead of one).
// SLEEP: with every workgroup of the grid polling, not one relay.
template <bool SLEEP>
__device__ __forceinline__ void cs_poll(const unsigned* flags, int n, unsigned target, unsigned* bar, unsigned& spin) {
  const int l = threadIdx.x;
  const unsigned* f0 = flags + (l < n ? l : n - 1);
  const unsigned* f1 = flags + (l + 64 < n ? l + 64 : n - 1);
  const unsigned* f2 = flags + (l + 128 < n ? l + 128 : n - 1);
  const unsigned* f3 = flags + (l + 192 < n ? l + 192 : n - 1);
  for (;;) {
    const unsigned a0 = __hip_atomic_load(f0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned a1 = __hip_atomic_load(f1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned a2 = __hip_atomic_load(f2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned a3 = __hip_atomic_load(f3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // flags count up across launches (base = launch epoch << 7): signed distance, wrap-safe
    const bool ok = (int)(a0 - target) >= 0 && (int)(a1 - target) >= 0 && (int)(a2 - target) >= 0 && (int)(a3 - target) >= 0;
    if (__all(ok)) break;
    if (rc_give_up(bar, spin)) break;
    if (SLEEP) __builtin_amdgcn_s_sleep(1);
  }
}
// up to 64 flags, one per lane (`mine` = this lane's; spare lanes point at any flag of the set), then the optional acquire
__device__ __forceinline__ void cs_poll_wave(const unsigned* mine, unsigned target, unsigned* bar) {
  unsigned spin = 0;
  while (!__all((int)(__hip_atomic_load(mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) >= 0)) { if (rc_give_up(bar, spin)) break; }
  if (RC_ACQUIRE_INV) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// ---------------------------------------------------------------- arrive / wait / release
// the linear index of this workgroup: the hardware deals workgroups to XCD cs_wg() % 8
__device__ __forceinline__ int cs_wg() { return (int)(blockIdx.y * gridDim.x + blockIdx.x); }
__device__ __forceinline__ void cs_arrive(unsigned* flag, unsigned v) {
  if (threadIdx.x == 0) __hip_atomic_store(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The hand-over tail of a producer: its write-through stores are acknowledged (cs_publish_sync: by every thread of the workgroup), then
// it arrives.  Stores nobody waits for are issued BEHIND this, so that they do not sit in the vmcnt that is being waited for.
__device__ __forceinline__ void cs_publish_sync() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}
__device__ __forceinline__ void cs_publish_arrive(unsigned* flag, unsigned v) {
  cs_publish_sync();
  cs_arrive(flag, v);
}
// every workgroup of the grid polls every flag
__device__ __forceinline__ void cs_wait_grid(unsigned* bar, unsigned target) {
#ifndef RC_PROBE_NO_BARRIER
  if (threadIdx.x < 64) {
    unsigned spin = 0;
    cs_poll<true>(bar, gridDim.x * gridDim.y, target, bar, spin);
#ifndef RC_PROBE_NO_FENCE
    if (RC_ACQUIRE_INV) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
  }
#endif
  __syncthreads();
}
// Barrier through a master workgroup.  With every workgroup polling every flag, the 130-190 pollers (four wave loads each
// per round, all to the same six lines) queue up at the memory side: the flag round cost 2.7 us, while an uncontended
// store -> load hand-over between two CUs is 0.3-0.4 us (tools/micro/xcd_pingpong.hip).  Here one extra workgroup does
// nothing but poll the arrival flags (cs_poll) and, when all have reached a phase, write that phase into eight release words (one
// 128-byte line per XCD-sized group of workgroups); the workers poll only their release word.
__device__ __forceinline__ void cs_release(unsigned* bar, int slot, unsigned v) {
  if (threadIdx.x < 8) __hip_atomic_store(bar + CS_RELEASE + slot + threadIdx.x * CS_LINE, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// workers: wave 0 polls the release word in the line of this workgroup's XCD (wg = its linear index)
__device__ __forceinline__ void cs_wait_release(unsigned* bar, int slot, int wg, unsigned target) {
#ifndef RC_PROBE_NO_BARRIER
  if (threadIdx.x < 64) {
    const unsigned* r = bar + CS_RELEASE + slot + (wg & 7) * CS_LINE;
    unsigned spin = 0;
    while ((int)(__hip_atomic_load(r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0) { if (rc_give_up(bar, spin)) break; }
    if (RC_ACQUIRE_INV) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
#endif
  __syncthreads();
}

// Partial hand-over B -> A of the decoder chains (round 5).  A phase-A workgroup reads only the `own` = 28 panel rows of its row
// part, i.e. the rows of 28 captions, and phase B of a caption polls the stamped words of the unit groups of ITS part: the
// dependencies close inside a row part, so nothing needs the whole grid.  Against a relayed grid barrier (arrive -> master sees all
// 128 -> release word -> waiter) that is one memory round trip instead of two, and a part does not wait for the stragglers of the
// other three.
// A caption writes its arrival into one replica of its part's flag line per XCD that hosts the part's phase-A workgroups (rep:
// [8][CS_PARTS][32] words, a 128-byte line per (XCD, part)); a waiter polls the replica of its own XCD (blockIdx % 8) with one wave load.
// With ONE copy polled by all 128 workgroups the step got 0.9 us LONGER (measured: 315 against 288 us per launch) — a line that is
// written from eight XCDs and read from eight is the worst case for the L2s; in this form every line has its readers in one XCD.
// Workgroups without a phase A (on = false) do not wait.  n = captions of the part in this launch.
__device__ __forceinline__ void cs_wait_part(bool on, unsigned* rep, int part, int n, unsigned target, unsigned* bar) {
  if (on && threadIdx.x < 64 && n > 0)
    cs_poll_wave(rep + ((blockIdx.x & 7) * CS_PARTS + part) * CS_LINE + ((int)threadIdx.x < n ? (int)threadIdx.x : n - 1), target, bar);
  __syncthreads();
}
// caption `slot` of row part `part`: the replicas of the part's two XCDs
__device__ __forceinline__ void cs_arrive_part(unsigned* rep, int part, int slot, unsigned v) {
  if (threadIdx.x < 2) __hip_atomic_store(rep + ((2 * part + threadIdx.x) * CS_PARTS + part) * CS_LINE + slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- write-through stores, exchange panels
// 16 bytes per lane, written through to the agent's coherence point: the instruction an agent-scope relaxed atomic store compiles
// to (global_store_dwordx2 ... sc1), in its 16-byte form — one request per lane instead of two
// (the s_nop 1 = the TWO wait states a VMEM store of more than 8 bytes needs before a VALU instruction may overwrite its data
// registers: the compiler's hazard recognizer inserts `s_nop 1` behind its own dwordx4 stores and does not look inside inline asm —
// without it the next loop iteration's adds corrupted the stored values; `s_nop 0` was one state short)
__device__ __forceinline__ void rc_store16f(float* dst, f32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(dst), "v"(v) : "memory");
}
__device__ __forceinline__ void rc_store16(bf16_t* dst, const bf16_t* src) {
  rc_store16f(reinterpret_cast<float*>(dst), *reinterpret_cast<const f32x4*>(src));
}
#define RC_MB 7               // 16-row blocks: B <= 112
// Layout of the copy of h_t that the chain itself reads back.  An MFMA A-fragment load (16 rows x 32 k, 16 bytes per
// lane) is issued by the texture unit 16 lanes at a time, and in a row-major matrix those 16 lanes are 16 different
// rows = 16 different cache lines for 256 bytes (measured: ~58 clocks per wave load, 8 us per step for the 307 KB
// block).  Stored as [k / 8][row][8] the same 16 lanes read 256 contiguous bytes (two full lines), and a workgroup's
// 8 units x B rows are one contiguous run for the writer.
#define RC_PAN_ROWS (RC_MB * 16)
// elements of one step's panel for a contraction length K (k-groups padded to whole 32-k steps)
__host__ __device__ inline size_t rc_pan_elems(int K) { return (size_t)(((K + 31) >> 5) << 2) * RC_PAN_ROWS * 8; }
// zero the k-groups that pad K to a multiple of 32, in every step's panel (one workgroup, K % 32 != 0): a partly live k-step
// reads them (against zero weights — but 0 x garbage could be NaN).  Published by the first barrier like h_0.
__device__ __forceinline__ void rc_pan_zero_pad(bf16_t* Pan, int K, int T, int tid) {
  const size_t pan_t = rc_pan_elems(K);
  const int pad0 = K >> 3, padn = (((K + 31) >> 5) << 2) - pad0;
  for (int t = 0; t < T; ++t)
    for (int j = tid; j < padn * RC_PAN_ROWS * 2; j += 256)
      __hip_atomic_store(reinterpret_cast<uint64_t*>(Pan + (size_t)t * pan_t + (size_t)pad0 * RC_PAN_ROWS * 8) + j, (uint64_t)0,
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- the barrier workspace of a handle (host; 4-byte words)
// CS_WS_BLOCKS blocks of CS_BLOCK words: block k belongs to the chain whose status bit is 1 << k (recnet_chain_status), except
// block CS_WS_EPOCH_BLOCK, which holds the launch epochs (one word per chain, in the order of wait_chain's k), the phase stamps in
// the 256-byte line behind them (rc_stamp_slot) and the stamps of the grouped launches; behind the blocks the two replica regions
// of the decoder chains (cs_wait_part).  lcbig_bwd_kernel stands in for the local backward chain and uses its entry.
enum CsChain { CS_DEC_FWD, CS_DEC_BWD, CS_REC_FWD, CS_REC_BWD, CS_LOC_FWD, CS_LOC_BWD, CS_CHAINS };      // = epoch word, stamp pair
struct CsChainWs { int block, status_bit; };
constexpr CsChainWs cs_chain_ws[CS_CHAINS] = {{2, 4}, {3, 8}, {0, 1}, {1, 2}, {5, 32}, {6, 64}};
constexpr int CS_WS_BLOCKS = 7, CS_WS_EPOCH_BLOCK = 4;
constexpr int CS_WS_EPOCH = CS_WS_EPOCH_BLOCK * CS_BLOCK;      // epoch word of chain c at + c
constexpr int CS_WS_STAMPS = CS_WS_EPOCH + 64;                 // [CS_CHAINS] x (begin, end), 8-byte words
constexpr int CS_WS_GROUP_STAMPS = CS_WS_EPOCH + 128;          // [8 sites] x (start, end), 8-byte words
constexpr int CS_WS_REP_DEC_BWD = 4352, CS_WS_REP_DEC_FWD = CS_WS_REP_DEC_BWD + CS_REP_WORDS;
constexpr int CS_WS_WORDS = CS_WS_REP_DEC_FWD + CS_REP_WORDS;
inline unsigned* cs_ws_bar(unsigned* ws, CsChain c) { return ws + cs_chain_ws[c].block * CS_BLOCK; }
inline unsigned* cs_ws_epoch(unsigned* ws, CsChain c) { return ws + CS_WS_EPOCH + c; }
inline unsigned* cs_ws_sticky(unsigned* ws, int block) { return ws + block * CS_BLOCK + CS_STICKY; }
constexpr bool cs_ws_table_ok() {
  for (int c = 0; c < CS_CHAINS; ++c) {
    if (cs_chain_ws[c].status_bit != 1 << cs_chain_ws[c].block) return false;
    if (cs_chain_ws[c].block >= CS_WS_BLOCKS || cs_chain_ws[c].block == CS_WS_EPOCH_BLOCK) return false;
    for (int d = 0; d < c; ++d) if (cs_chain_ws[d].block == cs_chain_ws[c].block) return false;
  }
  return true;
}
static_assert(cs_ws_table_ok(), "every chain has a block of its own, none the epoch block, and status bit 1 << block");
static_assert(CS_STICKY % CS_LINE != CS_REL_A && CS_STICKY % CS_LINE != CS_REL_B && CS_STICKY % CS_LINE != CS_REL_C && CS_STICKY < CS_RELEASE + CS_LINE,
              "the sticky word lies in release line 0 and is no release word");
static_assert(CS_CHAINS <= 8 && (CS_WS_EPOCH * 4) % 256 == 0 && CS_WS_STAMPS == CS_WS_EPOCH + 64,
              "rc_stamp_slot: the epoch words share one 256-byte line, the stamp line is the one behind it");
static_assert(CS_WS_STAMPS + 4 * CS_CHAINS <= CS_WS_GROUP_STAMPS && CS_WS_GROUP_STAMPS + 4 * 8 <= CS_WS_EPOCH + CS_STICKY,
              "epoch block: epochs, stamps and group stamps do not overlap and stay below the word recnet_chain_status reads as bit 16");
static_assert(CS_WS_BLOCKS * CS_BLOCK <= CS_WS_REP_DEC_BWD && CS_WS_REP_DEC_BWD + CS_REP_WORDS <= CS_WS_REP_DEC_FWD &&
              CS_WS_REP_DEC_FWD + CS_REP_WORDS <= CS_WS_WORDS, "blocks, then the two replica regions, inside the allocation");
static_assert(CS_WS_EPOCH == 2048 && CS_WS_REP_DEC_FWD == 5376 && CS_WS_WORDS == 6400 && CS_BLOCK == 512 && CS_STICKY == 257,
              "recorded profiles and tests/test_gpu_loop.py address these words by number");
