// What the persistent chain kernels (rec_chain.hpp, loc_chain.hpp, loc_big.hpp) share of their compute half: the rotated k-step.  The
// other blocks they repeat stay written out — as function templates they compiled to other instruction streams (DESIGN.md section 4:
// the table of forms tried, and the rule that a change here is checked with tools/kernel_isa_diff.py before it goes to a GPU).
#pragma once
#include "common.hpp"
// k of step (pair pr, half hh) of a wave whose K range starts at kw0 and holds NP pairs of 32-k steps, ROTATED by rot pairs (workgroups
// start at different k: spreads the L2 channels).  ct_k_of<NP>: the chain kernels' k_of lambdas — only with NP a template parameter are
// their listings the ones of the written-out expression.  ct_k_of(NP, ..): the packers of the streamed images, where NP is a run-time value.
__host__ __device__ __forceinline__ constexpr int ct_k_of(int NP, int kw0, int rot, int pr, int hh) { int prr = pr + rot; prr = prr >= NP ? prr - NP : prr; return kw0 + (prr * 2 + hh) * 32; }
template <int NP> __host__ __device__ __forceinline__ constexpr int ct_k_of(int kw0, int rot, int pr, int hh) { int prr = pr + rot; prr = prr >= NP ? prr - NP : prr; return kw0 + (prr * 2 + hh) * 32; }
template <int NP> constexpr bool ct_k_of_forms_agree(int i = 0) {      // i = (rot, pr, hh)
  return i == 2 * NP * NP || (ct_k_of<NP>(96, i / (2 * NP), i / 2 % NP, i & 1) == ct_k_of(NP, 96, i / (2 * NP), i / 2 % NP, i & 1) && ct_k_of_forms_agree<NP>(i + 1));
}
static_assert(ct_k_of_forms_agree<1>() && ct_k_of_forms_agree<2>() && ct_k_of_forms_agree<7>() && ct_k_of_forms_agree<14>(), "the two forms of ct_k_of are one function");
