// vss_returns.hip — a rollout's advantages and returns in one launch (gfx950): vss_gae of include/vss.h.
//
// The train loop's timeout-aware GAE (ppo_continuous_action_isaacgym.py compute_gae, the reference's
// ppo…:282-296) is a reversed scan over the T steps of the rollout: per step nine small torch kernels, and
// for the fused policy a where / cat merge of the terminal values in front of it (vss_amd/policy.py
// TerminalValues.next_values) -- about 1,160 launches per update at T = 128, whatever the row count.  Here:
//
//   one lane per column e (a learner row of the batch), 64-lane workgroups; the lane walks t = T-1 .. 0 with
//   the running advantage in a register.  Every access is one dword per lane, 256 contiguous bytes per
//   wave-instruction per (t, array); row widths such as 4,095 rule out 16-B vectors.
//
//   The loads do not depend on the recurrence: the t loop is unrolled by kUnroll steps whose 5 loads each
//   (rewards, values, next_values or term_values, next_dones, next_timeouts) are all issued before the
//   group's dependent chain runs -- 40 in flight at kUnroll = 8, under the 63 the vmcnt counter holds.  The
//   T % kUnroll steps at the low end of t run one at a time.  Stores are plain.
//
//   The sum is NOT split over t (no affine scan across waves): that would reassociate it.  The float
//   operation order is that of the torch expressions, with FMA contraction off (-ffp-contract=off and the
//   pragma below), so the result equals compute_gae bit for bit (tests/test_gae.py):
//     nnt   = (next_dones != 0 && next_timeouts == 0) ? 0.f : 1.f
//     delta = ((rewards + (gamma * nv) * nnt) - values)
//     last  = delta + ((gamma_lambda * (1.f - next_dones)) * last)
//     advantages[t][e] = last;  returns[t][e] = last + values[t][e]
//
//   Form B merges the terminal values in the kernel: nv = next_dones != 0 ? term_values[t][e] : values[t+1][e]
//   (v_last[e] above the last step).  values[t+1][e] is the register the previous iteration loaded; the merge
//   is a select, so a stale term_values of a row that did not reset never enters a sum.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vss.h"

#pragma clang fp contract(off)

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "vss_returns.hip targets gfx950 (CDNA4) only"
#endif

// steps per load group: 8 or 4 (measured: DESIGN.md §14, profiles/gae_bench.json)
#ifndef VSS_GAE_UNROLL
#define VSS_GAE_UNROLL 8
#endif

namespace vret {

constexpr int kWave = 64;
constexpr int kUnroll = VSS_GAE_UNROLL;
static_assert(kUnroll >= 1 && kUnroll * 5 <= 63, "a group's loads must fit the vmcnt counter");

// one step of the recurrence; `x` is next_values (form A) or term_values (form B, MERGE), v_up = values[t + 1]
template <bool MERGE>
__device__ __forceinline__ float gae_step(float r, float v, float x, float d, float o, float v_up, float gamma, float gl,
                                          float last) {
  const float nv = MERGE ? (d != 0.f ? x : v_up) : x;
  const float nnt = (d != 0.f && o == 0.f) ? 0.f : 1.f;
  const float delta = (r + (gamma * nv) * nnt) - v;
  return delta + (gl * (1.f - d)) * last;
}

template <int U, bool MERGE>
__global__ __launch_bounds__(kWave) void gae_kernel(int64_t T, int64_t E, const float* __restrict__ rew,
                                                    const float* __restrict__ val, const float* __restrict__ nvt,
                                                    const float* __restrict__ v_last, const float* __restrict__ dn,
                                                    const float* __restrict__ to, float gamma, float gl,
                                                    float* __restrict__ adv, float* __restrict__ ret) {
  const int64_t e = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (e >= E) return;
  float last = 0.f;
  float v_up = 0.f;  // values[t + 1][e]; form B only
  if constexpr (MERGE) v_up = v_last[e];
  int64_t t = T;
  while (t >= U) {
    t -= U;  // the group's steps t + U-1 .. t, highest first
    float r[U], v[U], x[U], d[U], o[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int64_t i = (t + (U - 1 - j)) * E + e;
      r[j] = rew[i];
      v[j] = val[i];
      x[j] = nvt[i];
      d[j] = dn[i];
      o[j] = to[i];
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int64_t i = (t + (U - 1 - j)) * E + e;
      last = gae_step<MERGE>(r[j], v[j], x[j], d[j], o[j], v_up, gamma, gl, last);
      adv[i] = last;
      ret[i] = last + v[j];
      v_up = v[j];
    }
  }
  while (t > 0) {
    --t;
    const int64_t i = t * E + e;
    const float v = val[i];
    last = gae_step<MERGE>(rew[i], v, nvt[i], dn[i], to[i], v_up, gamma, gl, last);
    adv[i] = last;
    ret[i] = last + v;
    v_up = v;
  }
}

inline bool misaligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

}  // namespace vret

extern "C" {

int vss_gae(void* stream, int64_t n_steps, int64_t n_rows, const float* rewards, const float* values,
            const float* next_values, const float* term_values, const float* v_last, const float* next_dones,
            const float* next_timeouts, float gamma, float gamma_lambda, float* advantages, float* returns) {
  using vret::misaligned4;
  if (n_steps < 0 || n_rows < 0) return VSS_E_ARG;
  if (!rewards || !values || !next_dones || !next_timeouts || !advantages || !returns) return VSS_E_ARG;
  const bool form_a = next_values != nullptr;
  if ((term_values != nullptr) != (v_last != nullptr)) return VSS_E_ARG;  // one of the pair without the other
  const bool form_b = term_values != nullptr;
  if (form_a == form_b) return VSS_E_ARG;  // both forms, or neither
  if (misaligned4(rewards) || misaligned4(values) || misaligned4(next_values) || misaligned4(term_values) ||
      misaligned4(v_last) || misaligned4(next_dones) || misaligned4(next_timeouts) || misaligned4(advantages) ||
      misaligned4(returns))
    return VSS_E_ARG;
  if (!isfinite(gamma) || !isfinite(gamma_lambda)) return VSS_E_ARG;
  if (n_steps == 0 || n_rows == 0) return VSS_OK;
  const int64_t blocks = n_rows / vret::kWave + (n_rows % vret::kWave != 0);
  // the element index t * E + e stays an int64 byte offset; the grid an unsigned x dimension
  if (blocks > INT32_MAX || n_steps > (INT64_MAX / 4) / n_rows) return VSS_E_ARG;
  const dim3 grid((unsigned)blocks), block(vret::kWave);
  if (form_b)
    hipLaunchKernelGGL((vret::gae_kernel<vret::kUnroll, true>), grid, block, 0, (hipStream_t)stream, n_steps, n_rows,
                       rewards, values, term_values, v_last, next_dones, next_timeouts, gamma, gamma_lambda, advantages,
                       returns);
  else
    hipLaunchKernelGGL((vret::gae_kernel<vret::kUnroll, false>), grid, block, 0, (hipStream_t)stream, n_steps, n_rows,
                       rewards, values, next_values, v_last, next_dones, next_timeouts, gamma, gamma_lambda, advantages,
                       returns);
  return hipGetLastError() == hipSuccess ? VSS_OK : VSS_E_LAUNCH;
}

}  // extern "C"
