// vss_referee.hip — the referee in one launch (gfx950): vss_referee of include/vss.h.
//
// After the step and the set plays, every field's three counters are advanced -- the steps the ball has been stuck,
// the steps two defenders, and the steps two attackers, have stood in a goal area with the ball -- and a field whose
// counter reaches its threshold is whistled: placed again from the free ball, the penalty or the goal kick of a table
// of three plays, with the mirrorings decided by the verdict, and its dof velocities and observation rows rewritten.
// vss_amd/referee.py reference_referee is the specification -- float32, one operation per line -- and this file
// follows it line by line: + - *, comparisons, selects and integer operations only, no FMA contraction
// (-ffp-contract=off and the pragma below).  The result equals the reference bit for bit (tests/test_referee_gpu.py).
//
//   The placement of a field from its play's registers, the stores of its state and rows and the entry's checks of a
//   play, the views and the outputs are vss_placement.h's, shared with vss_setplay.hip; what is the referee's own is
//   here: the detection and the counters, the flips decided by the verdict, the purpose byte, the dof velocities, the
//   counts and the parameters' rules.  The tests still pin the placed state to reference_setplay with forced flips and
//   the rows to vss_compute_observations (they restate vss_step.hip's write_obs_record: see vss_placement.h).
//
//   one field per lane, no LDS.  A lane loads its done flag, its counters (one 16-B load) and 16 coalesced state
//   channels (the ball's four, the robots' x and y); the detection is a few dozen compares; every lane stores its
//   counters (one 16-B store) and its verdict.  Hardly any field is whistled in a step, so a wave without a whistled
//   lane leaves there, before any Philox round.
//
//   The table and the parameters travel in the kernel arguments.  A whistled lane's play is picked by a loop over the
//   three plays whose index is uniform (scalar loads of the table, selects into registers): no register array is
//   indexed at run time.
//
//   counts follows vss_setplay: a wave adds its whistled lanes up per code (ballot, popcount) and lane 0 issues the
//   64-bit atomicAdds -- integer sums, exact in any order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vss.h"
#include "vss_numerics.h"
#include "vss_placement.h"

#pragma clang fp contract(off)

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "vss_referee.hip targets gfx950 (CDNA4) only"
#endif

namespace vrf {

using namespace vnum;
using namespace vplace;
using namespace vplace::host;

constexpr int kBlock = 256;  // fields per workgroup (four waves)
constexpr int kDof = 12;     // floats of dof_vel per field
constexpr int kCap = 1 << 30;  // a counter stops counting here
constexpr uint32_t kPurpose = 11u << 24;  // the Philox counter's purpose byte (the step 0..6, the channels 7..9, set plays 10)

struct Args {
  int64_t n, done_stride;
  uint32_t k0, k1, call;
  int32_t n_views;
  const int64_t* done;
  float* state;
  float* dof_vel;
  int32_t* counters;
  unsigned long long* counts;
  int32_t* verdict;
  vss_setplay_view view[2];
  vss_referee_params prm;
  vss_referee_table tab;
};

__device__ __forceinline__ int bump(bool holds, int c) { return holds ? (c + 1 < kCap ? c + 1 : kCap) : 0; }

__global__ __launch_bounds__(kBlock) void referee_kernel(const Args a) {
  const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool in = f < a.n;
  const int64_t n = a.n;
  const bool done = in && a.done != nullptr && a.done[f * a.done_stride] != 0;
  int4* cnt = reinterpret_cast<int4*>(a.counters);
  int4 c = make_int4(0, 0, 0, 0);
  float bx = 0.0f, by = 0.0f, bvx = 0.0f, bvy = 0.0f, rx[6], ry[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) rx[r] = ry[r] = 0.0f;
  if (in) {
    c = cnt[f];
    const float* s = a.state + f;
    bx = s[0 * n]; by = s[1 * n]; bvx = s[2 * n]; bvy = s[3 * n];
#pragma unroll
    for (int r = 0; r < 6; ++r) { rx[r] = s[(kChRX + r) * n]; ry[r] = s[(kChRY + r) * n]; }
  }

  // ---- the detection ----
  const vss_referee_params& p = a.prm;
  float v2 = bvx * bvx;
  v2 = v2 + bvy * bvy;
  const bool left = bx < 0.0f, low = by < 0.0f;
  const bool in_area = fabsf(bx) > p.area_x && fabsf(by) < p.area_y;
  int nb = 0, ny = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const bool inside = fabsf(rx[r]) > p.area_x && fabsf(ry[r]) < p.area_y && (rx[r] < 0.0f) == left;
    if (r < 3) nb += inside ? 1 : 0;
    else ny += inside ? 1 : 0;
  }
  const int def_n = left ? nb : ny, att_n = left ? ny : nb;  // side 0 (bx < 0) is blue's own area
  int stall = bump(v2 < p.stall_speed_sq, c.x);
  int defend = bump(in_area && def_n >= 2, c.y);
  int attack = bump(in_area && att_n >= 2, c.z);
  int stops = c.w;
  int code = -1;
  if (p.max_stops == 0 || stops < p.max_stops) {
    if (p.area_steps > 0 && defend >= p.area_steps) code = left ? 5 : 4;
    else if (p.area_steps > 0 && attack >= p.area_steps) code = left ? 6 : 7;
    else if (p.stall_steps > 0 && stall >= p.stall_steps) code = (left ? 2 : 0) + (low ? 1 : 0);
  }
  if (done) { stall = defend = attack = stops = 0; code = -1; }
  const bool whistled = in && code >= 0;
  if (whistled) { stall = defend = attack = 0; stops = stops + 1; }
  if (in) {
    cnt[f] = make_int4(stall, defend, attack, stops);
    if (a.verdict) a.verdict[f] = code;
  }
  if (__ballot(whistled) == 0ull) return;  // uniform over the wave: the normal case, no Philox round

  if (whistled) {
    const int sel = code < 4 ? 0 : (code < 6 ? 1 : 2);
    const bool flip_x = code < 4 ? left : (code == 5 || code == 7);
    const bool flip_y = sel == 1 ? false : low;
    const uint32_t c0 = (uint32_t)f;

    // the lane's play, by selects under a uniform index
    float ex[7], ey[7], eyaw[7], rp[7], ryw[7];
    float pvx = 0.0f, pvy = 0.0f, rv = 0.0f;
#pragma unroll
    for (int e = 0; e < 7; ++e) ex[e] = ey[e] = eyaw[e] = rp[e] = ryw[e] = 0.0f;
#pragma unroll 1
    for (int k = 0; k < VSS_REFEREE_PLAYS; ++k) {
      const vss_referee_play& P = a.tab.play[k];
      const bool mine = sel == k;
#pragma unroll
      for (int e = 0; e < 7; ++e) {
        ex[e] = mine ? P.e[e].x : ex[e];
        ey[e] = mine ? P.e[e].y : ey[e];
        eyaw[e] = mine ? P.e[e].yaw : eyaw[e];
        rp[e] = mine ? P.e[e].r_pos : rp[e];
        ryw[e] = mine ? P.e[e].r_yaw : ryw[e];
      }
      pvx = mine ? P.ball_vx : pvx;
      pvy = mine ? P.ball_vy : pvy;
      rv = mine ? P.r_vel : rv;
    }

    World W;
    float rqz[6], rqw[6];
    place_field(ex, ey, eyaw, rp, ryw, pvx, pvy, rv, flip_x, flip_y, a.k0, a.k1, c0, a.call, kPurpose, W, rqz, rqw);
    store_state(a.state, n, f, W, rqz, rqw);  // whistled implies f < n

    // ---- the dof velocities: twelve floats, three 16-B stores ----
    float4* d = reinterpret_cast<float4*>(a.dof_vel) + f * (kDof / 4);
    d[0] = d[1] = d[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

    store_views(a.view, a.n_views, f, W);
  }
  if (a.counts) {
    for (int k = 0; k < VSS_REFEREE_CODES; ++k) {  // uniform
      const unsigned long long m = __ballot(whistled && code == k);
      if (m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(a.counts + k, (unsigned long long)__popcll(m));
    }
  }
}

// ---- the entry's checks (host) ---------------------------------------------------------------------------------------
// vss_amd/referee.py Params.validate
inline bool params_ok(const vss_referee_params* p) {
  if (p->stall_steps < 0 || p->area_steps < 0 || p->max_stops < 0) return false;
  if (!(p->stall_speed_sq >= 0.0f) || !isfinite(p->stall_speed_sq)) return false;
  if (!((double)p->area_x > 0.0 && (double)p->area_x < 0.75)) return false;
  if (!((double)p->area_y > 0.0 && (double)p->area_y <= 0.65)) return false;
  return true;
}

// vss_amd/referee.py RefTable.validate, rule by rule, in double on the table's float32 values
inline bool table_ok(const vss_referee_table* t, const vss_referee_params* prm) {
  for (int k = 0; k < VSS_REFEREE_PLAYS; ++k) {
    const vss_referee_play& p = t->play[k];
    if (!play_ok(p.e, p.ball_vx, p.ball_vy, p.r_vel)) return false;
    // a free ball or a penalty whose ball can lie inside a goal area would be whistled again
    const vss_setplay_entity& b = p.e[0];
    if (k < 2 && fabs((double)b.x) + (double)b.r_pos > (double)prm->area_x &&
        fabs((double)b.y) - (double)b.r_pos < (double)prm->area_y)
      return false;
  }
  return true;
}

}  // namespace vrf

extern "C" {

int vss_referee(void* stream, int64_t n_fields, const vss_referee_table* tab, const vss_referee_params* prm,
                uint64_t seed, uint32_t call, const int64_t* done, int64_t done_stride, float* state, float* dof_vel,
                int32_t* counters, int32_t n_views, const vss_setplay_view* views, int64_t* counts, int32_t* verdict) {
  using namespace vrf;
  if (!tab || !prm || !state || !dof_vel || !counters) return VSS_E_ARG;
  if (!views_ok(n_views, views)) return VSS_E_ARG;
  if (!params_ok(prm) || !table_ok(tab, prm)) return VSS_E_ARG;
  if (misaligned(state, 4) || misaligned(verdict, 4) || misaligned(done, 8) || misaligned(counts, 8) ||
      misaligned(dof_vel, 16) || misaligned(counters, 16))
    return VSS_E_ARG;
  if (n_fields < 0 || (done && done_stride < 1)) return VSS_E_ARG;
  constexpr int kOuts = 7;
  const void* outs[kOuts] = {state, dof_vel, counters, counts, verdict, n_views > 0 ? views[0].obs : nullptr,
                             n_views > 1 ? views[1].obs : nullptr};
  if (outputs_alias(outs, kOuts, done)) return VSS_E_ARG;
  if (n_fields == 0) return VSS_OK;

  int64_t blocks;
  uint64_t span[2];
  if (!grid_ok(n_fields, kBlock, done, done_stride, blocks) || !view_spans(n_fields, n_views, views, span))
    return VSS_E_ARG;
  const uint64_t out_b[kOuts] = {(uint64_t)n_fields * kChannels * 4, (uint64_t)n_fields * kDof * 4, (uint64_t)n_fields * 16,
                                 (uint64_t)VSS_REFEREE_CODES * 8, (uint64_t)n_fields * 4, span[0], span[1]};
  const uint64_t done_b = done ? (uint64_t)((n_fields - 1) * done_stride + 1) * 8 : 0;
  if (outputs_overlap(outs, out_b, kOuts, done, done_b)) return VSS_E_ARG;

  Args a;
  a.n = n_fields; a.done_stride = done ? done_stride : 0;
  a.k0 = (uint32_t)(seed & 0xFFFFFFFFu); a.k1 = (uint32_t)(seed >> 32); a.call = call;
  a.n_views = n_views; a.done = done; a.state = state; a.dof_vel = dof_vel; a.counters = counters;
  a.counts = reinterpret_cast<unsigned long long*>(counts); a.verdict = verdict;
  fill_views(a.view, n_views, views);
  a.prm = *prm;
  a.tab = *tab;
  const dim3 grid((unsigned)blocks), block(kBlock);
  hipLaunchKernelGGL(referee_kernel, grid, block, 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? VSS_OK : VSS_E_LAUNCH;
}

}  // extern "C"
