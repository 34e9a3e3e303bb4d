// vss_setplay.hip — the set plays in one launch (gfx950): vss_setplay of include/vss.h.
//
// After the step has reset the fields that finished (a uniform drop, envs/vss.py:267-333), a share of them is placed
// again from a table of named plays -- anchor + uniform jitter per entity, then the two mirrorings -- and their
// observation rows are rewritten from the new state.  vss_amd/setplay.py reference_setplay is the specification --
// float32, one operation per line -- and this file follows it line by line: + - *, comparisons, selects and integer
// operations only, no FMA contraction (-ffp-contract=off and the pragma below).  The result equals the reference
// bit for bit (tests/test_setplay_gpu.py).
//
//   The placement of a field from its play's registers, the stores of its state and rows and the entry's checks of a
//   play, the views and the outputs are vss_placement.h's, shared with vss_referee.hip; what is the set plays' own is
//   here: the draw of the share, the play and the two flips, the purpose byte, the counts and the table's weights.
//   (The rows restate vss_step.hip's write_obs_record, which stays on the hot path: see vss_placement.h.)
//
//   one field per lane, no LDS.  In a normal step about one field in 400 is done, so a lane loads its done flag
//   first and a wave without a done lane stores its chosen = -1 and leaves before any Philox round.
//
//   The table travels in the kernel arguments.  A lane's play is picked by a loop over `count` whose index is
//   uniform (scalar loads of the table, selects into registers): no register array is indexed at run time.
//
//   counts follows vss_match_tally: a wave adds its staged lanes up per play (ballot, popcount) and lane 0 issues
//   the 64-bit atomicAdds -- integer sums, exact in any order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vss.h"
#include "vss_numerics.h"
#include "vss_placement.h"

#pragma clang fp contract(off)

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "vss_setplay.hip targets gfx950 (CDNA4) only"
#endif

namespace vsp {

using namespace vnum;
using namespace vplace;
using namespace vplace::host;

constexpr int kBlock = 256;  // fields per workgroup (four waves)
constexpr uint32_t kPurpose = 10u << 24;  // the Philox counter's purpose byte (the step 0..6, the channels 7..9)

struct Args {
  int64_t n, done_stride;
  uint32_t k0, k1, call;
  int32_t n_views;
  const int64_t* done;
  float* state;
  unsigned long long* counts;
  int32_t* chosen;
  vss_setplay_view view[2];
  vss_setplay_table tab;
};

__global__ __launch_bounds__(kBlock) void setplay_kernel(const Args a) {
  const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool in = f < a.n;
  const bool done = in && (a.done == nullptr || a.done[f * a.done_stride] != 0);
  if (__ballot(done) == 0ull) {  // uniform over the wave: nothing to stage
    if (in && a.chosen) a.chosen[f] = -1;
    return;
  }
  const int count = a.tab.count;
  const uint32_t c0 = (uint32_t)f;
  bool staged = false;
  int sel = -1;
  uint32_t w0[4] = {0u, 0u, 0u, 0u};
  if (done) {
    philox(a.k0, a.k1, c0, a.call, kPurpose, 0u, w0);
    staged = u01(w0[0]) < a.tab.share;
  }
  if (staged) {
    const float up = u01(w0[1]) * a.tab.total_weight;
    sel = count - 1;
    for (int k = count - 2; k >= 0; --k)  // the first k with up < cum_weight[k]
      if (up < a.tab.play[k].cum_weight) sel = k;

    // the lane's play, by selects under a uniform index
    float ex[7], ey[7], eyaw[7], rp[7], ryw[7];
    float pvx = 0.0f, pvy = 0.0f, rv = 0.0f, pfx = 0.0f, pfy = 0.0f;
#pragma unroll
    for (int e = 0; e < 7; ++e) ex[e] = ey[e] = eyaw[e] = rp[e] = ryw[e] = 0.0f;
#pragma unroll 1
    for (int k = 0; k < count; ++k) {
      const vss_setplay_play& P = a.tab.play[k];
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
      pfx = mine ? P.p_flip_x : pfx;
      pfy = mine ? P.p_flip_y : pfy;
    }
    const bool flip_x = u01(w0[2]) < pfx;
    const bool flip_y = u01(w0[3]) < pfy;

    World W;
    float rqz[6], rqw[6];
    place_field(ex, ey, eyaw, rp, ryw, pvx, pvy, rv, flip_x, flip_y, a.k0, a.k1, c0, a.call, kPurpose, W, rqz, rqw);
    store_state(a.state, a.n, f, W, rqz, rqw);
    store_views(a.view, a.n_views, f, W);
  }
  if (in && a.chosen) a.chosen[f] = sel;  // -1 unless staged
  if (a.counts) {
    for (int k = 0; k < count; ++k) {  // uniform
      const unsigned long long m = __ballot(staged && sel == k);
      if (m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(a.counts + k, (unsigned long long)__popcll(m));
    }
  }
}

// ---- the entry's checks (host) ---------------------------------------------------------------------------------------
inline bool unit_ok(float p) { return p >= 0.0f && p <= 1.0f; }  // false for a NaN

// vss_amd/setplay.py Table.validate, rule by rule, in double on the table's float32 values
inline bool table_ok(const vss_setplay_table* t) {
  if (t->count < 1 || t->count > VSS_SETPLAY_MAX_PLAYS) return false;
  if (!unit_ok(t->share)) return false;
  float prev = 0.0f;
  for (int k = 0; k < t->count; ++k) {
    const vss_setplay_play& p = t->play[k];
    if (!(p.cum_weight >= prev) || !(p.cum_weight <= 3.4028235e38f)) return false;  // decreasing, negative, NaN, inf
    prev = p.cum_weight;
    if (!unit_ok(p.p_flip_x) || !unit_ok(p.p_flip_y)) return false;
    if (!play_ok(p.e, p.ball_vx, p.ball_vy, p.r_vel)) return false;
  }
  if (!(prev > 0.0f) || t->total_weight != prev) return false;
  return true;
}

}  // namespace vsp

extern "C" {

int vss_setplay(void* stream, int64_t n_fields, const vss_setplay_table* tab, uint64_t seed, uint32_t call,
                const int64_t* done, int64_t done_stride, float* state, int32_t n_views, const vss_setplay_view* views,
                int64_t* counts, int32_t* chosen) {
  using namespace vsp;
  if (!tab || !state) return VSS_E_ARG;
  if (!views_ok(n_views, views)) return VSS_E_ARG;
  if (!table_ok(tab)) return VSS_E_ARG;
  if (misaligned(state, 4) || misaligned(chosen, 4) || misaligned(done, 8) || misaligned(counts, 8)) return VSS_E_ARG;
  if (n_fields < 0 || (done && done_stride < 1)) return VSS_E_ARG;
  const void* outs[5] = {state, counts, chosen, n_views > 0 ? views[0].obs : nullptr, n_views > 1 ? views[1].obs : nullptr};
  if (outputs_alias(outs, 5, done)) return VSS_E_ARG;
  if (n_fields == 0) return VSS_OK;

  int64_t blocks;
  uint64_t span[2];
  if (!grid_ok(n_fields, kBlock, done, done_stride, blocks) || !view_spans(n_fields, n_views, views, span))
    return VSS_E_ARG;
  const uint64_t out_b[5] = {(uint64_t)n_fields * kChannels * 4, (uint64_t)VSS_SETPLAY_MAX_PLAYS * 8,
                             (uint64_t)n_fields * 4, span[0], span[1]};
  const uint64_t done_b = done ? (uint64_t)((n_fields - 1) * done_stride + 1) * 8 : 0;
  if (outputs_overlap(outs, out_b, 5, done, done_b)) return VSS_E_ARG;

  Args a;
  a.n = n_fields; a.done_stride = done ? done_stride : 0;
  a.k0 = (uint32_t)(seed & 0xFFFFFFFFu); a.k1 = (uint32_t)(seed >> 32); a.call = call;
  a.n_views = n_views; a.done = done; a.state = state;
  a.counts = reinterpret_cast<unsigned long long*>(counts); a.chosen = chosen;
  fill_views(a.view, n_views, views);
  a.tab = *tab;
  const dim3 grid((unsigned)blocks), block(kBlock);
  hipLaunchKernelGGL(setplay_kernel, grid, block, 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? VSS_OK : VSS_E_LAUNCH;
}

}  // extern "C"
