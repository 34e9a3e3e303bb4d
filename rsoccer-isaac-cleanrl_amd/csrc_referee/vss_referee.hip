// vss_referee.hip — the referee in one launch (gfx950): vss_referee of include/vss_referee.h.
//
// After the step and the set plays, every field's three counters are advanced -- the steps the ball has been stuck,
// the steps two defenders, and the steps two attackers, have stood in a goal area with the ball -- and a field whose
// counter reaches its threshold is whistled: placed again from the free ball, the penalty or the goal kick of a table
// of three plays, with the mirrorings decided by the verdict, and its dof velocities and observation rows rewritten.
// vss_amd/referee.py reference_referee is the specification -- float32, one operation per line -- and this file
// follows it line by line: + - *, comparisons, selects and integer operations only, no FMA contraction
// (-ffp-contract=off and the pragma below).  The result equals the reference bit for bit (tests/test_referee_gpu.py).
//
//   The placement (anchor + jitter, flip_y, flip_x with the role swap, the yaw wrap, sincos_small) restates
//   csrc_setplay/vss_setplay.hip's, and the observation rows (heading c = qw^2 - qz^2, s = 2 qw qz; the yellow view
//   negated; own slot j = robot (k + j) % 3) restate csrc/vss_step.hip's write_obs_record and gather table: this unit
//   shares a header with neither, whose stamped file lists are closed.  The tests pin both restatements: the placed
//   state to reference_setplay with forced flips, the rows to vss_compute_observations.
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

#include "../../include/vss_referee.h"
#include "../csrc/vss_numerics.h"

#pragma clang fp contract(off)

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "vss_referee.hip targets gfx950 (CDNA4) only"
#endif

namespace vrf {

using namespace vnum;
using namespace vnum::host;

constexpr int kBlock = 256;  // fields per workgroup (four waves)
constexpr int kObs = 52;     // floats per row
constexpr int kQuads = 13;   // 16-B pieces per row
constexpr int kChannels = 58;
constexpr int kDof = 12;     // floats of dof_vel per field
constexpr int kCap = 1 << 30;  // a counter stops counting here
constexpr uint32_t kPurpose = 11u << 24;  // the Philox counter's purpose byte (the step 0..6, the channels 7..9, set plays 10)
constexpr float kPi = 3.1415927f, kTwoPi = 6.2831855f;
// include/vss.h VSS_CH_*
constexpr int kChRX = 4, kChRY = 10, kChRQX = 16, kChRQY = 22, kChRQZ = 28, kChRQW = 34, kChRVX = 40, kChRVY = 46,
              kChRW = 52;

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
  vss_referee_view view[2];
  vss_referee_params prm;
  vss_referee_table tab;
};

// the world of one whistled field: the ball, and per robot (0..2 blue, 3..5 yellow) position and heading
struct World {
  float bx, by, bvx, bvy;
  float x[6], y[6], c[6], s[6];
};

__device__ __forceinline__ float jitter(uint32_t w, float r) {
  float t = 2.0f * u01(w);
  t = t - 1.0f;
  return t * r;
}

// One row: the view of robot I of team T (csrc/vss_step.hip make_obs_table, with zero velocities, yaw rates and
// own-action floats).  Negation is the sign flip, -0.0 for the zeros included.
template <int T, int I>
__device__ __forceinline__ void store_row(float* obs, int64_t row, const World& w) {
  float v[kObs];
  v[0] = T ? -w.bx : w.bx; v[1] = T ? -w.by : w.by; v[2] = T ? -w.bvx : w.bvx; v[3] = T ? -w.bvy : w.bvy;
  const float zero = T ? -0.0f : 0.0f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int r = 3 * T + (I + j) % 3;
    float* o = v + 4 + 9 * j;
    o[0] = T ? -w.x[r] : w.x[r]; o[1] = T ? -w.y[r] : w.y[r]; o[2] = zero; o[3] = zero;
    o[4] = T ? -w.c[r] : w.c[r]; o[5] = T ? -w.s[r] : w.s[r]; o[6] = 0.0f; o[7] = 0.0f; o[8] = 0.0f;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int r = 3 * (1 - T) + j;
    float* o = v + 31 + 7 * j;
    o[0] = T ? -w.x[r] : w.x[r]; o[1] = T ? -w.y[r] : w.y[r]; o[2] = zero; o[3] = zero;
    o[4] = T ? -w.c[r] : w.c[r]; o[5] = T ? -w.s[r] : w.s[r]; o[6] = 0.0f;
  }
  float4* p = reinterpret_cast<float4*>(obs) + row * kQuads;
#pragma unroll
  for (int q = 0; q < kQuads; ++q) p[q] = make_float4(v[4 * q + 0], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

template <int T>
__device__ __forceinline__ void store_team(float* obs, int64_t row, int robots, const World& w) {
  store_row<T, 0>(obs, row, w);
  if (robots == 3) {
    store_row<T, 1>(obs, row + 1, w);
    store_row<T, 2>(obs, row + 2, w);
  }
}

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

    // the ball: block 1, words x y vx vy
    World W;
    {
      uint32_t w[4];
      philox(a.k0, a.k1, c0, a.call, kPurpose, 1u, w);
      float x = ex[0] + jitter(w[0], rp[0]);
      float y = ey[0] + jitter(w[1], rp[0]);
      float vx = pvx + jitter(w[2], rv);
      float vy = pvy + jitter(w[3], rv);
      if (flip_y) { y = -y; vy = -vy; }
      if (flip_x) { x = -x; vx = -vx; }
      W.bx = x; W.by = y; W.bvx = vx; W.bvy = vy;
    }
    // the robots: entity e in block 1 + e, words x y yaw (the fourth is not used)
    float px[6], py[6], qz[6], qw[6];
#pragma unroll
    for (int e = 1; e < 7; ++e) {
      uint32_t w[4];
      philox(a.k0, a.k1, c0, a.call, kPurpose, (uint32_t)(1 + e), w);
      float x = ex[e] + jitter(w[0], rp[e]);
      float y = ey[e] + jitter(w[1], rp[e]);
      float yaw = eyaw[e] + jitter(w[2], ryw[e]);
      if (flip_y) { y = -y; yaw = -yaw; }
      if (flip_x) { x = -x; yaw = kPi - yaw; }
      if (yaw > kPi) yaw = yaw - kTwoPi;
      if (yaw < -kPi) yaw = yaw + kTwoPi;
      float sz, cw;
      sincos_small(0.5f * yaw, sz, cw);
      px[e - 1] = x; py[e - 1] = y; qz[e - 1] = sz; qw[e - 1] = cw;
    }
    // flip_x is the role swap: blue i takes yellow i's placement and vice versa
    float rqz[6], rqw[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const int o = (r + 3) % 6;
      W.x[r] = flip_x ? px[o] : px[r];
      W.y[r] = flip_x ? py[o] : py[r];
      rqz[r] = flip_x ? qz[o] : qz[r];
      rqw[r] = flip_x ? qw[o] : qw[r];
      W.c[r] = rqw[r] * rqw[r] - rqz[r] * rqz[r];
      W.s[r] = 2.0f * rqw[r] * rqz[r];
    }

    // ---- the state: 58 strided 4-B stores (whistled implies f < n) ----
    float* s = a.state + f;
    s[0 * n] = W.bx; s[1 * n] = W.by; s[2 * n] = W.bvx; s[3 * n] = W.bvy;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      s[(kChRX + r) * n] = W.x[r];
      s[(kChRY + r) * n] = W.y[r];
      s[(kChRQX + r) * n] = 0.0f;
      s[(kChRQY + r) * n] = 0.0f;
      s[(kChRQZ + r) * n] = rqz[r];
      s[(kChRQW + r) * n] = rqw[r];
      s[(kChRVX + r) * n] = 0.0f;
      s[(kChRVY + r) * n] = 0.0f;
      s[(kChRW + r) * n] = 0.0f;
    }
    static_assert(kChRW + 6 == kChannels, "the state has 58 channels");

    // ---- the dof velocities: twelve floats, three 16-B stores ----
    float4* d = reinterpret_cast<float4*>(a.dof_vel) + f * (kDof / 4);
    d[0] = d[1] = d[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

    // ---- the rows: 16-B stores, view by view ----
#pragma unroll 1
    for (int v = 0; v < a.n_views; ++v) {
      const vss_referee_view& vw = a.view[v];
#pragma unroll 1
      for (int b = 0; b < vw.n_teams; ++b) {
        const int64_t row = (int64_t)b * vw.team_stride + f * vw.field_stride;
        if (vw.first_team + b == 0) store_team<0>(vw.obs, row, vw.robots, W);
        else store_team<1>(vw.obs, row, vw.robots, W);
      }
    }
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
    if (!isfinite(p.ball_vx) || !isfinite(p.ball_vy) || !(p.r_vel >= 0.0f) || !isfinite(p.r_vel)) return false;
    for (int e = 0; e < 7; ++e) {
      const vss_referee_entity& q = p.e[e];
      if (!isfinite(q.x) || !isfinite(q.y) || !isfinite(q.yaw) || !isfinite(q.r_pos) || !isfinite(q.r_yaw)) return false;
      if (q.r_pos < 0.0f) return false;
      if (fabsf(q.yaw) > kPi || q.r_yaw < 0.0f || q.r_yaw > kPi) return false;  // pi as the float32 the kernel uses
      const double hx = e == 0 ? 0.75 : 0.71, hy = e == 0 ? 0.65 : 0.61;
      if (fabs((double)q.x) + (double)q.r_pos > hx || fabs((double)q.y) + (double)q.r_pos > hy) return false;
      for (int j = 0; j < e; ++j) {
        const vss_referee_entity& o = p.e[j];
        const double dx = (double)q.x - (double)o.x, dy = (double)q.y - (double)o.y;
        const double gap = sqrt(dx * dx + dy * dy) - 1.4142135623730951 * ((double)q.r_pos + (double)o.r_pos);
        if (gap < 0.08) return false;
      }
    }
    // a free ball or a penalty whose ball can lie inside a goal area would be whistled again
    const vss_referee_entity& b = p.e[0];
    if (k < 2 && fabs((double)b.x) + (double)b.r_pos > (double)prm->area_x &&
        fabs((double)b.y) - (double)b.r_pos < (double)prm->area_y)
      return false;
  }
  return true;
}

}  // namespace vrf

extern "C" {

int vss_referee_abi_version(void) { return VSS_REFEREE_ABI_VERSION; }

int vss_referee(void* stream, int64_t n_fields, const vss_referee_table* tab, const vss_referee_params* prm,
                uint64_t seed, uint32_t call, const int64_t* done, int64_t done_stride, float* state, float* dof_vel,
                int32_t* counters, int32_t n_views, const vss_referee_view* views, int64_t* counts, int32_t* verdict) {
  using namespace vrf;
  if (!tab || !prm || !state || !dof_vel || !counters) return VSS_REFEREE_E_ARG;
  if (n_views < 0 || n_views > 2 || (n_views > 0 && !views)) return VSS_REFEREE_E_ARG;
  if (!params_ok(prm) || !table_ok(tab, prm)) return VSS_REFEREE_E_ARG;
  if (misaligned(state, 4) || misaligned(verdict, 4) || misaligned(done, 8) || misaligned(counts, 8) ||
      misaligned(dof_vel, 16) || misaligned(counters, 16))
    return VSS_REFEREE_E_ARG;
  if (n_fields < 0 || (done && done_stride < 1)) return VSS_REFEREE_E_ARG;
  for (int v = 0; v < n_views; ++v) {
    const vss_referee_view& w = views[v];
    if (!w.obs || misaligned(w.obs, 16)) return VSS_REFEREE_E_ARG;
    if ((w.robots != 1 && w.robots != 3) || (w.n_teams != 1 && w.n_teams != 2)) return VSS_REFEREE_E_ARG;
    if (w.first_team < 0 || w.first_team > 2 - w.n_teams) return VSS_REFEREE_E_ARG;  // n_teams is 1 or 2 here
    if (w.field_stride < w.robots) return VSS_REFEREE_E_ARG;
  }
  constexpr int kOuts = 7;
  const void* outs[kOuts] = {state, dof_vel, counters, counts, verdict, n_views > 0 ? views[0].obs : nullptr,
                             n_views > 1 ? views[1].obs : nullptr};
  // the pointer-equality part of the aliasing rule holds at any size
  for (int i = 0; i < kOuts; ++i) {
    if (!outs[i]) continue;
    if (outs[i] == (const void*)done) return VSS_REFEREE_E_ARG;
    for (int j = i + 1; j < kOuts; ++j)
      if (outs[i] == outs[j]) return VSS_REFEREE_E_ARG;
  }
  if (n_fields == 0) return VSS_REFEREE_OK;

  // sizes: the grid is an unsigned x dimension; every byte offset stays an int64 (208 B per row, 58 x 4 B per field)
  const int64_t kMaxRows = INT64_MAX / (4 * kObs) / 8;
  const int64_t m = n_fields - 1;
  if (n_fields > kMaxRows / 6 || (done && done_stride > (INT64_MAX / 8) / n_fields)) return VSS_REFEREE_E_ARG;
  const int64_t blocks = n_fields / kBlock + (n_fields % kBlock != 0);
  if (blocks > INT32_MAX) return VSS_REFEREE_E_ARG;
  uint64_t span[2] = {0, 0};
  for (int v = 0; v < n_views; ++v) {
    const vss_referee_view& w = views[v];
    if (w.field_stride > kMaxRows / n_fields) return VSS_REFEREE_E_ARG;
    const int64_t block_rows = m * w.field_stride + w.robots;  // rows one team block spans
    // two teams: block after block, or both inside one field stride (FULL's (N, 2, 3, 52))
    if (w.n_teams == 2 && (w.team_stride < w.robots || w.team_stride > kMaxRows - block_rows ||
                           (w.team_stride < block_rows && w.team_stride + w.robots > w.field_stride)))
      return VSS_REFEREE_E_ARG;
    span[v] = (uint64_t)((w.n_teams == 2 ? w.team_stride : 0) + block_rows) * kObs * 4;
  }
  // an output overlapping done or another output
  const uint64_t out_b[kOuts] = {(uint64_t)n_fields * kChannels * 4, (uint64_t)n_fields * kDof * 4, (uint64_t)n_fields * 16,
                                 (uint64_t)VSS_REFEREE_CODES * 8, (uint64_t)n_fields * 4, span[0], span[1]};
  const uint64_t done_b = done ? (uint64_t)(m * done_stride + 1) * 8 : 0;
  for (int i = 0; i < kOuts; ++i) {
    if (overlap(outs[i], out_b[i], done, done_b)) return VSS_REFEREE_E_ARG;
    for (int j = i + 1; j < kOuts; ++j)
      if (overlap(outs[i], out_b[i], outs[j], out_b[j])) return VSS_REFEREE_E_ARG;
  }

  Args a;
  a.n = n_fields; a.done_stride = done ? done_stride : 0;
  a.k0 = (uint32_t)(seed & 0xFFFFFFFFu); a.k1 = (uint32_t)(seed >> 32); a.call = call;
  a.n_views = n_views; a.done = done; a.state = state; a.dof_vel = dof_vel; a.counters = counters;
  a.counts = reinterpret_cast<unsigned long long*>(counts); a.verdict = verdict;
  for (int v = 0; v < 2; ++v) {
    if (v < n_views) a.view[v] = views[v];
    else a.view[v] = vss_referee_view{nullptr, 0, 0, 1, 1, 0};
    if (a.view[v].n_teams != 2) a.view[v].team_stride = 0;
  }
  a.prm = *prm;
  a.tab = *tab;
  const dim3 grid((unsigned)blocks), block(kBlock);
  hipLaunchKernelGGL(referee_kernel, grid, block, 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? VSS_REFEREE_OK : VSS_REFEREE_E_LAUNCH;
}

}  // extern "C"
