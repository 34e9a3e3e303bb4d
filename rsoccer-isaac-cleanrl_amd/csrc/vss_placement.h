// vss_placement.h — the one definition of what the set plays and the referee share: the placement of a field from a
// play, the stores of its state and observation rows, and the entries' checks of a play, the views and the outputs.
//
// vss_setplay.hip and vss_referee.hip include this file.  What differs stays with each: how the play and the two flips
// are chosen (drawn, or decided by the verdict), the Philox purpose byte, the counts ballots, the referee's detection,
// counters and dof velocities, and each entry's own null and alignment list.  vss_amd/setplay.py reference_setplay
// and vss_amd/referee.py reference_referee are the specification -- float32, one operation per line -- and the
// functions below follow them line by line: + - *, comparisons, selects and integer operations only, no FMA
// contraction (the pragma below, and -ffp-contract=off on both units).  An edit here changes both units at once, and
// the library's source stamp (this file is on the Makefile's STAMPED line).
//
//   The observation rows (heading c = qw^2 - qz^2, s = 2 qw qz; the yellow view negated; own slot j = robot
//   (k + j) % 3) restate vss_step.hip's write_obs_record and gather table on purpose: that writer is on the hot path,
//   fused with the step's physics and its store policies, and is not shared.  tests/test_setplay_gpu.py and
//   tests/test_referee_gpu.py pin the rows here to vss_compute_observations.
//
// A unit pulls the device functions in with `using namespace vplace;` inside its own namespace and the host checks
// with `using namespace vplace::host;`, as with vss_numerics.h.
#ifndef VSS_PLACEMENT_H
#define VSS_PLACEMENT_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vss.h"
#include "vss_numerics.h"

#pragma clang fp contract(off)

namespace vplace {

using namespace vnum;

constexpr int kObs = 52;     // floats per row
constexpr int kQuads = 13;   // 16-B pieces per row
constexpr int kChannels = VSS_STATE_CHANNELS;
constexpr float kPi = 3.1415927f, kTwoPi = 6.2831855f;
constexpr int kChRX = VSS_CH_RX, kChRY = VSS_CH_RY, kChRQX = VSS_CH_RQX, kChRQY = VSS_CH_RQY, kChRQZ = VSS_CH_RQZ,
              kChRQW = VSS_CH_RQW, kChRVX = VSS_CH_RVX, kChRVY = VSS_CH_RVY, kChRW = VSS_CH_RW;

// the world of one placed field: the ball, and per robot (0..2 blue, 3..5 yellow) position and heading
struct World {
  float bx, by, bvx, bvy;
  float x[6], y[6], c[6], s[6];
};

__device__ __forceinline__ float jitter(uint32_t w, float r) {
  float t = 2.0f * u01(w);
  t = t - 1.0f;
  return t * r;
}

// One field from its play's registers (anchors ex ey eyaw, jitter half-widths rp ryw, the ball's velocity pvx pvy and
// its jitter rv), the two flips and the draws of key (k0, k1), counter (c0, call, purpose, block): the world, and the
// robots' quaternion z and w for the state.
__device__ __forceinline__ void place_field(const float (&ex)[7], const float (&ey)[7], const float (&eyaw)[7],
                                            const float (&rp)[7], const float (&ryw)[7], float pvx, float pvy, float rv,
                                            bool flip_x, bool flip_y, uint32_t k0, uint32_t k1, uint32_t c0,
                                            uint32_t call, uint32_t purpose, World& W, float (&rqz)[6], float (&rqw)[6]) {
  // the ball: block 1, words x y vx vy
  {
    uint32_t w[4];
    philox(k0, k1, c0, call, purpose, 1u, w);
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
    philox(k0, k1, c0, call, purpose, (uint32_t)(1 + e), w);
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
}

// the state of field f of n: 58 strided 4-B stores
__device__ __forceinline__ void store_state(float* state, int64_t n, int64_t f, const World& W, const float (&rqz)[6],
                                            const float (&rqw)[6]) {
  float* s = state + f;
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
}

// One row: the view of robot I of team T (vss_step.hip make_obs_table, with zero velocities, yaw rates and
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

// the rows of field f: 16-B stores, view by view
__device__ __forceinline__ void store_views(const vss_setplay_view (&view)[2], int32_t n_views, int64_t f,
                                            const World& W) {
#pragma unroll 1
  for (int v = 0; v < n_views; ++v) {
    const vss_setplay_view& vw = view[v];
#pragma unroll 1
    for (int b = 0; b < vw.n_teams; ++b) {
      const int64_t row = (int64_t)b * vw.team_stride + f * vw.field_stride;
      if (vw.first_team + b == 0) store_team<0>(vw.obs, row, vw.robots, W);
      else store_team<1>(vw.obs, row, vw.robots, W);
    }
  }
}

// ---- the entries' checks (host) --------------------------------------------------------------------------------------
namespace host {

using namespace vnum::host;

// the rules of one play that vss_amd/setplay.py Table.validate and vss_amd/referee.py RefTable.validate share, rule by
// rule, in double on the play's float32 values
inline bool play_ok(const vss_setplay_entity (&e)[7], float ball_vx, float ball_vy, float r_vel) {
  if (!isfinite(ball_vx) || !isfinite(ball_vy) || !(r_vel >= 0.0f) || !isfinite(r_vel)) return false;
  for (int i = 0; i < 7; ++i) {
    const vss_setplay_entity& q = e[i];
    if (!isfinite(q.x) || !isfinite(q.y) || !isfinite(q.yaw) || !isfinite(q.r_pos) || !isfinite(q.r_yaw)) return false;
    if (q.r_pos < 0.0f) return false;
    if (fabsf(q.yaw) > kPi || q.r_yaw < 0.0f || q.r_yaw > kPi) return false;  // pi as the float32 the kernel uses
    const double hx = i == 0 ? 0.75 : 0.71, hy = i == 0 ? 0.65 : 0.61;
    if (fabs((double)q.x) + (double)q.r_pos > hx || fabs((double)q.y) + (double)q.r_pos > hy) return false;
    for (int j = 0; j < i; ++j) {
      const vss_setplay_entity& o = e[j];
      const double dx = (double)q.x - (double)o.x, dy = (double)q.y - (double)o.y;
      const double gap = sqrt(dx * dx + dy * dy) - 1.4142135623730951 * ((double)q.r_pos + (double)o.r_pos);
      if (gap < 0.08) return false;
    }
  }
  return true;
}

// n_views in 0..2 and every view's own fields (sizes apart: view_spans)
inline bool views_ok(int32_t n_views, const vss_setplay_view* views) {
  if (n_views < 0 || n_views > 2 || (n_views > 0 && !views)) return false;
  for (int v = 0; v < n_views; ++v) {
    const vss_setplay_view& w = views[v];
    if (!w.obs || misaligned(w.obs, 16)) return false;
    if ((w.robots != 1 && w.robots != 3) || (w.n_teams != 1 && w.n_teams != 2)) return false;
    if (w.first_team < 0 || w.first_team > 2 - w.n_teams) return false;  // n_teams is 1 or 2 here
    if (w.field_stride < w.robots) return false;
  }
  return true;
}

// sizes: the grid is an unsigned x dimension; every byte offset stays an int64 (208 B per row, 58 x 4 B per field)
constexpr int64_t kMaxRows = INT64_MAX / (4 * kObs) / 8;

// n_fields >= 1 fields in workgroups of `block`: the grid's size, or false where it or done's offsets overflow
inline bool grid_ok(int64_t n_fields, int block, const int64_t* done, int64_t done_stride, int64_t& blocks) {
  if (n_fields > kMaxRows / 6 || (done && done_stride > (INT64_MAX / 8) / n_fields)) return false;
  blocks = n_fields / block + (n_fields % block != 0);
  return blocks <= INT32_MAX;
}

// the bytes every view's rows span over n_fields >= 1 fields, or false where they overflow or two teams' blocks overlap
inline bool view_spans(int64_t n_fields, int32_t n_views, const vss_setplay_view* views, uint64_t (&span)[2]) {
  const int64_t m = n_fields - 1;
  span[0] = span[1] = 0;
  for (int v = 0; v < n_views; ++v) {
    const vss_setplay_view& w = views[v];
    if (w.field_stride > kMaxRows / n_fields) return false;
    const int64_t block_rows = m * w.field_stride + w.robots;  // rows one team block spans
    // two teams: block after block, or both inside one field stride (FULL's (N, 2, 3, 52))
    if (w.n_teams == 2 && (w.team_stride < w.robots || w.team_stride > kMaxRows - block_rows ||
                           (w.team_stride < block_rows && w.team_stride + w.robots > w.field_stride)))
      return false;
    span[v] = (uint64_t)((w.n_teams == 2 ? w.team_stride : 0) + block_rows) * kObs * 4;
  }
  return true;
}

// an output that is done or another output: the pointer-equality part of the aliasing rule, which holds at any size
inline bool outputs_alias(const void* const* outs, int n, const void* done) {
  for (int i = 0; i < n; ++i) {
    if (!outs[i]) continue;
    if (outs[i] == done) return true;
    for (int j = i + 1; j < n; ++j)
      if (outs[i] == outs[j]) return true;
  }
  return false;
}

// an output overlapping done or another output
inline bool outputs_overlap(const void* const* outs, const uint64_t* out_b, int n, const void* done, uint64_t done_b) {
  for (int i = 0; i < n; ++i) {
    if (overlap(outs[i], out_b[i], done, done_b)) return true;
    for (int j = i + 1; j < n; ++j)
      if (overlap(outs[i], out_b[i], outs[j], out_b[j])) return true;
  }
  return false;
}

// the kernel's two views: the caller's, an unused one empty, team_stride 0 unless it is read
inline void fill_views(vss_setplay_view (&dst)[2], int32_t n_views, const vss_setplay_view* views) {
  for (int v = 0; v < 2; ++v) {
    if (v < n_views) dst[v] = views[v];
    else dst[v] = vss_setplay_view{nullptr, 0, 0, 1, 1, 0};
    if (dst[v].n_teams != 2) dst[v].team_stride = 0;
  }
}

}  // namespace host
}  // namespace vplace

#endif  // VSS_PLACEMENT_H
