// vss_track.hip — the tracking channel in one launch (gfx950): vss_track of include/vss.h.
//
// Every perceived observation row is filtered across calls in its own frame: the last filtered row (`est`, the
// caller's state) is moved one control step with the project's drive model and the command that moved that frame,
// then corrected body by body with the new row -- a fixed gain per kind of body behind a position / velocity /
// heading gate.  vss_amd/track.py reference_track is the specification -- float32, one operation per line -- and
// this file follows it line by line: + - * /, comparisons, selects and integer operations only, all correctly
// rounded, denormals kept, no FMA contraction (-ffp-contract=off and the pragma below).  The result equals the
// reference bit for bit (tests/test_track_gpu.py).
//
//   The one-step drive model below (drive, move, turn, the ball's damping) restates vss_estimate.hip's: it
//   was written when this unit was a library of its own.  In Python there is one copy (reference_track calls
//   estimate.predict_rows) and the bit-equality test pins this restatement to it.  Now that both are units of one
//   library a shared header can remove the duplicate; that is not done yet.
//
//   one row per lane, as vss_estimate.hip: est, age and hist are per row, so a lane reads and writes only its own
//   state, nothing goes through LDS and the workgroup shape (256 rows, four waves) is free of the layout.
//
//   All of a lane's loads -- done, age, the three rows (13 x 16 B each), its one history entry (three 8-B loads) --
//   are issued before it computes or stores anything.  No output may overlap an input (refused by the entry); the
//   history slot written, call % delay, is the one a saturated row reads, by the same lane, before it writes.
//
//   The work is separable by body and is scheduled body by body: a body's floats of est are copied, moved and
//   corrected with the two input rows' floats in place, so three rows are live and never four.  The two corrections
//   are not shared: one is ~40 operations per body, against 3 x 208 B of traffic per row each way.
//
//   Bodies are picked with compile-time offsets: an array indexed by a run-time value goes to scratch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vss.h"
#include "vss_numerics.h"

#pragma clang fp contract(off)

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "vss_track.hip targets gfx950 (CDNA4) only"
#endif

namespace vtrk {

using namespace vnum;
using namespace vnum::host;

constexpr int kBlock = 256;  // rows per workgroup (four waves)
constexpr int kObs = 52;     // floats per row
constexpr int kQuads = 13;   // 16-B pieces per row
constexpr int kNsub = 2;     // substeps per control step

enum Kind { kBall, kTeam, kOpp };

struct Args {
  int64_t rows;  // n_teams * n_fields * robots: one lane each
  int64_t n_fields, field_stride, team_stride, done_stride;
  int32_t delay, slot;  // slot = call % delay (0 for delay 0): read by a saturated row, written by every row
  float gain_team, gain_opp, gain_ball, gate_pos, gate_vel;
  const float* obs;
  const float* term;
  const int64_t* done;
  float* est;
  float* hist;
  int32_t* age;
  float* obs_out;
  float* term_out;
};

struct Row { float v[kObs]; };   // indexed by compile-time constants only
struct Body { float v[7]; };     // x y vx vy cos sin w (the ball: the first four)

__device__ __forceinline__ float clamp_sym(float x, float lim) { return x < -lim ? -lim : (x > lim ? lim : x); }

__device__ __forceinline__ Row load_row(const float* base, int64_t at) {
  const float4* p = reinterpret_cast<const float4*>(base) + at * kQuads;
  Row r;
#pragma unroll
  for (int q = 0; q < kQuads; ++q) {
    const float4 x = p[q];
    r.v[4 * q + 0] = x.x; r.v[4 * q + 1] = x.y; r.v[4 * q + 2] = x.z; r.v[4 * q + 3] = x.w;
  }
  return r;
}

__device__ __forceinline__ void store_row(float* base, int64_t at, const Row& r) {
  float4* p = reinterpret_cast<float4*>(base) + at * kQuads;
#pragma unroll
  for (int q = 0; q < kQuads; ++q) p[q] = make_float4(r.v[4 * q + 0], r.v[4 * q + 1], r.v[4 * q + 2], r.v[4 * q + 3]);
}

// ---- the one-step motion model: vss_estimate.hip's lines, per body -------------------------------------------------
__device__ __forceinline__ void move(Body& b) {
  b.v[0] = b.v[0] + b.v[2] * 0.025f;
  b.v[1] = b.v[1] + b.v[3] * 0.025f;
}

__device__ __forceinline__ void turn(Body& b) {
  const float c = b.v[4], s = b.v[5];
  float se, ce;
  sincos_small(b.v[6] * 0.025f, se, ce);
  const float c1 = c * ce - s * se;
  const float s1 = s * ce + c * se;
  const float k = 1.5f - 0.5f * (c1 * c1 + s1 * s1);
  b.v[4] = c1 * k;
  b.v[5] = s1 * k;
}

__device__ __forceinline__ void drive(Body& b, float tl, float tr) {
  const float c = b.v[4], s = b.v[5];
  const float vx = b.v[2], vy = b.v[3], w = b.v[6];
  float vf = c * vx + s * vy;
  float vl = c * vy - s * vx;
  float wl = vf - w * 0.03375f;
  float wr = vf + w * 0.03375f;
  wl = wl + clamp_sym(tl - wl, 0.15f);
  wr = wr + clamp_sym(tr - wr, 0.15f);
  vf = (wl + wr) * 0.5f;
  b.v[6] = (wr - wl) * 14.814815f;
  vl = vl - clamp_sym(vl, 0.171675f);
  b.v[2] = c * vf - s * vl;
  b.v[3] = s * vf + c * vl;
}

// one control step of the body (estimate.py predict_rows with a lead of 1, the body's lines)
template <int KIND>
__device__ __forceinline__ void advance(Body& b, float al, float ar) {
  const float tl = (al * 42.0f) * 0.024f, tr = (ar * 42.0f) * 0.024f;
#pragma unroll
  for (int sub = 0; sub < kNsub; ++sub) {
    if (KIND == kTeam) drive(b, tl, tr);
    if (KIND == kBall) {
      b.v[2] = b.v[2] * 0.99625f;
      b.v[3] = b.v[3] * 0.99625f;
    }
    move(b);
    if (KIND != kBall) turn(b);
  }
}

// ---- the correction ------------------------------------------------------------------------------------------------
// reference_track's update of one body: p the prediction, z the input row's floats at B (replaced by the result)
template <int KIND, int B>
__device__ __forceinline__ void update(const Body& p, Row& zr, float g, float gate_pos, float gate_vel, bool keep) {
  constexpr int NF = KIND == kBall ? 4 : 7;
  float z[NF], o[NF];
#pragma unroll
  for (int i = 0; i < NF; ++i) z[i] = zr.v[B + i];
  const float dx = z[0] - p.v[0], dy = z[1] - p.v[1], dvx = z[2] - p.v[2], dvy = z[3] - p.v[3];
  o[0] = p.v[0] + g * dx;
  o[1] = p.v[1] + g * dy;
  o[2] = p.v[2] + g * dvx;
  o[3] = p.v[3] + g * dvy;
  bool trip = (gate_pos > 0.0f && (fabsf(dx) > gate_pos || fabsf(dy) > gate_pos)) ||
              (gate_vel > 0.0f && (fabsf(dvx) > gate_vel || fabsf(dvy) > gate_vel));
  if (KIND != kBall) {
    const float cp = p.v[4], sp = p.v[5];
    const float dot = cp * z[4] + sp * z[5];
    const float e = g * (cp * z[5] - sp * z[4]);
    float se, ce;
    sincos_small(e, se, ce);
    const float c1 = cp * ce - sp * se;
    const float s1 = sp * ce + cp * se;
    const float k = 1.5f - 0.5f * (c1 * c1 + s1 * s1);
    o[4] = c1 * k;
    o[5] = s1 * k;
    o[6] = p.v[6] + g * (z[6] - p.v[6]);
    trip = trip || dot < 0.0f;
  }
  const bool take_z = keep || trip || g == 0.0f;  // bit for bit: -0.0 and NaNs pass
#pragma unroll
  for (int i = 0; i < NF; ++i) zr.v[B + i] = take_z ? z[i] : o[i];
}

// one body: predict from est, correct with term and with obs (obs keeps its floats where the field is done)
template <int KIND, int B>
__device__ __forceinline__ void body(const Row& est, Row& term, Row& obs, bool adv, bool done, float al, float ar,
                                     float g, float gate_pos, float gate_vel) {
  constexpr int NF = KIND == kBall ? 4 : 7;
  Body p, q;
#pragma unroll
  for (int i = 0; i < 7; ++i) p.v[i] = i < NF ? est.v[B + i] : 0.0f;
  q = p;
  advance<KIND>(q, al, ar);
#pragma unroll
  for (int i = 0; i < NF; ++i) p.v[i] = adv ? q.v[i] : p.v[i];
  update<KIND, B>(p, term, g, gate_pos, gate_vel, false);
  update<KIND, B>(p, obs, g, gate_pos, gate_vel, done);
}

// Two waves per SIMD: without the second bound the allocator takes 256 VGPRs and 3 AGPRs and one wave fits; with it
// the same code fits 256 registers with no scratch (make resource-usage).
template <int ROBOTS>
__global__ __launch_bounds__(kBlock, 2) void track_kernel(const Args a) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // the packed row (n_teams, n_fields, robots)
  if (p >= a.rows) return;
  const int64_t per_team = a.n_fields * ROBOTS;
  const int64_t b = p >= per_team ? 1 : 0;
  const int64_t in_team = p - b * per_team;
  const int64_t f = in_team / ROBOTS, k = in_team % ROBOTS;
  const int64_t at = b * a.team_stride + f * a.field_stride + k;
  const int D = a.delay;
  float2* slot = D >= 1 ? reinterpret_cast<float2*>(a.hist) + ((int64_t)a.slot * a.rows + p) * 3 : nullptr;

  if (a.term == nullptr) {  // the start call (uniform over the grid): every age 0, est = obs_out = obs
    const Row obs = load_row(a.obs, at);
    store_row(a.obs_out, at, obs);
    store_row(a.est, p, obs);
    if (D >= 1) {
      slot[0] = make_float2(obs.v[11], obs.v[12]);
      slot[1] = make_float2(obs.v[20], obs.v[21]);
      slot[2] = make_float2(obs.v[29], obs.v[30]);
    }
    a.age[p] = 0;
    return;
  }

  // ---- loads ----
  const bool done = a.done[f * a.done_stride] != 0;
  int age = a.age[p];
  Row obs = load_row(a.obs, at);
  Row term = load_row(a.term, at);
  const Row est = load_row(a.est, p);
  float2 c0 = make_float2(term.v[11], term.v[12]), c1 = make_float2(term.v[20], term.v[21]),
         c2 = make_float2(term.v[29], term.v[30]);  // delay 0: the command of this very call
  if (D >= 1) { c0 = slot[0]; c1 = slot[1]; c2 = slot[2]; }  // the command of call t - D (used by a saturated row only)
  age = age < 0 ? 0 : (age > D ? D : age);  // as read: whatever the buffer holds
  const int d = age + 1 < D ? age + 1 : D;
  const int age_new = done ? 0 : d;
  const bool adv = d == age;  // 1 - (d - a)
  const float2 own0 = make_float2(obs.v[11], obs.v[12]), own1 = make_float2(obs.v[20], obs.v[21]),
               own2 = make_float2(obs.v[29], obs.v[30]);

  // ---- body by body ----
  body<kBall, 0>(est, term, obs, adv, done, 0.0f, 0.0f, a.gain_ball, a.gate_pos, a.gate_vel);
  body<kTeam, 4>(est, term, obs, adv, done, c0.x, c0.y, a.gain_team, a.gate_pos, a.gate_vel);
  body<kTeam, 13>(est, term, obs, adv, done, c1.x, c1.y, a.gain_team, a.gate_pos, a.gate_vel);
  body<kTeam, 22>(est, term, obs, adv, done, c2.x, c2.y, a.gain_team, a.gate_pos, a.gate_vel);
  body<kOpp, 31>(est, term, obs, adv, done, 0.0f, 0.0f, a.gain_opp, a.gate_pos, a.gate_vel);
  body<kOpp, 38>(est, term, obs, adv, done, 0.0f, 0.0f, a.gain_opp, a.gate_pos, a.gate_vel);
  body<kOpp, 45>(est, term, obs, adv, done, 0.0f, 0.0f, a.gain_opp, a.gate_pos, a.gate_vel);

  // ---- stores ----
  store_row(a.term_out, at, term);
  store_row(a.obs_out, at, obs);
  store_row(a.est, p, obs);
  if (D >= 1) { slot[0] = own0; slot[1] = own1; slot[2] = own2; }
  a.age[p] = age_new;
}

inline bool gain_ok(float g) { return g >= 0.0f && g <= 1.0f; }            // false for a NaN
inline bool gate_ok(float g) { return g >= 0.0f && g <= 3.4028235e38f; }   // false for a NaN and for +inf

}  // namespace vtrk

extern "C" {

int vss_track(void* stream, int64_t n_fields, const vss_track_layout* lay, const vss_track_params* prm, int32_t delay,
              uint32_t call, const float* obs, const float* term, const int64_t* done, int64_t done_stride, float* est,
              float* hist, int32_t* age, float* obs_out, float* term_out) {
  using namespace vtrk;
  if (!lay || !prm || !obs || !done || !est || !age || !obs_out) return VSS_E_ARG;
  if (delay < 0 || delay > VSS_TRACK_MAX_DELAY) return VSS_E_ARG;
  if (delay >= 1 && !hist) return VSS_E_ARG;
  if ((term == nullptr) != (term_out == nullptr)) return VSS_E_ARG;
  if (!gain_ok(prm->gain_team) || !gain_ok(prm->gain_opp) || !gain_ok(prm->gain_ball) || !gate_ok(prm->gate_pos) ||
      !gate_ok(prm->gate_vel))
    return VSS_E_ARG;
  if (misaligned(obs, 16) || misaligned(term, 16) || misaligned(obs_out, 16) || misaligned(term_out, 16) ||
      misaligned(est, 16) || misaligned(done, 8) || misaligned(hist, 8) || misaligned(age, 4))
    return VSS_E_ARG;
  if ((lay->robots != 1 && lay->robots != 3) || (lay->n_teams != 1 && lay->n_teams != 2)) return VSS_E_ARG;
  if (n_fields < 0 || done_stride < 1 || lay->field_stride < lay->robots) return VSS_E_ARG;
  // the pointer-equality part of the aliasing rule holds at any size
  {
    const void* outs[5] = {obs_out, term_out, est, hist, age};
    const void* ins[3] = {obs, term, done};
    for (int i = 0; i < 5; ++i) {
      if (!outs[i]) continue;
      for (int j = 0; j < 3; ++j)
        if (outs[i] == ins[j]) return VSS_E_ARG;
      for (int j = i + 1; j < 5; ++j)
        if (outs[i] == outs[j]) return VSS_E_ARG;
    }
  }
  if (n_fields == 0) return VSS_OK;

  const int64_t R = (int64_t)lay->robots * lay->n_teams;
  // sizes: the grid is an unsigned x dimension; every byte offset stays an int64 (208 B per row, a ring of up to 15)
  const int64_t kMaxRows = INT64_MAX / (4 * kObs) / (VSS_TRACK_MAX_DELAY + 1);
  const int64_t m = n_fields - 1;
  if (n_fields > kMaxRows / R || lay->field_stride > kMaxRows / n_fields || done_stride > (INT64_MAX / 8) / n_fields)
    return VSS_E_ARG;
  const int64_t block_rows = m * lay->field_stride + lay->robots;  // rows one team block spans
  if (lay->n_teams == 2 && (lay->team_stride < block_rows || lay->team_stride > kMaxRows - block_rows))
    return VSS_E_ARG;
  const int64_t rows = n_fields * R;
  const int64_t blocks = rows / kBlock + (rows % kBlock != 0);
  if (blocks > INT32_MAX) return VSS_E_ARG;
  const uint64_t span = (uint64_t)((lay->n_teams == 2 ? lay->team_stride : 0) + block_rows) * kObs * 4;
  const uint64_t est_b = (uint64_t)rows * kObs * 4, hist_b = (uint64_t)delay * (uint64_t)rows * 24;
  const uint64_t age_b = (uint64_t)rows * 4, done_b = (uint64_t)(m * done_stride + 1) * 8;
  // an output overlapping an input or another output
  const void* outs[5] = {obs_out, term_out, est, delay >= 1 ? hist : nullptr, age};
  const uint64_t out_b[5] = {span, span, est_b, hist_b, age_b};
  const void* ins[3] = {obs, term, done};
  const uint64_t in_b[3] = {span, span, done_b};
  for (int i = 0; i < 5; ++i) {
    for (int j = 0; j < 3; ++j)
      if (overlap(outs[i], out_b[i], ins[j], in_b[j])) return VSS_E_ARG;
    for (int j = i + 1; j < 5; ++j)
      if (overlap(outs[i], out_b[i], outs[j], out_b[j])) return VSS_E_ARG;
  }

  Args a;
  a.rows = rows; a.n_fields = n_fields; a.field_stride = lay->field_stride;
  a.team_stride = lay->n_teams == 2 ? lay->team_stride : 0; a.done_stride = done_stride;
  a.delay = delay; a.slot = delay >= 1 ? (int32_t)(call % (uint32_t)delay) : 0;
  a.gain_team = prm->gain_team; a.gain_opp = prm->gain_opp; a.gain_ball = prm->gain_ball;
  a.gate_pos = prm->gate_pos; a.gate_vel = prm->gate_vel;
  a.obs = obs; a.term = term; a.done = done; a.est = est; a.hist = hist; a.age = age; a.obs_out = obs_out;
  a.term_out = term_out;
  const dim3 grid((unsigned)blocks), block(kBlock);
  hipStream_t s = (hipStream_t)stream;
  if (lay->robots == 1) hipLaunchKernelGGL((track_kernel<1>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((track_kernel<3>), grid, block, 0, s, a);
  return hipGetLastError() == hipSuccess ? VSS_OK : VSS_E_LAUNCH;
}

}  // extern "C"
