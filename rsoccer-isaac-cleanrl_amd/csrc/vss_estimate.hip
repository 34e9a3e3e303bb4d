// vss_estimate.hip — the estimation channel in one launch (gfx950): vss_estimate of include/vss.h.
//
// A perceived observation row is the state of `lead` control steps ago; its six own-action floats are the current
// step's commands.  The channel rolls every row forward to the present with DESIGN.md §3's drive, damping and
// integration steps (no contacts, no walls), `lead` times, with the commands the row's team gave in the meantime,
// which it keeps in a ring of its own.  vss_amd/estimate.py reference_estimate is the specification -- float32, one
// operation per line -- and this file follows it line by line: + - * /, comparisons, selects and integer operations
// only, all correctly rounded, denormals kept, no FMA contraction (-ffp-contract=off and the pragma below).  The
// drive lines are those of oracle/vss_oracle.c physics_field with (c, s) taken from the row; sincos_small is
// vss_numerics.h's, shared with vss_perceive.hip and vss_step.hip.  The result equals the reference bit for bit
// (tests/test_estimate_gpu.py, closed loop included).
//
//   one row per lane.  age and hist are per row, so a lane reads and writes only its own state: no lane depends on
//   another, nothing goes through LDS, and the workgroup shape (256 rows, four waves) is free of the layout.
//   Adjacent lanes hold adjacent 208-B rows of a block, as in vss_perceive.hip.
//
//   All of a lane's loads -- done, age, the two rows (13 x 16 B each), the up to delay - 1 history entries it needs
//   (three 8-B loads each) -- are issued before it computes or stores anything.  No output may overlap an input
//   (refused by the entry), and the history slot written, call % delay, is never one that is read.
//
//   The prediction loop runs `lead` times per lane (bounded by delay) and may diverge inside a wave: rows of one
//   wave differ in age only in the first `delay` steps after one of them was reset.  The specification evaluates
//   the prediction twice per row, for the terminal row and for the row itself; where both have the same lead and
//   the two input rows are equal bit for bit (every row of a field that is not done, as perception delivers them),
//   the second is the first's copy -- the same function of the same bits -- and is not computed again.
//
//   Robots are picked with compile-time-unrolled loops and the history entry of a step with selects: an array
//   indexed by a run-time value goes to scratch.  HMAX, the history entries kept in registers, is a template
//   parameter (0, 3 or 14, for delay <= 1, <= 4, <= 15), so a short delay does not pay the registers of a long one.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vss.h"
#include "vss_numerics.h"

#pragma clang fp contract(off)

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "vss_estimate.hip targets gfx950 (CDNA4) only"
#endif

namespace vest {

using namespace vnum;
using namespace vnum::host;

constexpr int kBlock = 256;  // rows per workgroup (four waves)
constexpr int kObs = 52;     // floats per row
constexpr int kQuads = 13;   // 16-B pieces per row
constexpr int kNsub = 2;     // substeps per control step

struct Args {
  int64_t rows;  // n_teams * n_fields * robots: one lane each
  int64_t n_fields, field_stride, team_stride, done_stride;
  int32_t delay, slot_w;  // slot_w = call % delay (0 for delay 0)
  const float* obs;
  const float* term;
  const int64_t* done;
  float* hist;
  int32_t* age;
  float* obs_out;
  float* term_out;
};

struct Row { float v[kObs]; };  // indexed by compile-time constants only

template <int HMAX>
struct History { float2 a[HMAX > 0 ? HMAX : 1][3]; };  // entry m: the commands of call t - d + 1 + m, (aL, aR) per own robot

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

__device__ __forceinline__ bool same_bits(const Row& a, const Row& b) {
  uint32_t diff = 0u;
#pragma unroll
  for (int i = 0; i < kObs; ++i) diff |= __float_as_uint(a.v[i]) ^ __float_as_uint(b.v[i]);
  return diff == 0u;
}

// x += vx h, y += vy h of the body at `B`
template <int B>
__device__ __forceinline__ void move(Row& r) {
  r.v[B + 0] = r.v[B + 0] + r.v[B + 2] * 0.025f;
  r.v[B + 1] = r.v[B + 1] + r.v[B + 3] * 0.025f;
}

// the heading of the robot at `B` rotated by w h, renormalised by one Newton step
template <int B>
__device__ __forceinline__ void turn(Row& r) {
  const float c = r.v[B + 4], s = r.v[B + 5];
  float se, ce;
  sincos_small(r.v[B + 6] * 0.025f, se, ce);
  const float c1 = c * ce - s * se;
  const float s1 = s * ce + c * se;
  const float k = 1.5f - 0.5f * (c1 * c1 + s1 * s1);
  r.v[B + 4] = c1 * k;
  r.v[B + 5] = s1 * k;
}

// the traction-limited differential drive of the own robot at `B` towards the wheel-rim targets (tl, tr)
template <int B>
__device__ __forceinline__ void drive(Row& r, float tl, float tr) {
  const float c = r.v[B + 4], s = r.v[B + 5];
  const float vx = r.v[B + 2], vy = r.v[B + 3], w = r.v[B + 6];
  float vf = c * vx + s * vy;
  float vl = c * vy - s * vx;
  float wl = vf - w * 0.03375f;
  float wr = vf + w * 0.03375f;
  wl = wl + clamp_sym(tl - wl, 0.15f);
  wr = wr + clamp_sym(tr - wr, 0.15f);
  vf = (wl + wr) * 0.5f;
  r.v[B + 6] = (wr - wl) * 14.814815f;
  vl = vl - clamp_sym(vl, 0.171675f);
  r.v[B + 2] = c * vf - s * vl;
  r.v[B + 3] = s * vf + c * vl;
}

// reference_estimate's predict: `lead` control steps; step i < lead - 1 takes h.a[i], the last one the row's own
// action floats (which stay as they are)
template <int HMAX>
__device__ __forceinline__ void predict(Row& r, int lead, const History<HMAX>& h) {
#pragma unroll 1
  for (int i = 0; i < lead; ++i) {
    float2 a0 = make_float2(r.v[11], r.v[12]), a1 = make_float2(r.v[20], r.v[21]), a2 = make_float2(r.v[29], r.v[30]);
#pragma unroll
    for (int m = 0; m < HMAX; ++m) {
      const bool use = i == m && m < lead - 1;
      a0.x = use ? h.a[m][0].x : a0.x; a0.y = use ? h.a[m][0].y : a0.y;
      a1.x = use ? h.a[m][1].x : a1.x; a1.y = use ? h.a[m][1].y : a1.y;
      a2.x = use ? h.a[m][2].x : a2.x; a2.y = use ? h.a[m][2].y : a2.y;
    }
    const float tl0 = (a0.x * 42.0f) * 0.024f, tr0 = (a0.y * 42.0f) * 0.024f;
    const float tl1 = (a1.x * 42.0f) * 0.024f, tr1 = (a1.y * 42.0f) * 0.024f;
    const float tl2 = (a2.x * 42.0f) * 0.024f, tr2 = (a2.y * 42.0f) * 0.024f;
#pragma unroll
    for (int sub = 0; sub < kNsub; ++sub) {
      drive<4>(r, tl0, tr0);
      drive<13>(r, tl1, tr1);
      drive<22>(r, tl2, tr2);
      r.v[2] = r.v[2] * 0.99625f;
      r.v[3] = r.v[3] * 0.99625f;
      move<0>(r);
      move<4>(r); move<13>(r); move<22>(r);
      move<31>(r); move<38>(r); move<45>(r);
      turn<4>(r); turn<13>(r); turn<22>(r);
      turn<31>(r); turn<38>(r); turn<45>(r);
    }
  }
}

template <int ROBOTS, int HMAX>
__global__ __launch_bounds__(kBlock) void estimate_kernel(const Args a) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // the packed row (n_teams, n_fields, robots)
  if (p >= a.rows) return;
  const int64_t per_team = a.n_fields * ROBOTS;
  const int64_t b = p >= per_team ? 1 : 0;
  const int64_t in_team = p - b * per_team;
  const int64_t f = in_team / ROBOTS, k = in_team % ROBOTS;
  const int64_t at = b * a.team_stride + f * a.field_stride + k;
  const bool start = a.term == nullptr;
  const int D = a.delay;

  // ---- loads ----
  int64_t done = 0;
  int age = 0;
  if (!start) {
    done = a.done[f * a.done_stride];
    age = a.age[p];
  }
  Row obs = load_row(a.obs, at);
  Row term = obs;
  if (!start) term = load_row(a.term, at);
  age = age < 0 ? 0 : (age > D ? D : age);  // as read: whatever the buffer holds, a lead stays within the ring
  const int d = start ? 0 : (age + 1 < D ? age + 1 : D);
  const int age_new = (start || done != 0) ? 0 : d;
  History<HMAX> h;
#pragma unroll
  for (int m = 0; m < HMAX; ++m) {
#pragma unroll
    for (int j = 0; j < 3; ++j) h.a[m][j] = make_float2(0.0f, 0.0f);
    if (m < d - 1) {  // the commands of call t - (d - 1 - m)
      int slot = a.slot_w - (d - 1 - m);
      slot = slot < 0 ? slot + D : slot;
      const float2* e = reinterpret_cast<const float2*>(a.hist) + ((int64_t)slot * a.rows + p) * 3;
#pragma unroll
      for (int j = 0; j < 3; ++j) h.a[m][j] = e[j];
    }
  }

  // ---- the two predictions ----
  const float2 own0 = make_float2(obs.v[11], obs.v[12]), own1 = make_float2(obs.v[20], obs.v[21]),
               own2 = make_float2(obs.v[29], obs.v[30]);
  const bool shared = !start && age_new == d && same_bits(obs, term);
  predict<HMAX>(obs, age_new, h);
  if (shared) term = obs;
  else if (!start) predict<HMAX>(term, d, h);

  // ---- stores ----
  store_row(a.obs_out, at, obs);
  if (!start) store_row(a.term_out, at, term);
  if (D >= 1) {
    float2* e = reinterpret_cast<float2*>(a.hist) + ((int64_t)a.slot_w * a.rows + p) * 3;
    e[0] = own0; e[1] = own1; e[2] = own2;
  }
  a.age[p] = age_new;
}

template <int ROBOTS>
inline void launch(int delay, dim3 grid, hipStream_t s, const Args& a) {
  const dim3 block(kBlock);
  if (delay <= 1) hipLaunchKernelGGL((estimate_kernel<ROBOTS, 0>), grid, block, 0, s, a);
  else if (delay <= 4) hipLaunchKernelGGL((estimate_kernel<ROBOTS, 3>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((estimate_kernel<ROBOTS, VSS_ESTIMATE_MAX_DELAY - 1>), grid, block, 0, s, a);
}

}  // namespace vest

extern "C" {

int vss_estimate(void* stream, int64_t n_fields, const vss_estimate_layout* lay, int32_t delay, uint32_t call, const float* obs,
                 const float* term, const int64_t* done, int64_t done_stride, float* hist, int32_t* age, float* obs_out,
                 float* term_out) {
  using namespace vest;
  if (!lay || !obs || !done || !age || !obs_out) return VSS_E_ARG;
  if (delay < 0 || delay > VSS_ESTIMATE_MAX_DELAY) return VSS_E_ARG;
  if (delay >= 1 && !hist) return VSS_E_ARG;
  if ((term == nullptr) != (term_out == nullptr)) return VSS_E_ARG;
  if (misaligned(obs, 16) || misaligned(term, 16) || misaligned(obs_out, 16) || misaligned(term_out, 16) ||
      misaligned(done, 8) || misaligned(hist, 8) || misaligned(age, 4))
    return VSS_E_ARG;
  if ((lay->robots != 1 && lay->robots != 3) || (lay->n_teams != 1 && lay->n_teams != 2)) return VSS_E_ARG;
  if (n_fields < 0 || done_stride < 1 || lay->field_stride < lay->robots) return VSS_E_ARG;
  // the pointer-equality part of the aliasing rule holds at any size
  if (obs_out == obs || obs_out == term || (term_out && (term_out == obs || term_out == term || term_out == obs_out)) ||
      (hist && ((const void*)hist == (const void*)obs || (const void*)hist == (const void*)term ||
                (void*)hist == (void*)obs_out || (void*)hist == (void*)term_out || (void*)hist == (void*)age)) ||
      (const void*)age == (const void*)obs || (const void*)age == (const void*)term || (void*)age == (void*)obs_out ||
      (void*)age == (void*)term_out || (const void*)age == (const void*)done || (const void*)obs_out == (const void*)done ||
      (term_out && (const void*)term_out == (const void*)done) || (hist && (const void*)hist == (const void*)done))
    return VSS_E_ARG;
  if (n_fields == 0) return VSS_OK;

  const int64_t R = (int64_t)lay->robots * lay->n_teams;
  // sizes: the grid is an unsigned x dimension; every byte offset stays an int64 (208 B per row, a ring of up to 15)
  const int64_t kMaxRows = INT64_MAX / (4 * kObs) / (VSS_ESTIMATE_MAX_DELAY + 1);
  const int64_t m = n_fields - 1;
  if (n_fields > kMaxRows / R || lay->field_stride > kMaxRows / n_fields || done_stride > (INT64_MAX / 8) / n_fields)
    return VSS_E_ARG;
  const int64_t block_rows = m * lay->field_stride + lay->robots;  // rows one team block spans
  if (lay->n_teams == 2 && (lay->team_stride < block_rows || lay->team_stride > kMaxRows - block_rows)) return VSS_E_ARG;
  const int64_t rows = n_fields * R;
  const int64_t blocks = rows / kBlock + (rows % kBlock != 0);
  if (blocks > INT32_MAX) return VSS_E_ARG;
  const uint64_t span = (uint64_t)((lay->n_teams == 2 ? lay->team_stride : 0) + block_rows) * kObs * 4;
  const uint64_t hist_b = (uint64_t)delay * (uint64_t)rows * 24, age_b = (uint64_t)rows * 4;
  const uint64_t done_b = (uint64_t)(m * done_stride + 1) * 8;
  // an output overlapping an input or another output
  const void* outs[4] = {obs_out, term_out, delay >= 1 ? hist : nullptr, age};
  const uint64_t out_b[4] = {span, span, hist_b, age_b};
  const void* ins[3] = {obs, term, done};
  const uint64_t in_b[3] = {span, span, done_b};
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 3; ++j)
      if (overlap(outs[i], out_b[i], ins[j], in_b[j])) return VSS_E_ARG;
    for (int j = i + 1; j < 4; ++j)
      if (overlap(outs[i], out_b[i], outs[j], out_b[j])) return VSS_E_ARG;
  }

  Args a;
  a.rows = rows; a.n_fields = n_fields; a.field_stride = lay->field_stride;
  a.team_stride = lay->n_teams == 2 ? lay->team_stride : 0; a.done_stride = done_stride;
  a.delay = delay; a.slot_w = delay >= 1 ? (int32_t)(call % (uint32_t)delay) : 0;
  a.obs = obs; a.term = term; a.done = done; a.hist = hist; a.age = age; a.obs_out = obs_out; a.term_out = term_out;
  const dim3 grid((unsigned)blocks);
  hipStream_t s = (hipStream_t)stream;
  if (lay->robots == 1) launch<1>(delay, grid, s, a);
  else launch<3>(delay, grid, s, a);
  return hipGetLastError() == hipSuccess ? VSS_OK : VSS_E_LAUNCH;
}

}  // extern "C"
