// vss_perceive.hip — the perception channel in one launch (gfx950): vss_perceive of include/vss.h.
//
// What an overhead camera hands a policy: observation rows `delay` control steps late, with Gaussian noise on
// every pose.  vss_amd/perceive.py reference_perceive is the specification -- float32, one operation per line --
// and this file follows it line by line: + - * /, sqrtf, comparisons, selects and integer operations only, all
// correctly rounded, denormals kept, no FMA contraction (-ffp-contract=off and the pragma below).  The Philox
// block, u01 / u01_open0, sincos_small and the unit box_muller are vss_numerics.h's, the step's own: Box-Muller
// here is the step's box_muller_ou without the OU factor.  The result equals the reference bit for bit
// (tests/test_perceive_gpu.py, closed loop included).
//
//   one row per lane, one wave per workgroup, and all rows of a field in one wave: with R = n_teams * robots
//   rows per field a wave takes 64 / R fields (64, 32, 21 or 10; lanes past R * (64 / R) idle).  A field's age
//   is read by every one of its lanes and written by its first: inside one wave the load instruction has
//   returned for all lanes (s_waitcnt covers the whole instruction) before the store issues, so no lane can
//   read the new age.  Across waves nothing is shared.
//
//   Each lane loads its true row, the ring frame it needs and the six own-action floats of the terminal row --
//   13 + 13 + 4 16-byte loads, all issued before the first use -- then draws the field's 40 normals (ten Philox
//   blocks, twenty Box-Muller pairs: the loads' latency is behind them), and only then stores: ring slot,
//   obs_out, term_out, age.  Every global load of a lane is complete before its first store.  For delay >= 1
//   the slot read, (call - d) % (delay + 1) with 1 <= d <= delay, is never the slot written, call % (delay + 1).
//
//   Row-per-lane direct loads, not a cooperative LDS transpose: adjacent lanes hold adjacent 208-B rows, so the
//   13 load instructions of a wave together touch each 128-B line of a 13 KB span exactly once per row set --
//   every byte fetched is used, only spread over 13 instructions instead of one -- and the kernel runs at about
//   0.4 of the HBM spec on its algorithmic bytes (profiles/perceive_bench.json).  A transpose
//   would save address processing, not bytes, at the price of 13 KB of LDS per wave and two barriers.
//
//   The draws are computed by every lane of a field (up to six times the same 40 normals): sharing them would
//   need a cross-lane exchange keyed on a layout that varies per call site.  They add 6-10 us to a call of
//   21-130 us at 65,536 fields: mostly hidden behind the loads at six rows per field, visible at one.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vss.h"
#include "vss_numerics.h"

#pragma clang fp contract(off)

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "vss_perceive.hip targets gfx950 (CDNA4) only"
#endif

namespace vper {

using namespace vnum;
using namespace vnum::host;

constexpr int kWave = 64;
constexpr int kObs = VSS_NUM_OBS;  // 52 floats = 13 float4
constexpr int kQ = kObs / 4;
constexpr uint32_t kPurpose = 7u;  // the Philox counter's purpose byte (vss_step.hip uses 0..6)

// ---- the noise of one field and call -------------------------------------------------------------------------
// ball: n[0..3] = x y vx vy; robot e (0..2 blue, 3..5 yellow) in the world frame: x y vx vy at 4 + 6 e, then
// se, ce (the heading's rotation) and w's term.  A class whose sigma is 0 is never read.
struct Entity { float x, y, vx, vy, se, ce, w; };
struct Noise { float bx, by, bvx, bvy; Entity r[6]; };
struct Flags { bool pos, vel, ang, angvel; };

__device__ __forceinline__ void draw_noise(Noise& n, const vss_perceive_noise& sg, const Flags& on, uint32_t k0, uint32_t k1,
                                           uint32_t field, uint32_t call) {
  float z[40];
#pragma unroll
  for (int i = 0; i < 40; ++i) z[i] = 0.0f;
#pragma unroll
  for (int b = 0; b < 10; ++b) {
    // pair p: 0 ball position, 1 ball velocity, 2 + 3 e position, 3 + 3 e velocity, 4 + 3 e heading and yaw rate
    bool need[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int p = 2 * b + h;
      const int kind = p < 2 ? p : (p - 2) % 3;
      need[h] = kind == 0 ? on.pos : kind == 1 ? on.vel : (on.ang || on.angvel);
    }
    if (!(need[0] || need[1])) continue;  // uniform: the flags are kernel arguments
    uint32_t w[4];
    philox(k0, k1, field, call, kPurpose << 24, (uint32_t)b, w);
    if (need[0]) box_muller(w[0], w[1], z[4 * b + 0], z[4 * b + 1]);
    if (need[1]) box_muller(w[2], w[3], z[4 * b + 2], z[4 * b + 3]);
  }
  n.bx = sg.pos * z[0];
  n.by = sg.pos * z[1];
  n.bvx = sg.vel * z[2];
  n.bvy = sg.vel * z[3];
#pragma unroll
  for (int e = 0; e < 6; ++e) {
    n.r[e].x = sg.pos * z[4 + 6 * e];
    n.r[e].y = sg.pos * z[5 + 6 * e];
    n.r[e].vx = sg.vel * z[6 + 6 * e];
    n.r[e].vy = sg.vel * z[7 + 6 * e];
    const float eps = sg.ang * z[8 + 6 * e];
    sincos_small(eps, n.r[e].se, n.r[e].ce);
    n.r[e].w = sg.angvel * z[9 + 6 * e];
  }
}

__device__ __forceinline__ Entity pick(bool c, const Entity& a, const Entity& b) {
  Entity o;
  o.x = c ? a.x : b.x; o.y = c ? a.y : b.y; o.vx = c ? a.vx : b.vx; o.vy = c ? a.vy : b.vy;
  o.se = c ? a.se : b.se; o.ce = c ? a.ce : b.ce; o.w = c ? a.w : b.w;
  return o;
}

// one robot's seven floats at v[0..6]: x y vx vy cos sin w (sgn: the row's frame)
__device__ __forceinline__ void add_robot(float* v, const Entity& e, float sgn, const Flags& on) {
  if (on.pos) {
    v[0] = v[0] + sgn * e.x;
    v[1] = v[1] + sgn * e.y;
  }
  if (on.vel) {
    v[2] = v[2] + sgn * e.vx;
    v[3] = v[3] + sgn * e.vy;
  }
  if (on.ang) {
    const float c = v[4], s = v[5];
    v[4] = c * e.ce - s * e.se;
    v[5] = s * e.ce + c * e.se;
  }
  if (on.angvel) v[6] = v[6] + e.w;
}

// the noise on one row of team `yellow`, robot k: own[j], opp[j] are the entities of the row's slots
__device__ __forceinline__ void add_noise(float* v, const Noise& n, const Entity own[3], const Entity opp[3], float sgn,
                                          const Flags& on) {
  if (on.pos) {
    v[0] = v[0] + sgn * n.bx;
    v[1] = v[1] + sgn * n.by;
  }
  if (on.vel) {
    v[2] = v[2] + sgn * n.bvx;
    v[3] = v[3] + sgn * n.bvy;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) add_robot(v + 4 + 9 * j, own[j], sgn, on);
#pragma unroll
  for (int j = 0; j < 3; ++j) add_robot(v + 31 + 7 * j, opp[j], sgn, on);
}

__device__ __forceinline__ void load_row(float* v, const float* p) {
  const float4* q = reinterpret_cast<const float4*>(p);
#pragma unroll
  for (int i = 0; i < kQ; ++i) {
    const float4 x = q[i];
    v[4 * i] = x.x; v[4 * i + 1] = x.y; v[4 * i + 2] = x.z; v[4 * i + 3] = x.w;
  }
}

__device__ __forceinline__ void store_row(float* p, const float* v) {
  float4* q = reinterpret_cast<float4*>(p);
#pragma unroll
  for (int i = 0; i < kQ; ++i) q[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
}

// the own-action floats 11, 12 / 20, 21 / 29, 30 are in the row's float4s 2, 3, 5 and 7
__device__ __forceinline__ void load_actions(float a[6], const float* p) {
  const float4* q = reinterpret_cast<const float4*>(p);
  const float4 q2 = q[2], q3 = q[3], q5 = q[5], q7 = q[7];
  a[0] = q2.w; a[1] = q3.x; a[2] = q5.x; a[3] = q5.y; a[4] = q7.y; a[5] = q7.z;
}

__device__ __forceinline__ void set_actions(float* v, const float a[6]) {
  v[11] = a[0]; v[12] = a[1]; v[20] = a[2]; v[21] = a[3]; v[29] = a[4]; v[30] = a[5];
}

struct Args {
  int64_t n_fields, field_stride, team_stride, done_stride;
  int32_t first_team, delay;
  vss_perceive_noise noise;
  uint32_t k0, k1, call;
  const float* obs;
  const float* term;
  const int64_t* done;
  float* ring;
  int32_t* age;
  float* obs_out;
  float* term_out;
};

template <int ROBOTS, int TEAMS>
__global__ __launch_bounds__(kWave) void perceive_kernel(const Args a) {
  constexpr int R = ROBOTS * TEAMS;      // rows per field
  constexpr int kFields = kWave / R;     // fields per wave
  const int lane = threadIdx.x;
  const int fl = lane / R, r = lane % R;
  const int64_t f = (int64_t)blockIdx.x * kFields + fl;
  if (fl >= kFields || f >= a.n_fields) return;
  const int b = r / ROBOTS, k = r % ROBOTS;
  const bool yellow = (a.first_team ^ b) != 0;
  const bool start = a.term == nullptr;
  const int32_t D = a.delay;
  const int32_t slots = D + 1;

  const int64_t row = (int64_t)b * a.team_stride + f * a.field_stride + k;
  const int64_t packed = ((int64_t)b * a.n_fields + f) * ROBOTS + k;  // the ring's (n_teams, n_fields, robots)
  const int64_t frame = a.n_fields * R;                                // rows of one ring slot

  // ---- loads ----
  int32_t age = 0;
  bool done = false;
  if (!start) {
    age = a.age[f];
    age = age < 0 ? 0 : (age > D ? D : age);  // whatever the buffer holds, the slot arithmetic stays inside the ring
    done = a.done[f * a.done_stride] != 0;
  }
  const int32_t d = age + 1 < D ? age + 1 : D;
  const int32_t age_new = (start || done) ? 0 : d;
  const int32_t slot_w = (int32_t)(a.call % (uint32_t)slots);
  const int32_t slot_r = (slot_w + slots - d) % slots;

  float o[kObs], x[kObs], ta[6];
  load_row(o, a.obs + row * kObs);
  if (!start) {
    // the delayed frame, or for delay 0 the terminal row itself (then its own actions go back into it below)
    const float* src = D >= 1 ? a.ring + ((int64_t)slot_r * frame + packed) * kObs : a.term + row * kObs;
    load_row(x, src);
    load_actions(ta, a.term + row * kObs);
  } else {  // unused: the start call's row is the true one
#pragma unroll
    for (int i = 0; i < kObs; ++i) x[i] = o[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) ta[i] = 0.0f;
  }

  // ---- the field's draws ----
  Flags on;
  on.pos = a.noise.pos != 0.0f; on.vel = a.noise.vel != 0.0f; on.ang = a.noise.ang != 0.0f; on.angvel = a.noise.angvel != 0.0f;
  const bool any = on.pos || on.vel || on.ang || on.angvel;
  Noise n;
  Entity own[3], opp[3];
  const float sgn = yellow ? -1.0f : 1.0f;
  if (any) {
    draw_noise(n, a.noise, on, a.k0, a.k1, (uint32_t)f, a.call);
    Entity mine[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      mine[j] = pick(yellow, n.r[3 + j], n.r[j]);
      opp[j] = pick(yellow, n.r[j], n.r[3 + j]);
    }
    // own slot j is robot (k + j) % 3
    if (ROBOTS == 1) {
      own[0] = mine[0]; own[1] = mine[1]; own[2] = mine[2];
    } else {
      own[0] = pick(k == 0, mine[0], pick(k == 1, mine[1], mine[2]));
      own[1] = pick(k == 0, mine[1], pick(k == 1, mine[2], mine[0]));
      own[2] = pick(k == 0, mine[2], pick(k == 1, mine[0], mine[1]));
    }
  }

  // ---- outputs ----
  float t[kObs];
  if (!start) {
#pragma unroll
    for (int i = 0; i < kObs; ++i) t[i] = x[i];
    set_actions(t, ta);
    if (any) add_noise(t, n, own, opp, sgn, on);
  }
  const bool fresh = age_new == 0;  // the start call, a finished field, or delay 0
  float p[kObs];
#pragma unroll
  for (int i = 0; i < kObs; ++i) p[i] = fresh ? o[i] : x[i];
  p[11] = o[11]; p[12] = o[12]; p[20] = o[20]; p[21] = o[21]; p[29] = o[29]; p[30] = o[30];
  if (any) add_noise(p, n, own, opp, sgn, on);

  // ---- stores ----
  store_row(a.ring + ((int64_t)slot_w * frame + packed) * kObs, o);
  store_row(a.obs_out + row * kObs, p);
  if (!start) store_row(a.term_out + row * kObs, t);
  if (r == 0) a.age[f] = age_new;
}

}  // namespace vper

extern "C" {

int vss_perceive(void* stream, int64_t n_fields, const vss_perceive_layout* lay, int32_t delay,
                 const vss_perceive_noise* noise, uint64_t seed, uint32_t call, const float* obs, const float* term,
                 const int64_t* done, int64_t done_stride, float* ring, int32_t* age, float* obs_out, float* term_out) {
  using namespace vper;
  if (!lay || !noise || !obs || !done || !ring || !age || !obs_out) return VSS_E_ARG;
  if ((term == nullptr) != (term_out == nullptr)) return VSS_E_ARG;
  if (misaligned(obs, 16) || misaligned(term, 16) || misaligned(ring, 16) || misaligned(obs_out, 16) ||
      misaligned(term_out, 16) || misaligned(done, 8) || misaligned(age, 4))
    return VSS_E_ARG;
  if (delay < 0 || delay > VSS_PERCEIVE_MAX_DELAY) return VSS_E_ARG;
  const float sg[4] = {noise->pos, noise->vel, noise->ang, noise->angvel};
  for (float s : sg)
    if (!(s >= 0.0f) || !(s <= 3.4028235e38f)) return VSS_E_ARG;  // negative, NaN or infinite
  if ((lay->robots != 1 && lay->robots != 3) || (lay->n_teams != 1 && lay->n_teams != 2) ||
      (lay->first_team != 0 && lay->first_team != 1))
    return VSS_E_ARG;
  if (n_fields < 0 || done_stride < 1 || lay->field_stride < lay->robots) return VSS_E_ARG;
  const int64_t R = (int64_t)lay->robots * lay->n_teams;
  const int64_t fields_per_wave = kWave / R;
  // sizes: the grid is an unsigned x dimension; every byte offset stays an int64
  const int64_t kMaxRows = INT64_MAX / (4 * kObs) / (VSS_PERCEIVE_MAX_DELAY + 1);
  if (n_fields > 0) {
    const int64_t m = n_fields - 1;
    if (n_fields > kMaxRows / R || lay->field_stride > kMaxRows / n_fields || done_stride > (INT64_MAX / 8) / n_fields)
      return VSS_E_ARG;
    const int64_t block_rows = m * lay->field_stride + lay->robots;  // rows one team block spans
    if (lay->n_teams == 2 && (lay->team_stride < block_rows || lay->team_stride > kMaxRows - block_rows)) return VSS_E_ARG;
    const int64_t blocks = n_fields / fields_per_wave + (n_fields % fields_per_wave != 0);
    if (blocks > INT32_MAX) return VSS_E_ARG;
    const uint64_t span = (uint64_t)((lay->n_teams == 2 ? lay->team_stride : 0) + block_rows) * kObs * 4;
    const uint64_t ring_b = (uint64_t)(delay + 1) * (uint64_t)(n_fields * R) * kObs * 4;
    const uint64_t age_b = (uint64_t)n_fields * 4, done_b = (uint64_t)(m * done_stride + 1) * 8;
    // an output overlapping an input or another output
    const void* outs[4] = {obs_out, term_out, ring, age};
    const uint64_t out_b[4] = {span, span, ring_b, age_b};
    const void* ins[3] = {obs, term, done};
    const uint64_t in_b[3] = {span, span, done_b};
    for (int i = 0; i < 4; ++i) {
      for (int j = 0; j < 3; ++j)
        if (overlap(outs[i], out_b[i], ins[j], in_b[j])) return VSS_E_ARG;
      for (int j = i + 1; j < 4; ++j)
        if (overlap(outs[i], out_b[i], outs[j], out_b[j])) return VSS_E_ARG;
    }
    Args a;
    a.n_fields = n_fields; a.field_stride = lay->field_stride; a.team_stride = lay->n_teams == 2 ? lay->team_stride : 0;
    a.done_stride = done_stride; a.first_team = lay->first_team; a.delay = delay; a.noise = *noise;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.call = call;
    a.obs = obs; a.term = term; a.done = done; a.ring = ring; a.age = age; a.obs_out = obs_out; a.term_out = term_out;
    const dim3 grid((unsigned)blocks), block(kWave);
    hipStream_t s = (hipStream_t)stream;
    if (lay->robots == 1 && lay->n_teams == 1) hipLaunchKernelGGL((perceive_kernel<1, 1>), grid, block, 0, s, a);
    else if (lay->robots == 1) hipLaunchKernelGGL((perceive_kernel<1, 2>), grid, block, 0, s, a);
    else if (lay->n_teams == 1) hipLaunchKernelGGL((perceive_kernel<3, 1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((perceive_kernel<3, 2>), grid, block, 0, s, a);
    return hipGetLastError() == hipSuccess ? VSS_OK : VSS_E_LAUNCH;
  }
  // n_fields == 0: the pointer-equality part of the aliasing rule still holds, then nothing to do
  if (obs_out == obs || obs_out == term || (term_out && (term_out == obs || term_out == term || term_out == obs_out)) ||
      (const void*)ring == (const void*)obs || (const void*)ring == (const void*)term || (void*)ring == (void*)obs_out ||
      (void*)ring == (void*)term_out)
    return VSS_E_ARG;
  return VSS_OK;
}

}  // extern "C"
