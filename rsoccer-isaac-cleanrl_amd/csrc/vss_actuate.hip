// vss_actuate.hip — the actuation channel in one launch (gfx950): vss_actuate of include/vss.h.
//
// What a VSS robot's wheels receive of what a policy commands: the radio's range and quantisation, a lost packet
// (the robot keeps the command it had), a deadband, the episode's per-wheel motor gains and per-step command
// noise.  vss_amd/actuate.py reference_actuate is the specification -- float32, one operation per line -- and this
// file follows it line by line: + - * /, rintf, sqrtf, comparisons, selects and integer operations only, all
// correctly rounded, denormals kept, no FMA contraction (-ffp-contract=off and the pragma below).  The Philox
// block, u01 and the unit box_muller are vss_numerics.h's, shared with vss_perceive.hip and vss_step.hip.  The
// result equals the reference bit for bit (tests/test_actuate_gpu.py, closed loop included).
//
//   one field per lane: the lane loops over its n_teams * robots commands with 8-byte loads and stores.  The
//   field's draws are therefore computed once (the perception channel computes them up to six times), episode[f]
//   is read and written by the same lane (no cross-lane hazard), and nothing goes through LDS.
//
//   All of a lane's loads -- done_prev, episode, its commands, held, gain -- are issued before the draws, whose
//   arithmetic covers their latency; the stores follow the draws.  A lane reads every command of its field before
//   it writes one, and no two lanes share a command, so out == cmd (in place) is safe.
//
//   Only the Philox blocks whose entities are present are computed (block q holds the normals of entities 2 q and
//   2 q + 1): SA needs one, a team of three two, both teams three.  The loss block is computed only for
//   loss_prob > 0 and the gain draws only by the lanes whose field begins an episode.  Entities are picked from
//   the blocks' words with selects, not by indexing: an array indexed by a run-time value goes to scratch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vss.h"
#include "vss_numerics.h"

#pragma clang fp contract(off)

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "vss_actuate.hip targets gfx950 (CDNA4) only"
#endif

namespace vact {

using namespace vnum;
using namespace vnum::host;

constexpr int kBlock = 256;              // fields per workgroup (four waves)
constexpr uint32_t kPurposeStep = 8u;    // the Philox counter's purpose byte: per-step draws (noise, loss)
constexpr uint32_t kPurposeEpisode = 9u;  // per-episode draws (gains); 0..6 are the step's, 7 perception's
constexpr uint32_t kLossBlock = 3u;

struct Args {
  int64_t n_fields, field_stride, team_stride, done_stride;
  int32_t first_team, levels;
  float gain_sigma, noise_sigma, deadband, loss_prob;
  uint32_t k0, k1, call;
  const float* cmd;
  const int64_t* done;
  float* held;
  float* gain;
  uint32_t* episode;
  float* out;
};

// the entity of command j = b * ROBOTS + k: 0..2 blue, 3..5 yellow
template <int ROBOTS>
__device__ __forceinline__ int entity_of(int j, int first_team) {
  return 3 * (first_team ^ (j / ROBOTS)) + j % ROBOTS;
}

// The unit normals of the lane's commands: z[j] = (left, right) of entity e = pair e of the counter
// (field, c1, purpose << 24, block): words (w0, w1) of block e / 2 for an even e, (w2, w3) for an odd one.
template <int ROBOTS, int TEAMS>
__device__ __forceinline__ void draw_normals(float2 z[ROBOTS * TEAMS], uint32_t k0, uint32_t k1, uint32_t field, uint32_t c1,
                                             uint32_t purpose, int first_team) {
  constexpr int C = ROBOTS * TEAMS;
  uint32_t w[3][4];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    bool need = false;  // uniform: first_team is a kernel argument
#pragma unroll
    for (int j = 0; j < C; ++j) need = need || (entity_of<ROBOTS>(j, first_team) >> 1) == q;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[q][i] = 0u;
    if (need) philox(k0, k1, field, c1, purpose << 24, (uint32_t)q, w[q]);
  }
#pragma unroll
  for (int j = 0; j < C; ++j) {
    const int e = entity_of<ROBOTS>(j, first_team);
    const uint32_t wa = e == 0 ? w[0][0] : e == 1 ? w[0][2] : e == 2 ? w[1][0] : e == 3 ? w[1][2] : e == 4 ? w[2][0] : w[2][2];
    const uint32_t wb = e == 0 ? w[0][1] : e == 1 ? w[0][3] : e == 2 ? w[1][1] : e == 3 ? w[1][3] : e == 4 ? w[2][1] : w[2][3];
    box_muller(wa, wb, z[j].x, z[j].y);
  }
}

struct Wheel { float r, G, o; };  // held', gain', out

// one wheel, reference_actuate's lines in order
__device__ __forceinline__ Wheel wheel(float u, float held, float gain, bool fresh, bool lost, float zg, float zn, const Args& a,
                                       float L) {
  float G = gain;
  if (fresh) {
    G = 1.0f;
    if (a.gain_sigma != 0.0f) {
      const float zc = zg < -3.0f ? -3.0f : (zg > 3.0f ? 3.0f : zg);
      const float t = a.gain_sigma * zc;
      G = 1.0f + t;
    }
  }
  const float H = fresh ? 0.0f : held;
  const float c = u < -1.0f ? -1.0f : (u > 1.0f ? 1.0f : u);
  float q = c;
  if (a.levels > 0) {
    const float s = c * L;
    const float n = rintf(s);
    q = n / L;
  }
  const float r = lost ? H : q;
  const float m = (a.deadband > 0.0f && fabsf(r) < a.deadband) ? 0.0f : r;
  const float g = m * G;
  float o = g;
  if (a.noise_sigma != 0.0f) {
    const float t = a.noise_sigma * zn;
    o = g + t;
  }
  Wheel out;
  out.r = r; out.G = G; out.o = o;
  return out;
}

template <int ROBOTS, int TEAMS>
__global__ __launch_bounds__(kBlock) void actuate_kernel(const Args a) {
  constexpr int C = ROBOTS * TEAMS;  // commands per field
  const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= a.n_fields) return;
  const float2* cmd = reinterpret_cast<const float2*>(a.cmd);
  float2* out = reinterpret_cast<float2*>(a.out);
  float2* held = reinterpret_cast<float2*>(a.held);
  float2* gain = reinterpret_cast<float2*>(a.gain);

  // ---- loads ----
  int64_t done = 1;  // the start call: every field begins an episode
  if (a.done != nullptr) done = a.done[f * a.done_stride];
  uint32_t ep = a.episode[f];
  float2 u[C], h[C], g[C];
  int64_t at[C], packed[C];
#pragma unroll
  for (int j = 0; j < C; ++j) {
    const int b = j / ROBOTS, k = j % ROBOTS;
    at[j] = (int64_t)b * a.team_stride + f * a.field_stride + k;
    packed[j] = ((int64_t)b * a.n_fields + f) * ROBOTS + k;  // (n_teams, n_fields, robots)
    u[j] = cmd[at[j]];
    h[j] = held[packed[j]];
    g[j] = gain[packed[j]];
  }
  const bool fresh = done != 0;
  ep += fresh ? 1u : 0u;

  // ---- the field's draws ----
  float2 zn[C], zg[C];
#pragma unroll
  for (int j = 0; j < C; ++j) zn[j] = zg[j] = make_float2(0.0f, 0.0f);
  if (a.noise_sigma != 0.0f) draw_normals<ROBOTS, TEAMS>(zn, a.k0, a.k1, (uint32_t)f, a.call, kPurposeStep, a.first_team);
  bool lost0 = false, lost1 = false;  // blue's packet, yellow's
  if (a.loss_prob > 0.0f) {
    uint32_t w[4];
    philox(a.k0, a.k1, (uint32_t)f, a.call, kPurposeStep << 24, kLossBlock, w);
    lost0 = u01(w[0]) < a.loss_prob;
    lost1 = u01(w[1]) < a.loss_prob;
  }
  if (fresh && a.gain_sigma != 0.0f)
    draw_normals<ROBOTS, TEAMS>(zg, a.k0, a.k1, (uint32_t)f, ep, kPurposeEpisode, a.first_team);

  // ---- the commands, then the stores ----
  const float L = (float)a.levels;
#pragma unroll
  for (int j = 0; j < C; ++j) {
    const bool lost = (a.first_team ^ (j / ROBOTS)) != 0 ? lost1 : lost0;
    const Wheel l = wheel(u[j].x, h[j].x, g[j].x, fresh, lost, zg[j].x, zn[j].x, a, L);
    const Wheel r = wheel(u[j].y, h[j].y, g[j].y, fresh, lost, zg[j].y, zn[j].y, a, L);
    held[packed[j]] = make_float2(l.r, r.r);
    gain[packed[j]] = make_float2(l.G, r.G);
    out[at[j]] = make_float2(l.o, r.o);
  }
  a.episode[f] = ep;
}

}  // namespace vact

extern "C" {

int vss_actuate(void* stream, int64_t n_fields, const vss_actuate_layout* lay, const vss_actuate_params* prm, uint64_t seed,
                uint32_t call, const float* cmd, const int64_t* done_prev, int64_t done_stride, float* held, float* gain,
                uint32_t* episode, float* out) {
  using namespace vact;
  if (!lay || !prm || !cmd || !held || !gain || !episode || !out) return VSS_E_ARG;
  if (misaligned(cmd, 8) || misaligned(out, 8) || misaligned(held, 8) || misaligned(gain, 8) || misaligned(done_prev, 8) ||
      misaligned(episode, 4))
    return VSS_E_ARG;
  // each comparison is false for a NaN
  if (!(prm->gain_sigma >= 0.0f && prm->gain_sigma <= 0.3f)) return VSS_E_ARG;
  if (!(prm->noise_sigma >= 0.0f && prm->noise_sigma <= 3.4028235e38f)) return VSS_E_ARG;
  if (!(prm->deadband >= 0.0f && prm->deadband <= 1.0f)) return VSS_E_ARG;
  if (!(prm->loss_prob >= 0.0f && prm->loss_prob < 1.0f)) return VSS_E_ARG;
  if (prm->levels < 0 || prm->levels > VSS_ACTUATE_MAX_LEVELS) return VSS_E_ARG;
  if ((lay->robots != 1 && lay->robots != 3) || (lay->n_teams != 1 && lay->n_teams != 2) ||
      (lay->first_team != 0 && lay->first_team != 1))
    return VSS_E_ARG;
  if (n_fields < 0 || lay->field_stride < lay->robots || (done_prev && done_stride < 1)) return VSS_E_ARG;
  // the state on itself or on the commands, by address (at any size)
  if ((void*)held == (void*)gain || (void*)held == (void*)episode || (void*)gain == (void*)episode ||
      (const void*)held == (const void*)cmd || (const void*)gain == (const void*)cmd || (const void*)episode == (const void*)cmd ||
      (void*)held == (void*)out || (void*)gain == (void*)out || (void*)episode == (void*)out)
    return VSS_E_ARG;
  if (n_fields == 0) return VSS_OK;

  const int64_t C = (int64_t)lay->robots * lay->n_teams;
  // sizes: the field index is a 32-bit counter word and the grid an unsigned x dimension; every byte offset stays
  // an int64 (8 bytes per command and per done flag)
  const int64_t kMaxCommands = INT64_MAX / 16;
  const int64_t m = n_fields - 1;
  if (n_fields > (int64_t)UINT32_MAX || n_fields > kMaxCommands / C || lay->field_stride > kMaxCommands / n_fields ||
      (done_prev && done_stride > (INT64_MAX / 8) / n_fields))
    return VSS_E_ARG;
  const int64_t block_span = m * lay->field_stride + lay->robots;  // commands one team block spans
  if (lay->n_teams == 2 && (lay->team_stride < block_span || lay->team_stride > kMaxCommands - block_span)) return VSS_E_ARG;
  const int64_t blocks = n_fields / kBlock + (n_fields % kBlock != 0);
  if (blocks > INT32_MAX) return VSS_E_ARG;
  const uint64_t span = (uint64_t)((lay->n_teams == 2 ? lay->team_stride : 0) + block_span) * 8;
  const uint64_t state_b = (uint64_t)(n_fields * C) * 8, ep_b = (uint64_t)n_fields * 4;
  const uint64_t done_b = done_prev ? (uint64_t)(m * done_stride + 1) * 8 : 0;
  if (out != cmd && overlap(out, span, cmd, span)) return VSS_E_ARG;
  const void* st[3] = {held, gain, episode};
  const uint64_t st_b[3] = {state_b, state_b, ep_b};
  const void* io[3] = {cmd, out, done_prev};
  const uint64_t io_b[3] = {span, span, done_b};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      if (overlap(st[i], st_b[i], io[j], io_b[j])) return VSS_E_ARG;
    for (int j = i + 1; j < 3; ++j)
      if (overlap(st[i], st_b[i], st[j], st_b[j])) return VSS_E_ARG;
  }

  Args a;
  a.n_fields = n_fields; a.field_stride = lay->field_stride; a.team_stride = lay->n_teams == 2 ? lay->team_stride : 0;
  a.done_stride = done_prev ? done_stride : 0; a.first_team = lay->first_team; a.levels = prm->levels;
  a.gain_sigma = prm->gain_sigma; a.noise_sigma = prm->noise_sigma; a.deadband = prm->deadband; a.loss_prob = prm->loss_prob;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.call = call;
  a.cmd = cmd; a.done = done_prev; a.held = held; a.gain = gain; a.episode = episode; a.out = out;
  const dim3 grid((unsigned)blocks), block(kBlock);
  hipStream_t s = (hipStream_t)stream;
  if (lay->robots == 1 && lay->n_teams == 1) hipLaunchKernelGGL((actuate_kernel<1, 1>), grid, block, 0, s, a);
  else if (lay->robots == 1) hipLaunchKernelGGL((actuate_kernel<1, 2>), grid, block, 0, s, a);
  else if (lay->n_teams == 1) hipLaunchKernelGGL((actuate_kernel<3, 1>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((actuate_kernel<3, 2>), grid, block, 0, s, a);
  return hipGetLastError() == hipSuccess ? VSS_OK : VSS_E_LAUNCH;
}

}  // extern "C"
