// vss_scripted.hip — the scripted benchmark team in one launch (gfx950): vss_scripted_team of include/vss.h.
//
// A deterministic attacker / defender / keeper controller, a pure function of robot 0's observation row of
// each field: no state, no random draw.  vss_amd/scripted.py reference_actions is its specification -- float32,
// one operation per line -- and this file follows it line by line: only + - * /, sqrtf, fabsf, fminf / fmaxf,
// comparisons and selects, all correctly rounded (hipcc's default for fp32 / and sqrt), denormals kept, and no
// FMA contraction (-ffp-contract=off and the pragma below).  The result equals it bit for bit
// (tests/test_scripted_gpu.py, closed loop included).
//
//   one field per lane, 64-lane workgroups.  The controller needs 14 floats of the row: the ball's position and
//   the three own robots' positions and headings, all within the row's first 28 floats.  Each lane reads them
//   as seven 16-byte loads straight from its row (rows are 16-B aligned: obs is, and the field stride is a
//   multiple of 4 floats), all issued before the first use, and writes its six floats as three 8-byte stores.
//
//   Why not the step kernel's cooperative load through LDS: the lanes' rows are 624 or 1,248 B apart, so each of
//   the seven load instructions touches 64 different 128-B lines (the later ones hit the lines the first brought
//   in), where a cooperative copy -- seven adjacent lanes per row -- would touch about a fifth as many per
//   instruction.  That is a cost in address processing, not in bytes: either way the lines fetched are the one
//   or two that hold a row's first 112 B (the opponents' block, floats 31..51, is never fetched), and the
//   cooperative form adds an LDS round trip and a barrier in front of about 150 dependent flops.  The whole
//   input is 7 MB at 65,536 fields, four waves per CU: the kernel runs at launch latency, far from either the
//   HBM or the address-rate bound, so the simpler form is kept (profiles/scripted_bench.json).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vss.h"

#pragma clang fp contract(off)

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "vss_scripted.hip targets gfx950 (CDNA4) only"
#endif

namespace vscr {

constexpr int kWave = 64;

// controller 1's constants (vss_amd/scripted.py)
constexpr float kGoalX = 0.75f, kPush = 0.15f, kBehind = -0.10f, kLateral = 0.05f;
constexpr float kKeeperX = -0.69f, kKeeperY = 0.17f, kDefenderX = -0.30f, kDefenderY = 0.35f;
constexpr float kDefenderAttacks = -0.1f, kEps = 1e-6f, kSlow = 8.0f, kTurn = 1.2f;

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// scripted.py _attack_target
__device__ __forceinline__ void attack_target(float bx, float by, float px, float py, float& tx, float& ty) {
  const float gx = kGoalX - bx;
  const float gy = 0.0f - by;
  const float gn = sqrtf(gx * gx + gy * gy) + kEps;
  const float hx = gx / gn;
  const float hy = gy / gn;
  const float rx = px - bx;
  const float ry = py - by;
  const float along = rx * hx + ry * hy;
  const float lat = ry * hx - rx * hy;
  const float k = (along < 0.0f && fabsf(lat) < kLateral) ? kPush : kBehind;
  tx = bx + k * hx;
  ty = by + k * hy;
}

// scripted.py _go_to
__device__ __forceinline__ float2 go_to(float px, float py, float c, float s, float tx, float ty) {
  const float dx = tx - px;
  const float dy = ty - py;
  const float ef = dx * c + dy * s;
  const float el = dy * c - dx * s;
  const float dist = sqrtf(ef * ef + el * el) + kEps;
  const float sg = ef < 0.0f ? -1.0f : 1.0f;
  const float v = (sg * (fabsf(ef) / dist)) * fminf(1.0f, kSlow * dist);
  const float w = (kTurn * (sg * el)) / dist;
  return make_float2(clampf(v - w, -1.0f, 1.0f), clampf(v + w, -1.0f, 1.0f));
}

__global__ __launch_bounds__(kWave) void scripted_team_v1(int64_t n, const float* __restrict__ obs, int64_t obs_stride,
                                                          float* __restrict__ act, int64_t act_stride) {
  const int64_t f = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (f >= n) return;
  const float4* row = reinterpret_cast<const float4*>(obs + f * obs_stride);
  float4 q[7];  // floats 0..27: the ball and the own robots up to robot 2's heading
#pragma unroll
  for (int i = 0; i < 7; ++i) q[i] = row[i];
  const float bx = q[0].x, by = q[0].y;
  // own robot k at 4 + 9 k: x, y at +0, +1; cos, sin at +4, +5
  const float p0x = q[1].x, p0y = q[1].y, c0 = q[2].x, s0 = q[2].y;   // 4, 5, 8, 9
  const float p1x = q[3].y, p1y = q[3].z, c1 = q[4].y, s1 = q[4].z;   // 13, 14, 17, 18
  const float p2x = q[5].z, p2y = q[5].w, c2 = q[6].z, s2 = q[6].w;   // 22, 23, 26, 27

  float tx, ty;
  attack_target(bx, by, p0x, p0y, tx, ty);  // robot 0: the attacker
  const float2 a0 = go_to(p0x, p0y, c0, s0, tx, ty);

  attack_target(bx, by, p1x, p1y, tx, ty);  // robot 1: the defender, a second attacker while the ball is deep
  const bool home = !(bx < kDefenderAttacks);
  tx = home ? kDefenderX : tx;
  ty = home ? clampf(by, -kDefenderY, kDefenderY) : ty;
  const float2 a1 = go_to(p1x, p1y, c1, s1, tx, ty);

  const float2 a2 = go_to(p2x, p2y, c2, s2, kKeeperX, clampf(by, -kKeeperY, kKeeperY));  // robot 2: the keeper

  float2* out = reinterpret_cast<float2*>(act + f * act_stride);
  out[0] = a0;
  out[1] = a1;
  out[2] = a2;
}

inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace vscr

extern "C" {

int vss_scripted_team(void* stream, int64_t n_fields, int32_t version, const float* obs, int64_t obs_field_stride,
                      float* act, int64_t act_field_stride) {
  if (n_fields < 0 || version != VSS_SCRIPTED_VERSION) return VSS_E_ARG;
  if (!obs || !act || vscr::misaligned(obs, 16) || vscr::misaligned(act, 8)) return VSS_E_ARG;
  if (obs_field_stride < 52 || obs_field_stride % 4 != 0) return VSS_E_ARG;
  if (act_field_stride < 6 || act_field_stride % 2 != 0) return VSS_E_ARG;
  if (n_fields == 0) return VSS_OK;
  const int64_t blocks = n_fields / vscr::kWave + (n_fields % vscr::kWave != 0);
  // the float index f * stride stays an int64 byte offset; the grid an unsigned x dimension
  if (blocks > INT32_MAX || obs_field_stride > (INT64_MAX / 4) / n_fields || act_field_stride > (INT64_MAX / 4) / n_fields)
    return VSS_E_ARG;
  hipLaunchKernelGGL(vscr::scripted_team_v1, dim3((unsigned)blocks), dim3(vscr::kWave), 0, (hipStream_t)stream, n_fields,
                     obs, obs_field_stride, act, act_field_stride);
  return hipGetLastError() == hipSuccess ? VSS_OK : VSS_E_LAUNCH;
}

}  // extern "C"
