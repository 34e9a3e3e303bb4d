// vss_numerics.h — the one definition of the device numerics that the step and the three channels share, and of the
// channels' host-side pointer checks.
//
// The project's promise is kernel == float32 numpy specification == C oracle, bit for bit.  The draws (Philox4x32-10,
// the uniforms, Box-Muller) and the transcendental-free sin / cos / log below are on every side of it: vss_step.hip,
// vss_perceive.hip, vss_actuate.hip and vss_estimate.hip include this file, vss_amd/perceive.py
// (_philox .. _box_muller) states the same operations in numpy, one per line, and oracle/vss_oracle.c keeps a copy of
// its own on purpose: an oracle that shared text with what it checks would check nothing.  An edit here changes all
// four units at once, and the library's source stamp (this file is on the Makefile's STAMPED line).
//
// Everything is float32 with FMA contraction off: the pragma below covers this file's functions wherever they are
// inlined, and each including unit is compiled with -ffp-contract=off as well.  A unit pulls the device functions in
// with `using namespace vnum;` inside its own namespace, the channels also `using namespace vnum::host;`.
#ifndef VSS_NUMERICS_H
#define VSS_NUMERICS_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace vnum {

// Philox4x32-10: counter (c0..c3), key (k0, k1)
__device__ __forceinline__ void philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2,
                                       uint32_t c3, uint32_t out[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    // one 32 x 32 -> 64-bit product each (v_mad_u64_u32) instead of separate mul_hi / mul_lo
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// 24 bits to [0, 1) and to (0, 1]
__device__ __forceinline__ float u01(uint32_t x) { return (float)(x >> 8) * 5.9604645e-08f; }
__device__ __forceinline__ float u01_open0(uint32_t x) { return (float)((x >> 8) + 1u) * 5.9604645e-08f; }

__device__ __forceinline__ void sincos_poly(float r, float& s, float& c) {
  float r2 = r * r;
  s = r + r * r2 * (-0.16666667f + r2 * (0.008333334f + r2 * (-1.9841270e-4f + r2 * 2.7557319e-6f)));
  c = 1.0f + r2 * (-0.5f + r2 * (0.041666668f + r2 * (-1.3888889e-3f + r2 * (2.4801587e-5f + r2 * (-2.7557319e-7f)))));
}

__device__ __forceinline__ void sincos_small(float x, float& s, float& c) {
  if (fabsf(x) < 0.78f) {  // |x| < pi/4: no reduction (always the case for yaw steps)
    sincos_poly(x, s, c);
    return;
  }
  int k = (int)(x * 0.63661977f + (x >= 0.0f ? 0.5f : -0.5f));
  float kf = (float)k;
  float r = (x - kf * 1.5707964f) - kf * (-4.3711390e-8f);
  float sr, cr;
  sincos_poly(r, sr, cr);
  if (k == 0) { s = sr; c = cr; }
  else if (k == 1) { s = cr; c = -sr; }
  else if (k == -1) { s = -cr; c = sr; }
  else { s = -sr; c = -cr; }
}

// sin and cos of 2 pi u, u in [0, 1): by quadrant, the polynomial on [-pi/4, pi/4]
__device__ __forceinline__ void sincos_turn(float u, float& s, float& c) {
  float v = u * 4.0f;
  int q = (int)v;
  float t = v - (float)q;
  float r = (t - 0.5f) * 1.5707964f;
  float sr, cr;
  sincos_poly(r, sr, cr);
  float cp = (cr - sr) * 0.70710677f;
  float sp = (cr + sr) * 0.70710677f;
  if (q == 0) { c = cp; s = sp; }
  else if (q == 1) { c = -sp; s = cp; }
  else if (q == 2) { c = -cp; s = -sp; }
  else { c = sp; s = -cp; }
}

__device__ __forceinline__ float logf_poly(float x) {
  uint32_t u = __float_as_uint(x);
  int e = (int)((u >> 23) & 0xffu) - 127;
  float m = __uint_as_float((u & 0x7fffffu) | 0x3f800000u);
  if (m > 1.4142135f) { m = m * 0.5f; e = e + 1; }
  float s = (m - 1.0f) / (m + 1.0f);
  float s2 = s * s;
  float p = 2.0f + s2 * (0.6666667f + s2 * (0.4f + s2 * (0.2857143f + s2 * (0.22222222f + s2 * 0.18181819f))));
  return (float)e * 0.69314718f + s * p;
}

// a unit normal pair of two counter words (the step's box_muller_ou scales the same pair by the OU sigma)
__device__ __forceinline__ void box_muller(uint32_t w1, uint32_t w2, float& zc, float& zs) {
  const float u1 = u01_open0(w1), u2 = u01(w2);
  const float rad = sqrtf(-2.0f * logf_poly(u1));
  float sz, cz;
  sincos_turn(u2, sz, cz);
  zc = rad * cz;
  zs = rad * sz;
}

// ---- the channels' entry checks (host) --------------------------------------------------------------------------
namespace host {

inline bool misaligned(const void* p, uintptr_t al) { return (reinterpret_cast<uintptr_t>(p) & (al - 1)) != 0; }

// [p, p + bytes) and [q, q + bytes2) share a byte (a null pointer overlaps nothing)
inline bool overlap(const void* p, uint64_t bytes, const void* q, uint64_t bytes2) {
  if (!p || !q) return false;
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  if (a == b) return true;
  return a < b ? b - a < bytes : a - b < bytes2;
}

}  // namespace host
}  // namespace vnum

#endif  // VSS_NUMERICS_H
