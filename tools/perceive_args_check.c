/* Host-side argument validation of vss_perceive (include/vss.h) as a stand-alone program for ASan + UBSan.
 * Every call below is rejected (or returns VSS_OK for a zero size) before any HIP call, so it runs on a
 * CPU-only machine; the pointers are fake, non-null and never dereferenced.  Build the host code of
 * vss_perceive.hip with the sanitizers and run (from the repository root):
 *
 *   O=tools/_build; mkdir -p $O; C=rsoccer-isaac-cleanrl_amd/csrc
 *   SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
 *   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off $SAN -c $C/vss_perceive.hip -o $O/pc.o
 *   hipcc -fsanitize=address,undefined -fno-sanitize-recover=undefined -g -x c tools/perceive_args_check.c \
 *         -x none $O/pc.o -o $O/perceive_args_check && $O/perceive_args_check
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../include/vss.h"

static int failures = 0;
#define EXPECT(call, want)                                                        \
  do {                                                                            \
    int rc_ = (call);                                                             \
    if (rc_ != (want)) {                                                          \
      printf("FAIL line %d: %s = %d, want %d\n", __LINE__, #call, rc_, (want)); \
      ++failures;                                                                 \
    }                                                                             \
  } while (0)

#define FAKE ((uintptr_t)1 << 20)
#define GAP ((uintptr_t)1 << 24) /* between two fake buffers: further than any extent of 64 fields */

typedef struct call_args {
  int64_t n;
  vss_perceive_layout lay;
  int32_t delay;
  vss_perceive_noise noise;
  uintptr_t obs, term, done, ring, age, obs_out, term_out;
  int64_t done_stride;
  int null_lay, null_noise;
} call_args;

static call_args good(void) {
  call_args a = {64, {3, 0, 3, 1, 0}, 2, {0.0f, 0.0f, 0.0f, 0.0f}, FAKE, FAKE + GAP, FAKE + 2 * GAP, FAKE + 3 * GAP,
                 FAKE + 5 * GAP, FAKE + 6 * GAP, FAKE + 7 * GAP, 1, 0, 0};
  return a;
}

static int run(call_args a) {
  return vss_perceive(NULL, a.n, a.null_lay ? NULL : &a.lay, a.delay, a.null_noise ? NULL : &a.noise, 1u, 0u,
                      (const float*)a.obs, (const float*)a.term, (const int64_t*)a.done, a.done_stride, (float*)a.ring,
                      (int32_t*)a.age, (float*)a.obs_out, (float*)a.term_out);
}

int main(void) {
  call_args a;
  /* zero size: OK, no launch -- a step call, a start call, two teams */
  a = good(); a.n = 0; EXPECT(run(a), VSS_OK);
  a = good(); a.n = 0; a.term = a.term_out = 0; EXPECT(run(a), VSS_OK);
  a = good(); a.n = 0; a.lay.n_teams = 2; a.lay.team_stride = 0; EXPECT(run(a), VSS_OK);
  /* null pointers, also at zero size */
  for (int z = 0; z < 2; ++z) {
    a = good(); a.n = z ? 0 : 64; a.obs = 0; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.n = z ? 0 : 64; a.done = 0; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.n = z ? 0 : 64; a.ring = 0; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.n = z ? 0 : 64; a.age = 0; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.n = z ? 0 : 64; a.obs_out = 0; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.n = z ? 0 : 64; a.null_lay = 1; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.n = z ? 0 : 64; a.null_noise = 1; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.n = z ? 0 : 64; a.term = 0; EXPECT(run(a), VSS_E_ARG);     /* exactly one of term / term_out */
    a = good(); a.n = z ? 0 : 64; a.term_out = 0; EXPECT(run(a), VSS_E_ARG);
  }
  /* alignment: rows 16 B, done 8 B, age 4 B */
  for (uintptr_t off = 1; off < 16; ++off) {
    a = good(); a.obs += off; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.term += off; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.ring += off; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.obs_out += off; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.term_out += off; EXPECT(run(a), VSS_E_ARG);
    if (off % 8) { a = good(); a.done += off; EXPECT(run(a), VSS_E_ARG); }
    if (off % 4) { a = good(); a.age += off; EXPECT(run(a), VSS_E_ARG); }
  }
  /* an output on an input or on another output: equal addresses and overlapping ranges (192 rows of 208 B) */
  a = good(); a.obs_out = a.obs; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.obs_out = a.term; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.term_out = a.obs; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.term_out = a.term; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.term_out = a.obs_out; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.ring = a.obs; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.ring = a.obs_out; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.obs_out = a.obs + 191 * 208; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.obs_out = a.obs - 191 * 208; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.ring = a.term_out + 16; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.age = a.done; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.n = 0; a.obs_out = a.obs; EXPECT(run(a), VSS_E_ARG);
  /* delay and the sigmas */
  {
    const int32_t bad_delay[] = {-1, 16, 100, INT32_MIN, INT32_MAX};
    const float bad_sigma[] = {-1e-9f, -1.0f, INFINITY, -INFINITY, NAN};
    for (unsigned i = 0; i < sizeof bad_delay / sizeof *bad_delay; ++i) { a = good(); a.delay = bad_delay[i]; EXPECT(run(a), VSS_E_ARG); }
    for (unsigned i = 0; i < sizeof bad_sigma / sizeof *bad_sigma; ++i) {
      a = good(); a.noise.pos = bad_sigma[i]; EXPECT(run(a), VSS_E_ARG);
      a = good(); a.noise.vel = bad_sigma[i]; EXPECT(run(a), VSS_E_ARG);
      a = good(); a.noise.ang = bad_sigma[i]; EXPECT(run(a), VSS_E_ARG);
      a = good(); a.noise.angvel = bad_sigma[i]; EXPECT(run(a), VSS_E_ARG);
    }
  }
  /* the layout */
  {
    const int32_t bad_robots[] = {0, 2, 4, -1, INT32_MAX}, bad_teams[] = {0, 3, -1, INT32_MIN}, bad_first[] = {-1, 2, 7};
    const int64_t bad_field[] = {2, 0, -3, INT64_MIN}, bad_team[] = {191, 0, -192, INT64_MIN, INT64_MAX}, bad_done[] = {0, -1, INT64_MIN};
    for (unsigned i = 0; i < sizeof bad_robots / sizeof *bad_robots; ++i) { a = good(); a.lay.field_stride = 8; a.lay.robots = bad_robots[i]; EXPECT(run(a), VSS_E_ARG); }
    for (unsigned i = 0; i < sizeof bad_teams / sizeof *bad_teams; ++i) { a = good(); a.lay.team_stride = 192; a.lay.n_teams = bad_teams[i]; EXPECT(run(a), VSS_E_ARG); }
    for (unsigned i = 0; i < sizeof bad_first / sizeof *bad_first; ++i) { a = good(); a.lay.first_team = bad_first[i]; EXPECT(run(a), VSS_E_ARG); }
    for (unsigned i = 0; i < sizeof bad_field / sizeof *bad_field; ++i) { a = good(); a.lay.field_stride = bad_field[i]; EXPECT(run(a), VSS_E_ARG); }
    for (unsigned i = 0; i < sizeof bad_team / sizeof *bad_team; ++i) { a = good(); a.lay.n_teams = 2; a.lay.team_stride = bad_team[i]; EXPECT(run(a), VSS_E_ARG); }
    for (unsigned i = 0; i < sizeof bad_done / sizeof *bad_done; ++i) { a = good(); a.done_stride = bad_done[i]; EXPECT(run(a), VSS_E_ARG); }
    a = good(); a.lay.robots = 1; a.lay.field_stride = 0; EXPECT(run(a), VSS_E_ARG);
  }
  /* negative sizes; sizes whose grid or byte offsets do not fit */
  a = good(); a.n = -1; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.n = INT64_MIN; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.n = INT64_MAX; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.n = (int64_t)1 << 60; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.n = (int64_t)1 << 40; a.lay.field_stride = (int64_t)1 << 30; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.lay.field_stride = INT64_MAX; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.done_stride = INT64_MAX; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.lay.n_teams = 2; a.lay.team_stride = (int64_t)1 << 62; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.n = ((int64_t)1 << 31) * 70; a.lay.robots = 1; a.lay.field_stride = 1; EXPECT(run(a), VSS_E_ARG);
  if (failures) return 1;
  printf("perceive argument checks ok\n");
  return 0;
}
