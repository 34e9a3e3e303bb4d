/* Host-side argument validation of vss_actuate (include/vss.h) as a stand-alone program for ASan + UBSan.
 * Every call below is rejected (or returns VSS_OK for a zero size) before any HIP call, so it runs on a
 * CPU-only machine; the pointers are fake, non-null and never dereferenced.  Build the host code of
 * vss_actuate.hip with the sanitizers and run (from the repository root):
 *
 *   O=tools/_build; mkdir -p $O; C=rsoccer-isaac-cleanrl_amd/csrc
 *   SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
 *   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off $SAN -c $C/vss_actuate.hip -o $O/ac.o
 *   hipcc -fsanitize=address,undefined -fno-sanitize-recover=undefined -g -x c tools/actuate_args_check.c \
 *         -x none $O/ac.o -o $O/actuate_args_check && $O/actuate_args_check
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
  vss_actuate_layout lay;
  vss_actuate_params prm;
  uintptr_t cmd, done, held, gain, episode, out;
  int64_t done_stride;
  int null_lay, null_prm;
} call_args;

static call_args good(void) {
  call_args a = {64, {3, 0, 3, 1, 0}, {0.0f, 0.0f, 0.0f, 0.0f, 0}, FAKE, FAKE + GAP, FAKE + 2 * GAP, FAKE + 3 * GAP,
                 FAKE + 4 * GAP, FAKE + 5 * GAP, 1, 0, 0};
  return a;
}

static int run(call_args a) {
  return vss_actuate(NULL, a.n, a.null_lay ? NULL : &a.lay, a.null_prm ? NULL : &a.prm, 1u, 0u, (const float*)a.cmd,
                     (const int64_t*)a.done, a.done_stride, (float*)a.held, (float*)a.gain, (uint32_t*)a.episode,
                     (float*)a.out);
}

int main(void) {
  call_args a;
  /* zero size: OK, no launch -- a step call, a start call, in place, two teams */
  a = good(); a.n = 0; EXPECT(run(a), VSS_OK);
  a = good(); a.n = 0; a.done = 0; EXPECT(run(a), VSS_OK);
  a = good(); a.n = 0; a.done = 0; a.done_stride = 0; EXPECT(run(a), VSS_OK);
  a = good(); a.n = 0; a.out = a.cmd; EXPECT(run(a), VSS_OK);
  a = good(); a.n = 0; a.lay.n_teams = 2; a.lay.team_stride = 0; EXPECT(run(a), VSS_OK);
  a = good(); a.n = 0; a.prm.gain_sigma = 0.3f; a.prm.noise_sigma = 5.0f; a.prm.deadband = 1.0f; a.prm.loss_prob = 0.999f;
  a.prm.levels = VSS_ACTUATE_MAX_LEVELS; EXPECT(run(a), VSS_OK);
  /* null pointers, also at zero size */
  for (int z = 0; z < 2; ++z) {
    a = good(); a.n = z ? 0 : 64; a.cmd = 0; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.n = z ? 0 : 64; a.held = 0; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.n = z ? 0 : 64; a.gain = 0; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.n = z ? 0 : 64; a.episode = 0; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.n = z ? 0 : 64; a.out = 0; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.n = z ? 0 : 64; a.null_lay = 1; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.n = z ? 0 : 64; a.null_prm = 1; EXPECT(run(a), VSS_E_ARG);
  }
  /* alignment: commands, state and done 8 B, episode 4 B */
  for (uintptr_t off = 1; off < 8; ++off) {
    a = good(); a.cmd += off; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.out += off; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.held += off; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.gain += off; EXPECT(run(a), VSS_E_ARG);
    a = good(); a.done += off; EXPECT(run(a), VSS_E_ARG);
    if (off % 4) { a = good(); a.episode += off; EXPECT(run(a), VSS_E_ARG); }
  }
  /* out partly on cmd; the state on itself, the commands or the done flags (192 robots of 8 B) */
  a = good(); a.out = a.cmd + 191 * 8; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.out = a.cmd - 191 * 8; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.out = a.cmd + 8; EXPECT(run(a), VSS_E_ARG);
  {
    uintptr_t* state[3];
    for (int i = 0; i < 3; ++i) {
      a = good(); state[0] = &a.held; state[1] = &a.gain; state[2] = &a.episode;
      *state[i] = a.cmd; EXPECT(run(a), VSS_E_ARG);
      a = good(); state[0] = &a.held; state[1] = &a.gain; state[2] = &a.episode;
      *state[i] = a.out + 190 * 8; EXPECT(run(a), VSS_E_ARG);
      a = good(); state[0] = &a.held; state[1] = &a.gain; state[2] = &a.episode;
      *state[i] = a.done + 8; EXPECT(run(a), VSS_E_ARG);
      a = good(); state[0] = &a.held; state[1] = &a.gain; state[2] = &a.episode;
      *state[i] = *state[(i + 1) % 3]; EXPECT(run(a), VSS_E_ARG);
      a = good(); a.n = 0; state[0] = &a.held; state[1] = &a.gain; state[2] = &a.episode;
      *state[i] = *state[(i + 1) % 3]; EXPECT(run(a), VSS_E_ARG);
    }
  }
  a = good(); a.gain = a.held + 191 * 8; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.episode = a.gain + 191 * 8 + 4; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.episode = a.done - 63 * 4; EXPECT(run(a), VSS_E_ARG);
  /* the parameters */
  {
    const float bad_gain[] = {-1e-9f, 0.31f, 1.0f, INFINITY, -INFINITY, NAN};
    const float bad_noise[] = {-1e-9f, -1.0f, INFINITY, -INFINITY, NAN};
    const float bad_band[] = {-1e-9f, 1.0001f, INFINITY, NAN};
    const float bad_loss[] = {-1e-9f, 1.0f, 1.5f, INFINITY, NAN};
    const int32_t bad_levels[] = {-1, 32768, INT32_MAX, INT32_MIN};
    for (unsigned i = 0; i < sizeof bad_gain / sizeof *bad_gain; ++i) { a = good(); a.prm.gain_sigma = bad_gain[i]; EXPECT(run(a), VSS_E_ARG); }
    for (unsigned i = 0; i < sizeof bad_noise / sizeof *bad_noise; ++i) { a = good(); a.prm.noise_sigma = bad_noise[i]; EXPECT(run(a), VSS_E_ARG); }
    for (unsigned i = 0; i < sizeof bad_band / sizeof *bad_band; ++i) { a = good(); a.prm.deadband = bad_band[i]; EXPECT(run(a), VSS_E_ARG); }
    for (unsigned i = 0; i < sizeof bad_loss / sizeof *bad_loss; ++i) { a = good(); a.prm.loss_prob = bad_loss[i]; EXPECT(run(a), VSS_E_ARG); }
    for (unsigned i = 0; i < sizeof bad_levels / sizeof *bad_levels; ++i) { a = good(); a.prm.levels = bad_levels[i]; EXPECT(run(a), VSS_E_ARG); }
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
  /* negative sizes; sizes whose grid, field counter or byte offsets do not fit */
  a = good(); a.n = -1; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.n = INT64_MIN; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.n = INT64_MAX; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.n = (int64_t)1 << 60; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.n = (int64_t)1 << 30; a.lay.field_stride = (int64_t)1 << 40; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.lay.field_stride = INT64_MAX; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.done_stride = INT64_MAX; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.lay.n_teams = 2; a.lay.team_stride = (int64_t)1 << 62; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.n = ((int64_t)1 << 31) * 70; a.lay.robots = 1; a.lay.field_stride = 1; EXPECT(run(a), VSS_E_ARG);
  a = good(); a.n = ((int64_t)1 << 32); a.lay.robots = 1; a.lay.field_stride = 1; EXPECT(run(a), VSS_E_ARG);
  if (failures) return 1;
  printf("actuate argument checks ok\n");
  return 0;
}
