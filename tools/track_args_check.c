/* Host-side argument validation of vss_track (include/vss.h) as a stand-alone program for ASan + UBSan.
 * Every call below is rejected (or returns VSS_OK for a zero size) before any HIP call, so it runs on a
 * CPU-only machine; the pointers are fake, non-null and never dereferenced.  Build the host code of
 * vss_track.hip with the sanitizers and run (from the repository root):
 *
 *   O=tools/_build; mkdir -p $O; C=rsoccer-isaac-cleanrl_amd/csrc
 *   SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
 *   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off $SAN -c $C/vss_track.hip -o $O/tr.o
 *   hipcc -fsanitize=address,undefined -fno-sanitize-recover=undefined -g -x c tools/track_args_check.c \
 *         -x none $O/tr.o -o $O/track_args_check && $O/track_args_check
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
#define ROW ((uintptr_t)208)
#define E_ARG VSS_E_ARG
#define OK VSS_OK

typedef struct call_args {
  int64_t n;
  vss_track_layout lay;
  vss_track_params prm;
  int32_t delay;
  uintptr_t obs, term, done, hist, est, age, obs_out, term_out;
  int64_t done_stride;
  int null_lay, null_prm;
} call_args;

static call_args good(void) {
  call_args a = {64, {3, 0, 3, 1}, {0.2f, 0.5f, 0.5f, 0.03f, 0.5f}, 2, FAKE, FAKE + GAP, FAKE + 2 * GAP, FAKE + 3 * GAP,
                 FAKE + 4 * GAP, FAKE + 5 * GAP, FAKE + 6 * GAP, FAKE + 7 * GAP, 1, 0, 0};
  return a;
}

static int run(call_args a) {
  return vss_track(NULL, a.n, a.null_lay ? NULL : &a.lay, a.null_prm ? NULL : &a.prm, a.delay, 7u, (const float*)a.obs,
                   (const float*)a.term, (const int64_t*)a.done, a.done_stride, (float*)a.est, (float*)a.hist,
                   (int32_t*)a.age, (float*)a.obs_out, (float*)a.term_out);
}

int main(void) {
  call_args a;
  /* zero size: OK, no launch -- a step call, a start call, two teams, no delay and no ring, the longest delay */
  a = good(); a.n = 0; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.term = 0; a.term_out = 0; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.lay.n_teams = 2; a.lay.team_stride = 0; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.delay = 0; a.hist = 0; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.delay = VSS_TRACK_MAX_DELAY; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.lay.robots = 1; a.lay.field_stride = 1; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.prm.gain_team = 0.0f; a.prm.gain_opp = 1.0f; a.prm.gate_pos = 0.0f; a.prm.gate_vel = 3e38f; EXPECT(run(a), OK);
  /* null pointers, also at zero size; exactly one of term / term_out */
  for (int z = 0; z < 2; ++z) {
    a = good(); a.n = z ? 0 : 64; a.obs = 0; EXPECT(run(a), E_ARG);
    a = good(); a.n = z ? 0 : 64; a.done = 0; EXPECT(run(a), E_ARG);
    a = good(); a.n = z ? 0 : 64; a.age = 0; EXPECT(run(a), E_ARG);
    a = good(); a.n = z ? 0 : 64; a.est = 0; EXPECT(run(a), E_ARG);
    a = good(); a.n = z ? 0 : 64; a.obs_out = 0; EXPECT(run(a), E_ARG);
    a = good(); a.n = z ? 0 : 64; a.hist = 0; EXPECT(run(a), E_ARG);
    a = good(); a.n = z ? 0 : 64; a.null_lay = 1; EXPECT(run(a), E_ARG);
    a = good(); a.n = z ? 0 : 64; a.null_prm = 1; EXPECT(run(a), E_ARG);
    a = good(); a.n = z ? 0 : 64; a.term = 0; EXPECT(run(a), E_ARG);
    a = good(); a.n = z ? 0 : 64; a.term_out = 0; EXPECT(run(a), E_ARG);
  }
  /* gains outside [0, 1] or not finite; gates negative or not finite */
  {
    const float bad_gain[] = {-0.001f, 1.001f, 2.0f, NAN, INFINITY, -INFINITY};
    const float bad_gate[] = {-0.001f, NAN, INFINITY, -INFINITY};
    for (unsigned i = 0; i < sizeof bad_gain / sizeof *bad_gain; ++i)
      for (int z = 0; z < 2; ++z) {
        a = good(); a.n = z ? 0 : 64; a.prm.gain_team = bad_gain[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = z ? 0 : 64; a.prm.gain_opp = bad_gain[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = z ? 0 : 64; a.prm.gain_ball = bad_gain[i]; EXPECT(run(a), E_ARG);
      }
    for (unsigned i = 0; i < sizeof bad_gate / sizeof *bad_gate; ++i)
      for (int z = 0; z < 2; ++z) {
        a = good(); a.n = z ? 0 : 64; a.prm.gate_pos = bad_gate[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = z ? 0 : 64; a.prm.gate_vel = bad_gate[i]; EXPECT(run(a), E_ARG);
      }
  }
  /* alignment: rows and est 16 B, done and hist 8 B, age 4 B */
  for (uintptr_t off = 1; off < 16; ++off) {
    a = good(); a.obs += off; EXPECT(run(a), E_ARG);
    a = good(); a.term += off; EXPECT(run(a), E_ARG);
    a = good(); a.est += off; EXPECT(run(a), E_ARG);
    a = good(); a.obs_out += off; EXPECT(run(a), E_ARG);
    a = good(); a.term_out += off; EXPECT(run(a), E_ARG);
    if (off % 8) { a = good(); a.done += off; EXPECT(run(a), E_ARG); }
    if (off % 8) { a = good(); a.hist += off; EXPECT(run(a), E_ARG); }
    if (off % 4) { a = good(); a.age += off; EXPECT(run(a), E_ARG); }
  }
  /* an output on an input or on another output (192 rows of 208 B; a ring of 2 x 192 x 24 B; 192 ages) */
  {
    uintptr_t* outs[3];
    for (int i = 0; i < 3; ++i) {
#define OUTS outs[0] = &a.obs_out; outs[1] = &a.term_out; outs[2] = &a.est
      a = good(); OUTS; *outs[i] = a.obs; EXPECT(run(a), E_ARG);
      a = good(); OUTS; *outs[i] = a.term + 191 * ROW; EXPECT(run(a), E_ARG);
      a = good(); OUTS; *outs[i] = a.obs - 191 * ROW; EXPECT(run(a), E_ARG);
      a = good(); OUTS; *outs[i] = a.done + 16; EXPECT(run(a), E_ARG);
      a = good(); a.n = 0; OUTS; *outs[i] = a.obs; EXPECT(run(a), E_ARG);
#undef OUTS
    }
  }
  a = good(); a.term_out = a.obs_out; EXPECT(run(a), E_ARG);
  a = good(); a.term_out = a.obs_out + 191 * ROW; EXPECT(run(a), E_ARG);
  a = good(); a.est = a.obs_out; EXPECT(run(a), E_ARG);
  a = good(); a.est = a.term_out - 191 * ROW; EXPECT(run(a), E_ARG);
  a = good(); a.est = a.age; EXPECT(run(a), E_ARG);
  a = good(); a.hist = a.obs; EXPECT(run(a), E_ARG);
  a = good(); a.hist = a.term + 191 * ROW; EXPECT(run(a), E_ARG);
  a = good(); a.hist = a.obs_out - (2 * 192 * 24 - 8); EXPECT(run(a), E_ARG);
  a = good(); a.hist = a.est + 191 * ROW; EXPECT(run(a), E_ARG);
  a = good(); a.hist = a.done + 8; EXPECT(run(a), E_ARG);
  a = good(); a.age = a.obs + 4; EXPECT(run(a), E_ARG);
  a = good(); a.age = a.term_out - 191 * 4; EXPECT(run(a), E_ARG);
  a = good(); a.age = a.est + 191 * ROW + 204; EXPECT(run(a), E_ARG);
  a = good(); a.age = a.done + 8; EXPECT(run(a), E_ARG);
  a = good(); a.age = a.hist; EXPECT(run(a), E_ARG);
  a = good(); a.age = a.hist + 2 * 192 * 24 - 4; EXPECT(run(a), E_ARG);
  a = good(); a.n = 0; a.hist = a.term; EXPECT(run(a), E_ARG);
  a = good(); a.n = 0; a.est = a.done; EXPECT(run(a), E_ARG);
  /* the delay and the layout */
  {
    const int32_t bad_delay[] = {-1, 16, 100, INT32_MAX, INT32_MIN};
    const int32_t bad_robots[] = {0, 2, 4, -1, INT32_MAX}, bad_teams[] = {0, 3, -1, INT32_MIN};
    const int64_t bad_field[] = {2, 0, -3, INT64_MIN}, bad_team[] = {191, 0, -192, INT64_MIN, INT64_MAX}, bad_done[] = {0, -1, INT64_MIN};
    for (unsigned i = 0; i < sizeof bad_delay / sizeof *bad_delay; ++i) { a = good(); a.delay = bad_delay[i]; EXPECT(run(a), E_ARG); }
    for (unsigned i = 0; i < sizeof bad_robots / sizeof *bad_robots; ++i) { a = good(); a.lay.field_stride = 8; a.lay.robots = bad_robots[i]; EXPECT(run(a), E_ARG); }
    for (unsigned i = 0; i < sizeof bad_teams / sizeof *bad_teams; ++i) { a = good(); a.lay.team_stride = 192; a.lay.n_teams = bad_teams[i]; EXPECT(run(a), E_ARG); }
    for (unsigned i = 0; i < sizeof bad_field / sizeof *bad_field; ++i) { a = good(); a.lay.field_stride = bad_field[i]; EXPECT(run(a), E_ARG); }
    for (unsigned i = 0; i < sizeof bad_team / sizeof *bad_team; ++i) { a = good(); a.lay.n_teams = 2; a.lay.team_stride = bad_team[i]; EXPECT(run(a), E_ARG); }
    for (unsigned i = 0; i < sizeof bad_done / sizeof *bad_done; ++i) { a = good(); a.done_stride = bad_done[i]; EXPECT(run(a), E_ARG); }
    a = good(); a.lay.robots = 1; a.lay.field_stride = 0; EXPECT(run(a), E_ARG);
  }
  /* negative sizes; sizes whose grid or byte offsets do not fit */
  a = good(); a.n = -1; EXPECT(run(a), E_ARG);
  a = good(); a.n = INT64_MIN; EXPECT(run(a), E_ARG);
  a = good(); a.n = INT64_MAX; EXPECT(run(a), E_ARG);
  a = good(); a.n = (int64_t)1 << 60; EXPECT(run(a), E_ARG);
  a = good(); a.n = (int64_t)1 << 30; a.lay.field_stride = (int64_t)1 << 40; EXPECT(run(a), E_ARG);
  a = good(); a.lay.field_stride = INT64_MAX; EXPECT(run(a), E_ARG);
  a = good(); a.done_stride = INT64_MAX; EXPECT(run(a), E_ARG);
  a = good(); a.lay.n_teams = 2; a.lay.team_stride = (int64_t)1 << 62; EXPECT(run(a), E_ARG);
  a = good(); a.n = ((int64_t)1 << 31) * 300; a.lay.robots = 1; a.lay.field_stride = 1; EXPECT(run(a), E_ARG);
  if (failures) return 1;
  printf("track argument checks ok\n");
  return 0;
}
