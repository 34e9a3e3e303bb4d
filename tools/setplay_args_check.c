/* Host-side argument validation of vss_setplay (include/vss.h) as a stand-alone program for ASan + UBSan.
 * Every call below is rejected (or returns VSS_OK for a zero size) before any HIP call, so it runs on a
 * CPU-only machine; the pointers are fake, non-null and never dereferenced.  Build the host code of
 * vss_setplay.hip with the sanitizers and run (from the repository root):
 *
 *   O=tools/_build; mkdir -p $O; C=rsoccer-isaac-cleanrl_amd/csrc
 *   SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
 *   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off $SAN -c $C/vss_setplay.hip -o $O/sp.o
 *   hipcc -fsanitize=address,undefined -fno-sanitize-recover=undefined -g -x c tools/setplay_args_check.c \
 *         -x none $O/sp.o -o $O/setplay_args_check && $O/setplay_args_check
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
  vss_setplay_table tab;
  uintptr_t done, state, counts, chosen;
  int64_t done_stride;
  int32_t n_views;
  vss_setplay_view view[2];
  int null_tab, null_views;
} call_args;

/* the kickoff and a penalty, cumulative weights 1 and 3 */
static const vss_setplay_entity KICKOFF[7] = {{0, 0, 0, 0, 0}, {-0.10f, 0, 0, .01f, .2f}, {-0.35f, .25f, 0, .03f, .5f},
    {-0.62f, 0, 0, .02f, .5f}, {0.25f, 0, 3.1415927f, .02f, .5f}, {0.35f, -.25f, 3.1415927f, .03f, .5f},
    {0.62f, 0, 3.1415927f, .02f, .5f}};
static const vss_setplay_entity PENALTY[7] = {{.375f, 0, 0, 0, 0}, {.28f, 0, 0, .01f, .3f}, {-.10f, .30f, 0, .03f, .5f},
    {-.10f, -.30f, 0, .03f, .5f}, {-.15f, .10f, 3.1415927f, .02f, .5f}, {-.15f, -.10f, 3.1415927f, .02f, .5f},
    {.68f, 0, 1.5707964f, .02f, .3f}};

static call_args good(void) {
  call_args a = {0};
  a.n = 64;
  a.tab.count = 2; a.tab.share = 0.5f; a.tab.total_weight = 3.0f;
  for (int e = 0; e < 7; ++e) { a.tab.play[0].e[e] = KICKOFF[e]; a.tab.play[1].e[e] = PENALTY[e]; }
  a.tab.play[0].cum_weight = 1.0f; a.tab.play[1].cum_weight = 3.0f;
  a.tab.play[0].p_flip_x = a.tab.play[0].p_flip_y = 0.5f; a.tab.play[1].p_flip_x = 0.0f; a.tab.play[1].p_flip_y = 1.0f;
  a.done = FAKE; a.state = FAKE + GAP; a.counts = FAKE + 4 * GAP; a.chosen = FAKE + 5 * GAP; a.done_stride = 1;
  a.n_views = 2;
  a.view[0].obs = (float*)(FAKE + 2 * GAP); a.view[0].field_stride = 1; a.view[0].robots = 1; a.view[0].n_teams = 1;
  a.view[1].obs = (float*)(FAKE + 3 * GAP); a.view[1].field_stride = 3; a.view[1].robots = 3; a.view[1].n_teams = 1;
  a.view[1].first_team = 1;
  return a;
}

static int run(call_args a) {
  return vss_setplay(NULL, a.n, a.null_tab ? NULL : &a.tab, 7u, 3u, (const int64_t*)a.done, a.done_stride, (float*)a.state,
                     a.n_views, a.null_views ? NULL : a.view, (int64_t*)a.counts, (int32_t*)a.chosen);
}

int main(void) {
  call_args a;
  /* zero size: OK, no launch -- a step call, a start call, no views, no counts or chosen, FULL, a mirror, 8 plays */
  a = good(); a.n = 0; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.done = 0; a.done_stride = 0; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.n_views = 0; a.null_views = 1; a.counts = 0; a.chosen = 0; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.n_views = 1; a.view[0].field_stride = 6; a.view[0].team_stride = 3; a.view[0].robots = 3; a.view[0].n_teams = 2; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.n_views = 1; a.view[0].team_stride = 0; a.view[0].n_teams = 2; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.tab.count = 8; for (int k = 2; k < 8; ++k) a.tab.play[k] = a.tab.play[1]; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.tab.share = 0.0f; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.tab.share = 1.0f; a.tab.play[0].cum_weight = 0.0f; EXPECT(run(a), OK); /* a zero weight beside a positive one */
  for (int z = 0; z < 2; ++z) {
    const int64_t n = z ? 0 : 64;
    /* null pointers and the view count */
    a = good(); a.n = n; a.null_tab = 1; EXPECT(run(a), E_ARG);
    a = good(); a.n = n; a.state = 0; EXPECT(run(a), E_ARG);
    a = good(); a.n = n; a.null_views = 1; EXPECT(run(a), E_ARG);
    a = good(); a.n = n; a.view[1].obs = NULL; EXPECT(run(a), E_ARG);
    a = good(); a.n = n; a.n_views = 3; EXPECT(run(a), E_ARG);
    a = good(); a.n = n; a.n_views = -1; EXPECT(run(a), E_ARG);
    a = good(); a.n = n; a.n_views = INT32_MIN; EXPECT(run(a), E_ARG);
    /* the views' shapes */
    {
      const int32_t bad_robots[] = {0, 2, 4, -1, INT32_MAX}, bad_teams[] = {0, 3, -1, INT32_MIN}, bad_first[] = {2, -1, INT32_MAX, INT32_MIN};
      for (unsigned i = 0; i < sizeof bad_robots / sizeof *bad_robots; ++i) { a = good(); a.n = n; a.view[1].field_stride = 8; a.view[1].robots = bad_robots[i]; EXPECT(run(a), E_ARG); }
      for (unsigned i = 0; i < sizeof bad_teams / sizeof *bad_teams; ++i) { a = good(); a.n = n; a.view[0].n_teams = bad_teams[i]; EXPECT(run(a), E_ARG); }
      for (unsigned i = 0; i < sizeof bad_first / sizeof *bad_first; ++i) { a = good(); a.n = n; a.view[0].first_team = bad_first[i]; EXPECT(run(a), E_ARG); }
      a = good(); a.n = n; a.view[1].n_teams = 2; a.view[1].team_stride = 192; EXPECT(run(a), E_ARG); /* yellow first and two teams */
      a = good(); a.n = n; a.view[1].field_stride = 2; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.view[0].field_stride = 0; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.view[0].field_stride = INT64_MIN; EXPECT(run(a), E_ARG);
    }
    /* the table, rule by rule */
    {
      const float bad_unit[] = {-0.001f, 1.001f, 2.0f, NAN, INFINITY, -INFINITY};
      const float bad_value[] = {NAN, INFINITY, -INFINITY};
      const int32_t bad_count[] = {0, 9, -1, INT32_MAX, INT32_MIN};
      for (unsigned i = 0; i < sizeof bad_count / sizeof *bad_count; ++i) { a = good(); a.n = n; a.tab.count = bad_count[i]; EXPECT(run(a), E_ARG); }
      for (unsigned i = 0; i < sizeof bad_unit / sizeof *bad_unit; ++i) {
        a = good(); a.n = n; a.tab.share = bad_unit[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[0].p_flip_x = bad_unit[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[1].p_flip_y = bad_unit[i]; EXPECT(run(a), E_ARG);
      }
      for (unsigned i = 0; i < sizeof bad_value / sizeof *bad_value; ++i) {
        a = good(); a.n = n; a.tab.play[1].e[3].x = bad_value[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[1].e[3].y = bad_value[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[0].e[6].yaw = bad_value[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[0].e[0].r_pos = bad_value[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[0].e[2].r_yaw = bad_value[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[0].ball_vx = bad_value[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[0].ball_vy = bad_value[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[0].r_vel = bad_value[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[0].cum_weight = bad_value[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[1].cum_weight = a.tab.total_weight = bad_value[i]; EXPECT(run(a), E_ARG);
      }
      a = good(); a.n = n; a.tab.play[1].cum_weight = 0.5f; EXPECT(run(a), E_ARG);                 /* a negative weight */
      a = good(); a.n = n; a.tab.play[0].cum_weight = -1.0f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.total_weight = 2.0f; EXPECT(run(a), E_ARG);                      /* not the last cum */
      a = good(); a.n = n; a.tab.play[0].cum_weight = a.tab.play[1].cum_weight = a.tab.total_weight = 0.0f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[0].r_vel = -0.1f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[0].e[1].yaw = 3.2f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[0].e[1].yaw = -3.2f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[0].e[1].r_yaw = 3.2f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[0].e[1].r_yaw = -0.1f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[0].e[1].r_pos = -0.01f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[0].e[6].x = 0.70f; EXPECT(run(a), E_ARG);                   /* 0.70 + 0.02 > 0.71 */
      a = good(); a.n = n; a.tab.play[0].e[2].y = 0.59f; EXPECT(run(a), E_ARG);                   /* 0.59 + 0.03 > 0.61 */
      a = good(); a.n = n; a.tab.play[0].e[2].y = -0.59f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[0].e[0].x = 0.76f; EXPECT(run(a), E_ARG);                   /* the ball past the line */
      a = good(); a.n = n; a.tab.play[0].e[0].y = -0.66f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[0].e[1].x = -0.08f; EXPECT(run(a), E_ARG);                  /* 0.08 - sqrt(2) 0.01 < 0.08 */
      a = good(); a.n = n; a.tab.play[1].e[5].y = 0.05f; EXPECT(run(a), E_ARG);                   /* two yellow robots 0.05 apart */
    }
    /* an output on done or on another output: pointer equality holds at any size */
    a = good(); a.n = n; a.state = a.done; EXPECT(run(a), E_ARG);
    a = good(); a.n = n; a.chosen = a.done; EXPECT(run(a), E_ARG);
    a = good(); a.n = n; a.counts = a.done; EXPECT(run(a), E_ARG);
    a = good(); a.n = n; a.view[0].obs = (float*)a.done; EXPECT(run(a), E_ARG);
    a = good(); a.n = n; a.view[1].obs = a.view[0].obs; EXPECT(run(a), E_ARG);
    a = good(); a.n = n; a.view[1].obs = (float*)a.state; EXPECT(run(a), E_ARG);
    a = good(); a.n = n; a.counts = a.state; EXPECT(run(a), E_ARG);
    a = good(); a.n = n; a.chosen = a.counts; EXPECT(run(a), E_ARG);
  }
  /* alignment: rows 16 B, done and counts 8 B, state and chosen 4 B */
  for (uintptr_t off = 1; off < 16; ++off) {
    a = good(); a.view[0].obs = (float*)((uintptr_t)a.view[0].obs + off); EXPECT(run(a), E_ARG);
    a = good(); a.view[1].obs = (float*)((uintptr_t)a.view[1].obs + off); EXPECT(run(a), E_ARG);
    if (off % 8) { a = good(); a.done += off; EXPECT(run(a), E_ARG); }
    if (off % 8) { a = good(); a.counts += off; EXPECT(run(a), E_ARG); }
    if (off % 4) { a = good(); a.state += off; EXPECT(run(a), E_ARG); }
    if (off % 4) { a = good(); a.chosen += off; EXPECT(run(a), E_ARG); }
  }
  /* overlapping ranges (64 fields: the state 64 x 58 x 4 B, 64 and 192 rows of 208 B, 8 counts, 64 chosen) */
  a = good(); a.state = (uintptr_t)a.view[0].obs + 63 * ROW; EXPECT(run(a), E_ARG);
  a = good(); a.state = (uintptr_t)a.view[1].obs - (64 * 58 * 4 - 4); EXPECT(run(a), E_ARG);
  a = good(); a.view[1].obs = (float*)((uintptr_t)a.view[0].obs + 63 * ROW); EXPECT(run(a), E_ARG);
  a = good(); a.view[0].obs = (float*)((uintptr_t)a.view[1].obs + 191 * ROW); EXPECT(run(a), E_ARG);
  a = good(); a.chosen = a.state + 64 * 58 * 4 - 4; EXPECT(run(a), E_ARG);
  a = good(); a.chosen = (uintptr_t)a.view[1].obs + 16; EXPECT(run(a), E_ARG);
  a = good(); a.counts = a.chosen + 63 * 4 - 4; EXPECT(run(a), E_ARG);
  a = good(); a.counts = a.state - 56; EXPECT(run(a), E_ARG);
  a = good(); a.done = a.state + 8; EXPECT(run(a), E_ARG);
  a = good(); a.done = (uintptr_t)a.view[0].obs - 63 * 8; EXPECT(run(a), E_ARG);
  a = good(); a.done = a.chosen + 8; EXPECT(run(a), E_ARG);
  a = good(); a.done = a.counts + 56; EXPECT(run(a), E_ARG);
  /* strides */
  {
    const int64_t bad_done[] = {0, -1, INT64_MIN, INT64_MAX}, bad_team[] = {63, 0, -64, INT64_MIN, INT64_MAX, (int64_t)1 << 62};
    for (unsigned i = 0; i < sizeof bad_done / sizeof *bad_done; ++i) { a = good(); a.done_stride = bad_done[i]; EXPECT(run(a), E_ARG); }
    for (unsigned i = 0; i < sizeof bad_team / sizeof *bad_team; ++i) { a = good(); a.n_views = 1; a.view[0].n_teams = 2; a.view[0].team_stride = bad_team[i]; EXPECT(run(a), E_ARG); }
    /* both teams inside one field stride must not overlap there */
    a = good(); a.n_views = 1; a.view[0].robots = 3; a.view[0].n_teams = 2; a.view[0].field_stride = 6; a.view[0].team_stride = 4; EXPECT(run(a), E_ARG);
    a = good(); a.n_views = 1; a.view[0].robots = 3; a.view[0].n_teams = 2; a.view[0].field_stride = 6; a.view[0].team_stride = 2; EXPECT(run(a), E_ARG);
    a = good(); a.view[0].field_stride = INT64_MAX; EXPECT(run(a), E_ARG);
    a = good(); a.n = (int64_t)1 << 30; a.view[0].field_stride = (int64_t)1 << 40; EXPECT(run(a), E_ARG);
  }
  /* negative sizes; sizes whose grid or byte offsets do not fit */
  a = good(); a.n = -1; EXPECT(run(a), E_ARG);
  a = good(); a.n = INT64_MIN; EXPECT(run(a), E_ARG);
  a = good(); a.n = INT64_MAX; EXPECT(run(a), E_ARG);
  a = good(); a.n = (int64_t)1 << 60; EXPECT(run(a), E_ARG);
  a = good(); a.n = ((int64_t)1 << 31) * 300; a.n_views = 0; EXPECT(run(a), E_ARG);
  if (failures) return 1;
  printf("setplay argument checks ok\n");
  return 0;
}
