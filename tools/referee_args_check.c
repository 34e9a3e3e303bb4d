/* Host-side argument validation of vss_referee (include/vss.h) as a stand-alone program for ASan + UBSan.
 * Every call below is rejected (or returns VSS_OK for a zero size) before any HIP call, so it runs on a
 * CPU-only machine; the pointers are fake, non-null and never dereferenced.  Build the host code of
 * vss_referee.hip with the sanitizers and run (from the repository root):
 *
 *   O=tools/_build; mkdir -p $O; C=rsoccer-isaac-cleanrl_amd/csrc
 *   SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
 *   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off $SAN -c $C/vss_referee.hip -o $O/rf.o
 *   hipcc -fsanitize=address,undefined -fno-sanitize-recover=undefined -g -x c tools/referee_args_check.c \
 *         -x none $O/rf.o -o $O/referee_args_check && $O/referee_args_check
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
  vss_referee_table tab;
  vss_referee_params prm;
  uintptr_t done, state, dof, counters, counts, verdict;
  int64_t done_stride;
  int32_t n_views;
  vss_setplay_view view[2];
  int null_tab, null_prm, null_views;
} call_args;

/* the free ball, the penalty and the goal kick as blue's own piece in the +y half */
static const vss_setplay_entity FREE_BALL[7] = {{.375f, .4f, 0, 0, 0}, {.175f, .4f, 0, .01f, .2f}, {-.10f, 0, 0, .03f, .5f},
    {-.62f, .05f, 0, .02f, .5f}, {.575f, .4f, 3.1415927f, .01f, .2f}, {.45f, -.10f, 3.1415927f, .03f, .5f},
    {.66f, .05f, 3.1415927f, .02f, .5f}};
static const vss_setplay_entity PENALTY[7] = {{.375f, 0, 0, 0, 0}, {.28f, 0, 0, .01f, .3f}, {-.10f, .30f, 0, .03f, .5f},
    {-.10f, -.30f, 0, .03f, .5f}, {-.15f, .10f, 3.1415927f, .02f, .5f}, {-.15f, -.10f, 3.1415927f, .02f, .5f},
    {.68f, 0, 1.5707964f, .02f, .3f}};
static const vss_setplay_entity GOAL_KICK[7] = {{-.60f, .10f, 0, 0, 0}, {-.30f, .30f, 0, .03f, .5f}, {-.30f, -.30f, 0, .03f, .5f},
    {-.69f, .10f, 0, 0, .2f}, {0, 0, 3.1415927f, .03f, .5f}, {.20f, .30f, 3.1415927f, .03f, .5f},
    {.66f, 0, 3.1415927f, .02f, .5f}};

static call_args good(void) {
  call_args a = {0};
  a.n = 64;
  for (int e = 0; e < 7; ++e) { a.tab.play[0].e[e] = FREE_BALL[e]; a.tab.play[1].e[e] = PENALTY[e]; a.tab.play[2].e[e] = GOAL_KICK[e]; }
  a.prm.stall_speed_sq = 0.0025f; a.prm.area_x = 0.60f; a.prm.area_y = 0.35f;
  a.prm.stall_steps = 100; a.prm.area_steps = 20; a.prm.max_stops = 0;
  a.done = FAKE; a.state = FAKE + GAP; a.counts = FAKE + 4 * GAP; a.verdict = FAKE + 5 * GAP; a.dof = FAKE + 6 * GAP;
  a.counters = FAKE + 7 * GAP; a.done_stride = 1;
  a.n_views = 2;
  a.view[0].obs = (float*)(FAKE + 2 * GAP); a.view[0].field_stride = 1; a.view[0].robots = 1; a.view[0].n_teams = 1;
  a.view[1].obs = (float*)(FAKE + 3 * GAP); a.view[1].field_stride = 3; a.view[1].robots = 3; a.view[1].n_teams = 1;
  a.view[1].first_team = 1;
  return a;
}

static int run(call_args a) {
  return vss_referee(NULL, a.n, a.null_tab ? NULL : &a.tab, a.null_prm ? NULL : &a.prm, 7u, 3u, (const int64_t*)a.done,
                     a.done_stride, (float*)a.state, (float*)a.dof, (int32_t*)a.counters, a.n_views,
                     a.null_views ? NULL : a.view, (int64_t*)a.counts, (int32_t*)a.verdict);
}

int main(void) {
  call_args a;
  /* zero size: OK, no launch -- with a done mask and without, no views, no counts or verdict, FULL, a mirror, every call off */
  a = good(); a.n = 0; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.done = 0; a.done_stride = 0; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.n_views = 0; a.null_views = 1; a.counts = 0; a.verdict = 0; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.n_views = 1; a.view[0].field_stride = 6; a.view[0].team_stride = 3; a.view[0].robots = 3; a.view[0].n_teams = 2; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.n_views = 1; a.view[0].team_stride = 0; a.view[0].n_teams = 2; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.prm.stall_steps = a.prm.area_steps = 0; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.prm.stall_speed_sq = 0.0f; a.prm.max_stops = INT32_MAX; a.prm.area_y = 0.65f; EXPECT(run(a), OK);
  a = good(); a.n = 0; a.prm.area_x = 0.55f; EXPECT(run(a), OK); /* the goal kick's ball inside the area: no rule against it */
  for (int z = 0; z < 2; ++z) {
    const int64_t n = z ? 0 : 64;
    /* null pointers and the view count */
    a = good(); a.n = n; a.null_tab = 1; EXPECT(run(a), E_ARG);
    a = good(); a.n = n; a.null_prm = 1; EXPECT(run(a), E_ARG);
    a = good(); a.n = n; a.state = 0; EXPECT(run(a), E_ARG);
    a = good(); a.n = n; a.dof = 0; EXPECT(run(a), E_ARG);
    a = good(); a.n = n; a.counters = 0; EXPECT(run(a), E_ARG);
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
    /* the parameters, rule by rule */
    {
      const int32_t bad_steps[] = {-1, INT32_MIN};
      const float bad_sq[] = {-0.001f, NAN, INFINITY, -INFINITY}, bad_x[] = {0.0f, -0.6f, 0.75f, 1.0f, NAN, INFINITY, -INFINITY};
      const float bad_y[] = {0.0f, -0.35f, 0.66f, NAN, INFINITY, -INFINITY};
      for (unsigned i = 0; i < sizeof bad_steps / sizeof *bad_steps; ++i) {
        a = good(); a.n = n; a.prm.stall_steps = bad_steps[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.prm.area_steps = bad_steps[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.prm.max_stops = bad_steps[i]; EXPECT(run(a), E_ARG);
      }
      for (unsigned i = 0; i < sizeof bad_sq / sizeof *bad_sq; ++i) { a = good(); a.n = n; a.prm.stall_speed_sq = bad_sq[i]; EXPECT(run(a), E_ARG); }
      for (unsigned i = 0; i < sizeof bad_x / sizeof *bad_x; ++i) { a = good(); a.n = n; a.prm.area_x = bad_x[i]; EXPECT(run(a), E_ARG); }
      for (unsigned i = 0; i < sizeof bad_y / sizeof *bad_y; ++i) { a = good(); a.n = n; a.prm.area_y = bad_y[i]; EXPECT(run(a), E_ARG); }
    }
    /* the table, rule by rule */
    {
      const float bad_value[] = {NAN, INFINITY, -INFINITY};
      for (unsigned i = 0; i < sizeof bad_value / sizeof *bad_value; ++i) {
        a = good(); a.n = n; a.tab.play[1].e[3].x = bad_value[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[2].e[3].y = bad_value[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[0].e[6].yaw = bad_value[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[0].e[0].r_pos = bad_value[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[0].e[2].r_yaw = bad_value[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[1].ball_vx = bad_value[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[2].ball_vy = bad_value[i]; EXPECT(run(a), E_ARG);
        a = good(); a.n = n; a.tab.play[0].r_vel = bad_value[i]; EXPECT(run(a), E_ARG);
      }
      a = good(); a.n = n; a.tab.play[0].r_vel = -0.1f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[0].e[1].yaw = 3.2f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[0].e[1].yaw = -3.2f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[1].e[1].r_yaw = 3.2f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[2].e[1].r_yaw = -0.1f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[0].e[1].r_pos = -0.01f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[1].e[6].x = 0.70f; EXPECT(run(a), E_ARG);                   /* 0.70 + 0.02 > 0.71 */
      a = good(); a.n = n; a.tab.play[1].e[2].y = 0.59f; EXPECT(run(a), E_ARG);                   /* 0.59 + 0.03 > 0.61 */
      a = good(); a.n = n; a.tab.play[1].e[2].y = -0.59f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[2].e[0].x = -0.76f; EXPECT(run(a), E_ARG);                  /* the ball past the line */
      a = good(); a.n = n; a.tab.play[0].e[0].y = 0.66f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[1].e[1].x = 0.30f; EXPECT(run(a), E_ARG);                   /* 0.075 from the ball */
      a = good(); a.n = n; a.tab.play[1].e[5].y = 0.05f; EXPECT(run(a), E_ARG);                   /* two yellow robots 0.05 apart */
      /* a free ball or a penalty whose ball can lie inside a goal area (every other rule holds) */
      a = good(); a.n = n; a.tab.play[0].e[0].x = 0.62f; a.tab.play[0].e[0].y = 0.30f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.tab.play[0].e[0].x = 0.56f; a.tab.play[0].e[0].y = 0.20f; a.tab.play[0].e[0].r_pos = 0.05f; EXPECT(run(a), E_ARG);
      if (z) { a = good(); a.n = 0; a.tab.play[0].e[0].x = 0.54f; a.tab.play[0].e[0].y = 0.20f; a.tab.play[0].e[0].r_pos = 0.05f; EXPECT(run(a), OK); } /* just outside */
      a = good(); a.n = n; a.tab.play[1].e[0].x = 0.61f; a.tab.play[1].e[0].y = 0.20f; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.prm.area_x = 0.35f; a.prm.area_y = 0.50f; EXPECT(run(a), E_ARG);     /* the marks inside a huge area */
    }
    /* an output on done or on another output: pointer equality holds at any size */
    {
      uintptr_t* outs[5];
      for (int i = 0; i < 5; ++i) {
        a = good(); a.n = n;
        outs[0] = &a.state; outs[1] = &a.dof; outs[2] = &a.counters; outs[3] = &a.counts; outs[4] = &a.verdict;
        *outs[i] = a.done; EXPECT(run(a), E_ARG);
        for (int j = 0; j < 5; ++j) {
          if (j == i) continue;
          a = good(); a.n = n;
          outs[0] = &a.state; outs[1] = &a.dof; outs[2] = &a.counters; outs[3] = &a.counts; outs[4] = &a.verdict;
          *outs[i] = *outs[j]; EXPECT(run(a), E_ARG);
        }
        a = good(); a.n = n;
        outs[0] = &a.state; outs[1] = &a.dof; outs[2] = &a.counters; outs[3] = &a.counts; outs[4] = &a.verdict;
        *outs[i] = (uintptr_t)a.view[1].obs; EXPECT(run(a), E_ARG);
      }
      a = good(); a.n = n; a.view[0].obs = (float*)a.done; EXPECT(run(a), E_ARG);
      a = good(); a.n = n; a.view[1].obs = a.view[0].obs; EXPECT(run(a), E_ARG);
    }
  }
  /* alignment: rows, dof_vel and counters 16 B, done and counts 8 B, state and verdict 4 B */
  for (uintptr_t off = 1; off < 16; ++off) {
    a = good(); a.view[0].obs = (float*)((uintptr_t)a.view[0].obs + off); EXPECT(run(a), E_ARG);
    a = good(); a.view[1].obs = (float*)((uintptr_t)a.view[1].obs + off); EXPECT(run(a), E_ARG);
    a = good(); a.dof += off; EXPECT(run(a), E_ARG);
    a = good(); a.counters += off; EXPECT(run(a), E_ARG);
    if (off % 8) { a = good(); a.done += off; EXPECT(run(a), E_ARG); }
    if (off % 8) { a = good(); a.counts += off; EXPECT(run(a), E_ARG); }
    if (off % 4) { a = good(); a.state += off; EXPECT(run(a), E_ARG); }
    if (off % 4) { a = good(); a.verdict += off; EXPECT(run(a), E_ARG); }
  }
  /* overlapping ranges (64 fields: the state 64 x 58 x 4 B, dof_vel 64 x 48 B, counters 64 x 16 B, 64 and 192 rows of
   * 208 B, 8 counts, 64 verdicts) */
  a = good(); a.state = (uintptr_t)a.view[0].obs + 63 * ROW; EXPECT(run(a), E_ARG);
  a = good(); a.state = (uintptr_t)a.view[1].obs - (64 * 58 * 4 - 4); EXPECT(run(a), E_ARG);
  a = good(); a.view[1].obs = (float*)((uintptr_t)a.view[0].obs + 63 * ROW); EXPECT(run(a), E_ARG);
  a = good(); a.view[0].obs = (float*)((uintptr_t)a.view[1].obs + 191 * ROW); EXPECT(run(a), E_ARG);
  a = good(); a.verdict = a.state + 64 * 58 * 4 - 4; EXPECT(run(a), E_ARG);
  a = good(); a.verdict = (uintptr_t)a.view[1].obs + 16; EXPECT(run(a), E_ARG);
  a = good(); a.counts = a.verdict + 63 * 4 - 4; EXPECT(run(a), E_ARG);
  a = good(); a.counts = a.state - 56; EXPECT(run(a), E_ARG);
  a = good(); a.dof = a.state + 64 * 58 * 4 - 16; EXPECT(run(a), E_ARG);
  a = good(); a.dof = (uintptr_t)a.view[0].obs - (64 * 48 - 16); EXPECT(run(a), E_ARG);
  a = good(); a.counters = a.dof + 64 * 48 - 16; EXPECT(run(a), E_ARG);
  a = good(); a.counters = (uintptr_t)a.view[1].obs + 191 * ROW; EXPECT(run(a), E_ARG);
  a = good(); a.verdict = a.counters + 64 * 16 - 4; EXPECT(run(a), E_ARG);
  a = good(); a.counts = a.dof + 8; EXPECT(run(a), E_ARG);
  a = good(); a.done = a.state + 8; EXPECT(run(a), E_ARG);
  a = good(); a.done = (uintptr_t)a.view[0].obs - 63 * 8; EXPECT(run(a), E_ARG);
  a = good(); a.done = a.verdict + 8; EXPECT(run(a), E_ARG);
  a = good(); a.done = a.counts + 56; EXPECT(run(a), E_ARG);
  a = good(); a.done = a.dof + 64 * 48 - 8; EXPECT(run(a), E_ARG);
  a = good(); a.done = a.counters - 63 * 8; EXPECT(run(a), E_ARG);
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
  printf("referee argument checks ok\n");
  return 0;
}
