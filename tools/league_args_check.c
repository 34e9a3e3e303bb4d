/* Host-side argument validation of the league entries (include/vss.h: vss_actor_forward_grouped,
 * vss_policy_sample_grouped, vss_match_tally) as a stand-alone program for ASan + UBSan.  Every call below is
 * rejected (or returns VSS_OK for zero rows) before any HIP call, so it runs on a CPU-only machine; the
 * pointers are fake, non-null and never dereferenced.  Build the two sources' host code with the sanitizers
 * and run (from the repository root):
 *
 *   O=tools/_build; mkdir -p $O; C=rsoccer-isaac-cleanrl_amd/csrc
 *   SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
 *   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 $SAN -c $C/vss_policy.hip -o $O/lp.o
 *   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off $SAN -c $C/vss_step.hip -o $O/ls.o
 *   hipcc -fsanitize=address,undefined -fno-sanitize-recover=undefined -g -x c tools/league_args_check.c \
 *         -x none $O/lp.o $O/ls.o -o $O/league_args_check && $O/league_args_check
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

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

static float* const FAKE = (float*)(uintptr_t)4096;
static float* const ODD = (float*)(uintptr_t)4100; /* 4-B aligned, not 16 */

static vss_actor_groups table(int32_t count, int64_t group_rows) {
  vss_actor_groups g;
  memset(&g, 0, sizeof g);
  g.count = count;
  g.group_rows = group_rows;
  for (int i = 0; i < VSS_MAX_ACTOR_GROUPS; ++i) {
    g.actor_packed[i] = FAKE;
    g.logstd[i] = FAKE;
  }
  return g;
}

int main(void) {
  vss_actor_groups g = table(4, 64);
  /* both grouped entries: the table, the row range, n_act */
  for (int which = 0; which < 2; ++which) {
#define CALL(rows, n_act, in, gp)                                                           \
  (which ? vss_policy_sample_grouped(NULL, (rows), (n_act), (in), (gp), 1, 1, FAKE)         \
         : vss_actor_forward_grouped(NULL, (rows), (n_act), (in), (gp), 1, 1, FAKE, FAKE))
    vss_actor_groups b;
    b = table(0, 64);   EXPECT(CALL(200, 2, FAKE, &b), VSS_E_ARG);
    b = table(17, 64);  EXPECT(CALL(17 * 64, 2, FAKE, &b), VSS_E_ARG);
    b = table(-1, 64);  EXPECT(CALL(200, 2, FAKE, &b), VSS_E_ARG);
    b = table(4, 0);    EXPECT(CALL(200, 2, FAKE, &b), VSS_E_ARG);
    b = table(4, 96);   EXPECT(CALL(4 * 96, 2, FAKE, &b), VSS_E_ARG);
    b = table(4, -64);  EXPECT(CALL(200, 2, FAKE, &b), VSS_E_ARG);
    b = table(16, INT64_MAX / 64 * 64); EXPECT(CALL(200, 2, FAKE, &b), VSS_E_ARG); /* no overflow in the range check */
    EXPECT(CALL(4 * 64 + 1, 2, FAKE, &g), VSS_E_ARG);
    EXPECT(CALL(3 * 64, 2, FAKE, &g), VSS_E_ARG);
    EXPECT(CALL(-1, 2, FAKE, &g), VSS_E_ARG);
    EXPECT(CALL(INT64_MAX, 2, FAKE, &g), VSS_E_ARG);
    EXPECT(CALL(200, 3, FAKE, &g), VSS_E_ARG);
    EXPECT(CALL(200, 2, NULL, &g), VSS_E_ARG);
    EXPECT(CALL(200, 2, FAKE, NULL), VSS_E_ARG);
    b = table(4, 64); b.logstd[3] = NULL; EXPECT(CALL(200, 2, FAKE, &b), VSS_E_ARG);
    EXPECT(CALL(0, 2, FAKE, &g), VSS_OK);
    EXPECT(CALL(0, 6, FAKE, &g), VSS_OK);
#undef CALL
  }
  /* the packed weights: read by the forward only */
  {
    vss_actor_groups b = table(4, 64);
    b.actor_packed[2] = NULL;
    EXPECT(vss_actor_forward_grouped(NULL, 200, 2, FAKE, &b, 1, 1, FAKE, FAKE), VSS_E_ARG);
    EXPECT(vss_policy_sample_grouped(NULL, 0, 2, FAKE, &b, 1, 1, FAKE), VSS_OK);
    b.actor_packed[2] = ODD;
    EXPECT(vss_actor_forward_grouped(NULL, 200, 2, FAKE, &b, 1, 1, FAKE, FAKE), VSS_E_ARG);
    b = table(3, 64);
    b.actor_packed[3] = NULL; /* entries >= count are unused */
    EXPECT(vss_actor_forward_grouped(NULL, 0, 2, FAKE, &b, 1, 1, FAKE, FAKE), VSS_OK);
  }
  /* the tally */
  const int64_t* D = (const int64_t*)FAKE;
  int64_t* T = (int64_t*)FAKE;
  EXPECT(vss_match_tally(NULL, 300, 2, 128, 3, FAKE, D, FAKE, T), VSS_E_ARG);
  EXPECT(vss_match_tally(NULL, 300, 1, 128, 2, FAKE, D, FAKE, T), VSS_E_ARG);
  EXPECT(vss_match_tally(NULL, 300, 3, 99, 3, FAKE, D, FAKE, T), VSS_E_ARG);
  EXPECT(vss_match_tally(NULL, 300, 1, 0, 3, FAKE, D, FAKE, T), VSS_E_ARG);
  EXPECT(vss_match_tally(NULL, 300, 1, -5, 3, FAKE, D, FAKE, T), VSS_E_ARG);
  EXPECT(vss_match_tally(NULL, 300, 1, 128, 0, FAKE, D, FAKE, T), VSS_E_ARG);
  EXPECT(vss_match_tally(NULL, 300, 1, 128, 17, FAKE, D, FAKE, T), VSS_E_ARG);
  EXPECT(vss_match_tally(NULL, -1, 1, 128, 3, FAKE, D, FAKE, T), VSS_E_ARG);
  EXPECT(vss_match_tally(NULL, INT64_MAX, 1, INT64_MAX, 16, FAKE, D, FAKE, T), VSS_E_ARG);
  EXPECT(vss_match_tally(NULL, 300, 1, 128, 3, NULL, D, FAKE, T), VSS_E_ARG);
  EXPECT(vss_match_tally(NULL, 300, 1, 128, 3, FAKE, NULL, FAKE, T), VSS_E_ARG);
  EXPECT(vss_match_tally(NULL, 300, 1, 128, 3, FAKE, D, NULL, T), VSS_E_ARG);
  EXPECT(vss_match_tally(NULL, 300, 1, 128, 3, FAKE, D, FAKE, NULL), VSS_E_ARG);
  EXPECT(vss_match_tally(NULL, 300, 1, 128, 3, ODD, D, FAKE, T), VSS_E_ARG);
  EXPECT(vss_match_tally(NULL, 300, 1, 128, 3, FAKE, D, FAKE, (int64_t*)ODD), VSS_E_ARG);
  EXPECT(vss_match_tally(NULL, 0, 1, 128, 3, FAKE, D, FAKE, T), VSS_OK);
  if (failures) return 1;
  printf("league argument checks ok\n");
  return 0;
}
