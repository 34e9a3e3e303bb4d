/* Host-side argument validation of vss_step_mirror (include/vss.h) as a stand-alone program for ASan + UBSan.
 * Every call below is rejected (or returns VSS_OK for zero fields) before any HIP call, so it runs on a
 * CPU-only machine; the pointers are fake, non-null and never dereferenced.  Build the step source's host
 * code with the sanitizers and run (from the repository root):
 *
 *   O=tools/_build; mkdir -p $O; C=rsoccer-isaac-cleanrl_amd/csrc
 *   SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
 *   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off $SAN -c $C/vss_step.hip -o $O/ms.o
 *   hipcc -fsanitize=address,undefined -fno-sanitize-recover=undefined -g -x c tools/mirror_args_check.c \
 *         -x none $O/ms.o -o $O/mirror_args_check && $O/mirror_args_check
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

#define FAKE ((uintptr_t)4096)

static vss_params prm;
static vss_state st;

static vss_step_io blue(void) {
  vss_step_io io;
  io.actions = (const float*)FAKE; io.ou_buf = (float*)FAKE; io.obs = (float*)FAKE; io.terminal_obs = (float*)FAKE;
  io.rew = (float*)FAKE; io.reward_sum = (float*)FAKE; io.dones_rep = (int64_t*)FAKE; io.time_outs = (uint8_t*)FAKE;
  io.progress_f = (float*)FAKE;
  return io;
}

/* the yellow team's side with member `which` (declaration order, -1: none) at address `addr` */
static vss_mirror_io yellow(int which, uintptr_t addr) {
  uintptr_t a[8];
  for (int i = 0; i < 8; ++i) a[i] = i == which ? addr : FAKE;
  vss_mirror_io yl;
  yl.actions = (const float*)a[0]; yl.obs = (float*)a[1]; yl.terminal_obs = (float*)a[2]; yl.rew = (float*)a[3];
  yl.reward_sum = (float*)a[4]; yl.dones = (int64_t*)a[5]; yl.time_outs = (uint8_t*)a[6]; yl.progress_f = (float*)a[7];
  return yl;
}

int main(void) {
  memset(&prm, 0, sizeof prm);
  prm.clip_actions = 1.0f;
  prm.max_episode_length = 400;
  st.state = (float*)FAKE; st.progress_buf = (int64_t*)FAKE; st.reset_buf = (int64_t*)FAKE;
  st.dof_velocity_buf = (float*)FAKE; st.rng_counter = (uint32_t*)FAKE;
  vss_step_io io = blue();
  vss_mirror_io yl = yellow(-1, 0);
  if (sizeof(vss_mirror_io) != 64) { printf("FAIL: sizeof(vss_mirror_io) = %zu\n", sizeof(vss_mirror_io)); ++failures; }

  for (int32_t mode = VSS_MODE_SA; mode <= VSS_MODE_DMA; ++mode) {
    EXPECT(vss_step_mirror(NULL, 64, mode, &prm, &st, &io, NULL), VSS_E_ARG);
    EXPECT(vss_step_mirror(NULL, 64, mode, &prm, &st, NULL, &yl), VSS_E_ARG);
    EXPECT(vss_step_mirror(NULL, 64, mode, NULL, &st, &io, &yl), VSS_E_ARG);
    EXPECT(vss_step_mirror(NULL, 64, mode, &prm, NULL, &io, &yl), VSS_E_ARG);
    EXPECT(vss_step_mirror(NULL, -1, mode, &prm, &st, &io, &yl), VSS_E_ARG);
    EXPECT(vss_step_mirror(NULL, INT64_MAX, mode, &prm, &st, &io, &yl), VSS_E_ARG);
    for (int m = 0; m < 8; ++m) { /* each null member */
      vss_mirror_io b = yellow(m, 0);
      EXPECT(vss_step_mirror(NULL, 64, mode, &prm, &st, &io, &b), VSS_E_ARG);
    }
    /* misalignment: 8 B for actions and dones, 16 B for obs, terminal_obs and rew, 4 B for the float vectors */
    static const struct { int member; uintptr_t addr; } odd[] = {
        {0, 4100}, {5, 4100}, {1, 4104}, {2, 4104}, {3, 4104}, {4, 4098}, {7, 4098}};
    for (unsigned i = 0; i < sizeof odd / sizeof odd[0]; ++i) {
      vss_mirror_io b = yellow(odd[i].member, odd[i].addr);
      EXPECT(vss_step_mirror(NULL, 64, mode, &prm, &st, &io, &b), VSS_E_ARG);
    }
    /* the blue side: check_step_io's rules, and dones_rep in every mode */
    vss_step_io c = blue(); c.dones_rep = NULL;         EXPECT(vss_step_mirror(NULL, 64, mode, &prm, &st, &c, &yl), VSS_E_ARG);
    c = blue(); c.dones_rep = (int64_t*)(FAKE + 4);      EXPECT(vss_step_mirror(NULL, 64, mode, &prm, &st, &c, &yl), VSS_E_ARG);
    c = blue(); c.ou_buf = NULL;                         EXPECT(vss_step_mirror(NULL, 64, mode, &prm, &st, &c, &yl), VSS_E_ARG);
    c = blue(); c.reward_sum = NULL;                     EXPECT(vss_step_mirror(NULL, 64, mode, &prm, &st, &c, &yl), VSS_E_ARG);
    c = blue(); c.actions = (const float*)(FAKE + 4);    EXPECT(vss_step_mirror(NULL, 64, mode, &prm, &st, &c, &yl), VSS_E_ARG);
    c = blue(); c.obs = (float*)(FAKE + 8);              EXPECT(vss_step_mirror(NULL, 64, mode, &prm, &st, &c, &yl), VSS_E_ARG);
    EXPECT(vss_step_mirror(NULL, 0, mode, &prm, &st, &io, &yl), VSS_OK); /* nothing to do: no launch */
  }
  EXPECT(vss_step_mirror(NULL, 64, VSS_MODE_FULL, &prm, &st, &io, &yl), VSS_E_ARG);
  EXPECT(vss_step_mirror(NULL, 64, 7, &prm, &st, &io, &yl), VSS_E_ARG);
  EXPECT(vss_step_mirror(NULL, 64, -1, &prm, &st, &io, &yl), VSS_E_ARG);
  EXPECT(vss_step_mirror(NULL, 0, VSS_MODE_FULL, &prm, &st, &io, &yl), VSS_E_ARG);
  if (failures) return 1;
  printf("mirror argument checks ok\n");
  return 0;
}
