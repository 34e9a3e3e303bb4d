/* Host-side argument validation of vss_scripted_team (include/vss.h) as a stand-alone program for ASan + UBSan.
 * Every call below is rejected (or returns VSS_OK for a zero size) before any HIP call, so it runs on a
 * CPU-only machine; the pointers are fake, non-null and never dereferenced.  Build the host code of
 * vss_scripted.hip with the sanitizers and run (from the repository root):
 *
 *   O=tools/_build; mkdir -p $O; C=rsoccer-isaac-cleanrl_amd/csrc
 *   SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
 *   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off $SAN -c $C/vss_scripted.hip -o $O/sc.o
 *   hipcc -fsanitize=address,undefined -fno-sanitize-recover=undefined -g -x c tools/scripted_args_check.c \
 *         -x none $O/sc.o -o $O/scripted_args_check && $O/scripted_args_check
 */
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

#define FAKE ((uintptr_t)4096)

static int team(int64_t n, int32_t version, uintptr_t obs, int64_t obs_stride, uintptr_t act, int64_t act_stride) {
  return vss_scripted_team(NULL, n, version, (const float*)obs, obs_stride, (float*)act, act_stride);
}

int main(void) {
  const int32_t v = VSS_SCRIPTED_VERSION;
  /* zero size: OK, no launch, with both stride pairs */
  EXPECT(team(0, v, FAKE, 156, FAKE, 6), VSS_OK);
  EXPECT(team(0, v, FAKE, 312, FAKE, 12), VSS_OK);
  EXPECT(team(0, v, FAKE + 16, 52, FAKE + 8, 6), VSS_OK);
  /* null pointers, also at zero size */
  EXPECT(team(64, v, 0, 156, FAKE, 6), VSS_E_ARG);
  EXPECT(team(64, v, FAKE, 156, 0, 6), VSS_E_ARG);
  EXPECT(team(0, v, 0, 156, FAKE, 6), VSS_E_ARG);
  EXPECT(team(0, v, FAKE, 156, 0, 6), VSS_E_ARG);
  /* obs off 16-B, act off 8-B alignment */
  for (uintptr_t off = 1; off < 16; ++off) EXPECT(team(64, v, FAKE + off, 156, FAKE, 6), VSS_E_ARG);
  for (uintptr_t off = 1; off < 8; ++off) EXPECT(team(64, v, FAKE, 156, FAKE + off, 6), VSS_E_ARG);
  /* strides below the minimum or not a multiple of 4 / 2 */
  {
    const int64_t bad_obs[] = {51, 48, 0, -4, -156, 53, 54, 55, 157, 158, 159, INT64_MIN, INT64_MAX};
    const int64_t bad_act[] = {5, 4, 0, -2, -6, 7, 9, 13, INT64_MIN, INT64_MAX};
    for (unsigned i = 0; i < sizeof bad_obs / sizeof *bad_obs; ++i) EXPECT(team(64, v, FAKE, bad_obs[i], FAKE, 6), VSS_E_ARG);
    for (unsigned i = 0; i < sizeof bad_act / sizeof *bad_act; ++i) EXPECT(team(64, v, FAKE, 156, FAKE, bad_act[i]), VSS_E_ARG);
  }
  /* another controller version, also at zero size */
  EXPECT(team(64, 0, FAKE, 156, FAKE, 6), VSS_E_ARG);
  EXPECT(team(64, 2, FAKE, 156, FAKE, 6), VSS_E_ARG);
  EXPECT(team(64, -1, FAKE, 156, FAKE, 6), VSS_E_ARG);
  EXPECT(team(0, 2, FAKE, 156, FAKE, 6), VSS_E_ARG);
  /* negative sizes; sizes whose grid or byte offsets do not fit */
  EXPECT(team(-1, v, FAKE, 156, FAKE, 6), VSS_E_ARG);
  EXPECT(team(INT64_MIN, v, FAKE, 156, FAKE, 6), VSS_E_ARG);
  EXPECT(team(INT64_MAX, v, FAKE, 156, FAKE, 6), VSS_E_ARG);
  EXPECT(team((int64_t)1 << 40, v, FAKE, 156, FAKE, 6), VSS_E_ARG);
  EXPECT(team(1024, v, FAKE, (INT64_MAX / 4) & ~(int64_t)3, FAKE, 6), VSS_E_ARG);
  EXPECT(team(1024, v, FAKE, 156, FAKE, (INT64_MAX / 4) & ~(int64_t)1), VSS_E_ARG);
  if (failures) return 1;
  printf("scripted argument checks ok\n");
  return 0;
}
