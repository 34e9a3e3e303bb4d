/* Host-side argument validation of vss_gae (include/vss.h) as a stand-alone program for ASan + UBSan.
 * Every call below is rejected (or returns VSS_OK for a zero size) before any HIP call, so it runs on a
 * CPU-only machine; the pointers are fake, non-null and never dereferenced.  Build the host code of
 * vss_returns.hip with the sanitizers and run (from the repository root):
 *
 *   O=tools/_build; mkdir -p $O; C=rsoccer-isaac-cleanrl_amd/csrc
 *   SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
 *   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off $SAN -c $C/vss_returns.hip -o $O/gr.o
 *   hipcc -fsanitize=address,undefined -fno-sanitize-recover=undefined -g -x c tools/gae_args_check.c \
 *         -x none $O/gr.o -o $O/gae_args_check && $O/gae_args_check
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

#define FAKE ((uintptr_t)4096)

/* the nine pointers in declaration order: rewards, values, next_values, term_values, v_last, next_dones,
 * next_timeouts, advantages, returns */
enum { REW, VAL, NV, TV, VL, DN, TO, ADV, RET, NPTR };

static int gae(int64_t T, int64_t E, const uintptr_t* p, float gamma, float gl) {
  return vss_gae(NULL, T, E, (const float*)p[REW], (const float*)p[VAL], (const float*)p[NV], (const float*)p[TV],
                 (const float*)p[VL], (const float*)p[DN], (const float*)p[TO], gamma, gl, (float*)p[ADV],
                 (float*)p[RET]);
}

/* form 0: A (next_values), form 1: B (term_values + v_last) */
static void form(int which, uintptr_t* p) {
  for (int i = 0; i < NPTR; ++i) p[i] = FAKE;
  if (which == 0) p[TV] = p[VL] = 0;
  else p[NV] = 0;
}

int main(void) {
  const float g = 0.99f, gl = 0.9405f;
  uintptr_t p[NPTR];
  for (int f = 0; f < 2; ++f) {
    form(f, p);
    /* zero sizes: OK, no launch */
    EXPECT(gae(0, 64, p, g, gl), VSS_OK);
    EXPECT(gae(8, 0, p, g, gl), VSS_OK);
    EXPECT(gae(0, 0, p, g, gl), VSS_OK);
    /* negative sizes */
    EXPECT(gae(-1, 64, p, g, gl), VSS_E_ARG);
    EXPECT(gae(8, -1, p, g, gl), VSS_E_ARG);
    EXPECT(gae(INT64_MIN, 64, p, g, gl), VSS_E_ARG);
    EXPECT(gae(-1, 0, p, g, gl), VSS_E_ARG);
    /* sizes whose element count or grid does not fit */
    EXPECT(gae(INT64_MAX, INT64_MAX, p, g, gl), VSS_E_ARG);
    EXPECT(gae(1, INT64_MAX, p, g, gl), VSS_E_ARG);
    EXPECT(gae(INT64_MAX, 2, p, g, gl), VSS_E_ARG);
    /* non-finite constants */
    EXPECT(gae(8, 64, p, NAN, gl), VSS_E_ARG);
    EXPECT(gae(8, 64, p, INFINITY, gl), VSS_E_ARG);
    EXPECT(gae(8, 64, p, g, NAN), VSS_E_ARG);
    EXPECT(gae(8, 64, p, g, -INFINITY), VSS_E_ARG);
    EXPECT(gae(0, 64, p, NAN, gl), VSS_E_ARG);
    /* each required pointer null; each present pointer off 4-B alignment */
    for (int i = 0; i < NPTR; ++i) {
      if (p[i] == 0) continue;
      form(f, p);
      p[i] = 0;
      EXPECT(gae(8, 64, p, g, gl), VSS_E_ARG);
      EXPECT(gae(0, 0, p, g, gl), VSS_E_ARG);
      for (uintptr_t off = 1; off < 4; ++off) {
        form(f, p);
        p[i] = FAKE + off;
        EXPECT(gae(8, 64, p, g, gl), VSS_E_ARG);
      }
      form(f, p);
    }
  }
  /* both forms, neither, and one of the form-B pair without the other */
  form(0, p); p[TV] = p[VL] = FAKE;  EXPECT(gae(8, 64, p, g, gl), VSS_E_ARG);
  form(0, p); p[NV] = 0;             EXPECT(gae(8, 64, p, g, gl), VSS_E_ARG);
  form(0, p); p[TV] = FAKE;          EXPECT(gae(8, 64, p, g, gl), VSS_E_ARG);
  form(0, p); p[VL] = FAKE;          EXPECT(gae(8, 64, p, g, gl), VSS_E_ARG);
  form(1, p); p[VL] = 0;             EXPECT(gae(8, 64, p, g, gl), VSS_E_ARG);
  form(1, p); p[TV] = 0;             EXPECT(gae(8, 64, p, g, gl), VSS_E_ARG);
  if (failures) return 1;
  printf("gae argument checks ok\n");
  return 0;
}
