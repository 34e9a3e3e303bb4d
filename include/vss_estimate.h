/* vss_estimate.h — the estimation channel: delayed observation rows rolled forward to the present with the
 * project's own drive model (libvss_estimate.so, csrc/estimate/vss_estimate.hip, vss_amd/estimate.py).
 *
 * A library of its own beside libvss_amd.so and libvss_actuate.so: include/vss.h, its 61 entry points and the other
 * libraries' source stamps are untouched.  The conventions are vss.h's: `stream` is a hipStream_t (NULL: the default
 * stream), every pointer is device memory, the return value is VSS_OK or a VSS_E_* code of vss.h, and nothing
 * synchronises.
 *
 * A row is the 52-float observation row of envs/vss.py compute_obs: ball x y vx vy [0:4]; own robot j at 4 + 9 j:
 * x y vx vy cos sin w aL aR; opponent j at 31 + 7 j: x y vx vy cos sin w.  A perceived row (vss_perceive) is the state
 * of `lead` control steps ago, but its six own-action floats (11, 12, 20, 21, 29, 30) are the current step's
 * commands.  One call turns each row into an estimate of the present: DESIGN.md §3's drive, damping and integration
 * steps, run `lead` times with the commands the row's team gave in the meantime (kept here, in `hist`), every row in
 * its own frame and independently of every other.  There are no contacts and no walls.
 * vss_amd/estimate.py reference_estimate is the specification; the kernel equals it bit for bit.
 */
#ifndef VSS_AMD_VSS_ESTIMATE_H
#define VSS_AMD_VSS_ESTIMATE_H

#include <stdint.h>

#include "vss.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSS_ESTIMATE_ABI_VERSION 1
#define VSS_ESTIMATE_MAX_DELAY 15

/* Where the rows lie, as vss_perceive_layout without first_team: strides in 52-float rows; the row of team block b,
 * field f, robot k is at base + (b * team_stride + f * field_stride + k) * 52 floats, in obs, term and both
 * outputs.  team_stride is read with two teams only.
 *   SA, CMA: 1, -, 1, 1      DMA, opp_obs (N,3,52): 3, -, 3, 1      mirror: R, R N, R, 2
 *   the blue rows of FULL's (N,2,3,52): 6, -, 3, 1 */
typedef struct vss_estimate_layout {
  int64_t field_stride;
  int64_t team_stride;
  int32_t robots;   /* 1 or 3 */
  int32_t n_teams;  /* 1 or 2 */
} vss_estimate_layout;

/* One call of the channel, one launch.  obs, term: the perceived rows of call index `call` (term NULL: the start call
 * of reset(): every age 0, obs_out = obs, no term_out).  done: the step's int64 done flags, one per field every
 * done_stride elements (not read by a start call).  hist: (delay, n_teams, n_fields, robots, 6) fp32, a ring of each
 * row's own-action floats, call t in slot t % delay (not touched for delay 0); age: (n_teams, n_fields, robots) int32,
 * per row, perception's recurrence.  Per row:
 *   d = min(age + 1, delay);  age' = done ? 0 : d
 *   term_out = term rolled forward d steps, obs_out = obs rolled forward age' steps (0 steps: a copy)
 *   hist[call % delay] = obs's own-action floats
 *
 * VSS_E_ARG, before any HIP call: a null lay, obs, done, age or obs_out; hist null with delay >= 1; exactly one of
 * term / term_out null; a row pointer not 16-B, done or hist not 8-B or age not 4-B aligned; an output (obs_out,
 * term_out, hist, age) whose byte range overlaps an input's or another output's; delay outside
 * 0..VSS_ESTIMATE_MAX_DELAY; robots not 1 or 3; n_teams not 1 or 2; field_stride < robots; with two teams a
 * team_stride smaller than a block's span; done_stride < 1; n_fields < 0; sizes whose grid or byte offsets overflow.
 * n_fields == 0: VSS_OK, no launch. */
int vss_estimate(void* stream, int64_t n_fields, const vss_estimate_layout* lay, int32_t delay, uint32_t call,
                 const float* obs, const float* term, const int64_t* done, int64_t done_stride, float* hist,
                 int32_t* age, float* obs_out, float* term_out);

int vss_estimate_abi_version(void);

/* The first 16 hex digits of sha256 over the files of csrc/estimate/Makefile's STAMPED line, as built. */
const char* vss_estimate_source_hash(void);

#ifdef __cplusplus
}
#endif

#endif /* VSS_AMD_VSS_ESTIMATE_H */
