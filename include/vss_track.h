/* vss_track.h — the tracking channel's C ABI (libvss_track.so; csrc_track/vss_track.hip, vss_amd/track.py,
 * DESIGN.md §22).
 *
 * A recursive tracker between perception and estimation: every perceived 52-float row (include/vss.h, the
 * perception channel) is filtered in its own frame across calls -- predicted one control step with the project's
 * drive model, then corrected with the new row by a fixed gain per kind of body, behind a position / velocity /
 * heading gate -- in one launch per call.  vss_amd/track.py reference_track is the specification; the kernel equals
 * it bit for bit.
 *
 * The channel is a unit of its own beside the core library: this header, csrc_track/ and libvss_track.so.  It is
 * written in the subset of C that vss_amd/cheader.py parses, and the Python binding is derived from it.
 */
#ifndef VSS_AMD_VSS_TRACK_H
#define VSS_AMD_VSS_TRACK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSS_TRACK_ABI_VERSION 1
#define VSS_TRACK_MAX_DELAY 15

/* error codes, as include/vss.h */
#define VSS_TRACK_OK 0
#define VSS_TRACK_E_ARG 1     /* a bad argument: nothing was launched */
#define VSS_TRACK_E_LAUNCH 2  /* the kernel launch failed (hipGetLastError) */

/* Where the rows lie, as vss_estimate_layout: strides in 52-float rows; the row of team block b, field f, robot k
 * is b * team_stride + f * field_stride + k.  team_stride is read only with two teams.
 *   SA, CMA: 1, -, 1, 1      DMA, opp_obs (N,3,52): 3, -, 3, 1      mirror: R, R N, R, 2
 *   the blue rows of FULL's (N,2,3,52): 6, -, 3, 1 */
typedef struct vss_track_layout {
  int64_t field_stride;
  int64_t team_stride;
  int32_t robots;   /* 1 or 3 */
  int32_t n_teams;  /* 1 or 2 */
} vss_track_layout;

/* The correction's gain per kind of body, each in [0, 1] (0: the kind is not filtered, its floats are the input's
 * bit for bit), and the gates in the row's units (0: off). */
typedef struct vss_track_params {
  float gain_team;  /* the three own robots, which the drive model moves */
  float gain_opp;   /* the three opponents, at constant velocity */
  float gain_ball;  /* the ball, damped */
  float gate_pos;   /* |z - p| in x or y beyond which a body is re-initialised from the input */
  float gate_vel;   /* the same in vx or vy */
} vss_track_params;

int vss_track_abi_version(void);
const char* vss_track_source_hash(void);

/* One call of the channel, one launch.  obs, term: the perceived rows of call index `call` (term NULL: the start
 * call -- every age 0, est = obs_out = obs, the ring's slot written).  State is the caller's, per row, packed
 * (n_teams, n_fields, robots): est (rows, 52) the last filtered row; age int32, perception's recurrence saturating
 * at delay; hist (delay, rows, 6) a ring of the row's own-action floats, call t in slot t % delay.  Per row, with
 * its field's done:
 *   a = clamp(age, 0, delay);  d = min(a + 1, delay);  age' = done ? 0 : d;  adv = 1 - (d - a)
 *   cmd = delay == 0 ? term's own-action floats : hist[(call - d) % delay]
 *   P = adv ? est moved one control step with cmd : est
 *   term_out = update(P, term);  obs_out = done ? obs : update(P, obs)
 *   est = obs_out;  age = age';  hist[call % delay] = obs's own-action floats
 *
 * VSS_TRACK_E_ARG, before any HIP call: a null lay, prm, obs, done, est, age or obs_out; hist null with delay >= 1;
 * exactly one of term / term_out null; a row pointer or est not 16-B, done or hist not 8-B or age not 4-B aligned;
 * an output (obs_out, term_out, est, hist, age) whose byte range overlaps an input's or another output's; delay
 * outside 0..VSS_TRACK_MAX_DELAY; a gain outside [0, 1] or not finite; a negative or non-finite gate; robots not 1
 * or 3; n_teams not 1 or 2; field_stride < robots; with two teams a team_stride smaller than a block's span;
 * done_stride < 1; n_fields < 0; sizes whose grid or byte offsets overflow.  n_fields == 0: VSS_TRACK_OK, no
 * launch. */
int vss_track(void* stream, int64_t n_fields, const vss_track_layout* lay, const vss_track_params* prm, int32_t delay,
              uint32_t call, const float* obs, const float* term, const int64_t* done, int64_t done_stride,
              float* est, float* hist, int32_t* age, float* obs_out, float* term_out);

#ifdef __cplusplus
}
#endif

#endif /* VSS_AMD_VSS_TRACK_H */
