/* vss_setplay.h — the set plays' C ABI (libvss_setplay.so; csrc_setplay/vss_setplay.hip, vss_amd/setplay.py,
 * DESIGN.md §23).
 *
 * A share of the fields that finished an episode starts the next one from a named, table-driven placement -- a
 * kickoff, a free ball, a penalty ... -- with jitter and mirroring instead of the step's uniform drop: one launch
 * per call, after the step, over the step's own state and observation rows.  vss_amd/setplay.py reference_setplay
 * is the specification; the kernel equals it bit for bit.
 *
 * The unit stands beside the core library as the tracking channel's does: this header, csrc_setplay/ and
 * libvss_setplay.so.  It is written in the subset of C that vss_amd/cheader.py parses, and the Python binding is
 * derived from it.
 */
#ifndef VSS_AMD_VSS_SETPLAY_H
#define VSS_AMD_VSS_SETPLAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSS_SETPLAY_ABI_VERSION 1
#define VSS_SETPLAY_MAX_PLAYS 8

/* error codes, as include/vss.h */
#define VSS_SETPLAY_OK 0
#define VSS_SETPLAY_E_ARG 1     /* a bad argument: nothing was launched */
#define VSS_SETPLAY_E_LAUNCH 2  /* the kernel launch failed (hipGetLastError) */

/* One entity's anchor (m, rad) and the half-widths of its uniform jitter.  Entities in order: the ball, blue 0..2,
 * yellow 0..2; blue attacks +x.  The ball's yaw and r_yaw are not read. */
typedef struct vss_setplay_entity { float x, y, yaw, r_pos, r_yaw; } vss_setplay_entity;

/* A play: seven entities, the ball's velocity and its jitter, the cumulative weight up to and including this play
 * (float32 running sum, computed on the host) and the probabilities of the two mirrorings. */
typedef struct vss_setplay_play {
  vss_setplay_entity e[7];
  float ball_vx, ball_vy, r_vel, cum_weight, p_flip_x, p_flip_y;
} vss_setplay_play;

/* 1..VSS_SETPLAY_MAX_PLAYS plays; share in [0, 1]: the probability that a finished field is staged;
 * total_weight == play[count - 1].cum_weight > 0. */
typedef struct vss_setplay_table {
  int32_t count;
  float share, total_weight;
  vss_setplay_play play[VSS_SETPLAY_MAX_PLAYS];
} vss_setplay_table;

/* Observation rows to rewrite for a staged field, as vss_perceive_layout: strides in 52-float rows; the row of team
 * block b, field f, robot k is obs + (b * team_stride + f * field_stride + k) * 52 floats and is the view of robot k
 * of team first_team + b.  team_stride is read with two teams only.
 *   SA, CMA: 1, -, 1, 1, 0      DMA: 3, -, 3, 1, 0      opp_obs (N,3,52): 3, -, 3, 1, 1
 *   mirror: R, R N, R, 2, 0     FULL's (N,2,3,52): 6, 3, 3, 2, 0 */
typedef struct vss_setplay_view {
  float* obs;
  int64_t field_stride, team_stride;
  int32_t robots, n_teams, first_team;
} vss_setplay_view;

int vss_setplay_abi_version(void);
const char* vss_setplay_source_hash(void);

/* One call, one launch.  Per field f that is done (done NULL: the start call, every field), with the draws of
 * Philox4x32-10, key (seed lo, seed hi), counter (f, call, 10 << 24, block) -- see reference_setplay for the words:
 *   staged = u_share < share;   k = the first play with u_play * total_weight < cum_weight
 *   every entity at its anchor + (2u - 1) r, then flip_y (y, vy, yaw negated), then flip_x (the teams swapped,
 *   x, vx negated, yaw -> pi - yaw), the yaw wrapped into [-pi, pi], (qz, qw) = sincos_small(yaw / 2)
 * A staged field's 58 state channels (state is (58, n_fields), include/vss.h VSS_CH_*) and its rows in every view
 * are written -- the rows as vss_compute_observations gives them from that state with zero own-action floats --
 * chosen[f] = k and counts[k] += 1; every other field's state and rows stay and chosen[f] = -1.
 *
 * VSS_SETPLAY_E_ARG, before any HIP call: a null tab or state; views null with n_views > 0; n_views outside 0..2;
 * a view with a null obs, robots not 1 or 3, n_teams not 1 or 2, first_team + n_teams > 2, first_team < 0,
 * field_stride < robots, or with two teams blocks that overlap (team_stride neither a block's span nor, with both
 * teams inside one field stride as in FULL, robots <= team_stride <= field_stride - robots); obs not 16-B, done or counts
 * not 8-B, state or chosen not 4-B aligned; done_stride < 1 with a done; n_fields < 0; sizes whose grid or byte
 * offsets overflow; an output (state, a view's rows, counts, chosen) whose byte range overlaps done's or another
 * output's; and a table that vss_amd/setplay.py Table.validate refuses: a count outside 1..8, a non-finite value, a
 * share or flip probability outside [0, 1], cumulative weights that decrease, are negative or end at 0, or a
 * total_weight that is not the last of them, |anchor yaw| > pi, r_yaw outside [0, pi], a negative radius, a robot
 * with |x| + r_pos > 0.71 or |y| + r_pos > 0.61, a ball with |x| + r_pos > 0.75 or |y| + r_pos > 0.65, or two
 * entities with |anchor distance| - sqrt(2) (r_i + r_j) < 0.08.  n_fields == 0: VSS_SETPLAY_OK, no launch. */
int vss_setplay(void* stream, int64_t n_fields, const vss_setplay_table* tab, uint64_t seed, uint32_t call,
                const int64_t* done, int64_t done_stride, float* state, int32_t n_views,
                const vss_setplay_view* views, int64_t* counts, int32_t* chosen);

#ifdef __cplusplus
}
#endif

#endif /* VSS_AMD_VSS_SETPLAY_H */
