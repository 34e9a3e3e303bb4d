/* vss_referee.h — the referee's C ABI (libvss_referee.so; csrc_referee/vss_referee.hip, vss_amd/referee.py,
 * DESIGN.md §24).
 *
 * Inside an episode a VSS match is stopped for a free ball (the ball is stuck), a penalty (two defenders in their own
 * goal area with the ball) and a goal kick (two attackers in it), and restarts from the matching placement.  One launch
 * per call, after the step and after the set plays, over the step's own state, dof velocities and observation rows:
 * per field three counters are advanced and, where one reaches its threshold, the field is placed again from a table
 * of three plays.  vss_amd/referee.py reference_referee is the specification; the kernel equals it bit for bit.
 *
 * The unit stands beside the core library as the set plays' does: this header, csrc_referee/ and libvss_referee.so.
 * It is written in the subset of C that vss_amd/cheader.py parses, and the Python binding is derived from it.
 */
#ifndef VSS_AMD_VSS_REFEREE_H
#define VSS_AMD_VSS_REFEREE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSS_REFEREE_ABI_VERSION 1
#define VSS_REFEREE_PLAYS 3   /* free ball, penalty, goal kick */
#define VSS_REFEREE_CODES 8   /* verdict codes, the length of counts */

/* error codes, as include/vss.h */
#define VSS_REFEREE_OK 0
#define VSS_REFEREE_E_ARG 1     /* a bad argument: nothing was launched */
#define VSS_REFEREE_E_LAUNCH 2  /* the kernel launch failed (hipGetLastError) */

/* One entity's anchor (m, rad) and the half-widths of its uniform jitter, as vss_setplay_entity.  Entities in order:
 * the ball, blue 0..2, yellow 0..2; blue attacks +x.  The ball's yaw and r_yaw are not read. */
typedef struct vss_referee_entity { float x, y, yaw, r_pos, r_yaw; } vss_referee_entity;

/* A play: seven entities, the ball's velocity and its jitter; written as blue's own piece in the +y half. */
typedef struct vss_referee_play { vss_referee_entity e[7]; float ball_vx, ball_vy, r_vel; } vss_referee_play;

/* play[0] the free ball, play[1] the penalty, play[2] the goal kick */
typedef struct vss_referee_table { vss_referee_play play[3]; } vss_referee_table;

/* stall_speed_sq: the ball counts as stuck while vx^2 + vy^2 is below it; area_x, area_y: a goal area is |x| > area_x
 * and |y| < area_y; stall_steps, area_steps: the steps a condition must hold for a call (0: that call is off);
 * max_stops: calls per episode (0: no cap). */
typedef struct vss_referee_params {
  float stall_speed_sq, area_x, area_y;
  int32_t stall_steps, area_steps, max_stops;
} vss_referee_params;

/* Observation rows to rewrite for a whistled field, as vss_setplay_view: strides in 52-float rows; the row of team
 * block b, field f, robot k is obs + (b * team_stride + f * field_stride + k) * 52 floats and is the view of robot k
 * of team first_team + b.  team_stride is read with two teams only.
 *   SA, CMA: 1, -, 1, 1, 0      DMA: 3, -, 3, 1, 0      opp_obs (N,3,52): 3, -, 3, 1, 1
 *   mirror: R, R N, R, 2, 0     FULL's (N,2,3,52): 6, 3, 3, 2, 0 */
typedef struct vss_referee_view {
  float* obs;
  int64_t field_stride, team_stride;
  int32_t robots, n_teams, first_team;
} vss_referee_view;

int vss_referee_abi_version(void);
const char* vss_referee_source_hash(void);

/* One call, one launch.  counters is (n_fields, 4) int32: stall, defend, attack, stops.  Per field f:
 *   done (done NULL: no field is done): the four counters = 0, verdict[f] = -1, nothing else is touched.
 *   otherwise, with the ball (bx, by, bvx, bvy) and the robots' positions of state (58, n_fields), VSS_CH_*:
 *     stall  = bvx^2 + bvy^2 < stall_speed_sq ? min(stall + 1, 1 << 30) : 0
 *     in_area = |bx| > area_x && |by| < area_y;  side = bx < 0 ? 0 : 1  (0: blue's own area);  a robot is inside
 *     when |x| > area_x && |y| < area_y && (x < 0) == (bx < 0);  def_n, att_n: the defending and the attacking
 *     team's robots inside
 *     defend = in_area && def_n >= 2 ? min(defend + 1, 1 << 30) : 0;  attack likewise with att_n
 *     while max_stops == 0 || stops < max_stops, the first that holds:
 *       area_steps > 0 && defend >= area_steps: a penalty for the attacking team   code 4 (blue's, side 1), 5
 *       area_steps > 0 && attack >= area_steps: a goal kick for the defending team code 6 (blue's, side 0), 7
 *       stall_steps > 0 && stall >= stall_steps: a free ball  code 0 (bx >= 0, by >= 0), 1 (by < 0), 2 (bx < 0), 3
 *   A whistled field is placed from its play as vss_setplay places one -- anchor + (2u - 1) r per entity, flip_y, then
 *   flip_x with the role swap, the yaw wrapped, (qz, qw) = sincos_small(yaw / 2) -- with the flips decided by the
 *   verdict (free ball: flip_x = bx < 0, flip_y = by < 0; penalty: flip_x = code 5; goal kick: flip_x = code 7,
 *   flip_y = by < 0) and the draws of Philox4x32-10, key (seed lo, seed hi), counter (f, call, 11 << 24, 1 + e) for
 *   entity e.  Written: its 58 state channels (robot velocities and yaw rates 0), its twelve floats of dof_vel
 *   (n_fields, 2, 3, 2) = +0.0, its rows in every view (own-action floats +0.0), stall = defend = attack = 0,
 *   stops += 1, verdict[f] = code, counts[code] += 1.  Every other field keeps its state, dof_vel and rows, gets its
 *   counters stored and verdict[f] = -1.
 *
 * VSS_REFEREE_E_ARG, before any HIP call: a null tab, prm, state, dof_vel or counters; views null with n_views > 0;
 * n_views outside 0..2; a view with a null obs, robots not 1 or 3, n_teams not 1 or 2, first_team + n_teams > 2,
 * first_team < 0, field_stride < robots, or with two teams blocks that overlap (team_stride neither a block's span
 * nor, with both teams inside one field stride as in FULL, robots <= team_stride <= field_stride - robots); obs,
 * dof_vel or counters not 16-B, done or counts not 8-B, state or verdict not 4-B aligned; done_stride < 1 with a done;
 * n_fields < 0; sizes whose grid or byte offsets overflow; an output (state, dof_vel, counters, a view's rows, counts,
 * verdict) whose byte range overlaps done's or another output's; parameters that vss_amd/referee.py Params.validate
 * refuses: a negative stall_steps, area_steps or max_stops, a stall_speed_sq that is negative or not finite, area_x
 * outside (0, 0.75), area_y outside (0, 0.65]; and a table that vss_amd/referee.py RefTable.validate refuses: per play
 * every entity rule of vss_setplay's table (a non-finite value, |anchor yaw| > pi, r_yaw outside [0, pi], a negative
 * radius, a robot with |x| + r_pos > 0.71 or |y| + r_pos > 0.61, a ball with |x| + r_pos > 0.75 or |y| + r_pos > 0.65,
 * two entities with |anchor distance| - sqrt(2) (r_i + r_j) < 0.08), and a free-ball or penalty play whose ball can
 * lie inside a goal area (|x| + r_pos > area_x and |y| - r_pos < area_y).  n_fields == 0: VSS_REFEREE_OK, no launch. */
int vss_referee(void* stream, int64_t n_fields, const vss_referee_table* tab, const vss_referee_params* prm,
                uint64_t seed, uint32_t call, const int64_t* done, int64_t done_stride, float* state, float* dof_vel,
                int32_t* counters, int32_t n_views, const vss_referee_view* views, int64_t* counts, int32_t* verdict);

#ifdef __cplusplus
}
#endif

#endif /* VSS_AMD_VSS_REFEREE_H */
