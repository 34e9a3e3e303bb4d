/*
 * vss.h — C ABI of the MI355X-native VSS (IEEE Very Small Size, 3v3) match step.
 *
 * This is the drop-in boundary for the hot path named by BASELINE.json `north_star`:
 * the reference's `VSS.step` (envs/vss.py:180-333 + the Ext IsaacGymEnvs VecTask.step that
 * drives it, + PhysX `gym.simulate`) and the SA/CMA/DMA wrapper packing
 * (envs/wrappers.py:5-19,89-180).  The Python classes in
 * `rsoccer-isaac-cleanrl_amd/envs/{vss,wrappers}.py` bind these entry points with ctypes.
 *
 * Conventions:
 *   - every buffer is a caller-owned DEVICE allocation (torch tensors); the library allocates
 *     nothing and keeps no hidden state besides what is passed in;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); no host synchronisation;
 *   - return value 0 = ok, otherwise a VSS_E_* code (vss_error_string() describes it);
 *   - runtime parameters (reward weights, episode length, clip, seed) are passed per call.
 *
 * Field state layout (struct-of-arrays, fp32, `state[channel * n_fields + field]`), chosen so
 * the reference's tensor views (envs/vss.py:112-132) are plain strided views of one buffer:
 *   VSS_CH_BALL_X..VSS_CH_BALL_VY             ball x, y, vx, vy
 *   VSS_CH_RX + r, VSS_CH_RY + r               robot r position      (r = team*3 + robot)
 *   VSS_CH_RQX..VSS_CH_RQW + r                 robot r quaternion x,y,z,w (x,y unused: planar)
 *   VSS_CH_RVX + r, VSS_CH_RVY + r             robot r linear velocity
 *   VSS_CH_RW + r                              robot r yaw rate
 */
#ifndef VSS_AMD_VSS_H
#define VSS_AMD_VSS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSS_ABI_VERSION 2

#define VSS_NUM_TEAMS 2          /* envs/vss.py:24 */
#define VSS_NUM_ROBOTS 3         /* envs/vss.py:25 */
#define VSS_NUM_AGENTS 6
#define VSS_NUM_OBS 52           /* envs/vss.yaml:4, layout envs/vss.py:530-575 */
#define VSS_NUM_ACTIONS 2        /* envs/vss.yaml:5 (left wheel, right wheel) */
#define VSS_NUM_REW 4            /* goal, grad, move, energy: envs/vss.py:90-92 */

/* state channels */
#define VSS_CH_BALL_X 0
#define VSS_CH_BALL_Y 1
#define VSS_CH_BALL_VX 2
#define VSS_CH_BALL_VY 3
#define VSS_CH_RX 4
#define VSS_CH_RY 10
#define VSS_CH_RQX 16
#define VSS_CH_RQY 22
#define VSS_CH_RQZ 28
#define VSS_CH_RQW 34
#define VSS_CH_RVX 40
#define VSS_CH_RVY 46
#define VSS_CH_RW 52
#define VSS_STATE_CHANNELS 58

/* which wrapper the step is fused with (envs/wrappers.py:43-48) */
#define VSS_MODE_FULL 0  /* raw VSS.step: actions (N,2,3,2), obs (N,2,3,52), rew (N,2,3,4) */
#define VSS_MODE_SA 1    /* SingleAgent: learner = blue robot 0 (envs/wrappers.py:89-115)   */
#define VSS_MODE_CMA 2   /* CMA: learner = blue team, one 6-vector (envs/wrappers.py:118-148) */
#define VSS_MODE_DMA 3   /* DMA: learner = blue robots 0..2, one row each (wrappers.py:151-180) */

/* Alignment (checked; VSS_E_ARG otherwise): observation, reward, dof_velocity, OU and FULL /
 * rollout action buffers 16 B (float4 access); SA/CMA/DMA action buffers 8 B; int64 buffers 8 B;
 * packed MLP weights 16 B.  Allocator (hipMalloc / torch) pointers always qualify; a view at an
 * odd element offset may not. */

/* error codes */
#define VSS_OK 0
#define VSS_E_ARG 1      /* null or misaligned pointer / bad size / bad mode */
#define VSS_E_LAUNCH 2   /* kernel launch failed (hipGetLastError) */

typedef struct vss_params {
  float w_goal;              /* rew_weights.goal   envs/vss.yaml:9,  envs/vss.py:44 */
  float w_grad;              /* rew_weights.grad   envs/vss.yaml:10 */
  float w_move;              /* rew_weights.move   envs/vss.yaml:11 */
  float w_energy;            /* rew_weights.energy envs/vss.yaml:12 */
  float clip_actions;        /* env.clipActions    envs/vss.yaml:7 (Ext VecTask clamp) */
  int32_t max_episode_length;/* env.maxEpisodeLength envs/vss.yaml:6 */
  uint64_t seed;             /* Philox key for reset sampling and OU noise */
} vss_params;

typedef struct vss_state {
  float* state;              /* [VSS_STATE_CHANNELS][n_fields] fp32 SoA (see above)       */
  int64_t* progress_buf;     /* [n_fields]   envs/vss.py:95                               */
  int64_t* reset_buf;        /* [n_fields]   envs/vss.py:93                               */
  float* dof_velocity_buf;   /* [n_fields][2][3][2] last clamped actions, envs/vss.py:137  */
  uint32_t* rng_counter;     /* [n_fields]   per-field Philox step counter                */
} vss_state;

/*
 * Per-step inputs/outputs.  Shapes by mode (N = n_fields, R = 3 for DMA else 1):
 *   actions      FULL (N,2,3,2) | SA (N,2) | CMA (N,6) | DMA (3N,2)             read
 *   ou_buf       wrapper action buffer (N,2,3,2); SA/CMA/DMA only                 read+write
 *   obs          FULL (N,2,3,52) | SA/CMA (N,52) | DMA (3N,52)                     write
 *   terminal_obs same shape as obs (pre-reset observation)                        write
 *   rew          FULL (N,2,3,4) | SA/CMA (N,4) | DMA (3N,4)                        write
 *   reward_sum   SA/CMA (N,) | DMA (3N,) = rews.sum(-1); may be NULL in FULL       write
 *   dones_rep    DMA only: (3N,) int64 = dones.repeat_interleave(3); else NULL     write
 *   time_outs    (R*N,) uint8 (torch.bool)                                          write
 *   progress_f   (R*N,) fp32 = progress_buf.float() before the reset              write
 */
typedef struct vss_step_io {
  const float* actions;
  float* ou_buf;
  float* obs;
  float* terminal_obs;
  float* rew;
  float* reward_sum;
  int64_t* dones_rep;
  uint8_t* time_outs;
  float* progress_f;
} vss_step_io;

/*
 * Open-loop rollout buffers for vss_rollout (K = n_steps, N = n_fields), step-major:
 *   actions      (K,N,2,3,2) fp32                                                   read
 *   obs          (K,N,2,3,52), terminal_obs (K,N,2,3,52), rew (K,N,2,3,4) fp32      write
 *   dones        (K,N) int64 = reset_buf after each step                            write
 *   time_outs    (K,N) uint8, progress_f (K,N) fp32                                 write
 */
typedef struct vss_rollout_io {
  const float* actions;
  float* obs;
  float* terminal_obs;
  float* rew;
  int64_t* dones;
  uint8_t* time_outs;
  float* progress_f;
} vss_rollout_io;

/*
 * Recorded random draws for the parity entries vss_step_replay / vss_reset_dones_replay: the
 * reference's own torch draws, so the product kernels can be run against golden fixtures made by
 * the reference (tests/golden/) instead of the Philox stream.  Per field f, row
 * uniforms[f * uniform_stride ...] holds the draws the reference's reset_dones consumed for f in
 * this call, in its order (envs/vss.py:267-333):
 *   14 per rejection round r at [14 r, 14 r + 14): f's (7, 2) row of
 *      torch.rand((len(close_ids), 7, 2)) (ball, then robots blue 0-2, yellow 0-2; x, y)
 *      in the rounds where f was still too close (envs/vss.py:281-299);
 *   then, after the R rounds f used, [14 R, 14 R + 6): f's row of torch_rand_float(-pi, pi,
 *      (n, 6)) (robot yaws, envs/vss.py:307-312) and [14 R + 6, 14 R + 8): f's row of
 *      torch.rand((n, 2)) (ball velocity, envs/vss.py:318-325).
 * Rows of fields that do not reset are not read.  uniform_stride >= 22; a row holds
 * (uniform_stride - 8) / 14 rounds (capped at 64, the product's bound).
 * normals (SA/CMA/DMA; may be NULL in FULL): (n_fields, 12), the step's
 * torch.normal(0, 0.15, (N, 2, 3, 2)) of random_ou (envs/wrappers.py:5-19), already scaled.
 */
typedef struct vss_replay_draws {
  const float* uniforms;
  int64_t uniform_stride;
  const float* normals;
} vss_replay_draws;

/* ABI version (VSS_ABI_VERSION). */
int vss_abi_version(void);

/* The build's source stamp: 16 hex digits of sha256 over the library's sources (csrc/Makefile
 * STAMPED).  The Python loader recomputes it from the tree and refuses a stale library. */
const char* vss_source_hash(void);

/* Human-readable text for a VSS_E_* code. */
const char* vss_error_string(int code);

/*
 * One control step of every field.  Replaces, for mode FULL, Ext VecTask.step →
 * VSS.pre_physics_step (envs/vss.py:180-187) → gym.simulate → VSS.post_physics_step
 * (envs/vss.py:189-203) → time_outs; for SA/CMA/DMA additionally the wrapper's
 * random_ou + learner overwrite + slicing (envs/wrappers.py:101-115, 133-148, 163-180).
 */
int vss_step(void* stream, int64_t n_fields, int32_t mode, const vss_params* params,
             const vss_state* st, const vss_step_io* io);

/*
 * Parity entry: vss_step with the reset and OU draws taken from `draws` (recorded reference
 * draws, see vss_replay_draws) instead of the Philox stream.  The same kernel template as
 * vss_step (REPLAY instantiation); everything but the draw source is shared.  Test use only.
 */
int vss_step_replay(void* stream, int64_t n_fields, int32_t mode, const vss_params* params,
                    const vss_state* st, const vss_step_io* io, const vss_replay_draws* draws);

/*
 * The yellow team's side of vss_step_versus (N = n_fields):
 *   opp_actions  (N,3,2) actions of yellow robots 0..2; 8-B aligned                     read
 *   opp_obs      (N,3,52) the yellow robots' observations AFTER the step's reset
 *                (= rows [:,1] of FULL's obs); 16-B aligned                             write
 */
typedef struct vss_versus_io {
  const float* opp_actions;
  float* opp_obs;
} vss_versus_io;

/*
 * vss_step in mode SA / CMA / DMA with the yellow team driven by `vs->opp_actions` (a policy's
 * actions: a snapshot of the learner, a checkpoint, a scripted team) instead of the OU process.
 * Every vss_step_io output keeps the meaning it has in vss_step for that mode.  Action slots: the
 * learner's from io->actions, yellow's (6..11) from opp_actions; in SA blue robots 1-2 (slots 2..5)
 * keep their OU update with the values vss_step(SA) would draw (same Philox counter, same
 * operations); CMA and DMA draw no OU noise.  ou_buf afterwards holds all twelve applied, pre-clamp
 * actions (zeroed for finished fields); rng_counter advances by 1.  The opponent does not learn, so
 * it gets no terminal observation.  FULL takes all twelve actions itself: VSS_E_ARG.
 */
int vss_step_versus(void* stream, int64_t n_fields, int32_t mode, const vss_params* params,
                    const vss_state* st, const vss_step_io* io, const vss_versus_io* vs);

/*
 * The yellow team's learner rows of vss_step_mirror (N = n_fields, R = 3 for DMA, else 1); every
 * member has the shape of the same member of vss_step_io for the mode:
 *   actions      SA (N,2) yellow robot 0 | CMA (N,6) | DMA (3N,2); 8-B aligned             read
 *   obs          SA/CMA (N,52) = agent 3 | DMA (3N,52) = agents 3..5; after the reset      write
 *   terminal_obs same shape, before the reset                                              write
 *   rew          SA (N,4) = yellow robot 0's | CMA (N,4) = ((r3+r4)+r5)/3 | DMA (3N,4)     write
 *   reward_sum   (R*N,) = ((goal+grad)+move)+energy of the row, as vss_step                write
 *   dones        (R*N,) int64 = the field's done, repeated R times                         write
 *   time_outs    (R*N,) uint8, the same values as io->time_outs                            write
 *   progress_f   (R*N,) fp32, the same values as io->progress_f                            write
 * obs, terminal_obs and rew are 16-B aligned, dones 8-B, the float vectors 4-B.
 */
typedef struct vss_mirror_io {
  const float* actions;
  float* obs;
  float* terminal_obs;
  float* rew;
  float* reward_sum;
  int64_t* dones;
  uint8_t* time_outs;
  float* progress_f;
} vss_mirror_io;

/*
 * Two-sided self-play: vss_step in mode SA / CMA / DMA with both teams' robots as learner rows.
 * `io` is the blue team's and keeps every meaning it has in vss_step for the mode, except that
 * io->dones_rep is required in all three modes, (R*N,); `yl` is the yellow team's, the same rows
 * seen from the other side (observations team-relative, goal and grad rewards sign-flipped): every
 * output equals the FULL step's on the twelve applied actions, agent 0 / 0..2 for blue and agent
 * 3 / 3..5 for yellow.  Action slots: blue's from io->actions, yellow's from yl->actions (SA 6..7,
 * CMA / DMA 6..11); in SA blue robots 1-2 and yellow robots 1-2 (slots 2..5, 8..11) keep their OU
 * update with the values vss_step(SA) would draw (same Philox counter, same operations); CMA and
 * DMA draw no OU noise.  ou_buf afterwards holds all twelve applied, pre-clamp actions (zeroed for
 * finished fields); rng_counter advances by 1.  FULL already has both teams' rows: VSS_E_ARG.
 */
int vss_step_mirror(void* stream, int64_t n_fields, int32_t mode, const vss_params* params,
                    const vss_state* st, const vss_step_io* io, const vss_mirror_io* yl);

/*
 * K consecutive FULL-mode steps in one launch for a pre-supplied action sequence (random-action
 * benchmarks, scripted / OU opponents, evaluation): bit-identical to K vss_step(FULL) calls — the
 * same reference semantics per step (envs/vss.py:180-333) — with the field state kept on chip
 * between steps.  State buffers (st) are updated as after the K-th step.
 */
int vss_rollout(void* stream, int64_t n_fields, int32_t n_steps, const vss_params* params,
                const vss_state* st, const vss_rollout_io* io);

/*
 * Re-sample every field whose reset_buf != 0 (VSS.reset_dones, envs/vss.py:267-333);
 * callable externally after `reset_buf[:] = 1` (play.py:132-133).  Does not touch
 * reset_buf / progress_buf and does not compute observations (same as the reference).
 */
int vss_reset_dones(void* stream, int64_t n_fields, const vss_params* params,
                    const vss_state* st);

/* Parity entry: vss_reset_dones with recorded reference draws (e.g. the construction-time
 * reset, envs/vss.py:72); normals unused.  Test use only. */
int vss_reset_dones_replay(void* stream, int64_t n_fields, const vss_params* params,
                           const vss_state* st, const vss_replay_draws* draws);

/*
 * compute_obs (envs/vss.py:205-216, 530-575) for agents [0, n_agents): n_agents = 6 writes
 * (N,2,3,52), 3 writes the blue team (N,3,52), 1 writes blue robot 0 (N,52).
 */
int vss_compute_observations(void* stream, int64_t n_fields, const vss_state* st,
                             float* obs, int32_t n_agents);

/* ---------------------------------------------------------------------------------------------
 * Fused rollout policy: the reference Agent's actor and critic MLPs
 * (ppo_continuous_action_isaacgym.py:127-164, 52 -> 256 -> 512 -> 512 -> 256 -> n_out, tanh)
 * on the fp32 matrix cores, activations kept in registers across the five layers.
 * ------------------------------------------------------------------------------------------- */

/* floats needed for one network's packed weights (n_out = 1 critic, 2 or 6 actor); -1 if bad */
int64_t vss_mlp_packed_size(int32_t n_out);

/*
 * Repack one network (torch nn.Linear layout: weights[i] is (out, in) row-major, biases[i] (out))
 * into the kernel's lane order.  Call once per parameter update.
 */
int vss_mlp_pack(void* stream, int32_t n_out, const float* const* weights, const float* const* biases,
                 float* packed);

/*
 * Agent.get_action_and_value (ppo…:157-164) on `rows` observations (rows, 52):
 * mean = actor(obs); action = action_in if given, else mean + exp(logstd) * N(0,1) (Philox on
 * (seed, counter, row)); log-prob and entropy summed over the n_act dims (torch Normal
 * formulas); value = critic(obs).  With actor_packed == NULL only the critic runs
 * (Agent.get_value, ppo…:154-155).  Any output pointer may be NULL.
 */
int vss_policy_forward(void* stream, int64_t rows, int32_t n_act, const float* obs,
                       const float* actor_packed, const float* logstd, const float* critic_packed,
                       uint64_t seed, uint64_t counter, const float* action_in, float* action_out,
                       float* logprob_out, float* entropy_out, float* value_out, float* mean_out);

/*
 * vss_policy_forward with an optional row mask for the critic-only form (actor_packed == NULL):
 * only rows with row_mask[row] != 0 (e.g. the step's dones) are evaluated and written.  Used
 * for the terminal-observation values of the fields that reset (ppo…:272): for every other field
 * the terminal observation equals the next observation, whose value the next step computes.
 */
int vss_value_forward_masked(void* stream, int64_t rows, int32_t n_act, const float* obs,
                             const float* actor_packed, const float* logstd, const float* critic_packed,
                             uint64_t seed, uint64_t counter, const float* action_in, float* action_out,
                             float* logprob_out, float* entropy_out, float* value_out, float* mean_out,
                             const int64_t* row_mask);

/*
 * The actor alone (an opponent policy needs actions, not values): mean = actor(obs), action = mean +
 * exp(logstd) * N(0,1) with the Philox stream and sampling formula of vss_policy_forward -- for equal
 * (seed, counter, row) the sampled action is the same.  No critic is evaluated.  action_out / mean_out
 * (rows, n_act); either may be NULL.
 */
int vss_actor_forward(void* stream, int64_t rows, int32_t n_act, const float* obs, const float* actor_packed,
                      const float* logstd, uint64_t seed, uint64_t counter, float* action_out, float* mean_out);

/*
 * The actor tail of Agent.get_action_and_value (ppo_continuous_action_isaacgym.py:157-164) from
 * actor means computed elsewhere (the rollout's GEMM-chain path, vss_amd/policy.py): per row,
 * action = mean + exp(logstd) z with z from the same Philox stream (seed, counter, row) as
 * vss_policy_forward (or action_in when given), log-prob and entropy summed over the n_act dims.
 * mean / action_in / action_out (rows, n_act), logprob_out / entropy_out (rows,); outputs may be NULL.
 */
int vss_policy_sample(void* stream, int64_t rows, int32_t n_act, const float* mean, const float* logstd, uint64_t seed,
                      uint64_t counter, const float* action_in, float* action_out, float* logprob_out,
                      float* entropy_out);

/*
 * Several actors in one launch (an opponent pool: vss_amd/opponent.py OpponentPool).  The rows are cut
 * into `count` groups of `group_rows` rows (the last may be shorter); group g is evaluated with
 * actor_packed[g] and logstd[g].  A host struct: the pointers travel to the kernel as kernel arguments.
 */
#define VSS_MAX_ACTOR_GROUPS 16
typedef struct vss_actor_groups {
  int32_t count;            /* 1..VSS_MAX_ACTOR_GROUPS */
  int64_t group_rows;       /* rows per group: > 0, a multiple of 64; group g owns rows
                               [g*group_rows, min(rows, (g+1)*group_rows));
                               (count-1)*group_rows < rows <= count*group_rows */
  const float* actor_packed[VSS_MAX_ACTOR_GROUPS];  /* vss_mlp_pack output, 16-B aligned; entries >= count unused */
  const float* logstd[VSS_MAX_ACTOR_GROUPS];        /* (n_act,) each */
} vss_actor_groups;

/*
 * vss_actor_forward with per-group weights: row r uses actor_packed[r / group_rows] and
 * logstd[r / group_rows]; the Philox row is the global row r.  The rows of group g in action_out /
 * mean_out are bit-identical to vss_actor_forward(rows, ..., actor_packed[g], logstd[g], seed, counter, ...)
 * over the whole batch (count == 1: the whole output).  The kernel is chosen by the total row count,
 * as in vss_actor_forward.  VSS_E_ARG: a null group / obs / used weight or log-std pointer, a misaligned
 * actor_packed, count outside 1..16, group_rows not a positive multiple of 64, rows outside
 * ((count-1)*group_rows, count*group_rows] (rows == 0 is VSS_OK, no launch), n_act not in {2, 6}.
 */
int vss_actor_forward_grouped(void* stream, int64_t rows, int32_t n_act, const float* obs, const vss_actor_groups* g,
                              uint64_t seed, uint64_t counter, float* action_out, float* mean_out);

/*
 * vss_policy_sample's action draw with logstd[row / group_rows] and the global row as the Philox row
 * (means from per-group GEMM chains): the rows of group g equal vss_policy_sample(rows, ..., logstd[g],
 * ..., action_out, NULL, NULL) over the whole batch.  actor_packed is not read and may be NULL.
 * Argument checks as vss_actor_forward_grouped (mean in place of obs).
 */
int vss_policy_sample_grouped(void* stream, int64_t rows, int32_t n_act, const float* mean, const vss_actor_groups* g,
                              uint64_t seed, uint64_t counter, float* action_out);

/* ---------------------------------------------------------------------------------------------
 * PPO-update helper: the backward of a hidden layer's tanh
 * (ppo_continuous_action_isaacgym.py:104-111, autograd of nn.Tanh + nn.Linear's bias) in one pass:
 *   grad_in = grad_out * (1 - y^2)             (rows, cols) row-major, y = tanh output
 *   bias_partial[c][j] = sum of grad_in[r][j] over the rows r of part c
 * with vss_tanh_grad_chunks(rows, cols) parts (fixed row sets, -1 for a bad size); the bias
 * gradient is the sum of bias_partial over its parts (caller-side, deterministic).  cols in {64, 128, 256, 512, 1024};
 * every pointer 16-B aligned.  Replaces torch's tanh_backward + the bias-gradient reduction.
 * ------------------------------------------------------------------------------------------- */
int64_t vss_tanh_grad_chunks(int64_t rows, int32_t cols);
int vss_tanh_grad_bias(void* stream, int64_t rows, int32_t cols, const float* grad_out, const float* y,
                       float* grad_in, float* bias_partial);

/*
 * The forward of a hidden layer (nn.Linear then nn.Tanh, ppo…:104-111; in the update:
 * ppo…:331 → Agent.get_action_and_value) in one launch on the fp32 matrix cores:
 * y = tanh(x W^T + b) with x (rows, k_in), W (n_out, k_in) (nn.Linear's layout), both row-major,
 * y (rows, n_out).  k_in % 4 == 0, n_out % 128 == 0; x, W, y 16-B aligned.  Replaces torch's
 * addmm + tanh (the activation is written once instead of written, read and written again).
 */
int vss_linear_tanh(void* stream, int64_t rows, int32_t k_in, int32_t n_out, const float* x, const float* w,
                    const float* bias, float* y);

/*
 * vss_linear_tanh for the LAST hidden layer with the output layer folded in (ppo…:104-111: Linear(512,
 * 256), Tanh, Linear(256, k_out)): y = tanh(x W^T + b) as vss_linear_tanh, and
 *   out_part[s][r][a] = sum over the 64 columns c of slice s (s = 0..3) of y[r][c] w_out[a][c]
 * so the output layer is out = sum_s out_part[s] + b_out without a second read of y.  n_out = 256,
 * rows % 256 == 0, k_in % 64 == 0, k_out in {1, 2, 6}; w_out (k_out, 256) row-major; out_part
 * (4, rows, k_out).  VSS_E_ARG for other shapes (the caller uses vss_linear_tanh + a GEMM then).
 */
int vss_linear_tanh_out(void* stream, int64_t rows, int32_t k_in, int32_t n_out, const float* x, const float* w,
                        const float* bias, float* y, int32_t k_out, const float* w_out, float* out_part);

/*
 * The backward through a layer and the tanh below it (autograd of nn.Linear → nn.Tanh,
 * ppo…:104-111, in loss.backward() at ppo…:357) in one launch on the fp32 matrix cores:
 *   grad_in = (grad_next W_next) * (1 - y^2),   bias_partial[c][j] = sum of grad_in[r][j] over part c
 * grad_next (rows, k_next) = the pre-activation gradient of the layer above, w_next_t (n_out, k_next)
 * = that layer's weight TRANSPOSED (row-major), y (rows, n_out) = this layer's tanh output,
 * grad_in (rows, n_out) = this layer's pre-activation gradient.  The bias gradient is the sum over
 * the vss_linear_tanh_backward_chunks(rows, k_next, n_out) parts (fixed, deterministic; -1 for a bad
 * shape).  k_next % 4 == 0, n_out % 128 == 0; every pointer 16-B aligned.  Replaces torch's dX GEMM +
 * vss_tanh_grad_bias (the gradient is written once instead of written, read and written again).
 */
int64_t vss_linear_tanh_backward_chunks(int64_t rows, int32_t k_next, int32_t n_out);
int vss_linear_tanh_backward(void* stream, int64_t rows, int32_t k_next, int32_t n_out, const float* grad_next,
                             const float* w_next_t, const float* y, float* grad_in, float* bias_partial);

/* The Agent's output layer backward in one streaming pass (ppo_continuous_action_isaacgym.py:104-111
 * under loss.backward(), :357): for the output nn.Linear (k_out = 1, 2 or 6 columns, g_out and its
 * weight zero-padded by the caller to k_pad = 4 or 8 columns / rows) over a tanh layer of width n
 * (n in {128, 256, 512, 1024}):
 *   grad_in = (g_out W_out) * (1 - y^2)        the tanh layer's pre-activation gradient (rows, n)
 *   bias_partial (chunks, n)                   column-sum parts of grad_in (its bias gradient)
 *   wgrad_partial (chunks, k_pad, n)           parts of g_out^T y, the output layer's weight gradient
 * g_out (rows, k_pad), w_out_t (n, k_pad) = the padded weight TRANSPOSED, y (rows, n) = the tanh
 * output (the output layer's input); chunks = vss_output_backward_chunks(rows, k_pad, n) (-1 for a
 * bad shape), summed in a fixed order by the caller.  Every pointer 16-B aligned.  Replaces the
 * output layer's dX GEMM + tanh_backward + bias reduction and its dW GEMM (two reads of y -> one).
 */
int64_t vss_output_backward_chunks(int64_t rows, int32_t k_pad, int32_t n);
int vss_output_backward(void* stream, int64_t rows, int32_t k_pad, int32_t n, const float* g_out, const float* w_out_t,
                        const float* y, float* grad_in, float* bias_partial, float* wgrad_partial);

/* vss_output_backward_direct: the same pass for the update's minibatch without autograd
 * (vss_amd/minibatch.py direct_minibatch): g_out (rows, k_out) as vss_ppo_loss_direct
 * writes it and w_out (k_out, n) as nn.Linear holds it -- no padded copies; k_out in {1, 2, 3, 4, 6, 8},
 * n in {128, 256, 512, 1024}.  bias_partial (chunks, n), wgrad_partial (chunks, k_out, n) with chunks =
 * vss_output_backward_direct_chunks(rows, k_out, n) <= 256 (-1 for a bad shape), few enough for one
 * vss_sum_parts launch.  y, grad_in and the partials 16-B aligned; g_out, w_out 4-B aligned.
 */
int64_t vss_output_backward_direct_chunks(int64_t rows, int32_t k_out, int32_t n);
int vss_output_backward_direct(void* stream, int64_t rows, int32_t k_out, int32_t n, const float* g_out,
                               const float* w_out, const float* y, float* grad_in, float* bias_partial,
                               float* wgrad_partial);

/* ---------------------------------------------------------------------------------------------
 * The update's hidden-layer GEMMs in fp32 arithmetic on the bf16 matrix cores (csrc/vss_gemm_x6.hip;
 * ppo_continuous_action_isaacgym.py:104-111 under the update's forward ppo…:331 and loss.backward()
 * ppo…:357).  Every fp32 operand is split exactly into three bf16 parts (hi + mid + lo) and each
 * product is the six partial products above 2^-23 |a||b|, accumulated in fp32: the error is that of
 * an fp32 GEMM (tests/test_gemm_x6.py).  Exact shapes only (the update's minibatches); VSS_E_ARG
 * otherwise, and the caller uses the fp32-MFMA entries above.
 *
 * vss_linear_tanh_bf16x6 / _out_bf16x6 / vss_linear_tanh_backward_bf16x6: the same contracts as
 * vss_linear_tanh / vss_linear_tanh_out / vss_linear_tanh_backward with rows % 256 == 0,
 * n_out % 128 == 0, k % 64 == 0 (k_in resp. k_next); the backward's bias gradient is the sum over the
 * vss_linear_tanh_backward_chunks_bf16x6 parts.  w_split: caller-owned scratch of 3 * n_out * k
 * uint16 (16-B aligned) that the call fills with the weight's bf16 planes before its GEMM reads them.
 *
 * w (resp. w_next_t) == NULL: w_split already holds the weight's planes, written by
 * vss_weight_planes_bf16x6 for this (n_out, k) since the weight last changed (no split launch).
 *
 * vss_weight_planes_bf16x6: the planes of `count` (1..16) weights in ONE launch, into the w_split
 * buffers the GEMM entries above then take with a NULL weight: job q is an (n[q], k[q]) operand
 * (n % 128 == 0, n <= 4096, k % 64 == 0), stored row-major as w[q] (n, k) when transpose[q] == 0, or
 * as its transpose (k, n) when transpose[q] == 1 (the backward's W_next^T straight from nn.Linear's
 * weight, no transposed copy).  Host arrays of `count` entries; w_split 16-B aligned, w 16-B
 * aligned when not transposed.  Replaces one split launch per GEMM and the backward's transposes.
 *
 * vss_weight_grad_bf16x6: a Linear layer's weight gradient (autograd of nn.Linear, ppo…:357)
 *   partial[s][o][i] = sum over the rows r of part s of grad[r][o] x[r][i]
 * grad (rows, n_out) = the layer's output gradient, x (rows, k_in) = its input; dW = the sum over the
 * vss_weight_grad_chunks_bf16x6(rows, n_out, k_in) parts (-1 for a bad shape).  rows % 64 == 0,
 * n_out % 256 == 0, k_in % 128 == 0; every pointer 16-B aligned.  Replaces hipBLASLt's split-K
 * grad^T x GEMM.
 *
 * vss_first_weight_grad_bf16x6: the same for the Agent's FIRST layer (nn.Linear(obs, 256),
 * ppo_continuous_action_isaacgym.py:131,142; its weight gradient under loss.backward(), ppo…:352),
 * whose input x (rows, k_in) is the observation: n_out == 256, k_in <= 64 and k_in % 4 == 0 (52 for
 * every VSS wrapper), rows % 64 == 0; grad and x 16-B aligned.  partial (parts, 256, k_in), parts =
 * vss_first_weight_grad_chunks_bf16x6(rows, n_out, k_in) (-1 for a bad shape).  Replaces hipBLASLt's
 * batched grad^T x + torch.sum (the split-K dW of the first layer).
 *
 * vss_first_layer_bf16x6: the Agent's FIRST layer forward, y = tanh(x W^T + b) (nn.Linear(obs, 256) +
 * nn.Tanh, ppo…:131,142) with x (rows, k_in) the observations, w (256, k_in) nn.Linear's weight,
 * bias (256,), y (rows, 256): n_out == 256, 0 < k_in <= 64, k_in % 4 == 0, any rows >= 0; x and y
 * 16-B aligned.  The same split products as above (k zero-padded to 64); tanh as the other epilogues.
 * Replaces the fp32-MFMA first_layer_kernel (vss_linear_tanh) on the update and rollout paths.
 * ------------------------------------------------------------------------------------------- */
int vss_linear_tanh_bf16x6(void* stream, int64_t rows, int32_t k_in, int32_t n_out, const float* x, const float* w,
                           const float* bias, float* y, uint16_t* w_split);
int vss_linear_tanh_out_bf16x6(void* stream, int64_t rows, int32_t k_in, int32_t n_out, const float* x,
                               const float* w, const float* bias, float* y, int32_t k_out, const float* w_out,
                               float* out_part, uint16_t* w_split);
int64_t vss_linear_tanh_backward_chunks_bf16x6(int64_t rows, int32_t k_next, int32_t n_out);
int vss_linear_tanh_backward_bf16x6(void* stream, int64_t rows, int32_t k_next, int32_t n_out, const float* grad_next,
                                    const float* w_next_t, const float* y, float* grad_in, float* bias_partial,
                                    uint16_t* w_split);
/* vss_linear_tanh_loss_bf16x6: the last hidden layer, the output layer, the minibatch's PPO loss terms and
 * the output layer's backward in ONE x6 launch (direct_minibatch): y = tanh(x W^T + b) stays in the
 * accumulators, out = y w_out^T + b_out, each row's loss terms and gradient g_out as vss_ppo_loss_direct
 * forms them (role 0: the actor's policy terms, k_out in {1, 2}, advantages normalised from adv_part as
 * there; role 1: the critic's value terms, k_out == 1), and grad_in (rows_pad, 256) = (g_out w_out)
 * (1 - y^2) -- the hidden layer's pre-activation gradient, written instead of y.  Rows >= rows are
 * padding: zero gradient, no loss term.  Per block b of vss_linear_tanh_loss_blocks_bf16x6(rows_pad, k_in,
 * n_out) (-1 for a bad shape): part_cs[b] (256,) its column sums of grad_in (the hidden bias gradient),
 * part_dwo[b] (k_out, 256) its g_out^T y (the output weight gradient), part_stats[b] (32,) its loss sums
 * (csrc/vss_loss_row.h kBlockStats) for vss_ppo_loss_fused_finish.  n_out == 256, rows_pad % 256 == 0,
 * k_in % 64 == 0; w_split the weight's bf16 planes (vss_weight_planes_bf16x6), x / grad_in 16-B aligned.
 * Replaces vss_linear_tanh_out_bf16x6 + vss_ppo_loss_direct's row pass + vss_output_backward_direct. */
int64_t vss_linear_tanh_loss_blocks_bf16x6(int64_t rows, int32_t k_in, int32_t n_out);
int vss_linear_tanh_loss_bf16x6(void* stream, int32_t role, int64_t rows_pad, int64_t rows, int32_t k_in, int32_t n_out,
                                const float* x, const float* bias, int32_t k_out, const float* w_out, const float* b_out,
                                const float* action, const float* logprob_old, const float* adv, const double* adv_part,
                                int32_t adv_nparts, double adv_count, const float* logstd, const float* returns,
                                const float* values_old, float clip_coef, float clip_lo, float clip_hi, float vf_coef,
                                int32_t clip_vloss, float* grad_in, float* part_cs, float* part_dwo, float* part_stats,
                                const uint16_t* w_split);
int vss_weight_planes_bf16x6(void* stream, int32_t count, const float* const* w, const int32_t* n, const int32_t* k,
                             const int32_t* transpose, uint16_t* const* w_split);
int64_t vss_weight_grad_chunks_bf16x6(int64_t rows, int32_t n_out, int32_t k_in);
int vss_weight_grad_bf16x6(void* stream, int64_t rows, int32_t n_out, int32_t k_in, const float* grad, const float* x,
                           float* partial);
int vss_first_layer_bf16x6(void* stream, int64_t rows, int32_t k_in, int32_t n_out, const float* x, const float* w,
                           const float* bias, float* y);
int64_t vss_first_weight_grad_chunks_bf16x6(int64_t rows, int32_t n_out, int32_t k_in);
int vss_first_weight_grad_bf16x6(void* stream, int64_t rows, int32_t n_out, int32_t k_in, const float* grad,
                                 const float* x, float* partial);

/* ---------------------------------------------------------------------------------------------
 * The clipped PPO loss of one update minibatch and its gradients (SURVEY §8 A13;
 * ppo_continuous_action_isaacgym.py:314-349: Normal(mean, exp(logstd)).log_prob(action).sum(1), the
 * ratio to the rollout's log-prob, the clipped surrogate, the (optionally clipped) value loss, the
 * entropy, loss = pg_loss - ent_coef entropy_loss + vf_coef v_loss, and old_approx_kl / approx_kl /
 * clipfrac), in two launches.  Replaces torch's loss expressions and their autograd (~100 kernels).
 *   mean, action (rows_pad, n_act); value (rows_pad,) the critic output; logstd (n_act,);
 *   logprob_old, adv, returns, values_old (rows,) the minibatch's stored rows (adv already normalised);
 *   clip_lo / clip_hi: 1 - clip_coef and 1 + clip_coef as fp32 (the clamp bounds);
 *   grad_mean (rows_pad, n_act), grad_value (rows_pad,), grad_logstd (n_act,): d loss / d input, with
 *     torch's conventions at the kinks (maximum splits a tie in half, clamp passes [lo, hi]); rows
 *     [rows, rows_pad) (padding copies the loss does not see) get zero;
 *   loss_out[1] = loss; stats_out[6] = pg_loss, v_loss, entropy_loss, old_approx_kl, approx_kl, clipfrac;
 *   partial: scratch of vss_ppo_loss_scratch_floats(rows_pad, n_act) floats (-1 for a bad size),
 *     reduced in a fixed order (deterministic).
 * n_act in {1, 2, 3, 4, 6, 8}; every pointer 4-B aligned.
 * ------------------------------------------------------------------------------------------- */
int64_t vss_ppo_loss_scratch_floats(int64_t rows_pad, int32_t n_act);
int vss_ppo_loss(void* stream, int64_t rows, int64_t rows_pad, int32_t n_act, const float* mean, const float* logstd,
                 const float* value, const float* action, const float* logprob_old, const float* adv,
                 const float* returns, const float* values_old, float clip_coef, float clip_lo, float clip_hi,
                 float ent_coef, float vf_coef, int32_t clip_vloss, float* grad_mean, float* grad_value,
                 float* grad_logstd, float* loss_out, float* stats_out, float* partial);

/* vss_ppo_loss_direct: the same loss for the update's minibatch without autograd
 * (vss_amd/minibatch.py direct_minibatch), from what the networks' last launches leave:
 *   mean_parts (mean_nparts, rows_pad, n_act) + mean_bias (n_act,): the actor's output as the parts of
 *     vss_linear_tanh_out_bf16x6's out_part (summed in order, then the bias); value_parts
 *     (value_nparts, rows_pad) + value_bias (1,) the critic's;
 *   adv (rows,) RAW advantages, normalised in the kernel when adv_part != NULL: adv_part (adv_nparts, 2)
 *     fp64 (sum, sum of squares) parts over adv_count values (vss_minibatch_gather's, or their all-reduced
 *     sum), (a - mean) / (std + 1e-8) with mean = s / n, std = sqrt(max((q - n mean^2) / (n - 1), 0)) in
 *     fp64 (ppo…:325-326, normalize_advantages' data-parallel formula); adv_part NULL: adv as given;
 *   grad_mean_bias (n_act,), grad_value_bias (1,): the output layers' bias gradients (column sums of
 *     grad_mean / grad_value, fixed order), written like grad_logstd;
 * the other arguments as vss_ppo_loss; partial: vss_ppo_loss_direct_scratch_floats(rows_pad, n_act).
 *
 * vss_minibatch_gather: one update minibatch's rows (ppo…:310-317) in one launch: for r < rows_pad,
 *   i = inds[r < mb ? r : (r - mb) % mb] (the padding rows repeat the minibatch), obs[r] = b_obs[i]
 *   (obs_w floats), act[r] = b_act[i] (act_w floats); for r < mb, logp / adv / ret / val[r] = b_*[i];
 *   adv_part (vss_minibatch_gather_parts(mb), 2) fp64 (sum, sum of squares) parts of the gathered
 *   advantages (fixed order).  An index outside [0, batch) gathers NaN.  inds int64 (mb,).
 * vss_adv_part_sum: out[2] = the nparts parts summed in order (for the data-parallel all-reduce).
 */
int64_t vss_ppo_loss_direct_scratch_floats(int64_t rows_pad, int32_t n_act);
int vss_ppo_loss_direct(void* stream, int64_t rows, int64_t rows_pad, int32_t n_act, const float* mean_parts,
                        int32_t mean_nparts, const float* mean_bias, const float* value_parts, int32_t value_nparts,
                        const float* value_bias, const float* logstd, const float* action, const float* logprob_old,
                        const float* adv, const double* adv_part, int32_t adv_nparts, double adv_count,
                        const float* returns, const float* values_old, float clip_coef, float clip_lo, float clip_hi,
                        float ent_coef, float vf_coef, int32_t clip_vloss, float* grad_mean, float* grad_value,
                        float* grad_logstd, float* grad_mean_bias, float* grad_value_bias, float* loss_out,
                        float* stats_out, float* partial);
/* vss_ppo_loss_fused_finish: vss_linear_tanh_loss_bf16x6's per-block loss sums of the actor (actor_blocks)
 * and the critic (critic_blocks) -> loss_out[1], stats_out[6], grad_logstd, grad_mean_bias (n_act,) and
 * grad_value_bias (1,) as vss_ppo_loss_direct writes them; n_act in {1, 2}. */
int vss_ppo_loss_fused_finish(void* stream, int64_t rows, int32_t n_act, int64_t actor_blocks, const float* actor_stats,
                              int64_t critic_blocks, const float* critic_stats, const float* logstd, float ent_coef,
                              float vf_coef, float* grad_logstd, float* grad_mean_bias, float* grad_value_bias,
                              float* loss_out, float* stats_out);
/* vss_randperm: the epoch's minibatch permutation (ppo…:309, torch.randperm(batch)): out (n,) int64 a
 * uniformly random permutation of [0, n) determined by seed[0] (one int64 on the device, drawn from the
 * update's generator), 0 < n < 2^31.  scratch: vss_randperm_scratch_bytes(n) bytes (-1 for a bad n),
 * 256-B aligned.  Each index gets 32 random bits (splitmix64 of seed and index); a radix sort on them
 * (4 passes, hipcub) orders the indices, and every run of tied bits is then shuffled (Fisher-Yates from a
 * second stream), so the permutation is uniform.  vss_randperm_bits: the same with key_bits (1..32) random
 * bits per index -- fewer bits force ties (the tie pass's test entry); vss_randperm = key_bits 32. */
int64_t vss_randperm_scratch_bytes(int64_t n);
int vss_randperm(void* stream, int64_t n, const int64_t* seed, int64_t* out, void* scratch, int64_t scratch_bytes);
int vss_randperm_bits(void* stream, int64_t n, int32_t key_bits, const int64_t* seed, int64_t* out, void* scratch,
                      int64_t scratch_bytes);
int64_t vss_minibatch_gather_parts(int64_t mb);
int vss_minibatch_gather(void* stream, int64_t mb, int64_t rows_pad, int64_t batch, const int64_t* inds, int64_t obs_w,
                         int64_t act_w, const float* b_obs, const float* b_act, const float* b_logp, const float* b_adv,
                         const float* b_ret, const float* b_val, float* obs, float* act, float* logp, float* adv,
                         float* ret, float* val, double* adv_part);
int vss_adv_part_sum(void* stream, int32_t nparts, const double* part, double* out);

/* ---------------------------------------------------------------------------------------------
 * A rollout's advantages and returns in one launch (csrc/vss_returns.hip): the train loop's
 * timeout-aware GAE (ppo_continuous_action_isaacgym.py compute_gae; the reference's ppo…:282-296),
 * bit for bit.  T = n_steps, E = n_rows (the batch's learner rows).  rewards, values, next_dones,
 * next_timeouts, advantages, returns and next_values / term_values are (T, E) fp32, row-major
 * [t * E + e]; v_last is (E,); every pointer 4-B aligned.  next_dones and next_timeouts are the loop's
 * float storage: nonzero means set.
 *   Form A (next_values given; term_values and v_last NULL): nv[t][e] = next_values[t][e], as
 *     compute_gae takes it.
 *   Form B (next_values NULL; term_values and v_last given): the merge of vss_amd/policy.py
 *     TerminalValues.next_values in the kernel,
 *       nv[t][e] = next_dones[t][e] != 0 ? term_values[t][e] : (t + 1 < T ? values[t + 1][e] : v_last[e])
 *     -- a select, not arithmetic: term_values of rows that did not reset are never read into a sum.
 * Exactly one form must be present.  Per column e, walking t = T-1 .. 0 from last = 0, in float32 with
 * the operation order of the torch expressions and no FMA contraction:
 *   nnt   = (next_dones != 0 && next_timeouts == 0) ? 0.f : 1.f
 *   delta = ((rewards + (gamma * nv) * nnt) - values)
 *   last  = delta + ((gamma_lambda * (1.f - next_dones)) * last)
 *   advantages[t][e] = last;  returns[t][e] = last + values[t][e]
 * gamma_lambda = (float)((double)gamma * (double)lambda): the product is formed in double and rounded
 * once, as Python's `gamma * lam` reaches torch; (float)gamma * (float)lambda is another number for
 * some settings (0.997, 0.9).  advantages and returns must not overlap any input (nor each other).
 * VSS_E_ARG, before any HIP call: a null required pointer, both forms or neither, one of term_values /
 * v_last without the other, a pointer that is not 4-B aligned, negative n_steps or n_rows, a non-finite
 * gamma or gamma_lambda.  n_steps == 0 or n_rows == 0: VSS_OK, no launch.
 * ------------------------------------------------------------------------------------------- */
int vss_gae(void* stream, int64_t n_steps, int64_t n_rows, const float* rewards, const float* values,
            const float* next_values, const float* term_values, const float* v_last, const float* next_dones,
            const float* next_timeouts, float gamma, float gamma_lambda, float* advantages, float* returns);

/* ---------------------------------------------------------------------------------------------
 * The update's gradient bookkeeping on flat buffers (csrc/vss_optim.hip; vss_amd/flat.py
 * FlatGrads / FlatAdam).  Replaces, per minibatch, nn.utils.clip_grad_norm_ (ppo…:353)
 * and optim.Adam(eps=1e-5).step() (ppo…:166,354) -- torch's per-tensor norm chain and multi-tensor
 * Adam -- with two launches, and the split GEMMs' torch.sum reductions with one launch per backward.
 *
 * vss_grad_sq_partials: partial[b] = sum of grad[i]^2 over block b's chunk, b < count =
 *   vss_grad_sq_partials_count(n) (= min(1024, ceil(n / 4096)); -1 for n <= 0): with chunk =
 *   ceil(n / count), block b's chunk is the elements [b chunk, (b + 1) chunk) below n (a block whose
 *   range starts at or past n writes 0); fixed order (deterministic).
 * vss_adam_step_clipped: norm = sqrt(sum of the nparts partials); with max_norm >= 0 the gradients are
 *   scaled in place by min(1, max_norm / (norm + 1e-6)) (clip_grad_norm_: max_norm 0 zeroes them, as
 *   torch's does), with max_norm < 0 they are left alone (no clip requested); then Adam's step `step`
 *   (>= 1, the count after this step): m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2,
 *   p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps), evaluated in fp32 from these fp32
 *   hyper-parameters (1 - powf(b, step)).  Torch's Adam forms the bias corrections in double from double
 *   betas; against that, 1 - b2^step is up to 1.3e-5 relative away at small step counts and about half of
 *   it reaches the update (measured figures: DESIGN.md §5.7; pinned by tests/test_optim.py).
 *   norm_out (1 float, may be NULL) receives the pre-clip norm.  All buffers n fp32 elements.
 * vss_sum_parts: `count` (1..32) jobs; job q: dst[r * dst_ld + c] = sum over s = 0 .. parts - 1 of
 *   src[s * part_stride + r * src_ld + c], r < rows, c < cols, in a fixed order (parts s = w + 4 (u + 8 i)
 *   into running sum (w, u), then those sums in a fixed tree: deterministic).  Host arrays of count
 *   entries; device buffers; src parts must not overlap dst.
 * ------------------------------------------------------------------------------------------- */
int64_t vss_grad_sq_partials_count(int64_t n);
int vss_grad_sq_partials(void* stream, int64_t n, const float* grad, float* partial);
int vss_adam_step_clipped(void* stream, int64_t n, int32_t nparts, const float* partial, float max_norm, float lr,
                          float beta1, float beta2, float eps, int64_t step, float* grad, float* param, float* exp_avg,
                          float* exp_avg_sq, float* norm_out);
int vss_sum_parts(void* stream, int32_t count, const float* const* src, float* const* dst, const int64_t* parts,
                  const int64_t* part_stride, const int64_t* rows, const int64_t* cols, const int64_t* src_ld,
                  const int64_t* dst_ld);

/* ---------------------------------------------------------------------------------------------
 * Episode statistics: RecordEpisodeStatisticsTorch.step (envs/wrappers.py:66-87)
 * for `rows` learner rows in one launch, in the reference's order:
 *   ep_returns += rews; ep_lengths += 1; returned_returns = ep_returns; returned_lengths =
 *   ep_lengths; return_sum = ((r0 + r1) + r2) + r3 of returned_returns; then
 *   ep_returns *= 1 - dones; ep_lengths *= 1 - dones.
 * rews, ep_returns, returned_returns: (rows, 4) fp32, 16-B aligned; ep_lengths,
 * returned_lengths: (rows,) int32; dones: (rows,) int64; return_sum: (rows,) fp32.
 * ------------------------------------------------------------------------------------------- */
int vss_episode_stats(void* stream, int64_t rows, const float* rews, const int64_t* dones, float* ep_returns,
                      int32_t* ep_lengths, float* returned_returns, int32_t* returned_lengths, float* return_sum);

/*
 * Match results per opponent group, after a versus step: for every field f whose learner row
 * r = f * rows_per_field has dones[r] != 0, with q = f / group_fields,
 *   tally[q][0] += 1 (episodes); tally[q][1] += 1 if rew[r][0] > 0 (the learner scored);
 *   tally[q][2] += 1 if rew[r][0] < 0 (the learner conceded); tally[q][3] += (int64) progress_f[r] (steps).
 * The goal term's sign tells who scored only for w_goal > 0 (the caller's check).  Integer adds only:
 * exact, independent of order.  Accumulates -- the caller zeroes tally (count, 4) int64.  rew
 * (n_fields * rows_per_field, 4) fp32, 16-B aligned; dones int64 and progress_f fp32 over the same rows.
 * VSS_E_ARG: rows_per_field not 1 or 3, group_fields <= 0, count outside 1..16,
 * count * group_fields < n_fields, a null or misaligned pointer.  n_fields == 0: VSS_OK, no launch.
 */
int vss_match_tally(void* stream, int64_t n_fields, int32_t rows_per_field, int64_t group_fields, int32_t count,
                    const float* rew, const int64_t* dones, const float* progress_f, int64_t* tally);

/* ---------------------------------------------------------------------------------------------
 * The scripted benchmark team (csrc/vss_scripted.hip; vss_amd/scripted.py): the six
 * wheel commands of one team per field from robot 0's observation row, in one launch.  A pure
 * function of that row -- no state, no random draw, graph-safe -- and equal bit for bit to
 * vss_amd.scripted.reference_actions, which specifies controller `version` operation by operation.
 * VSS_SCRIPTED_VERSION names the controller: a change of behaviour gets a new number, 1 stays.
 *
 * obs: robot 0's 52-float row of field 0 for the team driven (team frame: it attacks +x); field f's row is
 *   at obs + f * obs_field_stride floats.  Only the ball's position and the own robots' positions and
 *   headings are read (floats 0..27 of the row); rows of robots 1-2 are not read.  obs_field_stride: a
 *   multiple of 4, >= 52 -- 156 for a contiguous (N,3,52) team block, 312 for one team of (N,2,3,52).
 * act: field f's six floats (robots 0..2: left, right wheel, each in [-1, 1]) at act + f * act_field_stride;
 *   act_field_stride: a multiple of 2, >= 6 -- 6 for (N,3,2), 12 for one team's half of (N,2,3,2).
 *   Nothing else is written: the gap between two fields' six floats is untouched.
 * VSS_E_ARG, before any HIP call: a null pointer, obs not 16-B or act not 8-B aligned, a stride below its
 * minimum or not a multiple as above, version != 1, n_fields < 0.  n_fields == 0: VSS_OK, no launch.
 * ------------------------------------------------------------------------------------------- */
#define VSS_SCRIPTED_VERSION 1
int vss_scripted_team(void* stream, int64_t n_fields, int32_t version, const float* obs, int64_t obs_field_stride,
                      float* act, int64_t act_field_stride);

/* ---------------------------------------------------------------------------------------------
 * The perception channel (csrc/vss_perceive.hip; vss_amd/perceive.py): what an overhead
 * camera hands a policy instead of the simulator's state -- observation rows `delay` control steps late
 * and with Gaussian noise on every pose -- in one launch per call.  vss_amd.perceive.reference_perceive
 * specifies it operation by operation and the kernel equals it bit for bit.
 *
 * Rows: the 52-float row of team block b, field f, robot k is at
 *   base + (b * team_stride + f * field_stride + k) * 52 floats
 * for obs, term, obs_out and term_out alike; block b's team is first_team ^ b (0 blue, 1 yellow).
 * State (the caller's, zero-initialised or not: a start call initialises it):
 *   ring (delay + 1, n_teams, n_fields, robots, 52) fp32: the last delay + 1 true `obs` frames, the frame
 *     of call t in slot t % (delay + 1);  age (n_fields) int32: steps since the field's episode began,
 *     saturating at delay.
 * One call, per field (done = done[f * done_stride] != 0):
 *   d = min(age + 1, delay);  R = ring frame call - d (delay >= 1)
 *   term_out = R with the six own-action floats (11, 12, 20, 21, 29, 30) of `term`;  `term` itself for delay 0
 *   age' = done ? 0 : d;  ring slot call % (delay + 1) = obs
 *   obs_out = age' == 0 ? obs : R with the six own-action floats of `obs`
 *   then the same noise on both outputs: one set of 40 unit normals per (field, call) -- Philox4x32-10,
 *   key (seed low, seed high), counter (field, call, 7 << 24, block 0..9), Box-Muller as the step's OU
 *   draws -- scaled by the class's sigma: positions (m), velocities (m/s), headings (rad, a rotation of
 *   (cos, sin)) and yaw rates (rad/s) of the ball and the six robots in the world frame, so every row
 *   of a field sees the same world.  A class with sigma 0 is copied unchanged.
 * term == NULL (and term_out == NULL) is the start call of reset(): age = 0, the slot is written,
 * obs_out = obs + noise.  No frame of an earlier episode is ever read.
 * call: the caller's call index, +1 per call; the slot and the frame arithmetic are modulo delay + 1.
 *
 * VSS_E_ARG, before any HIP call: a null lay, noise, obs, done, ring, age or obs_out; exactly one of term /
 * term_out null; a row pointer not 16-B, done not 8-B or age not 4-B aligned; an output (obs_out, term_out,
 * ring, age) overlapping an input or another output; delay outside 0..VSS_PERCEIVE_MAX_DELAY; a negative or
 * non-finite sigma; robots not 1 or 3; n_teams not 1 or 2; first_team not 0 or 1; field_stride < robots;
 * with two teams team_stride < (n_fields - 1) * field_stride + robots; done_stride < 1; n_fields < 0; sizes
 * whose grid or byte offsets overflow.  n_fields == 0: VSS_OK, no launch.
 * ------------------------------------------------------------------------------------------- */
#define VSS_PERCEIVE_MAX_DELAY 15
typedef struct vss_perceive_layout {
  int64_t field_stride;  /* rows from field f to f+1 within a team block               */
  int64_t team_stride;   /* rows from team block 0 to block 1 (n_teams == 2)           */
  int32_t robots;        /* rows per field and team, 1 or 3; row k is robot k          */
  int32_t n_teams;       /* 1 or 2                                                     */
  int32_t first_team;    /* team of block 0: 0 blue, 1 yellow; block 1 is the other    */
} vss_perceive_layout;
typedef struct vss_perceive_noise { float pos, vel, ang, angvel; } vss_perceive_noise;
int vss_perceive(void* stream, int64_t n_fields, const vss_perceive_layout* lay, int32_t delay,
                 const vss_perceive_noise* noise, uint64_t seed, uint32_t call,
                 const float* obs, const float* term /* NULL: start */, const int64_t* done, int64_t done_stride,
                 float* ring /* (delay+1, n_teams, n_fields, robots, 52) */, int32_t* age /* (n_fields) */,
                 float* obs_out, float* term_out /* NULL iff term is */);

/* ---------------------------------------------------------------------------------------------
 * The actuation channel (csrc/vss_actuate.hip; vss_amd/actuate.py): what a VSS robot's wheels
 * receive of what a policy commands.
 *
 * A command is the two floats (left wheel, right wheel) of one robot.  One call takes the commands of one control
 * step through the channel: the radio's range and 8-bit-like quantisation, the loss of a team's packet (the robot
 * keeps the command it had), a deadband, the episode's per-wheel motor gains and per-step command noise.
 * vss_amd/actuate.py reference_actuate is the specification; the kernel equals it bit for bit.
 * ------------------------------------------------------------------------------------------- */
#define VSS_ACTUATE_MAX_LEVELS 32767

/* Where the commands lie: strides in robots (2 floats); the command of team block b, field f, robot k is at
 * base + (b * team_stride + f * field_stride + k) * 2 floats.  team_stride is read with two teams only.
 *   SA (N,2): 1, -, 1, 1, 0      CMA (N,6), DMA (3N,2): 3, -, 3, 1, 0      opp_act (N,3,2): 3, -, 3, 1, 1
 *   mirror SA (2N,2): 1, N, 1, 2, 0      mirror CMA (2N,6) / DMA (6N,2): 3, 3N, 3, 2, 0
 *   the blue half of FULL's (N,2,3,2): 6, -, 3, 1, 0 */
typedef struct vss_actuate_layout {
  int64_t field_stride;
  int64_t team_stride;
  int32_t robots;      /* 1 or 3 */
  int32_t n_teams;     /* 1 or 2 */
  int32_t first_team;  /* 0 blue, 1 yellow; block 1 is the other */
} vss_actuate_layout;

/* gain_sigma in [0, 0.3]: wheel gain 1 + gain_sigma * clamp(z, -3, 3), drawn once per episode (so >= 0.1);
 * noise_sigma >= 0: added to the applied command every step; deadband in [0, 1]: |command| below it is 0;
 * loss_prob in [0, 1): a team's packet is lost with this probability; levels in 0..VSS_ACTUATE_MAX_LEVELS:
 * the command is rounded to a multiple of 1 / levels (0: not quantised).  A zero switches its effect off. */
typedef struct vss_actuate_params {
  float gain_sigma, noise_sigma, deadband, loss_prob;
  int32_t levels;
} vss_actuate_params;

/* One control step of the channel, one launch.  cmd, out: commands in the layout (out may be cmd itself: in
 * place; otherwise they must not overlap).  held, gain: (n_teams, n_fields, robots, 2) fp32 packed, the last
 * received command and the episode's gains; episode: (n_fields) uint32.  done_prev: the int64 done flags the
 * previous step returned, one every done_stride elements; NULL is the start call (every field begins an episode).
 * seed, call: the Philox key and the call index of the draws; fields, entities and teams index them, never the
 * layout, so two channels with one seed and call index act in one world.
 *
 * VSS_E_ARG, before any HIP call: a null lay, prm, cmd, held, gain, episode or out; cmd, out, held, gain or
 * done_prev not 8-B or episode not 4-B aligned; out partly overlapping cmd; held, gain or episode overlapping each
 * other, cmd, out or done_prev; a parameter outside its range above or not finite; robots not 1 or 3; n_teams not
 * 1 or 2; first_team not 0 or 1; field_stride < robots; with two teams a team_stride smaller than a block's span;
 * done_stride < 1 with done_prev given; n_fields < 0; sizes whose grid or byte offsets overflow.
 * n_fields == 0: VSS_OK, no launch. */
int vss_actuate(void* stream, int64_t n_fields, const vss_actuate_layout* lay, const vss_actuate_params* prm,
                uint64_t seed, uint32_t call, const float* cmd, const int64_t* done_prev, int64_t done_stride,
                float* held, float* gain, uint32_t* episode, float* out);

/* ---------------------------------------------------------------------------------------------
 * The estimation channel (csrc/vss_estimate.hip; vss_amd/estimate.py): delayed observation rows
 * rolled forward to the present with the project's own drive model.
 *
 * A row is the 52-float observation row of envs/vss.py compute_obs: ball x y vx vy [0:4]; own robot j at 4 + 9 j:
 * x y vx vy cos sin w aL aR; opponent j at 31 + 7 j: x y vx vy cos sin w.  A perceived row (vss_perceive) is the state
 * of `lead` control steps ago, but its six own-action floats (11, 12, 20, 21, 29, 30) are the current step's
 * commands.  One call turns each row into an estimate of the present: DESIGN.md §3's drive, damping and integration
 * steps, run `lead` times with the commands the row's team gave in the meantime (kept here, in `hist`), every row in
 * its own frame and independently of every other.  There are no contacts and no walls.
 * vss_amd/estimate.py reference_estimate is the specification; the kernel equals it bit for bit.
 * ------------------------------------------------------------------------------------------- */
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

/* ---------------------------------------------------------------------------------------------
 * The tracking channel (csrc/vss_track.hip; vss_amd/track.py): a recursive tracker between perception
 * and estimation.
 *
 * Every perceived 52-float row (the perception channel) is filtered in its own frame across calls -- predicted one
 * control step with the project's drive model, then corrected with the new row by a fixed gain per kind of body,
 * behind a position / velocity / heading gate -- in one launch per call.  vss_amd/track.py reference_track is the
 * specification; the kernel equals it bit for bit.
 * ------------------------------------------------------------------------------------------- */
#define VSS_TRACK_MAX_DELAY 15

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
 * VSS_E_ARG, before any HIP call: a null lay, prm, obs, done, est, age or obs_out; hist null with delay >= 1;
 * exactly one of term / term_out null; a row pointer or est not 16-B, done or hist not 8-B or age not 4-B aligned;
 * an output (obs_out, term_out, est, hist, age) whose byte range overlaps an input's or another output's; delay
 * outside 0..VSS_TRACK_MAX_DELAY; a gain outside [0, 1] or not finite; a negative or non-finite gate; robots not 1
 * or 3; n_teams not 1 or 2; field_stride < robots; with two teams a team_stride smaller than a block's span;
 * done_stride < 1; n_fields < 0; sizes whose grid or byte offsets overflow.  n_fields == 0: VSS_OK, no launch. */
int vss_track(void* stream, int64_t n_fields, const vss_track_layout* lay, const vss_track_params* prm, int32_t delay,
              uint32_t call, const float* obs, const float* term, const int64_t* done, int64_t done_stride,
              float* est, float* hist, int32_t* age, float* obs_out, float* term_out);

/* ---------------------------------------------------------------------------------------------
 * The set plays (csrc/vss_setplay.hip; vss_amd/setplay.py): named restarts instead of the uniform drop.
 *
 * A share of the fields that finished an episode starts the next one from a named, table-driven placement -- a
 * kickoff, a free ball, a penalty ... -- with jitter and mirroring instead of the step's uniform drop: one launch
 * per call, after the step, over the step's own state and observation rows.  vss_amd/setplay.py reference_setplay
 * is the specification; the kernel equals it bit for bit.
 * ------------------------------------------------------------------------------------------- */
#define VSS_SETPLAY_MAX_PLAYS 8

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

/* Observation rows to rewrite for a placed field (the set plays' and the referee's), as vss_perceive_layout: strides
 * in 52-float rows; the row of team block b, field f, robot k is obs + (b * team_stride + f * field_stride + k) * 52
 * floats and is the view of robot k of team first_team + b.  team_stride is read with two teams only.
 *   SA, CMA: 1, -, 1, 1, 0      DMA: 3, -, 3, 1, 0      opp_obs (N,3,52): 3, -, 3, 1, 1
 *   mirror: R, R N, R, 2, 0     FULL's (N,2,3,52): 6, 3, 3, 2, 0 */
typedef struct vss_setplay_view {
  float* obs;
  int64_t field_stride, team_stride;
  int32_t robots, n_teams, first_team;
} vss_setplay_view;

/* One call, one launch.  Per field f that is done (done NULL: the start call, every field), with the draws of
 * Philox4x32-10, key (seed lo, seed hi), counter (f, call, 10 << 24, block) -- see reference_setplay for the words:
 *   staged = u_share < share;   k = the first play with u_play * total_weight < cum_weight
 *   every entity at its anchor + (2u - 1) r, then flip_y (y, vy, yaw negated), then flip_x (the teams swapped,
 *   x, vx negated, yaw -> pi - yaw), the yaw wrapped into [-pi, pi], (qz, qw) = sincos_small(yaw / 2)
 * A staged field's 58 state channels (state is (58, n_fields), VSS_CH_*) and its rows in every view are written --
 * the rows as vss_compute_observations gives them from that state with zero own-action floats -- chosen[f] = k and
 * counts[k] += 1; every other field's state and rows stay and chosen[f] = -1.
 *
 * VSS_E_ARG, before any HIP call: a null tab or state; views null with n_views > 0; n_views outside 0..2;
 * a view with a null obs, robots not 1 or 3, n_teams not 1 or 2, first_team + n_teams > 2, first_team < 0,
 * field_stride < robots, or with two teams blocks that overlap (team_stride neither a block's span nor, with both
 * teams inside one field stride as in FULL, robots <= team_stride <= field_stride - robots); obs not 16-B, done or counts
 * not 8-B, state or chosen not 4-B aligned; done_stride < 1 with a done; n_fields < 0; sizes whose grid or byte
 * offsets overflow; an output (state, a view's rows, counts, chosen) whose byte range overlaps done's or another
 * output's; and a table that vss_amd/setplay.py Table.validate refuses: a count outside 1..8, a non-finite value, a
 * share or flip probability outside [0, 1], cumulative weights that decrease, are negative or end at 0, or a
 * total_weight that is not the last of them, |anchor yaw| > pi, r_yaw outside [0, pi], a negative radius, a robot
 * with |x| + r_pos > 0.71 or |y| + r_pos > 0.61, a ball with |x| + r_pos > 0.75 or |y| + r_pos > 0.65, or two
 * entities with |anchor distance| - sqrt(2) (r_i + r_j) < 0.08.  n_fields == 0: VSS_OK, no launch. */
int vss_setplay(void* stream, int64_t n_fields, const vss_setplay_table* tab, uint64_t seed, uint32_t call,
                const int64_t* done, int64_t done_stride, float* state, int32_t n_views,
                const vss_setplay_view* views, int64_t* counts, int32_t* chosen);

/* ---------------------------------------------------------------------------------------------
 * The referee (csrc/vss_referee.hip; vss_amd/referee.py): stoppages inside an episode.
 *
 * Inside an episode a VSS match is stopped for a free ball (the ball is stuck), a penalty (two defenders in their own
 * goal area with the ball) and a goal kick (two attackers in it), and restarts from the matching placement.  One launch
 * per call, after the step and after the set plays, over the step's own state, dof velocities and observation rows:
 * per field three counters are advanced and, where one reaches its threshold, the field is placed again from a table
 * of three plays.  vss_amd/referee.py reference_referee is the specification; the kernel equals it bit for bit.
 * ------------------------------------------------------------------------------------------- */
#define VSS_REFEREE_PLAYS 3   /* free ball, penalty, goal kick */
#define VSS_REFEREE_CODES 8   /* verdict codes, the length of counts */

/* A play: seven entities (vss_setplay_entity), the ball's velocity and its jitter; written as blue's own piece in the
 * +y half. */
typedef struct vss_referee_play { vss_setplay_entity e[7]; float ball_vx, ball_vy, r_vel; } vss_referee_play;

/* play[0] the free ball, play[1] the penalty, play[2] the goal kick */
typedef struct vss_referee_table { vss_referee_play play[3]; } vss_referee_table;

/* stall_speed_sq: the ball counts as stuck while vx^2 + vy^2 is below it; area_x, area_y: a goal area is |x| > area_x
 * and |y| < area_y; stall_steps, area_steps: the steps a condition must hold for a call (0: that call is off);
 * max_stops: calls per episode (0: no cap). */
typedef struct vss_referee_params {
  float stall_speed_sq, area_x, area_y;
  int32_t stall_steps, area_steps, max_stops;
} vss_referee_params;

/* One call, one launch.  counters is (n_fields, 4) int32: stall, defend, attack, stops.  views: the rows to rewrite for
 * a whistled field, as vss_setplay's.  Per field f:
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
 * VSS_E_ARG, before any HIP call: a null tab, prm, state, dof_vel or counters; views null with n_views > 0;
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
 * lie inside a goal area (|x| + r_pos > area_x and |y| - r_pos < area_y).  n_fields == 0: VSS_OK, no launch. */
int vss_referee(void* stream, int64_t n_fields, const vss_referee_table* tab, const vss_referee_params* prm,
                uint64_t seed, uint32_t call, const int64_t* done, int64_t done_stride, float* state, float* dof_vel,
                int32_t* counters, int32_t n_views, const vss_setplay_view* views, int64_t* counts, int32_t* verdict);

#ifdef __cplusplus
}
#endif

#endif /* VSS_AMD_VSS_H */
