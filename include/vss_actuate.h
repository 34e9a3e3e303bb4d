/* vss_actuate.h — the actuation channel: what a VSS robot's wheels receive of what a policy commands
 * (libvss_actuate.so, csrc/actuate/vss_actuate.hip, vss_amd/actuate.py).
 *
 * A library of its own beside libvss_amd.so: include/vss.h, its 61 entry points and the core library's source
 * stamp are untouched.  The conventions are vss.h's: `stream` is a hipStream_t (NULL: the default stream), every
 * pointer is device memory, the return value is VSS_OK or a VSS_E_* code of vss.h, and nothing synchronises.
 *
 * A command is the two floats (left wheel, right wheel) of one robot.  One call takes the commands of one control
 * step through the channel: the radio's range and 8-bit-like quantisation, the loss of a team's packet (the robot
 * keeps the command it had), a deadband, the episode's per-wheel motor gains and per-step command noise.
 * vss_amd/actuate.py reference_actuate is the specification; the kernel equals it bit for bit.
 */
#ifndef VSS_AMD_VSS_ACTUATE_H
#define VSS_AMD_VSS_ACTUATE_H

#include <stdint.h>

#include "vss.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSS_ACTUATE_ABI_VERSION 1
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

int vss_actuate_abi_version(void);

/* The first 16 hex digits of sha256 over the files of csrc/actuate/Makefile's STAMPED line, as built. */
const char* vss_actuate_source_hash(void);

#ifdef __cplusplus
}
#endif

#endif /* VSS_AMD_VSS_ACTUATE_H */
