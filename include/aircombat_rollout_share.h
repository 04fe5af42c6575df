/* aircombat_rollout_share.h -- C ABI of the device MAPPO rollout collector: a whole rollout of the share runner queued in one call.
 *
 * The MAPPO twin of aircombat_rollout.h. With the env (aircombat.h), the MAPPO rollout policy and opponent pool (aircombat.h,
 * ac_policy_mappo_create / AC_POOL_MAPPO) and the shared rollout buffer (aircombat_buffer.h, share_obs_dim > 0) in HBM, one step of
 *   R/runner/share_jsbsim_runner.py:157-185 (collect), :196-223 (insert)   (R = the reference repository)
 * is the policy launch, the opponent launch (self-play), the env step and the runner's insert(). ac_share_rollout_collect queues n such
 * steps from C++ with no host work in between; insert() and SharedReplayBuffer.insert (R/algorithms/utils/buffer.py:312-343) are one
 * kernel, the share post-step kernel (csrc/rollout_collect.hpp). Same library as aircombat.h (libaircombat_hip.so), same errors:
 * 0 on success, -1 on failure with the message in ac_last_error(). One caller thread per handle.
 *
 * The learner owns agents [0, na) of every env (na = A, or A / 2 for self-play) and the buffer's N = E * na columns, in (env, agent)
 * order. share_obs of a column is its env's whole observation block, A * obs_dim floats. Step t of a call works on buffer slot
 * s = the buffer's step index + t:
 *   learner   actor reads OBS[s] (compact [N][obs_dim] rows), critic reads SHARE_OBS[s] ([N][share_obs_dim] rows), both RNN_ACTOR[s],
 *             RNN_CRITIC[s], MASKS[s]; writes its actions into the env's action rows, VALUES[s], the new GRU states into
 *             RNN_ACTOR[s + 1], RNN_CRITIC[s + 1] and its log-probs into a scratch array [N] of the collector's
 *   opponent  acts for agents [na, A) from the env's observations with the collector's own GRU states and masks (in place)
 *   env       ac_step_async_device's launches (the low-level controller first for hierarchical handles)
 *   post-step dones_env = all agents of the env done; the env's obs / rewards / the learner's action columns -> OBS[s + 1], REWARDS[s],
 *             ACTIONS[s]; the env's observation block -> SHARE_OBS[s + 1]; the scratch log-prob into every column of LOGP[s];
 *             MASKS[s + 1] = 1 - dones_env; ACTIVE_MASKS[s + 1] = 0 where the agent is done and its env is not, else 1; rows of
 *             RNN_ACTOR[s + 1], RNN_CRITIC[s + 1] and of the opponent's states zeroed where dones_env; the opponent's masks =
 *             1 - dones_env. BAD_MASKS is left alone (SharedReplayBuffer.insert never forwards it).
 *
 * Streams: as aircombat_rollout.h. Every launch of a call goes to the env's stream (ac_stream), in program order. On entry that stream
 * is made to wait for the work already queued on the caller's `stream` and on the buffer's stream; on return both are made to wait for
 * the last post-step kernel: two events at each end, none per step, nothing waited for on the host.
 */
#ifndef AIRCOMBAT_ROLLOUT_SHARE_H
#define AIRCOMBAT_ROLLOUT_SHARE_H
#include <stdint.h>
#include "aircombat.h"
#include "aircombat_buffer.h"
#include "aircombat_rollout.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ac_share_rollout ac_share_rollout_t;

/* cfg: ac_rollout_config_t with the same na, opponent kinds and deterministic flags; opponent kind 1 is an actor-only ac_policy_t of
 * the MAPPO form, kind 2 an AC_POOL_MAPPO ac_policy_pool_t whose plan is already assigned.
 * Refused, naming the mismatch: handles on different devices; a PPO-form learner or a buffer with share_obs_dim == 0; share_obs_dim
 * other than A * obs_dim, or the learner's cent_obs_dim other than share_obs_dim; logp_dim other than act_dim; E, na, obs_dim, act_dim
 * or the hidden size disagreeing between env, policy and buffer; a learner without a critic; na other than A or A / 2; an opponent kind
 * that does not fit A - na; a PPO-form opponent policy or pool; a pool with no assignment or one assigned for another E. The handles
 * must outlive the collector. */
int ac_share_rollout_create(ac_env_t* env, ac_policy_t* learner, ac_buffer_t* buffer, void* opponent, const ac_rollout_config_t* cfg,
                            ac_share_rollout_t** out);
int ac_share_rollout_destroy(ac_share_rollout_t* r);
/* the opponent's GRU states [E * (A - na)][128] (zero at creation) and masks [E * (A - na)] (one at creation): device memory the
 * collector owns; both NULL without an opponent */
int ac_share_rollout_opponent_state(ac_share_rollout_t* r, float** d_h, float** d_masks);
/* Queue n_steps steps starting at the buffer's step index and return; step t draws with counter0 + t. The buffer's step index
 * advances as n_steps inserts advance it. Refused before anything is queued or written: n_steps < 1, step index + n_steps >
 * buffer_size, weights not loaded, a hierarchical env whose controller is not loaded. Should the runtime refuse a launch later, the
 * call returns -1 after queuing the exit ordering, and the buffer's step index has advanced by the steps queued in full. */
int ac_share_rollout_collect(ac_share_rollout_t* r, void* stream, int32_t n_steps, uint64_t learner_seed, uint64_t learner_counter0,
                             uint64_t opponent_seed, uint64_t opponent_counter0);

/* The share post-step kernel's row function on host arrays (no GPU, no handle): one step at buffer slot s of a buffer with T slots.
 * Env side: obs [E][A][obs_dim], rewards [E][A], dones uint8 [E][A], actions [E][A][env_act_dim]; logp [N], the learner's summed
 * log-probs of the step. Buffer side, whole arrays in the layout of aircombat_buffer.h with N = E * na columns:
 * OBS [T + 1][N][obs_dim], SHARE_OBS [T + 1][N][A * obs_dim], REWARDS [T][N], ACTIONS, LOGP [T][N][act_dim], MASKS, ACTIVE_MASKS
 * [T + 1][N], RNN_ACTOR, RNN_CRITIC [T + 1][N][hidden]. opp_h [E * (A - na)][hidden] and opp_masks [E * (A - na)] may both be NULL. */
typedef struct {
  int32_t E, A, na, obs_dim, env_act_dim, act_dim, hidden, T, s;
  const float *obs, *rewards, *actions;
  const uint8_t* dones;
  const float* logp;
  float *OBS, *SHARE_OBS, *REWARDS, *ACTIONS, *LOGP, *MASKS, *ACTIVE_MASKS, *RNN_ACTOR, *RNN_CRITIC;
  float *opp_h, *opp_masks;
} ac_share_rollout_post_step_t;
int ac_share_rollout_post_step_host(const ac_share_rollout_post_step_t* step);

#ifdef __cplusplus
}
#endif
#endif
