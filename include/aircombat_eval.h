/* aircombat_eval.h -- C ABI of the device evaluator: evaluation episodes of the runners queued from C++, with a per-env episode log.
 *
 * With the env (aircombat.h) and the policies or the opponent pool (aircombat.h, ac_policy_*) in HBM, one step of a runner's eval() loop
 *   R/runner/jsbsim_runner.py:136-172, R/runner/selfplay_jsbsim_runner.py:127-239, R/runner/share_jsbsim_runner.py:226-300
 *   (R = the reference repository)
 * is act() for the learner, act() for the opponent (self-play), the env step and numpy bookkeeping: dones_env, the cumulative rewards,
 * the returns of the episodes that ended, zeroed GRU rows and masks. ac_eval_run queues n such steps with no host work in between; the
 * bookkeeping is one kernel, the post-step kernel (csrc/eval_collect.hpp). Same library as aircombat.h (libaircombat_hip.so), same
 * errors: 0 on success, -1 on failure with the message in ac_last_error(). One caller thread per handle.
 *
 * The learner owns agents [0, na) of every env (na = A, or A / 2 for self-play), the opponent agents [na, A). Both sides read the env's
 * own observation buffer; there is no rollout buffer, no critic and no share_obs. The evaluator owns both sides' GRU states and masks,
 * the running sums and the log, all in device memory. Step t of the evaluator (t counts from ac_eval_begin):
 *   learner   acts for agents [0, na) from the env's observations, its states in place, its actions into the env's action rows
 *   opponent  the same for agents [na, A)
 *   env       ac_step_async_device's launches (the low-level controller first for hierarchical handles)
 *   post-step dones_env = all agents of the env done (the opponent's included). Per env e:
 *               cum[e][a] += rewards[e][a] for every agent a (float32, one add per step, in step order); len[e] += 1
 *               where dones_env: if count[e] < K, log slot count[e] := (cum[e][:], len[e], t), and if that was slot K - 1,
 *                 remaining -= 1; then count[e] += 1, cum[e][:] = 0, len[e] = 0 (episodes after the K-th are counted, not logged);
 *                 the env's rows of both sides' GRU states are zeroed
 *               both sides' masks of the env's rows = 1 - dones_env, every step
 *
 * Streams. Every launch goes to the env's stream (ac_stream), in program order. On entry that stream is made to wait for the work
 * already queued on the caller's `stream`; on return the caller's stream is made to wait for the last kernel: one event at each end,
 * none per step, nothing waited for on the host.
 */
#ifndef AIRCOMBAT_EVAL_H
#define AIRCOMBAT_EVAL_H
#include <stdint.h>
#include "aircombat.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ac_eval ac_eval_t;
enum { AC_EVAL_NO_OPPONENT = 0, AC_EVAL_OPPONENT_POLICY = 1, AC_EVAL_OPPONENT_POOL = 2, AC_EVAL_MAX_EPISODES = 64 };
typedef struct {
  int32_t na;                    /* learner agents [0, na) of every env: A, or A / 2 */
  int32_t opponent_kind;         /* 0 none, 1 an ac_policy_t of the learner's form, 2 an ac_policy_pool_t of the learner's form whose plan is assigned */
  int32_t learner_deterministic, opponent_deterministic;
  int32_t episodes_per_env;      /* K: log slots per env, 1 .. AC_EVAL_MAX_EPISODES */
} ac_eval_config_t;

/* The learner is an ac_policy_t of either form (ac_policy_create / ac_policy_mappo_create); only its actor is used, a critic is ignored
 * and an actor-only policy is accepted. Refused, naming the mismatch: handles on different devices; obs_dim disagreeing; the env's
 * act_dim smaller than a side's heads; na other than A or A / 2; an opponent kind that does not fit A - na; an opponent of the other
 * form; a pool without an assignment or assigned for another E; K out of range. The handles must outlive the evaluator. */
int ac_eval_create(ac_env_t* env, ac_policy_t* learner, void* opponent, const ac_eval_config_t* cfg, ac_eval_t** out);
int ac_eval_destroy(ac_eval_t* ev);
/* Queue the start of an evaluation, ordered around `stream` as ac_eval_run is: both sides' GRU states zero, both masks one, cum, len,
 * count and the log zero, remaining = E, the evaluator's step index 0. The env is not reset: the caller resets it first. */
int ac_eval_begin(ac_eval_t* ev, void* stream);
/* Queue n_steps steps and return; step t of the call draws with counter0 + t. Refused before anything is queued or written:
 * n_steps < 1, a call before ac_eval_begin, weights not loaded, a pool whose assignment no longer covers the env's E, a hierarchical env
 * whose controller is not loaded. Should the runtime refuse a launch later, the call returns -1 after queuing the exit ordering, and
 * the evaluator's step index has advanced by the steps queued in full. */
int ac_eval_run(ac_eval_t* ev, void* stream, int32_t n_steps, uint64_t learner_seed, uint64_t learner_counter0, uint64_t opponent_seed,
                uint64_t opponent_counter0);

/* Everything the evaluator owns (device pointers, valid while it lives) and its sizes. opp_h / opp_masks are NULL without an opponent.
 * log_end holds the evaluator's step index t of the step that ended the episode; remaining is the number of envs with count < K. */
typedef struct {
  int32_t E, A, na, K;
  int32_t step;                  /* steps queued since ac_eval_begin; -1 before the first ac_eval_begin */
  int32_t pad_;
  float *lrn_h, *lrn_masks;      /* [E * na][128], [E * na] */
  float *opp_h, *opp_masks;      /* [E * (A - na)][128], [E * (A - na)] */
  float* cum;                    /* [E][A] */
  int32_t *len, *count;          /* [E], [E] */
  float* log_ret;                /* [E][K][A] */
  int32_t *log_len, *log_end;    /* [E][K], [E][K] */
  int32_t* remaining;            /* [1] */
} ac_eval_state_t;
int ac_eval_state(ac_eval_t* ev, ac_eval_state_t* out);

/* The post-step kernel's work-item function on host arrays (no GPU, no handle): step `step` of an evaluation. rewards [E][A], dones
 * uint8 [E][A]; the other arrays as in ac_eval_state_t with `hidden` floats per GRU row. opp_h and opp_masks may both be NULL. */
typedef struct {
  int32_t E, A, na, hidden, K, step;
  const float* rewards;
  const uint8_t* dones;
  float *lrn_h, *lrn_masks, *opp_h, *opp_masks;
  float* cum;
  int32_t *len, *count;
  float* log_ret;
  int32_t *log_len, *log_end;
  int32_t* remaining;
} ac_eval_post_step_t;
int ac_eval_post_step_host(const ac_eval_post_step_t* step);

#ifdef __cplusplus
}
#endif
#endif
