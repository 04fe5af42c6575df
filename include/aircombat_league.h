/* aircombat_league.h -- C ABI of the device league: a round-robin of the members of an opponent pool against each other, queued from
 * C++, with a per-env episode log and its reduction into a payoff table of member i (agents [0, A/2)) against member j (agents [A/2, A)).
 *
 * The reference keeps one Elo number per checkpoint, moved only when the checkpoint is drawn against `latest`
 * (R/runner/selfplay_jsbsim_runner.py:136-227; R = the reference repository), and PFSP.choose (R/algorithms/utils/selfplay.py:50-60)
 * samples from those numbers. The table of every member against every other is what prioritised fictitious self-play, Nash averaging or
 * pruning a pool start from. Same library as aircombat.h (libaircombat_hip.so), same errors: 0 on success, -1 on failure with the message
 * in ac_last_error(). One caller thread per handle.
 *
 * The pool holds a sided assignment (ac_policy_pool_assign_sides, aircombat.h): members2[e] = (i, j). The league owns ONE state array for
 * both sides, h [E * A][128] and masks [E * A] in (env, agent) order, the running sums and the log. Step t (t counts from
 * ac_league_begin):
 *   pool      ONE launch of ac_policy_pool_act over the whole range: every agent of every env acts with its side's member from the env's
 *             observations, its state in place, its actions into the env's action rows
 *   env       ac_step_async_device's launches (the low-level controller first for hierarchical handles), so an attached flight
 *             recorder or spawn bank works as it does for the evaluator
 *   post-step the evaluator's bookkeeping (header comment of aircombat_eval.h) over the one state array. dones_env = all agents of the
 *             env done. Per env e:
 *               cum[e][a] += rewards[e][a] for every agent a (float32, one add per step, in step order); len[e] += 1
 *               where dones_env: if count[e] < K, log slot count[e] := (cum[e][:], len[e], t, word 1 of the env's info row of this
 *                 step = its AC_DONE_* code), and if that was slot K - 1, remaining -= 1; then count[e] += 1, cum[e][:] = 0,
 *                 len[e] = 0 (episodes after the K-th are counted, not logged); the env's A rows of h are zeroed
 *               the masks of the env's rows = 1 - dones_env, every step
 *
 * Streams. As aircombat_eval.h: every launch goes to the env's stream; on entry it waits for the work already queued on the caller's
 * `stream`, on return the caller's stream waits for the last kernel. ac_league_run waits for nothing on the host. ac_league_begin reads
 * the assignment back once (8 E + 8 bytes) to refuse a side assigned -1 or a member that is not loaded.
 */
#ifndef AIRCOMBAT_LEAGUE_H
#define AIRCOMBAT_LEAGUE_H
#include <stdint.h>
#include "aircombat.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ac_league ac_league_t;
enum { AC_LEAGUE_MAX_EPISODES = 64 };
typedef struct {
  int32_t episodes_per_env;      /* K: log slots per env, 1 .. AC_LEAGUE_MAX_EPISODES */
  int32_t deterministic;         /* both sides */
  float win_margin;              /* finite, >= 0; the reference's threshold is 100 (R/runner/selfplay_jsbsim_runner.py:217-220) */
  int32_t pad_;
} ac_league_config_t;

/* Refused, naming the mismatch: pool and env on different devices; obs_dim disagreeing; the env's act_dim smaller than the heads; odd A;
 * a pool without a sided plan, or with one for another E or A; K out of range; a margin that is negative or not finite. The handles
 * must outlive the league. */
int ac_league_create(ac_env_t* env, ac_policy_pool_t* pool, const ac_league_config_t* cfg, ac_league_t** out);
int ac_league_destroy(ac_league_t* lg);
/* The start of a round, ordered around `stream`: states zero, masks one, cum, len, count and the log zero, remaining = E, the step index
 * 0, and the pool's members2 copied into the league (what ac_league_table groups by). Refused with nothing written: no sided plan for
 * the env's E and A in force, a side assigned -1, a member out of range or not loaded. The env is not reset: the caller resets it. */
int ac_league_begin(ac_league_t* lg, void* stream);
/* Queue n_steps steps and return; step t of the call draws with counter0 + t. Refused before anything is queued or written:
 * n_steps < 1, a call before ac_league_begin, a pool re-assigned since ac_league_begin, a hierarchical env whose controller is not loaded.
 * Should the runtime refuse a launch later, the call returns -1 after queuing the exit ordering, and the step index has advanced by the
 * steps queued in full. */
int ac_league_run(ac_league_t* lg, void* stream, int32_t n_steps, uint64_t seed, uint64_t counter0);

/* Everything the league owns (device pointers, valid while it lives) and its sizes. log_end holds the step index t of the step that
 * ended the episode, log_code its AC_DONE_* code; remaining is the number of envs with count < K. */
typedef struct {
  int32_t E, A, K, C;            /* C: the pool's capacity, the side of the table */
  int32_t step;                  /* steps queued since ac_league_begin; -1 before the first ac_league_begin */
  int32_t pad_;
  float *h, *masks;              /* [E * A][128], [E * A] */
  float* cum;                    /* [E][A] */
  int32_t *len, *count;          /* [E], [E] */
  float* log_ret;                /* [E][K][A] */
  int32_t *log_len, *log_end, *log_code;   /* [E][K] each */
  int32_t* members2;             /* [E][2]: the assignment as of ac_league_begin */
  int32_t* remaining;            /* [1] */
} ac_league_state_t;
int ac_league_state(ac_league_t* lg, ac_league_state_t* out);

/* The post-step kernel's work-item function on host arrays (no GPU, no handle): step `step` of a round. rewards [E][A], dones uint8
 * [E][A], info int32 [E][4]; the other arrays as in ac_league_state_t with `hidden` floats per GRU row. */
typedef struct {
  int32_t E, A, hidden, K, step, pad_;
  const float* rewards;
  const uint8_t* dones;
  const int32_t* info;
  float *h, *masks;
  float* cum;
  int32_t *len, *count;
  float* log_ret;
  int32_t *log_len, *log_end, *log_code;
  int32_t* remaining;
} ac_league_post_step_t;
int ac_league_post_step_host(const ac_league_post_step_t* step);

/* ---- the payoff table. Cell (i, j) covers every logged episode (slot < min(count[e], K)) of every env with members2[e] = (i, j).
 * The side reward of an episode is the float32 mean of the side's agents' logged returns, summed in agent order from 0.0f, then divided
 * by A / 2 (the convention of the evaluator's per-opponent averages and of the spawn bank). With d = ra - rb in float32: d > margin is a
 * win for side a, d < -margin a win for side b, anything else (exactly +margin or -margin included) a draw. sum_a / sum_b accumulate
 * the side rewards in float64, steps sums log_len, timeouts counts log_code == AC_DONE_TIMEOUT.
 *
 * The summation order is part of the contract, so that the table is bit-identical from run to run and equal to the host twin:
 *   1. each env's partial sums run over its slots ascending, from 0.0 (parallel over envs);
 *   2. each cell's total runs over its envs' partials ascending by env, from 0.0 (parallel over cells).
 * No floating-point atomics. Cells without episodes are all-zero. */
typedef struct { int64_t episodes, wins_a, wins_b, draws, timeouts, steps; double sum_a, sum_b; } ac_league_cell_t;   /* 64 bytes */
/* d_out: [C][C] cells in device memory, C the pool's capacity; queued around `stream` as ac_league_run is. Refused before ac_league_begin. */
int ac_league_table(ac_league_t* lg, void* stream, ac_league_cell_t* d_out);
/* The same reduction on host arrays: the log as in ac_league_state_t, out [C][C]. Envs whose pair is outside [0, C) are left out. */
typedef struct {
  int32_t E, A, K, C;
  float margin;
  int32_t pad_;
  const float* log_ret;
  const int32_t *log_len, *log_code, *count, *members2;
  ac_league_cell_t* out;
} ac_league_table_args_t;
int ac_league_table_host(const ac_league_table_args_t* args);

#ifdef __cplusplus
}
#endif
#endif
