/* aircombat_spawn.h -- C ABI of the spawn curriculum: a bank of K reset templates in HBM and a per-env stage that picks the template
 * every reset of that env respawns from, kept and advanced on the device.
 *
 * The *_curriculum tasks of the reference (R/envs/JSBSim/tasks/scenario1_task.py:147-195, scenario2_task.py:318-383; R = the reference
 * repository) respawn the ego team from env.reset_simulators_curriculum(angle), 181 stages on a circle about the enemy
 * (singlecombat_env.py:87-122, multiplecombat_env.py:185-248), and mean to advance the angle with the ego win rate. A handle has one
 * reset template, built by the create call; every env and every auto-reset inside the step kernels copies it. A bank attached to a
 * handle holds K more templates, built by the handle's own init kernel from K rows of initial conditions, and one small kernel queued
 * behind every step (and behind ac_reset) re-copies the envs that have just been reset from the bank entry their stage selects. The
 * step kernels are untouched: what their reset has already done and does not depend on the spawn (munition slots, extension state,
 * controller rows) stays as they left it. Same library as aircombat.h (libaircombat_hip.so), same errors: 0 on success, -1 on failure
 * with the message in ac_last_error and nothing changed. One caller thread per handle.
 *
 * Per env, after every step, in this order (the shared body behind ac_spawn_post_step_host):
 *   1. ret_acc += (rew[0] + ... + rew[n_ego - 1]) / n_ego, in float32, in that operation order;
 *   2. where the step's info row says the env was reset (word 3), the episode ends: played += 1, return_sum += ret_acc, the win bit
 *      (ret_acc >= win_return) is shifted into the 32-bit register `wins` from below, ret_acc = 0. Behind ac_reset every env ends its
 *      running episode without scoring it (ret_acc = 0 alone);
 *   3. mode AC_SPAWN_AUTO: if played >= window and popcount(wins & the low `window` bits) >= min_wins, then stage = min(stage + 1, K - 1)
 *      and played, wins and return_sum are cleared;
 *   4. episode += 1 and the entry is chosen: AC_SPAWN_AT takes clamp(stage, 0, K - 1), AC_SPAWN_UPTO draws uniformly from
 *      [0, clamp(stage, 0, K - 1)] with the library's keyed generator, key (seed, env, episode) -- ac_spawn_draw_host is that draw;
 *   5. `spawned` takes the entry's index, and the entry's state and reset observation are copied over the env (into the device buffers
 *      and, on a host step, into the step's host set).
 * An env that was not reset costs one info word, n_ego rewards and its accumulator. The stage is clamped on the device at every use:
 * whatever the caller writes into `stage`, no index leaves the bank. A written stage takes effect at that env's next reset.
 *
 * Hooks. Behind every step the handle takes (ac_step, ac_step_host*, ac_step_async_device, ac_step_timed_device, the steps queued by the
 * collectors and the evaluator) and behind ac_reset, ahead of the flight recorder's capture, so a recorded frame shows the respawned
 * aircraft. A handle with a bank attached takes its host steps through HIP launches instead of the AQL queue. With nothing attached
 * every path dispatches exactly as it does without this header.
 *
 * Out of scope: AC_TASK_HEADING (it has no template: every reset draws inside the kernel), snapshots (a snapshot carries no stage;
 * restoring or cloning envs leaves the per-env arrays as they are), per-stage changes to anything but initial conditions, graph capture.
 */
#ifndef AIRCOMBAT_SPAWN_H
#define AIRCOMBAT_SPAWN_H
#include <stdint.h>
#include "aircombat.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ac_spawn ac_spawn_t;
enum { AC_SPAWN_FIXED = 0, AC_SPAWN_AUTO = 1 };   /* mode: the stage moves only when the caller writes it / by the rule of step 3 */
enum { AC_SPAWN_AT = 0, AC_SPAWN_UPTO = 1 };      /* sample: the stage's own entry / a keyed uniform draw from the entries up to it */
enum { AC_SPAWN_MAX_BANK = 1024, AC_SPAWN_MAX_WINDOW = 32 };

typedef struct ac_spawn_config {
  int32_t mode, sample;
  int32_t window;        /* 1 .. 32 episodes */
  int32_t min_wins;      /* 1 .. window */
  float win_return;      /* an episode whose mean ego return reaches it is a win; finite in AC_SPAWN_AUTO */
  int32_t pad_;
  uint64_t seed;         /* key of the AC_SPAWN_UPTO draws */
} ac_spawn_config_t;

/* What the attach call refuses without needing a device: a task without a template (AC_TASK_HEADING), K outside 1 .. 1024, an entry
 * that the create call would refuse as cfg.init (non-finite, latitude beyond 89 deg, altitude outside -1400 .. 85000 ft; the message
 * names the entry), window outside 1 .. 32, min_wins outside 1 .. window, a non-finite win_return in AC_SPAWN_AUTO, unknown mode or
 * sample. init is [K][A] (NULL: the rule alone is checked). */
int ac_spawn_check(int32_t task, int32_t A, const ac_init_state_t* init, int32_t K, const ac_spawn_config_t* cfg);

/* Builds the bank from init[K][A] (A = the handle's aircraft per env) with the handle's own init kernel and attaches it. The per-env
 * arrays start at stage 0, spawned -1 (the handle's own template), everything else 0. Refused besides the above: a second bank on one
 * handle, an allocation the runtime refuses. */
int ac_spawn_attach(ac_env_t* env, const ac_init_state_t* init, int32_t K, const ac_spawn_config_t* cfg, ac_spawn_t** out);
/* Detaches and frees the handle's bank (nothing attached: not an error); its ac_spawn_t is gone with it. Destroying the handle does the same. */
int ac_spawn_detach(ac_env_t* env);
/* The mode, rule and sampling from the next step on. */
int ac_spawn_set_config(ac_spawn_t* bank, const ac_spawn_config_t* cfg);

typedef struct ac_spawn_state {
  int32_t E, K;
  int32_t* stage;        /* [E] device pointers, valid while the bank is attached; written on the handle's stream */
  int32_t* spawned;      /* the bank entry of the running episode, -1 before the env's first respawn */
  int32_t* episode;      /* ordinal of the running episode, counted from the attach */
  float* ret_acc;        /* mean ego return of the running episode so far */
  int32_t* wins;         /* shift register of win bits, the latest episode in bit 0 */
  int32_t* played;       /* episodes scored at this stage */
  float* return_sum;     /* sum of their returns */
} ac_spawn_state_t;
int ac_spawn_state(ac_spawn_t* bank, ac_spawn_state_t* out);

/* Steps 1-4 on HOST arrays, the body the spawn kernel runs (compiled for both): rewards [E][A], info [E][4], the per-env arrays [E];
 * index [E] receives the chosen entry, -1 where the env is not respawned. all_envs != 0 is the form queued behind ac_reset. */
typedef struct ac_spawn_post_step {
  int32_t E, A, n_ego, K, all_envs, pad_;
  ac_spawn_config_t cfg;
  const float* rewards;
  const int32_t* info;
  int32_t* stage; int32_t* spawned; int32_t* episode; float* ret_acc; int32_t* wins; int32_t* played; float* return_sum;
  int32_t* index;
} ac_spawn_post_step_t;
int ac_spawn_post_step_host(const ac_spawn_post_step_t* step);
/* The AC_SPAWN_UPTO draw of (seed, env, episode) for a clamped stage `stage` >= 0: an index in [0, stage]. */
int ac_spawn_draw_host(uint64_t seed, int64_t env, int64_t episode, int32_t stage, int32_t* index);

#ifdef __cplusplus
}
#endif
#endif
