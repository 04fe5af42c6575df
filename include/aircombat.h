/* aircombat.h — C ABI of the MI355X-native vectorised air-combat step().
 *
 * Drop-in boundary for the reference's VecEnv hot path. Each entry point names the reference interface it
 * replaces ("R/" = junghoseong/aircombat-selfplay). Plain pointers and sizes only; the caller owns every buffer.
 * All functions return 0 on success or a negative error code; ac_last_error() gives the message.
 * Blocking unless the name says _async. One handle drives one GPU; handles are not thread-safe.
 *
 * Non-finite state. A NaN / Inf in an aircraft's integrator state (or its reward) terminates that aircraft like the reference's
 * ExtremeState condition (R/envs/JSBSim/core/catalog.py:386-416, whose `>=` tests a NaN would pass unnoticed) and makes every call that
 * completes a step -- ac_step, ac_step_host_wait / ac_step_host, ac_sync, ac_step_timed_device -- return -1 with
 * "JSBSim failed. Non-finite state or reward in env E, agent A" in ac_last_error(), until ac_reset clears it: the reference's
 * RuntimeError("JSBSim failed.") (R/envs/JSBSim/core/simulatior.py:223-225) in place of its pdb NaN trap (R/envs/JSBSim/envs/env_base.py:277-281).
 *
 * Array conventions (E = n_envs, A = n_agents, row-major, agents ordered ego team first then enemy team,
 * exactly like BaseEnv._pack, R/envs/JSBSim/envs/env_base.py:269-283):
 *   actions  float32 [E][A][act_dim]   integer-valued indices, as the runners hand them over (act_dim = ac_act_dim(): control
 *                                      indices, or the [3,5,3] choice (+ weapon bits) when cfg.hierarchical)
 *   obs      float32 [E][A][obs_dim]
 *   rewards  float32 [E][A]
 *   dones    uint8   [E][A]
 *   info     int32   [E][4] = {current_step, done_code, heading_turn_counts, episode_was_reset}
 */
#ifndef AIRCOMBAT_H
#define AIRCOMBAT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define AC_MAX_AGENTS 8
#define AC_MAX_MISSILES_PER_AGENT 4

/* task semantics, R/envs/JSBSim/tasks/ */
enum {
  AC_TASK_HEADING = 0,        /* heading_task.py:9-110 HeadingTask under SingleControlEnv (BASELINE C1): 1 aircraft, obs 12, act [41,41,41,30],
                                 randomised reset and UnreachHeading draws from the env's numpy Generator(PCG64), see ac_seed_envs */
  AC_TASK_SINGLECOMBAT = 1,   /* singlecombat_task.py:16-207 SingleCombatTask: obs 15, act [41,41,41,30] */
  AC_TASK_DODGE_MISSILE = 2,  /* singlecombat_with_missile_task.py:12-124 rule-based launch from the lock window, MissilePostureReward: obs 21, act 4 */
  AC_TASK_SHOOT_MISSILE = 3,  /* singlecombat_with_missile_task.py:147-204 learned shoot bit: obs 21, act 5 */
  AC_TASK_SCENARIO1 = 5,      /* scenario1_task.py:11-145 (1v1): gun / AIM-120B / AIM-9M / chaff rules, 11 reward terms; obs 21;
                                 act 8 = [41,41,41,30] + [gun, AIM-9M, AIM-120B, chaff] (low-level control; the controller net is row N1) */
  AC_TASK_SCENARIO_NVN = 6,   /* scenario2_task.py / scenario3_task.py *_NvN (2v2, 4v4) under MultipleCombatEnv.step: obs 9+6A+6, act 8 */
  AC_TASK_WVR = 7,            /* WVR_task.py:10-90 WVRTask (1v1): 15-value observation, unlimited gun, eight reward terms, no SafeReturn; act 4 (or [3,5,3]) */
  AC_TASK_MANEUVER = 8,       /* singlecombat_task.py:264-359 Maneuver_curriculum (1v1): WVR's gun, nine reward terms, the ordinary 1v1 terminations */
  AC_TASK_MULTICOMBAT = 4     /* multiplecombat_task.py:15-151 MultipleCombatTask under MultipleCombatEnv.step (NvN, n_agents 4 or 8):
                                 obs 9+6*(A-1), act [41,41,41,30]; share_obs is obs flattened per env (env_base.py:183-189) */
};
/* AircraftSimulator status, R/envs/JSBSim/core/simulatior.py:93-95 */
enum { AC_ALIVE = 0, AC_CRASH = 1, AC_SHOTDOWN = 2 };
/* which termination condition fired (info['done_condition'] of R/envs/JSBSim/termination_conditions/) */
enum { AC_DONE_NONE = 0, AC_DONE_LOW_ALTITUDE = 1, AC_DONE_EXTREME_STATE = 2, AC_DONE_OVERLOAD = 3, AC_DONE_SHOTDOWN = 4,
       AC_DONE_CRASHED = 5, AC_DONE_MISSION_COMPLETE = 6, AC_DONE_TIMEOUT = 7, AC_DONE_UNREACH_HEADING = 8 };

/* init_state block of a scenario YAML (R/envs/JSBSim/configs/, keys ic_*), defaults of simulatior.py:192-208 */
typedef struct ac_init_state {
  double lon_deg, lat_geod_deg, h_sl_ft, psi_deg, u_fps, v_fps, w_fps, p_rad_sec, q_rad_sec, r_rad_sec;
} ac_init_state_t;

/* Scalars of one scenario YAML as parsed by parse_config (R/envs/JSBSim/utils/utils.py:7-23) */
typedef struct ac_config {
  int32_t task;
  int32_t n_agents;                 /* aircraft per env */
  int32_t n_ego;                    /* first n_ego aircraft are team A */
  int32_t sim_freq;                 /* 60 */
  int32_t agent_interaction_steps;  /* 6 */
  int32_t max_steps;
  double center_lon, center_lat, center_alt;   /* battle_field_center */
  double altitude_limit;            /* m, LowAltitude */
  double acc_limit_x, acc_limit_y, acc_limit_z;
  ac_init_state_t init[AC_MAX_AGENTS];
  int32_t num_missiles[AC_MAX_AGENTS];
  double posture_scale;  int32_t posture_potential;
  double altitude_scale; int32_t altitude_potential;
  double event_scale;    int32_t event_potential;
  double missile_posture_scale;
  double shoot_penalty_scale; int32_t shoot_penalty_potential;
  double alt_safe, alt_danger, alt_kv;
  double max_attack_angle, max_attack_distance; int32_t min_attack_interval;
  int32_t use_artillery;
  /* HeadingTask only: HeadingReward_scale / _potential (reward_function_base.py:14-15), UnreachHeading limits (unreach_heading.py:27-31) */
  double heading_scale; int32_t heading_potential;
  double max_heading_increment, max_altitude_increment, max_velocities_u_increment, check_interval;
  int32_t legacy_obs;               /* Scenario2 / Scenario3 (the non-_NvN classes, scenario2_task.py:14-157): AC_TASK_SCENARIO_NVN rules with the 21-value
                                       observation of MultipleCombatShootMissileTask against the enemy of the same team index */
  int32_t rwr;                      /* *_RWR variants of the scenario tasks: obs_dim + 2 reserved zero slots; Scenario1_RWR also blanks the
                                       missile block of its observation (scenario1_task.py:213-314, scenario2_task.py:385-476) */
  int32_t use_baseline;             /* scripted enemy team (`use_baseline: true`, `baseline_type`, singlecombat_task.py:19-27, model/baseline.py):
                                       0 none, 1 PursueAgent, 2 ManeuverAgent('triangle'); the enemy rows of `actions` are ignored */
  int32_t hierarchical;             /* Hierarchical* / Scenario* tasks as shipped: actions are MultiDiscrete [3,5,3] (+ the four weapon
                                       bits) and go through the low-level controller (singlecombat_task.py:209-262); 0 = control indices */
  int32_t approach;                 /* AC_TASK_HEADING only: ApproachTask (`task: approach`, tasks/approach_task.py:9-120): the same env, reset
                                       draws and observation, reward = AltitudeReward alone, terminations LowAltitude, ExtremeState,
                                       Overload, Timeout (no UnreachHeading: the targets stay at their reset values) */
  int32_t controller_precision;     /* with cfg.hierarchical: the arithmetic of the low-level controller's products. AC_CTL_FAST (0, the
                                       default): two fp16 pieces per value, three terms per product (22 bits per value, the fastest form);
                                       AC_CTL_FP32: three bf16 pieces, six terms -- every product at least as exact as the reference's fp32
                                       (torch on the CPU), at about 1.5x the controller's time. ac_create refuses other values, and a
                                       non-zero value without cfg.hierarchical. AIRCOMBAT_CTL_PRECISION=fast|fp32 in the environment pins
                                       the form of every hierarchical handle created while it is set. */
} ac_config_t;
enum { AC_CTL_FAST = 0, AC_CTL_FP32 = 1 };

typedef struct ac_env ac_env_t;

/* Number of doubles in the per-aircraft state vector of ac_get_state / ac_set_state, and the field names. */
#define AC_STATE_LEN 128
const char* ac_state_field_name(int i);

/* replaces SubprocVecEnv.__init__ (R/envs/env_wrappers.py:231-267): builds E envs on one GPU, runs every
 * aircraft's initial-condition pass (AircraftSimulator.reload, simulatior.py:152-190) on the device */
int ac_create(const ac_config_t* cfg, int32_t n_envs, int32_t device_id, uint64_t seed, ac_env_t** out);
/* replaces SubprocVecEnv.close (env_wrappers.py:300-310) */
int ac_destroy(ac_env_t* h);
int ac_obs_dim(const ac_env_t* h);
int ac_act_dim(const ac_env_t* h);
int ac_num_envs(const ac_env_t* h);
int ac_num_agents(const ac_env_t* h);

/* replaces SubprocVecEnv.reset (env_wrappers.py:284-290) -> obs[E][A][obs_dim] into a HOST buffer */
int ac_reset(ac_env_t* h, float* obs);
/* replaces SubprocVecEnv.step = step_async + step_wait (env_wrappers.py:269-282) with HOST buffers.
 * Envs whose agents are all done are reset inside the call and return the reset observation with the
 * terminal reward/done, like worker() does (env_wrappers.py:191-204). */
int ac_step(ac_env_t* h, const float* actions, float* obs, float* rewards, uint8_t* dones, int32_t* info);

/* Zero-copy form of the same step for the VecEnv shim: the library owns up to AC_HOST_SETS sets of page-locked host buffers that are mapped into
 * the device (rows padded to a multiple of 64 aircraft); the step kernel reads the actions of set `set` straight from host memory
 * and writes obs / rewards / dones / info of the step into the same set -- no copy commands. The caller fills the action buffer,
 * calls ac_step_host_async (= SubprocVecEnv.step_async, R/envs/env_wrappers.py:269-273) and ac_step_host_wait (= step_wait,
 * :275-282); alternating the two sets keeps the arrays of one step valid while the next one runs. The device buffers of
 * ac_device_buffers are written as well. ac_reset(h, obs) may be pointed at a set's obs buffer. */
/* `info` of a set is ONE packed word per env (the four-word rows of ac_step / ac_device_buffers are 11 % of a step's bytes across PCIe
 * otherwise): current_step in bits 0-15, done_code in bits 16-23, heading_turn_counts in bits 24-30, episode_was_reset in bit 31. */
#define AC_INFO_STEP(w) ((int32_t)((uint32_t)(w) & 0xFFFFu))
#define AC_INFO_DONE_CODE(w) ((int32_t)(((uint32_t)(w) >> 16) & 0xFFu))
#define AC_INFO_TURN_COUNTS(w) ((int32_t)(((uint32_t)(w) >> 24) & 0x7Fu))
#define AC_INFO_WAS_RESET(w) ((int32_t)((uint32_t)(w) >> 31))
#define AC_HOST_SETS 8   /* sets 0 .. 7, each allocated by its first ac_host_buffers call */
int ac_host_buffers(ac_env_t* h, int32_t set, float** actions, float** obs, float** rewards, uint8_t** dones, int32_t** info);
/* SubprocVecEnv.step_wait hands the caller arrays it owns for good (np.stack, env_wrappers.py:276-282). The shim gets the same without a
 * copy by handing out a set's arrays only while nobody holds that set's previous ones; a set still held when the VecEnv closes is
 * detached (ac_destroy no longer frees it, the handle can no longer step into it) and freed by its holder with ac_host_set_free. */
int ac_host_set_detach(ac_env_t* h, int32_t set);
void ac_host_set_free(void* actions, void* obs, void* rewards, void* dones, void* info);
int ac_step_host_async(ac_env_t* h, int32_t set);
int ac_step_host_wait(ac_env_t* h);
int ac_step_host(ac_env_t* h, int32_t set);   /* both in one call: VecEnv.step (env_wrappers.py:30-42) */
/* The same step from the caller's own array (`n_floats` = envs x agents x act_dim floats, any alignment): the library copies it into
 * set `set`. For the three-wave SingleCombat kernel (act_dim 4) on the AQL path the order is header word, doorbell, copy, wait: a share
 * (ac_late_config's `fraction`) of the rows crosses into the mapped buffer UNDER the launch. Each 16-byte row then carries a two-bit
 * tag (1 / 2, alternating per use of the set) in the two lowest mantissa bits of its fourth element, which the kernel checks and
 * masks: a throttle index whose two trailing mantissa bits are zero (every integer below 2^22) arrives bit-exact, any other is
 * rounded toward zero by at most 3 ulp. A systems wave whose rows do not carry the step's tag sleeps and asks again, at most `budget`
 * times; then the call returns -1 ("... did not reach the device within the retry budget ...") and every later step does until
 * ac_reset. Every other kernel form, and a handle off the AQL path, copies first, untagged, and then behaves like ac_step_host. */
int ac_step_host_actions(ac_env_t* h, int32_t set, const float* actions, size_t n_floats);
/* The two halves of that call: _begin returns once the doorbell is rung and the batch copied (`actions` is not read after it), _wait
 * blocks until the step is complete and reports like ac_step_host_wait. Host work placed between them runs while the kernel does
 * (the native VecEnv.step, csrc/native_step.cpp, builds what it returns there). After a _begin that returned 0 call _wait exactly once,
 * from the same thread, before any other call on the handle; after one that failed, do not. */
int ac_step_host_actions_begin(ac_env_t* h, int32_t set, const float* actions, size_t n_floats);
int ac_step_host_actions_wait(ac_env_t* h);
#define AC_LATE_FRACTION_DEFAULT 1.0    /* share of the batch copied behind the doorbell (profiles/late_actions_summary.txt) */
#define AC_LATE_BUDGET_DEFAULT 400000   /* tries of ~1.6 us each (a sleep and a read across PCIe): 0.6 s, well under the 10 s AQL deadline */
#define AC_LATE_WINDOW 1024                  /* late steps per window of the self-check */
#define AC_LATE_WINDOW_MAX_RETRY_STEPS 16    /* retrying steps a window may hold: five times what a held-up host thread was seen to cause */
typedef struct {
  int64_t steps;          /* steps taken the late way */
  int64_t retries;        /* row loads the systems waves re-issued, over all of them ... */
  int32_t last_retries;   /* ... and in the last one */
  int32_t last_late;      /* 1: the last host step went the late way */
  int64_t retry_steps;    /* steps in which any load was re-issued */
  int64_t lowered;        /* how often the self-check moved a quarter of the batch back in front of the doorbell ... */
  int64_t disabled;       /* ... and 1 once nothing was left behind it: the handle is back on copy-first */
  double fraction;        /* the share copied behind the doorbell now */
  int64_t timed_steps;    /* while `timing` is on: steps in, and microseconds summed into, the four fields below */
  double copy_before_us, dispatch_us, copy_after_us, wait_us;   /* header + rows in front of the doorbell; packet + doorbell; rows behind it; wait */
} ac_late_stats_t;
/* Self-check: when more than AC_LATE_WINDOW_MAX_RETRY_STEPS of AC_LATE_WINDOW consecutive late steps had a wave ask again, the copy does
 * not fit under the launch on this host: `fraction` drops by a quarter, and at 0 the handle goes back to copy-first (the plain kernel),
 * until ac_late_config sets `fraction` again.
 * fraction in 0 .. 1, budget in tries, delay_us: a pause between doorbell and copy (tests: nothing else makes the kernel retry), timing 0 / 1;
 * a negative value leaves that parameter as it is. */
int ac_late_config(ac_env_t* h, double fraction, int32_t budget, int32_t delay_us, int32_t timing);
int ac_late_stats(ac_env_t* h, ac_late_stats_t* out);

/* Device-resident variant of the same step: d_actions is a DEVICE pointer (or NULL to use the
 * handle's own action buffer); results stay in the handle's device buffers; asynchronous on the handle's stream. */
int ac_step_async_device(ac_env_t* h, const float* d_actions);
int ac_device_buffers(ac_env_t* h, float** d_actions, float** d_obs, float** d_rewards, uint8_t** d_dones, int32_t** d_info);
void* ac_stream(ac_env_t* h);   /* hipStream_t the kernels are launched on (created non-blocking: NOT ordered against other streams) */
/* How the handle's host steps (ac_step_host_async / ac_step_host) are dispatched: "aql" (one AQL packet on a queue the handle owns, kernargs
 * written once per host set; the default after the first host step), "pending" (before the first host step, which goes through HIP and
 * sets the queue up), "AIRCOMBAT_DISPATCH=hip" (the environment variable, read by ac_create, pins the HIP runtime's launch), or
 * "fallback: <reason>" (the set-up failed or the queue faulted; host steps go through HIP), or, while a spawn bank is attached
 * (aircombat_spawn.h), "hip: a spawn bank is attached". Host steps inside an ac_timing_begin .. ac_timing_end bracket always go
 * through HIP. The handle owns the returned string. */
const char* ac_dispatch_path(ac_env_t* h);
int ac_sync(ac_env_t* h);
/* Ordering against the caller's streams without a host sync: ac_order_after makes the steps launched from now on wait for the work
 * already queued on `producer_stream` (the policy that wrote the actions); ac_order_before makes `consumer_stream` wait for the
 * steps launched so far (whoever reads obs / rewards / dones next). NULL = the device's default stream. */
int ac_order_after(ac_env_t* h, void* producer_stream);
int ac_order_before(ac_env_t* h, void* consumer_stream);

/* test/render access, mirrors env.agents[uid] property reads and env.agents[uid].crash() (R/tests/test_jsbsim.py:147-186) */
int ac_get_state(ac_env_t* h, int32_t env, int32_t agent, double* out /* [AC_STATE_LEN] */);
int ac_set_state(ac_env_t* h, int32_t env, int32_t agent, const double* in /* [AC_STATE_LEN] */);
int ac_set_status(ac_env_t* h, int32_t env, int32_t agent, int32_t status);
/* lon deg, lat deg, alt m, roll, pitch, yaw rad, vN, vE, vDown m/s, N, E, U m  (BaseSimulator getters, simulatior.py:47-61) */
int ac_get_entity(ac_env_t* h, int32_t env, int32_t agent, double out[12]);
/* missile k of an agent: status, N,E,U, vN,vE,vU, theta, psi, t, mass, model (0 AIM-9L, 1 AIM-120B, 2 AIM-9M) (MissileSimulator, simulatior.py:393-608) */
int ac_get_missile(ac_env_t* h, int32_t env, int32_t agent, int32_t k, double out[12]);
/* the aircraft (index within the env) that missile k of an agent was launched at (MissileSimulator.target_aircraft); meaningless for a slot never launched */
int ac_get_missile_target(ac_env_t* h, int32_t env, int32_t agent, int32_t k, int32_t* target);

/* Order-independent 64-bit digest of all aircraft states on the device (sum over aircraft of a per-field hash): E envs in the
 * same state give E times the digest of one env (mod 2^64). Test / profiling aid: one read-only pass over the state arrays with
 * the step kernel's access pattern, (4*63 + 4*12 + 8*3) bytes per aircraft; no reference counterpart. */
int ac_state_checksum(ac_env_t* h, uint64_t* out);

/* Number of munitions with status LAUNCHED over the whole handle (len of the live entries of env._tempsims, R/envs/JSBSim/envs/env_base.py:142-143,
 * summed over envs): the bench prices SURVEY 8(d)'s 192 algorithmic bytes per live missile-step with it. 0 for the tasks without munitions. */
int ac_munitions_in_flight(ac_env_t* h, int32_t* count);

/* AC_TASK_HEADING: replaces env.seed(seed) -> gymnasium seeding.np_random(seed) (R/envs/JSBSim/envs/env_base.py:252-258): the four
 * 64-bit words (state_hi, state_lo, inc_hi, inc_lo) of numpy's PCG64 bit generator for every env, [E][4]. The reference seeds env i
 * with seed + 1000 i (scripts/train/train_jsbsim.py:33); resets and UnreachHeading then draw exactly numpy's stream on the device. */
int ac_seed_envs(ac_env_t* h, const uint64_t* states);
/* test access: sim_time, target heading deg / altitude ft / speed m/s, next check time, heading_turn_counts, last p, last q */
int ac_get_heading_state(ac_env_t* h, int32_t env, double out[8]);

/* Optional: page-lock a caller-owned host buffer that is handed to ac_step / ac_reset repeatedly, so that the copies run as
 * direct DMA instead of through a staging buffer (the caller still owns the memory; unpin before freeing it). The reference has
 * no counterpart: its workers pickle arrays through pipes (env_wrappers.py:182-229). */
int ac_pin_host_buffer(ac_env_t* h, void* ptr, int64_t bytes);
int ac_unpin_host_buffer(ac_env_t* h, void* ptr);

/* Low-level controller of the hierarchical tasks: replaces BaselineActor() + load_state_dict(baseline_model.pt) of
 * HierarchicalSingleCombatTask.__init__ (R/envs/JSBSim/tasks/singlecombat_task.py:211-219). `weights` = the 137753 float32 of
 * aircombat-selfplay_amd/data/baseline_actor.f32 (layout in tools/export_baseline_actor.py). Must be called once before the first
 * step of a handle created with cfg.hierarchical. */
int ac_load_controller(ac_env_t* h, const float* weights, int64_t n);
/* test access to _inner_rnn_states[agent] (float[128]) and the controller's last output (float[act_low]: 4 control indices (+ bits)) */
int ac_get_controller_state(ac_env_t* h, int32_t env, int32_t agent, float* hidden, float* low_action);
int ac_set_controller_state(ac_env_t* h, int32_t env, int32_t agent, const float* hidden);
/* the form of the handle's controller after AIRCOMBAT_CTL_PRECISION: AC_CTL_FAST or AC_CTL_FP32 (-1 on a null handle) */
int ac_controller_precision(ac_env_t* h);
/* The low-level controller on given inputs, no env handle: n calls of BaselineActor's forward, batched, on the device (the kernel bodies of
 * the env path). x [n][12] in, h [n][128] in/out (GRU state), logits [n][153] out (may be NULL), action [n][4] out (argmax indices); all
 * host memory. precision: AC_CTL_FAST or AC_CTL_FP32; weights as for ac_load_controller. Synchronous. */
int ac_controller_forward(int32_t device_id, int32_t precision, const float* weights, int64_t n_weights,
                          int64_t n, const float* x, float* h, float* logits, int32_t* action);
/* Host-side check of the arithmetic behind the controller's GEMMs (no GPU, no handle): every fp32 weight and activation is taken apart
 * into two fp16 pieces, hi = fp16(x), lo = fp16(x - hi), |x - hi - lo| <= 2^-22 |x|, and the products run on the fp16 matrix path
 * (controller_pieces.hpp). Writes the two pieces of x[0..n) as float32 values (each with at most 11 significant bits). */
int ac_split_f16x2(const float* x, int64_t n, float* hi, float* lo);
/* The same for the AC_CTL_FP32 form (no GPU, no handle): x = b0 + b1 + b2, b0 = bf16(x), b1 = bf16(x - b0), b2 = bf16(x - b0 - b1), each
 * rounded to nearest-even; the products keep the six terms with i + j <= 2 on the bf16 matrix path. |x - b0 - b1 - b2| <= 2^-24 |x|
 * (in fact zero) for 2^-103 <= |x| < 2^128 (1 - 2^-9), the range where, under the build's flush-to-zero, every piece is a normal
 * number and b0 is finite; below 2^-103 the remainder is under 2^-126. Writes the pieces of x[0..n) as float32 values (each with at
 * most 8 significant bits). */
int ac_split_bf16x3(const float* x, int64_t n, float* b0, float* b1, float* b2);
/* Device self-test (needs the GPU, no handle): the closed form the NvN kernels use for MissilePostureReward's agent-by-agent walk over its
 * shared remembered missile (missile_posture_reward.py:18-46) against the round-by-round walk, for every combination of agent states
 * of a 2v2 and a 4v4 env. *mismatches receives the number of combinations that differ (0 = the two agree everywhere). */
int ac_selftest_missile_walk(int32_t device_id, int32_t* mismatches);
/* Test access to the device math primitives (needs the GPU): runs primitive `op` on n rows of arguments in one launch of a kernel that
 * calls the inline functions the step kernels call. in [n][AC_PROBE_IN], out [n][AC_PROBE_OUT], host memory, row-major; arguments are
 * read from the front of a row in the order listed below, results are written from the front of a row and the rest is zero. fp32
 * primitives take (float)in[k] (pass float32-exact values) and their results are widened exactly. The handle supplies the battle-field
 * constants (centre, radii of curvature) that missile_height and neu_height64 read; no env state is read or changed. Synchronous.
 * Refused: a null handle or pointer, an op outside [0, AC_PROBE_NOPS), n <= 0 or n > AC_PROBE_MAX_ROWS. */
enum { AC_PROBE_IN = 6, AC_PROBE_OUT = 12, AC_PROBE_MAX_ROWS = 1 << 22 };
enum {
  AC_PROBE_FX_RCP = 0,        /* (x)                           -> fx::rcp */
  AC_PROBE_FX_RSQRT,          /* (x)                           -> fx::rsqrt */
  AC_PROBE_FX_SQRT,           /* (x)                           -> fx::sqrt */
  AC_PROBE_FX_SQRT_BOTH,      /* (x)                           -> sqrt, 1 / sqrt */
  AC_PROBE_FX_SINCOS,         /* (x)                           -> sin, cos */
  AC_PROBE_ATAN2_FAST,        /* (y, x)                        -> f16::atan2_fast */
  AC_PROBE_ACOS_FAST,         /* (x)                           -> acos_fast */
  AC_PROBE_POW_POS,           /* (x, y)                        -> f16::pow_pos */
  AC_PROBE_TANH_FAST,         /* (x)                           -> tanh_fast */
  AC_PROBE_ATANH_FAST,        /* (x)                           -> atanh_fast */
  AC_PROBE_SIGMOID_F,         /* (x)                           -> ctl::sigmoid_f */
  AC_PROBE_TANH_F,            /* (x)                           -> ctl::tanh_f */
  AC_PROBE_ATMOSPHERE,        /* (h_ft)                        -> T [R], P [psf], rho [slug/ft3], a [ft/s] */
  AC_PROBE_PITOT,             /* (mach, p)                     -> f16::pitot_impact_pressure */
  AC_PROBE_VCAS,              /* (qc)                          -> f16::vcas_from_impact_pressure [ft/s] */
  AC_PROBE_IN_RANGE_DEG,      /* (a)                           -> in_range_deg_f */
  AC_PROBE_IN_RANGE_RAD,      /* (a)                           -> ctl::in_range_rad_f */
  AC_PROBE_SLEW,              /* (out, in, lo, hi, rate)       -> f16::slew */
  AC_PROBE_TEF_KINEMATIC,     /* (out, in)                     -> f16::tef_kinematic */
  AC_PROBE_SEEK,              /* (v, target, accel, decel, dt) -> f16::seek */
  AC_PROBE_POSTURE_FN,        /* (AO, TA, R km)                -> posture_fn */
  AC_PROBE_MISSILE_HEIGHT_F,  /* (n, e, u) [m]                 -> missile_height, fp32 form */
  AC_PROBE_MISSILE_HEIGHT_D,  /* (n, e, u) [m]                 -> missile_height, fp64 form */
  AC_PROBE_NEU_HEIGHT64,      /* (n, e, u) [m]                 -> neu_height64 */
  AC_PROBE_LOCATE,            /* (rx, ry, rz [ft, ECI], ticks) -> h_sl_ft, n_eci[3], e_eci[3], d_eci[3]  (f16::locate) */
  AC_PROBE_LOCATE_FAST,       /* the same from f16::locate_fast (ticks is not read) */
  AC_PROBE_NOPS
};
int ac_probe_math(ac_env_t* h, int32_t op, int64_t n, const double* in, double* out);
/* Test access to the device missile integrators (needs the GPU): one lane per row runs `ticks` consecutive calls of the step kernels' own
 * missile_run -- form AC_PROBE_MSL_FP32 the MslT<float> template of the 1v1 missile tasks, AC_PROBE_MSL_FP64 the MslD overload of the
 * scenario tasks -- with the AIM-9L or the AIM-120B parameter set and the handle's battle-field constants. The step kernels fly fp32 +
 * AIM-9L, fp64 + AIM-120B and fp64 + AIM-9L; fp32 + AIM-120B is refused. Host memory, row-major doubles:
 *   launch [n][AC_PROBE_MSL_IN]          px py pz [m NEU], vx vy vz [m/s], theta, psi, t, m, dtheta, dphi, dprev (inf at launch), recede,
 *                                        status (0 launched), one unused
 *   target [ticks][n][AC_PROBE_MSL_TGT]  position [m NEU], the velocity record as the target's pose holds it, alive (non-zero)
 *   out    [ticks][n][AC_PROBE_MSL_OUT]  status, px py pz, vx vy vz, theta, psi, t, m, dtheta, dphi, dprev, recede, moved
 * after every tick; `moved` is the fp64 overload's return value (1 / 0) and -1 for the fp32 form. As in the step kernels, a row that
 * reports HIT on a live target sees the target dead in its later ticks, and finished missiles keep being run. No env state is read or
 * changed. Synchronous. Refused before any device call: a null handle or pointer, an unknown form or model, n outside
 * [1, AC_PROBE_MSL_MAX_ROWS], ticks outside [1, AC_PROBE_MSL_MAX_TICKS], n * ticks above AC_PROBE_MSL_MAX_CELLS. */
enum { AC_PROBE_MSL_IN = 16, AC_PROBE_MSL_TGT = 7, AC_PROBE_MSL_OUT = 16, AC_PROBE_MSL_MAX_ROWS = 512, AC_PROBE_MSL_MAX_TICKS = 4200,
       AC_PROBE_MSL_MAX_CELLS = 1 << 19 };
enum { AC_PROBE_MSL_FP32 = 0, AC_PROBE_MSL_FP64 = 1 };
enum { AC_PROBE_MSL_AIM9L = 0, AC_PROBE_MSL_AIM120B = 1 };
int ac_probe_missile(ac_env_t* h, int32_t form, int32_t model, int32_t n, int32_t ticks, const double* launch, const double* target, double* out);

/* timing helper for the bench: average device milliseconds per step kernel over the last n ac_step* calls, measured
 * with HIP events on the handle's stream */
int ac_timing_begin(ac_env_t* h);
int ac_timing_end(ac_env_t* h, float* total_ms);
/* one device-resident step (as ac_step_async_device + ac_sync) with HIP events around its two kernels: the low-level controller of the
 * hierarchical tasks (0 for the control-index form) and the step kernel, each in milliseconds. For the bench's per-kernel rooflines. */
int ac_step_timed_device(ac_env_t* h, const float* d_actions, float* controller_ms, float* step_ms);

/* Snapshot, restore and clone of the env state (no reference counterpart: the reference's JSBSim processes end with the run).
 * A snapshot is everything a later step reads that ac_reset does not rebuild from the config: the aircraft record (the 19 groups of
 * ac_get_state's storage and the fp64 position), every munition slot, the scenario tasks' extension words, the HeadingTask targets,
 * clocks and numpy-PCG64 states (ac_seed_envs), the hierarchical tasks' GRU state, last low-level action and scripted-opponent
 * counters, and the last outputs (obs / rewards / dones / info, so a restore hands back the observation of that moment). Layout: a
 * 1024-byte header (magic "ACSN", format, ac_version(), task, E, A, munition slots, obs_dim, act_dim, controller precision, a
 * digest of the config, seed, reset template, controller weights and kernel form, the section table), then the arrays in their
 * device layout, each at a 256-byte boundary. A load refuses a snapshot whose header differs from the handle's; a
 * fresh handle made with the same config and seed accepts it (resume). Every call is ordered on ac_stream(h). */
int ac_snapshot_bytes(ac_env_t* h, int64_t* bytes);                 /* size of one whole-batch snapshot */
int ac_snapshot_header(ac_env_t* h, void* out /* [1024] */);        /* the header a snapshot of this handle carries */
/* whole batch to / from device memory: one copy per array, stream-ordered on ac_stream(h), no host wait on save; a load reads the
 * header first (one host wait on ac_stream(h)). The save has finished only for work ordered after it on ac_stream(h): a reader on
 * any other stream -- a copy to the host, or ac_snapshot_load / ac_snapshot_load_envs on ANOTHER handle, which run on that handle's
 * stream -- must first be ordered after it (ac_order_before(h, stream), ac_sync(h), or an event recorded on ac_stream(h)).
 * A save is refused when the non-finite guard has fired in a step that completed before the call; a step still queued ahead of the
 * save that trips the guard is reported by the next ac_sync / step wait, and the snapshot then holds that state. A whole-batch load
 * clears the guard (a non-finite state loaded back fires it again at the next step). */
int ac_snapshot_save(ac_env_t* h, void* d_dst);
int ac_snapshot_load(ac_env_t* h, const void* d_src);
/* the same layout in host memory (checkpoint files); synchronous */
int ac_snapshot_save_host(ac_env_t* h, void* dst, int64_t bytes);
int ac_snapshot_load_host(ac_env_t* h, const void* src, int64_t bytes);
/* env src[k] -> env dst[k] for k < n, every agent and array of a snapshot (one gather / scatter kernel). src may repeat (one env
 * into many), dst may not, no source may be written by another pair from a different env (chains, swaps: clone in two calls),
 * and every index must be below E: all checked on the host, so the indices (device or host memory)
 * are read after the work already queued on the stream (one host wait), then the kernel runs stream-ordered. The scenario tasks'
 * decoy draws are keyed by the env index, so two clones of one env part ways at their first chaff-against-missile draw. */
int ac_clone_envs(ac_env_t* h, const int32_t* src, const int32_t* dst, int32_t n);
/* restore only envs idx[0..n) from a whole-batch snapshot in device memory (the same kernel as ac_clone_envs); others untouched */
int ac_snapshot_load_envs(ac_env_t* h, const void* d_src, const int32_t* idx, int32_t n);
/* the current observation buffer [E*A][obs_dim] to host memory, after the work queued on the stream */
int ac_get_obs(ac_env_t* h, float* obs);
/* 64-bit digest of every array a snapshot holds (ac_state_checksum covers the aircraft record only); test aid */
int ac_snapshot_checksum(ac_env_t* h, uint64_t* out);

/* ---- the PPO rollout policy on the device (PPOPolicy.get_actions / .act of the reference; DESIGN.md, "The PPO rollout policy"). Actor and, optionally,
 * critic of the recurrent MLP policy (hidden sizes "128 128", GRU 128, ReLU) with MultiDiscrete heads (<= 160 logits) and, optionally,
 * the four BetaShootBernoulli munition heads of Tuple(MultiDiscrete, MultiDiscrete([2, 2, 2, 2])) with use_prior. Everything else is
 * refused at creation (ac_last_error names what). */
typedef struct ac_policy_s ac_policy_t;
typedef struct {
  int32_t obs_dim;                      /* 1 .. 32 */
  int32_t n_cat;                        /* MultiDiscrete heads, 1 .. 8 */
  int32_t nvec[8];
  int32_t n_shoot;                      /* 0, or 4: MultiDiscrete([2, 2, 2, 2]) munition heads (need use_prior and obs_dim >= 14) */
  int32_t single_shoot;                 /* Tuple(MultiDiscrete, Discrete(2)): refused */
  int32_t hidden_size[2], act_hidden_size[2];   /* 128, 128 */
  int32_t recurrent_hidden_size, recurrent_hidden_layers;   /* 128, 1 */
  int32_t activation_id;                /* 1 (ReLU) */
  int32_t use_recurrent_policy, use_feature_normalization, use_prior;
  int32_t precision;                    /* AC_CTL_FAST (two fp16 pieces per product) or AC_CTL_FP32 (three bf16 pieces) */
  int32_t has_critic;
} ac_policy_config_t;
/* rows of one call: n rows, or (na > 0) the agent range [a0, a0 + na) of an [E, A, .] obs / action layout with n = E * na; the
 * action rows are act_stride floats apart. The states, masks, log-probs and values are always compact [n, .]. */
typedef struct {
  int64_t n;
  int32_t na, A, a0, act_stride;
} ac_policy_rows_t;
/* lengths of the fp32 source blobs (order: policy_host.hpp / policy.py); no device needed */
int ac_policy_blob_floats(const ac_policy_config_t* cfg, int64_t* actor_floats, int64_t* critic_floats);
int ac_policy_create(int32_t device_id, const ac_policy_config_t* cfg, ac_policy_t** out);
int ac_policy_destroy(ac_policy_t* h);
/* host blobs (critic may be NULL); refused, leaving the previous weights in place, when a weight is not finite or (fast form) |w| >= 65504 */
int ac_policy_load(ac_policy_t* h, const float* actor, int64_t n_actor, const float* critic, int64_t n_critic);
/* device blobs, packed on the device ordered on `stream` (no host round trip); a refused load leaves the previous weights in place and is
 * reported by ac_policy_load_refused, which waits for the stream */
int ac_policy_load_device(ac_policy_t* h, void* stream, const float* d_actor, int64_t n_actor, const float* d_critic, int64_t n_critic);
int ac_policy_load_refused(ac_policy_t* h, void* stream, int32_t* actor_refused, int32_t* critic_refused);
/* the packed weights of the actor (0) / critic (1) on the device (test aid) */
int ac_policy_packed(ac_policy_t* h, int32_t net, void** d_ptr, int64_t* floats);
/* one launch on `stream`: obs, masks [n], GRU states [n, 128] in and out (in place allowed), actions as float32 in the reference's
 * concatenated head order, log-probs [n] summed over the heads, values [n]. The critic's three pointers all NULL = actor only (.act).
 * deterministic: the mode; otherwise inverse-CDF draws keyed by (seed, counter, row, head) -- ac_policy_draw_host. */
int ac_policy_get_actions(ac_policy_t* h, void* stream, const ac_policy_rows_t* rows, const float* d_obs, const float* d_rnn_actor,
                          const float* d_rnn_critic, const float* d_masks, int32_t deterministic, uint64_t seed, uint64_t counter,
                          float* d_values, float* d_actions, float* d_logp, float* d_rnn_actor_out, float* d_rnn_critic_out);
/* ---- the MAPPO rollout policy on the device (algorithms/mappo/ppo_policy.py of the reference; DESIGN.md, "The PPO rollout policy"): the
 * same actor and heads, input widths up to 640 for both networks, and a centralised critic whose input is cent_obs_dim wide. Its blobs
 * are the PPO ones with the critic's feature_norm / base.mlp.fc.0.weight [128, cent_obs_dim]. Loads, ac_policy_packed and
 * ac_policy_destroy take both kinds of handle. */
typedef struct {
  ac_policy_config_t base;              /* base.obs_dim: 1 .. 640 */
  int32_t cent_obs_dim;                 /* 1 .. 640 (the critic's input width; checked when base.has_critic) */
} ac_policy_mappo_config_t;
#define AC_CENT_EXPLICIT 0              /* critic row r reads d_cent_obs + r * cent_obs_dim */
#define AC_CENT_ENV_SHARE 1             /* critic row r of an agent-range call reads env r / na's whole obs block (cent_obs_dim = A * obs_dim) */
int ac_policy_mappo_blob_floats(const ac_policy_mappo_config_t* cfg, int64_t* actor_floats, int64_t* critic_floats);
int ac_policy_mappo_create(int32_t device_id, const ac_policy_mappo_config_t* cfg, ac_policy_t** out);
/* ac_policy_get_actions for a MAPPO handle: the actor reads d_obs (rows as there), the critic reads cent_mode's input (d_cent_obs is
 * unused with AC_CENT_ENV_SHARE). The critic's three pointers all NULL = actor only. */
int ac_policy_get_actions_mappo(ac_policy_t* h, void* stream, const ac_policy_rows_t* rows, const float* d_obs, const float* d_cent_obs,
                                int32_t cent_mode, const float* d_rnn_actor, const float* d_rnn_critic, const float* d_masks,
                                int32_t deterministic, uint64_t seed, uint64_t counter, float* d_values, float* d_actions, float* d_logp,
                                float* d_rnn_actor_out, float* d_rnn_critic_out);
/* the critic alone (get_values; values [n] and its new state): d_in is the obs rows of a PPO handle (AC_CENT_EXPLICIT only), or
 * cent_mode's input of a MAPPO handle (the obs buffer with AC_CENT_ENV_SHARE). Bit-identical to the values of a get_actions call. */
int ac_policy_get_values(ac_policy_t* h, void* stream, const ac_policy_rows_t* rows, const float* d_in, int32_t cent_mode,
                         const float* d_rnn_critic, const float* d_masks, float* d_values, float* d_rnn_critic_out);
/* the draws of rows row0 .. row0 + nrows - 1, one head, on the host: uniform on [0, 1) in steps of 2^-24 */
int ac_policy_draw_host(uint64_t seed, uint64_t counter, int64_t row0, int64_t nrows, int32_t head, float* out);

/* ---- a pool of actors on the device (the self-play opponents; DESIGN.md, "The opponent pool"): `capacity` actors in one device array,
 * each packed as a DevicePolicy (AC_POOL_PPO, obs_dim <= 32) or DeviceMAPPOPolicy (AC_POOL_MAPPO, obs_dim <= 640) packs its actor; one
 * precision and one form for the whole pool. cfg is the policy's configuration (a MAPPO configuration's base); has_critic is ignored.
 * An assignment maps each env to a member, and one launch acts for every assigned row with its member's weights. */
typedef struct ac_policy_pool_s ac_policy_pool_t;
#define AC_POOL_PPO 0
#define AC_POOL_MAPPO 1
/* no device needed: the refusals of ac_policy_pool_create, and the source / packed float count of one member */
int ac_policy_pool_member_floats(const ac_policy_config_t* cfg, int32_t form, int32_t capacity, int64_t* src_floats, int64_t* packed_floats);
/* 0 when a policy of (cfg, form) may be copied into a pool of (pool_cfg, pool_form); else -1, ac_last_error naming what differs */
int ac_policy_pool_compatible(const ac_policy_config_t* pool_cfg, int32_t pool_form, const ac_policy_config_t* cfg, int32_t form);
int ac_policy_pool_create(int32_t device_id, const ac_policy_config_t* cfg, int32_t form, int32_t capacity, ac_policy_pool_t** out);
int ac_policy_pool_destroy(ac_policy_pool_t* p);
/* member loads, refused as ac_policy_load / ac_policy_load_device refuse, keeping the member's previous weights. A member is loaded
 * once a load of it has passed; an assignment reads that state when it is planned (assign after loading). */
int ac_policy_pool_load(ac_policy_pool_t* p, int32_t member, const float* actor, int64_t n);
int ac_policy_pool_load_device(ac_policy_pool_t* p, void* stream, int32_t member, const float* d_actor, int64_t n);
int ac_policy_pool_load_refused(ac_policy_pool_t* p, void* stream, int32_t* refused);
/* a policy's packed actor, device to device on `stream`; refused when the form, precision or configuration differ */
int ac_policy_pool_copy_from(ac_policy_pool_t* p, void* stream, int32_t member, ac_policy_t* policy);
int ac_policy_pool_packed(ac_policy_pool_t* p, int32_t member, void** d_ptr, int64_t* floats);
/* the assignment: d_members [E] int32, member of each env (-1: its rows are not acted for), for calls of E * na rows (na rows per env).
 * Copied and planned on `stream` (a stable sort of the rows by member, tiles of <= 32 rows of one member); the plan is kept for every
 * later ac_policy_pool_act, and rebuilt by a call whose na differs. */
int ac_policy_pool_assign(ac_policy_pool_t* p, void* stream, const int32_t* d_members, int64_t E, int32_t na);
/* the sided assignment (the league, aircombat_league.h): members2 is [E][2]: env e's agents [0, A/2) act with members2[e][0], agents
 * [A/2, A) with members2[e][1] (-1: that side is not acted for). A even, >= 2. Planned on `stream` like ac_policy_pool_assign, as that
 * plan over the 2 E half-envs of A / 2 rows: half-env 2 e + side, row k is call row e * A + side * A / 2 + k. While it is in force
 * ac_policy_pool_act takes exactly the whole-range call (rows->n = E * A, rows->na = rows->A = A, rows->a0 = 0), one launch in which row
 * e * A + a acts with its side's member and the row's own keyed draws; any other geometry is refused, naming the sided plan, and the
 * plan is never rebuilt by a call. ac_policy_pool_check reports the first bad env (not half-env); ac_policy_pool_max_tiles and
 * ac_policy_pool_plan_host describe the plan with (2 E, A / 2). A later ac_policy_pool_assign returns the pool to the per-env form. */
int ac_policy_pool_assign_sides(ac_policy_pool_t* p, void* stream, const int32_t* d_members2, int64_t E, int32_t A);
/* waits for `stream`: the first env whose member is out of range or not loaded (-1: none; such envs are not acted for) and the plan's
 * tile count, which later act calls then use as their grid */
int ac_policy_pool_check(ac_policy_pool_t* p, void* stream, int32_t* bad_env, int32_t* ntiles);
/* the plan on the host (the device's code): order [E * na] call rows, tiles [3 * ac_policy_pool_max_tiles] {member, p0, p1} = rows
 * order[p0 .. p1 - 1]; loaded [capacity] or NULL (all loaded) */
int ac_policy_pool_plan_host(const int32_t* members, int64_t E, int32_t na, int32_t capacity, const int32_t* loaded, int32_t* order,
                             int32_t* tiles, int32_t* ntiles, int32_t* bad_env);
int ac_policy_pool_max_tiles(int64_t E, int32_t na, int32_t capacity, int64_t* out);
/* 1 (the default): deal a member's tiles to workgroups that share blockIdx.x % 8 (one XCD's L2); 0: member-major order. Speed only. */
int ac_policy_pool_set_tile_order(ac_policy_pool_t* p, int32_t xcd);
/* one launch on `stream`: ac_policy_get_actions' actor part (rows, obs, masks, states, actions, log-probs as there; rows->n = E * na of
 * the assignment) with each row's member; draws keyed by (seed, counter, call row, head) like ac_policy_get_actions. Unassigned rows'
 * actions, states and log-probs are left untouched. */
int ac_policy_pool_act(ac_policy_pool_t* p, void* stream, const ac_policy_rows_t* rows, const float* d_obs, const float* d_h_in,
                       const float* d_masks, int32_t deterministic, uint64_t seed, uint64_t counter, float* d_actions, float* d_logp,
                       float* d_h_out);

/* ---- the PPO update's GRU on the device ("The training GRU"): the recurrence of the reference's one-layer GRULayer,
 * input and hidden 128, torch's gate order (r, z, n), over N chunks of T steps, rows T-major ([T * N, .], row t * N + j = step t of
 * chunk j). One launch per call on `stream`, returning at once; every pointer is a device pointer of float32. Each step starts from
 * h_in = h_{t-1} * masks[t * N + j]. Refused: a NULL required pointer, N or T < 1, N * T beyond the kernels' 32-bit row index. */
/* forward: d_gi [T*N, 384] = x W_ihᵀ + b_ih, d_hxs [N, 128], d_masks [T*N], d_w_hh [384, 128], d_b_hh [384] -> d_y [T*N, 128] (the
 * outputs before the LayerNorm), d_h_T [N, 128]; d_saved [T*N, 512] (r, z, n, W_hn h_in + b_hn) for a backward, or NULL */
int ac_gru_seq_forward(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_gi, const float* d_hxs, const float* d_masks,
                       const float* d_w_hh, const float* d_b_hh, float* d_y, float* d_h_T, float* d_saved);
/* backward: upstream d_dy [T*N, 128] and d_dh_T [N, 128] (either NULL = zero), the forward's d_saved and d_y, its d_hxs, d_masks and
 * d_w_hh -> d_dgi, d_dgh [T*N, 384] (gradients of the input-side and hidden-side gate pre-activations; they differ in the n block
 * only) and d_dhxs [N, 128] (NULL: not computed) */
int ac_gru_seq_backward(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_dy, const float* d_dh_T, const float* d_saved,
                        const float* d_y, const float* d_hxs, const float* d_masks, const float* d_w_hh, float* d_dgi, float* d_dgh,
                        float* d_dhxs);
/* How the two recurrence kernels multiply by W_hh ("The training GRU"). AC_PRODUCTS_FP32: the fp32 matrix instruction,
 * what the calls above do. AC_PRODUCTS_BF16X3: every value as three bf16 pieces (their sum is the value exactly) and the six piece
 * products of order <= 2 on the bf16 matrix instruction, accumulated in fp32: each product good to about 2^-23 of itself. W_hh is still
 * the caller's fp32 tensor, read and split at every call. */
#define AC_PRODUCTS_FP32 0
#define AC_PRODUCTS_BF16X3 1
/* the two calls above with `products`; AC_PRODUCTS_FP32 launches exactly what they launch. Also refused, before any launch: an
 * unknown `products`. */
int ac_gru_seq_forward_p(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_gi, const float* d_hxs, const float* d_masks,
                         const float* d_w_hh, const float* d_b_hh, float* d_y, float* d_h_T, float* d_saved, int32_t products);
int ac_gru_seq_backward_p(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_dy, const float* d_dh_T, const float* d_saved,
                          const float* d_y, const float* d_hxs, const float* d_masks, const float* d_w_hh, float* d_dgi, float* d_dgh,
                          float* d_dhxs, int32_t products);

/* ---- the whole GRU layer of the PPO update on the device ("The whole GRU layer"): the reference's GRULayer, nn.GRU
 * 128 -> 128 of one layer then nn.LayerNorm(128), as one call per direction: the input product, the recurrence above, the LayerNorm and,
 * backward, the weight, bias and input gradients. Shapes, row order and masks as above; every pointer is a device pointer of float32;
 * the calls launch on `stream` and return at once. Refused before any launch: a NULL required pointer, N or T < 1, N * T beyond the
 * kernels' 32-bit row index, and a [., 128] array, the workspace or the stats that is not 16-byte aligned. */
/* floats of d_workspace for this shape (the gate pre-activations or their gradients, and one set of parameter-gradient partial sums
 * per workgroup); the forward uses the first T * N * 384 of them only; -1: refused */
int64_t ac_gru_layer_workspace_floats(int32_t N, int32_t T);
/* forward, three launches: d_x [T*N, 128], d_hxs [N, 128], d_masks [T*N], d_w_ih, d_w_hh [384, 128], d_b_ih, d_b_hh [384], d_gamma,
 * d_beta [128] and the LayerNorm's eps -> d_out [T*N, 128], d_h_T [N, 128], and d_y [T*N, 128] (the recurrence's outputs before the
 * LayerNorm). For a backward also d_saved [T*N, 512] and d_stats [T*N, 2] (each row's mean and 1 / sqrt(var + eps)); both NULL: the
 * inference form, nothing kept. */
int ac_gru_layer_forward(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_x, const float* d_hxs, const float* d_masks,
                         const float* d_w_ih, const float* d_w_hh, const float* d_b_ih, const float* d_b_hh, const float* d_gamma,
                         const float* d_beta, float eps, float* d_workspace, float* d_out, float* d_h_T, float* d_y, float* d_saved,
                         float* d_stats);
/* backward: upstream d_g_out [T*N, 128] (of d_out) and d_g_h_T [N, 128] (either NULL = zero), the forward's inputs and its d_y, d_saved,
 * d_stats -> d_dx [T*N, 128] (NULL: not computed), d_dhxs [N, 128] (NULL: not computed), d_dw_ih, d_dw_hh [384, 128], d_db_ih, d_db_hh
 * [384], d_dgamma, d_dbeta [128]. Results are bit-identical from run to run (no atomics). */
int ac_gru_layer_backward(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_g_out, const float* d_g_h_T, const float* d_x,
                          const float* d_hxs, const float* d_masks, const float* d_w_ih, const float* d_w_hh, const float* d_gamma,
                          const float* d_y, const float* d_saved, const float* d_stats, float* d_workspace, float* d_dx, float* d_dhxs,
                          float* d_dw_ih, float* d_dw_hh, float* d_db_ih, float* d_db_hh, float* d_dgamma, float* d_dbeta);
/* the two calls above with `products` (AC_PRODUCTS_FP32 / AC_PRODUCTS_BF16X3, above): it selects the recurrence kernel alone; the
 * input product, the LayerNorm, the weight and input gradients and the workspace are the same. AC_PRODUCTS_FP32 launches exactly what
 * the calls above launch; an unknown `products` is refused before any launch. */
int ac_gru_layer_forward_p(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_x, const float* d_hxs, const float* d_masks,
                           const float* d_w_ih, const float* d_w_hh, const float* d_b_ih, const float* d_b_hh, const float* d_gamma,
                           const float* d_beta, float eps, float* d_workspace, float* d_out, float* d_h_T, float* d_y, float* d_saved,
                           float* d_stats, int32_t products);
int ac_gru_layer_backward_p(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_g_out, const float* d_g_h_T,
                            const float* d_x, const float* d_hxs, const float* d_masks, const float* d_w_ih, const float* d_w_hh,
                            const float* d_gamma, const float* d_y, const float* d_saved, const float* d_stats, float* d_workspace,
                            float* d_dx, float* d_dhxs, float* d_dw_ih, float* d_dw_hh, float* d_db_ih, float* d_db_hh, float* d_dgamma,
                            float* d_dbeta, int32_t products);
/* the two `_p` calls with `dense_products` (AC_PRODUCTS_FP32 / AC_PRODUCTS_BF16X3) as well: it selects, independently of `products`,
 * how the layer's three dense products are formed -- gi = x W_ihᵀ, dx = dgi W_ih and the weight gradients dW_ih, dW_hh. AC_PRODUCTS_BF16X3:
 * every value as three bf16 pieces and the six piece products of order <= 2 on the bf16 matrix instruction, accumulated in fp32; W_ih
 * is still the caller's fp32 tensor, read and split at every call; the bias gradients stay fp32 sums. Arguments, outputs, the
 * workspace and its size are the same; results are bit-identical from run to run. AC_PRODUCTS_FP32 launches exactly what the `_p`
 * calls launch. Refused as there, and an unknown `dense_products` before any launch. */
int ac_gru_layer_forward_pd(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_x, const float* d_hxs, const float* d_masks,
                            const float* d_w_ih, const float* d_w_hh, const float* d_b_ih, const float* d_b_hh, const float* d_gamma,
                            const float* d_beta, float eps, float* d_workspace, float* d_out, float* d_h_T, float* d_y, float* d_saved,
                            float* d_stats, int32_t products, int32_t dense_products);
int ac_gru_layer_backward_pd(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_g_out, const float* d_g_h_T,
                             const float* d_x, const float* d_hxs, const float* d_masks, const float* d_w_ih, const float* d_w_hh,
                             const float* d_gamma, const float* d_y, const float* d_saved, const float* d_stats, float* d_workspace,
                             float* d_dx, float* d_dhxs, float* d_dw_ih, float* d_dw_hh, float* d_db_ih, float* d_db_hh, float* d_dgamma,
                             float* d_dbeta, int32_t products, int32_t dense_products);
/* the kernels' constants, for tests that size themselves: 0 rows per tile (every kernel), then the workgroups at most of 1 the input
 * product, 2 the LayerNorm forward, 3 the LayerNorm backward, 4 the weight gradients (per gradient), 5 the input gradient; -1 otherwise */
int32_t ac_gru_layer_constant(int32_t which);

/* ---- the PPO update's MLP layers on the device ("The training MLP blocks"): one block of the reference's MLPLayer,
 * y = LayerNorm_128(relu(x Wᵀ + b)) * gamma + beta, x [M, K], W [128, K] (nn.Linear's layout), b, gamma, beta [128], biased variance.
 * Every pointer is a device pointer of float32; the calls launch on `stream` and return at once. Refused: a NULL required pointer,
 * M < 1, K outside 1 .. 256, M * 128 beyond the kernels' 32-bit index. */
/* floats of ac_mlp_block_backward's d_workspace for this shape (one set of parameter-gradient partial sums per workgroup); -1: refused */
int64_t ac_mlp_block_workspace_floats(int32_t M, int32_t K);
/* forward, one launch: -> d_y [M, 128]; d_stats [M, 2] (mean and 1 / sqrt(var + eps) of relu(z) per row) for a backward, or NULL */
int ac_mlp_block_forward(int32_t device_id, void* stream, int32_t M, int32_t K, float eps, const float* d_x, const float* d_w, const float* d_b,
                         const float* d_gamma, const float* d_beta, float* d_y, float* d_stats);
/* backward, two launches (the block's kernel, then the fixed-order sum of its partials): upstream d_dy [M, 128], the forward's d_x and
 * d_stats -> d_dx [M, K] (NULL: not computed), d_dw [128, K], d_db, d_dgamma, d_dbeta [128]. z is recomputed from x, W, b; eps is
 * already in d_stats. Results are bit-identical from run to run (no atomics). */
int ac_mlp_block_backward(int32_t device_id, void* stream, int32_t M, int32_t K, const float* d_dy, const float* d_x, const float* d_w,
                          const float* d_b, const float* d_gamma, const float* d_stats, float* d_workspace, float* d_dx, float* d_dw,
                          float* d_db, float* d_dgamma, float* d_dbeta);
/* the two calls above with `products` (AC_PRODUCTS_FP32 / AC_PRODUCTS_BF16X3, above). AC_PRODUCTS_BF16X3 forms the block's three
 * products -- z = x Wᵀ (in the forward and again in the backward's recomputation, by one shared function, so the ReLU mask is the
 * same bit for bit), dx = dz W and dW = dzᵀ x -- from three bf16 pieces per value and the six piece products of order <= 2 on the bf16
 * matrix instruction, accumulated in fp32; W is still the caller's fp32 tensor, read and split at every call; the bias, the ReLU, the
 * LayerNorm and db, dgamma, dbeta stay fp32. Arguments, outputs, the workspace and its size are the same; results are bit-identical
 * from run to run. A forward and its backward must be given the same `products`. Where the padded K has no split kernel
 * (ac_mlp_block_constant(3)) AC_PRODUCTS_BF16X3 launches the fp32 kernels; AC_PRODUCTS_FP32 launches exactly what the calls above
 * launch. Refused as there, and an unknown `products` before any launch. */
int ac_mlp_block_forward_p(int32_t device_id, void* stream, int32_t M, int32_t K, float eps, const float* d_x, const float* d_w,
                           const float* d_b, const float* d_gamma, const float* d_beta, float* d_y, float* d_stats, int32_t products);
int ac_mlp_block_backward_p(int32_t device_id, void* stream, int32_t M, int32_t K, const float* d_dy, const float* d_x, const float* d_w,
                            const float* d_b, const float* d_gamma, const float* d_stats, float* d_workspace, float* d_dx, float* d_dw,
                            float* d_db, float* d_dgamma, float* d_dbeta, int32_t products);
/* the kernels' constants, for tests that size themselves: 0 rows per tile, 1 the forward's workgroups at most, 2 the backward's (also
 * its partial sets at most), 3 a bitmask of the padded K (32, 64, 128, 256; K <= 32 pads to 32 in the split form) for which
 * AC_PRODUCTS_BF16X3 runs a split kernel; -1 otherwise */
int32_t ac_mlp_block_constant(int32_t which);

/* ---- the PPO update's action heads on the device ("The training action heads"): ACTLayer.evaluate_actions of the reference
 * for n_cat Categorical heads (logits_net: W_h [nvec[h], 128], b_h [nvec[h]]) and, with n_shoot_cols 1 or 4, ONE BetaShootBernoulli head
 * (net: W [2, 128], b [2]; the last module of action_outs) whose probability is applied to all the shoot columns. d_w / d_b (and d_dw /
 * d_db) are HOST arrays of n_cat (+ 1 with shoot columns) device pointers, the shoot head last. x [M, 128]; actions [M, n_cat +
 * n_shoot_cols] float32 as the buffer stores them; alpha0, beta0 [M] with shoot columns only. Every device pointer is float32; the calls
 * launch on `stream` and return at once. Refused, each with its own message: a NULL required pointer, M < 1, n_cat outside 1 .. 8, a
 * head size below 2, more than 160 categorical logits, n_shoot_cols not 0, 1 or 4, shoot columns without alpha0 / beta0, M * 128 beyond
 * the kernels' 32-bit index. An action that is not an integer in 0 .. nvec[h] - 1 makes that row's logp NaN and touches nothing else: the
 * taken logit is picked by compare-and-select, never by indexing; in the backward such an action matches no logit. */
typedef struct {
  int32_t n_cat;                        /* Categorical heads, 1 .. 8 */
  int32_t nvec[8];                      /* their sizes, each >= 2, at most 160 in all */
  int32_t n_shoot_cols;                 /* 0, 1 (MultiDiscrete + Discrete(2)) or 4 (MultiDiscrete + MultiDiscrete([2, 2, 2, 2])) */
} ac_act_heads_t;
/* floats of ac_act_eval_backward's d_workspace: one set of 129 * (sum nvec + 2 [shoot]) partial sums per workgroup, one workgroup per
 * 32-row tile up to 256; -1: refused */
int64_t ac_act_eval_workspace_floats(const ac_act_heads_t* heads, int32_t M);
/* forward, one launch: -> d_logp [M] (sum over heads of the taken action's log-probability; the shoot head's summed over its columns)
 * and d_ent [M] (sum over heads of the entropy, unscaled; the shoot head's counted once) */
int ac_act_eval_forward(int32_t device_id, void* stream, const ac_act_heads_t* heads, int32_t M, const float* d_x, const float* const* d_w,
                        const float* const* d_b, const float* d_actions, const float* d_alpha0, const float* d_beta0, float* d_logp,
                        float* d_ent);
/* backward, two launches (the heads' kernel, then the fixed-order sum of its partials): upstream d_dlogp, d_dent [M] (NULL: zero) ->
 * d_dx [M, 128] (NULL: not computed), d_dw[h] [nvec[h], 128] and d_db[h] [nvec[h]] per head. The logits are recomputed from x. Results
 * are bit-identical from run to run (no atomics). */
int ac_act_eval_backward(int32_t device_id, void* stream, const ac_act_heads_t* heads, int32_t M, const float* d_dlogp, const float* d_dent,
                         const float* d_x, const float* const* d_w, const float* const* d_b, const float* d_actions, const float* d_alpha0,
                         const float* d_beta0, float* d_workspace, float* d_dx, float* const* d_dw, float* const* d_db);

/* ---- the rest of the PPO update on the device ("The loss, the clip and Adam"): the reference's loss
 * (algorithms/ppo/ppo_trainer.py:44-61), torch's clip_grad_norm_ per optimiser param group and torch's single-tensor Adam. Every device
 * pointer is float32; the calls launch on `stream` and return at once. No floating-point atomics: results are bit-identical from run to
 * run. Refused, each with its own message and before any launch: a NULL required pointer, M or n_ent < 1 or beyond the kernels' 32-bit
 * index; for the optimiser, no entries or more than 512, n_groups outside 1 .. 8, an entry with a NULL or misaligned pointer, numel < 1,
 * a group outside 0 .. n_groups - 1, or a first_chunk that ac_optim_workspace_floats did not lay out. */
/* d_stats [AC_PPO_NSTAT]: */
#define AC_PPO_STAT_LOSS 0
#define AC_PPO_STAT_POLICY_LOSS 1
#define AC_PPO_STAT_VALUE_LOSS 2
#define AC_PPO_STAT_ENTROPY_LOSS 3   /* -mean(ent) */
#define AC_PPO_STAT_RATIO_MEAN 4
#define AC_PPO_STAT_DENOMINATOR 5    /* M, or the sum of d_active */
#define AC_PPO_NSTAT 8
/* floats of ac_ppo_loss_forward's d_workspace (five sums per workgroup); -1: refused */
int64_t ac_ppo_loss_workspace_floats(int32_t M, int32_t n_ent);
/* forward, two launches. Per row (each array [M]; d_old_logp [M, old_cols], 1 .. 64 columns against which logp broadcasts as in the
 * reference, whose MAPPO buffer keeps one old log-probability per action column: the row's term is the sum over the columns and
 * ratio.mean() runs over all M old_cols ratios): ratio = exp(logp - old_logp); min(ratio adv, clamp(ratio, 1 - c, 1 + c) adv);
 * 0.5 max((v - R)^2, (vp + clamp(v - vp, -c, c) - R)^2), or 0.5 (R - v)^2 with use_clipped_value_loss 0. Both means are plain means, or
 * with d_active [M] (NULL: none) sum(. active) / sum(active); the entropy term is -mean(d_ent [n_ent]) always. loss = policy +
 * value_loss_coef value + entropy_coef entropy_loss. -> d_stats, d_loss [1] (NULL: not written; the loss again, for a caller that
 * keeps it in a tensor of its own), and d_dlogp, d_dvalues [M]: dloss/dlogp and dloss/dvalues for a unit
 * upstream gradient (torch's conventions: clamp passes the gradient on its closed interval, min / max split a tie evenly);
 * dloss/dent is the constant -entropy_coef / n_ent. */
int ac_ppo_loss_forward(int32_t device_id, void* stream, int32_t M, int32_t n_ent, int32_t old_cols, const float* d_logp,
                        const float* d_old_logp, const float* d_adv, const float* d_values, const float* d_value_preds, const float* d_returns, const float* d_active,
                        const float* d_ent, double clip_param, double value_loss_coef, double entropy_coef, int32_t use_clipped_value_loss,
                        float* d_workspace, float* d_stats, float* d_loss, float* d_dlogp, float* d_dvalues);
/* backward, one launch: d_upstream [1] (a device scalar) times the forward's d_dlogp, d_dvalues and the entropy's constant ->
 * d_g_logp, d_g_values [M], d_g_ent [n_ent] (each may be NULL: not computed) */
int ac_ppo_loss_backward(int32_t device_id, void* stream, int32_t M, int32_t n_ent, const float* d_upstream, const float* d_dlogp,
                         const float* d_dvalues, double entropy_coef, float* d_g_logp, float* d_g_values, float* d_g_ent);

/* One entry of the optimiser's tensor table per parameter that has a gradient: any 4-byte-aligned device pointers (vector loads are
 * used where all four are 16-byte aligned), numel >= 1. The work is cut into chunks of 2048 elements of one tensor, one workgroup each,
 * so the launch count does not depend on the number of tensors. The same bytes serve as the host table (checked, laid out) and as its
 * device copy (read by the kernels): fill it in pinned memory, call ac_optim_workspace_floats, then copy it to the device on `stream`. */
typedef struct {
  float* p;                  /* the parameter, */
  float* g;                  /* its gradient (rewritten with the clipped gradient), */
  float* m;                  /* exp_avg and */
  float* v;                  /* exp_avg_sq */
  int64_t numel;
  int32_t group;             /* the optimiser's param group, 0 .. n_groups - 1: one norm and one clip coefficient per group */
  int32_t first_chunk;       /* written by ac_optim_workspace_floats */
  double lr, eps, beta1, beta2;
  double bias_correction1;   /* 1 - beta1^step and */
  double bias_correction2;   /* 1 - beta2^step of THIS tensor after its step count was incremented, computed by the host in double */
} ac_optim_entry_t;
/* checks the table, writes every first_chunk and returns the floats of d_workspace (two per chunk); -1: refused */
int64_t ac_optim_workspace_floats(ac_optim_entry_t* entries, int32_t n_entries, int32_t n_groups);
/* two launches (the chunks' sums of squares, then their fixed-order sum): d_norms [n_groups] = the L2 norm of each group's gradients
 * (0 for a group without entries), left in device memory. `entries` is the host table, `d_entries` its device copy. */
int ac_optim_grad_norms(int32_t device_id, void* stream, const ac_optim_entry_t* entries, const ac_optim_entry_t* d_entries, int32_t n_entries,
                        int32_t n_groups, float* d_workspace, float* d_norms);
/* one launch: per group coef = min(1, max_grad_norm / (norm + 1e-6)) as torch's clip_grad_norm_ (a NaN norm gives a NaN coefficient;
 * with use_max_grad_norm 0 the coefficient is 1), g <- g coef, then torch's single-tensor Adam: m <- m + (1 - beta1)(g - m),
 * v <- beta2 v + (1 - beta2) g^2, p <- p - (lr / bias_correction1) m / (sqrt(v) / sqrt(bias_correction2) + eps). */
int ac_optim_clip_adam_step(int32_t device_id, void* stream, const ac_optim_entry_t* entries, const ac_optim_entry_t* d_entries,
                            int32_t n_entries, int32_t n_groups, const float* d_norms, double max_grad_norm, int32_t use_max_grad_norm);
/* the kernels' constants, for callers that size tests and tables by them: 0 rows of the loss per workgroup pass, 1 its workgroups at
 * most, 2 elements per optimiser chunk, 3 entries at most, 4 groups at most; -1 otherwise */
int32_t ac_ppo_update_constant(int32_t which);

/* ---- the PPO update's actor and critic as one call each ("The networks as one call"). First the three pieces no layer
 * above covers, each usable on its own; then the chains. Every device pointer is float32; the calls launch on `stream` and return at
 * once; sums over rows are fixed-order (no atomics), so results are bit-identical from run to run. Refused, each with its message and
 * before any launch: a NULL required pointer, M < 1, K outside 1 .. 256, a row count beyond the kernels' 32-bit index, a misaligned x, w
 * or dx of the value head (16 bytes). */
/* the critic's value_out, nn.Linear(128, 1): d_v [M] = x w + b, x [M, 128], w [128], b [1] */
int ac_value_head_forward(int32_t device_id, void* stream, int32_t M, const float* d_x, const float* d_w, const float* d_b, float* d_v);
/* floats of ac_value_head_backward's d_workspace: 129 per workgroup, one workgroup per 64-row tile up to 256; -1: refused */
int64_t ac_value_head_workspace_floats(int32_t M);
/* two launches: upstream d_g [M] -> d_dx [M, 128] = g w (NULL: not computed), d_dw [128] = sum_m g[m] x[m], d_db [1] = sum_m g[m] */
int ac_value_head_backward(int32_t device_id, void* stream, int32_t M, const float* d_g, const float* d_x, const float* d_w, float* d_workspace,
                           float* d_dx, float* d_dw, float* d_db);
/* base.feature_norm, nn.LayerNorm(K) over the raw observation: d_y [M, K] = (x - mean) / sqrt(var + eps) * gamma + beta, biased
 * variance; d_stats [M, 2] (each row's mean and 1 / sqrt(var + eps)) for a backward, or NULL */
int ac_feature_norm_forward(int32_t device_id, void* stream, int32_t M, int32_t K, float eps, const float* d_x, const float* d_gamma,
                            const float* d_beta, float* d_y, float* d_stats);
/* floats of ac_feature_norm_backward's d_workspace: 2 K per workgroup, one workgroup per 64-row tile up to 256; -1: refused */
int64_t ac_feature_norm_workspace_floats(int32_t M, int32_t K);
/* two launches: upstream d_dy [M, K], the forward's d_x and d_stats -> d_dx [M, K] (NULL: not computed; the observation never needs
 * it), d_dgamma, d_dbeta [K] */
int ac_feature_norm_backward(int32_t device_id, void* stream, int32_t M, int32_t K, const float* d_dy, const float* d_x, const float* d_gamma,
                             const float* d_stats, float* d_workspace, float* d_dx, float* d_dgamma, float* d_dbeta);
/* the reference actor's shoot prior (algorithms/ppo/ppo_actor.py:40-49) from d_obs [M, K], K >= 14, in fp32: with a = obs[11] *
 * 57.29577951308232f and d = obs[13] * 10000.0f, alpha0 = 10 if d <= 8000, else 6 if d <= 12000, else 3; beta0 = 3 if a <= 22.5, else
 * 6 if a <= 45, else 10 (a NaN keeps 3 and 10). -> d_alpha0, d_beta0 [M] */
int ac_shoot_prior(int32_t device_id, void* stream, int32_t M, int32_t K, const float* d_obs, float* d_alpha0, float* d_beta0);
/* the three kernels' constants: 0 rows per tile, 1 the forwards' workgroups at most, 2 the backwards' (also their partial sets at
 * most); -1 otherwise */
int32_t ac_net_constant(int32_t which);

/* One network of the reference's PPO / MAPPO policy: [feature_norm] -> base.mlp's blocks -> the GRU layer -> the head MLP's blocks
 * (act.mlp of the actor, mlp of the critic) -> the action heads (actor) or value_out (critic). heads.n_cat == 0 says critic.
 * `params` holds device pointers in this order, `count` of them:
 *   feature_norm (if present): gamma, beta [obs_dim]
 *   each base block:           W [128, K], b, gamma, beta [128]      (K = obs_dim for the first, 128 after)
 *   the GRU layer:             W_ih, W_hh [384, 128], b_ih, b_hh [384], the LayerNorm's gamma, beta [128]
 *   each head block:           W [128, 128], b, gamma, beta [128]
 *   actor:  each categorical head's W [nvec[h], 128], b [nvec[h]], then with shoot columns the one shoot head's W [2, 128], b [2]
 *   critic: value_out's W [128], b [1]
 * A backward's d_grads is a HOST array of `count` device pointers in the same order; every one is written, nothing is accumulated. */
#define AC_NET_MAX_BLOCKS 4
#define AC_NET_MAX_PARAMS 64
typedef struct {
  int32_t obs_dim;               /* the observation's width, 1 .. 256 */
  int32_t feature_norm;          /* 1: base.feature_norm is present */
  int32_t base_blocks;           /* blocks of base.mlp, 1 .. 4 */
  int32_t head_blocks;           /* blocks of the head MLP, 0 .. 4 */
  ac_act_heads_t heads;          /* the actor's heads; n_cat == 0: a critic */
  int32_t mlp_products;          /* AC_PRODUCTS_ of the MLP blocks, */
  int32_t gru_products;          /* of the GRU's recurrence and */
  int32_t gru_dense_products;    /* of the GRU layer's dense products */
  float feature_norm_eps;
  float block_eps[2 * AC_NET_MAX_BLOCKS];   /* the blocks' LayerNorm eps: base blocks first, then head blocks */
  float gru_eps;                 /* the GRU layer's LayerNorm eps */
  const float* params[AC_NET_MAX_PARAMS];
} ac_net_t;
/* Both sizes below round every segment up to a multiple of 4 floats (r4), with M = N T, B = base_blocks + head_blocks:
 * d_saved = [feature_norm: r4(2 M) + r4(M obs_dim)] + B r4(2 M) + (B + 1) 128 M  (each stage's output: an input of the next)
 *           + 128 M (the GRU's y) + 512 M (its gates) + r4(2 M) (its stats) + [shoot columns: 2 r4(M)].
 * It holds what the layer calls keep one by one: each block's input and stats and the GRU layer's y, saved and stats.
 * d_workspace = the larger of
 *   forward:  384 M + 128 N + d_saved's floats without the r4(2 M) terms and the 512 M (the activations of a forward that saves nothing)
 *   backward: 2 * 128 M + [feature_norm: r4(M obs_dim)] + the largest workspace of the layers' own backwards for this shape.
 * -1 with ac_last_error: a NULL net, N or T < 1, obs_dim outside 1 .. 256, base_blocks outside 1 .. 4, head_blocks outside 0 .. 4,
 * an unknown products code, heads that ac_act_eval_* refuses, shoot columns with obs_dim < 14 or without categorical heads. */
int64_t ac_net_workspace_floats(const ac_net_t* net, int32_t N, int32_t T);
int64_t ac_net_saved_floats(const ac_net_t* net, int32_t N, int32_t T);
/* The actor's evaluate_actions: the prior (with shoot columns), [feature_norm], the base blocks, the GRU layer, the head blocks and the
 * heads, queued back to back by the calls above (ac_shoot_prior, ac_feature_norm_*, ac_mlp_block_*_p, ac_gru_layer_*_pd, ac_act_eval_*).
 * d_obs [N T, obs_dim] step-major, d_hxs [N, 128], d_masks [N T], d_actions [N T, n_cat + n_shoot_cols] -> d_logp, d_ent [N T], unscaled.
 * d_saved NULL: nothing is kept for a backward. d_workspace and d_saved are caller-owned, 16-byte aligned; nothing is allocated,
 * nothing waits for the device. Refused as the sizes above, and: a NULL pointer (a parameter's too), a description of the other kind. */
int ac_actor_eval_forward(int32_t device_id, void* stream, const ac_net_t* net, int32_t N, int32_t T, const float* d_obs, const float* d_hxs,
                          const float* d_masks, const float* d_actions, float* d_workspace, float* d_saved, float* d_logp, float* d_ent);
/* upstream d_dlogp, d_dent [N T] (NULL: zero) and the forward's inputs and d_saved -> every parameter's gradient in d_grads */
int ac_actor_eval_backward(int32_t device_id, void* stream, const ac_net_t* net, int32_t N, int32_t T, const float* d_dlogp, const float* d_dent,
                           const float* d_obs, const float* d_hxs, const float* d_masks, const float* d_actions, const float* d_saved,
                           float* d_workspace, float* const* d_grads);
/* The critic: [feature_norm], the base blocks, the GRU layer, the head blocks and value_out -> d_values [N T], d_h_T [N, 128] */
int ac_critic_forward(int32_t device_id, void* stream, const ac_net_t* net, int32_t N, int32_t T, const float* d_obs, const float* d_hxs,
                      const float* d_masks, float* d_workspace, float* d_saved, float* d_values, float* d_h_T);
/* upstream d_dvalues [N T] and d_dh_T [N, 128] (NULL: zero) -> every parameter's gradient in d_grads */
int ac_critic_backward(int32_t device_id, void* stream, const ac_net_t* net, int32_t N, int32_t T, const float* d_dvalues, const float* d_dh_T,
                       const float* d_obs, const float* d_hxs, const float* d_masks, const float* d_saved, float* d_workspace,
                       float* const* d_grads);

const char* ac_last_error(void);
const char* ac_version(void);

#ifdef __cplusplus
}
#endif
#endif
