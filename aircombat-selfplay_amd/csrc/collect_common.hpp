// What the device collectors share (rollout_collect.hpp: the PPO and the MAPPO rollout; eval_collect.hpp: the evaluator;
// league_collect.hpp: the league). Included at the end of aircombat.hip ahead of them (same library, same error channel). Two halves:
//
// The row pieces of the post-step kernels, `__host__ __device__` so that the *_post_step_host exports run the very same code. The kernels
// are streaming kernels with no reuse: ROW_LANES = 32 threads per row, rows = the learner's E * na rows followed by the opponent's
// E * (A - na). A row's threads read the env's done bytes (one address per row: a broadcast) and, only where the env is done, zero the
// row's GRU state with one 16-byte store per lane (32 lanes x 16 B = the 512-byte row).
//
// The host core: CollectCore is what every handle holds (env, learner, opponent, the opponent's state), core_check the refusals every
// create shares, queue_steps the loop every collect / run is: refusals, entry ordering, per step learner -> opponent -> env -> post-step,
// exit ordering. What a form adds (its buffer, its kernel's argument struct, its learner launch) stays with the form.
#pragma once
#include <type_traits>
#include "../../include/aircombat_eval.h"
#include "../../include/aircombat_rollout.h"
#include "../../include/aircombat_rollout_share.h"

namespace roll {
constexpr int ROW_LANES = 32;
constexpr int ONE_BITS = 0x3f800000;   // 1.0f, for hipMemsetD32Async

__host__ __device__ inline void store4(float* p, float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  *reinterpret_cast<float4*>(p) = make_float4(v, v, v, v);   // rows of `hidden` floats (a multiple of 4) off 16-byte aligned arrays
#else
  p[0] = v; p[1] = v; p[2] = v; p[3] = v;
#endif
}
__host__ __device__ inline void copy4(float* dst, const float* src) {
#if defined(__HIP_DEVICE_COMPILE__)
  *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);   // 16-byte aligned: bases from hipMalloc, offsets multiples of 4 floats
#else
  dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
#endif
}
__host__ __device__ inline bool env_done(const uint8_t* dones, int A, int e) {
  bool all = true;
  for (int a = 0; a < A; ++a) all = all && dones[(size_t)e * A + a] != 0;   // every agent of the env, the opponent's included
  return all;
}
// work item `item` = (row, lane): lane `item % ROW_LANES` of row `item / ROW_LANES`; rows [0, E * na) are the learner's, rows
// [E * na, E * A) the opponent's. The caller passes every item below row_items once.
__host__ __device__ inline long long row_items(int E, int A, int na, bool has_opponent) {
  return ((long long)E * na + (has_opponent ? (long long)E * (A - na) : 0)) * ROW_LANES;
}
template <class P>   // any of the three argument structs
__host__ __device__ inline long long post_row_items(const P& p) { return row_items(p.E, p.A, p.na, p.opp_h != nullptr); }
// row j of a side's own state: its mask = 1 - dones_env from lane 0, its GRU row zeroed where the env is done
__host__ __device__ inline void reset_row(float* h, float* masks, long long j, int hidden, int lane, bool done) {
  if (lane == 0) masks[j] = done ? 0.0f : 1.0f;
  if (done)
    for (int k = 4 * lane; k < hidden; k += 4 * ROW_LANES) store4(h + (size_t)j * hidden + k, 0.0f);
}
// the row items of the two rollout forms, P = ac_rollout_post_step_t or ac_share_rollout_post_step_t: what insert() and the buffer's
// insert do for a learner column, and the opponent's rows. The share form's own stores are the ones under `share`.
template <class P>
__host__ __device__ inline void post_rows_one(const P& p, long long item) {
  constexpr bool share = std::is_same_v<P, ac_share_rollout_post_step_t>;
  const int lane = (int)(item % ROW_LANES);
  const long long row = item / ROW_LANES, N = (long long)p.E * p.na;
  if (row < N) {
    const int e = (int)(row / p.na), a = (int)(row % p.na);
    const bool done = env_done(p.dones, p.A, e);
    const size_t src = (size_t)e * p.A + a, next = (size_t)(p.s + 1) * N + row, cur = (size_t)p.s * N + row;
    for (int k = lane; k < p.obs_dim; k += ROW_LANES) p.OBS[next * p.obs_dim + k] = p.obs[src * p.obs_dim + k];
    for (int k = lane; k < p.act_dim; k += ROW_LANES) {
      p.ACTIONS[cur * p.act_dim + k] = p.actions[src * p.env_act_dim + k];
      if constexpr (share) p.LOGP[cur * p.act_dim + k] = p.logp[row];   // the summed log-prob once per head column
    }
    if (lane == 0) p.REWARDS[cur] = p.rewards[src];
    if (lane == ROW_LANES - 1) p.MASKS[next] = done ? 0.0f : 1.0f;
    if constexpr (share)
      if (lane == ROW_LANES - 2) p.ACTIVE_MASKS[next] = (p.dones[src] != 0 && !done) ? 0.0f : 1.0f;
    if (done)
      for (int k = 4 * lane; k < p.hidden; k += 4 * ROW_LANES) {
        store4(p.RNN_ACTOR + next * p.hidden + k, 0.0f);
        store4(p.RNN_CRITIC + next * p.hidden + k, 0.0f);
      }
  } else {
    const long long j = row - N;
    reset_row(p.opp_h, p.opp_masks, j, p.hidden, lane, env_done(p.dones, p.A, (int)(j / (p.A - p.na))));
  }
}
// "" when the sizes and pointers of a rollout step (either form) are usable
template <class P>
inline std::string post_step_error(const P& p) {
  if (p.E < 1 || p.A < 1 || p.A > AC_MAX_AGENTS || p.na < 1 || p.na > p.A) return "E, A (1 .. 8) and na (1 .. A) out of range";
  if (p.obs_dim < 1 || p.act_dim < 1 || p.env_act_dim < p.act_dim) return "obs_dim, act_dim >= 1 and env_act_dim >= act_dim are required";
  if (p.hidden < 4 || p.hidden % 4) return "hidden must be a positive multiple of 4";
  if (p.T < 1 || p.s < 0 || p.s >= p.T) return "slot s must be in 0 .. T - 1";
  if (!p.obs || !p.rewards || !p.actions || !p.dones || !p.OBS || !p.REWARDS || !p.ACTIONS || !p.MASKS || !p.RNN_ACTOR || !p.RNN_CRITIC)
    return "null array";
  if constexpr (std::is_same_v<P, ac_share_rollout_post_step_t>)
    if (!p.logp || !p.SHARE_OBS || !p.LOGP || !p.ACTIVE_MASKS) return "null array";
  if ((p.opp_h == nullptr) != (p.opp_masks == nullptr)) return "opp_h and opp_masks go together";
  if (p.opp_h && p.na == p.A) return "opponent arrays with na = A";
  return "";
}

// ---- the host core
struct CollectCore {
  int device;
  ac_env* env;
  ac_policy_s* learner;              // NULL for the league, whose learner step is the pool's whole-range launch
  ac_policy_s* opp_policy;           // opponent_kind 1
  ac_policy_pool_s* opp_pool;        // opponent_kind 2
  int na, kind;                      // AC_ROLLOUT_* opponent kinds; AC_EVAL_*'s are the same three numbers
  int learner_deterministic, opponent_deterministic;
  int N, M;                          // learner rows E * na, opponent rows E * (A - na)
  float *d_opp_h, *d_opp_masks, *d_opp_logp;
};
static_assert(AC_EVAL_NO_OPPONENT == AC_ROLLOUT_NO_OPPONENT && AC_EVAL_OPPONENT_POLICY == AC_ROLLOUT_OPPONENT_POLICY &&
              AC_EVAL_OPPONENT_POOL == AC_ROLLOUT_OPPONENT_POOL, "one set of opponent kinds");

inline std::string form_mismatch(int opp_wide, const char* what, int learner_wide) {
  auto form = [](int wide) { return wide ? "MAPPO" : "PPO"; };
  return std::string("a ") + form(opp_wide) + "-form opponent " + what + " does not fit a " + form(learner_wide) + "-form learner";
}
inline std::string vs(const char* what, long long a, const char* wa, long long b, const char* wb) {
  return std::string(what) + " differs (" + wa + " " + std::to_string(a) + ", " + wb + " " + std::to_string(b) + ")";
}
// The refusals every create shares, as `fn`: 0 with *c filled in (no device memory yet, the deterministic flags left to the caller),
// -1 with the mismatch named.
inline int core_check(const std::string& fn, ac_env* env, ac_policy_s* learner, void* opponent, int kind, int na, CollectCore* c) {
  auto bad = [&](const std::string& m) { return fail(fn + ": " + m); };
  const int A = env->A;
  if (kind < AC_ROLLOUT_NO_OPPONENT || kind > AC_ROLLOUT_OPPONENT_POOL) return bad("unknown opponent_kind (0 none, 1 policy, 2 pool)");
  if ((kind != AC_ROLLOUT_NO_OPPONENT) != (opponent != nullptr)) return bad("opponent_kind and the opponent handle disagree");
  if (learner->device != env->device) return bad(vs("device", env->device, "env", learner->device, "policy"));
  if (na != A && !(A % 2 == 0 && na == A / 2))
    return bad("na must be A or A / 2 (na " + std::to_string(na) + ", A " + std::to_string(A) + ")");
  if (learner->cfg.obs_dim != env->obs_dim) return bad(vs("obs_dim", env->obs_dim, "env", learner->cfg.obs_dim, "policy"));
  const int nh = learner->cfg.n_cat + learner->cfg.n_shoot;
  if (env->act_dim < nh) return bad(vs("act_dim", env->act_dim, "env", nh, "policy heads"));
  const int M = env->E * (A - na);
  ac_policy_s* op = nullptr;
  ac_policy_pool_s* pool = nullptr;
  if (kind == AC_ROLLOUT_NO_OPPONENT && M != 0)
    return bad("opponent_kind 0 (none) does not fit A - na = " + std::to_string(A - na) + " opponent agents");
  if (kind != AC_ROLLOUT_NO_OPPONENT && M == 0)
    return bad("opponent_kind " + std::to_string(kind) + " does not fit A - na = 0: the learner owns every agent");
  if (kind == AC_ROLLOUT_OPPONENT_POLICY) {
    op = (ac_policy_s*)opponent;
    if (op->wide != learner->wide) return bad(form_mismatch(op->wide, "policy", learner->wide));
    if (op->device != env->device) return bad(vs("device", env->device, "env", op->device, "opponent"));
    if (op->cfg.obs_dim != env->obs_dim) return bad(vs("obs_dim", env->obs_dim, "env", op->cfg.obs_dim, "opponent"));
    if (env->act_dim < op->cfg.n_cat + op->cfg.n_shoot)
      return bad(vs("act_dim", env->act_dim, "env", op->cfg.n_cat + op->cfg.n_shoot, "opponent heads"));
  } else if (kind == AC_ROLLOUT_OPPONENT_POOL) {
    pool = (ac_policy_pool_s*)opponent;
    const ac_policy_config_t& pc = pool->net.cfg;
    if (pool->net.wide != learner->wide) return bad(form_mismatch(pool->net.wide, "pool", learner->wide));
    if (pool->device != env->device) return bad(vs("device", env->device, "env", pool->device, "opponent pool"));
    if (pc.obs_dim != env->obs_dim) return bad(vs("obs_dim", env->obs_dim, "env", pc.obs_dim, "opponent pool"));
    if (env->act_dim < pc.n_cat + pc.n_shoot) return bad(vs("act_dim", env->act_dim, "env", pc.n_cat + pc.n_shoot, "opponent pool heads"));
    if (pool->E < 0) return bad("opponent_kind 2: the pool has no assignment (ac_policy_pool_assign)");
    if (pool->E != env->E) return bad(vs("E", env->E, "env", pool->E, "opponent pool's assignment"));
  }
  *c = CollectCore{env->device, env, learner, op, pool, na, kind, 0, 0, env->E * na, M, nullptr, nullptr, nullptr};
  return 0;
}
// the opponent's state: nothing without an opponent. core_clear queues its initial contents: h and logp zero, masks one.
inline hipError_t core_alloc(CollectCore* c) {
  if (c->M == 0) return hipSuccess;
  hipError_t err = hipMalloc(&c->d_opp_h, sizeof(float) * (size_t)c->M * pol::HID);
  if (err == hipSuccess) err = hipMalloc(&c->d_opp_masks, sizeof(float) * (size_t)c->M);
  if (err == hipSuccess) err = hipMalloc(&c->d_opp_logp, sizeof(float) * (size_t)c->M);
  return err;
}
inline hipError_t core_clear(const CollectCore& c, hipStream_t s) {
  if (c.M == 0) return hipSuccess;
  hipError_t err = hipMemsetAsync(c.d_opp_h, 0, sizeof(float) * (size_t)c.M * pol::HID, s);
  if (err == hipSuccess) err = hipMemsetD32Async((hipDeviceptr_t)c.d_opp_masks, ONE_BITS, (size_t)c.M, s);
  if (err == hipSuccess) err = hipMemsetAsync(c.d_opp_logp, 0, sizeof(float) * (size_t)c.M, s);
  return err;
}
inline void core_free(CollectCore* c) {
  for (float* q : {c->d_opp_h, c->d_opp_masks, c->d_opp_logp}) if (q) (void)hipFree(q);
}

// The loop of ac_rollout_collect, ac_share_rollout_collect, ac_eval_run and ac_league_run, as `fn`. Refused before anything is queued or written:
// weights not loaded (the critic's only where the learner's launch uses it), a pool that no longer fits, what the step itself would
// refuse. Then every launch goes to the env's stream: on entry it is made to wait for the work already queued on `caller` and on
// `extra` (the buffer's stream, a created one; NULL: there is none), with one event of ev_in each; on return both are made to wait
// for the last launch. learner_step(t) queues the learner's launch of step t; post_step(t) queues the form's post-step kernel and
// advances the form's step index; both return 0, or -1 with the error set.
template <class LearnerStep, class PostStep>
int queue_steps(const CollectCore& c, const std::string& fn, hipStream_t caller, hipStream_t extra, const hipEvent_t* ev_in,
                hipEvent_t ev_out, int n_steps, uint64_t opponent_seed, uint64_t opponent_counter0, bool needs_critic,
                LearnerStep learner_step, PostStep post_step) {
  ac_env* env = c.env;
  // (the league has no learner policy: its learner step is the pool's launch, whose members' load state its begin has checked)
  if (c.learner && (!c.learner->loaded[0] || (needs_critic && !c.learner->loaded[1]))) return fail(fn + ": the learner's weights are not loaded");
  if (c.opp_policy && !c.opp_policy->loaded[0]) return fail(fn + ": the opponent's weights are not loaded");
  if (c.opp_pool && c.opp_pool->E != env->E) return fail(fn + ": the opponent pool's assignment no longer covers the env's E");
  if (c.opp_pool && c.opp_pool->net.wide != c.learner->wide)
    return fail(fn + ": " + form_mismatch(c.opp_pool->net.wide, "pool", c.learner->wide));
  if (host_entry(env)) return -1;
  HIP_OK(hipSetDevice(c.device));
  {   // the step's plan built once without launching it: what launch_step would refuse (a hierarchical handle whose controller was
      // never loaded) is refused here, before anything is queued or written
    StepPlan dry;
    if (step_plan(env, nullptr, -1, &dry)) return -1;
  }
  hipStream_t es = env->stream;
  // everything already queued on the entry streams comes first. A failure here has queued no work.
  HIP_OK(hipEventRecord(ev_in[0], caller));
  if (extra) HIP_OK(hipEventRecord(ev_in[1], extra));
  HIP_OK(hipStreamWaitEvent(es, ev_in[0], 0));
  if (extra) HIP_OK(hipStreamWaitEvent(es, ev_in[1], 0));
  const std::string opp_fn = fn + " (opponent)";
  const int det = c.opponent_deterministic;
  const ac_policy_rows_t orows{(int64_t)c.M, env->A - c.na, env->A, c.na, env->act_dim};
  // A launch that fails (none does once the checks above have passed; what is left is the runtime refusing a launch) ends the loop.
  // The form's step index counts the steps queued in full, which is how a caller learns how far a failed call got (rollout.py and
  // evaluate.py advance their counters by it); the exit ordering below is attempted whatever happened.
  int rc = 0;
  for (int t = 0; t < n_steps && rc == 0; ++t) {
    rc = learner_step(t);   // 1. the learner, its actions into the env's action rows
    // 2. the opponent for agents [na, A), on the env's observations, its states in place
    if (!rc && c.opp_policy)
      rc = policy_launch(c.opp_policy, es, &orows, opp_fn, true, false, env->dp.obs, nullptr, AC_CENT_EXPLICIT, c.d_opp_h, nullptr,
                         c.d_opp_masks, det, opponent_seed, opponent_counter0 + t, nullptr, env->d_actions, c.d_opp_logp, c.d_opp_h, nullptr);
    if (!rc && c.opp_pool)
      rc = ac_policy_pool_act(c.opp_pool, es, &orows, env->dp.obs, c.d_opp_h, c.d_opp_masks, det, opponent_seed, opponent_counter0 + t,
                              env->d_actions, c.d_opp_logp, c.d_opp_h);
    if (!rc) rc = launch_step(env, nullptr);   // 3. the env step (the controller first for hierarchical handles)
    if (!rc) rc = post_step(t);                // 4. insert(), or the evaluator's bookkeeping
  }
  // whatever is queued next on the entry streams comes after the steps
  const hipError_t e0 = hipEventRecord(ev_out, es);
  const hipError_t e1 = e0 == hipSuccess ? hipStreamWaitEvent(caller, ev_out, 0) : e0;
  const hipError_t e2 = e0 == hipSuccess && extra ? hipStreamWaitEvent(extra, ev_out, 0) : e0;
  if (rc) return rc;   // (the launch's own message stays in ac_last_error)
  for (hipError_t e : {e0, e1, e2})
    if (e != hipSuccess) return fail(fn + ": ordering after the steps: " + hipGetErrorString(e));
  return 0;
}
}  // namespace roll
