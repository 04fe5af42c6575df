// The device evaluator (include/aircombat_eval.h): evaluation steps of the runners' eval() queued from C++, and the post-step kernel
// that stands in for the loops' numpy bookkeeping (runner/jsbsim_runner.py:136-172, runner/selfplay_jsbsim_runner.py:127-239,
// runner/share_jsbsim_runner.py:226-300). Included at the end of aircombat.hip after rollout_collect.hpp, whose roll:: helpers it shares.
//
// eval_post_kernel is a streaming kernel with no reuse, in two parts of one item space. Part one is rollout_post_kernel's shape:
// ROW_LANES = 32 threads per row, rows = the learner's E * na agent rows followed by the opponent's E * (A - na); a row's threads read
// the env's done bytes (one address per row: a broadcast), lane 0 writes the row's mask and, only where the env is done, every lane
// zeroes its 16 bytes of the row's GRU state. Part two is one item per env: the env's accounting (cum, len, count, the log) for all
// A <= 8 agents, so every word of it is read and written by that one item. `remaining` is the only word items share, and it is only
// ever decremented with an integer atomic, so no result depends on the order in which workgroups run.
#pragma once
#include "../../include/aircombat_eval.h"

namespace roll {
__host__ __device__ inline bool eval_env_done(const ac_eval_post_step_t& p, int e) {
  bool all = true;
  for (int a = 0; a < p.A; ++a) all = all && p.dones[(size_t)e * p.A + a] != 0;   // every agent of the env, the opponent's included
  return all;
}
// items of part one: (row, lane) as in rollout_post_items
__host__ __device__ inline long long eval_row_items(const ac_eval_post_step_t& p) {
  return ((long long)p.E * p.na + (p.opp_h ? (long long)p.E * (p.A - p.na) : 0)) * ROW_LANES;
}
__host__ __device__ inline long long eval_post_items(const ac_eval_post_step_t& p) { return eval_row_items(p) + p.E; }
__host__ __device__ inline void eval_one_fewer(int32_t* remaining) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicSub(remaining, 1);
#else
  --*remaining;
#endif
}
// work item `item` below eval_post_items, each passed once
__host__ __device__ inline void eval_post_one(const ac_eval_post_step_t& p, long long item) {
  const long long row_items = eval_row_items(p);
  if (item >= row_items) {   // the env's accounting
    const int e = (int)(item - row_items), A = p.A, K = p.K;
    const bool done = eval_env_done(p, e);
    float c[AC_MAX_AGENTS];
    for (int a = 0; a < A; ++a) c[a] = p.cum[(size_t)e * A + a] + p.rewards[(size_t)e * A + a];
    const int len = p.len[e] + 1;
    if (done) {
      const int n = p.count[e];
      if (n < K) {
        const size_t slot = (size_t)e * K + n;
        for (int a = 0; a < A; ++a) p.log_ret[slot * A + a] = c[a];
        p.log_len[slot] = len;
        p.log_end[slot] = p.step;
        if (n == K - 1) eval_one_fewer(p.remaining);
      }
      p.count[e] = n + 1;
    }
    for (int a = 0; a < A; ++a) p.cum[(size_t)e * A + a] = done ? 0.0f : c[a];
    p.len[e] = done ? 0 : len;
    return;
  }
  const int lane = (int)(item % ROW_LANES);
  const long long row = item / ROW_LANES, N = (long long)p.E * p.na;
  const bool learner = row < N;
  const long long j = learner ? row : row - N;
  const int e = (int)(j / (learner ? p.na : p.A - p.na));
  float* h = learner ? p.lrn_h : p.opp_h;
  float* masks = learner ? p.lrn_masks : p.opp_masks;
  const bool done = eval_env_done(p, e);
  if (lane == 0) masks[j] = done ? 0.0f : 1.0f;
  if (done)
    for (int k = 4 * lane; k < p.hidden; k += 4 * ROW_LANES) store4(h + (size_t)j * p.hidden + k, 0.0f);
}
// "" when the sizes and pointers of a step are usable
inline std::string eval_post_step_error(const ac_eval_post_step_t& p) {
  if (p.E < 1 || p.A < 1 || p.A > AC_MAX_AGENTS || p.na < 1 || p.na > p.A) return "E, A (1 .. 8) and na (1 .. A) out of range";
  if (p.hidden < 4 || p.hidden % 4) return "hidden must be a positive multiple of 4";
  if (p.K < 1 || p.K > AC_EVAL_MAX_EPISODES) return "episodes_per_env K must be in 1 .. " + std::to_string((int)AC_EVAL_MAX_EPISODES);
  if (p.step < 0) return "step must be >= 0";
  if (!p.rewards || !p.dones || !p.lrn_h || !p.lrn_masks || !p.cum || !p.len || !p.count || !p.log_ret || !p.log_len || !p.log_end || !p.remaining)
    return "null array";
  if ((p.opp_h == nullptr) != (p.opp_masks == nullptr)) return "opp_h and opp_masks go together";
  if (p.opp_h && p.na == p.A) return "opponent arrays with na = A";
  return "";
}
}  // namespace roll

__global__ __launch_bounds__(256) void eval_post_kernel(const ac_eval_post_step_t p, const long long items) {
  const long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (item < items) roll::eval_post_one(p, item);
}

struct ac_eval {
  int device;
  ac_env* env;
  ac_policy_s* learner;
  ac_policy_s* opp_policy;           // opponent_kind 1
  ac_policy_pool_s* opp_pool;        // opponent_kind 2
  ac_eval_config_t cfg;
  int N, M;                          // learner rows E * na, opponent rows E * (A - na)
  int step;                          // steps queued since ac_eval_begin; -1 before the first
  float *d_lrn_h, *d_lrn_masks, *d_lrn_logp, *d_opp_h, *d_opp_masks, *d_opp_logp;
  float *d_cum, *d_log_ret;
  int32_t *d_len, *d_count, *d_log_len, *d_log_end, *d_remaining;
  hipEvent_t ev_in, ev_out;          // entry: the caller's stream; exit: the env's stream
};

namespace {
// the start of an evaluation on stream `s`: states zero, masks one, accounting and log zero, remaining = E
hipError_t eval_clear(ac_eval* v, hipStream_t s) {
  const size_t E = (size_t)v->env->E, A = (size_t)v->env->A, K = (size_t)v->cfg.episodes_per_env, hid = pol::HID;
  const float one = 1.0f;
  unsigned one_bits;
  memcpy(&one_bits, &one, sizeof one_bits);
  hipError_t err = hipMemsetAsync(v->d_lrn_h, 0, sizeof(float) * v->N * hid, s);
  if (err == hipSuccess) err = hipMemsetD32Async((hipDeviceptr_t)v->d_lrn_masks, (int)one_bits, (size_t)v->N, s);
  if (err == hipSuccess) err = hipMemsetAsync(v->d_lrn_logp, 0, sizeof(float) * v->N, s);
  if (err == hipSuccess && v->M > 0) {
    err = hipMemsetAsync(v->d_opp_h, 0, sizeof(float) * v->M * hid, s);
    if (err == hipSuccess) err = hipMemsetD32Async((hipDeviceptr_t)v->d_opp_masks, (int)one_bits, (size_t)v->M, s);
    if (err == hipSuccess) err = hipMemsetAsync(v->d_opp_logp, 0, sizeof(float) * v->M, s);
  }
  if (err == hipSuccess) err = hipMemsetAsync(v->d_cum, 0, sizeof(float) * E * A, s);
  if (err == hipSuccess) err = hipMemsetAsync(v->d_len, 0, sizeof(int32_t) * E, s);
  if (err == hipSuccess) err = hipMemsetAsync(v->d_count, 0, sizeof(int32_t) * E, s);
  if (err == hipSuccess) err = hipMemsetAsync(v->d_log_ret, 0, sizeof(float) * E * K * A, s);
  if (err == hipSuccess) err = hipMemsetAsync(v->d_log_len, 0, sizeof(int32_t) * E * K, s);
  if (err == hipSuccess) err = hipMemsetAsync(v->d_log_end, 0, sizeof(int32_t) * E * K, s);
  if (err == hipSuccess) err = hipMemsetD32Async((hipDeviceptr_t)v->d_remaining, (int)E, 1, s);
  return err;
}
}  // namespace

extern "C" {

int ac_eval_post_step_host(const ac_eval_post_step_t* step) {
  if (!step) return fail("ac_eval_post_step_host: null argument");
  const std::string e = roll::eval_post_step_error(*step);
  if (!e.empty()) return fail("ac_eval_post_step_host: " + e);
  const long long items = roll::eval_post_items(*step);
  for (long long i = 0; i < items; ++i) roll::eval_post_one(*step, i);
  return 0;
}

int ac_eval_create(ac_env_t* env, ac_policy_t* learner, void* opponent, const ac_eval_config_t* cfg, ac_eval_t** out) {
  if (!env || !learner || !cfg || !out) return fail("ac_eval_create: null argument");
  *out = nullptr;
  auto bad = [](const std::string& m) { return fail("ac_eval_create: " + m); };
  auto vs = [](const char* what, long long a, const char* wa, long long b, const char* wb) {
    return std::string(what) + " differs (" + wa + " " + std::to_string(a) + ", " + wb + " " + std::to_string(b) + ")";
  };
  auto form = [](int wide) { return wide ? "MAPPO" : "PPO"; };
  const int kind = cfg->opponent_kind, A = env->A, na = cfg->na, K = cfg->episodes_per_env;
  if (kind < AC_EVAL_NO_OPPONENT || kind > AC_EVAL_OPPONENT_POOL) return bad("unknown opponent_kind (0 none, 1 policy, 2 pool)");
  if ((kind != AC_EVAL_NO_OPPONENT) != (opponent != nullptr)) return bad("opponent_kind and the opponent handle disagree");
  if (K < 1 || K > AC_EVAL_MAX_EPISODES)
    return bad("episodes_per_env must be in 1 .. " + std::to_string((int)AC_EVAL_MAX_EPISODES) + " (got " + std::to_string(K) + ")");
  if (learner->device != env->device) return bad(vs("device", env->device, "env", learner->device, "policy"));
  if (na != A && !(A % 2 == 0 && na == A / 2))
    return bad("na must be A or A / 2 (na " + std::to_string(na) + ", A " + std::to_string(A) + ")");
  if (learner->cfg.obs_dim != env->obs_dim) return bad(vs("obs_dim", env->obs_dim, "env", learner->cfg.obs_dim, "policy"));
  const int nh = learner->cfg.n_cat + learner->cfg.n_shoot;
  if (env->act_dim < nh) return bad(vs("act_dim", env->act_dim, "env", nh, "policy heads"));
  const int M = env->E * (A - na);
  ac_policy_s* op = nullptr;
  ac_policy_pool_s* pool = nullptr;
  if (kind == AC_EVAL_NO_OPPONENT && M != 0)
    return bad("opponent_kind 0 (none) does not fit A - na = " + std::to_string(A - na) + " opponent agents");
  if (kind != AC_EVAL_NO_OPPONENT && M == 0) return bad("opponent_kind " + std::to_string(kind) + " does not fit A - na = 0: the learner owns every agent");
  if (kind == AC_EVAL_OPPONENT_POLICY) {
    op = (ac_policy_s*)opponent;
    if (op->wide != learner->wide)
      return bad(std::string("a ") + form(op->wide) + "-form opponent policy does not fit a " + form(learner->wide) + "-form learner");
    if (op->device != env->device) return bad(vs("device", env->device, "env", op->device, "opponent"));
    if (op->cfg.obs_dim != env->obs_dim) return bad(vs("obs_dim", env->obs_dim, "env", op->cfg.obs_dim, "opponent"));
    if (env->act_dim < op->cfg.n_cat + op->cfg.n_shoot) return bad(vs("act_dim", env->act_dim, "env", op->cfg.n_cat + op->cfg.n_shoot, "opponent heads"));
  } else if (kind == AC_EVAL_OPPONENT_POOL) {
    pool = (ac_policy_pool_s*)opponent;
    const ac_policy_config_t& c = pool->net.cfg;
    if (pool->net.wide != learner->wide)
      return bad(std::string("a ") + form(pool->net.wide) + "-form opponent pool does not fit a " + form(learner->wide) + "-form learner");
    if (pool->device != env->device) return bad(vs("device", env->device, "env", pool->device, "opponent pool"));
    if (c.obs_dim != env->obs_dim) return bad(vs("obs_dim", env->obs_dim, "env", c.obs_dim, "opponent pool"));
    if (env->act_dim < c.n_cat + c.n_shoot) return bad(vs("act_dim", env->act_dim, "env", c.n_cat + c.n_shoot, "opponent pool heads"));
    if (pool->E < 0) return bad("opponent_kind 2: the pool has no assignment (ac_policy_pool_assign)");
    if (pool->E != env->E) return bad(vs("E", env->E, "env", pool->E, "opponent pool's assignment"));
  }
  HIP_OK(hipSetDevice(env->device));
  ac_eval* v = new ac_eval();
  memset(v, 0, sizeof *v);
  v->device = env->device; v->env = env; v->learner = learner; v->opp_policy = op; v->opp_pool = pool; v->cfg = *cfg;
  v->N = env->E * na; v->M = M; v->step = -1;
  const size_t E = (size_t)env->E, hid = pol::HID;
  hipError_t err = hipEventCreateWithFlags(&v->ev_in, hipEventDisableTiming);
  if (err == hipSuccess) err = hipEventCreateWithFlags(&v->ev_out, hipEventDisableTiming);
  auto alloc = [&](auto** q, size_t words) {
    if (err == hipSuccess) err = hipMalloc((void**)q, 4 * words);
  };
  alloc(&v->d_lrn_h, v->N * hid); alloc(&v->d_lrn_masks, v->N); alloc(&v->d_lrn_logp, v->N);
  if (M > 0) { alloc(&v->d_opp_h, M * hid); alloc(&v->d_opp_masks, M); alloc(&v->d_opp_logp, M); }
  alloc(&v->d_cum, E * A); alloc(&v->d_len, E); alloc(&v->d_count, E);
  alloc(&v->d_log_ret, E * K * A); alloc(&v->d_log_len, E * K); alloc(&v->d_log_end, E * K); alloc(&v->d_remaining, 1);
  if (err == hipSuccess) err = eval_clear(v, env->stream);   // defined contents for views taken before the first ac_eval_begin
  if (err == hipSuccess) err = hipStreamSynchronize(env->stream);
  if (err != hipSuccess) {
    ac_eval_destroy(v);
    return bad(hipGetErrorString(err));
  }
  *out = v;
  return 0;
}

int ac_eval_destroy(ac_eval_t* v) {
  if (!v) return 0;
  (void)hipSetDevice(v->device);
  (void)hipDeviceSynchronize();
  for (void* q : {(void*)v->d_lrn_h, (void*)v->d_lrn_masks, (void*)v->d_lrn_logp, (void*)v->d_opp_h, (void*)v->d_opp_masks, (void*)v->d_opp_logp,
                  (void*)v->d_cum, (void*)v->d_len, (void*)v->d_count, (void*)v->d_log_ret, (void*)v->d_log_len, (void*)v->d_log_end,
                  (void*)v->d_remaining})
    if (q) (void)hipFree(q);
  for (hipEvent_t e : {v->ev_in, v->ev_out}) if (e) (void)hipEventDestroy(e);
  delete v;
  return 0;
}

int ac_eval_state(ac_eval_t* v, ac_eval_state_t* out) {
  if (!v || !out) return fail("ac_eval_state: null argument");
  out->E = v->env->E; out->A = v->env->A; out->na = v->cfg.na; out->K = v->cfg.episodes_per_env; out->step = v->step; out->pad_ = 0;
  out->lrn_h = v->d_lrn_h; out->lrn_masks = v->d_lrn_masks; out->opp_h = v->d_opp_h; out->opp_masks = v->d_opp_masks;
  out->cum = v->d_cum; out->len = v->d_len; out->count = v->d_count;
  out->log_ret = v->d_log_ret; out->log_len = v->d_log_len; out->log_end = v->d_log_end; out->remaining = v->d_remaining;
  return 0;
}

int ac_eval_begin(ac_eval_t* v, void* stream) {
  if (!v) return fail("ac_eval_begin: null handle");
  ac_env* env = v->env;
  if (host_entry(env)) return -1;
  HIP_OK(hipSetDevice(v->device));
  hipStream_t es = env->stream;
  HIP_OK(hipEventRecord(v->ev_in, (hipStream_t)stream));
  HIP_OK(hipStreamWaitEvent(es, v->ev_in, 0));
  const hipError_t err = eval_clear(v, es);
  const hipError_t e0 = hipEventRecord(v->ev_out, es);
  const hipError_t e1 = e0 == hipSuccess ? hipStreamWaitEvent((hipStream_t)stream, v->ev_out, 0) : e0;
  for (hipError_t e : {err, e0, e1})
    if (e != hipSuccess) return fail(std::string("ac_eval_begin: ") + hipGetErrorString(e));
  v->step = 0;
  return 0;
}

int ac_eval_run(ac_eval_t* v, void* stream, int32_t n_steps, uint64_t learner_seed, uint64_t learner_counter0, uint64_t opponent_seed,
                uint64_t opponent_counter0) {
  if (!v) return fail("ac_eval_run: null handle");
  ac_env* env = v->env;
  if (n_steps < 1) return fail("ac_eval_run: n_steps must be at least 1");
  if (v->step < 0) return fail("ac_eval_run: called before ac_eval_begin");
  if ((long long)v->step + n_steps > INT32_MAX) return fail("ac_eval_run: the step index would pass 2^31 - 1");
  if (!v->learner->loaded[0]) return fail("ac_eval_run: the learner's weights are not loaded");
  if (v->opp_policy && !v->opp_policy->loaded[0]) return fail("ac_eval_run: the opponent's weights are not loaded");
  if (v->opp_pool && v->opp_pool->E != env->E) return fail("ac_eval_run: the opponent pool's assignment no longer covers the env's E");
  if (host_entry(env)) return -1;
  HIP_OK(hipSetDevice(v->device));
  {   // the step's plan built once without launching it: what launch_step would refuse (a hierarchical handle whose controller was
      // never loaded) is refused here, before anything is queued or written
    StepPlan dry;
    if (step_plan(env, nullptr, -1, &dry)) return -1;
  }
  hipStream_t es = env->stream;
  // everything already queued on the caller's stream comes first. A failure here has queued no work.
  HIP_OK(hipEventRecord(v->ev_in, (hipStream_t)stream));
  HIP_OK(hipStreamWaitEvent(es, v->ev_in, 0));
  const int E = env->E, A = env->A, na = v->cfg.na;
  const ac_policy_rows_t lrows{(int64_t)v->N, na, A, 0, env->act_dim};
  const ac_policy_rows_t orows{(int64_t)v->M, A - na, A, na, env->act_dim};
  ac_eval_post_step_t p{};
  p.E = E; p.A = A; p.na = na; p.hidden = pol::HID; p.K = v->cfg.episodes_per_env;
  p.rewards = env->dp.rew; p.dones = env->dp.done;
  p.lrn_h = v->d_lrn_h; p.lrn_masks = v->d_lrn_masks; p.opp_h = v->d_opp_h; p.opp_masks = v->d_opp_masks;
  p.cum = v->d_cum; p.len = v->d_len; p.count = v->d_count;
  p.log_ret = v->d_log_ret; p.log_len = v->d_log_len; p.log_end = v->d_log_end; p.remaining = v->d_remaining;
  const long long items = roll::eval_post_items(p);
  const dim3 grid((unsigned)((items + 255) / 256));
  // A launch that fails (none does once the checks above have passed; what is left is the runtime refusing a launch) ends the loop.
  // The step index counts the steps queued in full, which is how a caller learns how far a failed call got (evaluate.py advances its
  // counters by it); the exit ordering below is attempted whatever happened.
  auto one_step = [&](int t) -> int {
    // 1. the learner's actor on the env's observations, its states in place, the actions into the env's action rows
    if (policy_launch(v->learner, es, &lrows, "ac_eval_run", true, false, env->dp.obs, nullptr, AC_CENT_EXPLICIT, v->d_lrn_h, nullptr,
                      v->d_lrn_masks, v->cfg.learner_deterministic, learner_seed, learner_counter0 + t, nullptr, env->d_actions, v->d_lrn_logp,
                      v->d_lrn_h, nullptr))
      return -1;
    // 2. the opponent, the same for agents [na, A)
    if (v->opp_policy &&
        policy_launch(v->opp_policy, es, &orows, "ac_eval_run (opponent)", true, false, env->dp.obs, nullptr, AC_CENT_EXPLICIT, v->d_opp_h,
                      nullptr, v->d_opp_masks, v->cfg.opponent_deterministic, opponent_seed, opponent_counter0 + t, nullptr, env->d_actions,
                      v->d_opp_logp, v->d_opp_h, nullptr))
      return -1;
    if (v->opp_pool &&
        ac_policy_pool_act(v->opp_pool, es, &orows, env->dp.obs, v->d_opp_h, v->d_opp_masks, v->cfg.opponent_deterministic, opponent_seed,
                           opponent_counter0 + t, env->d_actions, v->d_opp_logp, v->d_opp_h))
      return -1;
    // 3. the env step (the controller first for hierarchical handles)
    if (launch_step(env, nullptr)) return -1;
    // 4. the bookkeeping
    p.step = v->step;
    hipLaunchKernelGGL(eval_post_kernel, grid, dim3(256), 0, es, p, items);
    HIP_OK(hipGetLastError());
    v->step += 1;
    return 0;
  };
  int rc = 0;
  for (int t = 0; t < n_steps && rc == 0; ++t) rc = one_step(t);
  // whatever is queued next on the caller's stream comes after the evaluation steps
  const hipError_t e0 = hipEventRecord(v->ev_out, es);
  const hipError_t e1 = e0 == hipSuccess ? hipStreamWaitEvent((hipStream_t)stream, v->ev_out, 0) : e0;
  if (rc) return rc;   // (the launch's own message stays in ac_last_error)
  for (hipError_t e : {e0, e1})
    if (e != hipSuccess) return fail(std::string("ac_eval_run: ordering after the steps: ") + hipGetErrorString(e));
  return 0;
}

}  // extern "C"
