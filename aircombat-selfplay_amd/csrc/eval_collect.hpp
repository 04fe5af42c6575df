// The device evaluator (include/aircombat_eval.h): evaluation steps of the runners' eval() queued from C++ on the core of
// collect_common.hpp, and the post-step kernel that stands in for the loops' numpy bookkeeping (runner/jsbsim_runner.py:136-172,
// runner/selfplay_jsbsim_runner.py:127-239, runner/share_jsbsim_runner.py:226-300). Included at the end of aircombat.hip after
// collect_common.hpp.
//
// eval_post_kernel is a streaming kernel with no reuse, in two parts of one item space. Part one is the rows of collect_common.hpp, the
// learner's E * na agent rows followed by the opponent's E * (A - na), every one a roll::reset_row: lane 0 writes the row's mask and,
// only where the env is done, every lane zeroes its 16 bytes of the row's GRU state. Part two is one item per env: the env's accounting
// (cum, len, count, the log) for all A <= 8 agents, so every word of it is read and written by that one item. `remaining` is the only
// word items share, and it is only ever decremented with an integer atomic, so no result depends on the order in which workgroups run.
#pragma once
#include "collect_common.hpp"

namespace roll {
__host__ __device__ inline long long eval_post_items(const ac_eval_post_step_t& p) { return post_row_items(p) + p.E; }
__host__ __device__ inline void eval_one_fewer(int32_t* remaining) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicSub(remaining, 1);
#else
  --*remaining;
#endif
}
// env e's accounting for one step, P = ac_eval_post_step_t or ac_league_post_step_t (league_collect.hpp): every word of it is read and
// written by this one item. Returns the log slot the step filled, -1 where it filled none.
template <class P>
__host__ __device__ inline int account_env(const P& p, int e) {
  const int A = p.A, K = p.K;
  const bool done = env_done(p.dones, A, e);
  float c[AC_MAX_AGENTS];
  for (int a = 0; a < A; ++a) c[a] = p.cum[(size_t)e * A + a] + p.rewards[(size_t)e * A + a];
  const int len = p.len[e] + 1;
  int logged = -1;
  if (done) {
    const int n = p.count[e];
    if (n < K) {
      const size_t slot = (size_t)e * K + n;
      for (int a = 0; a < A; ++a) p.log_ret[slot * A + a] = c[a];
      p.log_len[slot] = len;
      p.log_end[slot] = p.step;
      if (n == K - 1) eval_one_fewer(p.remaining);
      logged = n;
    }
    p.count[e] = n + 1;
  }
  for (int a = 0; a < A; ++a) p.cum[(size_t)e * A + a] = done ? 0.0f : c[a];
  p.len[e] = done ? 0 : len;
  return logged;
}
// work item `item` below eval_post_items, each passed once
__host__ __device__ inline void eval_post_one(const ac_eval_post_step_t& p, long long item) {
  const long long rows = post_row_items(p);
  if (item >= rows) {   // the env's accounting
    (void)account_env(p, (int)(item - rows));
    return;
  }
  const int lane = (int)(item % ROW_LANES);
  const long long row = item / ROW_LANES, N = (long long)p.E * p.na;
  const bool learner = row < N;
  const long long j = learner ? row : row - N;
  const int e = (int)(j / (learner ? p.na : p.A - p.na));
  reset_row(learner ? p.lrn_h : p.opp_h, learner ? p.lrn_masks : p.opp_masks, j, p.hidden, lane, env_done(p.dones, p.A, e));
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
  roll::CollectCore core;
  int K;                             // episodes_per_env: log slots per env
  int step;                          // steps queued since ac_eval_begin; -1 before the first
  float *d_lrn_h, *d_lrn_masks, *d_lrn_logp;
  float *d_cum, *d_log_ret;
  int32_t *d_len, *d_count, *d_log_len, *d_log_end, *d_remaining;
  hipEvent_t ev_in, ev_out;          // entry: the caller's stream; exit: the env's stream
};

namespace {
// the start of an evaluation on stream `s`: states zero, masks one, accounting and log zero, remaining = E
hipError_t eval_clear(ac_eval* v, hipStream_t s) {
  const roll::CollectCore& c = v->core;
  const size_t E = (size_t)c.env->E, A = (size_t)c.env->A, K = (size_t)v->K, hid = pol::HID;
  hipError_t err = hipMemsetAsync(v->d_lrn_h, 0, sizeof(float) * c.N * hid, s);
  if (err == hipSuccess) err = hipMemsetD32Async((hipDeviceptr_t)v->d_lrn_masks, roll::ONE_BITS, (size_t)c.N, s);
  if (err == hipSuccess) err = hipMemsetAsync(v->d_lrn_logp, 0, sizeof(float) * c.N, s);
  if (err == hipSuccess) err = roll::core_clear(c, s);
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
  const int K = cfg->episodes_per_env;
  if (K < 1 || K > AC_EVAL_MAX_EPISODES)
    return fail("ac_eval_create: episodes_per_env must be in 1 .. " + std::to_string((int)AC_EVAL_MAX_EPISODES) + " (got " + std::to_string(K) + ")");
  roll::CollectCore core;
  if (roll::core_check("ac_eval_create", env, learner, opponent, cfg->opponent_kind, cfg->na, &core)) return -1;
  core.learner_deterministic = cfg->learner_deterministic; core.opponent_deterministic = cfg->opponent_deterministic;
  HIP_OK(hipSetDevice(env->device));
  ac_eval* v = new ac_eval();
  memset(v, 0, sizeof *v);
  v->core = core; v->K = K; v->step = -1;
  const size_t E = (size_t)env->E, A = (size_t)env->A, N = (size_t)core.N, hid = pol::HID;
  hipError_t err = hipEventCreateWithFlags(&v->ev_in, hipEventDisableTiming);
  if (err == hipSuccess) err = hipEventCreateWithFlags(&v->ev_out, hipEventDisableTiming);
  auto alloc = [&](auto** q, size_t words) {
    if (err == hipSuccess) err = hipMalloc((void**)q, 4 * words);
  };
  alloc(&v->d_lrn_h, N * hid); alloc(&v->d_lrn_masks, N); alloc(&v->d_lrn_logp, N);
  if (err == hipSuccess) err = roll::core_alloc(&v->core);
  alloc(&v->d_cum, E * A); alloc(&v->d_len, E); alloc(&v->d_count, E);
  alloc(&v->d_log_ret, E * K * A); alloc(&v->d_log_len, E * K); alloc(&v->d_log_end, E * K); alloc(&v->d_remaining, 1);
  if (err == hipSuccess) err = eval_clear(v, env->stream);   // defined contents for views taken before the first ac_eval_begin
  if (err == hipSuccess) err = hipStreamSynchronize(env->stream);
  if (err != hipSuccess) {
    ac_eval_destroy(v);
    return fail(std::string("ac_eval_create: ") + hipGetErrorString(err));
  }
  *out = v;
  return 0;
}

int ac_eval_destroy(ac_eval_t* v) {
  if (!v) return 0;
  (void)hipSetDevice(v->core.device);
  (void)hipDeviceSynchronize();
  roll::core_free(&v->core);
  for (void* q : {(void*)v->d_lrn_h, (void*)v->d_lrn_masks, (void*)v->d_lrn_logp, (void*)v->d_cum, (void*)v->d_len, (void*)v->d_count,
                  (void*)v->d_log_ret, (void*)v->d_log_len, (void*)v->d_log_end, (void*)v->d_remaining})
    if (q) (void)hipFree(q);
  for (hipEvent_t e : {v->ev_in, v->ev_out}) if (e) (void)hipEventDestroy(e);
  delete v;
  return 0;
}

int ac_eval_state(ac_eval_t* v, ac_eval_state_t* out) {
  if (!v || !out) return fail("ac_eval_state: null argument");
  const roll::CollectCore& c = v->core;
  out->E = c.env->E; out->A = c.env->A; out->na = c.na; out->K = v->K; out->step = v->step; out->pad_ = 0;
  out->lrn_h = v->d_lrn_h; out->lrn_masks = v->d_lrn_masks; out->opp_h = c.d_opp_h; out->opp_masks = c.d_opp_masks;
  out->cum = v->d_cum; out->len = v->d_len; out->count = v->d_count;
  out->log_ret = v->d_log_ret; out->log_len = v->d_log_len; out->log_end = v->d_log_end; out->remaining = v->d_remaining;
  return 0;
}

int ac_eval_begin(ac_eval_t* v, void* stream) {
  if (!v) return fail("ac_eval_begin: null handle");
  ac_env* env = v->core.env;
  if (host_entry(env)) return -1;
  HIP_OK(hipSetDevice(v->core.device));
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
  const roll::CollectCore& c = v->core;
  ac_env* env = c.env;
  if (n_steps < 1) return fail("ac_eval_run: n_steps must be at least 1");
  if (v->step < 0) return fail("ac_eval_run: called before ac_eval_begin");
  if ((long long)v->step + n_steps > INT32_MAX) return fail("ac_eval_run: the step index would pass 2^31 - 1");
  hipStream_t es = env->stream;
  const ac_policy_rows_t lrows{(int64_t)c.N, c.na, env->A, 0, env->act_dim};
  ac_eval_post_step_t p{};
  p.E = env->E; p.A = env->A; p.na = c.na; p.hidden = pol::HID; p.K = v->K;
  p.rewards = env->dp.rew; p.dones = env->dp.done;
  p.lrn_h = v->d_lrn_h; p.lrn_masks = v->d_lrn_masks; p.opp_h = c.d_opp_h; p.opp_masks = c.d_opp_masks;
  p.cum = v->d_cum; p.len = v->d_len; p.count = v->d_count;
  p.log_ret = v->d_log_ret; p.log_len = v->d_log_len; p.log_end = v->d_log_end; p.remaining = v->d_remaining;
  const long long items = roll::eval_post_items(p);
  const dim3 grid((unsigned)((items + 255) / 256));
  // the learner's actor on the env's observations, its states in place, the actions into the env's action rows
  auto learner_step = [&](int t) -> int {
    return policy_launch(c.learner, es, &lrows, "ac_eval_run", true, false, env->dp.obs, nullptr, AC_CENT_EXPLICIT, v->d_lrn_h, nullptr,
                         v->d_lrn_masks, c.learner_deterministic, learner_seed, learner_counter0 + t, nullptr, env->d_actions, v->d_lrn_logp,
                         v->d_lrn_h, nullptr);
  };
  auto post_step = [&](int) -> int {
    p.step = v->step;
    hipLaunchKernelGGL(eval_post_kernel, grid, dim3(256), 0, es, p, items);
    HIP_OK(hipGetLastError());
    v->step += 1;
    return 0;
  };
  return roll::queue_steps(c, "ac_eval_run", (hipStream_t)stream, nullptr, &v->ev_in, v->ev_out, n_steps, opponent_seed, opponent_counter0,
                           false, learner_step, post_step);
}

}  // extern "C"
