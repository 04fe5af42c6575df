// The device league (include/aircombat_league.h): a round-robin of a pool's members against each other on the core of
// collect_common.hpp, and the reduction of its episode log into the [C][C] payoff table. Included at the end of aircombat.hip after
// eval_collect.hpp, whose per-env accounting (roll::account_env) and row pieces (roll::reset_row) it runs.
//
// The "learner" launch of a step is the pool's whole-range launch under a sided plan (policy_pool.hpp): one launch acts for both sides
// of every env. There is no opponent step, so the league owns ONE state array, [E * A] rows in (env, agent) order.
//
// league_post_kernel is a streaming kernel with no reuse, in the two parts of eval_post_kernel over one item space: the E * A rows at
// ROW_LANES = 32 threads per row (lane 0 writes the row's mask; where the env is done every lane zeroes its 16 bytes of the row's GRU
// state with one store), then one item per env for the env's accounting, which also logs the done code of the ending step.
//
// The table is two kernels, both without floating-point atomics and with a fixed summation order. league_partial_kernel: one thread
// per env sums the env's logged slots ascending into the env's partial cell. league_cells_kernel: one wave per cell scans members2 in
// runs of 64 envs; the integer fields add up per lane and are reduced at the end (exact in any order), the two float64 sums are added
// in ascending env order on every lane, each matching env's partial broadcast from its lane in the order of the run's match bits.
#pragma once
#include "eval_collect.hpp"
#include "../../include/aircombat_league.h"

namespace roll {
__host__ __device__ inline long long league_post_items(const ac_league_post_step_t& p) { return ((long long)p.E * p.A) * ROW_LANES + p.E; }
// work item `item` below league_post_items, each passed once
__host__ __device__ inline void league_post_one(const ac_league_post_step_t& p, long long item) {
  const long long rows = (long long)p.E * p.A * ROW_LANES;
  if (item >= rows) {   // the env's accounting, and the done code of the step that ended a logged episode
    const int e = (int)(item - rows);
    const int slot = account_env(p, e);
    if (slot >= 0) p.log_code[(size_t)e * p.K + slot] = p.info[(size_t)e * 4 + 1];
    return;
  }
  const long long row = item / ROW_LANES;
  reset_row(p.h, p.masks, row, p.hidden, (int)(item % ROW_LANES), env_done(p.dones, p.A, (int)(row / p.A)));
}
inline std::string league_post_step_error(const ac_league_post_step_t& p) {
  if (p.E < 1 || p.A < 2 || p.A > AC_MAX_AGENTS || p.A % 2) return "E >= 1 and an even A in 2 .. 8 are required";
  if (p.hidden < 4 || p.hidden % 4) return "hidden must be a positive multiple of 4";
  if (p.K < 1 || p.K > AC_LEAGUE_MAX_EPISODES) return "episodes_per_env K must be in 1 .. " + std::to_string((int)AC_LEAGUE_MAX_EPISODES);
  if (p.step < 0) return "step must be >= 0";
  if (!p.rewards || !p.dones || !p.info || !p.h || !p.masks || !p.cum || !p.len || !p.count || !p.log_ret || !p.log_len || !p.log_end ||
      !p.log_code || !p.remaining)
    return "null array";
  return "";
}

// ---- the table
__host__ __device__ inline ac_league_cell_t league_zero_cell() { return ac_league_cell_t{0, 0, 0, 0, 0, 0, 0.0, 0.0}; }
// env e's partial cell: its logged slots ascending, the float64 sums from 0.0
__host__ __device__ inline ac_league_cell_t league_env_partial(const ac_league_table_args_t& t, int e) {
  ac_league_cell_t c = league_zero_cell();
  const int A = t.A, half = A / 2, n = t.count[e] < t.K ? t.count[e] : t.K;
  for (int k = 0; k < n; ++k) {
    const size_t slot = (size_t)e * t.K + k;
    const float ra = spawn::mean_reward(t.log_ret + slot * A, half), rb = spawn::mean_reward(t.log_ret + slot * A + half, half);
    const float d = ra - rb;
    c.episodes += 1;
    if (d > t.margin) c.wins_a += 1;
    else if (d < -t.margin) c.wins_b += 1;
    else c.draws += 1;
    if (t.log_code[slot] == AC_DONE_TIMEOUT) c.timeouts += 1;
    c.steps += t.log_len[slot];
    c.sum_a += (double)ra;
    c.sum_b += (double)rb;
  }
  return c;
}
__host__ __device__ inline bool league_env_in_cell(const int32_t* members2, int e, int i, int j) {
  return members2[2 * (size_t)e] == i && members2[2 * (size_t)e + 1] == j;
}
inline std::string league_table_error(const ac_league_table_args_t& t) {
  if (t.E < 1 || t.A < 2 || t.A > AC_MAX_AGENTS || t.A % 2) return "E >= 1 and an even A in 2 .. 8 are required";
  if (t.K < 1 || t.K > AC_LEAGUE_MAX_EPISODES) return "episodes_per_env K must be in 1 .. " + std::to_string((int)AC_LEAGUE_MAX_EPISODES);
  if (t.C < 1) return "C must be >= 1";
  if (!std::isfinite(t.margin) || t.margin < 0.0f) return "win_margin must be finite and >= 0";
  if (!t.log_ret || !t.log_len || !t.log_code || !t.count || !t.members2 || !t.out) return "null array";
  return "";
}
}  // namespace roll

__global__ __launch_bounds__(256) void league_post_kernel(const ac_league_post_step_t p, const long long items) {
  const long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (item < items) roll::league_post_one(p, item);
}
// part [E]: every env's partial cell
__global__ __launch_bounds__(256) void league_partial_kernel(const ac_league_table_args_t t, ac_league_cell_t* __restrict__ part) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < t.E) part[e] = roll::league_env_partial(t, e);
}
// one wave per cell (blockIdx.x = i * C + j): t.out[cell] from the partials of the cell's envs, ascending by env
__global__ __launch_bounds__(64) void league_cells_kernel(const ac_league_table_args_t t, const ac_league_cell_t* __restrict__ part) {
  const int cell = blockIdx.x, i = cell / t.C, j = cell % t.C, lane = threadIdx.x;
  long long n[6] = {0, 0, 0, 0, 0, 0};
  double sa = 0.0, sb = 0.0;
  for (int base = 0; base < t.E; base += 64) {
    const int e = base + lane;
    bool mine = false;
    if (e < t.E) mine = roll::league_env_in_cell(t.members2, e, i, j);
    double pa = 0.0, pb = 0.0;
    if (mine) {
      const ac_league_cell_t c = part[e];
      n[0] += c.episodes; n[1] += c.wins_a; n[2] += c.wins_b; n[3] += c.draws; n[4] += c.timeouts; n[5] += c.steps;
      pa = c.sum_a; pb = c.sum_b;
    }
    unsigned long long m = __ballot(mine);   // the run's matches; every lane walks them in env order and adds the same values
    while (m) {
      const int src = __ffsll((long long)m) - 1;
      m &= m - 1;
      sa += __shfl(pa, src, 64);
      sb += __shfl(pb, src, 64);
    }
  }
  for (int k = 0; k < 6; ++k)
    for (int off = 32; off > 0; off >>= 1) n[k] += __shfl_xor(n[k], off, 64);
  if (lane == 0) t.out[cell] = ac_league_cell_t{n[0], n[1], n[2], n[3], n[4], n[5], sa, sb};
}

struct ac_league {
  roll::CollectCore core;            // no learner policy, no opponent: na = A, M = 0
  ac_policy_pool_s* pool;
  int K, deterministic;
  float margin;
  int step;                          // steps queued since ac_league_begin; -1 before the first
  uint64_t plan_gen;                 // the pool's plan as of ac_league_begin
  float *d_h, *d_masks, *d_logp;
  float *d_cum, *d_log_ret;
  int32_t *d_len, *d_count, *d_log_len, *d_log_end, *d_log_code, *d_members2, *d_remaining;
  ac_league_cell_t* d_part;          // [E] the table's per-env partials
  hipEvent_t ev_in, ev_out;          // entry: the caller's stream; exit: the env's stream
};

namespace {
// "" when the pool holds a sided plan for the env's E and A
std::string league_plan_error(const ac_policy_pool_s* pool, const ac_env* env) {
  if (pool->E < 0 || !pool->sided) return "the pool has no sided plan (ac_policy_pool_assign_sides)";
  if (pool->E != env->E) return roll::vs("E", env->E, "env", pool->E, "pool's sided plan");
  if (pool->na != env->A) return roll::vs("A", env->A, "env", pool->na, "pool's sided plan");
  return "";
}
// the start of a round on stream `s`: states zero, masks one, accounting and log zero, remaining = E
hipError_t league_clear(ac_league* v, hipStream_t s) {
  const size_t E = (size_t)v->core.env->E, A = (size_t)v->core.env->A, K = (size_t)v->K, N = E * A;
  hipError_t err = hipMemsetAsync(v->d_h, 0, sizeof(float) * N * pol::HID, s);
  if (err == hipSuccess) err = hipMemsetD32Async((hipDeviceptr_t)v->d_masks, roll::ONE_BITS, N, s);
  if (err == hipSuccess) err = hipMemsetAsync(v->d_logp, 0, sizeof(float) * N, s);
  if (err == hipSuccess) err = hipMemsetAsync(v->d_cum, 0, sizeof(float) * N, s);
  if (err == hipSuccess) err = hipMemsetAsync(v->d_len, 0, sizeof(int32_t) * E, s);
  if (err == hipSuccess) err = hipMemsetAsync(v->d_count, 0, sizeof(int32_t) * E, s);
  if (err == hipSuccess) err = hipMemsetAsync(v->d_log_ret, 0, sizeof(float) * E * K * A, s);
  for (int32_t* q : {v->d_log_len, v->d_log_end, v->d_log_code})
    if (err == hipSuccess) err = hipMemsetAsync(q, 0, sizeof(int32_t) * E * K, s);
  if (err == hipSuccess) err = hipMemsetD32Async((hipDeviceptr_t)v->d_remaining, (int)E, 1, s);
  return err;
}
ac_league_table_args_t league_table_args(const ac_league* v, ac_league_cell_t* out) {
  ac_league_table_args_t t{};
  t.E = v->core.env->E; t.A = v->core.env->A; t.K = v->K; t.C = v->pool->capacity; t.margin = v->margin;
  t.log_ret = v->d_log_ret; t.log_len = v->d_log_len; t.log_code = v->d_log_code; t.count = v->d_count; t.members2 = v->d_members2;
  t.out = out;
  return t;
}
}  // namespace

extern "C" {

int ac_league_post_step_host(const ac_league_post_step_t* step) {
  if (!step) return fail("ac_league_post_step_host: null argument");
  const std::string e = roll::league_post_step_error(*step);
  if (!e.empty()) return fail("ac_league_post_step_host: " + e);
  const long long items = roll::league_post_items(*step);
  for (long long i = 0; i < items; ++i) roll::league_post_one(*step, i);
  return 0;
}

int ac_league_table_host(const ac_league_table_args_t* args) {
  if (!args) return fail("ac_league_table_host: null argument");
  const ac_league_table_args_t& t = *args;
  const std::string err = roll::league_table_error(t);
  if (!err.empty()) return fail("ac_league_table_host: " + err);
  std::vector<ac_league_cell_t> part((size_t)t.E);
  for (int e = 0; e < t.E; ++e) part[e] = roll::league_env_partial(t, e);
  for (int i = 0; i < t.C; ++i)
    for (int j = 0; j < t.C; ++j) {
      ac_league_cell_t c = roll::league_zero_cell();
      for (int e = 0; e < t.E; ++e) {
        if (!roll::league_env_in_cell(t.members2, e, i, j)) continue;
        const ac_league_cell_t& q = part[e];
        c.episodes += q.episodes; c.wins_a += q.wins_a; c.wins_b += q.wins_b; c.draws += q.draws; c.timeouts += q.timeouts;
        c.steps += q.steps; c.sum_a += q.sum_a; c.sum_b += q.sum_b;
      }
      t.out[(size_t)i * t.C + j] = c;
    }
  return 0;
}

int ac_league_create(ac_env_t* env, ac_policy_pool_t* pool, const ac_league_config_t* cfg, ac_league_t** out) {
  if (!env || !pool || !cfg || !out) return fail("ac_league_create: null argument");
  *out = nullptr;
  auto bad = [&](const std::string& m) { return fail("ac_league_create: " + m); };
  const int K = cfg->episodes_per_env;
  if (K < 1 || K > AC_LEAGUE_MAX_EPISODES)
    return bad("episodes_per_env must be in 1 .. " + std::to_string((int)AC_LEAGUE_MAX_EPISODES) + " (got " + std::to_string(K) + ")");
  if (!std::isfinite(cfg->win_margin) || cfg->win_margin < 0.0f) return bad("win_margin must be finite and >= 0");
  const ac_policy_config_t& pc = pool->net.cfg;
  if (pool->device != env->device) return bad(roll::vs("device", env->device, "env", pool->device, "pool"));
  if (pc.obs_dim != env->obs_dim) return bad(roll::vs("obs_dim", env->obs_dim, "env", pc.obs_dim, "pool"));
  if (env->act_dim < pc.n_cat + pc.n_shoot) return bad(roll::vs("act_dim", env->act_dim, "env", pc.n_cat + pc.n_shoot, "pool heads"));
  if (env->A % 2) return bad("A must be even: the sides are agents [0, A/2) and [A/2, A) (A " + std::to_string(env->A) + ")");
  const std::string pe = league_plan_error(pool, env);
  if (!pe.empty()) return bad(pe);
  HIP_OK(hipSetDevice(env->device));
  ac_league* v = new ac_league();
  memset(v, 0, sizeof *v);
  v->core = roll::CollectCore{env->device, env, nullptr, nullptr, nullptr, env->A, AC_ROLLOUT_NO_OPPONENT, 0, 0, env->E * env->A, 0,
                              nullptr, nullptr, nullptr};
  v->pool = pool; v->K = K; v->deterministic = cfg->deterministic ? 1 : 0; v->margin = cfg->win_margin; v->step = -1;
  const size_t E = (size_t)env->E, A = (size_t)env->A, N = E * A, hid = pol::HID;
  hipError_t err = hipEventCreateWithFlags(&v->ev_in, hipEventDisableTiming);
  if (err == hipSuccess) err = hipEventCreateWithFlags(&v->ev_out, hipEventDisableTiming);
  auto alloc = [&](auto** q, size_t words) {
    if (err == hipSuccess) err = hipMalloc((void**)q, 4 * words);
  };
  alloc(&v->d_h, N * hid); alloc(&v->d_masks, N); alloc(&v->d_logp, N);
  alloc(&v->d_cum, N); alloc(&v->d_len, E); alloc(&v->d_count, E);
  alloc(&v->d_log_ret, E * K * A); alloc(&v->d_log_len, E * K); alloc(&v->d_log_end, E * K); alloc(&v->d_log_code, E * K);
  alloc(&v->d_members2, 2 * E); alloc(&v->d_remaining, 1);
  alloc(&v->d_part, E * sizeof(ac_league_cell_t) / 4);
  if (err == hipSuccess) err = league_clear(v, env->stream);   // defined contents for views taken before the first ac_league_begin
  if (err == hipSuccess) err = hipMemsetAsync(v->d_members2, 0xff, sizeof(int32_t) * 2 * E, env->stream);   // (-1, -1): no pair yet
  if (err == hipSuccess) err = hipStreamSynchronize(env->stream);
  if (err != hipSuccess) {
    ac_league_destroy(v);
    return fail(std::string("ac_league_create: ") + hipGetErrorString(err));
  }
  *out = v;
  return 0;
}

int ac_league_destroy(ac_league_t* v) {
  if (!v) return 0;
  (void)hipSetDevice(v->core.device);
  (void)hipDeviceSynchronize();
  for (void* q : {(void*)v->d_h, (void*)v->d_masks, (void*)v->d_logp, (void*)v->d_cum, (void*)v->d_len, (void*)v->d_count, (void*)v->d_log_ret,
                  (void*)v->d_log_len, (void*)v->d_log_end, (void*)v->d_log_code, (void*)v->d_members2, (void*)v->d_remaining, (void*)v->d_part})
    if (q) (void)hipFree(q);
  for (hipEvent_t e : {v->ev_in, v->ev_out}) if (e) (void)hipEventDestroy(e);
  delete v;
  return 0;
}

int ac_league_state(ac_league_t* v, ac_league_state_t* out) {
  if (!v || !out) return fail("ac_league_state: null argument");
  out->E = v->core.env->E; out->A = v->core.env->A; out->K = v->K; out->C = v->pool->capacity; out->step = v->step; out->pad_ = 0;
  out->h = v->d_h; out->masks = v->d_masks; out->cum = v->d_cum; out->len = v->d_len; out->count = v->d_count;
  out->log_ret = v->d_log_ret; out->log_len = v->d_log_len; out->log_end = v->d_log_end; out->log_code = v->d_log_code;
  out->members2 = v->d_members2; out->remaining = v->d_remaining;
  return 0;
}

int ac_league_begin(ac_league_t* v, void* stream) {
  if (!v) return fail("ac_league_begin: null handle");
  ac_env* env = v->core.env;
  ac_policy_pool_s* pool = v->pool;
  auto bad = [&](const std::string& m) { return fail("ac_league_begin: " + m); };
  const std::string pe = league_plan_error(pool, env);
  if (!pe.empty()) return bad(pe);
  if (host_entry(env)) return -1;
  HIP_OK(hipSetDevice(v->core.device));
  hipStream_t es = env->stream;
  HIP_OK(hipEventRecord(v->ev_in, (hipStream_t)stream));
  HIP_OK(hipStreamWaitEvent(es, v->ev_in, 0));
  {   // the assignment and its plan's verdict read back: the one host wait of a round, before anything is written
    const int64_t E = env->E;
    std::vector<int32_t> m2((size_t)(2 * E));
    const pol::Plan a = pool_plan_args(nullptr, 0, 1, pool->capacity, nullptr, pool->d_scratch, nullptr, nullptr);
    int32_t bad_half = -1;
    HIP_OK(hipMemcpyAsync(m2.data(), pool->d_members, sizeof(int32_t) * 2 * E, hipMemcpyDeviceToHost, es));
    HIP_OK(hipMemcpyAsync(&bad_half, a.bad_env, sizeof(int32_t), hipMemcpyDeviceToHost, es));
    HIP_OK(hipStreamSynchronize(es));
    for (int64_t i = 0; i < 2 * E; ++i)
      if (m2[i] == -1)
        return bad("env " + std::to_string(i / 2) + " has side " + std::to_string(i % 2) + " assigned -1: a league acts for both sides of every env");
    if (bad_half >= 0)
      return bad("env " + std::to_string(bad_half / 2) + " has member " + std::to_string(m2[bad_half]) + " on side " + std::to_string(bad_half % 2) +
                 ", which is out of range (capacity " + std::to_string(pool->capacity) + ") or not loaded");
  }
  hipError_t err = hipMemcpyAsync(v->d_members2, pool->d_members, sizeof(int32_t) * 2 * env->E, hipMemcpyDeviceToDevice, es);
  if (err == hipSuccess) err = league_clear(v, es);
  const hipError_t e0 = hipEventRecord(v->ev_out, es);
  const hipError_t e1 = e0 == hipSuccess ? hipStreamWaitEvent((hipStream_t)stream, v->ev_out, 0) : e0;
  for (hipError_t e : {err, e0, e1})
    if (e != hipSuccess) return fail(std::string("ac_league_begin: ") + hipGetErrorString(e));
  v->step = 0;
  v->plan_gen = pool->plan_gen;
  return 0;
}

int ac_league_run(ac_league_t* v, void* stream, int32_t n_steps, uint64_t seed, uint64_t counter0) {
  if (!v) return fail("ac_league_run: null handle");
  const roll::CollectCore& c = v->core;
  ac_env* env = c.env;
  ac_policy_pool_s* pool = v->pool;
  if (n_steps < 1) return fail("ac_league_run: n_steps must be at least 1");
  if (v->step < 0) return fail("ac_league_run: called before ac_league_begin");
  if ((long long)v->step + n_steps > INT32_MAX) return fail("ac_league_run: the step index would pass 2^31 - 1");
  const std::string pe = league_plan_error(pool, env);
  if (!pe.empty()) return fail("ac_league_run: " + pe);
  if (pool->plan_gen != v->plan_gen) return fail("ac_league_run: the pool was assigned again since ac_league_begin (begin a new round)");
  hipStream_t es = env->stream;
  const ac_policy_rows_t rows{(int64_t)c.N, env->A, env->A, 0, env->act_dim};
  ac_league_post_step_t p{};
  p.E = env->E; p.A = env->A; p.hidden = pol::HID; p.K = v->K;
  p.rewards = env->dp.rew; p.dones = env->dp.done; p.info = env->dp.info;
  p.h = v->d_h; p.masks = v->d_masks; p.cum = v->d_cum; p.len = v->d_len; p.count = v->d_count;
  p.log_ret = v->d_log_ret; p.log_len = v->d_log_len; p.log_end = v->d_log_end; p.log_code = v->d_log_code; p.remaining = v->d_remaining;
  const long long items = roll::league_post_items(p);
  const dim3 grid((unsigned)((items + 255) / 256));
  // both sides of every env in the pool's one launch, on the env's observations, the states in place, the actions into the env's rows
  auto pool_step = [&](int t) -> int {
    return ac_policy_pool_act(pool, es, &rows, env->dp.obs, v->d_h, v->d_masks, v->deterministic, seed, counter0 + t, env->d_actions,
                              v->d_logp, v->d_h);
  };
  auto post_step = [&](int) -> int {
    p.step = v->step;
    hipLaunchKernelGGL(league_post_kernel, grid, dim3(256), 0, es, p, items);
    HIP_OK(hipGetLastError());
    v->step += 1;
    return 0;
  };
  return roll::queue_steps(c, "ac_league_run", (hipStream_t)stream, nullptr, &v->ev_in, v->ev_out, n_steps, 0, 0, false, pool_step, post_step);
}

int ac_league_table(ac_league_t* v, void* stream, ac_league_cell_t* d_out) {
  if (!v || !d_out) return fail("ac_league_table: null argument");
  if (v->step < 0) return fail("ac_league_table: called before ac_league_begin");
  ac_env* env = v->core.env;
  if (host_entry(env)) return -1;
  HIP_OK(hipSetDevice(v->core.device));
  hipStream_t es = env->stream;
  const ac_league_table_args_t t = league_table_args(v, d_out);
  HIP_OK(hipEventRecord(v->ev_in, (hipStream_t)stream));
  HIP_OK(hipStreamWaitEvent(es, v->ev_in, 0));
  hipLaunchKernelGGL(league_partial_kernel, dim3((unsigned)((t.E + 255) / 256)), dim3(256), 0, es, t, v->d_part);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) {
    hipLaunchKernelGGL(league_cells_kernel, dim3((unsigned)(t.C * t.C)), dim3(64), 0, es, t, (const ac_league_cell_t*)v->d_part);
    err = hipGetLastError();
  }
  const hipError_t e0 = hipEventRecord(v->ev_out, es);
  const hipError_t e1 = e0 == hipSuccess ? hipStreamWaitEvent((hipStream_t)stream, v->ev_out, 0) : e0;
  for (hipError_t e : {err, e0, e1})
    if (e != hipSuccess) return fail(std::string("ac_league_table: ") + hipGetErrorString(e));
  return 0;
}

}  // extern "C"
