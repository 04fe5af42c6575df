// The device rollout collectors: a whole rollout queued from C++ on the core of collect_common.hpp, in two forms, and the post-step
// kernels that stand in for the runners' insert() plus the buffer's insert.
//   PPO   (include/aircombat_rollout.h)        runner/jsbsim_runner.py:122-133, runner/selfplay_jsbsim_runner.py:103-124 and
//                                              ReplayBuffer.insert (algorithms/utils/buffer.py:77-111)
//   MAPPO (include/aircombat_rollout_share.h)  runner/share_jsbsim_runner.py:196-223 and SharedReplayBuffer.insert (buffer.py:312-343)
// Included at the end of aircombat.hip after collect_common.hpp.
//
// rollout_post_kernel is roll::post_rows_one alone, one item per thread: a learner row's threads copy obs_dim consecutive floats (lanes
// on consecutive addresses) and, only where the env is done, zero the row's two GRU states with one 16-byte store per lane and array.
// The policy kernel has already written the new states, values and log-probs into the buffer's slots, so nothing else of a row moves.
//
// rollout_share_post_kernel has two parts in one item space. Part one is the same rows, which also spread the row's log-prob over
// LOGP's act_dim columns and write ACTIVE_MASKS. Part two is the traffic: SHARE_OBS[s + 1], whose rows (each its env's whole
// A * obs_dim block) lie back to back, so the slot is one linear run of N * A * obs_dim floats and item i of the part writes piece i of
// it: a float4 where A * obs_dim is a multiple of 4 (a uniform choice per launch; every 2v2 / 4v4 env), a float where it is not (1v1 at
// 2 x 15). The sources are the env's obs blocks, each read na times and L2-resident. The grid is capped and strides, so a wave's lanes
// stay on consecutive addresses in every pass. Each kernel keeps its own argument struct (the share form's already spills).
#pragma once
#include "collect_common.hpp"

namespace roll {
constexpr int SHARE_MAX_BLOCKS = 2048;   // 256 CUs x 8 workgroups of 256: the rest of the items by stride

// pieces (float4 or float) of one share row
__host__ __device__ inline int share_row_pieces(const ac_share_rollout_post_step_t& p) {
  const int W = p.A * p.obs_dim;
  return W % 4 == 0 ? W / 4 : W;
}
__host__ __device__ inline long long share_post_items(const ac_share_rollout_post_step_t& p) {
  return post_row_items(p) + (long long)p.E * p.na * share_row_pieces(p);
}
// work item `item` below share_post_items, each passed once
__host__ __device__ inline void share_post_one(const ac_share_rollout_post_step_t& p, long long item) {
  const long long N = (long long)p.E * p.na, rows = post_row_items(p);
  if (item >= rows) {   // SHARE_OBS[s + 1]: piece i of the slot from piece i % pieces of env (i / pieces) / na's block
    const long long i = item - rows;
    const int W = p.A * p.obs_dim, pieces = share_row_pieces(p);
    const long long row = i / pieces;
    const int k = (int)(i % pieces), e = (int)(row / p.na);
    float* dst = p.SHARE_OBS + (size_t)(p.s + 1) * N * W;
    const float* src = p.obs + (size_t)e * W;
    if (W % 4 == 0) copy4(dst + 4 * (size_t)i, src + 4 * k);
    else dst[i] = src[k];
    return;
  }
  post_rows_one(p, item);
}
template <class P>
int post_step_host(const std::string& fn, const P* step, long long (*items_of)(const P&), void (*one)(const P&, long long)) {
  if (!step) return fail(fn + ": null argument");
  const std::string e = post_step_error(*step);
  if (!e.empty()) return fail(fn + ": " + e);
  const long long items = items_of(*step);
  for (long long i = 0; i < items; ++i) one(*step, i);
  return 0;
}
}  // namespace roll

__global__ __launch_bounds__(256) void rollout_post_kernel(const ac_rollout_post_step_t p, const long long items) {
  const long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (item < items) roll::post_rows_one(p, item);
}
__global__ __launch_bounds__(256) void rollout_share_post_kernel(const ac_share_rollout_post_step_t p, const long long items) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x; item < items; item += stride) roll::share_post_one(p, item);
}

struct ac_rollout {
  roll::CollectCore core;
  ac_buffer* buf;
  bool share;                        // the MAPPO form
  float* d_logp;                     // share: [E * na] the learner's summed log-probs of the step in flight; else NULL
  hipEvent_t ev_in[2], ev_out;       // entry: the caller's and the buffer's stream; exit: the env's stream
};
struct ac_share_rollout : ac_rollout {};   // the MAPPO form's opaque name for the same handle

namespace roll {
int rollout_destroy(ac_rollout* r) {
  if (!r) return 0;
  (void)hipSetDevice(r->core.device);
  (void)hipDeviceSynchronize();
  core_free(&r->core);
  if (r->d_logp) (void)hipFree(r->d_logp);
  for (hipEvent_t e : {r->ev_in[0], r->ev_in[1], r->ev_out}) if (e) (void)hipEventDestroy(e);
  if (r->share) delete static_cast<ac_share_rollout*>(r);
  else delete r;
  return 0;
}

int rollout_create_impl(bool share, const std::string& fn, ac_env* env, ac_policy_s* learner, ac_buffer* buffer, void* opponent,
                        const ac_rollout_config_t* cfg, ac_rollout** out) {
  if (!env || !learner || !buffer || !cfg || !out) return fail(fn + ": null argument");
  *out = nullptr;
  auto bad = [&](const std::string& m) { return fail(fn + ": " + m); };
  const ac_buffer_config_t& bc = buffer->cfg;
  // the form first: a handle of the other form gets the pointer to its own create, whatever else differs
  if (!share && learner->wide) return bad("a MAPPO-form policy (ac_policy_mappo_create) is not supported");
  if (!share && bc.share_obs_dim > 0) return bad("a shared buffer (share_obs_dim > 0) is not supported");
  if (share && !learner->wide) return bad("a PPO-form policy (ac_policy_create) is not supported: use ac_rollout_create");
  if (share && bc.share_obs_dim == 0) return bad("a buffer without share_obs (share_obs_dim == 0) is not supported: use ac_rollout_create");
  CollectCore core;
  if (core_check(fn, env, learner, opponent, cfg->opponent_kind, cfg->na, &core)) return -1;
  core.learner_deterministic = cfg->learner_deterministic; core.opponent_deterministic = cfg->opponent_deterministic;
  const int A = env->A, na = cfg->na, nh = learner->cfg.n_cat + learner->cfg.n_shoot;
  if (buffer->device != env->device) return bad(vs("device", env->device, "env", buffer->device, "buffer"));
  if (!learner->cfg.has_critic) return bad("the learner has no critic (values are part of every step)");
  if (bc.n_envs != env->E) return bad(vs("E", env->E, "env", bc.n_envs, "buffer"));
  if (bc.n_agents != na) return bad(vs("na", na, "config", bc.n_agents, "buffer n_agents"));
  if (bc.obs_dim != env->obs_dim) return bad(vs("obs_dim", env->obs_dim, "env", bc.obs_dim, "buffer"));
  if (share && bc.share_obs_dim != A * env->obs_dim)
    return bad(vs("share_obs_dim", (long long)A * env->obs_dim, "env A * obs_dim", bc.share_obs_dim, "buffer"));
  if (share && learner->in_dim[1] != bc.share_obs_dim)
    return bad(vs("cent_obs_dim", bc.share_obs_dim, "buffer share_obs_dim", learner->in_dim[1], "policy"));
  if (bc.act_dim != nh) return bad(vs("act_dim", nh, "policy heads", bc.act_dim, "buffer"));
  if (!share && bc.logp_dim != 1) return bad("the buffer's logp_dim must be 1");
  if (share && bc.logp_dim != bc.act_dim) return bad(vs("logp_dim", bc.act_dim, "buffer act_dim", bc.logp_dim, "buffer logp_dim"));
  const int hid = bc.hidden_layers * bc.hidden_size;
  if (hid != pol::HID) return bad(vs("hidden size", pol::HID, "policy", hid, "buffer"));
  HIP_OK(hipSetDevice(env->device));
  ac_rollout* r = share ? new ac_share_rollout() : new ac_rollout();
  memset(r, 0, sizeof *r);
  r->core = core; r->buf = buffer; r->share = share;
  hipError_t err = hipEventCreateWithFlags(&r->ev_in[0], hipEventDisableTiming);
  if (err == hipSuccess) err = hipEventCreateWithFlags(&r->ev_in[1], hipEventDisableTiming);
  if (err == hipSuccess) err = hipEventCreateWithFlags(&r->ev_out, hipEventDisableTiming);
  if (err == hipSuccess && share) err = hipMalloc(&r->d_logp, sizeof(float) * (size_t)core.N);
  if (err == hipSuccess && share) err = hipMemsetAsync(r->d_logp, 0, sizeof(float) * (size_t)core.N, env->stream);
  if (err == hipSuccess) err = core_alloc(&r->core);
  if (err == hipSuccess) err = core_clear(r->core, env->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(env->stream);
  if (err != hipSuccess) {
    rollout_destroy(r);
    return bad(hipGetErrorString(err));
  }
  *out = r;
  return 0;
}

int rollout_opponent_state(const std::string& fn, ac_rollout* r, float** d_h, float** d_masks) {
  if (!r || !d_h || !d_masks) return fail(fn + ": null argument");
  *d_h = r->core.d_opp_h; *d_masks = r->core.d_opp_masks;
  return 0;
}

int rollout_collect_impl(const std::string& fn, ac_rollout* r, void* stream, int32_t n_steps, uint64_t learner_seed, uint64_t learner_counter0,
                         uint64_t opponent_seed, uint64_t opponent_counter0) {
  if (!r) return fail(fn + ": null handle");
  const CollectCore& c = r->core;
  ac_env* env = c.env;
  ac_buffer* b = r->buf;
  if (n_steps < 1) return fail(fn + ": n_steps must be at least 1");
  if (b->step + n_steps > b->T)
    return fail(fn + ": step index " + std::to_string(b->step) + " + n_steps " + std::to_string(n_steps) + " runs past buffer_size " +
                std::to_string(b->T));
  hipStream_t es = env->stream;
  const int A = env->A, N = c.N;
  const ac_policy_rows_t lrows{(int64_t)N, c.na, A, 0, env->act_dim};
  float* const* f = b->f;
  const size_t hid = pol::HID, W = (size_t)A * env->obs_dim;
  // the two forms' argument structs, filled alike (one is launched); the share form's own fields follow
  ac_rollout_post_step_t p{};
  ac_share_rollout_post_step_t q{};
  auto fill = [&](auto& a) {
    a.E = env->E; a.A = A; a.na = c.na; a.obs_dim = env->obs_dim; a.env_act_dim = env->act_dim; a.act_dim = b->cfg.act_dim; a.hidden = (int)hid;
    a.T = b->T;
    a.obs = env->dp.obs; a.rewards = env->dp.rew; a.actions = env->d_actions; a.dones = env->dp.done;
    a.OBS = f[AC_BUF_OBS]; a.REWARDS = f[AC_BUF_REWARDS]; a.ACTIONS = f[AC_BUF_ACTIONS]; a.MASKS = f[AC_BUF_MASKS];
    a.RNN_ACTOR = f[AC_BUF_RNN_ACTOR]; a.RNN_CRITIC = f[AC_BUF_RNN_CRITIC];
    a.opp_h = c.d_opp_h; a.opp_masks = c.d_opp_masks;
  };
  fill(p); fill(q);
  q.logp = r->d_logp; q.SHARE_OBS = f[AC_BUF_SHARE_OBS]; q.LOGP = f[AC_BUF_LOGP]; q.ACTIVE_MASKS = f[AC_BUF_ACTIVE_MASKS];
  const long long items = r->share ? share_post_items(q) : post_row_items(p);
  const long long blocks = (items + 255) / 256;
  const dim3 grid((unsigned)(r->share ? std::min<long long>(blocks, SHARE_MAX_BLOCKS) : blocks));
  // the learner: slot s in (compact obs rows; the share form's critic on explicit share_obs rows), slot s + 1 (states) and slot s
  // (values) out, the log-probs into LOGP[s] or the share form's scratch, the actions into the env's action rows
  auto learner_step = [&](int t) -> int {
    const size_t s = (size_t)b->step, s1 = s + 1;
    return policy_launch(c.learner, es, &lrows, fn, true, true, f[AC_BUF_OBS] + s * N * env->obs_dim,
                         r->share ? f[AC_BUF_SHARE_OBS] + s * N * W : nullptr, AC_CENT_EXPLICIT, f[AC_BUF_RNN_ACTOR] + s * N * hid,
                         f[AC_BUF_RNN_CRITIC] + s * N * hid, f[AC_BUF_MASKS] + s * N, c.learner_deterministic, learner_seed,
                         learner_counter0 + t, f[AC_BUF_VALUES] + s * N, env->d_actions, r->share ? r->d_logp : f[AC_BUF_LOGP] + s * N,
                         f[AC_BUF_RNN_ACTOR] + s1 * N * hid, f[AC_BUF_RNN_CRITIC] + s1 * N * hid, /*obs_compact=*/1);
  };
  auto post_step = [&](int) -> int {
    p.s = q.s = b->step;
    if (r->share) hipLaunchKernelGGL(rollout_share_post_kernel, grid, dim3(256), 0, es, q, items);
    else hipLaunchKernelGGL(rollout_post_kernel, grid, dim3(256), 0, es, p, items);
    HIP_OK(hipGetLastError());
    b->step = (b->step + 1) % b->T;
    return 0;
  };
  return queue_steps(c, fn, (hipStream_t)stream, b->stream, r->ev_in, r->ev_out, n_steps, opponent_seed, opponent_counter0, true,
                     learner_step, post_step);
}
}  // namespace roll

extern "C" {

int ac_rollout_post_step_host(const ac_rollout_post_step_t* step) {
  return roll::post_step_host<ac_rollout_post_step_t>("ac_rollout_post_step_host", step, roll::post_row_items, roll::post_rows_one);
}
int ac_share_rollout_post_step_host(const ac_share_rollout_post_step_t* step) {
  return roll::post_step_host("ac_share_rollout_post_step_host", step, roll::share_post_items, roll::share_post_one);
}

int ac_rollout_create(ac_env_t* env, ac_policy_t* learner, ac_buffer_t* buffer, void* opponent, const ac_rollout_config_t* cfg,
                      ac_rollout_t** out) {
  return roll::rollout_create_impl(false, "ac_rollout_create", env, learner, buffer, opponent, cfg, out);
}
int ac_share_rollout_create(ac_env_t* env, ac_policy_t* learner, ac_buffer_t* buffer, void* opponent, const ac_rollout_config_t* cfg,
                            ac_share_rollout_t** out) {
  ac_rollout* r = nullptr;
  const int rc = roll::rollout_create_impl(true, "ac_share_rollout_create", env, learner, buffer, opponent, cfg, out ? &r : nullptr);
  if (out) *out = static_cast<ac_share_rollout*>(r);   // (made as one: rollout_create_impl with share)
  return rc;
}

int ac_rollout_destroy(ac_rollout_t* r) { return roll::rollout_destroy(r); }
int ac_share_rollout_destroy(ac_share_rollout_t* r) { return roll::rollout_destroy(r); }

int ac_rollout_opponent_state(ac_rollout_t* r, float** d_h, float** d_masks) {
  return roll::rollout_opponent_state("ac_rollout_opponent_state", r, d_h, d_masks);
}
int ac_share_rollout_opponent_state(ac_share_rollout_t* r, float** d_h, float** d_masks) {
  return roll::rollout_opponent_state("ac_share_rollout_opponent_state", r, d_h, d_masks);
}

int ac_rollout_collect(ac_rollout_t* r, void* stream, int32_t n_steps, uint64_t learner_seed, uint64_t learner_counter0,
                       uint64_t opponent_seed, uint64_t opponent_counter0) {
  return roll::rollout_collect_impl("ac_rollout_collect", r, stream, n_steps, learner_seed, learner_counter0, opponent_seed, opponent_counter0);
}
int ac_share_rollout_collect(ac_share_rollout_t* r, void* stream, int32_t n_steps, uint64_t learner_seed, uint64_t learner_counter0,
                             uint64_t opponent_seed, uint64_t opponent_counter0) {
  return roll::rollout_collect_impl("ac_share_rollout_collect", r, stream, n_steps, learner_seed, learner_counter0, opponent_seed,
                                    opponent_counter0);
}

}  // extern "C"
