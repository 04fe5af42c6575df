// The device MAPPO rollout collector (include/aircombat_rollout_share.h): a whole rollout of the share runner queued from C++, and the
// post-step kernel that stands in for the runner's insert() (runner/share_jsbsim_runner.py:196-223) plus SharedReplayBuffer.insert
// (algorithms/utils/buffer.py:312-343). Included at the end of aircombat.hip after rollout_collect.hpp, whose roll:: helpers it shares.
//
// rollout_share_post_kernel is a streaming kernel with no reuse, in two parts of one item space. Part one is rollout_post_kernel's
// shape: ROW_LANES = 32 threads per row, rows = the learner's E * na buffer columns followed by the opponent's E * (A - na); a row's
// threads read the env's done bytes (a broadcast), copy obs_dim consecutive floats, spread the row's log-prob over LOGP's act_dim
// columns, write the two masks and, only where the env is done, zero the row's GRU states with 16-byte stores. Part two is the
// traffic: SHARE_OBS[s + 1], whose rows (each its env's whole A * obs_dim block) lie back to back, so the slot is one linear run of
// N * A * obs_dim floats and item i of the part writes piece i of it: a float4 where A * obs_dim is a multiple of 4 (a uniform choice
// per launch; every 2v2 / 4v4 env), a float where it is not (1v1 at 2 x 15). The sources are the env's obs blocks, each read na times
// and L2-resident. The grid is capped and strides, so a wave's lanes stay on consecutive addresses in every pass.
#pragma once
#include "../../include/aircombat_rollout_share.h"

namespace roll {
constexpr int SHARE_MAX_BLOCKS = 2048;   // 256 CUs x 8 workgroups of 256: the rest of the items by stride

__host__ __device__ inline void copy4(float* dst, const float* src) {
#if defined(__HIP_DEVICE_COMPILE__)
  *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);   // 16-byte aligned: bases from hipMalloc, offsets multiples of 4 floats
#else
  dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
#endif
}
__host__ __device__ inline bool share_env_done(const ac_share_rollout_post_step_t& p, int e) {
  bool all = true;
  for (int a = 0; a < p.A; ++a) all = all && p.dones[(size_t)e * p.A + a] != 0;   // every agent of the env, the opponent's included
  return all;
}
// items of part one: (row, lane) as in rollout_post_items
__host__ __device__ inline long long share_row_items(const ac_share_rollout_post_step_t& p) {
  return ((long long)p.E * p.na + (p.opp_h ? (long long)p.E * (p.A - p.na) : 0)) * ROW_LANES;
}
// pieces (float4 or float) of one share row
__host__ __device__ inline int share_row_pieces(const ac_share_rollout_post_step_t& p) {
  const int W = p.A * p.obs_dim;
  return W % 4 == 0 ? W / 4 : W;
}
__host__ __device__ inline long long share_post_items(const ac_share_rollout_post_step_t& p) {
  return share_row_items(p) + (long long)p.E * p.na * share_row_pieces(p);
}
// work item `item` below share_post_items, each passed once
__host__ __device__ inline void share_post_one(const ac_share_rollout_post_step_t& p, long long item) {
  const long long N = (long long)p.E * p.na, row_items = share_row_items(p);
  if (item >= row_items) {   // SHARE_OBS[s + 1]: piece i of the slot from piece i % pieces of env (i / pieces) / na's block
    const long long i = item - row_items;
    const int W = p.A * p.obs_dim, pieces = share_row_pieces(p);
    const long long row = i / pieces;
    const int k = (int)(i % pieces), e = (int)(row / p.na);
    float* dst = p.SHARE_OBS + (size_t)(p.s + 1) * N * W;
    const float* src = p.obs + (size_t)e * W;
    if (W % 4 == 0) copy4(dst + 4 * (size_t)i, src + 4 * k);
    else dst[i] = src[k];
    return;
  }
  const int lane = (int)(item % ROW_LANES);
  const long long row = item / ROW_LANES;
  if (row < N) {
    const int e = (int)(row / p.na), a = (int)(row % p.na);
    const bool done = share_env_done(p, e);
    const size_t src = (size_t)e * p.A + a, next = (size_t)(p.s + 1) * N + row, cur = (size_t)p.s * N + row;
    for (int k = lane; k < p.obs_dim; k += ROW_LANES) p.OBS[next * p.obs_dim + k] = p.obs[src * p.obs_dim + k];
    for (int k = lane; k < p.act_dim; k += ROW_LANES) {
      p.ACTIONS[cur * p.act_dim + k] = p.actions[src * p.env_act_dim + k];
      p.LOGP[cur * p.act_dim + k] = p.logp[row];   // the summed log-prob once per head column
    }
    if (lane == 0) p.REWARDS[cur] = p.rewards[src];
    if (lane == ROW_LANES - 1) p.MASKS[next] = done ? 0.0f : 1.0f;
    if (lane == ROW_LANES - 2) p.ACTIVE_MASKS[next] = (p.dones[src] != 0 && !done) ? 0.0f : 1.0f;
    if (done)
      for (int k = 4 * lane; k < p.hidden; k += 4 * ROW_LANES) {
        store4(p.RNN_ACTOR + next * p.hidden + k, 0.0f);
        store4(p.RNN_CRITIC + next * p.hidden + k, 0.0f);
      }
  } else {
    const long long j = row - N;
    const int e = (int)(j / (p.A - p.na));
    const bool done = share_env_done(p, e);
    if (lane == 0) p.opp_masks[j] = done ? 0.0f : 1.0f;
    if (done)
      for (int k = 4 * lane; k < p.hidden; k += 4 * ROW_LANES) store4(p.opp_h + (size_t)j * p.hidden + k, 0.0f);
  }
}
// "" when the sizes and pointers of a step are usable
inline std::string share_post_step_error(const ac_share_rollout_post_step_t& p) {
  if (p.E < 1 || p.A < 1 || p.A > AC_MAX_AGENTS || p.na < 1 || p.na > p.A) return "E, A (1 .. 8) and na (1 .. A) out of range";
  if (p.obs_dim < 1 || p.act_dim < 1 || p.env_act_dim < p.act_dim) return "obs_dim, act_dim >= 1 and env_act_dim >= act_dim are required";
  if (p.hidden < 4 || p.hidden % 4) return "hidden must be a positive multiple of 4";
  if (p.T < 1 || p.s < 0 || p.s >= p.T) return "slot s must be in 0 .. T - 1";
  if (!p.obs || !p.rewards || !p.actions || !p.dones || !p.logp || !p.OBS || !p.SHARE_OBS || !p.REWARDS || !p.ACTIONS || !p.LOGP || !p.MASKS ||
      !p.ACTIVE_MASKS || !p.RNN_ACTOR || !p.RNN_CRITIC)
    return "null array";
  if ((p.opp_h == nullptr) != (p.opp_masks == nullptr)) return "opp_h and opp_masks go together";
  if (p.opp_h && p.na == p.A) return "opponent arrays with na = A";
  return "";
}
}  // namespace roll

__global__ __launch_bounds__(256) void rollout_share_post_kernel(const ac_share_rollout_post_step_t p, const long long items) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x; item < items; item += stride) roll::share_post_one(p, item);
}

struct ac_share_rollout {
  int device;
  ac_env* env;
  ac_policy_s* learner;
  ac_buffer* buf;
  ac_policy_s* opp_policy;           // opponent_kind 1
  ac_policy_pool_s* opp_pool;        // opponent_kind 2
  ac_rollout_config_t cfg;
  int M;                             // opponent rows, E * (A - na)
  float* d_logp;                     // [E * na] the learner's summed log-probs of the step in flight
  float *d_opp_h, *d_opp_masks, *d_opp_logp;
  hipEvent_t ev_in[2], ev_out;       // entry: the caller's and the buffer's stream; exit: the env's stream
};

extern "C" {

int ac_share_rollout_post_step_host(const ac_share_rollout_post_step_t* step) {
  if (!step) return fail("ac_share_rollout_post_step_host: null argument");
  const std::string e = roll::share_post_step_error(*step);
  if (!e.empty()) return fail("ac_share_rollout_post_step_host: " + e);
  const long long items = roll::share_post_items(*step);
  for (long long i = 0; i < items; ++i) roll::share_post_one(*step, i);
  return 0;
}

int ac_share_rollout_create(ac_env_t* env, ac_policy_t* learner, ac_buffer_t* buffer, void* opponent, const ac_rollout_config_t* cfg,
                            ac_share_rollout_t** out) {
  if (!env || !learner || !buffer || !cfg || !out) return fail("ac_share_rollout_create: null argument");
  *out = nullptr;
  auto bad = [](const std::string& m) { return fail("ac_share_rollout_create: " + m); };
  auto vs = [](const char* what, long long a, const char* wa, long long b, const char* wb) {
    return std::string(what) + " differs (" + wa + " " + std::to_string(a) + ", " + wb + " " + std::to_string(b) + ")";
  };
  const int kind = cfg->opponent_kind, A = env->A, na = cfg->na;
  const ac_buffer_config_t& bc = buffer->cfg;
  if (kind < AC_ROLLOUT_NO_OPPONENT || kind > AC_ROLLOUT_OPPONENT_POOL) return bad("unknown opponent_kind (0 none, 1 policy, 2 pool)");
  if ((kind != AC_ROLLOUT_NO_OPPONENT) != (opponent != nullptr)) return bad("opponent_kind and the opponent handle disagree");
  if (learner->device != env->device) return bad(vs("device", env->device, "env", learner->device, "policy"));
  if (buffer->device != env->device) return bad(vs("device", env->device, "env", buffer->device, "buffer"));
  if (!learner->wide) return bad("a PPO-form policy (ac_policy_create) is not supported: use ac_rollout_create");
  if (bc.share_obs_dim == 0) return bad("a buffer without share_obs (share_obs_dim == 0) is not supported: use ac_rollout_create");
  if (!learner->cfg.has_critic) return bad("the learner has no critic (values are part of every step)");
  if (na != A && !(A % 2 == 0 && na == A / 2))
    return bad("na must be A or A / 2 (na " + std::to_string(na) + ", A " + std::to_string(A) + ")");
  if (bc.n_envs != env->E) return bad(vs("E", env->E, "env", bc.n_envs, "buffer"));
  if (bc.n_agents != na) return bad(vs("na", na, "config", bc.n_agents, "buffer n_agents"));
  if (learner->cfg.obs_dim != env->obs_dim) return bad(vs("obs_dim", env->obs_dim, "env", learner->cfg.obs_dim, "policy"));
  if (bc.obs_dim != env->obs_dim) return bad(vs("obs_dim", env->obs_dim, "env", bc.obs_dim, "buffer"));
  if (bc.share_obs_dim != A * env->obs_dim) return bad(vs("share_obs_dim", (long long)A * env->obs_dim, "env A * obs_dim", bc.share_obs_dim, "buffer"));
  if (learner->in_dim[1] != bc.share_obs_dim) return bad(vs("cent_obs_dim", bc.share_obs_dim, "buffer share_obs_dim", learner->in_dim[1], "policy"));
  const int nh = learner->cfg.n_cat + learner->cfg.n_shoot;
  if (bc.act_dim != nh) return bad(vs("act_dim", nh, "policy heads", bc.act_dim, "buffer"));
  if (env->act_dim < nh) return bad(vs("act_dim", env->act_dim, "env", nh, "policy heads"));
  if (bc.logp_dim != bc.act_dim) return bad(vs("logp_dim", bc.act_dim, "buffer act_dim", bc.logp_dim, "buffer logp_dim"));
  const int hid = bc.hidden_layers * bc.hidden_size;
  if (hid != pol::HID) return bad(vs("hidden size", pol::HID, "policy", hid, "buffer"));
  const int M = env->E * (A - na);
  ac_policy_s* op = nullptr;
  ac_policy_pool_s* pool = nullptr;
  if (kind == AC_ROLLOUT_NO_OPPONENT && M != 0)
    return bad("opponent_kind 0 (none) does not fit A - na = " + std::to_string(A - na) + " opponent agents");
  if (kind != AC_ROLLOUT_NO_OPPONENT && M == 0) return bad("opponent_kind " + std::to_string(kind) + " does not fit A - na = 0: the learner owns every agent");
  if (kind == AC_ROLLOUT_OPPONENT_POLICY) {
    op = (ac_policy_s*)opponent;
    if (!op->wide) return bad("a PPO-form opponent policy is not supported");
    if (op->device != env->device) return bad(vs("device", env->device, "env", op->device, "opponent"));
    if (op->cfg.obs_dim != env->obs_dim) return bad(vs("obs_dim", env->obs_dim, "env", op->cfg.obs_dim, "opponent"));
    if (env->act_dim < op->cfg.n_cat + op->cfg.n_shoot) return bad(vs("act_dim", env->act_dim, "env", op->cfg.n_cat + op->cfg.n_shoot, "opponent heads"));
  } else if (kind == AC_ROLLOUT_OPPONENT_POOL) {
    pool = (ac_policy_pool_s*)opponent;
    const ac_policy_config_t& c = pool->net.cfg;
    if (!pool->net.wide) return bad("a PPO-form opponent pool (AC_POOL_PPO) is not supported");
    if (pool->device != env->device) return bad(vs("device", env->device, "env", pool->device, "opponent pool"));
    if (c.obs_dim != env->obs_dim) return bad(vs("obs_dim", env->obs_dim, "env", c.obs_dim, "opponent pool"));
    if (env->act_dim < c.n_cat + c.n_shoot) return bad(vs("act_dim", env->act_dim, "env", c.n_cat + c.n_shoot, "opponent pool heads"));
    if (pool->E < 0) return bad("opponent_kind 2: the pool has no assignment (ac_policy_pool_assign)");
    if (pool->E != env->E) return bad(vs("E", env->E, "env", pool->E, "opponent pool's assignment"));
  }
  HIP_OK(hipSetDevice(env->device));
  ac_share_rollout* r = new ac_share_rollout();
  memset(r, 0, sizeof *r);
  r->device = env->device; r->env = env; r->learner = learner; r->buf = buffer; r->opp_policy = op; r->opp_pool = pool; r->cfg = *cfg; r->M = M;
  const size_t N = (size_t)env->E * na;
  hipError_t err = hipEventCreateWithFlags(&r->ev_in[0], hipEventDisableTiming);
  if (err == hipSuccess) err = hipEventCreateWithFlags(&r->ev_in[1], hipEventDisableTiming);
  if (err == hipSuccess) err = hipEventCreateWithFlags(&r->ev_out, hipEventDisableTiming);
  if (err == hipSuccess) err = hipMalloc(&r->d_logp, sizeof(float) * N);
  if (err == hipSuccess) err = hipMemsetAsync(r->d_logp, 0, sizeof(float) * N, env->stream);
  if (err == hipSuccess && M > 0) {
    err = hipMalloc(&r->d_opp_h, sizeof(float) * (size_t)M * pol::HID);
    if (err == hipSuccess) err = hipMalloc(&r->d_opp_masks, sizeof(float) * (size_t)M);
    if (err == hipSuccess) err = hipMalloc(&r->d_opp_logp, sizeof(float) * (size_t)M);
    if (err == hipSuccess) err = hipMemsetAsync(r->d_opp_h, 0, sizeof(float) * (size_t)M * pol::HID, env->stream);
    if (err == hipSuccess) err = hipMemsetAsync(r->d_opp_logp, 0, sizeof(float) * (size_t)M, env->stream);
    if (err == hipSuccess) {
      hipLaunchKernelGGL(rbuf::fill_kernel, dim3((M + 255) / 256), dim3(256), 0, env->stream, r->d_opp_masks, (int64_t)M, 1.0f);
      err = hipGetLastError();
    }
  }
  if (err == hipSuccess) err = hipStreamSynchronize(env->stream);
  if (err != hipSuccess) {
    ac_share_rollout_destroy(r);
    return bad(hipGetErrorString(err));
  }
  *out = r;
  return 0;
}

int ac_share_rollout_destroy(ac_share_rollout_t* r) {
  if (!r) return 0;
  (void)hipSetDevice(r->device);
  (void)hipDeviceSynchronize();
  for (float* q : {r->d_logp, r->d_opp_h, r->d_opp_masks, r->d_opp_logp}) if (q) (void)hipFree(q);
  for (hipEvent_t e : {r->ev_in[0], r->ev_in[1], r->ev_out}) if (e) (void)hipEventDestroy(e);
  delete r;
  return 0;
}

int ac_share_rollout_opponent_state(ac_share_rollout_t* r, float** d_h, float** d_masks) {
  if (!r || !d_h || !d_masks) return fail("ac_share_rollout_opponent_state: null argument");
  *d_h = r->d_opp_h; *d_masks = r->d_opp_masks;
  return 0;
}

int ac_share_rollout_collect(ac_share_rollout_t* r, void* stream, int32_t n_steps, uint64_t learner_seed, uint64_t learner_counter0,
                             uint64_t opponent_seed, uint64_t opponent_counter0) {
  if (!r) return fail("ac_share_rollout_collect: null handle");
  ac_env* env = r->env;
  ac_buffer* b = r->buf;
  if (n_steps < 1) return fail("ac_share_rollout_collect: n_steps must be at least 1");
  if (b->step + n_steps > b->T)
    return fail("ac_share_rollout_collect: step index " + std::to_string(b->step) + " + n_steps " + std::to_string(n_steps) +
                " runs past buffer_size " + std::to_string(b->T));
  if (!r->learner->loaded[0] || !r->learner->loaded[1]) return fail("ac_share_rollout_collect: the learner's weights are not loaded");
  if (r->opp_policy && !r->opp_policy->loaded[0]) return fail("ac_share_rollout_collect: the opponent's weights are not loaded");
  if (r->opp_pool && r->opp_pool->E != env->E) return fail("ac_share_rollout_collect: the opponent pool's assignment no longer covers the env's E");
  if (host_entry(env)) return -1;
  HIP_OK(hipSetDevice(r->device));
  {   // the step's plan built once without launching it: what launch_step would refuse (a hierarchical handle whose controller was
      // never loaded) is refused here, before anything is queued or written
    StepPlan dry;
    if (step_plan(env, nullptr, -1, &dry)) return -1;
  }
  hipStream_t es = env->stream;
  // everything already queued on the caller's stream and on the buffer's stream comes first. A failure here has queued no work.
  HIP_OK(hipEventRecord(r->ev_in[0], (hipStream_t)stream));
  HIP_OK(hipEventRecord(r->ev_in[1], b->stream));
  HIP_OK(hipStreamWaitEvent(es, r->ev_in[0], 0));
  HIP_OK(hipStreamWaitEvent(es, r->ev_in[1], 0));
  const int E = env->E, A = env->A, na = r->cfg.na, N = E * na;
  const ac_policy_rows_t lrows{(int64_t)N, na, A, 0, env->act_dim};
  const ac_policy_rows_t orows{(int64_t)r->M, A - na, A, na, env->act_dim};
  float* const* f = b->f;
  const size_t hid = pol::HID, W = (size_t)A * env->obs_dim;
  ac_share_rollout_post_step_t p{};
  p.E = E; p.A = A; p.na = na; p.obs_dim = env->obs_dim; p.env_act_dim = env->act_dim; p.act_dim = b->cfg.act_dim; p.hidden = (int)hid; p.T = b->T;
  p.obs = env->dp.obs; p.rewards = env->dp.rew; p.actions = env->d_actions; p.dones = env->dp.done; p.logp = r->d_logp;
  p.OBS = f[AC_BUF_OBS]; p.SHARE_OBS = f[AC_BUF_SHARE_OBS]; p.REWARDS = f[AC_BUF_REWARDS]; p.ACTIONS = f[AC_BUF_ACTIONS]; p.LOGP = f[AC_BUF_LOGP];
  p.MASKS = f[AC_BUF_MASKS]; p.ACTIVE_MASKS = f[AC_BUF_ACTIVE_MASKS]; p.RNN_ACTOR = f[AC_BUF_RNN_ACTOR]; p.RNN_CRITIC = f[AC_BUF_RNN_CRITIC];
  p.opp_h = r->d_opp_h; p.opp_masks = r->d_opp_masks;
  const long long items = roll::share_post_items(p);
  const dim3 grid((unsigned)std::min<long long>((items + 255) / 256, roll::SHARE_MAX_BLOCKS));
  // A launch that fails (none does once the checks above have passed; what is left is the runtime refusing a launch) ends the loop.
  // The buffer's step index counts the steps queued in full, which is how a caller learns how far a failed call got
  // (rollout.py advances its counters by it); the exit ordering below is attempted whatever happened.
  auto one_step = [&](int t) -> int {
    const size_t s = (size_t)b->step, s1 = s + 1;
    // 1. the learner: slot s in (compact obs rows, explicit share_obs rows), slot s + 1 (states) and slot s (values) out, the log-probs
    //    into the scratch, the actions into the env's action rows
    if (policy_launch(r->learner, es, &lrows, "ac_share_rollout_collect", true, true, f[AC_BUF_OBS] + s * N * env->obs_dim,
                      f[AC_BUF_SHARE_OBS] + s * N * W, AC_CENT_EXPLICIT, f[AC_BUF_RNN_ACTOR] + s * N * hid, f[AC_BUF_RNN_CRITIC] + s * N * hid,
                      f[AC_BUF_MASKS] + s * N, r->cfg.learner_deterministic, learner_seed, learner_counter0 + t, f[AC_BUF_VALUES] + s * N,
                      env->d_actions, r->d_logp, f[AC_BUF_RNN_ACTOR] + s1 * N * hid, f[AC_BUF_RNN_CRITIC] + s1 * N * hid, /*obs_compact=*/1))
      return -1;
    // 2. the opponent, on the env's observations, its states in place
    if (r->opp_policy &&
        policy_launch(r->opp_policy, es, &orows, "ac_share_rollout_collect (opponent)", true, false, env->dp.obs, nullptr, AC_CENT_EXPLICIT,
                      r->d_opp_h, nullptr, r->d_opp_masks, r->cfg.opponent_deterministic, opponent_seed, opponent_counter0 + t, nullptr,
                      env->d_actions, r->d_opp_logp, r->d_opp_h, nullptr))
      return -1;
    if (r->opp_pool &&
        ac_policy_pool_act(r->opp_pool, es, &orows, env->dp.obs, r->d_opp_h, r->d_opp_masks, r->cfg.opponent_deterministic, opponent_seed,
                           opponent_counter0 + t, env->d_actions, r->d_opp_logp, r->d_opp_h))
      return -1;
    // 3. the env step (the controller first for hierarchical handles)
    if (launch_step(env, nullptr)) return -1;
    // 4. insert()
    p.s = (int)s;
    hipLaunchKernelGGL(rollout_share_post_kernel, grid, dim3(256), 0, es, p, items);
    HIP_OK(hipGetLastError());
    b->step = (int)(s1 % (size_t)b->T);
    return 0;
  };
  int rc = 0;
  for (int t = 0; t < n_steps && rc == 0; ++t) rc = one_step(t);
  // whatever is queued next on the caller's stream or the buffer's stream comes after the rollout
  const hipError_t e0 = hipEventRecord(r->ev_out, es);
  const hipError_t e1 = e0 == hipSuccess ? hipStreamWaitEvent((hipStream_t)stream, r->ev_out, 0) : e0;
  const hipError_t e2 = e0 == hipSuccess ? hipStreamWaitEvent(b->stream, r->ev_out, 0) : e0;
  if (rc) return rc;   // (the launch's own message stays in ac_last_error)
  for (hipError_t e : {e0, e1, e2})
    if (e != hipSuccess) return fail(std::string("ac_share_rollout_collect: ordering after the rollout: ") + hipGetErrorString(e));
  return 0;
}

}  // extern "C"
