// The spawn curriculum (include/aircombat_spawn.h): a bank of K reset templates and a per-env stage, applied behind every step and
// reset of a handle. Included from aircombat.hip behind flight_recorder.hpp: launch_step, host_step and ac_reset call spawn_hook,
// declared ahead of them, before the recorder's hook.
//
// spawn_kernel is a streaming kernel: one lane per aircraft in 64-lane workgroups, no cross-lane work, no atomics. The A lanes of an env
// sit in one wave (A divides 64) and each of them computes the env's bookkeeping from the same loaded words -- spawn::post_step is a
// pure function of them -- so nothing is exchanged between lanes; the lane of aircraft 0 writes the env's words back, after every
// lane of the wave has loaded them (the arrays are not __restrict__: the stores stay behind the loads). An env that was not reset
// loads its info word, its n_ego rewards and its accumulator, and stores the accumulator. An env that was reset also takes the other
// six words, and every lane copies its aircraft from the chosen bank entry as reset_all_kernel copies the handle's own template:
// load_state from the entry, store_state to the lane, the entry's observation (the template's own `tobs` layout) into the lane's row.
//
// A bank entry is what an init kernel writes: [NSW][A] state words followed by [A][tobs] observation floats, and [ND][A] doubles; the
// entries' strides are padded to whole 16-byte groups.
#pragma once
#include "../../include/aircombat_spawn.h"
#include "keyed_uniform.hpp"

namespace spawn {
struct Env { int32_t stage, spawned, episode, wins, played; float ret_acc, return_sum; };

__host__ __device__ inline int clamp_stage(int s, int K) { return s < 0 ? 0 : (s > K - 1 ? K - 1 : s); }
// uniform on [0, s] from the keyed generator, key (seed, env, episode)
__host__ __device__ inline int draw(unsigned long long seed, long long env, long long episode, int s) {
  const float u = pol::policy_uniform(seed, (unsigned long long)episode, env, 0);
  const int k = (int)(u * (float)(s + 1));
  return k > s ? s : k;
}
// (rew[0] + ... + rew[n_ego - 1]) / n_ego in float32. The quotient goes through fp64 so that it is the correctly rounded float32 one
// whatever the build's fp32 division is: 53 bits are more than 2 x 24 + 2, so rounding the fp64 quotient to float32 rounds once.
__host__ __device__ inline float mean_reward(const float* rew, int n_ego) {
  float sum = rew[0];
  for (int j = 1; j < n_ego; ++j) sum += rew[j];
  return (float)((double)sum / (double)n_ego);
}
// Steps 1-4 of the header for one env: returns the bank entry the env is respawned from, -1 where it is not.
__host__ __device__ inline int post_step(const ac_spawn_config_t& r, int K, long long env, bool all, bool was_reset, float mean, Env& v) {
  if (!all) {
    v.ret_acc += mean;
    if (!was_reset) return -1;
    v.played += 1;
    v.return_sum += v.ret_acc;
    v.wins = (int32_t)(((uint32_t)v.wins << 1) | (v.ret_acc >= r.win_return ? 1u : 0u));
  }
  v.ret_acc = 0.0f;
  const uint32_t mask = r.window >= 32 ? 0xFFFFFFFFu : ((1u << r.window) - 1u);
  if (r.mode == AC_SPAWN_AUTO && v.played >= r.window && __builtin_popcount((uint32_t)v.wins & mask) >= r.min_wins) {
    v.stage = v.stage + 1 < K - 1 ? v.stage + 1 : K - 1;
    v.played = 0; v.wins = 0; v.return_sum = 0.0f;
  }
  v.episode += 1;
  const int s = clamp_stage(v.stage, K);
  v.spawned = r.sample == AC_SPAWN_UPTO ? draw(r.seed, env, v.episode, s) : s;
  return v.spawned;
}

// "" when the rule is usable
inline std::string config_error(const ac_spawn_config_t& r) {
  if (r.mode != AC_SPAWN_FIXED && r.mode != AC_SPAWN_AUTO) return "unknown mode (AC_SPAWN_FIXED = 0, AC_SPAWN_AUTO = 1)";
  if (r.sample != AC_SPAWN_AT && r.sample != AC_SPAWN_UPTO) return "unknown sample (AC_SPAWN_AT = 0, AC_SPAWN_UPTO = 1)";
  if (r.window < 1 || r.window > AC_SPAWN_MAX_WINDOW) return "window must be in 1 .. 32 (got " + std::to_string(r.window) + ")";
  if (r.min_wins < 1 || r.min_wins > r.window)
    return "min_wins must be in 1 .. window = " + std::to_string(r.window) + " (got " + std::to_string(r.min_wins) + ")";
  if (r.mode == AC_SPAWN_AUTO && !std::isfinite(r.win_return)) return "AC_SPAWN_AUTO needs a finite win_return";
  return "";
}
// "" when init[K][A] is a usable bank for a handle of that task: the checks of ac_create on cfg.init, entry by entry
inline std::string bank_error(int task, int A, const ac_init_state_t* init, int K) {
  if (task == AC_TASK_HEADING) return "AC_TASK_HEADING has no reset template (every reset draws inside the kernel): nothing to respawn from";
  if (A < 1 || A > AC_MAX_AGENTS) return "A must be in 1 .. 8";
  if (K < 1 || K > AC_SPAWN_MAX_BANK) return "K must be in 1 .. 1024 (got " + std::to_string(K) + ")";
  for (int k = 0; init && k < K; ++k)
    for (int i = 0; i < A; ++i) {
      const ac_init_state_t& ic = init[(size_t)k * A + i];
      const std::string where = "bank entry " + std::to_string(k) + ", aircraft " + std::to_string(i);
      const double v[10] = {ic.lon_deg, ic.lat_geod_deg, ic.h_sl_ft, ic.psi_deg, ic.u_fps, ic.v_fps, ic.w_fps, ic.p_rad_sec, ic.q_rad_sec, ic.r_rad_sec};
      for (double x : v)
        if (!std::isfinite(x)) return where + ": non-finite initial condition";
      if (fabs(ic.lat_geod_deg) > 89.0) return where + ": initial latitude beyond 89 deg (the local frame is not defined on a pole)";
      if (ic.h_sl_ft < -1400.0 || ic.h_sl_ft > 85000.0) return where + ": initial altitude outside -1400 .. 85000 ft (the catalogue's bounds of ic/h-sl-ft)";
    }
  return "";
}

struct Args {
  const float* bF; const double* bD;   // the bank: entry k at bF + k * strideF, bD + k * strideD
  unsigned strideF, strideD;
  int K, all;
  ac_spawn_config_t cfg;
  int32_t* stage; int32_t* spawned; int32_t* episode; float* ret_acc; int32_t* wins; int32_t* played; float* return_sum;
  float* obs2;                         // the host set's observations on a host step, else null
};
}  // namespace spawn

// HOST: a host step, whose set's observations take the respawned rows too. (A template also for where it puts the kernel: template
// kernels are emitted in the order of their first use, so the code object up to and including every step, controller and init kernel
// is laid out exactly as without this file.)
template <bool HOST>
__global__ __launch_bounds__(64) void spawn_kernel(DevPtrs P, DevCfg c, spawn::Args a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = c.N, A = c.A;
  if (n >= N) return;
  const int e = n / A, slot = n - e * A;
  const bool was_reset = a.all || P.info[(size_t)e * 4 + 3] != 0;
  spawn::Env v{};
  v.ret_acc = a.ret_acc[e];
  const float mean = a.all ? 0.0f : spawn::mean_reward(P.rew + (size_t)e * A, c.n_ego);
  if (was_reset) {
    v.stage = a.stage[e]; v.spawned = a.spawned[e]; v.episode = a.episode[e]; v.wins = a.wins[e]; v.played = a.played[e];
    v.return_sum = a.return_sum[e];
  }
  const int k = spawn::post_step(a.cfg, a.K, e, a.all != 0, was_reset, mean, v);
  if (slot == 0) {
    a.ret_acc[e] = v.ret_acc;
    if (was_reset) {
      a.stage[e] = v.stage; a.spawned[e] = v.spawned; a.episode[e] = v.episode; a.wins[e] = v.wins; a.played[e] = v.played;
      a.return_sum[e] = v.return_sum;
    }
  }
  if (k < 0) return;
  const float* tF = a.bF + (size_t)k * a.strideF;     // (k is post_step's clamped index: inside the bank whatever `stage` held)
  const double* tD = a.bD + (size_t)k * a.strideD;
  State s; Task t;
  load_state(tF, reinterpret_cast<const int*>(tF), tD, A, slot, s, t);
  store_state(P.F, P.I, P.D, N, n, s, t);
  const int OBS = c.obs_dim, TOBS = c.tobs;   // the template holds the kernel family's own layout (reset_all_kernel)
  const float* tobs = tF + (size_t)NSW * A + slot * TOBS;
  for (int q = 0; q < OBS; ++q) {
    const float x = (q < TOBS) ? tobs[q] : 0.0f;
    P.obs[(size_t)n * OBS + q] = x;
    if (HOST) a.obs2[(size_t)n * OBS + q] = x;
  }
}

struct ac_spawn {
  ac_env* env;
  int K;
  ac_spawn_config_t cfg;
  float* d_bF; double* d_bD;
  unsigned strideF, strideD;
  int32_t* d_words;   // the seven per-env arrays, one allocation: [7][E] 32-bit words in the order of ac_spawn_state_t
};

namespace spawn {
inline void release(ac_spawn* b) {
  for (void* q : {(void*)b->d_bF, (void*)b->d_bD, (void*)b->d_words})
    if (q) (void)hipFree(q);
  delete b;
}
inline Args args_of(const ac_spawn* b, int all, float* obs2) {
  const size_t E = (size_t)b->env->E;
  int32_t* w = b->d_words;
  return Args{b->d_bF, b->d_bD, b->strideF, b->strideD, b->K, all, b->cfg,
              w, w + E, w + 2 * E, reinterpret_cast<float*>(w + 3 * E), w + 4 * E, w + 5 * E, reinterpret_cast<float*>(w + 6 * E), obs2};
}
}  // namespace spawn

// the spawn kernel queued on the handle's stream behind a step (all = 0; host_set >= 0 on a host step) or a reset (all = 1)
static int spawn_hook(ac_env* h, int all, int host_set) {
  ac_spawn* b = h->spawn;
  if (!b) return 0;
  float* obs2 = host_set >= 0 ? h->hs[host_set].obs : nullptr;
  hipLaunchKernelGGL(obs2 ? spawn_kernel<true> : spawn_kernel<false>, dim3((h->N + 63) / 64), dim3(64), 0, h->stream, h->dp, h->dc, spawn::args_of(b, all, obs2));
  HIP_OK(hipGetLastError());
  h->stream_dirty = true;
  return 0;
}
static void spawn_env_gone(ac_env* h) {   // ac_destroy (the stream is idle): the bank goes with its handle
  if (h->spawn) { spawn::release(h->spawn); h->spawn = nullptr; }
}

extern "C" {

int ac_spawn_check(int32_t task, int32_t A, const ac_init_state_t* init, int32_t K, const ac_spawn_config_t* cfg) {
  if (!cfg) return fail("ac_spawn_check: null argument");
  std::string bad = spawn::bank_error(task, A, init, K);
  if (bad.empty()) bad = spawn::config_error(*cfg);
  return bad.empty() ? 0 : fail("ac_spawn_check: " + bad);
}

int ac_spawn_attach(ac_env_t* env, const ac_init_state_t* init, int32_t K, const ac_spawn_config_t* cfg, ac_spawn_t** out) {
  if (!env || !init || !cfg || !out) return fail("ac_spawn_attach: null argument");
  *out = nullptr;
  std::string bad = spawn::bank_error(env->cfg.task, env->A, init, K);
  if (bad.empty()) bad = spawn::config_error(*cfg);
  if (!bad.empty()) return fail("ac_spawn_attach: " + bad);
  if (env->spawn) return fail("ac_spawn_attach: the handle already has a bank attached (ac_spawn_detach first)");
  if (host_entry(env)) return -1;   // (a host step in flight on the AQL queue ends before the first hooked one)
  HIP_OK(hipSetDevice(env->device));
  const size_t A = (size_t)env->A, E = (size_t)env->E;
  ac_spawn* b = new ac_spawn();
  b->env = env; b->K = K; b->cfg = *cfg;
  b->strideF = (unsigned)(((size_t)NSW * A + A * (size_t)env->dc.tobs + 3) / 4 * 4);
  b->strideD = (unsigned)(((size_t)ND * A + 1) / 2 * 2);
  b->d_bF = nullptr; b->d_bD = nullptr; b->d_words = nullptr;
  const size_t bytesF = sizeof(float) * b->strideF * (size_t)K, bytesD = sizeof(double) * b->strideD * (size_t)K, bytesW = sizeof(int32_t) * 7 * E;
  hipError_t err = hipMalloc((void**)&b->d_bF, bytesF);
  if (err == hipSuccess) err = hipMalloc((void**)&b->d_bD, bytesD);
  if (err == hipSuccess) err = hipMalloc((void**)&b->d_words, bytesW);
  if (err == hipSuccess) err = hipMemsetAsync(b->d_bF, 0, bytesF, env->stream);
  if (err == hipSuccess) err = hipMemsetAsync(b->d_bD, 0, bytesD, env->stream);
  if (err == hipSuccess) err = hipMemsetAsync(b->d_words, 0, bytesW, env->stream);
  if (err == hipSuccess) err = hipMemsetD32Async((hipDeviceptr_t)(b->d_words + E), -1, E, env->stream);   // spawned: the handle's own template
  for (int k = 0; err == hipSuccess && k < K; ++k) {
    InitArgs ia{};
    for (size_t i = 0; i < A; ++i) ia.ic[i] = init[(size_t)k * A + i];
    float* tF = b->d_bF + (size_t)k * b->strideF;
    launch_init_template(env, ia, tF, reinterpret_cast<int*>(tF), b->d_bD + (size_t)k * b->strideD);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipStreamSynchronize(env->stream);
  if (err != hipSuccess) {
    (void)hipGetLastError();   // (an allocation the runtime refuses leaves its error behind for the next hipGetLastError)
    spawn::release(b);
    return fail(std::string("ac_spawn_attach: ") + hipGetErrorString(err) + " (a bank of " + std::to_string(bytesF + bytesD + bytesW) + " bytes)");
  }
  env->spawn = b;
  *out = b;
  return 0;
}

int ac_spawn_detach(ac_env_t* env) {
  if (!env) return fail("ac_spawn_detach: null handle");
  if (!env->spawn) return 0;
  if (host_entry(env)) return -1;
  HIP_OK(hipSetDevice(env->device));
  HIP_OK(hipStreamSynchronize(env->stream));   // no spawn kernel may still be reading the bank
  spawn::release(env->spawn);
  env->spawn = nullptr;
  return 0;
}

int ac_spawn_set_config(ac_spawn_t* b, const ac_spawn_config_t* cfg) {
  if (!b || !cfg) return fail("ac_spawn_set_config: null argument");
  const std::string bad = spawn::config_error(*cfg);
  if (!bad.empty()) return fail("ac_spawn_set_config: " + bad);
  b->cfg = *cfg;   // (a kernel argument of every launch: the launches already queued keep the rule they were queued with)
  return 0;
}

int ac_spawn_state(ac_spawn_t* b, ac_spawn_state_t* out) {
  if (!b || !out) return fail("ac_spawn_state: null argument");
  const spawn::Args a = spawn::args_of(b, 0, nullptr);
  out->E = b->env->E; out->K = b->K;
  out->stage = a.stage; out->spawned = a.spawned; out->episode = a.episode; out->ret_acc = a.ret_acc; out->wins = a.wins; out->played = a.played;
  out->return_sum = a.return_sum;
  return 0;
}

int ac_spawn_post_step_host(const ac_spawn_post_step_t* p) {
  if (!p) return fail("ac_spawn_post_step_host: null argument");
  std::string bad = spawn::config_error(p->cfg);
  if (bad.empty() && (p->E < 1 || p->A < 1 || p->A > AC_MAX_AGENTS || p->n_ego < 1 || p->n_ego > p->A)) bad = "E, A (1 .. 8) and n_ego (1 .. A) out of range";
  if (bad.empty() && (p->K < 1 || p->K > AC_SPAWN_MAX_BANK)) bad = "K must be in 1 .. 1024";
  if (bad.empty() && (!p->stage || !p->spawned || !p->episode || !p->ret_acc || !p->wins || !p->played || !p->return_sum || !p->index)) bad = "null array";
  if (bad.empty() && !p->all_envs && (!p->rewards || !p->info)) bad = "null array";
  if (!bad.empty()) return fail("ac_spawn_post_step_host: " + bad);
  for (int e = 0; e < p->E; ++e) {
    const bool all = p->all_envs != 0, was_reset = all || p->info[(size_t)e * 4 + 3] != 0;
    spawn::Env v{p->stage[e], p->spawned[e], p->episode[e], p->wins[e], p->played[e], p->ret_acc[e], p->return_sum[e]};
    const float mean = all ? 0.0f : spawn::mean_reward(p->rewards + (size_t)e * p->A, p->n_ego);
    p->index[e] = spawn::post_step(p->cfg, p->K, e, all, was_reset, mean, v);
    p->stage[e] = v.stage; p->spawned[e] = v.spawned; p->episode[e] = v.episode; p->wins[e] = v.wins; p->played[e] = v.played;
    p->ret_acc[e] = v.ret_acc; p->return_sum[e] = v.return_sum;
  }
  return 0;
}

int ac_spawn_draw_host(uint64_t seed, int64_t env, int64_t episode, int32_t stage, int32_t* index) {
  if (!index) return fail("ac_spawn_draw_host: null argument");
  if (stage < 0 || stage >= AC_SPAWN_MAX_BANK) return fail("ac_spawn_draw_host: stage must be in 0 .. 1023");
  *index = spawn::draw(seed, env, episode, stage);
  return 0;
}

}  // extern "C"
