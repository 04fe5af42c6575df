// Host side of the device PPO policy (include/aircombat.h, ac_policy_*; the kernel: policy_kernel.hpp). Included at the end of aircombat.hip.
//
// Source blob of one network (fp32, the reference's state_dict tensors in this order, policy.py builds it from the key names):
//   [base.feature_norm.weight, .bias  (obs_dim each, only with use_feature_normalization)]
//   base.mlp.fc.0.weight [128, obs_dim], .bias, fc.2.weight, .bias, fc.3.weight [128, 128], .bias, fc.5.weight, .bias
//   rnn.gru.weight_ih_l0 [384, 128], weight_hh_l0 [384, 128], bias_ih_l0, bias_hh_l0, rnn.norm.weight, .bias
//   actor:  act.mlp.fc.{0,2,3,5}.{weight,bias}, then per head: act.action_outs.i.logits_net.{weight,bias} (MultiDiscrete heads) and
//           act.action_outs.i.net.{weight [2, 128], bias} (munition heads)
//   critic: mlp.fc.{0,2,3,5}.{weight,bias}, value_out.weight [1, 128], value_out.bias
// A MAPPO handle (ac_policy_mappo_create) has the same blobs, the critic's input width being cent_obs_dim (feature_norm and fc.0.weight
// [128, cent_obs_dim]), and packs each network in the wide form (policy_kernel.hpp, WideLay).
#pragma once

struct ac_policy_s {
  int device;
  ac_policy_config_t cfg;
  int np;                                // pieces per value: 2 (AC_CTL_FAST) or 3 (AC_CTL_FP32)
  int64_t src_floats[2];                 // source blob lengths, actor / critic
  int wide = 0;                          // a MAPPO handle: the wide form, policy_wide_kernel
  int in_dim[2];                         // input width of the actor / critic (obs_dim; cent_obs_dim for the MAPPO critic)
  int64_t packed_n[2];                   // packed floats per network: Lay<np>::END, or WideLay<np>::END(kpad)
  pol::PackMap map[2];
  int cat_off[pol::MAXCAT], cat_cnt[pol::MAXCAT];
  float* d_packed[2] = {nullptr, nullptr};   // live weights
  float* d_stage[2] = {nullptr, nullptr};    // ac_policy_load_device packs here, then commits when the weights pass the checks
  int* d_flag = nullptr;                     // [2] 1 = the last device load of that network was refused
  bool loaded[2] = {false, false};
};

namespace {
int64_t policy_trunk_map(pol::PackMap& m, int obs_dim, int use_fn) {
  int64_t o = 0;
  auto take = [&](int64_t n) { const int64_t r = o; o += n; return (int)r; };
  m.obs_dim = obs_dim;
  m.f0g = use_fn ? take(obs_dim) : -1;
  m.f0b = use_fn ? take(obs_dim) : -1;
  m.w1 = take(128 * (int64_t)obs_dim); m.b1 = take(128); m.g1 = take(128); m.be1 = take(128);
  m.w2 = take(128 * 128); m.b2 = take(128); m.g2 = take(128); m.be2 = take(128);
  m.wih = take(384 * 128); m.whh = take(384 * 128); m.bih = take(384); m.bhh = take(384); m.gn = take(128); m.ben = take(128);
  m.w3 = take(128 * 128); m.b3 = take(128); m.g3 = take(128); m.be3 = take(128);
  m.w4 = take(128 * 128); m.b4 = take(128); m.g4 = take(128); m.be4 = take(128);
  for (int j = 0; j < pol::HCOLS; ++j) m.orow[j] = m.obias[j] = -1;
  return o;
}
// the refusals of ac_policy_create (out of scope), "" when the configuration is supported
std::string policy_config_error(const ac_policy_config_t* c, int maxobs = pol::MAXOBS) {
  if (c->activation_id != 1) return "unsupported activation_id (only 1, ReLU)";
  if (c->hidden_size[0] != 128 || c->hidden_size[1] != 128 || c->act_hidden_size[0] != 128 || c->act_hidden_size[1] != 128)
    return "unsupported hidden sizes (only \"128 128\" for hidden_size and act_hidden_size)";
  if (!c->use_recurrent_policy) return "unsupported use_recurrent_policy=False (the kernel is the recurrent policy)";
  if (c->recurrent_hidden_size != 128) return "unsupported recurrent_hidden_size (only 128)";
  if (c->recurrent_hidden_layers != 1) return "unsupported recurrent_hidden_layers (only 1)";
  if (c->obs_dim < 1 || c->obs_dim > maxobs) return "unsupported obs_dim (1 .. " + std::to_string(maxobs) + ")";
  if (c->single_shoot) return "unsupported action space Tuple(MultiDiscrete, Discrete(2)) (the single-shoot head)";
  if (c->n_cat < 1 || c->n_cat > pol::MAXCAT) return "unsupported number of MultiDiscrete heads (1 .. 8)";
  int tot = 0;
  for (int i = 0; i < c->n_cat; ++i) {
    if (c->nvec[i] < 1) return "MultiDiscrete nvec entries must be >= 1";
    tot += c->nvec[i];
  }
  if (tot > pol::MAXLOGITS) return "unsupported MultiDiscrete size (more than 160 logits in all)";
  if (c->n_shoot != 0 && c->n_shoot != pol::NSHOOT) return "unsupported munition part (only MultiDiscrete([2, 2, 2, 2]))";
  if (c->n_shoot && !c->use_prior) return "the munition heads need use_prior (their Beta prior comes from it)";
  if (c->n_shoot && c->obs_dim < 14) return "the munition heads' prior reads obs[:, 11] and obs[:, 13]: obs_dim must be >= 14";
  if (c->precision != AC_CTL_FAST && c->precision != AC_CTL_FP32) return "unknown precision (AC_CTL_FAST = 0, AC_CTL_FP32 = 1)";
  return "";
}
std::string mappo_config_error(const ac_policy_mappo_config_t* c) {
  const std::string e = policy_config_error(&c->base, pol::MAXWIDE);
  if (!e.empty()) return e;
  if (c->base.has_critic && (c->cent_obs_dim < 1 || c->cent_obs_dim > pol::MAXWIDE))
    return "unsupported cent_obs_dim (1 .. " + std::to_string(pol::MAXWIDE) + ")";
  return "";
}
void policy_maps(ac_policy_s* h) {
  const ac_policy_config_t& c = h->cfg;
  int64_t o = policy_trunk_map(h->map[0], c.obs_dim, c.use_feature_normalization);
  int col = 0;
  for (int i = 0; i < c.n_cat; ++i) {
    const int w = (int)o; o += 128 * (int64_t)c.nvec[i];
    const int b = (int)o; o += c.nvec[i];
    h->cat_off[i] = col; h->cat_cnt[i] = c.nvec[i];
    for (int j = 0; j < c.nvec[i]; ++j, ++col) { h->map[0].orow[col] = w + 128 * j; h->map[0].obias[col] = b + j; }
  }
  for (int s = 0; s < c.n_shoot; ++s) {
    const int w = (int)o; o += 256;
    const int b = (int)o; o += 2;
    for (int j = 0; j < 2; ++j) { h->map[0].orow[pol::MAXLOGITS + 2 * s + j] = w + 128 * j; h->map[0].obias[pol::MAXLOGITS + 2 * s + j] = b + j; }
  }
  h->src_floats[0] = o;
  o = policy_trunk_map(h->map[1], h->in_dim[1], c.use_feature_normalization);
  h->map[1].orow[0] = (int)o; o += 128;
  h->map[1].obias[0] = (int)o; o += 1;
  h->src_floats[1] = o;
  for (int k = 0; k < 2; ++k) {
    const int kpad = (h->in_dim[k] + 31) / 32 * 32;
    h->packed_n[k] = !h->wide ? (h->np == 3 ? pol::Lay<3>::END : pol::Lay<2>::END)
                              : (h->np == 3 ? pol::WideLay<3>::END(kpad) : pol::WideLay<2>::END(kpad));
  }
}
void policy_init(ac_policy_s* h, const ac_policy_config_t* cfg, int wide, int cent_dim) {
  h->cfg = *cfg; h->np = cfg->precision == AC_CTL_FP32 ? 3 : 2; h->wide = wide;
  h->in_dim[0] = cfg->obs_dim; h->in_dim[1] = wide ? cent_dim : cfg->obs_dim;
  policy_maps(h);
}
// packed float f of network k of h, either form (the host load path; the device one runs the same function in its kernels)
unsigned policy_pack_host(const ac_policy_s* h, int k, const float* src, int f) {
  if (h->wide) return h->np == 3 ? pol::policy_pack_wide<3>(src, h->map[k], f) : pol::policy_pack_wide<2>(src, h->map[k], f);
  return h->np == 3 ? pol::policy_pack_one<3>(src, h->map[k], f) : pol::policy_pack_one<2>(src, h->map[k], f);
}
// finite, and below fp16's largest finite value in the fast form (two fp16 pieces cannot hold more)
__host__ __device__ inline bool policy_weight_ok(float v, int np) { return v == v && fabsf(v) < (np == 2 ? 65504.0f : INFINITY); }
}  // namespace

template <int NP>
__global__ void policy_pack_kernel(const float* __restrict__ src, int64_t nsrc, float* __restrict__ dst, int* __restrict__ flag, pol::PackMap m) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nsrc && !policy_weight_ok(src[i], NP)) atomicOr(flag, 1);
  if (i < pol::Lay<NP>::END) reinterpret_cast<unsigned*>(dst)[i] = pol::policy_pack_one<NP>(src, m, (int)i);
}
template <int NP>
__global__ void policy_pack_wide_kernel(const float* __restrict__ src, int64_t nsrc, float* __restrict__ dst, int64_t ndst, int* __restrict__ flag,
                                        pol::PackMap m) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nsrc && !policy_weight_ok(src[i], NP)) atomicOr(flag, 1);
  if (i < ndst) reinterpret_cast<unsigned*>(dst)[i] = pol::policy_pack_wide<NP>(src, m, (int)i);
}
// stage -> live when the flag is clear (one launch: the refusal needs no host round trip)
__global__ void policy_commit_kernel(const float4* __restrict__ stage, float4* __restrict__ live, int64_t n4, const int* __restrict__ flag) {
  if (*flag) return;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) live[i] = stage[i];
}

extern "C" {
int ac_policy_blob_floats(const ac_policy_config_t* cfg, int64_t* actor_floats, int64_t* critic_floats) {
  if (!cfg || !actor_floats || !critic_floats) return fail("ac_policy_blob_floats: null argument");
  const std::string e = policy_config_error(cfg);
  if (!e.empty()) return fail("ac_policy: " + e);
  ac_policy_s tmp;
  policy_init(&tmp, cfg, 0, 0);
  *actor_floats = tmp.src_floats[0]; *critic_floats = tmp.src_floats[1];
  return 0;
}
int ac_policy_mappo_blob_floats(const ac_policy_mappo_config_t* cfg, int64_t* actor_floats, int64_t* critic_floats) {
  if (!cfg || !actor_floats || !critic_floats) return fail("ac_policy_mappo_blob_floats: null argument");
  const std::string e = mappo_config_error(cfg);
  if (!e.empty()) return fail("ac_policy: " + e);
  ac_policy_s tmp;
  policy_init(&tmp, &cfg->base, 1, cfg->cent_obs_dim);
  *actor_floats = tmp.src_floats[0]; *critic_floats = tmp.src_floats[1];
  return 0;
}
}  // extern "C"
namespace {
int policy_create(int32_t device_id, const ac_policy_config_t* cfg, int wide, int cent_dim, ac_policy_t** out) {
  int ndev = 0;
  HIP_OK(hipGetDeviceCount(&ndev));
  if (device_id < 0 || device_id >= ndev) return fail("ac_policy_create: no such HIP device");
  HIP_OK(hipSetDevice(device_id));
  ac_policy_s* h = new ac_policy_s();
  h->device = device_id;
  policy_init(h, cfg, wide, cent_dim);
  hipError_t err = hipSuccess;
  for (int k = 0; k < 2 && err == hipSuccess; ++k) {
    if (k == 1 && !cfg->has_critic) break;
    err = hipMalloc(&h->d_packed[k], sizeof(float) * h->packed_n[k]);
    if (err == hipSuccess) err = hipMalloc(&h->d_stage[k], sizeof(float) * h->packed_n[k]);
  }
  if (err == hipSuccess) err = hipMalloc(&h->d_flag, 2 * sizeof(int));
  if (err == hipSuccess) err = hipMemset(h->d_flag, 0, 2 * sizeof(int));
  if (err != hipSuccess) {
    for (int k = 0; k < 2; ++k) { if (h->d_packed[k]) (void)hipFree(h->d_packed[k]); if (h->d_stage[k]) (void)hipFree(h->d_stage[k]); }
    if (h->d_flag) (void)hipFree(h->d_flag);
    delete h;
    return fail(std::string("ac_policy_create: ") + hipGetErrorString(err));
  }
  *out = h;
  return 0;
}
}  // namespace
extern "C" {
int ac_policy_create(int32_t device_id, const ac_policy_config_t* cfg, ac_policy_t** out) {
  if (!cfg || !out) return fail("ac_policy_create: null argument");
  *out = nullptr;
  const std::string e = policy_config_error(cfg);
  if (!e.empty()) return fail("ac_policy: " + e);
  return policy_create(device_id, cfg, 0, 0, out);
}
int ac_policy_mappo_create(int32_t device_id, const ac_policy_mappo_config_t* cfg, ac_policy_t** out) {
  if (!cfg || !out) return fail("ac_policy_mappo_create: null argument");
  *out = nullptr;
  const std::string e = mappo_config_error(cfg);
  if (!e.empty()) return fail("ac_policy: " + e);
  return policy_create(device_id, &cfg->base, 1, cfg->cent_obs_dim, out);
}
int ac_policy_destroy(ac_policy_t* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  for (int k = 0; k < 2; ++k) { if (h->d_packed[k]) (void)hipFree(h->d_packed[k]); if (h->d_stage[k]) (void)hipFree(h->d_stage[k]); }
  if (h->d_flag) (void)hipFree(h->d_flag);
  delete h;
  return 0;
}
// host blobs: checked first, so that a refused load leaves the previous weights in place
int ac_policy_load(ac_policy_t* h, const float* actor, int64_t n_actor, const float* critic, int64_t n_critic) {
  if (!h || !actor) return fail("ac_policy_load: null argument");
  if (critic && !h->cfg.has_critic) return fail("ac_policy_load: the policy was created without a critic");
  const float* src[2] = {actor, critic};
  const int64_t ns[2] = {n_actor, n_critic};
  for (int k = 0; k < 2; ++k) {
    if (!src[k]) continue;
    if (ns[k] != h->src_floats[k])
      return fail(std::string("ac_policy_load: expected ") + std::to_string(h->src_floats[k]) + " floats for the " + (k ? "critic" : "actor") +
                  ", got " + std::to_string(ns[k]));
    for (int64_t i = 0; i < ns[k]; ++i)
      if (!policy_weight_ok(src[k][i], h->np))
        return fail(std::string("ac_policy_load: ") + (k ? "critic" : "actor") + " weight " + std::to_string(i) + " is " +
                    (src[k][i] == src[k][i] && std::isfinite(src[k][i]) ? "too large for the fast form's fp16 pieces (|w| >= 65504)" : "not finite"));
  }
  HIP_OK(hipSetDevice(h->device));
  for (int k = 0; k < 2; ++k) {
    if (!src[k]) continue;
    std::vector<unsigned> e((size_t)h->packed_n[k]);
    for (int64_t f = 0; f < h->packed_n[k]; ++f) e[f] = policy_pack_host(h, k, src[k], (int)f);
    HIP_OK(hipMemcpy(h->d_packed[k], e.data(), sizeof(float) * e.size(), hipMemcpyHostToDevice));
    h->loaded[k] = true;
  }
  return 0;
}
// device blobs, ordered on `stream`: checked and packed by one kernel into a staging copy, which a second one commits when the check passed
int ac_policy_load_device(ac_policy_t* h, void* stream, const float* d_actor, int64_t n_actor, const float* d_critic, int64_t n_critic) {
  if (!h || !d_actor) return fail("ac_policy_load_device: null argument");
  if (d_critic && !h->cfg.has_critic) return fail("ac_policy_load_device: the policy was created without a critic");
  const float* src[2] = {d_actor, d_critic};
  const int64_t ns[2] = {n_actor, n_critic};
  for (int k = 0; k < 2; ++k)
    if (src[k] && ns[k] != h->src_floats[k])
      return fail(std::string("ac_policy_load_device: expected ") + std::to_string(h->src_floats[k]) + " floats for the " + (k ? "critic" : "actor"));
  HIP_OK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  for (int k = 0; k < 2; ++k) {
    if (!src[k]) continue;
    HIP_OK(hipMemsetAsync(h->d_flag + k, 0, sizeof(int), s));
    const int64_t nt = std::max<int64_t>(h->packed_n[k], ns[k]);
    const dim3 g((unsigned)((nt + 255) / 256));
    if (h->wide && h->np == 3)
      hipLaunchKernelGGL(policy_pack_wide_kernel<3>, g, dim3(256), 0, s, src[k], ns[k], h->d_stage[k], h->packed_n[k], h->d_flag + k, h->map[k]);
    else if (h->wide)
      hipLaunchKernelGGL(policy_pack_wide_kernel<2>, g, dim3(256), 0, s, src[k], ns[k], h->d_stage[k], h->packed_n[k], h->d_flag + k, h->map[k]);
    else if (h->np == 3) hipLaunchKernelGGL(policy_pack_kernel<3>, g, dim3(256), 0, s, src[k], ns[k], h->d_stage[k], h->d_flag + k, h->map[k]);
    else hipLaunchKernelGGL(policy_pack_kernel<2>, g, dim3(256), 0, s, src[k], ns[k], h->d_stage[k], h->d_flag + k, h->map[k]);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(policy_commit_kernel, dim3(256), dim3(256), 0, s, reinterpret_cast<const float4*>(h->d_stage[k]),
                       reinterpret_cast<float4*>(h->d_packed[k]), h->packed_n[k] / 4, h->d_flag + k);
    HIP_OK(hipGetLastError());
    h->loaded[k] = true;   // (a refused first load leaves zero weights: ac_policy_load_refused reports it)
  }
  return 0;
}
// whether the last ac_policy_load_device of the actor / critic was refused (waits for `stream`)
int ac_policy_load_refused(ac_policy_t* h, void* stream, int32_t* actor_refused, int32_t* critic_refused) {
  if (!h || !actor_refused || !critic_refused) return fail("ac_policy_load_refused: null argument");
  HIP_OK(hipSetDevice(h->device));
  int f[2] = {0, 0};
  HIP_OK(hipMemcpyAsync(f, h->d_flag, sizeof(f), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  *actor_refused = f[0]; *critic_refused = f[1];
  return 0;
}
int ac_policy_packed(ac_policy_t* h, int32_t net, void** d_ptr, int64_t* floats) {
  if (!h || !d_ptr || !floats || net < 0 || net > 1) return fail("ac_policy_packed: bad argument");
  *d_ptr = h->d_packed[net]; *floats = h->d_packed[net] ? h->packed_n[net] : 0;
  return 0;
}
}  // extern "C"
namespace {
// checks and the launch of one policy call, either form. actor = false: a critic-only launch (get_values). obs_compact: d_obs is a
// compact [n][obs_dim] array whatever the agent range says (the rollout collectors' buffer slot, either form). The critic reads the
// obs rows (the PPO form), or (the wide form) cent_mode's input: explicit rows d_cin + r * cent_dim, or each env's obs block.
int policy_launch(ac_policy_t* h, void* stream, const ac_policy_rows_t* rows, const std::string& what, bool actor, bool critic,
                  const float* d_obs, const float* d_cin, int32_t cent_mode, const float* d_rnn_actor, const float* d_rnn_critic,
                  const float* d_masks, int32_t deterministic, uint64_t seed, uint64_t counter, float* d_values, float* d_actions,
                  float* d_logp, float* d_rnn_actor_out, float* d_rnn_critic_out, int obs_compact = 0) {
  if (obs_compact && !actor) return fail(what + ": compact obs rows are for get_actions launches only");
  if (critic && !h->cfg.has_critic) return fail(what + ": the policy was created without a critic");
  if ((actor && !h->loaded[0]) || (critic && !h->loaded[1])) return fail(what + ": weights not loaded");
  if (rows->n < 0 || rows->n > (1 << 24)) return fail(what + ": n must be in 0 .. 2^24");
  if (rows->n == 0) return 0;
  const int nh = h->cfg.n_cat + h->cfg.n_shoot;
  int na = rows->na, A = rows->A;
  if (na == 0) { na = 1; A = 1; }
  if (na < 1 || A < na || rows->a0 < 0 || rows->a0 + na > A || rows->n % na) return fail(what + ": bad agent range");
  if (actor && rows->act_stride < nh) return fail(what + ": act_stride is smaller than the number of heads");
  pol::Wide x{};
  if (h->wide) {
    x.dim[0] = h->in_dim[0]; x.dim[1] = h->in_dim[1];
    x.kpad[0] = (h->in_dim[0] + 31) / 32 * 32; x.kpad[1] = (h->in_dim[1] + 31) / 32 * 32;
    if (critic && cent_mode == AC_CENT_ENV_SHARE) {
      if (rows->na <= 0) return fail(what + ": the env-share critic input needs an agent range (na > 0)");
      if ((int64_t)rows->A * h->in_dim[0] != h->in_dim[1])
        return fail(what + ": env share needs cent_obs_dim = A * obs_dim (" + std::to_string(h->in_dim[1]) + " != " + std::to_string(rows->A) +
                    " * " + std::to_string(h->in_dim[0]) + ")");
      x.cin = d_obs; x.cna = na; x.cstride = (long long)rows->A * h->in_dim[0];
    } else if (critic) {
      if (cent_mode != AC_CENT_EXPLICIT) return fail(what + ": unknown cent_mode (AC_CENT_EXPLICIT = 0, AC_CENT_ENV_SHARE = 1)");
      if (!d_cin) return fail(what + ": the explicit critic input is NULL");
      x.cin = d_cin; x.cna = 1; x.cstride = h->in_dim[1];
    }
  }
  HIP_OK(hipSetDevice(h->device));
  pol::Args a{};
  a.W[0] = h->d_packed[0]; a.W[1] = h->d_packed[1];
  a.obs = d_obs; a.h_in[0] = d_rnn_actor; a.h_in[1] = d_rnn_critic; a.h_out[0] = d_rnn_actor_out; a.h_out[1] = d_rnn_critic_out;
  a.masks = d_masks; a.actions = d_actions; a.logp = d_logp; a.values = d_values;
  a.n = (int)rows->n; a.obs_dim = h->cfg.obs_dim; a.act_stride = rows->act_stride;
  a.na = na; a.A = A; a.a0 = rows->a0; a.obs_compact = obs_compact;
  a.n_cat = h->cfg.n_cat; a.n_shoot = h->cfg.n_shoot; a.use_fn = h->cfg.use_feature_normalization; a.deterministic = deterministic ? 1 : 0;
  for (int i = 0; i < pol::MAXCAT; ++i) { a.cat_off[i] = h->cat_off[i]; a.cat_cnt[i] = h->cat_cnt[i]; }
  a.seed = seed; a.counter = counter;
  x.net0 = actor ? 0 : 1;
  const dim3 g((unsigned)((rows->n + pol::R - 1) / pol::R), actor && critic ? 2 : 1);
  hipStream_t st = (hipStream_t)stream;
  if (h->wide && h->np == 3) hipLaunchKernelGGL(policy_wide_kernel<3>, g, dim3(512), 0, st, a, x);
  else if (h->wide) hipLaunchKernelGGL(policy_wide_kernel<2>, g, dim3(512), 0, st, a, x);
  else if (!actor && h->np == 3) hipLaunchKernelGGL(policy_values_kernel<3>, g, dim3(512), 0, st, a);
  else if (!actor) hipLaunchKernelGGL(policy_values_kernel<2>, g, dim3(512), 0, st, a);
  else if (h->np == 3) hipLaunchKernelGGL(policy_kernel<3>, g, dim3(512), 0, st, a);
  else hipLaunchKernelGGL(policy_kernel<2>, g, dim3(512), 0, st, a);
  HIP_OK(hipGetLastError());
  return 0;
}
}  // namespace
extern "C" {
int ac_policy_get_actions(ac_policy_t* h, void* stream, const ac_policy_rows_t* rows, const float* d_obs, const float* d_rnn_actor,
                          const float* d_rnn_critic, const float* d_masks, int32_t deterministic, uint64_t seed, uint64_t counter,
                          float* d_values, float* d_actions, float* d_logp, float* d_rnn_actor_out, float* d_rnn_critic_out) {
  if (!h || !rows || !d_obs || !d_rnn_actor || !d_masks || !d_actions || !d_logp || !d_rnn_actor_out)
    return fail("ac_policy_get_actions: null argument");
  if (h->wide) return fail("ac_policy_get_actions: a MAPPO handle (ac_policy_mappo_create): use ac_policy_get_actions_mappo");
  const bool critic = d_rnn_critic || d_values || d_rnn_critic_out;
  if (critic && !(d_rnn_critic && d_values && d_rnn_critic_out)) return fail("ac_policy_get_actions: the critic needs its state in, state out and values");
  return policy_launch(h, stream, rows, "ac_policy_get_actions", true, critic, d_obs, nullptr, AC_CENT_EXPLICIT, d_rnn_actor, d_rnn_critic,
                       d_masks, deterministic, seed, counter, d_values, d_actions, d_logp, d_rnn_actor_out, d_rnn_critic_out);
}
int ac_policy_get_actions_mappo(ac_policy_t* h, void* stream, const ac_policy_rows_t* rows, const float* d_obs, const float* d_cent_obs,
                                int32_t cent_mode, const float* d_rnn_actor, const float* d_rnn_critic, const float* d_masks,
                                int32_t deterministic, uint64_t seed, uint64_t counter, float* d_values, float* d_actions, float* d_logp,
                                float* d_rnn_actor_out, float* d_rnn_critic_out) {
  if (!h || !rows || !d_obs || !d_rnn_actor || !d_masks || !d_actions || !d_logp || !d_rnn_actor_out)
    return fail("ac_policy_get_actions_mappo: null argument");
  if (!h->wide) return fail("ac_policy_get_actions_mappo: a PPO handle (ac_policy_create): use ac_policy_get_actions");
  const bool critic = d_rnn_critic || d_values || d_rnn_critic_out;
  if (critic && !(d_rnn_critic && d_values && d_rnn_critic_out))
    return fail("ac_policy_get_actions_mappo: the critic needs its state in, state out and values");
  return policy_launch(h, stream, rows, "ac_policy_get_actions_mappo", true, critic, d_obs, d_cent_obs, cent_mode, d_rnn_actor, d_rnn_critic,
                       d_masks, deterministic, seed, counter, d_values, d_actions, d_logp, d_rnn_actor_out, d_rnn_critic_out);
}
int ac_policy_get_values(ac_policy_t* h, void* stream, const ac_policy_rows_t* rows, const float* d_in, int32_t cent_mode,
                         const float* d_rnn_critic, const float* d_masks, float* d_values, float* d_rnn_critic_out) {
  if (!h || !rows || !d_in || !d_rnn_critic || !d_masks || !d_values || !d_rnn_critic_out) return fail("ac_policy_get_values: null argument");
  if (!h->wide && cent_mode != AC_CENT_EXPLICIT) return fail("ac_policy_get_values: a PPO handle's critic reads its own obs rows (AC_CENT_EXPLICIT)");
  // the PPO form reads d_in as obs rows (agent-range indexing as get_actions); the wide form as cent_mode's input (env share: the obs buffer)
  return policy_launch(h, stream, rows, "ac_policy_get_values", false, true, d_in, d_in, cent_mode, nullptr, d_rnn_critic, d_masks, 0, 0, 0,
                       d_values, nullptr, nullptr, nullptr, d_rnn_critic_out);
}
int ac_policy_draw_host(uint64_t seed, uint64_t counter, int64_t row0, int64_t nrows, int32_t head, float* out) {
  if (!out || nrows < 0 || head < 0 || head > 255) return fail("ac_policy_draw_host: bad argument");
  for (int64_t i = 0; i < nrows; ++i) out[i] = pol::policy_uniform(seed, counter, row0 + i, head);
  return 0;
}
}  // extern "C"
