// A pool of actor networks on the device (include/aircombat.h, ac_policy_pool_*): the self-play opponents of the reference's runners
// (runner/selfplay_jsbsim_runner.py, share_jsbsim_runner.py: n_choose_opponents actors over np.array_split env ranges) as one
// array of packed actors in HBM, an assignment of envs to members, and one launch that acts for every assigned row with its member's
// weights (policy_pool_kernel / policy_pool_wide_kernel, the pool form of policy_body). Included by aircombat.hip after policy_host.hpp.
//
// Members are packed exactly as a DevicePolicy (Lay<NP>) or DeviceMAPPOPolicy (WideLay<NP>) packs its actor, by the same packers and
// with the same refusals. The plan (ac_policy_pool_assign) is a stable counting sort of the call's rows by member, then a list of tiles
// of at most 32 rows of one member each: pool_plan_phase, one __host__ __device__ function run by one workgroup on the device and by
// ac_policy_pool_plan_host on the host.
//
// A sided assignment (ac_policy_pool_assign_sides, the league's) is the same plan over the 2 E half-envs of A / 2 rows each: half-env
// 2 e + side, row k, is call row e * A + side * A / 2 + k of the whole-range call, so order[] holds call rows as before and neither the
// plan kernel nor the act kernels change; only the bookkeeping around them does (pool_units / pool_unit_rows).
#pragma once

namespace pol {
constexpr int PLAN_T = 256;   // workers of the plan (threads of its one workgroup; the host twin loops over them)
struct Plan {
  const int* members;         // [E]: member of each env, -1 = not acted for
  int E, na, cap;
  const int* loaded;          // [cap]: 1 = the member holds weights
  int* cnt;                   // [cap * PLAN_T + 1]: envs of member m in worker t's block (member-major), then their exclusive prefix
  int* part;                  // [PLAN_T + 1]: the prefix of worker t's segment of cnt
  int* bad;                   // [PLAN_T]: first bad env of worker t's block (E: none)
  int* tstart;                // [cap + 1]: tiles of member m, then the first tile of member m
  int4* tiles;                // [<= ceil(E * na / 32) + min(cap, E)]: {member, p0, p1, 0}
  int* order;                 // [E * na]: the call rows by member; row r of env e is e * na + r % na
  int* ntiles;                // [1]
  int* bad_env;               // [1]: the first env whose member is out of range or not loaded (-1: none); such envs are not acted for
};
// phase `phase` (0 .. PLAN_PHASES - 1) of worker t; every worker finishes a phase before any starts the next
constexpr int PLAN_PHASES = 8;
__host__ __device__ inline int pmin(int x, int y) { return x < y ? x : y; }
__host__ __device__ inline void pool_plan_phase(const Plan& p, int phase, int t) {
  constexpr int T = PLAN_T;
  const int B = (p.E + T - 1) / T, e0 = pmin(p.E, t * B), e1 = pmin(p.E, e0 + B);   // worker t's block of envs
  auto valid = [&](int m) { return m >= 0 && m < p.cap && p.loaded[m] != 0; };
  switch (phase) {
  case 0: {   // count the block's envs per member, note its first bad env
    for (int m = 0; m < p.cap; ++m) p.cnt[m * T + t] = 0;
    int bad = p.E;
    for (int e = e0; e < e1; ++e) {
      const int m = p.members[e];
      if (valid(m)) ++p.cnt[m * T + t];
      else if (m != -1 && bad == p.E) bad = e;
    }
    p.bad[t] = bad;
    break;
  }
  case 1: {   // worker t's segment [t cap, (t + 1) cap) of the member-major counts: its sum
    int s = 0;
    for (int i = t * p.cap; i < (t + 1) * p.cap; ++i) s += p.cnt[i];
    p.part[t] = s;
    break;
  }
  case 2:
    if (t == 0) {
      int s = 0, bad = p.E;
      for (int i = 0; i < T; ++i) { const int v = p.part[i]; p.part[i] = s; s += v; bad = pmin(bad, p.bad[i]); }
      p.part[T] = s;
      *p.bad_env = bad < p.E ? bad : -1;
    }
    break;
  case 3: {   // the exclusive prefix of the counts, in env units: member m's envs start at cnt[m T], worker t's of them at cnt[m T + t]
    int s = p.part[t];
    for (int i = t * p.cap; i < (t + 1) * p.cap; ++i) { const int v = p.cnt[i]; p.cnt[i] = s; s += v; }
    if (t == 0) p.cnt[p.cap * T] = p.part[T];
    break;
  }
  case 4:   // tiles of each member
    for (int m = t; m < p.cap; m += T) p.tstart[m] = ((p.cnt[(m + 1) * T] - p.cnt[m * T]) * p.na + 31) / 32;
    break;
  case 5:
    if (t == 0) {
      int s = 0;
      for (int m = 0; m < p.cap; ++m) { const int v = p.tstart[m]; p.tstart[m] = s; s += v; }
      p.tstart[p.cap] = s;
      *p.ntiles = s;
    }
    break;
  case 6:     // the tiles, member-major: member m's rows are positions na cnt[m T] .. na cnt[(m + 1) T] - 1 of order
    for (int m = t; m < p.cap; m += T) {
      const int r0 = p.cnt[m * T] * p.na, r1 = p.cnt[(m + 1) * T] * p.na;
      for (int k = p.tstart[m]; k < p.tstart[m + 1]; ++k) {
        const int q0 = r0 + 32 * (k - p.tstart[m]);
        p.tiles[k] = make_int4(m, q0, pmin(q0 + 32, r1), 0);
      }
    }
    break;
  case 7:     // the scatter, in env order within each worker's block (so stable): worker t owns its cnt[m T + t]
    for (int e = e0; e < e1; ++e) {
      const int m = p.members[e];
      if (!valid(m)) continue;
      const int pos = p.cnt[m * T + t]++;
      for (int r = 0; r < p.na; ++r) p.order[pos * p.na + r] = e * p.na + r;
    }
    break;
  }
}
}  // namespace pol

__global__ __launch_bounds__(pol::PLAN_T) void policy_pool_plan_kernel(pol::Plan p) {
  for (int ph = 0; ph < pol::PLAN_PHASES; ++ph) {
    pol::pool_plan_phase(p, ph, threadIdx.x);
    __syncthreads();
  }
}
// stage -> member slot when the flag is clear, and the member marked loaded
__global__ void policy_pool_commit_kernel(const float4* __restrict__ stage, float4* __restrict__ live, int64_t n4, const int* __restrict__ flag,
                                          int* __restrict__ loaded) {
  if (*flag) return;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) live[i] = stage[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) *loaded = 1;
}

struct ac_policy_pool_s {
  int device;
  ac_policy_s net;                        // the configuration, blob map and packed size of one member (no device buffers of its own)
  int form, capacity;
  float* d_w = nullptr;                   // [capacity][packed_n[0]]
  float* d_stage = nullptr;               // ac_policy_pool_load_device packs here
  int* d_flag = nullptr;                  // [1] the last device load was refused
  int* d_loaded = nullptr;                // [capacity]
  int xcd = 1;                            // tile order (pol::Pool::xcd): a member's tiles on one XCD, measured faster
  // the plan, rebuilt by assign (and by act when a call's agent count differs from the plan's)
  int* d_members = nullptr;               // [E] the assignment (a copy)
  int* d_scratch = nullptr;               // cnt, part, bad, tstart, ntiles, bad_env
  int4* d_tiles = nullptr;
  int* d_order = nullptr;
  int64_t E = -1, cap_E = 0, cap_rows = 0, cap_tiles = 0;
  int na = 0;
  // a sided plan (ac_policy_pool_assign_sides): d_members is [E][2] and the plan runs over the 2 E half-envs of na / 2 rows, half-env
  // 2 e + side, row k being call row e * na + side * na / 2 + k of the whole-range call; E and na stay the env's
  int sided = 0;
  uint64_t plan_gen = 0;                  // bumped by every assign: a holder of a snapshot (the league) tells a later re-assignment
  int ntiles_host = -1;                   // the tile count read back by ac_policy_pool_check (-1: not read for this plan)
};

namespace {
const char* pool_form_name(int f) { return f == AC_POOL_MAPPO ? "mappo" : "ppo"; }
std::string pool_config_error(const ac_policy_config_t* cfg, int32_t form, int32_t capacity) {
  if (form != AC_POOL_PPO && form != AC_POOL_MAPPO) return "unknown form (AC_POOL_PPO = 0, AC_POOL_MAPPO = 1)";
  if (capacity < 1) return "capacity must be >= 1";
  return policy_config_error(cfg, form == AC_POOL_MAPPO ? pol::MAXWIDE : pol::MAXOBS);
}
void pool_init(ac_policy_pool_s* p, const ac_policy_config_t* cfg, int32_t form, int32_t capacity) {
  ac_policy_config_t c = *cfg;
  c.has_critic = 0;
  policy_init(&p->net, &c, form == AC_POOL_MAPPO, c.obs_dim);
  p->form = form; p->capacity = capacity;
}
// the actor's part of two configurations that must agree for a member copy: everything the packed actor depends on
std::string pool_actor_mismatch(const ac_policy_config_t* a, int fa, const ac_policy_config_t* b, int fb) {
  if (fa != fb) return std::string("form differs (pool ") + pool_form_name(fa) + ", policy " + pool_form_name(fb) + ")";
  if (a->precision != b->precision) return "precision differs";
  bool same = a->obs_dim == b->obs_dim && a->n_cat == b->n_cat && a->n_shoot == b->n_shoot && a->single_shoot == b->single_shoot &&
              a->use_feature_normalization == b->use_feature_normalization && a->use_prior == b->use_prior &&
              a->activation_id == b->activation_id && a->use_recurrent_policy == b->use_recurrent_policy &&
              a->recurrent_hidden_size == b->recurrent_hidden_size && a->recurrent_hidden_layers == b->recurrent_hidden_layers;
  for (int i = 0; i < 2; ++i) same = same && a->hidden_size[i] == b->hidden_size[i] && a->act_hidden_size[i] == b->act_hidden_size[i];
  for (int i = 0; i < a->n_cat && i < 8; ++i) same = same && a->nvec[i] == b->nvec[i];
  return same ? "" : "configuration differs (obs_dim, heads or network fields)";
}
pol::Plan pool_plan_args(const int* members, int64_t E, int na, int cap, const int* loaded, int* scratch, int4* tiles, int* order) {
  pol::Plan p{};
  p.members = members; p.E = (int)E; p.na = na; p.cap = cap; p.loaded = loaded;
  p.cnt = scratch;
  p.part = p.cnt + (int64_t)cap * pol::PLAN_T + 1;
  p.bad = p.part + pol::PLAN_T + 1;
  p.tstart = p.bad + pol::PLAN_T;
  p.ntiles = p.tstart + cap + 1;
  p.bad_env = p.ntiles + 1;
  p.tiles = tiles; p.order = order;
  return p;
}
int64_t pool_scratch_ints(int cap) { return (int64_t)cap * pol::PLAN_T + 1 + pol::PLAN_T + 1 + pol::PLAN_T + cap + 1 + 2; }
int64_t pool_max_tiles(int64_t E, int na, int cap) { return (E * na + 31) / 32 + std::min<int64_t>(cap, E); }
// the units of the plan and the rows of each: the envs of na rows, or the half-envs of na / 2 rows of a sided plan
int64_t pool_units(const ac_policy_pool_s* p) { return p->sided ? 2 * p->E : p->E; }
int pool_unit_rows(const ac_policy_pool_s* p, int na) { return p->sided ? na / 2 : na; }
// (re)build the plan for E envs of na rows on `stream` from the assignment in p->d_members
int pool_build_plan(ac_policy_pool_s* p, hipStream_t s, int na) {
  const int64_t units = pool_units(p);
  const int ur = pool_unit_rows(p, na);
  const int64_t rows = p->E * na, mt = pool_max_tiles(units, ur, p->capacity);
  if (rows > p->cap_rows) {
    if (p->d_order) HIP_OK(hipFree(p->d_order));
    p->d_order = nullptr; p->cap_rows = 0;
    HIP_OK(hipMalloc(&p->d_order, sizeof(int) * std::max<int64_t>(rows, 1)));
    p->cap_rows = rows;
  }
  if (mt > p->cap_tiles) {
    if (p->d_tiles) HIP_OK(hipFree(p->d_tiles));
    p->d_tiles = nullptr; p->cap_tiles = 0;
    HIP_OK(hipMalloc(&p->d_tiles, sizeof(int4) * std::max<int64_t>(mt, 1)));
    p->cap_tiles = mt;
  }
  const pol::Plan a = pool_plan_args(p->d_members, units, ur, p->capacity, p->d_loaded, p->d_scratch, p->d_tiles, p->d_order);
  hipLaunchKernelGGL(policy_pool_plan_kernel, dim3(1), dim3(pol::PLAN_T), 0, s, a);
  HIP_OK(hipGetLastError());
  p->na = na;
  p->ntiles_host = -1;
  p->plan_gen += 1;
  return 0;
}
// the copy of an assignment of `n` ints, its plan on `s`: the tail of both assigns
int pool_assign(ac_policy_pool_s* p, hipStream_t s, const int32_t* d_members, int64_t n, int64_t E, int na, int sided) {
  if (n > p->cap_E) {
    if (p->d_members) HIP_OK(hipFree(p->d_members));
    p->d_members = nullptr; p->cap_E = 0; p->E = -1;
    HIP_OK(hipMalloc(&p->d_members, sizeof(int) * n));
    p->cap_E = n;
  }
  HIP_OK(hipMemcpyAsync(p->d_members, d_members, sizeof(int) * n, hipMemcpyDeviceToDevice, s));
  p->E = E; p->sided = sided;
  return pool_build_plan(p, s, na);
}
}  // namespace

extern "C" {
int ac_policy_pool_member_floats(const ac_policy_config_t* cfg, int32_t form, int32_t capacity, int64_t* src_floats, int64_t* packed_floats) {
  if (!cfg || !src_floats || !packed_floats) return fail("ac_policy_pool_member_floats: null argument");
  const std::string e = pool_config_error(cfg, form, capacity);
  if (!e.empty()) return fail("ac_policy_pool: " + e);
  ac_policy_pool_s tmp;
  pool_init(&tmp, cfg, form, capacity);
  *src_floats = tmp.net.src_floats[0]; *packed_floats = tmp.net.packed_n[0];
  return 0;
}
int ac_policy_pool_compatible(const ac_policy_config_t* pool_cfg, int32_t pool_form, const ac_policy_config_t* cfg, int32_t form) {
  if (!pool_cfg || !cfg) return fail("ac_policy_pool_compatible: null argument");
  const std::string e = pool_actor_mismatch(pool_cfg, pool_form, cfg, form);
  return e.empty() ? 0 : fail("ac_policy_pool_copy_from: " + e);
}
int ac_policy_pool_create(int32_t device_id, const ac_policy_config_t* cfg, int32_t form, int32_t capacity, ac_policy_pool_t** out) {
  if (!cfg || !out) return fail("ac_policy_pool_create: null argument");
  *out = nullptr;
  const std::string e = pool_config_error(cfg, form, capacity);
  if (!e.empty()) return fail("ac_policy_pool: " + e);
  int ndev = 0;
  HIP_OK(hipGetDeviceCount(&ndev));
  if (device_id < 0 || device_id >= ndev) return fail("ac_policy_pool_create: no such HIP device");
  HIP_OK(hipSetDevice(device_id));
  ac_policy_pool_s* p = new ac_policy_pool_s();
  p->device = device_id;
  pool_init(p, cfg, form, capacity);
  const int64_t per = p->net.packed_n[0];
  hipError_t err = hipMalloc(&p->d_w, sizeof(float) * per * capacity);
  if (err == hipSuccess) err = hipMemset(p->d_w, 0, sizeof(float) * per * capacity);
  if (err == hipSuccess) err = hipMalloc(&p->d_stage, sizeof(float) * per);
  if (err == hipSuccess) err = hipMalloc(&p->d_flag, sizeof(int));
  if (err == hipSuccess) err = hipMemset(p->d_flag, 0, sizeof(int));
  if (err == hipSuccess) err = hipMalloc(&p->d_loaded, sizeof(int) * capacity);
  if (err == hipSuccess) err = hipMemset(p->d_loaded, 0, sizeof(int) * capacity);
  if (err == hipSuccess) err = hipMalloc(&p->d_scratch, sizeof(int) * pool_scratch_ints(capacity));
  if (err != hipSuccess) {
    for (void* q : {(void*)p->d_w, (void*)p->d_stage, (void*)p->d_flag, (void*)p->d_loaded, (void*)p->d_scratch}) if (q) (void)hipFree(q);
    delete p;
    return fail(std::string("ac_policy_pool_create: ") + hipGetErrorString(err));
  }
  *out = p;
  return 0;
}
int ac_policy_pool_destroy(ac_policy_pool_t* p) {
  if (!p) return 0;
  (void)hipSetDevice(p->device);
  (void)hipDeviceSynchronize();
  for (void* q : {(void*)p->d_w, (void*)p->d_stage, (void*)p->d_flag, (void*)p->d_loaded, (void*)p->d_scratch, (void*)p->d_members,
                  (void*)p->d_tiles, (void*)p->d_order})
    if (q) (void)hipFree(q);
  delete p;
  return 0;
}
// a host blob into member `member`: checked first, so that a refused load keeps the member's previous weights
int ac_policy_pool_load(ac_policy_pool_t* p, int32_t member, const float* actor, int64_t n) {
  if (!p || !actor) return fail("ac_policy_pool_load: null argument");
  if (member < 0 || member >= p->capacity) return fail("ac_policy_pool_load: member out of range");
  if (n != p->net.src_floats[0]) return fail("ac_policy_pool_load: expected " + std::to_string(p->net.src_floats[0]) + " floats, got " + std::to_string(n));
  for (int64_t i = 0; i < n; ++i)
    if (!policy_weight_ok(actor[i], p->net.np))
      return fail("ac_policy_pool_load: actor weight " + std::to_string(i) + " is " +
                  (std::isfinite(actor[i]) ? "too large for the fast form's fp16 pieces (|w| >= 65504)" : "not finite"));
  HIP_OK(hipSetDevice(p->device));
  const int64_t per = p->net.packed_n[0];
  std::vector<unsigned> e((size_t)per);
  for (int64_t f = 0; f < per; ++f) e[f] = policy_pack_host(&p->net, 0, actor, (int)f);
  HIP_OK(hipMemcpy(p->d_w + member * per, e.data(), sizeof(float) * per, hipMemcpyHostToDevice));
  const int one = 1;
  HIP_OK(hipMemcpy(p->d_loaded + member, &one, sizeof(int), hipMemcpyHostToDevice));
  return 0;
}
// a device blob into member `member`, ordered on `stream`: checked and packed into the staging copy, committed when the check passed
int ac_policy_pool_load_device(ac_policy_pool_t* p, void* stream, int32_t member, const float* d_actor, int64_t n) {
  if (!p || !d_actor) return fail("ac_policy_pool_load_device: null argument");
  if (member < 0 || member >= p->capacity) return fail("ac_policy_pool_load_device: member out of range");
  if (n != p->net.src_floats[0]) return fail("ac_policy_pool_load_device: expected " + std::to_string(p->net.src_floats[0]) + " floats");
  HIP_OK(hipSetDevice(p->device));
  hipStream_t s = (hipStream_t)stream;
  const int64_t per = p->net.packed_n[0];
  HIP_OK(hipMemsetAsync(p->d_flag, 0, sizeof(int), s));
  const dim3 g((unsigned)((std::max<int64_t>(per, n) + 255) / 256));
  const pol::PackMap& m = p->net.map[0];
  if (p->net.wide && p->net.np == 3) hipLaunchKernelGGL(policy_pack_wide_kernel<3>, g, dim3(256), 0, s, d_actor, n, p->d_stage, per, p->d_flag, m);
  else if (p->net.wide) hipLaunchKernelGGL(policy_pack_wide_kernel<2>, g, dim3(256), 0, s, d_actor, n, p->d_stage, per, p->d_flag, m);
  else if (p->net.np == 3) hipLaunchKernelGGL(policy_pack_kernel<3>, g, dim3(256), 0, s, d_actor, n, p->d_stage, p->d_flag, m);
  else hipLaunchKernelGGL(policy_pack_kernel<2>, g, dim3(256), 0, s, d_actor, n, p->d_stage, p->d_flag, m);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(policy_pool_commit_kernel, dim3(256), dim3(256), 0, s, reinterpret_cast<const float4*>(p->d_stage),
                     reinterpret_cast<float4*>(p->d_w + member * per), per / 4, p->d_flag, p->d_loaded + member);
  HIP_OK(hipGetLastError());
  return 0;
}
int ac_policy_pool_load_refused(ac_policy_pool_t* p, void* stream, int32_t* refused) {
  if (!p || !refused) return fail("ac_policy_pool_load_refused: null argument");
  HIP_OK(hipSetDevice(p->device));
  int f = 0;
  HIP_OK(hipMemcpyAsync(&f, p->d_flag, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  *refused = f;
  return 0;
}
// a DevicePolicy's (DeviceMAPPOPolicy's) packed actor into member `member`, device to device on `stream`
int ac_policy_pool_copy_from(ac_policy_pool_t* p, void* stream, int32_t member, ac_policy_t* h) {
  if (!p || !h) return fail("ac_policy_pool_copy_from: null argument");
  if (member < 0 || member >= p->capacity) return fail("ac_policy_pool_copy_from: member out of range");
  const std::string e = pool_actor_mismatch(&p->net.cfg, p->form, &h->cfg, h->wide ? AC_POOL_MAPPO : AC_POOL_PPO);
  if (!e.empty()) return fail("ac_policy_pool_copy_from: " + e);
  if (h->device != p->device) return fail("ac_policy_pool_copy_from: the policy is on another device");
  if (!h->loaded[0]) return fail("ac_policy_pool_copy_from: the policy's actor is not loaded");
  const int64_t per = p->net.packed_n[0];
  if (h->packed_n[0] != per) return fail("ac_policy_pool_copy_from: packed sizes differ");
  HIP_OK(hipSetDevice(p->device));
  hipStream_t s = (hipStream_t)stream;
  HIP_OK(hipMemcpyAsync(p->d_w + member * per, h->d_packed[0], sizeof(float) * per, hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemsetD32Async((hipDeviceptr_t)(p->d_loaded + member), 1, 1, s));
  return 0;
}
int ac_policy_pool_packed(ac_policy_pool_t* p, int32_t member, void** d_ptr, int64_t* floats) {
  if (!p || !d_ptr || !floats || member < 0 || member >= p->capacity) return fail("ac_policy_pool_packed: bad argument");
  *d_ptr = p->d_w + member * p->net.packed_n[0]; *floats = p->net.packed_n[0];
  return 0;
}
int ac_policy_pool_set_tile_order(ac_policy_pool_t* p, int32_t xcd) {
  if (!p) return fail("ac_policy_pool_set_tile_order: null argument");
  p->xcd = xcd ? 1 : 0;
  return 0;
}
// the assignment of E envs (na rows each) to members, copied and planned on `stream`
int ac_policy_pool_assign(ac_policy_pool_t* p, void* stream, const int32_t* d_members, int64_t E, int32_t na) {
  if (!p || !d_members) return fail("ac_policy_pool_assign: null argument");
  if (E < 1 || na < 1 || E * na > (1 << 24)) return fail("ac_policy_pool_assign: E and na must be >= 1 with E * na <= 2^24");
  HIP_OK(hipSetDevice(p->device));
  return pool_assign(p, (hipStream_t)stream, d_members, E, E, na, 0);
}
// the sided assignment: members2 [E][2], one member per side of every env, planned over the half-envs for the whole-range call of A rows
int ac_policy_pool_assign_sides(ac_policy_pool_t* p, void* stream, const int32_t* d_members2, int64_t E, int32_t A) {
  if (!p || !d_members2) return fail("ac_policy_pool_assign_sides: null argument");
  if (A < 2 || A % 2) return fail("ac_policy_pool_assign_sides: A must be even and >= 2 (got " + std::to_string(A) + ")");
  if (E < 1 || E * A > (1 << 24)) return fail("ac_policy_pool_assign_sides: E must be >= 1 with E * A <= 2^24");
  HIP_OK(hipSetDevice(p->device));
  return pool_assign(p, (hipStream_t)stream, d_members2, 2 * E, E, A, 1);
}
// waits for `stream`: the first env of the plan's assignment whose member is out of range or not loaded (-1: none), and its tile count
int ac_policy_pool_check(ac_policy_pool_t* p, void* stream, int32_t* bad_env, int32_t* ntiles) {
  if (!p || !bad_env || !ntiles) return fail("ac_policy_pool_check: null argument");
  if (p->E < 0) return fail("ac_policy_pool_check: no assignment (ac_policy_pool_assign)");
  HIP_OK(hipSetDevice(p->device));
  const pol::Plan a = pool_plan_args(nullptr, 0, 1, p->capacity, nullptr, p->d_scratch, nullptr, nullptr);
  int v[2] = {0, 0};   // ntiles, bad_env (adjacent in the scratch)
  HIP_OK(hipMemcpyAsync(v, a.ntiles, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  *ntiles = v[0]; *bad_env = p->sided && v[1] >= 0 ? v[1] / 2 : v[1];   // (a sided plan's units are half-envs)
  p->ntiles_host = v[0];
  return 0;
}
int ac_policy_pool_plan_host(const int32_t* members, int64_t E, int32_t na, int32_t capacity, const int32_t* loaded, int32_t* order,
                             int32_t* tiles, int32_t* ntiles, int32_t* bad_env) {
  if (!members || !order || !tiles || !ntiles || !bad_env) return fail("ac_policy_pool_plan_host: null argument");
  if (E < 1 || na < 1 || capacity < 1 || E * na > (1 << 24)) return fail("ac_policy_pool_plan_host: bad size");
  std::vector<int> all(capacity, 1), scratch((size_t)pool_scratch_ints(capacity));
  std::vector<int4> t4((size_t)pool_max_tiles(E, na, capacity));
  const pol::Plan a = pool_plan_args(members, E, na, capacity, loaded ? loaded : all.data(), scratch.data(), t4.data(), order);
  for (int ph = 0; ph < pol::PLAN_PHASES; ++ph)
    for (int t = 0; t < pol::PLAN_T; ++t) pol::pool_plan_phase(a, ph, t);
  *ntiles = *a.ntiles; *bad_env = *a.bad_env;
  for (int k = 0; k < *ntiles; ++k) { tiles[3 * k] = t4[k].x; tiles[3 * k + 1] = t4[k].y; tiles[3 * k + 2] = t4[k].z; }
  return 0;
}
int ac_policy_pool_max_tiles(int64_t E, int32_t na, int32_t capacity, int64_t* out) {
  if (!out || E < 0 || na < 1 || capacity < 1) return fail("ac_policy_pool_max_tiles: bad argument");
  *out = pool_max_tiles(E, na, capacity);
  return 0;
}
// one launch on `stream` for the rows of the plan: each assigned row with its member's actor, in the row convention of
// ac_policy_get_actions; rows of envs assigned -1 (or a bad member) are not written
int ac_policy_pool_act(ac_policy_pool_t* p, void* stream, const ac_policy_rows_t* rows, const float* d_obs, const float* d_h_in,
                       const float* d_masks, int32_t deterministic, uint64_t seed, uint64_t counter, float* d_actions, float* d_logp,
                       float* d_h_out) {
  if (!p || !rows || !d_obs || !d_h_in || !d_masks || !d_actions || !d_logp || !d_h_out) return fail("ac_policy_pool_act: null argument");
  if (p->E < 0) return fail("ac_policy_pool_act: no assignment (ac_policy_pool_assign)");
  const ac_policy_config_t& c = p->net.cfg;
  const int nh = c.n_cat + c.n_shoot;
  int na = rows->na, A = rows->A;
  if (na == 0) { na = 1; A = 1; }
  if (na < 1 || A < na || rows->a0 < 0 || rows->a0 + na > A || rows->n % na) return fail("ac_policy_pool_act: bad agent range");
  if (rows->act_stride < nh) return fail("ac_policy_pool_act: act_stride is smaller than the number of heads");
  if (p->sided && (na != p->na || A != p->na || rows->a0 != 0 || rows->n != p->E * p->na))
    return fail("ac_policy_pool_act: a sided plan (ac_policy_pool_assign_sides) for " + std::to_string(p->E) + " envs of " +
                std::to_string(p->na) + " agents is in force and takes the whole-range call only (n " + std::to_string(p->E * p->na) +
                ", na = A = " + std::to_string(p->na) + ", a0 0); the call has n " + std::to_string(rows->n) + ", na " + std::to_string(na) +
                ", A " + std::to_string(A) + ", a0 " + std::to_string(rows->a0));
  if (rows->n != p->E * na)
    return fail("ac_policy_pool_act: the call has " + std::to_string(rows->n) + " rows, the assignment " + std::to_string(p->E) + " envs of " +
                std::to_string(na) + " rows");
  HIP_OK(hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)stream;
  if (na != p->na && pool_build_plan(p, st, na) != 0) return -1;
  pol::Args a{};
  a.obs = d_obs; a.h_in[0] = d_h_in; a.h_out[0] = d_h_out;
  a.masks = d_masks; a.actions = d_actions; a.logp = d_logp;
  a.n = (int)rows->n; a.obs_dim = c.obs_dim; a.act_stride = rows->act_stride;
  a.na = na; a.A = A; a.a0 = rows->a0;
  a.n_cat = c.n_cat; a.n_shoot = c.n_shoot; a.use_fn = c.use_feature_normalization; a.deterministic = deterministic ? 1 : 0;
  for (int i = 0; i < pol::MAXCAT; ++i) { a.cat_off[i] = p->net.cat_off[i]; a.cat_cnt[i] = p->net.cat_cnt[i]; }
  a.seed = seed; a.counter = counter;
  const pol::Plan pl = pool_plan_args(nullptr, 0, 1, p->capacity, nullptr, p->d_scratch, nullptr, nullptr);
  pol::Pool x{};
  x.W0 = p->d_w; x.stride = p->net.packed_n[0]; x.tiles = p->d_tiles; x.order = p->d_order; x.ntiles = pl.ntiles; x.xcd = p->xcd;
  // the exact tile count once ac_policy_pool_check has read it, else the plan's bound (workgroups past the count exit)
  int64_t nt = p->ntiles_host >= 0 ? p->ntiles_host : pool_max_tiles(pool_units(p), pool_unit_rows(p, na), p->capacity);
  if (nt == 0) return 0;
  if (p->xcd) nt = (nt + 7) / 8 * 8;
  const dim3 g((unsigned)nt);
  if (p->net.wide) {
    pol::Wide w{};
    w.dim[0] = p->net.in_dim[0]; w.kpad[0] = (p->net.in_dim[0] + 31) / 32 * 32;
    if (p->net.np == 3) hipLaunchKernelGGL(policy_pool_wide_kernel<3>, g, dim3(512), 0, st, a, w, x);
    else hipLaunchKernelGGL(policy_pool_wide_kernel<2>, g, dim3(512), 0, st, a, w, x);
  } else if (p->net.np == 3) hipLaunchKernelGGL(policy_pool_kernel<3>, g, dim3(512), 0, st, a, x);
  else hipLaunchKernelGGL(policy_pool_kernel<2>, g, dim3(512), 0, st, a, x);
  HIP_OK(hipGetLastError());
  return 0;
}
}  // extern "C"
