// The tail of the PPO / MAPPO update on the device ("The loss, the clip and Adam"): the reference's loss
// (algorithms/ppo/ppo_trainer.py:44-61), torch's clip_grad_norm_ per optimiser param group and torch's single-tensor Adam, fp32
// everywhere. Two launches for the loss forward, one for its backward, and three for the optimiser whatever the number of tensors:
// the chunks' sums of squares, their fixed-order sum per group, then clip + Adam over every chunk.
//
// No floating-point atomics: a thread adds its own elements in index order, a wave's 64 sums meet in a shuffle tree, a workgroup's four
// waves are added in wave order, and the workgroups' partials are added by one workgroup in the same way. The order depends on the
// sizes alone, so results are bit-identical from run to run.
//
// Gradient conventions (torch's, which the tests' float64 restatement decides): clamp passes the gradient on its CLOSED interval and
// nothing outside; min / max give the whole gradient to the smaller / larger argument and half to each on a tie.
#pragma once

namespace ppou {
constexpr int THREADS = 256;
constexpr int WG_ROWS = 1024;      // rows of the loss one workgroup takes per pass
constexpr int MAX_WGS = 256;       // workgroups of the loss at most; beyond MAX_WGS * WG_ROWS rows they take further passes
constexpr int NSUM = 5;            // the loss's sums: policy, value, active, ratio, entropy
constexpr int NSTAT = 8;           // the stats vector (AC_PPO_STAT_*)
constexpr int CHUNK = 2048;        // elements of one optimiser chunk = one workgroup
constexpr int MAX_ENTRIES = 512;
constexpr int MAX_GROUPS = 8;

// the sum of v over the workgroup in a fixed order, valid in thread 0; `sh` holds one float per wave
__device__ __forceinline__ float block_sum(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();   // the previous use of sh is behind
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + (sh[2] + sh[3]));
}

struct LossArgs {
  const float *logp, *old_logp, *adv, *values, *value_preds, *returns, *active, *ent;
  int M, n_ent, old_cols, clipped_value;
  float ratio_lo, ratio_hi, clip, value_coef, ent_coef;
};

// Pass 1: per row the two losses and their gradients before the division by the denominator (M, or the sum of active), the
// workgroup's five sums to ws[blockIdx.x * NSUM ..].
__global__ __launch_bounds__(THREADS) void ppo_loss_rows(const LossArgs a, float* __restrict__ ws, float* __restrict__ dlogp,
                                                         float* __restrict__ dvalues) {
  __shared__ float sh[4];
  float s_pol = 0.0f, s_val = 0.0f, s_act = 0.0f, s_ratio = 0.0f, s_ent = 0.0f;
  const int n = a.M > a.n_ent ? a.M : a.n_ent;
  for (int64_t base = (int64_t)blockIdx.x * WG_ROWS; base < n; base += (int64_t)gridDim.x * WG_ROWS) {
#pragma unroll
    for (int j = 0; j < WG_ROWS / THREADS; ++j) {
      const int64_t i = base + j * THREADS + threadIdx.x;
      if (i < a.n_ent) s_ent += a.ent[i];
      if (i >= a.M) continue;
      const float act = a.active ? a.active[i] : 1.0f;
      const float adv = a.adv[i], v = a.values[i], vp = a.value_preds[i], R = a.returns[i];
      // old_logp may hold several columns per row (the MAPPO buffer keeps one per action column): logp broadcasts against them
      const float lp = a.logp[i];
      float row_min = 0.0f, row_dl = 0.0f;
      for (int c = 0; c < a.old_cols; ++c) {
        const float ratio = expf(lp - a.old_logp[i * a.old_cols + c]);
        const float rc = fminf(fmaxf(ratio, a.ratio_lo), a.ratio_hi);
        const float s1 = ratio * adv, s2 = rc * adv;
        const bool inside = ratio >= a.ratio_lo && ratio <= a.ratio_hi;
        const float g1 = s1 < s2 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f), g2 = s2 < s1 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);
        row_min += fminf(s1, s2);
        row_dl += ratio * adv * (g1 + (inside ? g2 : 0.0f));
        s_ratio += ratio;
      }
      s_pol += row_min * act;
      s_act += act;
      dlogp[i] = -(act * row_dl);
      float vl, dv;
      if (a.clipped_value) {
        const float d = v - vp;
        const float vpc = vp + fminf(fmaxf(d, -a.clip), a.clip);
        const float e1 = v - R, e2 = vpc - R;
        const float l1 = e1 * e1, l2 = e2 * e2;
        const bool in_v = d >= -a.clip && d <= a.clip;
        const float h1 = l1 > l2 ? 1.0f : (l1 == l2 ? 0.5f : 0.0f), h2 = l2 > l1 ? 1.0f : (l1 == l2 ? 0.5f : 0.0f);
        vl = 0.5f * fmaxf(l1, l2);
        dv = h1 * e1 + (in_v ? h2 * e2 : 0.0f);
      } else {
        const float e = R - v;
        vl = 0.5f * (e * e);
        dv = -e;
      }
      s_val += vl * act;
      dvalues[i] = a.value_coef * (act * dv);
    }
  }
  const float sums[NSUM] = {s_pol, s_val, s_act, s_ratio, s_ent};
#pragma unroll
  for (int k = 0; k < NSUM; ++k) {
    const float t = block_sum(sums[k], sh);
    if (threadIdx.x == 0) ws[blockIdx.x * NSUM + k] = t;
  }
}

// Pass 2, on the same grid: every workgroup adds the G partials (the same order in each, so the same denominators), scales its own
// rows' gradients by 1 / denominator; workgroup 0 writes the stats.
__global__ __launch_bounds__(THREADS) void ppo_loss_finish(const LossArgs a, const float* __restrict__ ws, int G, float* __restrict__ stats,
                                                           float* __restrict__ loss, float* __restrict__ dlogp, float* __restrict__ dvalues) {
  __shared__ float sh[4];
  __shared__ float tot[NSUM];
#pragma unroll
  for (int k = 0; k < NSUM; ++k) {
    const float t = block_sum((int)threadIdx.x < G ? ws[threadIdx.x * NSUM + k] : 0.0f, sh);
    if (threadIdx.x == 0) tot[k] = t;
  }
  __syncthreads();
  const float den = a.active ? tot[2] : (float)a.M;
  const float inv = 1.0f / den;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const float pol = -(tot[0] / den), val = tot[1] / den, pel = -(tot[4] / (float)a.n_ent);
    const float total = pol + val * a.value_coef + pel * a.ent_coef;
    stats[0] = total;
    if (loss) loss[0] = total;
    stats[1] = pol;
    stats[2] = val;
    stats[3] = pel;
    stats[4] = tot[3] / ((float)a.M * (float)a.old_cols);
    stats[5] = den;
    stats[6] = 0.0f;
    stats[7] = 0.0f;
  }
  for (int64_t base = (int64_t)blockIdx.x * WG_ROWS; base < a.M; base += (int64_t)gridDim.x * WG_ROWS) {
#pragma unroll
    for (int j = 0; j < WG_ROWS / THREADS; ++j) {
      const int64_t i = base + j * THREADS + threadIdx.x;
      if (i < a.M) {
        dlogp[i] *= inv;
        dvalues[i] *= inv;
      }
    }
  }
}

// upstream (a device scalar) x the saved gradients, and the entropy's constant
__global__ __launch_bounds__(THREADS) void ppo_loss_bwd(const float* __restrict__ up, const float* __restrict__ dlogp, const float* __restrict__ dvalues,
                                                        int M, int n_ent, float ent_grad, float* __restrict__ g_logp, float* __restrict__ g_values,
                                                        float* __restrict__ g_ent) {
  const float u = up[0];
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i < M) {
    if (g_logp) g_logp[i] = u * dlogp[i];
    if (g_values) g_values[i] = u * dvalues[i];
  }
  if (g_ent && i < n_ent) g_ent[i] = u * ent_grad;
}

// ---- the optimiser: the device's view of ac_optim_entry_t (same layout)
struct Entry {
  float *p, *g, *m, *v;
  int64_t numel;
  int32_t group, first_chunk;
  double lr, eps, beta1, beta2, bias_correction1, bias_correction2;
};
static_assert(sizeof(Entry) == sizeof(ac_optim_entry_t), "ac_optim_entry_t");

// the entry whose chunks hold chunk c: the last one with first_chunk <= c (first_chunk is strictly increasing)
__device__ __forceinline__ int entry_of(const Entry* __restrict__ tab, int n, int c) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].first_chunk <= c) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// one workgroup per chunk: the sum of squares of its gradients to ws[c], its group (as a float) to ws[nchunks + c]
__global__ __launch_bounds__(THREADS) void grad_sq_chunks(const Entry* __restrict__ tab, int n, int nchunks, float* __restrict__ ws) {
  __shared__ float sh[4];
  const int c = blockIdx.x;
  const Entry e = tab[entry_of(tab, n, c)];
  const int64_t off = (int64_t)(c - e.first_chunk) * CHUNK;
  const int len = (int)(e.numel - off < CHUNK ? e.numel - off : CHUNK);
  const float* g = e.g + off;
  const bool vec = trn::aligned16(g);
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < CHUNK / (4 * THREADS); ++j) {
    const int i = 4 * (j * THREADS + threadIdx.x);
    if (vec && i + 4 <= len) {
      const float4 q = *reinterpret_cast<const float4*>(g + i);
      s += q.x * q.x;
      s += q.y * q.y;
      s += q.z * q.z;
      s += q.w * q.w;
    } else {
      for (int k = i; k < i + 4 && k < len; ++k) s += g[k] * g[k];
    }
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) {
    ws[c] = s;
    ws[nchunks + c] = (float)e.group;
  }
}

// one workgroup: norms[g] = sqrt of the sum of group g's chunks, chunk c added by thread c % 256 in the order of c
__global__ __launch_bounds__(THREADS) void grad_norms_reduce(const float* __restrict__ ws, int nchunks, int ngroups, float* __restrict__ norms) {
  __shared__ float sh[4];
  for (int grp = 0; grp < ngroups; ++grp) {
    float s = 0.0f;
    for (int c = threadIdx.x; c < nchunks; c += THREADS) s += ws[nchunks + c] == (float)grp ? ws[c] : 0.0f;
    s = block_sum(s, sh);
    if (threadIdx.x == 0) norms[grp] = sqrtf(s);
  }
}

__device__ __forceinline__ void adam_one(float& p, float& g, float& m, float& v, float coef, float w1, float b2, float w2, float step_size,
                                         float bc2_sqrt, float eps) {
  g = g * coef;
  m = m + w1 * (g - m);
  v = v * b2 + w2 * (g * g);
  p = p - step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
}

// one workgroup per chunk: g <- g * coef of its group, then torch's single-tensor Adam on (p, m, v)
__global__ __launch_bounds__(THREADS) void clip_adam_chunks(const Entry* __restrict__ tab, int n, const float* __restrict__ norms, float max_norm,
                                                            int clip) {
  const int c = blockIdx.x;
  const Entry e = tab[entry_of(tab, n, c)];
  const int64_t off = (int64_t)(c - e.first_chunk) * CHUNK;
  const int len = (int)(e.numel - off < CHUNK ? e.numel - off : CHUNK);
  float *p = e.p + off, *g = e.g + off, *m = e.m + off, *v = e.v + off;
  // clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1); a NaN stays a NaN
  const float q = max_norm / (norms[e.group] + 1e-6f);
  const float coef = clip ? (q > 1.0f ? 1.0f : q) : 1.0f;
  const float w1 = (float)(1.0 - e.beta1), b2 = (float)e.beta2, w2 = (float)(1.0 - e.beta2);
  const float step_size = (float)(e.lr / e.bias_correction1), bc2_sqrt = (float)sqrt(e.bias_correction2), eps = (float)e.eps;
  const bool vec = trn::aligned16(p) && trn::aligned16(g) && trn::aligned16(m) && trn::aligned16(v);
#pragma unroll
  for (int j = 0; j < CHUNK / (4 * THREADS); ++j) {
    const int i = 4 * (j * THREADS + threadIdx.x);
    if (vec && i + 4 <= len) {
      float4 P = *reinterpret_cast<float4*>(p + i), Gq = *reinterpret_cast<float4*>(g + i), Mq = *reinterpret_cast<float4*>(m + i),
             V = *reinterpret_cast<float4*>(v + i);
      adam_one(P.x, Gq.x, Mq.x, V.x, coef, w1, b2, w2, step_size, bc2_sqrt, eps);
      adam_one(P.y, Gq.y, Mq.y, V.y, coef, w1, b2, w2, step_size, bc2_sqrt, eps);
      adam_one(P.z, Gq.z, Mq.z, V.z, coef, w1, b2, w2, step_size, bc2_sqrt, eps);
      adam_one(P.w, Gq.w, Mq.w, V.w, coef, w1, b2, w2, step_size, bc2_sqrt, eps);
      *reinterpret_cast<float4*>(p + i) = P;
      *reinterpret_cast<float4*>(g + i) = Gq;
      *reinterpret_cast<float4*>(m + i) = Mq;
      *reinterpret_cast<float4*>(v + i) = V;
    } else {
      for (int k = i; k < i + 4 && k < len; ++k) adam_one(p[k], g[k], m[k], v[k], coef, w1, b2, w2, step_size, bc2_sqrt, eps);
    }
  }
}
}  // namespace ppou

// ------------------------------------------------------------------------------------------------ C ABI (include/aircombat.h)
extern "C" {
static int ppo_loss_M_ok(const std::string& w, int32_t M, int32_t n_ent) {
  if (M < 1) return fail(w + ": M must be at least 1");
  if (n_ent < 1) return fail(w + ": n_ent must be at least 1");
  const int64_t lim = (int64_t)INT32_MAX - ppou::WG_ROWS;
  if (M > lim || n_ent > lim) return fail(w + ": M exceeds the kernels' 32-bit index");
  return 0;
}

static int ppo_loss_wgs(int32_t M, int32_t n_ent) {
  const int64_t n = M > n_ent ? M : n_ent, g = (n + ppou::WG_ROWS - 1) / ppou::WG_ROWS;
  return (int)(g < ppou::MAX_WGS ? g : ppou::MAX_WGS);
}

int64_t ac_ppo_loss_workspace_floats(int32_t M, int32_t n_ent) {
  if (ppo_loss_M_ok("ac_ppo_loss_workspace_floats", M, n_ent)) return -1;
  return (int64_t)ppo_loss_wgs(M, n_ent) * ppou::NSUM;
}

int ac_ppo_loss_forward(int32_t device_id, void* stream, int32_t M, int32_t n_ent, int32_t old_cols, const float* d_logp,
                        const float* d_old_logp, const float* d_adv, const float* d_values, const float* d_value_preds, const float* d_returns, const float* d_active,
                        const float* d_ent, double clip_param, double value_loss_coef, double entropy_coef, int32_t use_clipped_value_loss,
                        float* d_workspace, float* d_stats, float* d_loss, float* d_dlogp, float* d_dvalues) {
  const std::string who = "ac_ppo_loss_forward";
  if (ppo_loss_M_ok(who, M, n_ent)) return -1;
  if (old_cols < 1 || old_cols > 64) return fail(who + ": old_cols must be 1 .. 64");
  if (!d_logp || !d_old_logp || !d_adv || !d_values || !d_value_preds || !d_returns || !d_ent || !d_workspace || !d_stats || !d_dlogp || !d_dvalues)
    return fail(who + ": null argument");
  ppou::LossArgs a{d_logp, d_old_logp, d_adv, d_values, d_value_preds, d_returns, d_active, d_ent, M, n_ent, old_cols, use_clipped_value_loss ? 1 : 0,
                   (float)(1.0 - clip_param), (float)(1.0 + clip_param), (float)clip_param, (float)value_loss_coef, (float)entropy_coef};
  HIP_OK(hipSetDevice(device_id));
  const int G = ppo_loss_wgs(M, n_ent);
  hipLaunchKernelGGL(ppou::ppo_loss_rows, dim3(G), dim3(ppou::THREADS), 0, (hipStream_t)stream, a, d_workspace, d_dlogp, d_dvalues);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(ppou::ppo_loss_finish, dim3(G), dim3(ppou::THREADS), 0, (hipStream_t)stream, a, (const float*)d_workspace, G, d_stats, d_loss,
                     d_dlogp, d_dvalues);
  HIP_OK(hipGetLastError());
  return 0;
}

int ac_ppo_loss_backward(int32_t device_id, void* stream, int32_t M, int32_t n_ent, const float* d_upstream, const float* d_dlogp,
                         const float* d_dvalues, double entropy_coef, float* d_g_logp, float* d_g_values, float* d_g_ent) {
  const std::string who = "ac_ppo_loss_backward";
  if (ppo_loss_M_ok(who, M, n_ent)) return -1;
  if (!d_upstream || !d_dlogp || !d_dvalues) return fail(who + ": null argument");
  HIP_OK(hipSetDevice(device_id));
  const int64_t n = M > n_ent ? M : n_ent;
  hipLaunchKernelGGL(ppou::ppo_loss_bwd, dim3((unsigned)((n + ppou::THREADS - 1) / ppou::THREADS)), dim3(ppou::THREADS), 0, (hipStream_t)stream,
                     d_upstream, d_dlogp, d_dvalues, (int)M, (int)n_ent, (float)(-entropy_coef / (double)n_ent), d_g_logp, d_g_values, d_g_ent);
  HIP_OK(hipGetLastError());
  return 0;
}

// the checked table: 0 and the number of chunks, or -1 with the message; with `fill`, first_chunk is written, else it must be right
static int optim_table_ok(const std::string& w, ac_optim_entry_t* tab, int32_t n, int32_t n_groups, bool fill, int64_t* nchunks) {
  if (!tab) return fail(w + ": null argument");
  if (n < 1) return fail(w + ": no entries (no parameter has a gradient)");
  if (n > ppou::MAX_ENTRIES) return fail(w + ": " + std::to_string(n) + " entries (at most " + std::to_string(ppou::MAX_ENTRIES) + ")");
  if (n_groups < 1 || n_groups > ppou::MAX_GROUPS) return fail(w + ": n_groups must be 1 .. " + std::to_string(ppou::MAX_GROUPS));
  int64_t c = 0;
  for (int i = 0; i < n; ++i) {
    const std::string at = w + ": entry " + std::to_string(i);
    if (!tab[i].p || !tab[i].g || !tab[i].m || !tab[i].v) return fail(at + ": null pointer");
    if (((uintptr_t)tab[i].p | (uintptr_t)tab[i].g | (uintptr_t)tab[i].m | (uintptr_t)tab[i].v) & 3) return fail(at + ": a pointer is not 4-byte aligned");
    if (tab[i].numel < 1) return fail(at + ": numel must be at least 1");
    if (tab[i].group < 0 || tab[i].group >= n_groups) return fail(at + ": group " + std::to_string(tab[i].group) + " out of range (0 .. " + std::to_string(n_groups - 1) + ")");
    if (fill) tab[i].first_chunk = (int32_t)c;
    else if (tab[i].first_chunk != c) return fail(at + ": first_chunk is not laid out (ac_optim_workspace_floats fills it)");
    c += (tab[i].numel + ppou::CHUNK - 1) / ppou::CHUNK;
    if (c > (int64_t)1 << 30) return fail(w + ": too many elements");
  }
  *nchunks = c;
  return 0;
}

int64_t ac_optim_workspace_floats(ac_optim_entry_t* entries, int32_t n_entries, int32_t n_groups) {
  int64_t nchunks;
  if (optim_table_ok("ac_optim_workspace_floats", entries, n_entries, n_groups, true, &nchunks)) return -1;
  return 2 * nchunks;
}

int ac_optim_grad_norms(int32_t device_id, void* stream, const ac_optim_entry_t* entries, const ac_optim_entry_t* d_entries, int32_t n_entries,
                        int32_t n_groups, float* d_workspace, float* d_norms) {
  const std::string who = "ac_optim_grad_norms";
  int64_t nchunks;
  if (optim_table_ok(who, const_cast<ac_optim_entry_t*>(entries), n_entries, n_groups, false, &nchunks)) return -1;
  if (!d_entries || !d_workspace || !d_norms) return fail(who + ": null argument");
  HIP_OK(hipSetDevice(device_id));
  hipLaunchKernelGGL(ppou::grad_sq_chunks, dim3((unsigned)nchunks), dim3(ppou::THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<const ppou::Entry*>(d_entries), (int)n_entries, (int)nchunks, d_workspace);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(ppou::grad_norms_reduce, dim3(1), dim3(ppou::THREADS), 0, (hipStream_t)stream, (const float*)d_workspace, (int)nchunks,
                     (int)n_groups, d_norms);
  HIP_OK(hipGetLastError());
  return 0;
}

int ac_optim_clip_adam_step(int32_t device_id, void* stream, const ac_optim_entry_t* entries, const ac_optim_entry_t* d_entries,
                            int32_t n_entries, int32_t n_groups, const float* d_norms, double max_grad_norm, int32_t use_max_grad_norm) {
  const std::string who = "ac_optim_clip_adam_step";
  int64_t nchunks;
  if (optim_table_ok(who, const_cast<ac_optim_entry_t*>(entries), n_entries, n_groups, false, &nchunks)) return -1;
  if (!d_entries || !d_norms) return fail(who + ": null argument");
  HIP_OK(hipSetDevice(device_id));
  hipLaunchKernelGGL(ppou::clip_adam_chunks, dim3((unsigned)nchunks), dim3(ppou::THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<const ppou::Entry*>(d_entries), (int)n_entries, d_norms, (float)max_grad_norm, use_max_grad_norm ? 1 : 0);
  HIP_OK(hipGetLastError());
  return 0;
}

int32_t ac_ppo_update_constant(int32_t which) {
  switch (which) {
    case 0: return ppou::WG_ROWS;
    case 1: return ppou::MAX_WGS;
    case 2: return ppou::CHUNK;
    case 3: return ppou::MAX_ENTRIES;
    case 4: return ppou::MAX_GROUPS;
    default: return -1;
  }
}
}  // extern "C"
