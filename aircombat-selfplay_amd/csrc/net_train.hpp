// The PPO update's actor and critic as one call each ("The networks as one call"): the pieces of the reference's two
// networks that no training layer covered, as kernels, and the host chains that queue a whole network's layer launches back to back.
//
// Kernels. value_head_*: the critic's value_out, v = x w + b with x [M, 128], and its gradients. feature_norm_*: nn.LayerNorm over the
// raw observation, K = 1 .. 256 wide, and its gradients. shoot_prior: alpha0 / beta0 of the reference's actor from columns 11 and 13
// of the observation. They are bandwidth kernels: a workgroup of eight waves walks 64-row tiles in a persistent loop, one wave per row
// (row r of the tile on wave r % 8, the loads of FLY rows in flight per wave). A lane takes columns 2 l, 2 l + 1 of the 128 (value
// head) or l, l + 64, l + 128, l + 192 of the K (feature norm), so every wave reads whole contiguous rows.
//
// Sums over rows follow ppo_update.hpp's convention: a thread adds the rows it owns in ascending order, a row's sum over columns is the
// xor-shuffle tree (mlpt::wave_sum), the eight waves' shares are added in wave order through LDS, and each workgroup leaves one set of
// partial sums in the workspace that net_sum_partials adds in trn::sum_sets' fixed order. No floating-point atomics: results are
// bit-identical from run to run. The sums over rows are kept in double until a workgroup's set is written (as fp32) and again while
// the sets are added: db of the value head and dbeta of a one-column feature norm are single numbers that cancel, so fp32 sums of a
// few dozen rows already miss the tests' bound, which is relative to the result; a bandwidth kernel does not notice the few DP adds.
//
// Chains. ac_actor_eval_* and ac_critic_* call the C entries of mlp_train.hpp, gru_layer_train.hpp and act_train.hpp, and this
// file's, in network order on the caller's stream, with the arguments the Python layers give them one by one; they allocate nothing,
// wait for nothing and read nothing back.
#pragma once

namespace nett {
constexpr int H = 128;
constexpr int RT = 64;          // rows per tile: eight per wave, four of them in flight at a time
constexpr int WAVES = 8;
constexpr int THREADS = 64 * WAVES;
constexpr int FLY = 4;          // rows a wave has loads in flight for
static_assert((RT / WAVES) % FLY == 0, "a wave's rows of a tile come in whole batches");
constexpr int KMAX = 256;
constexpr int FWD_WGS = 512;    // persistent workgroups at most
constexpr int BWD_WGS = 256;    // and for the backwards: also the number of partial sets net_sum_partials adds
constexpr int VH_NEL = H + 1;   // a value-head partial set: dw [128], db

// s / K to the last bit where K s' = s exactly (a row of equal entries has variance 0 then): the hardware reciprocal's quotient and
// one correction by its exact residual
__device__ __forceinline__ float div_k(float s, float Kf, float invK) {
  const float m = s * invK;
  return fmaf(fmaf(-m, Kf, s), invK, m);
}

// v [M] = x w + b
__global__ __launch_bounds__(THREADS) void value_head_fwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                      float* __restrict__ v, int M) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float2 wl = reinterpret_cast<const float2*>(w)[lane];
  const float bias = b[0];
  const int ntiles = (M + RT - 1) / RT;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll
    for (int j0 = 0; j0 < RT / WAVES; j0 += FLY) {
      float p[FLY];
#pragma unroll
      for (int j = 0; j < FLY; ++j) {
        const int row = tile * RT + wv + WAVES * (j0 + j);
        float2 t = {0.0f, 0.0f};
        if (row < M) t = reinterpret_cast<const float2*>(x + (size_t)row * H)[lane];
        p[j] = fmaf(t.y, wl.y, t.x * wl.x);
      }
#pragma unroll
      for (int j = 0; j < FLY; ++j) {
        const int row = tile * RT + wv + WAVES * (j0 + j);
        const float s = mlpt::wave_sum(p[j]);
        if (row < M && lane == 0) v[row] = s + bias;
      }
    }
  }
}

// One set per workgroup at ws + blockIdx.x * 129: dw[k] = sum_m g[m] x[m, k], db = sum_m g[m]. DX: dx[m, k] = g[m] w[k] is wanted.
template <bool DX>
__global__ __launch_bounds__(THREADS) void value_head_bwd(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ w,
                                                      float* __restrict__ ws, float* __restrict__ dx, int M) {
  __shared__ double part[WAVES][VH_NEL + 1];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const float2 wl = DX ? reinterpret_cast<const float2*>(w)[lane] : make_float2(0.0f, 0.0f);
  double a0 = 0.0, a1 = 0.0, ab = 0.0;
  const int ntiles = (M + RT - 1) / RT;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll
    for (int j0 = 0; j0 < RT / WAVES; j0 += FLY) {
      float gr[FLY];
      float2 t[FLY];
#pragma unroll
      for (int j = 0; j < FLY; ++j) {   // rows past M read nothing and add exact zeros
        const int row = tile * RT + wv + WAVES * (j0 + j);
        gr[j] = row < M ? g[row] : 0.0f;
        t[j] = row < M ? reinterpret_cast<const float2*>(x + (size_t)row * H)[lane] : make_float2(0.0f, 0.0f);
      }
#pragma unroll
      for (int j = 0; j < FLY; ++j) {
        const int row = tile * RT + wv + WAVES * (j0 + j);
        a0 += (double)gr[j] * (double)t[j].x;   // (a product of two floats is exact in double)
        a1 += (double)gr[j] * (double)t[j].y;
        ab += (double)gr[j];   // the same sum in every lane
        if (DX && row < M) reinterpret_cast<float2*>(dx + (size_t)row * H)[lane] = make_float2(gr[j] * wl.x, gr[j] * wl.y);
      }
    }
  }
  part[wv][2 * lane] = a0;
  part[wv][2 * lane + 1] = a1;
  if (lane == 0) part[wv][H] = ab;
  __syncthreads();
  if (tid < VH_NEL) {
    double s = part[0][tid];
#pragma unroll
    for (int p = 1; p < WAVES; ++p) s += part[p][tid];   // in wave order
    ws[(size_t)blockIdx.x * VH_NEL + tid] = (float)s;
  }
}

// trn::sum_sets with its order and double accumulators: chain j adds sets j, j + 8, .. ascending, then the eight chains pairwise
__device__ __forceinline__ float sum_sets_f64(const float* __restrict__ ws, int S, size_t nel, int e) {
  double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int s = 0;
  for (; s + 8 <= S; s += 8)
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += (double)ws[(size_t)(s + j) * nel + e];
  for (int j = 0; s < S; ++s, ++j) a[j] += (double)ws[(size_t)s * nel + e];
  return (float)(((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])));
}

// element e of the sum of the S partial sets of nel elements: the first n0 to o0, the rest to o1
__global__ __launch_bounds__(256) void net_sum_partials(const float* __restrict__ ws, int S, int nel, int n0, float* __restrict__ o0,
                                                        float* __restrict__ o1) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nel) return;
  const float s = sum_sets_f64(ws, S, (size_t)nel, e);
  if (e < n0) o0[e] = s;
  else o1[e - n0] = s;
}

// y [M, K] = (x - mean) / sqrt(var + eps) * gamma + beta over each row's K entries, biased variance; stats [M, 2] = (mean,
// 1 / sqrt(var + eps)) per row, or NULL (inference: nothing kept)
__global__ __launch_bounds__(THREADS) void feature_norm_fwd(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float* __restrict__ y, float* __restrict__ stats, int M, int K, float Kf, float invK,
                                                        float eps) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float gm[4], bt[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k = lane + 64 * c;
    gm[c] = k < K ? gamma[k] : 0.0f;
    bt[c] = k < K ? beta[k] : 0.0f;
  }
  const int ntiles = (M + RT - 1) / RT;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll
    for (int j0 = 0; j0 < RT / WAVES; j0 += FLY) {
      float v[FLY][4];
#pragma unroll
      for (int j = 0; j < FLY; ++j) {
        const int row = tile * RT + wv + WAVES * (j0 + j);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int k = lane + 64 * c;
          v[j][c] = (row < M && k < K) ? x[(size_t)row * K + k] : 0.0f;
        }
      }
#pragma unroll
      for (int j = 0; j < FLY; ++j) {
        const int row = tile * RT + wv + WAVES * (j0 + j);   // (row < M is the whole wave's: a row is a wave's)
        const float mean = div_k(mlpt::wave_sum((v[j][0] + v[j][1]) + (v[j][2] + v[j][3])), Kf, invK);
        float d[4], q = 0.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          d[c] = lane + 64 * c < K ? v[j][c] - mean : 0.0f;
          q = fmaf(d[c], d[c], q);
        }
        const float rstd = 1.0f / sqrtf(mlpt::wave_sum(q) * invK + eps);
        if (row < M) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int k = lane + 64 * c;
            if (k < K) y[(size_t)row * K + k] = (d[c] * rstd) * gm[c] + bt[c];
          }
          if (stats && lane < 2) stats[(size_t)row * 2 + lane] = lane ? rstd : mean;
        }
      }
    }
  }
}

// One set per workgroup at ws + blockIdx.x * 2 K: dgamma[k] = sum_m dy[m, k] xhat[m, k], dbeta[k] = sum_m dy[m, k], xhat recomputed
// from x and the forward's stats. DX: dx = rstd (g - mean_k(g) - xhat mean_k(g xhat)) with g = dy gamma is wanted.
template <bool DX>
__global__ __launch_bounds__(THREADS) void feature_norm_bwd(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ stats, float* __restrict__ ws, float* __restrict__ dx, int M,
                                                        int K, float invK) {
  __shared__ double part[WAVES][2 * KMAX];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  float gm[4];
  double dg[4], db[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k = lane + 64 * c;
    gm[c] = (DX && k < K) ? gamma[k] : 0.0f;
    dg[c] = 0.0;
    db[c] = 0.0;
  }
  const int ntiles = (M + RT - 1) / RT;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll
    for (int j0 = 0; j0 < RT / WAVES; j0 += FLY) {
      float gv[FLY][4], xv[FLY][4], mean[FLY], rstd[FLY];
#pragma unroll
      for (int j = 0; j < FLY; ++j) {   // rows past M read nothing: g = 0 and xhat = 0 add exact zeros to every sum
        const int row = tile * RT + wv + WAVES * (j0 + j);
        mean[j] = row < M ? stats[(size_t)row * 2] : 0.0f;
        rstd[j] = row < M ? stats[(size_t)row * 2 + 1] : 0.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int k = lane + 64 * c;
          gv[j][c] = (row < M && k < K) ? dy[(size_t)row * K + k] : 0.0f;
          xv[j][c] = (row < M && k < K) ? x[(size_t)row * K + k] : 0.0f;
        }
      }
#pragma unroll
      for (int j = 0; j < FLY; ++j) {
        const int row = tile * RT + wv + WAVES * (j0 + j);   // (row < M is the whole wave's)
        float xh[4], gg[4], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float g = gv[j][c];
          xh[c] = lane + 64 * c < K ? (xv[j][c] - mean[j]) * rstd[j] : 0.0f;
          dg[c] += (double)g * (double)xh[c];
          db[c] += (double)g;
          if (DX) {
            gg[c] = g * gm[c];
            s1 += gg[c];
            s2 = fmaf(gg[c], xh[c], s2);
          }
        }
        if (DX) {
          const float m1 = mlpt::wave_sum(s1) * invK, m2 = mlpt::wave_sum(s2) * invK;
          if (row < M) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const int k = lane + 64 * c;
              if (k < K) dx[(size_t)row * K + k] = rstd[j] * (gg[c] - m1 - xh[c] * m2);
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k = lane + 64 * c;
    part[wv][k] = dg[c];
    part[wv][KMAX + k] = db[c];
  }
  __syncthreads();
  static_assert(THREADS >= 2 * KMAX, "one thread per element of the set");
  if (tid < 2 * K) {   // the set: dgamma [K], dbeta [K]
    const int src = tid < K ? tid : KMAX + tid - K;
    double s = part[0][src];
#pragma unroll
    for (int p = 1; p < WAVES; ++p) s += part[p][src];   // in wave order
    ws[(size_t)blockIdx.x * 2 * K + tid] = (float)s;
  }
}

// ppo_actor.py:40-49 in the fp32 arithmetic of policy_kernel.hpp: alpha0 3 / 6 (<= 12 km) / 10 (<= 8 km), beta0 10 / 6 (<= 45 deg) /
// 3 (<= 22.5 deg); a NaN compares false and keeps 3 and 10
__global__ __launch_bounds__(256) void shoot_prior(const float* __restrict__ obs, float* __restrict__ alpha0, float* __restrict__ beta0, int M, int K) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const float ang = obs[(size_t)m * K + 11] * 57.29577951308232f, dist = obs[(size_t)m * K + 13] * 10000.0f;
  alpha0[m] = dist <= 8000.0f ? 10.0f : (dist <= 12000.0f ? 6.0f : 3.0f);
  beta0[m] = ang <= 22.5f ? 3.0f : (ang <= 45.0f ? 6.0f : 10.0f);
}

inline int64_t r4(int64_t n) { return (n + 3) & ~(int64_t)3; }   // every segment of the two float arrays starts 16-byte aligned

constexpr int MAXB = 4;   // blocks at most in base.mlp and in the head MLP
// Where a network's activations live, in floats from the start of d_saved (`save`), or of the workspace's unsaved part (without):
// out[i] is the [M, 128] output of stage i (the base blocks, the GRU layer, the head blocks), stats[i] block i's [M, 2].
struct Layout {
  int64_t fn_stats, xn, out[2 * MAXB + 1], stats[2 * MAXB], gru_y, gru_saved, gru_stats, alpha0, beta0, total;
};
inline Layout layout(const ac_net_t* net, int64_t M, bool save) {
  Layout l{};
  int64_t at = 0;
  auto take = [&](int64_t n) { const int64_t o = at; at += r4(n); return o; };
  const int nb = net->base_blocks, nh = net->head_blocks;
  if (net->feature_norm) {
    if (save) l.fn_stats = take(2 * M);
    l.xn = take(M * net->obs_dim);
  }
  for (int i = 0; i < nb + nh; ++i)
    if (save) l.stats[i] = take(2 * M);
  for (int i = 0; i < nb + nh + 1; ++i) l.out[i] = take(M * H);
  l.gru_y = take(M * H);
  if (save) {
    l.gru_saved = take(M * 4 * H);
    l.gru_stats = take(2 * M);
  }
  if (net->heads.n_shoot_cols) {
    l.alpha0 = take(M);
    l.beta0 = take(M);
  }
  l.total = at;
  return l;
}

// the parameter table's indices (include/aircombat.h, ac_net_t)
struct Index {
  int base, gru, head, out, count;
};
inline Index index(const ac_net_t* net) {
  Index ix;
  ix.base = net->feature_norm ? 2 : 0;
  ix.gru = ix.base + 4 * net->base_blocks;
  ix.head = ix.gru + 6;
  ix.out = ix.head + 4 * net->head_blocks;
  ix.count = ix.out + 2 * (net->heads.n_cat ? net->heads.n_cat + (net->heads.n_shoot_cols ? 1 : 0) : 1);
  return ix;
}
}  // namespace nett

// ------------------------------------------------------------------------------------------------ C ABI (include/aircombat.h)
extern "C" {
int32_t ac_net_constant(int32_t which) {
  switch (which) {
    case 0: return nett::RT;
    case 1: return nett::FWD_WGS;
    case 2: return nett::BWD_WGS;
    default: return -1;
  }
}

int64_t ac_value_head_workspace_floats(int32_t M) {
  if (mlp_shape_ok("ac_value_head_workspace_floats", M, nett::H)) return -1;
  return (int64_t)trn::capped_tiles(M, nett::RT, nett::BWD_WGS) * nett::VH_NEL;
}

int ac_value_head_forward(int32_t device_id, void* stream, int32_t M, const float* d_x, const float* d_w, const float* d_b, float* d_v) {
  const char* who = "ac_value_head_forward";
  if (!d_x || !d_w || !d_b || !d_v) return fail(std::string(who) + ": null argument");
  if (mlp_shape_ok(who, M, nett::H)) return -1;
  if (!trn::aligned16({d_x, d_w})) return fail(std::string(who) + ": x and w must be 16-byte aligned");
  HIP_OK(hipSetDevice(device_id));
  hipLaunchKernelGGL(nett::value_head_fwd, dim3(trn::capped_tiles(M, nett::RT, nett::FWD_WGS)), dim3(nett::THREADS), 0, (hipStream_t)stream, d_x, d_w, d_b,
                     d_v, (int)M);
  HIP_OK(hipGetLastError());
  return 0;
}

int ac_value_head_backward(int32_t device_id, void* stream, int32_t M, const float* d_g, const float* d_x, const float* d_w, float* d_workspace,
                           float* d_dx, float* d_dw, float* d_db) {
  const char* who = "ac_value_head_backward";
  if (!d_g || !d_x || !d_w || !d_workspace || !d_dw || !d_db) return fail(std::string(who) + ": null argument");
  if (mlp_shape_ok(who, M, nett::H)) return -1;
  if (!trn::aligned16({d_x, d_w, d_dx})) return fail(std::string(who) + ": x, w and dx must be 16-byte aligned");
  HIP_OK(hipSetDevice(device_id));
  const int G = trn::capped_tiles(M, nett::RT, nett::BWD_WGS);
  hipLaunchKernelGGL((d_dx ? nett::value_head_bwd<true> : nett::value_head_bwd<false>), dim3(G), dim3(nett::THREADS), 0, (hipStream_t)stream, d_g, d_x, d_w,
                     d_workspace, d_dx, (int)M);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(nett::net_sum_partials, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)d_workspace, G, nett::VH_NEL, nett::H, d_dw,
                     d_db);
  HIP_OK(hipGetLastError());
  return 0;
}

static int feature_norm_shape_ok(const char* who, int32_t M, int32_t K) {
  if (M < 1) return fail(std::string(who) + ": M must be at least 1");
  if (K < 1 || K > nett::KMAX) return fail(std::string(who) + ": K must be 1 .. 256");
  return trn::rows_fit_i32(who, M, K > nett::H ? K : nett::H, nett::RT);
}

int64_t ac_feature_norm_workspace_floats(int32_t M, int32_t K) {
  if (feature_norm_shape_ok("ac_feature_norm_workspace_floats", M, K)) return -1;
  return (int64_t)trn::capped_tiles(M, nett::RT, nett::BWD_WGS) * 2 * K;
}

int ac_feature_norm_forward(int32_t device_id, void* stream, int32_t M, int32_t K, float eps, const float* d_x, const float* d_gamma,
                            const float* d_beta, float* d_y, float* d_stats) {
  const char* who = "ac_feature_norm_forward";
  if (!d_x || !d_gamma || !d_beta || !d_y) return fail(std::string(who) + ": null argument");
  if (feature_norm_shape_ok(who, M, K)) return -1;
  HIP_OK(hipSetDevice(device_id));
  hipLaunchKernelGGL(nett::feature_norm_fwd, dim3(trn::capped_tiles(M, nett::RT, nett::FWD_WGS)), dim3(nett::THREADS), 0, (hipStream_t)stream, d_x, d_gamma,
                     d_beta, d_y, d_stats, (int)M, (int)K, (float)K, 1.0f / (float)K, eps);
  HIP_OK(hipGetLastError());
  return 0;
}

int ac_feature_norm_backward(int32_t device_id, void* stream, int32_t M, int32_t K, const float* d_dy, const float* d_x, const float* d_gamma,
                             const float* d_stats, float* d_workspace, float* d_dx, float* d_dgamma, float* d_dbeta) {
  const char* who = "ac_feature_norm_backward";
  if (!d_dy || !d_x || !d_gamma || !d_stats || !d_workspace || !d_dgamma || !d_dbeta) return fail(std::string(who) + ": null argument");
  if (feature_norm_shape_ok(who, M, K)) return -1;
  HIP_OK(hipSetDevice(device_id));
  const int G = trn::capped_tiles(M, nett::RT, nett::BWD_WGS);
  hipLaunchKernelGGL((d_dx ? nett::feature_norm_bwd<true> : nett::feature_norm_bwd<false>), dim3(G), dim3(nett::THREADS), 0, (hipStream_t)stream, d_dy, d_x,
                     d_gamma, d_stats, d_workspace, d_dx, (int)M, (int)K, 1.0f / (float)K);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(nett::net_sum_partials, dim3((2 * K + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)d_workspace, G, 2 * (int)K,
                     (int)K, d_dgamma, d_dbeta);
  HIP_OK(hipGetLastError());
  return 0;
}

int ac_shoot_prior(int32_t device_id, void* stream, int32_t M, int32_t K, const float* d_obs, float* d_alpha0, float* d_beta0) {
  const char* who = "ac_shoot_prior";
  if (!d_obs || !d_alpha0 || !d_beta0) return fail(std::string(who) + ": null argument");
  if (M < 1) return fail(std::string(who) + ": M must be at least 1");
  if (K < 14) return fail(std::string(who) + ": the observation has " + std::to_string(K) + " columns (the prior reads columns 11 and 13)");
  HIP_OK(hipSetDevice(device_id));
  hipLaunchKernelGGL(nett::shoot_prior, dim3((unsigned)(((int64_t)M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_obs, d_alpha0, d_beta0, (int)M, (int)K);
  HIP_OK(hipGetLastError());
  return 0;
}

// 0 and *actor (the description has action heads) or -1 with the message; `params`: the table's pointers are looked at too
static int net_ok(const char* who, const ac_net_t* net, int32_t N, int32_t T, bool params, bool* actor) {
  const std::string w(who);
  if (!net) return fail(w + ": null argument");
  if (gru_layer_shape_ok(who, N, T)) return -1;
  if (net->obs_dim < 1 || net->obs_dim > nett::KMAX) return fail(w + ": obs_dim must be 1 .. 256");
  if (net->feature_norm != 0 && net->feature_norm != 1) return fail(w + ": feature_norm must be 0 or 1");
  if (net->base_blocks < 1 || net->base_blocks > nett::MAXB) return fail(w + ": base_blocks must be 1 .. 4");
  if (net->head_blocks < 0 || net->head_blocks > nett::MAXB) return fail(w + ": head_blocks must be 0 .. 4");
  if (trn::products_ok(who, "products (mlp)", net->mlp_products) || trn::products_ok(who, "products (gru)", net->gru_products) ||
      trn::products_ok(who, "dense products", net->gru_dense_products))
    return -1;
  const int32_t M = N * T;
  if (feature_norm_shape_ok(who, M, net->obs_dim)) return -1;
  *actor = net->heads.n_cat != 0;
  if (*actor) {
    int total;
    if (act_heads_ok(who, &net->heads, M, &total)) return -1;
    if (net->heads.n_shoot_cols && net->obs_dim < 14) return fail(w + ": shoot columns need an observation of at least 14 columns (the prior reads 11 and 13)");
  } else if (net->heads.n_shoot_cols) {
    return fail(w + ": shoot columns without categorical heads");
  }
  if (params) {
    const nett::Index ix = nett::index(net);
    for (int i = 0; i < ix.count; ++i)
      if (!net->params[i]) return fail(w + ": null parameter " + std::to_string(i));
  }
  return 0;
}

int64_t ac_net_saved_floats(const ac_net_t* net, int32_t N, int32_t T) {
  bool actor;
  if (net_ok("ac_net_saved_floats", net, N, T, false, &actor)) return -1;
  return nett::layout(net, (int64_t)N * T, true).total;
}

// the backward's workspace: two [M, 128] gradients that take turns, the feature norm's [M, K] upstream, then the widest layer workspace
struct net_bwd_ws_t {
  int64_t g0, g1, dxn, layer, total;
};
static net_bwd_ws_t net_bwd_ws(const ac_net_t* net, int32_t N, int32_t T, bool actor) {
  const int32_t M = N * T;
  net_bwd_ws_t b;
  b.g0 = 0;
  b.g1 = (int64_t)M * nett::H;
  b.dxn = 2 * (int64_t)M * nett::H;
  b.layer = b.dxn + (net->feature_norm ? nett::r4((int64_t)M * net->obs_dim) : 0);
  int64_t widest = ac_gru_layer_workspace_floats(N, T);
  auto wider = [&](int64_t n) { widest = n > widest ? n : widest; };
  wider(ac_mlp_block_workspace_floats(M, net->obs_dim));
  wider(ac_mlp_block_workspace_floats(M, nett::H));
  wider(actor ? ac_act_eval_workspace_floats(&net->heads, M) : ac_value_head_workspace_floats(M));
  if (net->feature_norm) wider(ac_feature_norm_workspace_floats(M, net->obs_dim));
  b.total = b.layer + widest;
  return b;
}

int64_t ac_net_workspace_floats(const ac_net_t* net, int32_t N, int32_t T) {
  bool actor;
  if (net_ok("ac_net_workspace_floats", net, N, T, false, &actor)) return -1;
  const int64_t M = (int64_t)N * T;
  const int64_t fwd = M * 3 * nett::H + (int64_t)N * nett::H + nett::layout(net, M, false).total;
  const int64_t bwd = net_bwd_ws(net, N, T, actor).total;
  return fwd > bwd ? fwd : bwd;
}

// One network forward. Actor: o0 = logp, o1 = ent [M]. Critic: o0 = values [M], o1 = h_T [N, 128].
static int net_forward(const char* who, bool want_actor, int32_t device_id, void* stream, const ac_net_t* net, int32_t N, int32_t T,
                       const float* d_obs, const float* d_hxs, const float* d_masks, const float* d_actions, float* d_workspace, float* d_saved,
                       float* o0, float* o1) {
  bool actor;
  if (net_ok(who, net, N, T, true, &actor)) return -1;
  if (actor != want_actor) return fail(std::string(who) + (want_actor ? ": the description has no action heads" : ": the description has action heads"));
  if (!d_obs || !d_hxs || !d_masks || (actor && !d_actions) || !d_workspace || !o0 || !o1) return fail(std::string(who) + ": null argument");
  if (!trn::aligned16({d_workspace, d_saved})) return fail(std::string(who) + ": workspace and saved must be 16-byte aligned");
  const int32_t M = N * T;
  const bool save = d_saved != nullptr;
  const nett::Layout l = nett::layout(net, M, save);
  const nett::Index ix = nett::index(net);
  float* gi = d_workspace;
  float* h_T = actor ? d_workspace + (int64_t)M * 3 * nett::H : o1;
  float* base = save ? d_saved : d_workspace + (int64_t)M * 3 * nett::H + (int64_t)N * nett::H;
  const float* const* p = net->params;
  float *alpha0 = nullptr, *beta0 = nullptr;
  if (actor && net->heads.n_shoot_cols) {
    alpha0 = base + l.alpha0;
    beta0 = base + l.beta0;
    if (ac_shoot_prior(device_id, stream, M, net->obs_dim, d_obs, alpha0, beta0)) return -1;
  }
  const float* x = d_obs;
  if (net->feature_norm) {
    if (ac_feature_norm_forward(device_id, stream, M, net->obs_dim, net->feature_norm_eps, d_obs, p[0], p[1], base + l.xn, save ? base + l.fn_stats : nullptr))
      return -1;
    x = base + l.xn;
  }
  const int nb = net->base_blocks, nh = net->head_blocks;
  for (int j = 0; j < nb + nh + 1; ++j) {
    float* out = base + l.out[j];
    if (j == nb) {   // the GRU layer between the two MLPs
      const float* const* q = p + ix.gru;
      if (ac_gru_layer_forward_pd(device_id, stream, N, T, x, d_hxs, d_masks, q[0], q[1], q[2], q[3], q[4], q[5], net->gru_eps, gi, out, h_T,
                                  base + l.gru_y, save ? base + l.gru_saved : nullptr, save ? base + l.gru_stats : nullptr, net->gru_products,
                                  net->gru_dense_products))
        return -1;
    } else {
      const int b = j < nb ? j : j - 1;   // the block's number: base blocks, then head blocks
      const float* const* q = j < nb ? p + ix.base + 4 * j : p + ix.head + 4 * (j - nb - 1);
      if (ac_mlp_block_forward_p(device_id, stream, M, j == 0 ? net->obs_dim : nett::H, net->block_eps[b], x, q[0], q[1], q[2], q[3], out,
                                 save ? base + l.stats[b] : nullptr, net->mlp_products))
        return -1;
    }
    x = out;
  }
  if (!actor) return ac_value_head_forward(device_id, stream, M, x, p[ix.out], p[ix.out + 1], o0);
  const float *w[9], *b[9];
  for (int h = 0; 2 * h < ix.count - ix.out; ++h) {
    w[h] = p[ix.out + 2 * h];
    b[h] = p[ix.out + 2 * h + 1];
  }
  return ac_act_eval_forward(device_id, stream, &net->heads, M, x, w, b, d_actions, alpha0, beta0, o0, o1);
}

// One network backward. Actor: g0 = dlogp, g1 = dent [M], either may be NULL. Critic: g0 = dvalues [M], g1 = dh_T [N, 128] or NULL.
// Every parameter's gradient is written to d_grads[i], i as in the parameter table.
static int net_backward(const char* who, bool want_actor, int32_t device_id, void* stream, const ac_net_t* net, int32_t N, int32_t T, const float* g0,
                        const float* g1, const float* d_obs, const float* d_hxs, const float* d_masks, const float* d_actions,
                        const float* d_saved, float* d_workspace, float* const* d_grads) {
  bool actor;
  if (net_ok(who, net, N, T, true, &actor)) return -1;
  if (actor != want_actor) return fail(std::string(who) + (want_actor ? ": the description has no action heads" : ": the description has action heads"));
  if (!d_obs || !d_hxs || !d_masks || (actor && !d_actions) || !d_saved || !d_workspace || !d_grads || (!actor && !g0))
    return fail(std::string(who) + ": null argument");
  if (!trn::aligned16({d_workspace, d_saved})) return fail(std::string(who) + ": workspace and saved must be 16-byte aligned");
  const nett::Index ix = nett::index(net);
  for (int i = 0; i < ix.count; ++i)
    if (!d_grads[i]) return fail(std::string(who) + ": null gradient " + std::to_string(i));
  const int32_t M = N * T;
  const nett::Layout l = nett::layout(net, M, true);
  const net_bwd_ws_t b = net_bwd_ws(net, N, T, actor);
  float *cur = d_workspace + b.g0, *other = d_workspace + b.g1, *dxn = d_workspace + b.dxn, *lws = d_workspace + b.layer;
  const float* const* p = net->params;
  const int nb = net->base_blocks, nh = net->head_blocks;
  const float* x = d_saved + l.out[nb + nh];
  if (actor) {
    const float *w[9], *bb[9];
    float *dw[9], *db[9];
    for (int h = 0; 2 * h < ix.count - ix.out; ++h) {
      w[h] = p[ix.out + 2 * h];
      bb[h] = p[ix.out + 2 * h + 1];
      dw[h] = d_grads[ix.out + 2 * h];
      db[h] = d_grads[ix.out + 2 * h + 1];
    }
    const bool shoot = net->heads.n_shoot_cols != 0;
    if (ac_act_eval_backward(device_id, stream, &net->heads, M, g0, g1, x, w, bb, d_actions, shoot ? d_saved + l.alpha0 : nullptr,
                             shoot ? d_saved + l.beta0 : nullptr, lws, cur, dw, db))
      return -1;
  } else if (ac_value_head_backward(device_id, stream, M, g0, x, p[ix.out], lws, cur, d_grads[ix.out], d_grads[ix.out + 1])) {
    return -1;
  }
  for (int j = nb + nh; j >= 0; --j) {   // stage j's upstream gradient is in cur; its input's goes to other
    const float* in = j ? d_saved + l.out[j - 1] : (net->feature_norm ? d_saved + l.xn : d_obs);
    if (j == nb) {
      const float* const* q = p + ix.gru;
      float* const* dq = d_grads + ix.gru;
      if (ac_gru_layer_backward_pd(device_id, stream, N, T, cur, actor ? nullptr : g1, in, d_hxs, d_masks, q[0], q[1], q[4], d_saved + l.gru_y,
                                   d_saved + l.gru_saved, d_saved + l.gru_stats, lws, other, nullptr, dq[0], dq[1], dq[2], dq[3], dq[4], dq[5],
                                   net->gru_products, net->gru_dense_products))
        return -1;
    } else {
      const int blk = j < nb ? j : j - 1;
      const int o = j < nb ? ix.base + 4 * j : ix.head + 4 * (j - nb - 1);
      float* dx = j ? other : (net->feature_norm ? dxn : nullptr);   // the observation takes no gradient
      if (ac_mlp_block_backward_p(device_id, stream, M, j == 0 ? net->obs_dim : nett::H, cur, in, p[o], p[o + 1], p[o + 2], d_saved + l.stats[blk],
                                  lws, dx, d_grads[o], d_grads[o + 1], d_grads[o + 2], d_grads[o + 3], net->mlp_products))
        return -1;
    }
    float* t = cur;
    cur = other;
    other = t;
  }
  if (net->feature_norm)
    return ac_feature_norm_backward(device_id, stream, M, net->obs_dim, dxn, d_obs, p[0], d_saved + l.fn_stats, lws, nullptr, d_grads[0], d_grads[1]);
  return 0;
}

int ac_actor_eval_forward(int32_t device_id, void* stream, const ac_net_t* net, int32_t N, int32_t T, const float* d_obs, const float* d_hxs,
                          const float* d_masks, const float* d_actions, float* d_workspace, float* d_saved, float* d_logp, float* d_ent) {
  return net_forward("ac_actor_eval_forward", true, device_id, stream, net, N, T, d_obs, d_hxs, d_masks, d_actions, d_workspace, d_saved, d_logp,
                     d_ent);
}
int ac_actor_eval_backward(int32_t device_id, void* stream, const ac_net_t* net, int32_t N, int32_t T, const float* d_dlogp, const float* d_dent,
                           const float* d_obs, const float* d_hxs, const float* d_masks, const float* d_actions, const float* d_saved,
                           float* d_workspace, float* const* d_grads) {
  return net_backward("ac_actor_eval_backward", true, device_id, stream, net, N, T, d_dlogp, d_dent, d_obs, d_hxs, d_masks, d_actions, d_saved,
                      d_workspace, d_grads);
}
int ac_critic_forward(int32_t device_id, void* stream, const ac_net_t* net, int32_t N, int32_t T, const float* d_obs, const float* d_hxs,
                      const float* d_masks, float* d_workspace, float* d_saved, float* d_values, float* d_h_T) {
  return net_forward("ac_critic_forward", false, device_id, stream, net, N, T, d_obs, d_hxs, d_masks, nullptr, d_workspace, d_saved, d_values,
                     d_h_T);
}
int ac_critic_backward(int32_t device_id, void* stream, const ac_net_t* net, int32_t N, int32_t T, const float* d_dvalues, const float* d_dh_T,
                       const float* d_obs, const float* d_hxs, const float* d_masks, const float* d_saved, float* d_workspace,
                       float* const* d_grads) {
  return net_backward("ac_critic_backward", false, device_id, stream, net, N, T, d_dvalues, d_dh_T, d_obs, d_hxs, d_masks, nullptr, d_saved,
                      d_workspace, d_grads);
}
}  // extern "C"
