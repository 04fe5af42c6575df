// The PPO update's MLP layers on the device ("The training MLP blocks"): one block of the reference's MLPLayer
// (algorithms/utils/mlp.py), y = LayerNorm_128(relu(x Wᵀ + b)) * gamma + beta with x [M, K], W [128, K], fp32 everywhere, forward and
// backward, each one launch over all M rows (plus a small fixed-order sum of the parameter-gradient partials).
//
// A workgroup of eight waves walks 32-row tiles in a persistent loop. Wave w owns output units 16 w .. 16 w + 15 and keeps its slice of
// W in registers for the whole loop as fp32 operands of v_mfma_f32_16x16x4_f32 (exact fp32 products and sums, as in gru_train.hpp);
// the x tile is the A operand, read from LDS as float4 with the k order permuted (lane quarter q takes k = KP/4 q + s) so the reads are
// contiguous. K is zero-padded on chip to KP = 16, 32, 64, 128 or 256, one instantiation each. The next tile's rows are asked for into
// registers before the current tile's products, so the loads fly behind the MFMAs.
//
// Forward: relu(z) goes to an LDS tile, then each wave normalises four whole rows (two columns per lane, wave-wide sums) and writes
// them as contiguous 512-byte rows; z and relu(z) never reach HBM, the row's mean and 1/std do (8 bytes) when a backward will follow.
//
// Backward: z is recomputed from x (one more product instead of two saved [M, 128] tensors). Everything elementwise then stays in the
// product's result layout (row 4 q + i, unit 16 w + lane % 16): the two row sums of the LayerNorm backward cross the waves through a
// 2 KiB LDS table, and dz in that layout IS the A operand of dW = dzᵀ x (the step that sums rows {4 q + i} takes register i), whose
// 128 x KP result stays in the accumulators of the wave that owns the units for the whole persistent loop. dx = dz W takes dz through
// LDS once (the sum runs over units there) against a transposed register slice of W. Each workgroup ends by writing its share of dW,
// db, dgamma, dbeta to the workspace; mlp_block_reduce adds the shares in a fixed order. No floating-point atomics anywhere.
#pragma once

namespace mlpt {
typedef float floatx4 __attribute__((ext_vector_type(4)));
constexpr int H = 128;          // out-features, the LayerNorm's width
constexpr int RT = 32;          // rows per tile: two 16-row M-tiles, two independent accumulators per product
constexpr int HP = H + 4;       // LDS row stride (4 mod 64 banks: float4 reads of 16 rows and dword reads of rows 4 q + i stay conflict-free)
constexpr int KMAX = 256;
constexpr int FWD_WGS = 512;    // persistent workgroups at most (two per CU fit the forward's registers and LDS)
constexpr int BWD_WGS = 256;    // and for the backward: also the number of partial sets the reduce kernel adds

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float sum16(float v) {   // over the 16 lanes of a quarter
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// rows row0 .. row0 + RT - 1 of src [M, K] into registers, as the [RT][KP] tile store_tile lays out; rows >= M and columns >= K are 0.
// vec: K == KP and src 16-byte aligned, so whole float4s are loaded (KP >= 64 only: a thread then owns at least one).
template <int KP>
__device__ __forceinline__ void load_tile(float (&v)[RT * KP / 512], const float* __restrict__ src, int K, int M, int row0, int tid, int vec) {
  constexpr int E = RT * KP / 512;
  if constexpr (E >= 4) {
    if (vec) {
#pragma unroll
      for (int j = 0; j < E / 4; ++j) {
        const int f = tid + 512 * j, r = f / (KP / 4), c = 4 * (f % (KP / 4));
        float4 t = {0.0f, 0.0f, 0.0f, 0.0f};
        if (row0 + r < M) t = *reinterpret_cast<const float4*>(src + (size_t)(row0 + r) * KP + c);
        v[4 * j] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
      }
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int e = tid + 512 * j, r = e / KP, c = e % KP;
    v[j] = (row0 + r < M && c < K) ? src[(size_t)(row0 + r) * K + c] : 0.0f;
  }
}
template <int KP>
__device__ __forceinline__ void store_tile(const float (&v)[RT * KP / 512], float (*lds)[KP + 4], int tid, int vec) {
  constexpr int E = RT * KP / 512;
  if constexpr (E >= 4) {
    if (vec) {
#pragma unroll
      for (int j = 0; j < E / 4; ++j) {
        const int f = tid + 512 * j, r = f / (KP / 4), c = 4 * (f % (KP / 4));
        *reinterpret_cast<float4*>(&lds[r][c]) = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
      }
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int e = tid + 512 * j;
    lds[e / KP][e % KP] = v[j];
  }
}

// z (without the bias) of the tile in xs for this wave's 16 units: acc[mt][i] = row 16 mt + 4 q + i
template <int KP>
__device__ __forceinline__ void tile_product(floatx4 (&acc)[2], const float (*xs)[KP + 4], const float (&B)[KP / 4], int n, int q) {
  constexpr int KQ = KP / 4;
  acc[0] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
  acc[1] = acc[0];
#pragma unroll
  for (int s = 0; s < KQ; s += 4) {
    const float4 a0 = *reinterpret_cast<const float4*>(&xs[n][KQ * q + s]);
    const float4 a1 = *reinterpret_cast<const float4*>(&xs[16 + n][KQ * q + s]);
    const float v0[4] = {a0.x, a0.y, a0.z, a0.w}, v1[4] = {a1.x, a1.y, a1.z, a1.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0[j], B[s + j], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1[j], B[s + j], acc[1], 0, 0, 0);
    }
  }
}

// y [M, 128]; stats [M, 2] = (mean, 1 / sqrt(var + eps)) of relu(z) per row, or NULL (inference: nothing kept)
template <int KP>
__global__ __launch_bounds__(512) void mlp_block_fwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ y,
                                                     float* __restrict__ stats, int M, int K, float eps, int vec) {
  constexpr int KQ = KP / 4;
  __shared__ __attribute__((aligned(16))) float xs[RT][KP + 4];
  __shared__ __attribute__((aligned(16))) float as[RT][HP];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
  const int u = 16 * wv + n;
  float B[KQ];   // W[u][k = KQ q + s]
#pragma unroll
  for (int s = 0; s < KQ; ++s) {
    const int k = KQ * q + s;
    B[s] = k < K ? w[(size_t)u * K + k] : 0.0f;
  }
  const float bias = b[u];
  const float g0 = gamma[lane], g1 = gamma[lane + 64], be0 = beta[lane], be1 = beta[lane + 64];
  const int ntiles = (M + RT - 1) / RT;
  float pre[RT * KP / 512];
  int tile = blockIdx.x;
  if (tile < ntiles) load_tile<KP>(pre, x, K, M, tile * RT, tid, vec);
  for (; tile < ntiles; tile += gridDim.x) {
    store_tile<KP>(pre, xs, tid, vec);
    __syncthreads();
    const int next = tile + gridDim.x;
    if (next < ntiles) load_tile<KP>(pre, x, K, M, next * RT, tid, vec);
    floatx4 acc[2];
    tile_product<KP>(acc, xs, B, n, q);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float z = acc[mt][i] + bias;
        as[16 * mt + 4 * q + i][u] = z > 0.0f ? z : 0.0f;
      }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = 4 * wv + j, row = tile * RT + r;
      const float a0 = as[r][lane], a1 = as[r][lane + 64];
      const float mean = wave_sum(a0 + a1) * (1.0f / H);
      const float d0 = a0 - mean, d1 = a1 - mean;
      const float var = wave_sum(d0 * d0 + d1 * d1) * (1.0f / H);
      const float rstd = 1.0f / sqrtf(var + eps);
      if (row < M) {
        y[(size_t)row * H + lane] = (d0 * rstd) * g0 + be0;
        y[(size_t)row * H + lane + 64] = (d1 * rstd) * g1 + be1;
        if (stats && lane < 2) stats[(size_t)row * 2 + lane] = lane ? rstd : mean;
      }
    }
  }
}

// One set of partial sums per workgroup at ws + blockIdx.x * (128 K + 384): dW [128, K], db, dgamma, dbeta [128].
// DX: dx [M, K] is wanted; without it the dz W product, dz's trip through LDS and the transposed slice of W (32 or 64 registers) are
// not there at all (the first block of a trunk: its input is the observation).
template <int KP, bool DX>
__global__ __launch_bounds__(512) void mlp_block_bwd(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ b, const float* __restrict__ gamma,
                                                     const float* __restrict__ stats, float* __restrict__ ws, float* __restrict__ dx,
                                                     int M, int K, int vecx, int vecdy) {
  constexpr int KQ = KP / 4;
  constexpr int NJ = KP / 16;                   // 16-column tiles of dW per wave (all of them: the wave owns 16 rows of dW)
  constexpr bool PREX = KP < 256;               // at KP = 256 the registers go to W and dW: the x tile is loaded where it is needed
  constexpr int ND = KP > 128 ? KP / 128 : 1;   // 16-column tiles of dx per wave (wave w: columns 16 w + 128 jd + n; idle when 16 w >= KP)
  __shared__ __attribute__((aligned(16))) float xs[RT][KP + 4];
  __shared__ __attribute__((aligned(16))) float dys[RT][HP];
  __shared__ __attribute__((aligned(16))) float dzs[RT][HP];
  __shared__ __attribute__((aligned(16))) float part[RT][8][2];   // per row and wave: the sums over the wave's 16 units of g and g * a_hat
  __shared__ float st[RT][2];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
  const int u = 16 * wv + n;
  float B[KQ];   // W[u][k = KQ q + s]: the recomputed z
#pragma unroll
  for (int s = 0; s < KQ; ++s) {
    const int k = KQ * q + s;
    B[s] = k < K ? w[(size_t)u * K + k] : 0.0f;
  }
  const bool do_dx = DX && 16 * wv < KP;
  // W[unit 32 q + s][column 16 w + 128 jd + n]: dx = dz W sums over units. (KP = 256 with dx is the one instantiation that does not
  // fit the 256 VGPRs and spills; no shipped policy runs it: their wide first blocks take observations and want no dx.)
  float Bx[ND][32];
#pragma unroll
  for (int jd = 0; jd < ND; ++jd)
#pragma unroll
    for (int s = 0; s < 32; ++s) {
      const int kc = 16 * wv + 128 * jd + n;
      Bx[jd][s] = (do_dx && kc < K) ? w[(size_t)(32 * q + s) * K + kc] : 0.0f;
    }
  const float bias = b[u], gam = gamma[u];
  floatx4 accw[NJ];   // dW[unit 16 w + 4 q + i][column 16 j + n], summed over every row this workgroup walks
#pragma unroll
  for (int j = 0; j < NJ; ++j) accw[j] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
  float dgam = 0.0f, dbet = 0.0f, dbias = 0.0f;
  const int ntiles = (M + RT - 1) / RT;
  float prex[RT * KP / 512], pred[RT * H / 512], pres = 0.0f;
  int tile = blockIdx.x;
  if (tile < ntiles) {
    if constexpr (PREX) load_tile<KP>(prex, x, K, M, tile * RT, tid, vecx);
    load_tile<H>(pred, dy, H, M, tile * RT, tid, vecdy);
    if (tid < 2 * RT) pres = (tile * RT + tid / 2 < M) ? stats[(size_t)tile * RT * 2 + tid] : 0.0f;
  }
  for (; tile < ntiles; tile += gridDim.x) {
    const int row0 = tile * RT;
    if constexpr (!PREX) load_tile<KP>(prex, x, K, M, row0, tid, vecx);
    store_tile<KP>(prex, xs, tid, vecx);
    store_tile<H>(pred, dys, tid, vecdy);
    if (tid < 2 * RT) st[tid / 2][tid % 2] = pres;
    __syncthreads();
    const int next = tile + gridDim.x;
    if (next < ntiles) {
      if constexpr (PREX) load_tile<KP>(prex, x, K, M, next * RT, tid, vecx);
      load_tile<H>(pred, dy, H, M, next * RT, tid, vecdy);
      if (tid < 2 * RT) pres = (next * RT + tid / 2 < M) ? stats[(size_t)next * RT * 2 + tid] : 0.0f;
    }
    floatx4 acc[2];
    tile_product<KP>(acc, xs, B, n, q);
    // rows past M have x = 0, dy = 0 and stats = 0: a_hat, g and dz come out 0 and add nothing to any sum
    float g[2][4], ah[2][4], rs[2][4];
    bool pos[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 16 * mt + 4 * q + i;
        const float z = acc[mt][i] + bias;
        pos[mt][i] = z > 0.0f;   // a tie at 0 gets no gradient, as torch's threshold_backward
        const float a = pos[mt][i] ? z : 0.0f;
        rs[mt][i] = st[r][1];
        ah[mt][i] = (a - st[r][0]) * rs[mt][i];
        const float d = dys[r][u];
        g[mt][i] = d * gam;
        dgam += d * ah[mt][i];
        dbet += d;
        const float s1 = sum16(g[mt][i]);
        const float s2 = sum16(g[mt][i] * ah[mt][i]);
        if (n == 0) {
          part[r][wv][0] = s1;
          part[r][wv][1] = s2;
        }
      }
    __syncthreads();
    float dz[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 16 * mt + 4 * q + i;
        float m1 = 0.0f, m2 = 0.0f;
#pragma unroll
        for (int p = 0; p < 8; p += 2) {   // the eight waves' shares, in wave order
          const float4 t = *reinterpret_cast<const float4*>(&part[r][p][0]);
          m1 += t.x; m2 += t.y;
          m1 += t.z; m2 += t.w;
        }
        m1 *= 1.0f / H;
        m2 *= 1.0f / H;
        const float da = rs[mt][i] * (g[mt][i] - m1 - ah[mt][i] * m2);
        dz[mt][i] = pos[mt][i] ? da : 0.0f;
        dbias += dz[mt][i];
        if (DX) dzs[r][u] = dz[mt][i];
      }
    // dW += dz^T x: the step over rows {4 q + i} takes A = dz register i (unit on lane % 16, row on the quarter) and B = x[row][16 j + n]
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float* xr = &xs[16 * mt + 4 * q + i][n];
#pragma unroll
        for (int j = 0; j < NJ; ++j) accw[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(dz[mt][i], xr[16 * j], accw[j], 0, 0, 0);
      }
    __syncthreads();   // dzs complete; and every read of xs, dys, st, part of this tile is behind
    if (do_dx) {   // (false at compile time without DX)
      floatx4 ad[2][ND];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int jd = 0; jd < ND; ++jd) ad[mt][jd] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int s = 0; s < 32; s += 4) {
        const float4 a0 = *reinterpret_cast<const float4*>(&dzs[n][32 * q + s]);
        const float4 a1 = *reinterpret_cast<const float4*>(&dzs[16 + n][32 * q + s]);
        const float v0[4] = {a0.x, a0.y, a0.z, a0.w}, v1[4] = {a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int jd = 0; jd < ND; ++jd) {
            ad[0][jd] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0[j], Bx[jd][s + j], ad[0][jd], 0, 0, 0);
            ad[1][jd] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1[j], Bx[jd][s + j], ad[1][jd], 0, 0, 0);
          }
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int jd = 0; jd < ND; ++jd)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int row = row0 + 16 * mt + 4 * q + i, kc = 16 * wv + 128 * jd + n;
            if (row < M && kc < K) dx[(size_t)row * K + kc] = ad[mt][jd][i];
          }
    }
  }
  float* base = ws + (size_t)blockIdx.x * (H * K + 3 * H);
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = 16 * j + n;
      if (k < K) base[(size_t)(16 * wv + 4 * q + i) * K + k] = accw[j][i];
    }
  // the four quarters hold different rows' shares of the same unit
  dbias += __shfl_xor(dbias, 16); dbias += __shfl_xor(dbias, 32);
  dgam += __shfl_xor(dgam, 16); dgam += __shfl_xor(dgam, 32);
  dbet += __shfl_xor(dbet, 16); dbet += __shfl_xor(dbet, 32);
  if (q == 0) {
    base[H * K + u] = dbias;
    base[H * K + H + u] = dgam;
    base[H * K + 2 * H + u] = dbet;
  }
}

// dW, db, dgamma, dbeta = the sum of the G partial sets (trn::sum_sets)
__global__ __launch_bounds__(256) void mlp_block_reduce(const float* __restrict__ ws, int G, int K, float* __restrict__ dw, float* __restrict__ db,
                                                        float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int nel = H * K + 3 * H;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nel) return;
  const float s = trn::sum_sets(ws, G, nel, e);
  const int v = e - H * K;
  if (v < 0) dw[e] = s;
  else if (v < H) db[v] = s;
  else if (v < 2 * H) dgamma[v - H] = s;
  else dbeta[v - 2 * H] = s;
}
}  // namespace mlpt

// ------------------------------------------------------------------------------------------------ C ABI (include/aircombat.h)
extern "C" {
static int mlp_shape_ok(const char* who, int32_t M, int32_t K) {
  if (M < 1) return fail(std::string(who) + ": M must be at least 1");
  if (K < 1 || K > mlpt::KMAX) return fail(std::string(who) + ": K must be 1 .. 256");
  return trn::rows_fit_i32(who, M, mlpt::H, mlpt::RT);
}
static int mlp_kp(int32_t K) { return K <= 16 ? 16 : K <= 32 ? 32 : K <= 64 ? 64 : K <= 128 ? 128 : 256; }
static int mlp_vec(const void* p, int32_t K, int kp) { return K == kp && kp >= 64 && trn::aligned16(p); }

int64_t ac_mlp_block_workspace_floats(int32_t M, int32_t K) {
  if (mlp_shape_ok("ac_mlp_block_workspace_floats", M, K)) return -1;
  return (int64_t)trn::capped_tiles(M, mlpt::RT, mlpt::BWD_WGS) * (mlpt::H * K + 3 * mlpt::H);
}

int ac_mlp_block_forward(int32_t device_id, void* stream, int32_t M, int32_t K, float eps, const float* d_x, const float* d_w, const float* d_b,
                         const float* d_gamma, const float* d_beta, float* d_y, float* d_stats) {
  if (!d_x || !d_w || !d_b || !d_gamma || !d_beta || !d_y) return fail("ac_mlp_block_forward: null argument");
  if (mlp_shape_ok("ac_mlp_block_forward", M, K)) return -1;
  HIP_OK(hipSetDevice(device_id));
  const int kp = mlp_kp(K);
  const dim3 grid(trn::capped_tiles(M, mlpt::RT, mlpt::FWD_WGS)), block(512);
  const int vec = mlp_vec(d_x, K, kp);
#define AC_MLP_FWD(KP)                                                                                                                      \
  hipLaunchKernelGGL(mlpt::mlp_block_fwd<KP>, grid, block, 0, (hipStream_t)stream, d_x, d_w, d_b, d_gamma, d_beta, d_y, d_stats, (int)M, \
                     (int)K, eps, vec)
  switch (kp) {
    case 16: AC_MLP_FWD(16); break;
    case 32: AC_MLP_FWD(32); break;
    case 64: AC_MLP_FWD(64); break;
    case 128: AC_MLP_FWD(128); break;
    default: AC_MLP_FWD(256); break;
  }
#undef AC_MLP_FWD
  HIP_OK(hipGetLastError());
  return 0;
}

int ac_mlp_block_backward(int32_t device_id, void* stream, int32_t M, int32_t K, const float* d_dy, const float* d_x, const float* d_w,
                          const float* d_b, const float* d_gamma, const float* d_stats, float* d_workspace, float* d_dx, float* d_dw,
                          float* d_db, float* d_dgamma, float* d_dbeta) {
  if (!d_dy || !d_x || !d_w || !d_b || !d_gamma || !d_stats || !d_workspace || !d_dw || !d_db || !d_dgamma || !d_dbeta)
    return fail("ac_mlp_block_backward: null argument");
  if (mlp_shape_ok("ac_mlp_block_backward", M, K)) return -1;
  HIP_OK(hipSetDevice(device_id));
  const int kp = mlp_kp(K), G = trn::capped_tiles(M, mlpt::RT, mlpt::BWD_WGS);
  const dim3 grid(G), block(512);
  const int vecx = mlp_vec(d_x, K, kp), vecdy = mlp_vec(d_dy, mlpt::H, mlpt::H);
#define AC_MLP_BWD(KP)                                                                                                                        \
  if (d_dx)                                                                                                                                   \
    hipLaunchKernelGGL((mlpt::mlp_block_bwd<KP, true>), grid, block, 0, (hipStream_t)stream, d_dy, d_x, d_w, d_b, d_gamma, d_stats, d_workspace, \
                       d_dx, (int)M, (int)K, vecx, vecdy);                                                                                        \
  else                                                                                                                                        \
    hipLaunchKernelGGL((mlpt::mlp_block_bwd<KP, false>), grid, block, 0, (hipStream_t)stream, d_dy, d_x, d_w, d_b, d_gamma, d_stats, d_workspace, \
                       d_dx, (int)M, (int)K, vecx, vecdy)
  switch (kp) {
    case 16: AC_MLP_BWD(16); break;
    case 32: AC_MLP_BWD(32); break;
    case 64: AC_MLP_BWD(64); break;
    case 128: AC_MLP_BWD(128); break;
    default: AC_MLP_BWD(256); break;
  }
#undef AC_MLP_BWD
  HIP_OK(hipGetLastError());
  const int nel = mlpt::H * K + 3 * mlpt::H;
  hipLaunchKernelGGL(mlpt::mlp_block_reduce, dim3((nel + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)d_workspace, G, (int)K, d_dw,
                     d_db, d_dgamma, d_dbeta);
  HIP_OK(hipGetLastError());
  return 0;
}
}  // extern "C"
