// The training MLP blocks (mlp_train.hpp) with their three products on the bf16 matrix path ("The training MLP blocks"):
// the opt-in form `products` = AC_PRODUCTS_BF16X3. mlp_block_fwd_b3 and mlp_block_bwd_b3 take the arguments of mlp_block_fwd and
// mlp_block_bwd and write the same outputs to the same places: 32-row tiles, a persistent loop with the next tile asked for into
// registers before the current tile's products, the same (row, unit) ownership (wave w owns units 16 w .. 16 w + 15, lane (q, n) rows
// 16 mt + 4 q + i), and for the backward the same partial sets in the same layout, so mlp_block_reduce, the workspace and
// ac_mlp_block_workspace_floats are shared.
//
// The product is bf16x3.hpp's. K is zero-padded on chip to KP = 128 (a k-step is 32; KPS below). W is split once per workgroup. The
// bias, the ReLU, the LayerNorm statistics and their backward row sums, db, dgamma and dbeta are mlp_train.hpp's fp32 code on unsplit
// values.
//
//   x    split once per tile by the thread that stores it: a thread owns rows 2 rp, 2 rp + 1 and four adjacent columns. The row-major
//        image [32][KP + 8] per plane (272 B rows) is the A operand of z = x Wᵀ. tile_z is the ONE function that forms z, in the
//        forward and in the backward's recomputation: the same pieces, terms, order and accumulator chain, so the backward's ReLU
//        mask is the forward's bit for bit.
//   dW   the sum runs over the tile's rows (k slots), so dz in the product's result layout IS the A operand, split in registers; x
//        is the B operand from the transposed image, which the storing thread writes from the same pieces. One accumulator per
//        result for all six terms, over every row the workgroup walks.
//   dx   dz goes through LDS once as three planes [32][128 + 8] (written in the result layout, read as 16-byte rows) against the
//        pieces of a transposed register slice of W. Three chains per result, one per order of the terms (chains_by_order, and
//        why), one 16-row half of the tile after the other.
// The weight slices here are guarded (k < K, and 0 beyond K in a column), so they stay in this file: folding them into
// b3::row_slice / col_slice would put a run-time test into the GRU kernels. An aligned, unpadded row takes b3::read8.
// No floating-point atomics: results are bit-identical from run to run.
#pragma once

namespace mlps {
using mlpt::floatx4; using mlpt::H; using mlpt::RT; using mlpt::HP; using mlpt::wave_sum; using mlpt::sum16;
constexpr int KR = RT + 8;   // k slots per column of the transposed x image
constexpr int KZ = H + 8;    // bf16 per plane row of the dz tile
// The KP values AC_PRODUCTS_BF16X3 runs split (ac_mlp_block_constant(3)). A forward and its backward must form z the same way, so a KP
// is in only when its forward and both its backwards met the condition of profiles/mlp_split_bench.txt (measured with 32 | 64 | 128
// here): KP = 128 did, 0.67 - 0.71 / 0.79 / 0.84 of the fp32 kernels' time; KP = 64 without dx tied (0.170 ms both) and KP = 32 was slower
// than the fp32 form (which pads K <= 16 to 16 only). Those two were removed; the kernels below are instantiated for KP = 128 alone.
constexpr int KPS = 128;

// this thread's share of an x tile: rows 2 rp and 2 rp + 1, columns CW cq .. CW cq + CW - 1
template <int KP>
struct Patch {
  static constexpr int CW = KP / 32;
  static_assert(CW == 4, "512 threads own 16 row pairs x 32 column groups of four: KP = 128");
  static constexpr int KS = KP + 8, PLN = RT * KS, PLNT = KP * KR;
  float v[2][CW];

  // rows >= M and columns >= K are 0. vec: K == KP and src 16-byte aligned
  __device__ __forceinline__ void load(const float* __restrict__ src, int K, int M, int row0, int tid, int vec) {
    const int rp = tid & 15, cq = tid >> 4, c = CW * cq;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int row = row0 + 2 * rp + k;
#pragma unroll
      for (int e = 0; e < CW; ++e) v[k][e] = 0.0f;
      if (row < M) {
        if (vec) {
          const float4 t = *reinterpret_cast<const float4*>(src + (size_t)row * KP + c);
          v[k][0] = t.x; v[k][1] = t.y; v[k][2] = t.z; v[k][3] = t.w;
        } else {
#pragma unroll
          for (int e = 0; e < CW; ++e)
            if (c + e < K) v[k][e] = src[(size_t)row * K + c + e];
        }
      }
    }
  }

  // split and store: the row-major image xr [3][RT][KS] and, with TR, the transposed one xt [3][KP][KR]
  template <bool TR>
  __device__ __forceinline__ void store(unsigned short* xr, unsigned short* xt, int tid) const {
    const int rp = tid & 15, cq = tid >> 4, c = CW * cq;
    unsigned w[2][CW / 2][3];
#pragma unroll
    for (int k = 0; k < 2; ++k) b3::split_row(w[k], v[k]);
#pragma unroll
    for (int k = 0; k < 2; ++k) b3::store_words(xr + (2 * rp + k) * KS + c, PLN, w[k]);
    if constexpr (TR) {
#pragma unroll
      for (int e = 0; e < CW; ++e) {
        unsigned pair[3];   // column c + e of both rows, from the words that hold columns (c + e) & ~1 and the next
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          const unsigned w0 = w[0][e / 2][p], w1 = w[1][e / 2][p];
          pair[p] = (e & 1) ? ((w0 >> 16) | (w1 & 0xffff0000u)) : ((w0 & 0xffffu) | (w1 << 16));
        }
        b3::store_pair(xt, PLNT, KR, c + e, rp, pair);
      }
    }
  }
};

// B[s] = the pieces of W[u][k = 32 s + 8 q + e], 0 beyond K. vec: K == KP and w 16-byte aligned
template <int KP>
__device__ __forceinline__ void load_w(uint4 (&B)[KP / 32][3], const float* __restrict__ w, int K, int u, int q, int vec) {
#pragma unroll
  for (int s = 0; s < KP / 32; ++s) {
    const int k0 = 32 * s + 8 * q;
    float v[8];
    if (vec) {
      b3::read8(v, w + (size_t)u * KP + k0);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = k0 + e < K ? w[(size_t)u * K + k0 + e] : 0.0f;
    }
    b3::split8(v, B[s]);
  }
}

// z (without the bias) of the tile in xr for this wave's 16 units: acc[mt][i] = row 16 mt + 4 q + i. The forward and the backward both
// form z here and nowhere else.
template <int KP>
__device__ __forceinline__ void tile_z(floatx4 (&acc)[2], const unsigned short* xr, const uint4 (&B)[KP / 32][3], int n, int q) {
  constexpr int KS = KP + 8, PLN = RT * KS;
  acc[0] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
  acc[1] = acc[0];
  const unsigned short* arow = xr + n * KS + 8 * q;
#pragma unroll
  for (int s = 0; s < KP / 32; ++s) {
    uint4 A[2][3];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) b3::read3(A[mt], arow + 16 * mt * KS + 32 * s, PLN);
    b3::one_chain([&](int i, int j) {
      acc[0] = b3::mf(A[0][i], B[s][j], acc[0]);
      acc[1] = b3::mf(A[1][i], B[s][j], acc[1]);
    });
  }
}

template <int KP>
__global__ __launch_bounds__(512) void mlp_block_fwd_b3(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ y,
                                                        float* __restrict__ stats, int M, int K, float eps, int vecx, int vecw) {
  __shared__ __attribute__((aligned(16))) unsigned short xr[3][RT][KP + 8];
  __shared__ __attribute__((aligned(16))) float as[RT][HP];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
  const int u = 16 * wv + n;
  uint4 B[KP / 32][3];
  load_w<KP>(B, w, K, u, q, vecw);
  const float bias = b[u];
  const float g0 = gamma[lane], g1 = gamma[lane + 64], be0 = beta[lane], be1 = beta[lane + 64];
  const int ntiles = (M + RT - 1) / RT;
  Patch<KP> pre;
  int tile = blockIdx.x;
  if (tile < ntiles) pre.load(x, K, M, tile * RT, tid, vecx);
  for (; tile < ntiles; tile += gridDim.x) {
    pre.template store<false>(&xr[0][0][0], nullptr, tid);
    __syncthreads();
    const int next = tile + gridDim.x;
    if (next < ntiles) pre.load(x, K, M, next * RT, tid, vecx);
    floatx4 acc[2];
    tile_z<KP>(acc, &xr[0][0][0], B, n, q);
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

// Partial sets as mlp_block_bwd: one per workgroup at ws + blockIdx.x * (128 K + 384): dW [128, K], db, dgamma, dbeta [128].
template <int KP, bool DX>
__global__ __launch_bounds__(512) void mlp_block_bwd_b3(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ b, const float* __restrict__ gamma,
                                                        const float* __restrict__ stats, float* __restrict__ ws, float* __restrict__ dx,
                                                        int M, int K, int vecx, int vecw) {
  constexpr int NJ = KP / 16;   // 16-column tiles of dW per wave
  constexpr int PLNT = KP * KR, PLNZ = RT * KZ;
  __shared__ __attribute__((aligned(16))) unsigned short xr[3][RT][KP + 8];
  __shared__ __attribute__((aligned(16))) unsigned short xt[3][KP][KR];
  __shared__ __attribute__((aligned(16))) unsigned short dzs[DX ? 3 : 1][DX ? RT : 1][KZ];
  __shared__ __attribute__((aligned(16))) float part[RT][8][2];   // per row and wave: the sums over the wave's 16 units of g and g * a_hat
  __shared__ float st[RT][2];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
  const int u = 16 * wv + n;
  uint4 B[KP / 32][3];   // the recomputed z
  load_w<KP>(B, w, K, u, q, vecw);
  const int kc = 16 * wv + n;   // this lane's column of dx (the eight waves cover KP = 128)
  uint4 Bx[DX ? 4 : 1][3];      // the pieces of W[unit 32 s + 8 q + e][column kc]: dx = dz W sums over units
  if constexpr (DX) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = kc < K ? w[(size_t)(32 * s + 8 * q + e) * K + kc] : 0.0f;
      b3::split8(v, Bx[s]);
    }
  }
  const float bias = b[u], gam = gamma[u];
  floatx4 accw[NJ];   // dW[unit 16 w + 4 q + i][column 16 j + n], summed over every row this workgroup walks
#pragma unroll
  for (int j = 0; j < NJ; ++j) accw[j] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
  float dgam = 0.0f, dbet = 0.0f, dbias = 0.0f;
  const int ntiles = (M + RT - 1) / RT;
  Patch<KP> prex;
  float pred[2][4], pres = 0.0f;
  auto load = [&](int t) {
    const int row0 = t * RT;
    prex.load(x, K, M, row0, tid, vecx);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = row0 + 16 * mt + 4 * q + i;
        pred[mt][i] = row < M ? dy[(size_t)row * H + u] : 0.0f;
      }
    if (tid < 2 * RT) pres = (row0 + tid / 2 < M) ? stats[(size_t)row0 * 2 + tid] : 0.0f;
  };
  int tile = blockIdx.x;
  if (tile < ntiles) load(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    const int row0 = tile * RT;
    prex.template store<true>(&xr[0][0][0], &xt[0][0][0], tid);
    if (tid < 2 * RT) st[tid / 2][tid % 2] = pres;
    float d[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) d[mt][i] = pred[mt][i];
    __syncthreads();
    const int next = tile + gridDim.x;
    if (next < ntiles) load(next);
    floatx4 acc[2];
    tile_z<KP>(acc, &xr[0][0][0], B, n, q);
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
        g[mt][i] = d[mt][i] * gam;
        dgam += d[mt][i] * ah[mt][i];
        dbet += d[mt][i];
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
    for (int mt = 0; mt < 2; ++mt) {
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
      }
      if constexpr (DX) b3::write_column(&dzs[0][0][0] + (16 * mt + 4 * q) * KZ + u, PLNZ, KZ, dz[mt]);
    }
    // dW += dz^T x: the tile's 32 rows are one k-step; A = the pieces of dz of unit 16 w + n (this lane's k slots), B = the pieces
    // of x[those rows][column 16 c + n] from the transposed image
    {
      float v[8];
      b3::to_kslots(v, dz);
      uint4 A[3];
      b3::split8(v, A);
      const unsigned short* bcol = &xt[0][0][0] + n * KR + 8 * q;
#pragma unroll
      for (int c = 0; c < NJ; c += 2) {
        uint4 Bp[2][3];
#pragma unroll
        for (int h = 0; h < 2; ++h) b3::read3(Bp[h], bcol + 16 * (c + h) * KR, PLNT);
        b3::one_chain([&](int i, int j) {
          accw[c] = b3::mf(A[i], Bp[0][j], accw[c]);
          accw[c + 1] = b3::mf(A[i], Bp[1][j], accw[c + 1]);
        });
      }
    }
    __syncthreads();   // dzs complete; and every read of xr, xt, st, part of this tile is behind
    if constexpr (DX) {
      // dx is summed over rows downstream (dbeta and db of the block before): one chain per order of the terms
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        floatx4 c[3] = {};
        const unsigned short* arow = &dzs[0][0][0] + (16 * mt + n) * KZ + 8 * q;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          uint4 A[3];
          b3::read3(A, arow + 32 * s, PLNZ);
          b3::chains_by_order(c, A, Bx[s]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = row0 + 16 * mt + 4 * q + i;
          if (row < M && kc < K) dx[(size_t)row * K + kc] = b3::chain_sum(c, i);
        }
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
}  // namespace mlps

// ------------------------------------------------------------------------------------------------ C ABI (include/aircombat.h)
extern "C" {
// the KP of the split form (a k-step is 32), or 0 where `products` runs the fp32 kernels: the one place that decides. A KP named in
// mlps::KPS needs its instantiations in the two entries below.
static int mlp_split_kp(int32_t K, int32_t products) {
  const int kp = K <= 32 ? 32 : mlp_kp(K);
  return (products == AC_PRODUCTS_BF16X3 && (mlps::KPS & kp)) ? kp : 0;
}
static_assert(mlps::KPS == 128, "the entries below launch the KP = 128 kernels for every K that mlp_split_kp lets through");
static int mlp_split_vec(const void* p, int32_t K, int kp) { return K == kp && trn::aligned16(p); }

int32_t ac_mlp_block_constant(int32_t which) {
  switch (which) {
    case 0: return mlpt::RT;
    case 1: return mlpt::FWD_WGS;
    case 2: return mlpt::BWD_WGS;
    case 3: return mlps::KPS;
    default: return -1;
  }
}

int ac_mlp_block_forward_p(int32_t device_id, void* stream, int32_t M, int32_t K, float eps, const float* d_x, const float* d_w, const float* d_b,
                           const float* d_gamma, const float* d_beta, float* d_y, float* d_stats, int32_t products) {
  if (trn::products_ok("ac_mlp_block_forward_p", "products", products)) return -1;
  if (!d_x || !d_w || !d_b || !d_gamma || !d_beta || !d_y) return fail("ac_mlp_block_forward_p: null argument");
  if (mlp_shape_ok("ac_mlp_block_forward_p", M, K)) return -1;
  const int kp = mlp_split_kp(K, products);
  if (!kp) return ac_mlp_block_forward(device_id, stream, M, K, eps, d_x, d_w, d_b, d_gamma, d_beta, d_y, d_stats);
  HIP_OK(hipSetDevice(device_id));
  const dim3 grid(trn::capped_tiles(M, mlpt::RT, mlpt::FWD_WGS)), block(512);
  const int vecx = mlp_split_vec(d_x, K, kp), vecw = mlp_split_vec(d_w, K, kp);
  hipLaunchKernelGGL(mlps::mlp_block_fwd_b3<mlps::KPS>, grid, block, 0, (hipStream_t)stream, d_x, d_w, d_b, d_gamma, d_beta, d_y, d_stats,
                     (int)M, (int)K, eps, vecx, vecw);
  HIP_OK(hipGetLastError());
  return 0;
}

int ac_mlp_block_backward_p(int32_t device_id, void* stream, int32_t M, int32_t K, const float* d_dy, const float* d_x, const float* d_w,
                            const float* d_b, const float* d_gamma, const float* d_stats, float* d_workspace, float* d_dx, float* d_dw,
                            float* d_db, float* d_dgamma, float* d_dbeta, int32_t products) {
  if (trn::products_ok("ac_mlp_block_backward_p", "products", products)) return -1;
  if (!d_dy || !d_x || !d_w || !d_b || !d_gamma || !d_stats || !d_workspace || !d_dw || !d_db || !d_dgamma || !d_dbeta)
    return fail("ac_mlp_block_backward_p: null argument");
  if (mlp_shape_ok("ac_mlp_block_backward_p", M, K)) return -1;
  const int kp = mlp_split_kp(K, products);
  if (!kp)
    return ac_mlp_block_backward(device_id, stream, M, K, d_dy, d_x, d_w, d_b, d_gamma, d_stats, d_workspace, d_dx, d_dw, d_db, d_dgamma, d_dbeta);
  HIP_OK(hipSetDevice(device_id));
  const int G = trn::capped_tiles(M, mlpt::RT, mlpt::BWD_WGS);
  const dim3 grid(G), block(512);
  const int vecx = mlp_split_vec(d_x, K, kp), vecw = mlp_split_vec(d_w, K, kp);
  hipLaunchKernelGGL((d_dx ? mlps::mlp_block_bwd_b3<mlps::KPS, true> : mlps::mlp_block_bwd_b3<mlps::KPS, false>), grid, block, 0,
                     (hipStream_t)stream, d_dy, d_x, d_w, d_b, d_gamma, d_stats, d_workspace, d_dx, (int)M, (int)K, vecx, vecw);
  HIP_OK(hipGetLastError());
  const int nel = mlpt::H * K + 3 * mlpt::H;
  hipLaunchKernelGGL(mlpt::mlp_block_reduce, dim3((nel + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)d_workspace, G, (int)K, d_dw,
                     d_db, d_dgamma, d_dbeta);
  HIP_OK(hipGetLastError());
  return 0;
}
}  // extern "C"
