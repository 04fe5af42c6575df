// The training MLP blocks (mlp_train.hpp) with their three products on the bf16 matrix path ("The training MLP blocks"):
// the opt-in form `products` = AC_PRODUCTS_BF16X3. mlp_block_fwd_b3 and mlp_block_bwd_b3 take the arguments of mlp_block_fwd and
// mlp_block_bwd and write the same outputs to the same places: 32-row tiles, a persistent loop with the next tile asked for into
// registers before the current tile's products, the same (row, unit) ownership (wave w owns units 16 w .. 16 w + 15, lane (q, n) rows
// 16 mt + 4 q + i), and for the backward the same partial sets in the same layout, so mlp_block_reduce, the workspace and
// ac_mlp_block_workspace_floats are shared.
//
// The product is gru_train_split.hpp's: every fp32 value is three bf16 pieces (ctls::split3_pair, exact), a product keeps the six terms
// b_i b_j with i + j <= 2 on v_mfma_f32_16x16x32_bf16, smallest first within a k-step, into fp32 accumulators. K is zero-padded on
// chip to KP = 32, 64 or 128 (a k-step is 32; KPS below says which of them AC_PRODUCTS_BF16X3 dispatches). W is read from the caller's fp32 tensor at every call and split in
// registers once per workgroup (12 VGPRs per k-step); nothing is kept between calls. The bias, the ReLU, the LayerNorm statistics and
// their backward row sums, db, dgamma and dbeta are mlp_train.hpp's fp32 code on unsplit values.
//
//   x    split once per tile by the thread that stores it: a thread owns rows 2 rp, 2 rp + 1 and CW adjacent columns. The row-major
//        image [32][KP + 8] per plane (row strides 80, 144, 272 B: 20, 36, 68 dwords, so 16 consecutive rows' 16-byte reads start
//        in 16 different groups of four banks, as the planes of the GRU split kernels) is the A operand of z = x Wᵀ. tile_z is the ONE function that forms z, in the forward and in
//        the backward's recomputation: the same pieces, terms, order and accumulator chain, so the backward's ReLU mask is the
//        forward's bit for bit.
//   dW   the sum runs over the tile's rows: k slot 8 q + e of the instruction is row 16 (e / 4) + 4 q + e % 4 (gru_dw_b3), so dz in
//        the product's result layout IS the A operand, split in registers; x is the B operand from a transposed image [column][k slot]
//        (80 B per column), which the storing thread writes from the same pieces (a row pair of one column is one 32-bit word).
//        One accumulator per result for all six terms, over every row the workgroup walks.
//   dx   dz goes through LDS once as three planes [32][128 + 8] (written in the result layout, read as 16-byte rows) against the
//        pieces of a transposed register slice of W. Three accumulation chains per result, one per order of the terms, added
//        smallest first at the end, one 16-row half of the tile after the other: with all 24 terms in one chain dx came out with a
//        one-sided mean error (-0.044 of its rms error at 4096 x 60, fp32 kernels +0.0002), which the sums over rows downstream
//        (dbeta and db of the block before) collect: dbeta0 read 1.27 of its bound there.
// No floating-point atomics: results are bit-identical from run to run.
#pragma once

namespace mlps {
using mlpt::floatx4; using mlpt::H; using mlpt::RT; using mlpt::HP; using mlpt::wave_sum; using mlpt::sum16;
using grus::mf; using grus::split8;
constexpr int KR = RT + 8;   // k slots per column of the transposed x image
constexpr int KZ = H + 8;    // bf16 per plane row of the dz tile
constexpr int TI[6] = {2, 1, 0, 1, 0, 0}, TJ[6] = {0, 1, 2, 0, 1, 0};   // the six terms (A piece, B piece), smallest first
// The KP values AC_PRODUCTS_BF16X3 runs split (ac_mlp_block_constant(3)). A forward and its backward must form z the same way, so a KP
// is in only when its forward and both its backwards met the condition of profiles/mlp_split_bench.txt (measured with 32 | 64 | 128
// here): KP = 128 did, 0.67 - 0.71 / 0.79 / 0.84 of the fp32 kernels' time; KP = 64 without dx tied (0.170 ms both) and KP = 32 was slower
// than the fp32 form (which pads K <= 16 to 16 only). Their instantiations stay below as the forms that were measured.
constexpr int KPS = 128;

// this thread's share of an x tile: rows 2 rp and 2 rp + 1, columns CW cq .. CW cq + CW - 1 (at KP = 32 half the threads own one)
template <int KP>
struct Patch {
  static constexpr int CW = KP >= 64 ? KP / 32 : 2;
  static constexpr int KS = KP + 8, PLN = RT * KS, PLNT = KP * KR;
  float v[2][CW];

  // rows >= M and columns >= K are 0. vec: K == KP and src 16-byte aligned (then rows are at least 8-byte aligned at every column pair)
  __device__ __forceinline__ void load(const float* __restrict__ src, int K, int M, int row0, int tid, int vec) {
    const int rp = tid & 15, cq = tid >> 4, c = CW * cq;
    if (c >= KP) return;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int row = row0 + 2 * rp + k;
#pragma unroll
      for (int e = 0; e < CW; ++e) v[k][e] = 0.0f;
      if (row < M) {
        if (vec) {
          const float* p = src + (size_t)row * KP + c;
          if constexpr (CW == 2) {
            const float2 t = *reinterpret_cast<const float2*>(p);
            v[k][0] = t.x; v[k][1] = t.y;
          } else {
#pragma unroll
            for (int e = 0; e < CW; e += 4) {
              const float4 t = *reinterpret_cast<const float4*>(p + e);
              v[k][e] = t.x; v[k][e + 1] = t.y; v[k][e + 2] = t.z; v[k][e + 3] = t.w;
            }
          }
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
    if (c >= KP) return;
    unsigned w[2][CW / 2][3];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int e = 0; e < CW / 2; ++e) ctls::split3_pair(v[k][2 * e], v[k][2 * e + 1], w[k][e][0], w[k][e][1], w[k][e][2]);
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        unsigned short* at = xr + p * PLN + (2 * rp + k) * KS + c;
        if constexpr (CW == 2) *reinterpret_cast<unsigned*>(at) = w[k][0][p];
        else if constexpr (CW == 4) *reinterpret_cast<uint2*>(at) = make_uint2(w[k][0][p], w[k][1][p]);
        else *reinterpret_cast<uint4*>(at) = make_uint4(w[k][0][p], w[k][1][p], w[k][2][p], w[k][3][p]);
      }
    if constexpr (TR) {
      const int ks = 8 * ((rp >> 1) & 3) + 4 * (rp >> 3) + 2 * (rp & 1);   // the k slot of row 2 rp; row 2 rp + 1 has the next
#pragma unroll
      for (int e = 0; e < CW; ++e)
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          const unsigned w0 = w[0][e / 2][p], w1 = w[1][e / 2][p];
          const unsigned pair = (e & 1) ? ((w0 >> 16) | (w1 & 0xffff0000u)) : ((w0 & 0xffffu) | (w1 << 16));
          *reinterpret_cast<unsigned*>(xt + p * PLNT + (c + e) * KR + ks) = pair;
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
      const float* p = w + (size_t)u * KP + k0;
      const float4 v0 = *reinterpret_cast<const float4*>(p), v1 = *reinterpret_cast<const float4*>(p + 4);
      v[0] = v0.x; v[1] = v0.y; v[2] = v0.z; v[3] = v0.w; v[4] = v1.x; v[5] = v1.y; v[6] = v1.z; v[7] = v1.w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = k0 + e < K ? w[(size_t)u * K + k0 + e] : 0.0f;
    }
    split8(v, B[s][0], B[s][1], B[s][2]);
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
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int p = 0; p < 3; ++p) A[mt][p] = *reinterpret_cast<const uint4*>(arow + p * PLN + 16 * mt * KS + 32 * s);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      acc[0] = mf(A[0][TI[k]], B[s][TJ[k]], acc[0]);
      acc[1] = mf(A[1][TI[k]], B[s][TJ[k]], acc[1]);
    }
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
  const bool do_dx = DX && 16 * wv < KP;
  const int kc = 16 * wv + n;   // this lane's column of dx
  uint4 Bx[DX ? 4 : 1][3];      // the pieces of W[unit 32 s + 8 q + e][column kc]: dx = dz W sums over units
  if constexpr (DX) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (do_dx && kc < K) ? w[(size_t)(32 * s + 8 * q + e) * K + kc] : 0.0f;
      split8(v, Bx[s][0], Bx[s][1], Bx[s][2]);
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
      if constexpr (DX) grus::write_column(&dzs[0][0][0] + (16 * mt + 4 * q) * KZ + u, PLNZ, KZ, dz[mt]);
    }
    // dW += dz^T x: the tile's 32 rows are one k-step; A = the pieces of dz (k slot 8 q + e = row 16 (e / 4) + 4 q + e % 4 of unit
    // 16 w + n), B = the pieces of x[that row][column 16 c + n] from the transposed image
    {
      const float v[8] = {dz[0][0], dz[0][1], dz[0][2], dz[0][3], dz[1][0], dz[1][1], dz[1][2], dz[1][3]};
      uint4 A[3];
      split8(v, A[0], A[1], A[2]);
      const unsigned short* bcol = &xt[0][0][0] + n * KR + 8 * q;
#pragma unroll
      for (int c = 0; c < NJ; c += 2) {
        uint4 Bp[2][3];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int p = 0; p < 3; ++p) Bp[h][p] = *reinterpret_cast<const uint4*>(bcol + p * PLNT + 16 * (c + h) * KR);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          accw[c] = mf(A[TI[k]], Bp[0][TJ[k]], accw[c]);
          accw[c + 1] = mf(A[TI[k]], Bp[1][TJ[k]], accw[c + 1]);
        }
      }
    }
    __syncthreads();   // dzs complete; and every read of xr, xt, st, part of this tile is behind
    if (do_dx) {   // (false at compile time without DX)
      // one accumulation chain per order of the terms (i + j = 2, 1, 0), added smallest first at the end: dx is summed over rows
      // downstream (dbeta and db of the block before), and the matrix instruction's accumulation leans to one side by a small
      // fraction of the accumulator's last place per step, so only the four b0 b0 steps run at the result's own magnitude
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        floatx4 c0 = {0.0f, 0.0f, 0.0f, 0.0f}, c1 = c0, c2 = c0;
        const unsigned short* arow = &dzs[0][0][0] + (16 * mt + n) * KZ + 8 * q;
#pragma unroll
        for (int s = 0; s < (DX ? 4 : 0); ++s) {
          uint4 A[3];
#pragma unroll
          for (int p = 0; p < 3; ++p) A[p] = *reinterpret_cast<const uint4*>(arow + p * PLNZ + 32 * s);
          c0 = mf(A[2], Bx[s][0], c0);
          c1 = mf(A[1], Bx[s][0], c1);
          c2 = mf(A[0], Bx[s][0], c2);
          c0 = mf(A[1], Bx[s][1], c0);
          c1 = mf(A[0], Bx[s][1], c1);
          c0 = mf(A[0], Bx[s][2], c0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = row0 + 16 * mt + 4 * q + i;
          if (row < M && kc < K) dx[(size_t)row * K + kc] = (c0[i] + c1[i]) + c2[i];
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
static int mlp_products_ok(const char* who, int32_t products) {
  if (products != AC_PRODUCTS_FP32 && products != AC_PRODUCTS_BF16X3)
    return fail(std::string(who) + ": unknown products " + std::to_string(products) + " (AC_PRODUCTS_FP32 or AC_PRODUCTS_BF16X3)");
  return 0;
}
// the KP of the split form (a k-step is 32), or 0 where `products` runs the fp32 kernels
static int mlp_split_kp(int32_t K, int32_t products) {
  const int kp = K <= 32 ? 32 : mlp_kp(K);
  return (products == AC_PRODUCTS_BF16X3 && (mlps::KPS & kp)) ? kp : 0;
}
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
  if (mlp_products_ok("ac_mlp_block_forward_p", products)) return -1;
  if (!d_x || !d_w || !d_b || !d_gamma || !d_beta || !d_y) return fail("ac_mlp_block_forward_p: null argument");
  if (mlp_shape_ok("ac_mlp_block_forward_p", M, K)) return -1;
  const int kp = mlp_split_kp(K, products);
  if (!kp) return ac_mlp_block_forward(device_id, stream, M, K, eps, d_x, d_w, d_b, d_gamma, d_beta, d_y, d_stats);
  HIP_OK(hipSetDevice(device_id));
  const dim3 grid(trn::capped_tiles(M, mlpt::RT, mlpt::FWD_WGS)), block(512);
  const int vecx = mlp_split_vec(d_x, K, kp), vecw = mlp_split_vec(d_w, K, kp);
#define AC_MLP_FWD(KP)                                                                                                                         \
  hipLaunchKernelGGL(mlps::mlp_block_fwd_b3<KP>, grid, block, 0, (hipStream_t)stream, d_x, d_w, d_b, d_gamma, d_beta, d_y, d_stats, (int)M, \
                     (int)K, eps, vecx, vecw)
  switch (kp) {
    case 32: AC_MLP_FWD(32); break;
    case 64: AC_MLP_FWD(64); break;
    default: AC_MLP_FWD(128); break;
  }
#undef AC_MLP_FWD
  HIP_OK(hipGetLastError());
  return 0;
}

int ac_mlp_block_backward_p(int32_t device_id, void* stream, int32_t M, int32_t K, const float* d_dy, const float* d_x, const float* d_w,
                            const float* d_b, const float* d_gamma, const float* d_stats, float* d_workspace, float* d_dx, float* d_dw,
                            float* d_db, float* d_dgamma, float* d_dbeta, int32_t products) {
  if (mlp_products_ok("ac_mlp_block_backward_p", products)) return -1;
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
#define AC_MLP_BWD(KP)                                                                                                                             \
  if (d_dx)                                                                                                                                        \
    hipLaunchKernelGGL((mlps::mlp_block_bwd_b3<KP, true>), grid, block, 0, (hipStream_t)stream, d_dy, d_x, d_w, d_b, d_gamma, d_stats, d_workspace, \
                       d_dx, (int)M, (int)K, vecx, vecw);                                                                                          \
  else                                                                                                                                             \
    hipLaunchKernelGGL((mlps::mlp_block_bwd_b3<KP, false>), grid, block, 0, (hipStream_t)stream, d_dy, d_x, d_w, d_b, d_gamma, d_stats, d_workspace, \
                       d_dx, (int)M, (int)K, vecx, vecw)
  switch (kp) {
    case 32: AC_MLP_BWD(32); break;
    case 64: AC_MLP_BWD(64); break;
    default: AC_MLP_BWD(128); break;
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
