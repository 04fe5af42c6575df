// The three dense products of the whole GRU layer (gru_layer_train.hpp) on the bf16 matrix path ("The whole GRU layer"):
// the opt-in form `dense_products` = AC_PRODUCTS_BF16X3, independent of `products`, which selects the recurrence kernels alone.
// gru_gi_fwd_b3, gru_dx_b3 and gru_dw_b3 take the arguments of gru_gi_fwd, gru_dx and gru_dw and write the same outputs to the same
// places: T-major rows, 32-row tiles, a persistent loop with the next tile asked for into registers before the current tile's
// products, and for gru_dw_b3 the same partial sets in the same layout, so gru_sum_partials, grul::layout and the workspace are shared.
//
// The product is bf16x3.hpp's. W_ih is split once per workgroup (36 uint4 = 144 VGPRs in gi and dx); the streamed operand is split
// once per tile by the thread that stores it.
//
//   gi   x tile [32][128 + 8] per plane (272 B rows), two buffers: one barrier per tile. A wave's 2 x 3 result tiles are six
//        independent accumulators, each one chain over the 4 k-steps (24 terms), as gru_seq_fwd_b3.
//   dx   dgi tile [32][384 + 8] per plane (784 B rows), two buffers (150 528 B of the CU's 160 KB; the 144 weight registers leave
//        room for one workgroup per CU whatever the LDS): one barrier per tile. Three chains per result (chains_pairs), as
//        gru_seq_bwd_b3; one 16-row half of the tile after the other (both at once spilled two registers).
//   dw   the sum runs over rows (k slots): the gate gradients are the A operand straight from memory in the very lanes gru_dw loads
//        them into (rows 16 mt + 4 q + i, gate column 48 w + 16 j + n), split in registers, and db is the same fp32 tree of the
//        unsplit values. x (or h_in, rebuilt while the tile is loaded) is the B operand from the transposed image, written as packed
//        row pairs by threads that load two adjacent rows each; two buffers, one barrier per tile.
//
// dW keeps one fp32 accumulator per result for all six terms (96 registers), not b0 b0 in one of its own: 192 accumulator registers
// do not fit beside the operands in the 256 a wave of a 512-thread workgroup has, and the measurement does not ask for it. In the
// emulation (tests/gru_dense_split_util.py) one accumulator over a workgroup's 1920 rows reads 6.2e-7 to 8.4e-7 against float64 and
// torch 4.6e-7 to 5.6e-7, a bound of 1.8e-6 at least; on the device at 4096 x 60 dW_ih and dW_hh read 9.1e-7 and 1.07e-6, 0.66 and
// 0.67 of their bounds (gru_dw: 7.9e-7 both; profiles/gru_dense_split_bench.txt). The per-workgroup partial sets are part of that:
// a workgroup's accumulator never covers more than 1/128 of the rows.
// No floating-point atomics: results are bit-identical from run to run.
#pragma once

namespace grls {
using grul::floatx4; using grul::H; using grul::G; using grul::RT;
constexpr int KX = H + 8;    // bf16 per plane row of an x tile
constexpr int KG = G + 8;    // of a dgi tile
constexpr int KR = RT + 8;   // of the transposed x image of gru_dw_b3: k slots per column

// gi [M, 384] = x [M, 128] W_ihᵀ + b_ih. Wave w owns gate columns 48 w .. 48 w + 47 as gru_gi_fwd: B[j][s] = the pieces of
// W_ih[48 w + 16 j + n][k = 32 s + 8 q + e].
__global__ __launch_bounds__(512) void gru_gi_fwd_b3(const float* __restrict__ x, const float* __restrict__ wih, const float* __restrict__ bih,
                                                     float* __restrict__ gi, int M) {
  __shared__ __attribute__((aligned(16))) unsigned short xs[2][3][RT][KX];
  constexpr int PLN = RT * KX;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
  const int c0 = 48 * wv + n;
  uint4 B[3][4][3];
  float bias[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    b3::row_slice<4>(B[j], wih + (size_t)(c0 + 16 * j) * H, q);
    bias[j] = bih[c0 + 16 * j];
  }
  const int ntiles = (M + RT - 1) / RT;
  float pre[RT * H / 512];
  int tile = blockIdx.x, buf = 0;
  if (tile < ntiles) grul::load_rows<H>(pre, x, M, tile * RT, tid);
  for (; tile < ntiles; tile += gridDim.x, buf ^= 1) {
    unsigned short* img = &xs[buf][0][0][0];
#pragma unroll
    for (int j = 0; j < RT * H / 2048; ++j) {
      const int f = tid + 512 * j;
      b3::store_row(img + (f / (H / 4)) * KX + 4 * (f % (H / 4)), PLN, pre + 4 * j);
    }
    __syncthreads();   // the only one per tile: the next store goes to the other buffer, the one after it follows the next barrier
    const int next = tile + gridDim.x;
    if (next < ntiles) grul::load_rows<H>(pre, x, M, next * RT, tid);
    floatx4 acc[2][3];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[mt][j] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
    const unsigned short* arow = img + n * KX + 8 * q;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      uint4 A[2][3];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) b3::read3(A[mt], arow + 16 * mt * KX + 32 * s, PLN);
      b3::one_chain([&](int ti, int tj) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          acc[0][j] = b3::mf(A[0][ti], B[j][s][tj], acc[0][j]);
          acc[1][j] = b3::mf(A[1][ti], B[j][s][tj], acc[1][j]);
        }
      });
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = tile * RT + 16 * mt + 4 * q + i;
        if (row < M) {
          float* o = gi + (size_t)row * G + c0;
#pragma unroll
          for (int j = 0; j < 3; ++j) o[16 * j] = acc[mt][j][i] + bias[j];
        }
      }
  }
}

// dx [M, 128] = dgi [M, 384] W_ih. Wave w owns columns 16 w .. 16 w + 15 as gru_dx: B[s] = the pieces of W_ih[k = 32 s + 8 q + e][16 w + n],
// as gru_seq_bwd_b3 holds W_hh.
__global__ __launch_bounds__(512) void gru_dx_b3(const float* __restrict__ dgi, const float* __restrict__ wih, float* __restrict__ dx, int M) {
  __shared__ __attribute__((aligned(16))) unsigned short gs[2][3][RT][KG];
  constexpr int PLN = RT * KG;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
  const int u = 16 * wv + n;
  uint4 B[12][3];
  b3::col_slice<12>(B, wih, H, u, q);
  const int ntiles = (M + RT - 1) / RT;
  float pre[RT * G / 512];
  int tile = blockIdx.x, buf = 0;
  if (tile < ntiles) grul::load_rows<G>(pre, dgi, M, tile * RT, tid);
  for (; tile < ntiles; tile += gridDim.x, buf ^= 1) {
    unsigned short* img = &gs[buf][0][0][0];
#pragma unroll
    for (int j = 0; j < RT * G / 2048; ++j) {
      const int f = tid + 512 * j;
      b3::store_row(img + (f / (G / 4)) * KG + 4 * (f % (G / 4)), PLN, pre + 4 * j);
    }
    __syncthreads();   // the only one per tile: the next store goes to the other buffer, the one after it follows the next barrier
    const int next = tile + gridDim.x;
    if (next < ntiles) grul::load_rows<G>(pre, dgi, M, next * RT, tid);
    // three accumulation chains per result; one 16-row half of the tile after the other (both at once do not fit the registers
    // beside the weights and the tile on its way)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      floatx4 c[3] = {};
      const unsigned short* arow = img + (16 * mt + n) * KG + 8 * q;
#pragma unroll
      for (int s = 0; s < 12; ++s) {
        uint4 A[3];
        b3::read3(A, arow + 32 * s, PLN);
        b3::chains_pairs(c, A, B[s]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = tile * RT + 16 * mt + 4 * q + i;
        if (row < M) dx[(size_t)row * H + u] = b3::chain_sum(c, i);
      }
    }
  }
}

// Workgroups, tiles and partial sets as gru_dw: workgroup b sums one weight gradient over tiles b / 2, b / 2 + gridDim.x / 2, ..
// (even b dW_ih and db_ih, odd b dW_hh and db_hh) and writes its set to ws + ((b & 1) * gridDim.x / 2 + b / 2) * DW_NEL.
__global__ __launch_bounds__(512) void gru_dw_b3(const float* __restrict__ dgi, const float* __restrict__ dgh, const float* __restrict__ x,
                                                 const float* __restrict__ hxs, const float* __restrict__ y, const float* __restrict__ masks,
                                                 float* __restrict__ ws, int N, int M) {
  __shared__ __attribute__((aligned(16))) unsigned short xt[2][3][H][KR];
  constexpr int PLN = H * KR;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
  const int hh = blockIdx.x & 1, wg = blockIdx.x >> 1, nwg = gridDim.x >> 1;
  const float* __restrict__ D = hh ? dgh : dgi;
  const int c0 = 48 * wv + n;
  // this thread's share of the B operand's tile: rows 2 rp and 2 rp + 1, columns 4 cq .. 4 cq + 3
  const int rp = tid & 15, cq = tid >> 4;
  floatx4 acc[3][8];   // dW[gate row 48 w + 16 j + 4 q + i][column 16 c + n], summed over every row this workgroup walks
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[j][c] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
  float dbias[3] = {0.0f, 0.0f, 0.0f};
  const int ntiles = (M + RT - 1) / RT;
  float pd[3][2][4], px[2][4];
  auto load = [&](int t) {
    const int row0 = t * RT;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = row0 + 16 * mt + 4 * q + i;
#pragma unroll
        for (int j = 0; j < 3; ++j) pd[j][mt][i] = row < M ? D[(size_t)row * G + c0 + 16 * j] : 0.0f;
      }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int row = row0 + 2 * rp + k, c = 4 * cq;
      float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      float m = 1.0f;
      if (row < M) {
        if (!hh) {
          v = *reinterpret_cast<const float4*>(x + (size_t)row * H + c);
        } else {
          v = *reinterpret_cast<const float4*>(row < N ? hxs + (size_t)row * H + c : y + (size_t)(row - N) * H + c);
          m = masks[row];
        }
      }
      px[k][0] = v.x * m; px[k][1] = v.y * m; px[k][2] = v.z * m; px[k][3] = v.w * m;
    }
  };
  int tile = wg, buf = 0;
  if (tile < ntiles) load(tile);
  for (; tile < ntiles; tile += nwg, buf ^= 1) {
    unsigned short* img = &xt[buf][0][0][0];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      unsigned b[3];
      ctls::split3_pair(px[0][e], px[1][e], b[0], b[1], b[2]);
      b3::store_pair(img, PLN, KR, 4 * cq + e, rp, b);
    }
    // the gate gradients of the tile: A[j] = the pieces of this lane's k slots of gate column c0 + 16 j
    uint4 A[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      float v[8];
      b3::to_kslots(v, pd[j]);
      b3::split8(v, A[j]);
      // the tile's eight rows of this lane as a tree, then the running sum
      dbias[j] += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    __syncthreads();   // the only one per tile: the next store goes to the other buffer, the one after it follows the next barrier
    if (tile + nwg < ntiles) load(tile + nwg);
    const unsigned short* bcol = img + n * KR + 8 * q;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      uint4 Bp[3];
      b3::read3(Bp, bcol + 16 * c * KR, PLN);
      b3::one_chain([&](int ti, int tj) {
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[j][c] = b3::mf(A[j][ti], Bp[tj], acc[j][c]);
      });
    }
  }
  float* base = ws + (size_t)(hh * nwg + wg) * grul::DW_NEL;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) base[(size_t)(48 * wv + 16 * j + 4 * q + i) * H + 16 * c + n] = acc[j][c][i];
    // the four quarters hold different rows' shares of the same gate column
    float s = dbias[j];
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (q == 0) base[G * H + c0 + 16 * j] = s;
  }
}
}  // namespace grls

// ------------------------------------------------------------------------------------------------ C ABI (include/aircombat.h)
extern "C" {
static grul::Dense gru_dense_kernels(int32_t dense_products) {
  if (dense_products == AC_PRODUCTS_FP32) return grul::dense_fp32();
  return {grls::gru_gi_fwd_b3, grls::gru_dw_b3, grls::gru_dx_b3};
}
int ac_gru_layer_forward_pd(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_x, const float* d_hxs, const float* d_masks,
                            const float* d_w_ih, const float* d_w_hh, const float* d_b_ih, const float* d_b_hh, const float* d_gamma,
                            const float* d_beta, float eps, float* d_workspace, float* d_out, float* d_h_T, float* d_y, float* d_saved,
                            float* d_stats, int32_t products, int32_t dense_products) {
  const char* who = "ac_gru_layer_forward_pd";
  if (trn::products_ok(who, "products", products) || trn::products_ok(who, "dense products", dense_products)) return -1;
  return gru_layer_forward("ac_gru_layer_forward_pd", products, gru_dense_kernels(dense_products), device_id, stream, N, T, d_x, d_hxs, d_masks,
                           d_w_ih, d_w_hh, d_b_ih, d_b_hh, d_gamma, d_beta, eps, d_workspace, d_out, d_h_T, d_y, d_saved, d_stats);
}
int ac_gru_layer_backward_pd(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_g_out, const float* d_g_h_T,
                             const float* d_x, const float* d_hxs, const float* d_masks, const float* d_w_ih, const float* d_w_hh,
                             const float* d_gamma, const float* d_y, const float* d_saved, const float* d_stats, float* d_workspace,
                             float* d_dx, float* d_dhxs, float* d_dw_ih, float* d_dw_hh, float* d_db_ih, float* d_db_hh, float* d_dgamma,
                             float* d_dbeta, int32_t products, int32_t dense_products) {
  const char* who = "ac_gru_layer_backward_pd";
  if (trn::products_ok(who, "products", products) || trn::products_ok(who, "dense products", dense_products)) return -1;
  return gru_layer_backward("ac_gru_layer_backward_pd", products, gru_dense_kernels(dense_products), device_id, stream, N, T, d_g_out, d_g_h_T,
                            d_x, d_hxs, d_masks, d_w_ih, d_w_hh, d_gamma, d_y, d_saved, d_stats, d_workspace, d_dx, d_dhxs, d_dw_ih, d_dw_hh,
                            d_db_ih, d_db_hh, d_dgamma, d_dbeta);
}
}  // extern "C"
