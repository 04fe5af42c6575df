// The PPO update's whole GRU layer on the device ("The whole GRU layer"): everything of the reference's GRULayer
// (algorithms/utils/gru.py: nn.GRU 128 -> 128, one layer, then nn.LayerNorm(128)) that gru_train.hpp leaves to its caller, so that the
// layer is one C call per direction with the recurrence kernels gru_seq_fwd / gru_seq_bwd between the kernels of this file:
//
//   forward    gru_gi_fwd  gi [M, 384] = x W_ihᵀ + b_ih          -> gru_seq_fwd -> gru_ln_fwd  out = LN_128(y) gamma + beta
//   backward   gru_ln_bwd  dy, and the partials of dgamma, dbeta  -> gru_seq_bwd -> gru_dw      the partials of dW_ih, dW_hh, db_ih, db_hh
//              gru_sum_partials (twice)                                           -> gru_dx      dx = dgi W_ih (only when wanted)
//
// M = T * N rows, T-major as in gru_train.hpp; fp32 everywhere. The three products use v_mfma_f32_16x16x4_f32 (exact fp32 products and
// sums) with the weight slice of a wave in registers for a persistent loop over 32-row tiles, the next tile's rows asked for into
// registers before the current tile's products, as in mlp_train.hpp; gi sums in two chains and dx in four, met in a tree. The two
// LayerNorm kernels are streaming: a wave owns whole rows, two adjacent columns per lane, four rows in flight.
//
// gru_dw: the two weight gradients are independent products over the same rows, and one of them fills a wave's registers (a wave owns
// 48 gate rows x 128 columns of dW: 96 accumulator registers), so even workgroups sum dW_ih = Σ dgiᵀ x and odd ones dW_hh = Σ dghᵀ h_in
// over the same tiles. The gate gradients are the A operand straight from memory (lane (n, q) takes row 4 q + i, gate column 48 w +
// 16 j + n: the eight waves of a workgroup read each row whole, every byte once); x or h_in is the B operand, through LDS.
// h_in(t, j) = (t == 0 ? hxs[j] : y[(t - 1) N + j]) * masks[t N + j] is row r - N of y (row r of hxs when r < N) times masks[r]: it is
// rebuilt while the tile is loaded and never stored. The bias gradients are the column sums of the same registers.
//
// Parameter-gradient sums: every workgroup writes its set of partial sums to the workspace and gru_sum_partials adds the sets in an
// order fixed by their number alone (eight interleaved running sums, then a tree). A workgroup's running sum covers its own rows only
// (1/128 of them in gru_dw, 1/4096 per wave in gru_ln_bwd). No floating-point atomics: results are bit-identical from run to run.
//
// gru_layer_train_split.hpp has a second form of the three products (gi, dw, dx) on the bf16 matrix path; the host code below launches
// either through grul::Dense.
#pragma once

#include "mlp_train.hpp"

namespace grul {
using mlpt::floatx4;
using mlpt::wave_sum;
constexpr int H = 128, G = 384;
constexpr int RT = mlpt::RT;            // rows per tile of every kernel here
constexpr int HP = H + 4, GP = G + 4;   // LDS row strides (4 mod 64 banks, as in gru_train.hpp)
constexpr int GI_WGS = 256;             // persistent workgroups at most: the products hold 96 weight registers, one workgroup per CU
constexpr int DX_WGS = 256;
constexpr int DW_WGS = 256;             // 128 per weight gradient; also the partial sets gru_sum_partials adds, 128 per gradient
constexpr int LN_WGS = 512;             // the streaming kernels: two workgroups per CU
constexpr int LNB_WGS = 512;
constexpr int DW_NEL = G * H + G;       // a partial set of gru_dw: dW [384, 128], db [384]
constexpr int LN_NEL = 2 * H;           // of gru_ln_bwd: dgamma, dbeta

// rows row0 .. row0 + RT - 1 of src [M, W] into registers as whole float4s (thread t takes float4 t, t + 512, ..: a row is W / 4 of
// them, so src is 16-byte aligned); rows >= M are 0. store_rows lays them out as the [RT][W + 4] tile in LDS. (Not mlpt::load_tile /
// store_tile: instantiating those here as well moved act_eval_bwd<2, false> from 188 to 192 VGPRs.)
template <int W>
__device__ __forceinline__ void load_rows(float (&v)[RT * W / 512], const float* __restrict__ src, int M, int row0, int tid) {
#pragma unroll
  for (int j = 0; j < RT * W / 2048; ++j) {
    const int f = tid + 512 * j, r = f / (W / 4), c = 4 * (f % (W / 4));
    float4 t = {0.0f, 0.0f, 0.0f, 0.0f};
    if (row0 + r < M) t = *reinterpret_cast<const float4*>(src + (size_t)(row0 + r) * W + c);
    v[4 * j] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
  }
}
template <int W>
__device__ __forceinline__ void store_rows(const float (&v)[RT * W / 512], float (*lds)[W + 4], int tid) {
#pragma unroll
  for (int j = 0; j < RT * W / 2048; ++j) {
    const int f = tid + 512 * j;
    *reinterpret_cast<float4*>(&lds[f / (W / 4)][4 * (f % (W / 4))]) = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
  }
}

// gi [M, 384] = x [M, 128] W_ihᵀ + b_ih. Wave w owns gate columns 48 w .. 48 w + 47 (three 16-column tiles, so a row of its results is
// 192 contiguous bytes): B[j][s] = W_ih[48 w + 16 j + n][k = 32 q + s].
__global__ __launch_bounds__(512) void gru_gi_fwd(const float* __restrict__ x, const float* __restrict__ wih, const float* __restrict__ bih,
                                                  float* __restrict__ gi, int M) {
  __shared__ __attribute__((aligned(16))) float xs[RT][HP];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
  const int c0 = 48 * wv + n;
  float B[3][32], bias[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int s = 0; s < 32; s += 4) {
      const float4 v = *reinterpret_cast<const float4*>(wih + (size_t)(c0 + 16 * j) * H + 32 * q + s);
      B[j][s] = v.x; B[j][s + 1] = v.y; B[j][s + 2] = v.z; B[j][s + 3] = v.w;
    }
    bias[j] = bih[c0 + 16 * j];
  }
  const int ntiles = (M + RT - 1) / RT;
  float pre[RT * H / 512];
  int tile = blockIdx.x;
  if (tile < ntiles) load_rows<H>(pre, x, M, tile * RT, tid);
  for (; tile < ntiles; tile += gridDim.x) {
    store_rows<H>(pre, xs, tid);
    __syncthreads();
    const int next = tile + gridDim.x;
    if (next < ntiles) load_rows<H>(pre, x, M, next * RT, tid);
    // two accumulation chains per result (k even, k odd), added at the end: half the length of a running fp32 sum
    floatx4 acc[2][3][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[mt][j][0] = acc[mt][j][1] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < 32; s += 4) {
      const float4 a0 = *reinterpret_cast<const float4*>(&xs[n][32 * q + s]);
      const float4 a1 = *reinterpret_cast<const float4*>(&xs[16 + n][32 * q + s]);
      const float v0[4] = {a0.x, a0.y, a0.z, a0.w}, v1[4] = {a1.x, a1.y, a1.z, a1.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          acc[0][j][k & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0[k], B[j][s + k], acc[0][j][k & 1], 0, 0, 0);
          acc[1][j][k & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1[k], B[j][s + k], acc[1][j][k & 1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = tile * RT + 16 * mt + 4 * q + i;
        if (row < M) {
          float* o = gi + (size_t)row * G + c0;
#pragma unroll
          for (int j = 0; j < 3; ++j) o[16 * j] = (acc[mt][j][0][i] + acc[mt][j][1][i]) + bias[j];
        }
      }
    __syncthreads();   // every read of xs is behind before the next tile is stored
  }
}

// out [M, 128] = (y - mean) / sqrt(var + eps) * gamma + beta, biased variance; stats [M, 2] = (mean, 1 / sqrt(var + eps)) or NULL
// (inference: nothing kept). Wave w of a workgroup takes rows 4 w .. 4 w + 3 of the tile, lane l columns 2 l and 2 l + 1.
__global__ __launch_bounds__(512) void gru_ln_fwd(const float* __restrict__ y, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  float* __restrict__ out, float* __restrict__ stats, int M, float eps) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float2 gm = *reinterpret_cast<const float2*>(gamma + 2 * lane), be = *reinterpret_cast<const float2*>(beta + 2 * lane);
  const int ntiles = (M + RT - 1) / RT;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int row0 = tile * RT + 4 * wv;
    float2 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      v[j] = row0 + j < M ? *reinterpret_cast<const float2*>(y + (size_t)(row0 + j) * H + 2 * lane) : make_float2(0.0f, 0.0f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = row0 + j;
      const float mean = wave_sum(v[j].x + v[j].y) * (1.0f / H);
      const float d0 = v[j].x - mean, d1 = v[j].y - mean;
      const float var = wave_sum(d0 * d0 + d1 * d1) * (1.0f / H);
      const float rstd = 1.0f / sqrtf(var + eps);
      if (row < M) {
        *reinterpret_cast<float2*>(out + (size_t)row * H + 2 * lane) = make_float2((d0 * rstd) * gm.x + be.x, (d1 * rstd) * gm.y + be.y);
        if (stats && lane < 2) stats[(size_t)row * 2 + lane] = lane ? rstd : mean;
      }
    }
  }
}

// dy [M, 128] = rstd (g - mean(g) - y_hat mean(g y_hat)) with g = g_out gamma and y_hat = (y - mean) rstd; the workgroup's partial
// dgamma = Σ g_out y_hat and dbeta = Σ g_out go to ws + blockIdx.x * 256. Rows as in gru_ln_fwd; a row past M loads zeros (its rstd
// too) and adds nothing.
__global__ __launch_bounds__(512) void gru_ln_bwd(const float* __restrict__ gout, const float* __restrict__ y, const float* __restrict__ stats,
                                                  const float* __restrict__ gamma, float* __restrict__ dy, float* __restrict__ ws, int M) {
  __shared__ __attribute__((aligned(16))) float part[8][LN_NEL];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const float2 gm = *reinterpret_cast<const float2*>(gamma + 2 * lane);
  float2 dg = make_float2(0.0f, 0.0f), db = dg;
  const int ntiles = (M + RT - 1) / RT;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int row0 = tile * RT + 4 * wv;
    float2 gv[4], yv[4], st[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool ok = row0 + j < M;
      const size_t o = (size_t)(row0 + j) * H + 2 * lane;
      gv[j] = ok ? *reinterpret_cast<const float2*>(gout + o) : make_float2(0.0f, 0.0f);
      yv[j] = ok ? *reinterpret_cast<const float2*>(y + o) : make_float2(0.0f, 0.0f);
      st[j] = ok ? *reinterpret_cast<const float2*>(stats + (size_t)(row0 + j) * 2) : make_float2(0.0f, 0.0f);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float rs = st[j].y;
      const float h0 = (yv[j].x - st[j].x) * rs, h1 = (yv[j].y - st[j].x) * rs;
      const float g0 = gv[j].x * gm.x, g1 = gv[j].y * gm.y;
      const float m1 = wave_sum(g0 + g1) * (1.0f / H);
      const float m2 = wave_sum(g0 * h0 + g1 * h1) * (1.0f / H);
      if (row0 + j < M)
        *reinterpret_cast<float2*>(dy + (size_t)(row0 + j) * H + 2 * lane) = make_float2(rs * (g0 - m1 - h0 * m2), rs * (g1 - m1 - h1 * m2));
      dg.x += gv[j].x * h0; dg.y += gv[j].y * h1;
      db.x += gv[j].x; db.y += gv[j].y;
    }
  }
  part[wv][2 * lane] = dg.x; part[wv][2 * lane + 1] = dg.y;
  part[wv][H + 2 * lane] = db.x; part[wv][H + 2 * lane + 1] = db.y;
  __syncthreads();
  if (tid < LN_NEL) {   // the eight waves' shares, as a tree in wave order
    const float s = ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) + ((part[4][tid] + part[5][tid]) + (part[6][tid] + part[7][tid]));
    ws[(size_t)blockIdx.x * LN_NEL + tid] = s;
  }
}

// Workgroup b sums one weight gradient over tiles b / 2, b / 2 + gridDim.x / 2, ..: even b dW_ih = Σ dgiᵀ x and db_ih = Σ dgi, odd b
// dW_hh = Σ dghᵀ h_in and db_hh = Σ dgh. Its partial set goes to ws + ((b & 1) * gridDim.x / 2 + b / 2) * DW_NEL.
// x, hxs and y are read as float4: the C ABI refuses them unless they are 16-byte aligned.
__global__ __launch_bounds__(512) void gru_dw(const float* __restrict__ dgi, const float* __restrict__ dgh, const float* __restrict__ x,
                                              const float* __restrict__ hxs, const float* __restrict__ y, const float* __restrict__ masks,
                                              float* __restrict__ ws, int N, int M) {
  __shared__ __attribute__((aligned(16))) float xs[RT][HP];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
  const int hh = blockIdx.x & 1, wg = blockIdx.x >> 1, nwg = gridDim.x >> 1;
  const float* __restrict__ D = hh ? dgh : dgi;
  const int c0 = 48 * wv + n;
  floatx4 acc[3][8];   // dW[gate row 48 w + 16 j + 4 q + i][column 16 c + n], summed over every row this workgroup walks
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[j][c] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
  float dbias[3] = {0.0f, 0.0f, 0.0f};
  const int ntiles = (M + RT - 1) / RT;
  float pd[2][4][3], px[RT * H / 512];
  // the gate gradients of a tile in the A operand's layout, and the B operand's rows (x, or h_in rebuilt) as store_rows lays them out
  auto load = [&](int t) {
    const int row0 = t * RT;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = row0 + 16 * mt + 4 * q + i;
#pragma unroll
        for (int j = 0; j < 3; ++j) pd[mt][i][j] = row < M ? D[(size_t)row * G + c0 + 16 * j] : 0.0f;
      }
    if (!hh) {
      load_rows<H>(px, x, M, row0, tid);
    } else {
#pragma unroll
      for (int k = 0; k < RT * H / 2048; ++k) {
        const int f = tid + 512 * k, row = row0 + f / (H / 4), c = 4 * (f % (H / 4));
        float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        float m = 0.0f;
        if (row < M) {
          v = *reinterpret_cast<const float4*>(row < N ? hxs + (size_t)row * H + c : y + (size_t)(row - N) * H + c);
          m = masks[row];
        }
        px[4 * k] = v.x * m; px[4 * k + 1] = v.y * m; px[4 * k + 2] = v.z * m; px[4 * k + 3] = v.w * m;
      }
    }
  };
  int tile = wg;
  if (tile < ntiles) load(tile);
  for (; tile < ntiles; tile += nwg) {
    store_rows<H>(px, xs, tid);
    float a[2][4][3];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) a[mt][i][j] = pd[mt][i][j];
    __syncthreads();
    if (tile + nwg < ntiles) load(tile + nwg);
    // the step over rows {16 mt + 4 q + i}: A = the gate gradient (gate column on lane % 16, row on the quarter), B = xs[row][16 c + n]
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float* xr = &xs[16 * mt + 4 * q + i][n];
        float b[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) b[c] = xr[16 * c];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[j][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][i][j], b[c], acc[j][c], 0, 0, 0);
      }
#pragma unroll
    for (int j = 0; j < 3; ++j)   // the tile's eight rows of this lane as a tree, then the running sum
      dbias[j] += ((a[0][0][j] + a[0][1][j]) + (a[0][2][j] + a[0][3][j])) + ((a[1][0][j] + a[1][1][j]) + (a[1][2][j] + a[1][3][j]));
    __syncthreads();   // every read of xs is behind before the next tile is stored
  }
  float* base = ws + (size_t)(hh * nwg + wg) * DW_NEL;
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

// dx [M, 128] = dgi [M, 384] W_ih. Wave w owns columns 16 w .. 16 w + 15: B[s] = W_ih[k = 96 q + s][16 w + n], as gru_seq_bwd holds W_hh.
__global__ __launch_bounds__(512) void gru_dx(const float* __restrict__ dgi, const float* __restrict__ wih, float* __restrict__ dx, int M) {
  __shared__ __attribute__((aligned(16))) float gs[RT][GP];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
  const int u = 16 * wv + n;
  float B[96];
#pragma unroll
  for (int s = 0; s < 96; ++s) B[s] = wih[(size_t)(96 * q + s) * H + u];
  const int ntiles = (M + RT - 1) / RT;
  float pre[RT * G / 512];
  int tile = blockIdx.x;
  if (tile < ntiles) load_rows<G>(pre, dgi, M, tile * RT, tid);
  for (; tile < ntiles; tile += gridDim.x) {
    store_rows<G>(pre, gs, tid);
    __syncthreads();
    const int next = tile + gridDim.x;
    if (next < ntiles) load_rows<G>(pre, dgi, M, next * RT, tid);
    // four accumulation chains per result (one per element of the float4), met in a tree: a single running fp32 sum over the 96
    // steps was 2.6 to 6.5 times torch's error in dx against float64
    floatx4 a0[4], a1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a0[k] = a1[k] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < 96; s += 4) {
      const float4 r0 = *reinterpret_cast<const float4*>(&gs[n][96 * q + s]);
      const float4 r1 = *reinterpret_cast<const float4*>(&gs[16 + n][96 * q + s]);
      const float v0[4] = {r0.x, r0.y, r0.z, r0.w}, v1[4] = {r1.x, r1.y, r1.z, r1.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a0[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0[k], B[s + k], a0[k], 0, 0, 0);
        a1[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1[k], B[s + k], a1[k], 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = tile * RT + 4 * q + i;
      if (row < M) dx[(size_t)row * H + u] = (a0[0][i] + a0[1][i]) + (a0[2][i] + a0[3][i]);
      if (row + 16 < M) dx[(size_t)(row + 16) * H + u] = (a1[0][i] + a1[1][i]) + (a1[2][i] + a1[3][i]);
    }
    __syncthreads();   // every read of gs is behind before the next tile is stored
  }
}

// out[e] = the sum over the S partial sets of ws[s * nel + e] (trn::sum_sets). blockIdx.y picks the family (gru_dw's two gradients): its sets start at ws + y * S * nel, its results go to o0 (the first n0
// elements of a set) and o1 (the rest), or to p0 and p1 for y = 1.
__global__ __launch_bounds__(256) void gru_sum_partials(const float* __restrict__ ws, int S, int nel, int n0, float* __restrict__ o0,
                                                        float* __restrict__ o1, float* __restrict__ p0, float* __restrict__ p1) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nel) return;
  const float r = trn::sum_sets(ws + (size_t)blockIdx.y * S * nel, S, nel, e);
  float* d0 = blockIdx.y ? p0 : o0;
  float* d1 = blockIdx.y ? p1 : o1;
  if (e < n0) d0[e] = r;
  else d1[e - n0] = r;
}

// the workspace, in floats: [dgi | gi: M * 384][dgh: M * 384][dy: M * 128][gru_dw's partial sets][gru_ln_bwd's partial sets]
struct Layout {
  int64_t dgh, dy, dwp, lnp, total;
  int dw_sets, ln_sets;   // per weight gradient; of gru_ln_bwd
};
inline Layout layout(int M) {
  Layout l;
  l.dw_sets = trn::capped_tiles(M, RT, DW_WGS / 2);
  l.ln_sets = trn::capped_tiles(M, RT, LNB_WGS);
  l.dgh = (int64_t)M * G;
  l.dy = l.dgh + (int64_t)M * G;
  l.dwp = l.dy + (int64_t)M * H;
  l.lnp = l.dwp + (int64_t)2 * l.dw_sets * DW_NEL;
  l.total = l.lnp + (int64_t)l.ln_sets * LN_NEL;
  return l;
}
// the three dense products' kernels: this file's, or those of gru_layer_train_split.hpp
struct Dense {
  void (*gi)(const float*, const float*, const float*, float*, int);
  void (*dw)(const float*, const float*, const float*, const float*, const float*, const float*, float*, int, int);
  void (*dx)(const float*, const float*, float*, int);
};
inline Dense dense_fp32() { return {gru_gi_fwd, gru_dw, gru_dx}; }
}  // namespace grul

// ------------------------------------------------------------------------------------------------ C ABI (include/aircombat.h)
extern "C" {
static int gru_layer_shape_ok(const char* who, int32_t N, int32_t T) { return gru_shape_ok(who, N, T, 2 * grul::RT); }

int64_t ac_gru_layer_workspace_floats(int32_t N, int32_t T) {
  if (gru_layer_shape_ok("ac_gru_layer_workspace_floats", N, T)) return -1;
  return grul::layout(N * T).total;
}

int32_t ac_gru_layer_constant(int32_t which) {
  switch (which) {
    case 0: return grul::RT;
    case 1: return grul::GI_WGS;
    case 2: return grul::LN_WGS;
    case 3: return grul::LNB_WGS;
    case 4: return grul::DW_WGS / 2;
    case 5: return grul::DX_WGS;
    default: return -1;
  }
}

// `who` names the entry in its refusals; `products` (checked by the caller) selects the recurrence kernel alone, `dense` the three
// dense products' kernels
static int gru_layer_forward(const std::string& who, int32_t products, const grul::Dense& dense, int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_x,
                             const float* d_hxs, const float* d_masks, const float* d_w_ih, const float* d_w_hh, const float* d_b_ih,
                             const float* d_b_hh, const float* d_gamma, const float* d_beta, float eps, float* d_workspace, float* d_out,
                             float* d_h_T, float* d_y, float* d_saved, float* d_stats) {
  if (!d_x || !d_hxs || !d_masks || !d_w_ih || !d_w_hh || !d_b_ih || !d_b_hh || !d_gamma || !d_beta || !d_workspace || !d_out || !d_h_T || !d_y)
    return fail(who + ": null argument");
  if ((d_saved == nullptr) != (d_stats == nullptr)) return fail(who + ": saved and stats go together (both, or both NULL)");
  if (gru_layer_shape_ok(who.c_str(), N, T)) return -1;
  if (!trn::aligned16({d_x, d_w_ih, d_gamma, d_beta, d_workspace, d_out, d_y, d_stats}))
    return fail(who + ": x, w_ih, gamma, beta, workspace, out, y and stats must be 16-byte aligned");
  HIP_OK(hipSetDevice(device_id));
  const int M = N * T;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(dense.gi, dim3(trn::capped_tiles(M, grul::RT, grul::GI_WGS)), dim3(512), 0, s, d_x, d_w_ih, d_b_ih, d_workspace, M);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(products == AC_PRODUCTS_BF16X3 ? grus::gru_seq_fwd_b3 : grut::gru_seq_fwd, dim3(trn::tiles(N, grut::RT)), dim3(512), 0, s,
                     (const float*)d_workspace, d_hxs, d_masks, d_w_hh, d_b_hh, d_y, d_h_T, d_saved, (int)N, (int)T);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(grul::gru_ln_fwd, dim3(trn::capped_tiles(M, grul::RT, grul::LN_WGS)), dim3(512), 0, s, (const float*)d_y, d_gamma, d_beta, d_out, d_stats, M, eps);
  HIP_OK(hipGetLastError());
  return 0;
}
int ac_gru_layer_forward(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_x, const float* d_hxs, const float* d_masks,
                         const float* d_w_ih, const float* d_w_hh, const float* d_b_ih, const float* d_b_hh, const float* d_gamma,
                         const float* d_beta, float eps, float* d_workspace, float* d_out, float* d_h_T, float* d_y, float* d_saved,
                         float* d_stats) {
  return gru_layer_forward("ac_gru_layer_forward", AC_PRODUCTS_FP32, grul::dense_fp32(), device_id, stream, N, T, d_x, d_hxs, d_masks, d_w_ih, d_w_hh, d_b_ih, d_b_hh,
                           d_gamma, d_beta, eps, d_workspace, d_out, d_h_T, d_y, d_saved, d_stats);
}
int ac_gru_layer_forward_p(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_x, const float* d_hxs, const float* d_masks,
                           const float* d_w_ih, const float* d_w_hh, const float* d_b_ih, const float* d_b_hh, const float* d_gamma,
                           const float* d_beta, float eps, float* d_workspace, float* d_out, float* d_h_T, float* d_y, float* d_saved,
                           float* d_stats, int32_t products) {
  if (trn::products_ok("ac_gru_layer_forward_p", "products", products)) return -1;
  return gru_layer_forward("ac_gru_layer_forward_p", products, grul::dense_fp32(), device_id, stream, N, T, d_x, d_hxs, d_masks, d_w_ih, d_w_hh, d_b_ih, d_b_hh,
                           d_gamma, d_beta, eps, d_workspace, d_out, d_h_T, d_y, d_saved, d_stats);
}

static int gru_layer_backward(const std::string& who, int32_t products, const grul::Dense& dense, int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_g_out,
                              const float* d_g_h_T, const float* d_x, const float* d_hxs, const float* d_masks, const float* d_w_ih,
                              const float* d_w_hh, const float* d_gamma, const float* d_y, const float* d_saved, const float* d_stats,
                              float* d_workspace, float* d_dx, float* d_dhxs, float* d_dw_ih, float* d_dw_hh, float* d_db_ih, float* d_db_hh,
                              float* d_dgamma, float* d_dbeta) {
  if (!d_x || !d_hxs || !d_masks || !d_w_ih || !d_w_hh || !d_gamma || !d_y || !d_saved || !d_stats || !d_workspace || !d_dw_ih || !d_dw_hh ||
      !d_db_ih || !d_db_hh || !d_dgamma || !d_dbeta)
    return fail(who + ": null argument");
  if (gru_layer_shape_ok(who.c_str(), N, T)) return -1;
  if (!trn::aligned16({d_g_out, d_x, d_hxs, d_gamma, d_y, d_stats, d_workspace, d_dx}))
    return fail(who + ": g_out, x, hxs, gamma, y, stats, workspace and dx must be 16-byte aligned");
  HIP_OK(hipSetDevice(device_id));
  const int M = N * T;
  const grul::Layout l = grul::layout(M);
  hipStream_t s = (hipStream_t)stream;
  float *dgi = d_workspace, *dgh = d_workspace + l.dgh, *dy = d_workspace + l.dy, *dwp = d_workspace + l.dwp, *lnp = d_workspace + l.lnp;
  if (d_g_out) {
    hipLaunchKernelGGL(grul::gru_ln_bwd, dim3(l.ln_sets), dim3(512), 0, s, d_g_out, d_y, d_stats, d_gamma, dy, lnp, M);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(grul::gru_sum_partials, dim3((grul::LN_NEL + 255) / 256, 1), dim3(256), 0, s, (const float*)lnp, l.ln_sets, grul::LN_NEL,
                       grul::H, d_dgamma, d_dbeta, d_dgamma, d_dbeta);
    HIP_OK(hipGetLastError());
  } else {   // no gradient reaches the LayerNorm: its parameters' are zero and the recurrence takes dh_T alone
    HIP_OK(hipMemsetAsync(d_dgamma, 0, grul::H * sizeof(float), s));
    HIP_OK(hipMemsetAsync(d_dbeta, 0, grul::H * sizeof(float), s));
  }
  hipLaunchKernelGGL(products == AC_PRODUCTS_BF16X3 ? grus::gru_seq_bwd_b3 : grut::gru_seq_bwd, dim3(trn::tiles(N, grut::RT)), dim3(512), 0, s,
                     d_g_out ? (const float*)dy : nullptr, d_g_h_T, d_saved, d_y, d_hxs, d_masks, d_w_hh, dgi, dgh, d_dhxs, (int)N, (int)T);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(dense.dw, dim3(2 * l.dw_sets), dim3(512), 0, s, (const float*)dgi, (const float*)dgh, d_x, d_hxs, d_y, d_masks, dwp, (int)N, M);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(grul::gru_sum_partials, dim3((grul::DW_NEL + 255) / 256, 2), dim3(256), 0, s, (const float*)dwp, l.dw_sets, grul::DW_NEL,
                     grul::G * grul::H, d_dw_ih, d_db_ih, d_dw_hh, d_db_hh);
  HIP_OK(hipGetLastError());
  if (d_dx) {
    hipLaunchKernelGGL(dense.dx, dim3(trn::capped_tiles(M, grul::RT, grul::DX_WGS)), dim3(512), 0, s, (const float*)dgi, d_w_ih, d_dx, M);
    HIP_OK(hipGetLastError());
  }
  return 0;
}
int ac_gru_layer_backward(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_g_out, const float* d_g_h_T, const float* d_x,
                          const float* d_hxs, const float* d_masks, const float* d_w_ih, const float* d_w_hh, const float* d_gamma,
                          const float* d_y, const float* d_saved, const float* d_stats, float* d_workspace, float* d_dx, float* d_dhxs,
                          float* d_dw_ih, float* d_dw_hh, float* d_db_ih, float* d_db_hh, float* d_dgamma, float* d_dbeta) {
  return gru_layer_backward("ac_gru_layer_backward", AC_PRODUCTS_FP32, grul::dense_fp32(), device_id, stream, N, T, d_g_out, d_g_h_T, d_x, d_hxs, d_masks, d_w_ih,
                            d_w_hh, d_gamma, d_y, d_saved, d_stats, d_workspace, d_dx, d_dhxs, d_dw_ih, d_dw_hh, d_db_ih, d_db_hh, d_dgamma, d_dbeta);
}
int ac_gru_layer_backward_p(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_g_out, const float* d_g_h_T,
                            const float* d_x, const float* d_hxs, const float* d_masks, const float* d_w_ih, const float* d_w_hh,
                            const float* d_gamma, const float* d_y, const float* d_saved, const float* d_stats, float* d_workspace,
                            float* d_dx, float* d_dhxs, float* d_dw_ih, float* d_dw_hh, float* d_db_ih, float* d_db_hh, float* d_dgamma,
                            float* d_dbeta, int32_t products) {
  if (trn::products_ok("ac_gru_layer_backward_p", "products", products)) return -1;
  return gru_layer_backward("ac_gru_layer_backward_p", products, grul::dense_fp32(), device_id, stream, N, T, d_g_out, d_g_h_T, d_x, d_hxs, d_masks, d_w_ih, d_w_hh,
                            d_gamma, d_y, d_saved, d_stats, d_workspace, d_dx, d_dhxs, d_dw_ih, d_dw_hh, d_db_ih, d_db_hh, d_dgamma, d_dbeta);
}
}  // extern "C"
