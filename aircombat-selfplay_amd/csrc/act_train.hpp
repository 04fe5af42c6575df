// The PPO update's action heads on the device ("The training action heads"): ACTLayer.evaluate_actions of the reference
// (algorithms/utils/act.py, distributions.py) for MultiDiscrete heads and the tuple spaces' shoot head, x [M, 128] -> logp [M], ent [M],
// fp32 everywhere, one launch forward and two backward (the heads' kernel, then a fixed-order sum of the parameter-gradient partials).
//
// All heads' logits are one product: the categorical heads' rows of W_h side by side (off[h] .. off[h + 1] - 1), then the two outputs of
// the shoot head's net, at most 162 columns, cut into 16-unit slices. A workgroup of eight waves walks 32-row tiles in mlp_train.hpp's
// persistent loop, with its loaders and its exact-fp32 v_mfma_f32_16x16x4_f32 product; wave w owns slice w, with those rows of W in
// registers, and above 128 columns (SPW = 2) waves 0 .. 2 also own slices 8 .. 10, whose rows of W sit in an LDS copy made once per
// workgroup (in registers as well they spill the backward). The logits go to an LDS tile and never further. There 16 lanes take
// one row: per head a max, a sum of exponentials, the taken entry picked by compare-and-select against (int)a (no memory is indexed by
// an action), and -sum p log p; then the shoot head's Bernoulli as torch.distributions computes it.
//
// Backward: the logits are recomputed from x, the row pass overwrites them in place with dL/dlogit, and that tile is the A operand of
// both products that follow: dW = dlᵀ x (the accumulators stay in the wave that owns the units for the whole loop) and dx = dl W (against
// a transposed register slice of W). Each workgroup ends by writing its share of dW and db to the workspace; act_eval_reduce adds the
// shares in a fixed order and scatters them to the heads' own gradient tensors. No floating-point atomics anywhere.
#pragma once

namespace actt {
using mlpt::floatx4;
using mlpt::H;
using mlpt::RT;
using mlpt::sum16;
constexpr int MAXH = 9;            // eight categorical heads and the shoot head
constexpr int MAX_LOGITS = 160;    // categorical logits at most (the shoot head adds two columns)
constexpr float BERN_EPS = 1.1920928955078125e-07f;   // torch.finfo(torch.float32).eps: Bernoulli(probs=p) clamps p to [eps, 1 - eps]

// off[h] .. off[h + 1] - 1: the columns of head h; off[h] = total for every h past the last head (their pointers are never taken)
struct Heads {
  const float* w[MAXH];
  const float* b[MAXH];
  int off[MAXH + 1];
  int n_cat, total, shoot_cols, act_cols;
};
struct Grads {
  float* dw[MAXH];
  float* db[MAXH];
};

__device__ __forceinline__ float max16(float v) {   // over the 16 lanes of a quarter
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// row c of the stacked [total, 128] weight and its bias; NULL past the last column (a compare-and-select chain: no table is indexed)
__device__ __forceinline__ const float* stacked_row(const Heads& hd, int c, const float*& bias) {
  const float* wr = nullptr;
  bias = nullptr;
#pragma unroll
  for (int h = 0; h < MAXH; ++h) {
    const bool in = c >= hd.off[h] && c < hd.off[h + 1];
    wr = in ? hd.w[h] + (size_t)(c - hd.off[h]) * H : wr;
    bias = in ? hd.b[h] + (c - hd.off[h]) : bias;
  }
  return wr;
}

__device__ __forceinline__ float softplus(float y) { return y > 20.0f ? y : log1pf(expf(y)); }   // torch: beta 1, identity above 20
__device__ __forceinline__ float softplus_grad(float y) {
  const float e = expf(y);
  return y > 20.0f ? 1.0f : e / (e + 1.0f);
}
// binary_cross_entropy_with_logits(x, t), elementwise
__device__ __forceinline__ float bce_logits(float x, float t) { return (1.0f - t) * x + fmaxf(-x, 0.0f) + log1pf(expf(-fabsf(x))); }

// mlpt::tile_product with the wave's 16 rows of W read from LDS (wrow: the lane's row, k contiguous) instead of registers
__device__ __forceinline__ void tile_product_lds(floatx4 (&acc)[2], const float (*xs)[H + 4], const float* wrow, int n, int q) {
  constexpr int KQ = H / 4;
  acc[0] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
  acc[1] = acc[0];
#pragma unroll
  for (int s = 0; s < KQ; s += 4) {
    const float4 a0 = *reinterpret_cast<const float4*>(&xs[n][KQ * q + s]);
    const float4 a1 = *reinterpret_cast<const float4*>(&xs[16 + n][KQ * q + s]);
    const float4 bb = *reinterpret_cast<const float4*>(&wrow[KQ * q + s]);
    const float v0[4] = {a0.x, a0.y, a0.z, a0.w}, v1[4] = {a1.x, a1.y, a1.z, a1.w}, vb[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0[j], vb[j], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1[j], vb[j], acc[1], 0, 0, 0);
    }
  }
}

// rows 128 .. 128 + W2 - 1 of the stacked weight into LDS (zeros past the last column); the caller's next barrier publishes them
template <int W2>
__device__ __forceinline__ void stage_w2(float (*w2s)[H + 4], const Heads& hd, int tid) {
#pragma unroll
  for (int j = 0; j < W2 * H / 512; ++j) {
    const int e = tid + 512 * j, r = e / H, k = e % H;
    const float* bp;
    const float* wr = stacked_row(hd, 128 + r, bp);
    w2s[r][k] = wr ? wr[k] : 0.0f;
  }
}

// The wave's slices of the tile's logits (bias added) into ls; columns past the last head come out 0. Slice w comes from the
// registers B; with SPW = 2 waves 0 .. 2 also take slice 8 + w (columns 128 .. 175) against the LDS copy of those rows of W.
template <int SPW, int LP>
__device__ __forceinline__ void logits_to_lds(float (*ls)[LP], const float (*xs)[H + 4], const float (&B)[H / 4], const float (&bias)[SPW],
                                              const float (*w2s)[H + 4], int wv, int n, int q) {
  floatx4 acc[2];
  mlpt::tile_product<H>(acc, xs, B, n, q);
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int i = 0; i < 4; ++i) ls[16 * mt + 4 * q + i][16 * wv + n] = acc[mt][i] + bias[0];
  if (SPW == 2 && 16 * (wv + 8) + 16 <= LP - 4) {
    int r2 = 16 * wv + n;
    asm volatile("" : "+v"(r2));   // opaque per tile: hoisted out of the tile loop, these loop-invariant reads would take 32 registers
    tile_product_lds(acc, xs, w2s[r2], n, q);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) ls[16 * mt + 4 * q + i][16 * (wv + 8) + n] = acc[mt][i] + bias[SPW - 1];
  }
}

// One row of the logits tile, on the 16 lanes n = 0 .. 15 of a quarter: logp and ent of the row (lane 0 writes them in the forward);
// in the backward lr is overwritten with dL/dlogit for upstream gl = dL/dlogp, ge = dL/dent. Rows past M run on zeros and store nothing.
template <bool BWD>
__device__ __forceinline__ void row_pass(const Heads& hd, float* lr, int row, int M, int n, const float* __restrict__ actions,
                                         const float* __restrict__ alpha0, const float* __restrict__ beta0, float gl, float ge,
                                         float* __restrict__ logp, float* __restrict__ ent) {
  const bool live = row < M;
  const float* arow = actions + (size_t)(live ? row : 0) * hd.act_cols;
  float lp_sum = 0.0f, ent_sum = 0.0f;
  for (int h = 0; h < hd.n_cat; ++h) {
    const int o = hd.off[h], nh = hd.off[h + 1] - o;
    const float a = live ? arow[h] : 0.0f;
    const int ia = (int)fminf(fmaxf(a, -1.0f), 1024.0f);          // (NaN -> -1)
    const bool ok = a == (float)ia && ia >= 0 && ia < nh;
    const int sel = ok ? ia : -1;                                 // a bad action matches no logit
    float m = -INFINITY;
    for (int k = n; k < nh; k += 16) m = fmaxf(m, lr[o + k]);
    m = max16(m);
    float se = 0.0f;
    for (int k = n; k < nh; k += 16) se += expf(lr[o + k] - m);
    se = sum16(se);
    const float lse = m + logf(se);
    float pl = 0.0f, tk = 0.0f;
    for (int k = n; k < nh; k += 16) {
      const float lq = lr[o + k] - lse, p = expf(lq);
      pl += p * lq;                                               // p underflowed to 0: 0 * finite = 0
      tk = k == sel ? lq : tk;
    }
    pl = sum16(pl);
    tk = sum16(tk);
    const float Hh = -pl;
    lp_sum += ok ? tk : NAN;
    ent_sum += Hh;
    if (BWD)
      for (int k = n; k < nh; k += 16) {
        const float lq = lr[o + k] - lse, p = expf(lq);
        lr[o + k] = gl * ((k == sel ? 1.0f : 0.0f) - p) - ge * (p * (lq + Hh));
      }
  }
  if (hd.shoot_cols) {
    const int o = hd.off[hd.n_cat];
    const float y0 = lr[o], y1 = lr[o + 1];
    const float a0 = live ? alpha0[row] : 1.0f, b0 = live ? beta0[row] : 1.0f;
    const float t0 = 100.0f - softplus(y0), t1 = 100.0f - softplus(y1);
    const float u0 = 100.0f - softplus(t0), u1 = 100.0f - softplus(t1);
    const float num = (1.0f + u0) + a0, den = (num + (1.0f + u1)) + b0;
    const float p = num / den;
    const float pc = fminf(fmaxf(p, BERN_EPS), 1.0f - BERN_EPS);
    const float lg = logf(pc) - log1pf(-pc);
    float vsum = 0.0f;
    for (int j = 0; j < hd.shoot_cols; ++j) {
      const float v = live ? arow[hd.n_cat + j] : 0.0f;
      lp_sum -= bce_logits(lg, v);
      vsum += v;
    }
    ent_sum += bce_logits(lg, p);                                 // counted once, whatever the number of columns
    if (BWD) {
      // d(-bce(lg, v))/dlg = v - sigmoid(lg) with sigmoid(lg) = pc; d bce(lg, p)/dlg = pc - p, d bce(lg, p)/dp = -lg
      const float g_lg = gl * (vsum - (float)hd.shoot_cols * pc) + ge * (pc - p);
      const bool inside = p >= BERN_EPS && p <= 1.0f - BERN_EPS;  // the clamp passes the gradient on its closed interval
      const float g_p = (inside ? g_lg * (1.0f / pc + 1.0f / (1.0f - pc)) : 0.0f) - ge * lg;
      const float g_u0 = g_p * (den - num) / (den * den), g_u1 = -g_p * num / (den * den);
      const float d0 = g_u0 * softplus_grad(t0) * softplus_grad(y0), d1 = g_u1 * softplus_grad(t1) * softplus_grad(y1);
      if (n == 0) {
        lr[o] = d0;
        lr[o + 1] = d1;
      }
    }
  }
  if (!BWD && live && n == 0) {
    logp[row] = lp_sum;
    ent[row] = ent_sum;
  }
}

// SPW: slices per wave (1: up to 128 columns, 2: up to 176)
template <int SPW>
__global__ __launch_bounds__(512) void act_eval_fwd(const float* __restrict__ x, const Heads hd, const float* __restrict__ actions,
                                                    const float* __restrict__ alpha0, const float* __restrict__ beta0, float* __restrict__ logp,
                                                    float* __restrict__ ent, int M, int vec) {
  constexpr int NP = SPW == 1 ? 128 : 176, LP = NP + 4;
  __shared__ __attribute__((aligned(16))) float xs[RT][H + 4];
  __shared__ __attribute__((aligned(16))) float ls[RT][LP];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
  __shared__ __attribute__((aligned(16))) float w2s[SPW == 2 ? NP - 128 : 1][H + 4];
  float B[H / 4], bias[SPW];   // W[column 16 w + n][k = 32 q + s]
#pragma unroll
  for (int sl = 0; sl < SPW; ++sl) {
    const float* bp;
    const float* wr = stacked_row(hd, 16 * (wv + 8 * sl) + n, bp);
    bias[sl] = wr ? *bp : 0.0f;
    if (sl == 0) {
#pragma unroll
      for (int s = 0; s < H / 4; ++s) B[s] = wr ? wr[H / 4 * q + s] : 0.0f;
    }
  }
  if (SPW == 2) stage_w2<NP - 128>(w2s, hd, tid);
  const int ntiles = (M + RT - 1) / RT;
  float pre[RT * H / 512];
  int tile = blockIdx.x;
  if (tile < ntiles) mlpt::load_tile<H>(pre, x, H, M, tile * RT, tid, vec);
  for (; tile < ntiles; tile += gridDim.x) {
    mlpt::store_tile<H>(pre, xs, tid, vec);
    __syncthreads();
    const int next = tile + gridDim.x;
    if (next < ntiles) mlpt::load_tile<H>(pre, x, H, M, next * RT, tid, vec);
    logits_to_lds<SPW, LP>(ls, xs, B, bias, w2s, wv, n, q);
    __syncthreads();
    row_pass<false>(hd, ls[tid >> 4], tile * RT + (tid >> 4), M, n, actions, alpha0, beta0, 0.0f, 0.0f, logp, ent);
  }
}

// One set of partial sums per workgroup at ws + blockIdx.x * 129 total: dW [total, 128] of the stacked weight, then db [total].
template <int SPW, bool DX>
__global__ __launch_bounds__(512) void act_eval_bwd(const float* __restrict__ dlogp, const float* __restrict__ dent, const float* __restrict__ x,
                                                    const Heads hd, const float* __restrict__ actions, const float* __restrict__ alpha0,
                                                    const float* __restrict__ beta0, float* __restrict__ ws, float* __restrict__ dx, int M, int vec) {
  constexpr int NP = SPW == 1 ? 128 : 176, LP = NP + 4, UQ = NP / 4, NJ = H / 16;
  __shared__ __attribute__((aligned(16))) float xs[RT][H + 4];
  __shared__ __attribute__((aligned(16))) float ls[RT][LP];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
  __shared__ __attribute__((aligned(16))) float w2s[SPW == 2 ? NP - 128 : 1][H + 4];
  float B[H / 4], bias[SPW];   // W[column 16 w + n][k = 32 q + s]
#pragma unroll
  for (int sl = 0; sl < SPW; ++sl) {
    const float* bp;
    const float* wr = stacked_row(hd, 16 * (wv + 8 * sl) + n, bp);
    bias[sl] = wr ? *bp : 0.0f;
    if (sl == 0) {
#pragma unroll
      for (int s = 0; s < H / 4; ++s) B[s] = wr ? wr[H / 4 * q + s] : 0.0f;
    }
  }
  if (SPW == 2) stage_w2<NP - 128>(w2s, hd, tid);
  float Bx[DX ? UQ : 1];   // W[column UQ q + s of the stack][input 16 w + n]: dx = dl W sums over the columns
  if (DX) {
#pragma unroll
    for (int s = 0; s < UQ; ++s) {
      const float* bp;
      const float* wr = stacked_row(hd, UQ * q + s, bp);
      Bx[s] = wr ? wr[16 * wv + n] : 0.0f;
    }
  }
  floatx4 accw[SPW][NJ];   // dW[column 16 (w + 8 sl) + 4 q + i][input 16 j + n], summed over every row this workgroup walks
  float dbias[SPW];
#pragma unroll
  for (int sl = 0; sl < SPW; ++sl) {
    dbias[sl] = 0.0f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) accw[sl][j] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  const int ntiles = (M + RT - 1) / RT;
  float pre[RT * H / 512];
  int tile = blockIdx.x;
  if (tile < ntiles) mlpt::load_tile<H>(pre, x, H, M, tile * RT, tid, vec);
  for (; tile < ntiles; tile += gridDim.x) {
    const int row0 = tile * RT;
    mlpt::store_tile<H>(pre, xs, tid, vec);
    __syncthreads();
    const int next = tile + gridDim.x;
    if (next < ntiles) mlpt::load_tile<H>(pre, x, H, M, next * RT, tid, vec);
    logits_to_lds<SPW, LP>(ls, xs, B, bias, w2s, wv, n, q);
    __syncthreads();
    {
      // rows past M have no upstream gradient: their dl comes out 0 and adds nothing to any sum
      const int row = row0 + (tid >> 4);
      const float gl = (dlogp && row < M) ? dlogp[row] : 0.0f, ge = (dent && row < M) ? dent[row] : 0.0f;
      row_pass<true>(hd, ls[tid >> 4], row, M, n, actions, alpha0, beta0, gl, ge, nullptr, nullptr);
    }
    __syncthreads();
    // dW += dl^T x: the step over rows {4 q + i} takes A = dl[row][column 16 s + n] and B = x[row][16 j + n]
#pragma unroll
    for (int sl = 0; sl < SPW; ++sl) {
      const int c0 = 16 * (wv + 8 * sl);
      if (c0 + 16 <= NP) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int r = 16 * mt + 4 * q + i;
            const float d = ls[r][c0 + n];
            const float* xr = &xs[r][n];
            dbias[sl] += d;
#pragma unroll
            for (int j = 0; j < NJ; ++j) accw[sl][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(d, xr[16 * j], accw[sl][j], 0, 0, 0);
          }
      }
    }
    if (DX) {
      floatx4 ad[2] = {floatx4{0.0f, 0.0f, 0.0f, 0.0f}, floatx4{0.0f, 0.0f, 0.0f, 0.0f}};
#pragma unroll
      for (int s = 0; s < UQ; s += 4) {
        const float4 a0 = *reinterpret_cast<const float4*>(&ls[n][UQ * q + s]);
        const float4 a1 = *reinterpret_cast<const float4*>(&ls[16 + n][UQ * q + s]);
        const float v0[4] = {a0.x, a0.y, a0.z, a0.w}, v1[4] = {a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ad[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0[j], Bx[DX ? s + j : 0], ad[0], 0, 0, 0);
          ad[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1[j], Bx[DX ? s + j : 0], ad[1], 0, 0, 0);
        }
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = row0 + 16 * mt + 4 * q + i;
          if (row < M) dx[(size_t)row * H + 16 * wv + n] = ad[mt][i];
        }
    }
    __syncthreads();   // every read of xs and ls of this tile is behind
  }
  float* base = ws + (size_t)blockIdx.x * ((H + 1) * hd.total);
#pragma unroll
  for (int sl = 0; sl < SPW; ++sl) {
    const int c0 = 16 * (wv + 8 * sl);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = c0 + 4 * q + i;
        if (c < hd.total) base[(size_t)c * H + 16 * j + n] = accw[sl][j][i];
      }
    // the four quarters hold different rows' shares of the same column
    float d = dbias[sl];
    d += __shfl_xor(d, 16);
    d += __shfl_xor(d, 32);
    if (q == 0 && c0 + n < hd.total) base[H * hd.total + c0 + n] = d;
  }
}

// dW_h, db_h of every head = the sum of the G partial sets (trn::sum_sets)
__global__ __launch_bounds__(256) void act_eval_reduce(const float* __restrict__ ws, int G, const Heads hd, const Grads gr) {
  const int nel = (H + 1) * hd.total;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nel) return;
  const float s = trn::sum_sets(ws, G, nel, e);
  const bool isw = e < H * hd.total;
  const int c = isw ? e / H : e - H * hd.total;
  float* dst = nullptr;
#pragma unroll
  for (int h = 0; h < MAXH; ++h) {
    const bool in = c >= hd.off[h] && c < hd.off[h + 1];
    float* p = isw ? gr.dw[h] + (size_t)(c - hd.off[h]) * H + e % H : gr.db[h] + (c - hd.off[h]);
    dst = in ? p : dst;
  }
  *dst = s;
}
}  // namespace actt

// ------------------------------------------------------------------------------------------------ C ABI (include/aircombat.h)
extern "C" {
// the checked configuration: 0 and the stacked column count (categorical logits, then two for the shoot head), or -1 with the message
static int act_heads_ok(const char* who, const ac_act_heads_t* hs, int32_t M, int* total) {
  const std::string w(who);
  if (!hs) return fail(w + ": null argument");
  if (M < 1) return fail(w + ": M must be at least 1");
  if (hs->n_cat < 1 || hs->n_cat > 8) return fail(w + ": n_cat must be 1 .. 8");
  int sum = 0;
  for (int i = 0; i < hs->n_cat; ++i) {
    if (hs->nvec[i] < 2) return fail(w + ": head " + std::to_string(i) + " has size " + std::to_string(hs->nvec[i]) + " (at least 2)");
    if (hs->nvec[i] > actt::MAX_LOGITS) return fail(w + ": the heads have more than 160 logits");
    sum += hs->nvec[i];
  }
  if (sum > actt::MAX_LOGITS) return fail(w + ": the heads have " + std::to_string(sum) + " logits (at most 160)");
  if (hs->n_shoot_cols != 0 && hs->n_shoot_cols != 1 && hs->n_shoot_cols != 4) return fail(w + ": n_shoot_cols must be 0, 1 or 4");
  if (trn::rows_fit_i32(w, M, mlpt::H, mlpt::RT)) return -1;
  *total = sum + (hs->n_shoot_cols ? 2 : 0);
  return 0;
}

// the kernels' view of the heads; -1 if one of the per-head pointers is NULL (w, b; dw, db when given)
static int act_heads_pack(const char* who, const ac_act_heads_t* hs, int total, const float* const* d_w, const float* const* d_b,
                          float* const* d_dw, float* const* d_db, actt::Heads* hd, actt::Grads* gr) {
  const int nh = hs->n_cat + (hs->n_shoot_cols ? 1 : 0);
  int off = 0;
  for (int h = 0; h < actt::MAXH; ++h) {
    hd->off[h] = h < nh ? off : total;
    hd->w[h] = h < nh ? d_w[h] : nullptr;
    hd->b[h] = h < nh ? d_b[h] : nullptr;
    if (gr) {
      gr->dw[h] = h < nh ? d_dw[h] : nullptr;
      gr->db[h] = h < nh ? d_db[h] : nullptr;
    }
    if (h < nh && (!hd->w[h] || !hd->b[h] || (gr && (!gr->dw[h] || !gr->db[h])))) return fail(std::string(who) + ": null argument (head " + std::to_string(h) + ")");
    if (h < nh) off += h < hs->n_cat ? hs->nvec[h] : 2;
  }
  hd->off[actt::MAXH] = total;
  hd->n_cat = hs->n_cat;
  hd->total = total;
  hd->shoot_cols = hs->n_shoot_cols;
  hd->act_cols = hs->n_cat + hs->n_shoot_cols;
  return 0;
}

int64_t ac_act_eval_workspace_floats(const ac_act_heads_t* heads, int32_t M) {
  int total;
  if (act_heads_ok("ac_act_eval_workspace_floats", heads, M, &total)) return -1;
  return (int64_t)trn::capped_tiles(M, mlpt::RT, mlpt::BWD_WGS) * (mlpt::H + 1) * total;
}

int ac_act_eval_forward(int32_t device_id, void* stream, const ac_act_heads_t* heads, int32_t M, const float* d_x, const float* const* d_w,
                        const float* const* d_b, const float* d_actions, const float* d_alpha0, const float* d_beta0, float* d_logp,
                        float* d_ent) {
  const char* who = "ac_act_eval_forward";
  int total;
  if (act_heads_ok(who, heads, M, &total)) return -1;
  if (!d_x || !d_w || !d_b || !d_actions || !d_logp || !d_ent) return fail(std::string(who) + ": null argument");
  if (heads->n_shoot_cols && (!d_alpha0 || !d_beta0)) return fail(std::string(who) + ": shoot columns need alpha0 and beta0");
  actt::Heads hd;
  if (act_heads_pack(who, heads, total, d_w, d_b, nullptr, nullptr, &hd, nullptr)) return -1;
  HIP_OK(hipSetDevice(device_id));
  const dim3 grid(trn::capped_tiles(M, mlpt::RT, mlpt::FWD_WGS)), block(512);
  const int vec = mlp_vec(d_x, mlpt::H, mlpt::H);
  if (total <= 128)
    hipLaunchKernelGGL(actt::act_eval_fwd<1>, grid, block, 0, (hipStream_t)stream, d_x, hd, d_actions, d_alpha0, d_beta0, d_logp, d_ent, (int)M, vec);
  else
    hipLaunchKernelGGL(actt::act_eval_fwd<2>, grid, block, 0, (hipStream_t)stream, d_x, hd, d_actions, d_alpha0, d_beta0, d_logp, d_ent, (int)M, vec);
  HIP_OK(hipGetLastError());
  return 0;
}

int ac_act_eval_backward(int32_t device_id, void* stream, const ac_act_heads_t* heads, int32_t M, const float* d_dlogp, const float* d_dent,
                         const float* d_x, const float* const* d_w, const float* const* d_b, const float* d_actions, const float* d_alpha0,
                         const float* d_beta0, float* d_workspace, float* d_dx, float* const* d_dw, float* const* d_db) {
  const char* who = "ac_act_eval_backward";
  int total;
  if (act_heads_ok(who, heads, M, &total)) return -1;
  if (!d_x || !d_w || !d_b || !d_actions || !d_workspace || !d_dw || !d_db) return fail(std::string(who) + ": null argument");
  if (heads->n_shoot_cols && (!d_alpha0 || !d_beta0)) return fail(std::string(who) + ": shoot columns need alpha0 and beta0");
  actt::Heads hd;
  actt::Grads gr;
  if (act_heads_pack(who, heads, total, d_w, d_b, d_dw, d_db, &hd, &gr)) return -1;
  HIP_OK(hipSetDevice(device_id));
  const int G = trn::capped_tiles(M, mlpt::RT, mlpt::BWD_WGS);
  const dim3 grid(G), block(512);
  const int vec = mlp_vec(d_x, mlpt::H, mlpt::H);
#define AC_ACT_BWD(SPW)                                                                                                                       \
  if (d_dx)                                                                                                                                   \
    hipLaunchKernelGGL((actt::act_eval_bwd<SPW, true>), grid, block, 0, (hipStream_t)stream, d_dlogp, d_dent, d_x, hd, d_actions, d_alpha0,  \
                       d_beta0, d_workspace, d_dx, (int)M, vec);                                                                              \
  else                                                                                                                                        \
    hipLaunchKernelGGL((actt::act_eval_bwd<SPW, false>), grid, block, 0, (hipStream_t)stream, d_dlogp, d_dent, d_x, hd, d_actions, d_alpha0, \
                       d_beta0, d_workspace, d_dx, (int)M, vec)
  if (total <= 128) { AC_ACT_BWD(1); } else { AC_ACT_BWD(2); }
#undef AC_ACT_BWD
  HIP_OK(hipGetLastError());
  const int nel = (mlpt::H + 1) * total;
  hipLaunchKernelGGL(actt::act_eval_reduce, dim3((nel + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)d_workspace, G, hd, gr);
  HIP_OK(hipGetLastError());
  return 0;
}
}  // extern "C"
