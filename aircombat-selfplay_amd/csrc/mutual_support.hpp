// The mutual-support discriminator on the device (include/aircombat_mutual.h; DESIGN.md, "The mutual-support scorer"): the intrinsic
// rewards of a whole rollout in ONE launch, and the gather of the discriminator's training mini-batches.
//
// mi_score_kernel. Rows are the 2 n E tuples, row g = 2 (sl E + e) + j (step s0 + sl, env e, tuple j): an env's two tuples are adjacent
// rows and share the 128 floats of h. A workgroup of eight waves walks 128-row tiles in a persistent loop, one workgroup per CU: the
// tile's activations live in ONE LDS image [128][260] (130 KiB) that is rewritten in place layer by layer, so nothing between x and the
// squared error ever reaches HBM. Per net (pred, then pred_wo):
//   x      built on chip from RNN_ACTOR / ACTIONS into the image (row stride 164), zero-padded to a multiple of 16 columns;
//   L1/L2  wave w owns output units 32 w .. 32 w + 31 for all 128 rows: 8 x 2 accumulators of v_mfma_f32_16x16x4_f32 (exact fp32
//          products and sums, as mlp_train.hpp). The A operand is a float4 of the image with the k order permuted (lane quarter q takes
//          k = KQ q + s, so LDS reads and weight reads are both contiguous); the B operand is a float4 of the weight row, read straight
//          from the torch parameter ([out][in], L2-resident: 0.9 MB for both nets) one k-chunk ahead of its use. Each 16-byte weight read
//          feeds 32 MFMAs (8 row tiles x 4 k-steps): that is what the 128-row tile is for. After a barrier relu(z + b) replaces the
//          image's contents;
//   L3     wave w owns ROWS 16 w .. 16 w + 15 and walks the ceil(D / 16) column tiles, so every wave works whatever D is and a row's
//          squared error is summed inside one wave: over the column tiles in a lane, then over the 16 lanes of a quarter with shuffles.
//          Padding columns (>= D) are left out of the sum; the mean divides by D.
// Lane 0 of each quarter ends up with both nets' MSEs of rows 4 q .. 4 q + 3 of the wave's 16 (two envs) and writes r_int, mse and
// REWARDS += ratio r_int for them: every (s, e, a) has one writer, there are no atomics and the result does not depend on the grid.
//
// mi_gather_kernel only copies: one wave per output row of X / Y.
#pragma once
#include "../../include/aircombat_mutual.h"

namespace mi {
typedef float floatx4 __attribute__((ext_vector_type(4)));
constexpr int H = AC_MI_HIDDEN, W = AC_MI_WIDTH;
constexpr int RT = 128;        // rows per tile
constexpr int NT = 512;        // eight waves
constexpr int LS = W + 4;      // row stride of the activation image (4 mod 64 banks: the float4 reads of 16 rows are conflict-free)
constexpr int XS = 164;        // row stride of the x image: up to 160 columns, 164 = 36 mod 64 spreads 16 rows over all banks
constexpr int XU = 40;         // float4 units per x row
constexpr int MAX_WGS = 256;   // one workgroup per CU (LDS)

struct Net { const float *w0, *b0, *w1, *b1, *w2, *b2; };
struct Score {
  int E, na, D, C, s0, n, add;
  float ratio;
  const float *OBS, *ACT, *RNN;
  float* REW;
  Net net[2];
  float *r_int, *mse;
  int vec[2][2];     // 16-byte weight rows: [net][w1, w2]
};

__device__ __forceinline__ float sum16(float v) {   // over the 16 lanes of a quarter, in a fixed order
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// W[u][k0 .. k0 + 3] of a row-major [.][K] matrix, 0 past K
__device__ __forceinline__ float4 load_w4(const float* __restrict__ w, int u, int K, int k0, int vec) {
  const float* p = w + (size_t)u * K + k0;
  if (vec) return *reinterpret_cast<const float4*>(p);
  float4 t;
  t.x = k0 < K ? p[0] : 0.0f;
  t.y = k0 + 1 < K ? p[1] : 0.0f;
  t.z = k0 + 2 < K ? p[2] : 0.0f;
  t.w = k0 + 3 < K ? p[3] : 0.0f;
  return t;
}

// acc[rt][j][i] = sum_k img[16 rt + 4 q + i][k] W[32 wv + 16 j + n][k] over k < 4 KQ (W is 0 past K)
__device__ __forceinline__ void dense(floatx4 (&acc)[8][2], const float* img, int stride, const float* __restrict__ w, int K, int KQ, int vec,
                                      int wv, int n, int q) {
#pragma unroll
  for (int rt = 0; rt < 8; ++rt) {
    acc[rt][0] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
    acc[rt][1] = acc[rt][0];
  }
  const int u0 = 32 * wv + n, u1 = u0 + 16;
  float4 n0 = load_w4(w, u0, K, KQ * q, vec), n1 = load_w4(w, u1, K, KQ * q, vec);
#pragma unroll 1
  for (int s = 0; s < KQ; s += 4) {
    const float4 c0 = n0, c1 = n1;
    if (s + 4 < KQ) {
      n0 = load_w4(w, u0, K, KQ * q + s + 4, vec);
      n1 = load_w4(w, u1, K, KQ * q + s + 4, vec);
    }
    const float b0[4] = {c0.x, c0.y, c0.z, c0.w}, b1[4] = {c1.x, c1.y, c1.z, c1.w};
#pragma unroll
    for (int rt = 0; rt < 8; ++rt) {
      const float4 a4 = *reinterpret_cast<const float4*>(&img[(16 * rt + n) * stride + KQ * q + s]);
      const float a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[rt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b0[e], acc[rt][0], 0, 0, 0);
        acc[rt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b1[e], acc[rt][1], 0, 0, 0);
      }
    }
  }
}

// relu(acc + b) into the activation image, in the product's result layout
__device__ __forceinline__ void store_act(const floatx4 (&acc)[8][2], float* img, const float* __restrict__ b, int wv, int n, int q) {
  const float bias0 = b[32 * wv + n], bias1 = b[32 * wv + 16 + n];
#pragma unroll
  for (int rt = 0; rt < 8; ++rt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float z0 = acc[rt][0][i] + bias0, z1 = acc[rt][1][i] + bias1;
      float* row = &img[(16 * rt + 4 * q + i) * LS + 32 * wv + n];
      row[0] = z0 > 0.0f ? z0 : 0.0f;
      row[16] = z1 > 0.0f ? z1 : 0.0f;
    }
}

__global__ __launch_bounds__(NT) void mi_score_kernel(const Score a) {
  __shared__ __attribute__((aligned(16))) float img[RT * LS];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
  const int E = a.E, D = a.D, C = a.C;
  const int64_t N = (int64_t)E * a.na, M = 2 * (int64_t)a.n * E;
  const int64_t ntiles = (M + RT - 1) / RT;
  const int DT = (D + 15) / 16;
  const float inv_d = 1.0f / (float)D;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * RT;
    // the four rows this lane's accumulators hold in layer 3: 16 wv + 4 q + i
    int64_t yoff[4];
    bool live[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t g = row0 + 16 * wv + 4 * q + i;
      live[i] = g < M;
      const int64_t p = live[i] ? g >> 1 : 0, sl = p / E, e = p - sl * E;
      yoff[i] = (((int64_t)a.s0 + sl + 1) * N + e * a.na + (g & 1)) * D;
    }
    float mse[2][4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const Net& net = a.net[k];
      const int Kin = H + (k == 0 ? 2 * C : C);     // pred_wo reads the first 128 + C columns
      const int KQ1 = ((Kin + 15) / 16) * 4;        // a quarter's share of the padded k range
      __syncthreads();                              // the image's previous readers are done
      // ---- x: [h, own action, partner's action (pred only), 0 ...]
      for (int f = tid; f < RT * XU; f += NT) {
        const int r = f / XU, c4 = f - r * XU;
        const int64_t g = row0 + r;
        float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (g < M && 4 * c4 < 4 * KQ1) {
          const int64_t p = g >> 1, sl = p / E, e = p - sl * E;
          const int64_t r0 = ((int64_t)a.s0 + sl) * N + e * a.na;
          const int j = (int)(g & 1);
          if (c4 < H / 4) {
            v = *reinterpret_cast<const float4*>(a.RNN + r0 * H + 4 * c4);
          } else {
            const float* own = a.ACT + (r0 + j) * C;
            const float* oth = a.ACT + (r0 + 1 - j) * C;
            float t[4];
#pragma unroll
            for (int z = 0; z < 4; ++z) {
              const int c = 4 * c4 + z - H;
              t[z] = c < C ? own[c] : (c + H < Kin ? oth[c - C] : 0.0f);
            }
            v = make_float4(t[0], t[1], t[2], t[3]);
          }
        }
        *reinterpret_cast<float4*>(&img[r * XS + 4 * c4]) = v;
      }
      __syncthreads();
      floatx4 acc[8][2];
      dense(acc, img, XS, net.w0, Kin, KQ1, 0, wv, n, q);
      __syncthreads();
      store_act(acc, img, net.b0, wv, n, q);
      __syncthreads();
      dense(acc, img, LS, net.w1, W, W / 4, a.vec[k][0], wv, n, q);
      __syncthreads();
      store_act(acc, img, net.b1, wv, n, q);
      __syncthreads();
      // ---- last layer and the squared error of this wave's 16 rows
      float se[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      const float* arow = &img[(16 * wv + n) * LS + (W / 4) * q];
#pragma unroll 1
      for (int ct = 0; ct < DT; ++ct) {
        const int u = 16 * ct + n;
        const bool col = u < D;
        const int uc = col ? u : D - 1;     // a padding column reads the last real row of the weights; its result is not used
        floatx4 c0 = {0.0f, 0.0f, 0.0f, 0.0f}, c1 = c0;
#pragma unroll 2
        for (int s = 0; s < W / 4; s += 8) {
          const float4 w0 = load_w4(net.w2, uc, W, (W / 4) * q + s, a.vec[k][1]);
          const float4 w1 = load_w4(net.w2, uc, W, (W / 4) * q + s + 4, a.vec[k][1]);
          const float4 x0 = *reinterpret_cast<const float4*>(arow + s);
          const float4 x1 = *reinterpret_cast<const float4*>(arow + s + 4);
          c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.x, w0.x, c0, 0, 0, 0);
          c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.x, w1.x, c1, 0, 0, 0);
          c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.y, w0.y, c0, 0, 0, 0);
          c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.y, w1.y, c1, 0, 0, 0);
          c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.z, w0.z, c0, 0, 0, 0);
          c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.z, w1.z, c1, 0, 0, 0);
          c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.w, w0.w, c0, 0, 0, 0);
          c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.w, w1.w, c1, 0, 0, 0);
        }
        const float bias = net.b2[uc];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float y = (col && live[i]) ? a.OBS[yoff[i] + u] : 0.0f;
          const float d = (c0[i] + c1[i]) + bias - y;
          se[i] += col ? d * d : 0.0f;
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) mse[k][i] = sum16(se[i]) * inv_d;
    }
    // ---- lane 0 of each quarter: the two envs of rows 4 q .. 4 q + 3
    if (n == 0) {
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int64_t g = row0 + 16 * wv + 4 * q + 2 * h2;
        if (g < M) {
          const int64_t p = g >> 1, sl = p / E, e = p - sl * E;
          // score(j) = mse_wo(j) - mse_with(j); agent 1 takes tuple 0's, agent 0 tuple 1's
          const float r0 = mse[1][2 * h2 + 1] - mse[0][2 * h2 + 1], r1 = mse[1][2 * h2] - mse[0][2 * h2];
          if (a.mse) {
            float* o = a.mse + p * 4;
            o[0] = mse[0][2 * h2]; o[1] = mse[1][2 * h2];
            o[2] = mse[0][2 * h2 + 1]; o[3] = mse[1][2 * h2 + 1];
          }
          if (a.r_int) {
            a.r_int[p * 2] = r0;
            a.r_int[p * 2 + 1] = r1;
          }
          if (a.add) {
            float* rw = a.REW + ((int64_t)a.s0 + sl) * N + e * a.na;
            // product and sum rounded separately, as the host row function's (the empty asm keeps the compiler from fusing them into
            // one fma): the two forms give the same bits for the same r_int
            float t0 = a.ratio * r0, t1 = a.ratio * r1;
            asm volatile("" : "+v"(t0), "+v"(t1));
            rw[0] += t0;
            rw[1] += t1;
          }
        }
      }
    }
  }
}

// the source of output row `row` of the gather: tuple j of env e at step t
struct Src { int64_t h, own, oth, y; };
__host__ __device__ __forceinline__ Src gather_src(int64_t row, int m, int E, int na, int C, int D, int T, const int32_t* times) {
  const int64_t per = (int64_t)m * E, j = row / per, rest = row - j * per, i = rest / E, e = rest - i * E;
  int64_t t = times[i];
  t = t < 0 ? 0 : (t > T - 1 ? T - 1 : t);      // memory safety, not validation
  const int64_t N = (int64_t)E * na, r0 = t * N + e * na;
  return Src{r0 * H, (r0 + j) * C, (r0 + 1 - j) * C, ((t + 1) * N + e * na + j) * D};
}

__global__ __launch_bounds__(256) void mi_gather_kernel(const float* __restrict__ OBS, const float* __restrict__ ACT, const float* __restrict__ RNN,
                                                        const int32_t* __restrict__ times, float* __restrict__ X, float* __restrict__ Y, int m, int E,
                                                        int na, int C, int D, int T) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), rows = 2 * (int64_t)m * E;
  if (row >= rows) return;
  const Src s = gather_src(row, m, E, na, C, D, T, times);
  float* x = X + row * (H + 2 * C);
  x[lane] = RNN[s.h + lane];
  x[lane + 64] = RNN[s.h + lane + 64];
  if (lane < C) x[H + lane] = ACT[s.own + lane];
  else if (lane < 2 * C) x[H + lane] = ACT[s.oth + lane - C];
  for (int d = lane; d < D; d += 64) Y[row * D + d] = OBS[s.y + d];
}

// one net on one row, plain fp32 in index order
static float net_mse_host(const Net& net, const float* x, int Kin, const float* y, int D) {
  float a1[W], a2[W];
  for (int u = 0; u < W; ++u) {
    float z = 0.0f;
    for (int k = 0; k < Kin; ++k) z += x[k] * net.w0[(size_t)u * Kin + k];
    z += net.b0[u];
    a1[u] = z > 0.0f ? z : 0.0f;
  }
  for (int u = 0; u < W; ++u) {
    float z = 0.0f;
    for (int k = 0; k < W; ++k) z += a1[k] * net.w1[(size_t)u * W + k];
    z += net.b1[u];
    a2[u] = z > 0.0f ? z : 0.0f;
  }
  float se = 0.0f;
  for (int d = 0; d < D; ++d) {
    float z = 0.0f;
    for (int k = 0; k < W; ++k) z += a2[k] * net.w2[(size_t)d * W + k];
    const float diff = z + net.b2[d] - y[d];
    se += diff * diff;
  }
  return se / (float)D;
}
}  // namespace mi

static int mi_shapes_ok(const char* fn, int32_t E, int32_t na, int32_t T, int32_t D, int32_t C, int32_t hidden) {
  if (C < 1 || C > AC_MI_MAX_ACT) return fail(std::string(fn) + ": act_dim " + std::to_string(C) + " is outside 1 .. 12");
  if (D < 1 || D > AC_MI_MAX_OBS) return fail(std::string(fn) + ": obs_dim " + std::to_string(D) + " is outside 1 .. 128");
  if (hidden != AC_MI_HIDDEN) return fail(std::string(fn) + ": hidden " + std::to_string(hidden) + " is not 128");
  if (na < 2) return fail(std::string(fn) + ": na " + std::to_string(na) + " is below 2");
  if (E < 1) return fail(std::string(fn) + ": E " + std::to_string(E) + " is below 1");
  if (T < 1) return fail(std::string(fn) + ": T " + std::to_string(T) + " is below 1");
  return 0;
}

static int mi_score_check(const char* fn, const ac_mi_score_t* a) {
  if (!a) return fail(std::string(fn) + ": null argument");
  if (mi_shapes_ok(fn, a->E, a->na, a->T, a->obs_dim, a->act_dim, a->hidden)) return -1;
  if (a->s0 < 0) return fail(std::string(fn) + ": s0 " + std::to_string(a->s0) + " is negative");
  if (a->n < 1) return fail(std::string(fn) + ": n " + std::to_string(a->n) + " is below 1");
  if ((int64_t)a->s0 + a->n > a->T) return fail(std::string(fn) + ": s0 + n = " + std::to_string((int64_t)a->s0 + a->n) + " exceeds T = " + std::to_string(a->T));
  if ((int64_t)a->n * a->E > (int64_t)0x3fffffff - mi::RT) return fail(std::string(fn) + ": n * E = " + std::to_string((int64_t)a->n * a->E) + " is too many rows for one launch");
  if (!a->OBS || !a->ACTIONS || !a->RNN_ACTOR || !a->p_w0 || !a->p_b0 || !a->p_w1 || !a->p_b1 || !a->p_w2 || !a->p_b2 || !a->q_w0 || !a->q_b0 ||
      !a->q_w1 || !a->q_b1 || !a->q_w2 || !a->q_b2)
    return fail(std::string(fn) + ": null array or weight pointer");
  if (a->add && !a->REWARDS) return fail(std::string(fn) + ": add is set and REWARDS is NULL");
  return 0;
}

static mi::Score mi_score_args(const ac_mi_score_t* a) {
  mi::Score s;
  memset(&s, 0, sizeof s);
  s.E = a->E; s.na = a->na; s.D = a->obs_dim; s.C = a->act_dim; s.s0 = a->s0; s.n = a->n; s.add = a->add != 0;
  s.ratio = a->ratio;
  s.OBS = a->OBS; s.ACT = a->ACTIONS; s.RNN = a->RNN_ACTOR; s.REW = a->REWARDS;
  s.net[0] = mi::Net{a->p_w0, a->p_b0, a->p_w1, a->p_b1, a->p_w2, a->p_b2};
  s.net[1] = mi::Net{a->q_w0, a->q_b0, a->q_w1, a->q_b1, a->q_w2, a->q_b2};
  s.r_int = a->r_int; s.mse = a->mse;
  for (int k = 0; k < 2; ++k) {
    s.vec[k][0] = ((uintptr_t)s.net[k].w1 & 15) == 0;
    s.vec[k][1] = ((uintptr_t)s.net[k].w2 & 15) == 0;
  }
  return s;
}

static int mi_gather_check(const char* fn, const ac_mi_gather_t* a) {
  if (!a) return fail(std::string(fn) + ": null argument");
  if (mi_shapes_ok(fn, a->E, a->na, a->T, a->obs_dim, a->act_dim, a->hidden)) return -1;
  if (a->m < 1) return fail(std::string(fn) + ": m " + std::to_string(a->m) + " is below 1");
  if (2 * (int64_t)a->m * a->E > (int64_t)0x7fffffff) return fail(std::string(fn) + ": 2 * m * E = " + std::to_string(2 * (int64_t)a->m * a->E) + " is too many rows for one launch");
  if (!a->OBS || !a->ACTIONS || !a->RNN_ACTOR || !a->times || !a->X || !a->Y) return fail(std::string(fn) + ": null pointer");
  return 0;
}

extern "C" {

int ac_mi_score(const ac_mi_score_t* args, void* stream) {
  const char* fn = "ac_mi_score";
  if (mi_score_check(fn, args)) return -1;
  if ((uintptr_t)args->RNN_ACTOR & 15) return fail(std::string(fn) + ": RNN_ACTOR is not 16-byte aligned");
  const mi::Score s = mi_score_args(args);
  const int64_t ntiles = (2 * (int64_t)s.n * s.E + mi::RT - 1) / mi::RT;
  const dim3 grid((unsigned)(ntiles < mi::MAX_WGS ? ntiles : mi::MAX_WGS)), block(mi::NT);
  hipLaunchKernelGGL(mi::mi_score_kernel, grid, block, 0, (hipStream_t)stream, s);
  HIP_OK(hipGetLastError());
  return 0;
}

int ac_mi_score_host(const ac_mi_score_t* args) {
  const char* fn = "ac_mi_score_host";
  if (mi_score_check(fn, args)) return -1;
  const mi::Score s = mi_score_args(args);
  const int C = s.C, D = s.D, E = s.E;
  const int64_t N = (int64_t)E * s.na;
  float x[mi::H + 2 * AC_MI_MAX_ACT];
  for (int64_t p = 0; p < (int64_t)s.n * E; ++p) {
    const int64_t sl = p / E, e = p % E, r0 = ((int64_t)s.s0 + sl) * N + e * s.na;
    float m[2][2];   // [tuple][with, wo]
    for (int j = 0; j < 2; ++j) {
      memcpy(x, s.RNN + r0 * mi::H, sizeof(float) * mi::H);
      memcpy(x + mi::H, s.ACT + (r0 + j) * C, sizeof(float) * C);
      memcpy(x + mi::H + C, s.ACT + (r0 + 1 - j) * C, sizeof(float) * C);
      const float* y = s.OBS + (((int64_t)s.s0 + sl + 1) * N + e * s.na + j) * D;
      m[j][0] = mi::net_mse_host(s.net[0], x, mi::H + 2 * C, y, D);
      m[j][1] = mi::net_mse_host(s.net[1], x, mi::H + C, y, D);
    }
    const float r0i = m[1][1] - m[1][0], r1i = m[0][1] - m[0][0];
    if (s.mse) { float* o = s.mse + p * 4; o[0] = m[0][0]; o[1] = m[0][1]; o[2] = m[1][0]; o[3] = m[1][1]; }
    if (s.r_int) { s.r_int[p * 2] = r0i; s.r_int[p * 2 + 1] = r1i; }
    if (s.add) {
      float* rw = s.REW + ((int64_t)s.s0 + sl) * N + e * s.na;
      rw[0] += s.ratio * r0i;
      rw[1] += s.ratio * r1i;
    }
  }
  return 0;
}

int ac_mi_gather(const ac_mi_gather_t* args, void* stream) {
  const char* fn = "ac_mi_gather";
  if (mi_gather_check(fn, args)) return -1;
  const int64_t rows = 2 * (int64_t)args->m * args->E;
  hipLaunchKernelGGL(mi::mi_gather_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, args->OBS, args->ACTIONS,
                     args->RNN_ACTOR, args->times, args->X, args->Y, (int)args->m, (int)args->E, (int)args->na, (int)args->act_dim,
                     (int)args->obs_dim, (int)args->T);
  HIP_OK(hipGetLastError());
  return 0;
}

int ac_mi_gather_host(const ac_mi_gather_t* args) {
  const char* fn = "ac_mi_gather_host";
  if (mi_gather_check(fn, args)) return -1;
  const int C = args->act_dim, D = args->obs_dim;
  for (int i = 0; i < args->m; ++i)
    if (args->times[i] < 0 || args->times[i] >= args->T)
      return fail(std::string(fn) + ": time index " + std::to_string(args->times[i]) + " is outside 0 .. T - 1");
  const int64_t rows = 2 * (int64_t)args->m * args->E;
  for (int64_t row = 0; row < rows; ++row) {
    const mi::Src s = mi::gather_src(row, args->m, args->E, args->na, C, D, args->T, args->times);
    float* x = args->X + row * (mi::H + 2 * C);
    memcpy(x, args->RNN_ACTOR + s.h, sizeof(float) * mi::H);
    memcpy(x + mi::H, args->ACTIONS + s.own, sizeof(float) * C);
    memcpy(x + mi::H + C, args->ACTIONS + s.oth, sizeof(float) * C);
    memcpy(args->Y + row * D, args->OBS + s.y, sizeof(float) * D);
  }
  return 0;
}

}  // extern "C"
