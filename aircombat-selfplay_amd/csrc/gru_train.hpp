// The PPO update's GRU on the device ("The training GRU"): the reference's one-layer GRULayer (algorithms/utils/gru.py),
// input 128, hidden 128, torch's gate order r, z, n and n = tanh(Wi_n x + b_in + r * (Wh_n h + b_hn)), over a whole minibatch of
// chunks in one launch per direction. Rows are T-major ([T * N, .], row t * N + j = step t of chunk j), as recurrent_generator yields
// them. The input products Gi = x W_ihᵀ + b_ih and the weight gradients are large GEMMs the caller runs (torch, or the kernels of gru_layer_train.hpp); what is here is
// the recurrence torch cannot batch: the hidden product, the gates, the masks and the reverse-time loop.
//
// One workgroup of eight waves owns 16 chunks (one 16-row M-tile) for all T steps. Wave w owns hidden units 16 w .. 16 w + 15, and W_hh
// is held in registers for the whole time loop as fp32 operands of v_mfma_f32_16x16x4_f32 (exact fp32 products and sums, the
// arithmetic of an fp32 GEMM): the forward wave holds its 48 gate columns x 128 k (96 VGPRs), the backward wave the transposed slice,
// 384 k x its 16 units (96 VGPRs). The only per-step traffic through LDS is the A operand: the 16 x 128 masked state (forward) or the
// 16 x 384 hidden-side gate gradients (backward), double-buffered so one barrier per step suffices. The state h and the carried dh stay
// fp32 in the registers of the lane that owns (row, unit): the MFMA result layout (row 4 (lane / 16) + i, column lane % 16) is the same
// (row, unit) map the gate algebra uses, so no value crosses lanes outside the product.
//
// The k order inside the product is a permutation (lane quarter q takes k = 32 q + s, or 96 q + s): each lane then reads its A operands
// as contiguous float4 from LDS, and the row strides (132, 388 floats: 4 mod 64 banks) keep the 16 rows of a quarter on distinct banks.
#pragma once

namespace grut {
typedef float floatx4 __attribute__((ext_vector_type(4)));
constexpr int H = 128, G = 384;
constexpr int RT = 16;                  // chunks per workgroup (one M-tile)
constexpr int HP = H + 4, GP = G + 4;   // LDS row strides
constexpr int SAVED = 4 * H;            // floats saved per (t, row) for the backward: r, z, n, Wh_n h + b_hn

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// y [T*N, 128] = h_t; h_T [N, 128]; saved [T*N, 512] (NULL: inference, nothing saved). Each step starts from h_in = h_{t-1} * m_t.
__global__ __launch_bounds__(512) void gru_seq_fwd(const float* __restrict__ gi, const float* __restrict__ hxs, const float* __restrict__ masks,
                                                   const float* __restrict__ whh, const float* __restrict__ bhh, float* __restrict__ y,
                                                   float* __restrict__ h_T, float* __restrict__ saved, int N, int T) {
  __shared__ __attribute__((aligned(16))) float hs[2][RT][HP];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
  const int u = 16 * w + n;
  const int row0 = blockIdx.x * RT;
  // B operands: W_hh[gate row g * 128 + u][k = 32 q + s]
  float B[3][32];
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int s = 0; s < 32; s += 4) {
      const float4 v = *reinterpret_cast<const float4*>(whh + (size_t)(g * H + u) * H + 32 * q + s);
      B[g][s] = v.x; B[g][s + 1] = v.y; B[g][s + 2] = v.z; B[g][s + 3] = v.w;
    }
  const float bh_r = bhh[u], bh_z = bhh[H + u], bh_n = bhh[2 * H + u];
  bool ok[4];
  float h[4], m[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = row0 + 4 * q + i;
    ok[i] = row < N;
    h[i] = ok[i] ? hxs[(size_t)row * H + u] : 0.0f;
    m[i] = ok[i] ? masks[row] : 0.0f;
  }
  for (int t = 0; t < T; ++t) {
    float (*buf)[HP] = hs[t & 1];
    float hin[4], gr[4], gz[4], gn[4], mn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      hin[i] = h[i] * m[i];
      buf[4 * q + i][u] = hin[i];
    }
    // this step's input gates and the next step's masks, asked for ahead of the product
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = t * N + row0 + 4 * q + i;
      gr[i] = ok[i] ? gi[(size_t)r * G + u] : 0.0f;
      gz[i] = ok[i] ? gi[(size_t)r * G + H + u] : 0.0f;
      gn[i] = ok[i] ? gi[(size_t)r * G + 2 * H + u] : 0.0f;
      mn[i] = (ok[i] && t + 1 < T) ? masks[r + N] : 0.0f;
    }
    __syncthreads();
    floatx4 ar = {0.0f, 0.0f, 0.0f, 0.0f}, az = ar, an = ar;
    const float* arow = &buf[n][32 * q];
#pragma unroll
    for (int s = 0; s < 32; s += 4) {
      const float4 a = *reinterpret_cast<const float4*>(arow + s);
      const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ar = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], B[0][s + j], ar, 0, 0, 0);
        az = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], B[1][s + j], az, 0, 0, 0);
        an = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], B[2][s + j], an, 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float r = sigm(gr[i] + (ar[i] + bh_r));
      const float z = sigm(gz[i] + (az[i] + bh_z));
      const float ghn = an[i] + bh_n;
      const float nn = tanhf(gn[i] + r * ghn);
      h[i] = (1.0f - z) * nn + z * hin[i];
      m[i] = mn[i];
      if (ok[i]) {
        const size_t o = (size_t)(t * N + row0 + 4 * q + i);
        y[o * H + u] = h[i];
        if (saved) {
          float* sv = saved + o * SAVED;
          sv[u] = r; sv[H + u] = z; sv[2 * H + u] = nn; sv[3 * H + u] = ghn;
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (ok[i]) h_T[(size_t)(row0 + 4 * q + i) * H + u] = h[i];
}

// Reverse-time loop: dh (fp32, registers) starts at dh_T (NULL: zero) and takes dy_t (NULL: zero) at every step; writes the gate
// gradients dGi = d(pre-activations) and dGh (the same but r * d(pre_n) in the n block), [T*N, 384] each, and dhxs = dh_in(0) * m_0
// (NULL: not wanted). h_in is rebuilt from y_{t-1} (hxs at t = 0) and m_t.
__global__ __launch_bounds__(512) void gru_seq_bwd(const float* __restrict__ dy, const float* __restrict__ dh_T, const float* __restrict__ saved,
                                                   const float* __restrict__ y, const float* __restrict__ hxs, const float* __restrict__ masks,
                                                   const float* __restrict__ whh, float* __restrict__ dgi, float* __restrict__ dgh,
                                                   float* __restrict__ dhxs, int N, int T) {
  __shared__ __attribute__((aligned(16))) float gs[2][RT][GP];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
  const int u = 16 * w + n;
  const int row0 = blockIdx.x * RT;
  // B operands: W_hh[gate row k = 96 q + s][unit 16 w + n]
  float B[96];
#pragma unroll
  for (int s = 0; s < 96; ++s) B[s] = whh[(size_t)(96 * q + s) * H + u];
  bool ok[4];
  float dh[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = row0 + 4 * q + i;
    ok[i] = row < N;
    dh[i] = (ok[i] && dh_T) ? dh_T[(size_t)row * H + u] : 0.0f;
  }
  for (int t = T - 1; t >= 0; --t) {
    float (*buf)[GP] = gs[t & 1];
    float direct[4], m[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float dr = 0.0f, dz = 0.0f, dn = 0.0f, dnh = 0.0f;
      direct[i] = 0.0f;
      m[i] = 0.0f;
      if (ok[i]) {
        const int row = row0 + 4 * q + i;
        const size_t o = (size_t)(t * N + row);
        if (dy) dh[i] += dy[o * H + u];
        const float* sv = saved + o * SAVED;
        const float r = sv[u], z = sv[H + u], nn = sv[2 * H + u], ghn = sv[3 * H + u];
        m[i] = masks[o];
        const float hprev = t > 0 ? y[(o - N) * H + u] : hxs[(size_t)row * H + u];
        const float hin = hprev * m[i];
        const float g = dh[i];
        dn = (g * (1.0f - z)) * (1.0f - nn * nn);
        dz = (g * (hin - nn)) * (z * (1.0f - z));
        dr = (dn * ghn) * (r * (1.0f - r));
        dnh = dn * r;
        direct[i] = g * z;
        float* a = dgi + o * G;
        a[u] = dr; a[H + u] = dz; a[2 * H + u] = dn;
        float* b = dgh + o * G;
        b[u] = dr; b[H + u] = dz; b[2 * H + u] = dnh;
      }
      buf[4 * q + i][u] = dr; buf[4 * q + i][H + u] = dz; buf[4 * q + i][2 * H + u] = dnh;
    }
    __syncthreads();
    // dh_in = dh * z + dGh W_hh, two accumulation chains (the dependent-accumulator latency is 40 cycles against a 32-cycle issue)
    floatx4 a0 = {0.0f, 0.0f, 0.0f, 0.0f}, a1 = a0;
    const float* arow = &buf[n][96 * q];
#pragma unroll
    for (int s = 0; s < 96; s += 4) {
      const float4 a = *reinterpret_cast<const float4*>(arow + s);
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, B[s], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, B[s + 1], a1, 0, 0, 0);
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, B[s + 2], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, B[s + 3], a1, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) dh[i] = (direct[i] + (a0[i] + a1[i])) * m[i];
  }
  if (dhxs) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (ok[i]) dhxs[(size_t)(row0 + 4 * q + i) * H + u] = dh[i];
  }
}
}  // namespace grut

// ------------------------------------------------------------------------------------------------ C ABI (include/aircombat.h)
extern "C" {
// slack: the rows past N * T that a kernel's tile may index before its bounds test (gru_layer_train.hpp walks 32-row tiles)
static int gru_shape_ok(const char* who, int32_t N, int32_t T, int slack = grut::RT) {
  if (N < 1 || T < 1) return fail(std::string(who) + ": N and T must be at least 1");
  if ((int64_t)N * T > (int64_t)INT32_MAX - slack) return fail(std::string(who) + ": N * T exceeds the kernels' 32-bit row index");
  return 0;
}
int ac_gru_seq_forward(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_gi, const float* d_hxs, const float* d_masks,
                       const float* d_w_hh, const float* d_b_hh, float* d_y, float* d_h_T, float* d_saved) {
  if (!d_gi || !d_hxs || !d_masks || !d_w_hh || !d_b_hh || !d_y || !d_h_T) return fail("ac_gru_seq_forward: null argument");
  if (gru_shape_ok("ac_gru_seq_forward", N, T)) return -1;
  HIP_OK(hipSetDevice(device_id));
  hipLaunchKernelGGL(grut::gru_seq_fwd, dim3(trn::tiles(N, grut::RT)), dim3(512), 0, (hipStream_t)stream, d_gi, d_hxs, d_masks,
                     d_w_hh, d_b_hh, d_y, d_h_T, d_saved, (int)N, (int)T);
  HIP_OK(hipGetLastError());
  return 0;
}
int ac_gru_seq_backward(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_dy, const float* d_dh_T, const float* d_saved,
                        const float* d_y, const float* d_hxs, const float* d_masks, const float* d_w_hh, float* d_dgi, float* d_dgh,
                        float* d_dhxs) {
  if (!d_saved || !d_y || !d_hxs || !d_masks || !d_w_hh || !d_dgi || !d_dgh) return fail("ac_gru_seq_backward: null argument");
  if (gru_shape_ok("ac_gru_seq_backward", N, T)) return -1;
  HIP_OK(hipSetDevice(device_id));
  hipLaunchKernelGGL(grut::gru_seq_bwd, dim3(trn::tiles(N, grut::RT)), dim3(512), 0, (hipStream_t)stream, d_dy, d_dh_T, d_saved, d_y,
                     d_hxs, d_masks, d_w_hh, d_dgi, d_dgh, d_dhxs, (int)N, (int)T);
  HIP_OK(hipGetLastError());
  return 0;
}
}  // extern "C"
