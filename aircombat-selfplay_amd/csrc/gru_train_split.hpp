// The recurrence kernels of gru_train.hpp with their hidden product on the bf16 matrix path ("The training GRU"): the
// opt-in form AC_PRODUCTS_BF16X3. Everything but the product is gru_seq_fwd / gru_seq_bwd as they are: the same arguments and T-major
// rows, the same saved values, the same (row, unit) ownership (wave w owns units 16 w .. 16 w + 15, lane (q, n) rows 4 q + i), h and
// the carried dh fp32 in that lane's registers, the same gate algebra, one workgroup of eight waves per 16 chunks, one barrier per step
// over double-buffered LDS.
//
// The product is bf16x3.hpp's. W_hh is the B operand, split at the start of every call (36 uint4 = 144 VGPRs in either direction). The
// A operand -- the masked state, or the hidden-side gate gradients -- is split by the lane that produces it and written to the planes
// [16][K + 8] (272 B and 784 B rows). The forward keeps one chain per gate; the backward's dh runs on three chains (chains_pairs).
#pragma once

namespace grus {
using grut::floatx4; using grut::H; using grut::G; using grut::RT; using grut::SAVED; using grut::sigm;
constexpr int KSF = H + 8;   // bf16 per plane row, forward (= ctls::KS)
constexpr int KSB = G + 8;   // backward

__global__ __launch_bounds__(512) void gru_seq_fwd_b3(const float* __restrict__ gi, const float* __restrict__ hxs, const float* __restrict__ masks,
                                                      const float* __restrict__ whh, const float* __restrict__ bhh, float* __restrict__ y,
                                                      float* __restrict__ h_T, float* __restrict__ saved, int N, int T) {
  __shared__ __attribute__((aligned(16))) unsigned short hs[2][3][RT][KSF];
  constexpr int PLN = RT * KSF;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
  const int u = 16 * w + n;
  const int row0 = blockIdx.x * RT;
  // B operands: W_hh[gate row g * 128 + u][k = 32 s + 8 q + j], the pieces of k-step s
  uint4 B[3][4][3];
#pragma unroll
  for (int g = 0; g < 3; ++g) b3::row_slice<4>(B[g], whh + (size_t)(g * H + u) * H, q);
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
    unsigned short* buf = &hs[t & 1][0][0][0];
    float hin[4], gr[4], gz[4], gn[4], mn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) hin[i] = h[i] * m[i];
    b3::write_column(buf + (4 * q) * KSF + u, PLN, KSF, hin);
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
    const unsigned short* arow = buf + n * KSF + 8 * q;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      uint4 A[3];
      b3::read3(A, arow + 32 * s, PLN);
      b3::one_chain([&](int i, int j) {
        ar = b3::mf(A[i], B[0][s][j], ar);
        az = b3::mf(A[i], B[1][s][j], az);
        an = b3::mf(A[i], B[2][s][j], an);
      });
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

__global__ __launch_bounds__(512) void gru_seq_bwd_b3(const float* __restrict__ dy, const float* __restrict__ dh_T, const float* __restrict__ saved,
                                                      const float* __restrict__ y, const float* __restrict__ hxs, const float* __restrict__ masks,
                                                      const float* __restrict__ whh, float* __restrict__ dgi, float* __restrict__ dgh,
                                                      float* __restrict__ dhxs, int N, int T) {
  __shared__ __attribute__((aligned(16))) unsigned short gs[2][3][RT][KSB];
  constexpr int PLN = RT * KSB;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
  const int u = 16 * w + n;
  const int row0 = blockIdx.x * RT;
  // B operands: W_hh[gate row k = 32 s + 8 q + j][unit 16 w + n], the pieces of k-step s
  uint4 B[12][3];
  b3::col_slice<12>(B, whh, H, u, q);
  bool ok[4];
  float dh[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = row0 + 4 * q + i;
    ok[i] = row < N;
    dh[i] = (ok[i] && dh_T) ? dh_T[(size_t)row * H + u] : 0.0f;
  }
  for (int t = T - 1; t >= 0; --t) {
    unsigned short* buf = &gs[t & 1][0][0][0];
    float direct[4], m[4], vr[4], vz[4], vn[4];
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
      vr[i] = dr; vz[i] = dz; vn[i] = dnh;
    }
    unsigned short* col = buf + (4 * q) * KSB + u;
    b3::write_column(col, PLN, KSB, vr);
    b3::write_column(col + H, PLN, KSB, vz);
    b3::write_column(col + 2 * H, PLN, KSB, vn);
    __syncthreads();
    // dh_in = dh * z + dGh W_hh on three accumulation chains
    floatx4 c[3] = {};
    const unsigned short* arow = buf + n * KSB + 8 * q;
#pragma unroll
    for (int s = 0; s < 12; ++s) {
      uint4 A[3];
      b3::read3(A, arow + 32 * s, PLN);
      b3::chains_pairs(c, A, B[s]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) dh[i] = (direct[i] + b3::chain_sum(c, i)) * m[i];
  }
  if (dhxs) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (ok[i]) dhxs[(size_t)(row0 + 4 * q + i) * H + u] = dh[i];
  }
}
}  // namespace grus

// ------------------------------------------------------------------------------------------------ C ABI (include/aircombat.h)
extern "C" {
int ac_gru_seq_forward_p(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_gi, const float* d_hxs, const float* d_masks,
                         const float* d_w_hh, const float* d_b_hh, float* d_y, float* d_h_T, float* d_saved, int32_t products) {
  if (!d_gi || !d_hxs || !d_masks || !d_w_hh || !d_b_hh || !d_y || !d_h_T) return fail("ac_gru_seq_forward_p: null argument");
  if (gru_shape_ok("ac_gru_seq_forward_p", N, T) || trn::products_ok("ac_gru_seq_forward_p", "products", products)) return -1;
  if (products == AC_PRODUCTS_FP32) return ac_gru_seq_forward(device_id, stream, N, T, d_gi, d_hxs, d_masks, d_w_hh, d_b_hh, d_y, d_h_T, d_saved);
  HIP_OK(hipSetDevice(device_id));
  hipLaunchKernelGGL(grus::gru_seq_fwd_b3, dim3(trn::tiles(N, grut::RT)), dim3(512), 0, (hipStream_t)stream, d_gi, d_hxs, d_masks,
                     d_w_hh, d_b_hh, d_y, d_h_T, d_saved, (int)N, (int)T);
  HIP_OK(hipGetLastError());
  return 0;
}
int ac_gru_seq_backward_p(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_dy, const float* d_dh_T, const float* d_saved,
                          const float* d_y, const float* d_hxs, const float* d_masks, const float* d_w_hh, float* d_dgi, float* d_dgh,
                          float* d_dhxs, int32_t products) {
  if (!d_saved || !d_y || !d_hxs || !d_masks || !d_w_hh || !d_dgi || !d_dgh) return fail("ac_gru_seq_backward_p: null argument");
  if (gru_shape_ok("ac_gru_seq_backward_p", N, T) || trn::products_ok("ac_gru_seq_backward_p", "products", products)) return -1;
  if (products == AC_PRODUCTS_FP32)
    return ac_gru_seq_backward(device_id, stream, N, T, d_dy, d_dh_T, d_saved, d_y, d_hxs, d_masks, d_w_hh, d_dgi, d_dgh, d_dhxs);
  HIP_OK(hipSetDevice(device_id));
  hipLaunchKernelGGL(grus::gru_seq_bwd_b3, dim3(trn::tiles(N, grut::RT)), dim3(512), 0, (hipStream_t)stream, d_dy, d_dh_T, d_saved, d_y,
                     d_hxs, d_masks, d_w_hh, d_dgi, d_dgh, d_dhxs, (int)N, (int)T);
  HIP_OK(hipGetLastError());
  return 0;
}
}  // extern "C"
