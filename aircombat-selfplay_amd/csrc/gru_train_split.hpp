// The recurrence kernels of gru_train.hpp with their hidden product on the bf16 matrix path ("The training GRU"): the
// opt-in form AC_PRODUCTS_BF16X3. Everything but the product is gru_seq_fwd / gru_seq_bwd as they are: the same arguments and T-major
// rows, the same saved values, the same (row, unit) ownership (wave w owns units 16 w .. 16 w + 15, lane (q, n) rows 4 q + i), h and
// the carried dh fp32 in that lane's registers, the same gate algebra, one workgroup of eight waves per 16 chunks, one barrier per step
// over double-buffered LDS.
//
// The product: every fp32 value is split into three bf16 pieces, x = b0 + b1 + b2 exactly (ctls::split3_pair, controller_pieces.hpp),
// and a product keeps the six terms b_i b_j with i + j <= 2, each an exact bf16 x bf16 product accumulated in fp32 by
// v_mfma_f32_16x16x32_bf16: good to about 2^-23 of itself, 24 instructions of 16 cycles per 128 k of a tile where the fp32 instruction
// takes 32 of 32 cycles. W_hh is read from the caller's fp32 tensor at the start of every call and split in registers (B operand: lane
// l holds k = 8 (l / 16) + j, j = 0 .. 7, of column l % 16; 36 uint4 = 144 VGPRs in either direction); nothing is kept between calls.
// The A operand -- the masked state, or the hidden-side gate gradients -- is split by the lane that produces it and written to three
// bf16 planes [16][K + 8] in LDS (row strides 272 B and 784 B: 4 banks mod 64, so the 16 rows of a lane quarter read distinct banks),
// and read back as one ds_read_b128 per piece and k-step (lane l: row l % 16, k = 8 (l / 16) + j). A masked row is +-0 and splits to
// three zero pieces. Within a k-step the terms run in the controller's order, smallest first (mfma_layers.hpp, gru_step).
#pragma once

namespace grus {
using grut::floatx4; using grut::H; using grut::G; using grut::RT; using grut::SAVED; using grut::sigm;
constexpr int KSF = H + 8;   // bf16 per plane row, forward (= ctls::KS)
constexpr int KSB = G + 8;   // backward

__device__ __forceinline__ floatx4 mf(const uint4& a, const uint4& b, floatx4 acc) { return ctl8::mf<3>(a, b, acc); }
// eight consecutive k of a weight row or column -> one B operand per piece
__device__ __forceinline__ void split8(const float (&v)[8], uint4& p0, uint4& p1, uint4& p2) {
  unsigned a[4], b[4], c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) ctls::split3_pair(v[2 * j], v[2 * j + 1], a[j], b[j], c[j]);
  p0 = make_uint4(a[0], a[1], a[2], a[3]); p1 = make_uint4(b[0], b[1], b[2], b[3]); p2 = make_uint4(c[0], c[1], c[2], c[3]);
}
// this lane's four rows of one column -> the three planes (plane stride `pln`, row stride `ks`, in bf16)
__device__ __forceinline__ void write_column(unsigned short* at, int pln, int ks, const float (&v)[4]) {
  unsigned lo[3], hi[3];
  ctls::split3_pair(v[0], v[1], lo[0], lo[1], lo[2]);
  ctls::split3_pair(v[2], v[3], hi[0], hi[1], hi[2]);
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    unsigned short* c = at + p * pln;
    c[0] = (unsigned short)lo[p]; c[ks] = (unsigned short)(lo[p] >> 16);
    c[2 * ks] = (unsigned short)hi[p]; c[3 * ks] = (unsigned short)(hi[p] >> 16);
  }
}

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
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float* p = whh + (size_t)(g * H + u) * H + 32 * s + 8 * q;
      const float4 v0 = *reinterpret_cast<const float4*>(p), v1 = *reinterpret_cast<const float4*>(p + 4);
      const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
      split8(v, B[g][s][0], B[g][s][1], B[g][s][2]);
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
    unsigned short* buf = &hs[t & 1][0][0][0];
    float hin[4], gr[4], gz[4], gn[4], mn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) hin[i] = h[i] * m[i];
    write_column(buf + (4 * q) * KSF + u, PLN, KSF, hin);
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
#pragma unroll
      for (int p = 0; p < 3; ++p) A[p] = *reinterpret_cast<const uint4*>(arow + p * PLN + 32 * s);
      constexpr int TI[6] = {2, 1, 0, 1, 0, 0}, TJ[6] = {0, 1, 2, 0, 1, 0};
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        ar = mf(A[TI[k]], B[0][s][TJ[k]], ar);
        az = mf(A[TI[k]], B[1][s][TJ[k]], az);
        an = mf(A[TI[k]], B[2][s][TJ[k]], an);
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
#pragma unroll
  for (int s = 0; s < 12; ++s) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = whh[(size_t)(32 * s + 8 * q + j) * H + u];
    split8(v, B[s][0], B[s][1], B[s][2]);
  }
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
    write_column(col, PLN, KSB, vr);
    write_column(col + H, PLN, KSB, vz);
    write_column(col + 2 * H, PLN, KSB, vn);
    __syncthreads();
    // dh_in = dh * z + dGh W_hh on three accumulation chains, two terms of every k-step each: the second-order terms lead, the
    // first-order ones and the leading one follow, and the chains are added smallest first
    floatx4 c0 = {0.0f, 0.0f, 0.0f, 0.0f}, c1 = c0, c2 = c0;
    const unsigned short* arow = buf + n * KSB + 8 * q;
#pragma unroll
    for (int s = 0; s < 12; ++s) {
      uint4 A[3];
#pragma unroll
      for (int p = 0; p < 3; ++p) A[p] = *reinterpret_cast<const uint4*>(arow + p * PLN + 32 * s);
      c0 = mf(A[2], B[s][0], c0);
      c1 = mf(A[1], B[s][1], c1);
      c2 = mf(A[0], B[s][2], c2);
      c0 = mf(A[1], B[s][0], c0);
      c1 = mf(A[0], B[s][1], c1);
      c2 = mf(A[0], B[s][0], c2);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) dh[i] = (direct[i] + ((c0[i] + c1[i]) + c2[i])) * m[i];
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
static int gru_products_ok(const char* who, int32_t products) {
  if (products != AC_PRODUCTS_FP32 && products != AC_PRODUCTS_BF16X3)
    return fail(std::string(who) + ": unknown products " + std::to_string(products) + " (AC_PRODUCTS_FP32 or AC_PRODUCTS_BF16X3)");
  return 0;
}
int ac_gru_seq_forward_p(int32_t device_id, void* stream, int32_t N, int32_t T, const float* d_gi, const float* d_hxs, const float* d_masks,
                         const float* d_w_hh, const float* d_b_hh, float* d_y, float* d_h_T, float* d_saved, int32_t products) {
  if (!d_gi || !d_hxs || !d_masks || !d_w_hh || !d_b_hh || !d_y || !d_h_T) return fail("ac_gru_seq_forward_p: null argument");
  if (gru_shape_ok("ac_gru_seq_forward_p", N, T) || gru_products_ok("ac_gru_seq_forward_p", products)) return -1;
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
  if (gru_shape_ok("ac_gru_seq_backward_p", N, T) || gru_products_ok("ac_gru_seq_backward_p", products)) return -1;
  if (products == AC_PRODUCTS_FP32)
    return ac_gru_seq_backward(device_id, stream, N, T, d_dy, d_dh_T, d_saved, d_y, d_hxs, d_masks, d_w_hh, d_dgi, d_dgh, d_dhxs);
  HIP_OK(hipSetDevice(device_id));
  hipLaunchKernelGGL(grus::gru_seq_bwd_b3, dim3(trn::tiles(N, grut::RT)), dim3(512), 0, (hipStream_t)stream, d_dy, d_dh_T, d_saved, d_y,
                     d_hxs, d_masks, d_w_hh, d_dgi, d_dgh, d_dhxs, (int)N, (int)T);
  HIP_OK(hipGetLastError());
  return 0;
}
}  // extern "C"
