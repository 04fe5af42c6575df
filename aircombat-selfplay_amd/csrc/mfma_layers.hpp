// The matrix-core layer pieces both 128-wide recurrent networks on the device share -- the low-level controller (controller8_kernel.hpp)
// and the PPO rollout policy (policy_kernel.hpp): weight-tile layout helpers, A / B operand loads, the piece products of one k-step
// (controller_pieces.hpp), a K = 128 layer, the GRU's k-steps, the LayerNorm epilogue into piece planes. Eight waves per workgroup, wave w
// owning 16 output columns of a layer; 16-row M-tiles, MTL of them per wave. Included by controller8_kernel.hpp.
#pragma once

namespace ctl8 {
using ctl::HID; using ctl::NH; using ctl::NHP; using ctl::MT; using ctl::LS;
using ctls::KS; using ctls::RS;
typedef float floatx4 __attribute__((ext_vector_type(4)));
// NP = pieces per value: 2 fp16 pieces (the fast form, AC_CTL_FAST) or 3 bf16 pieces (the reference-precision form, AC_CTL_FP32);
// every helper below and the kernel body are templates on it, the fast form's code is what it was before the second form existed
template <int NP>
struct Lay {
  static constexpr int tile_floats(int K) { return (K / 32) * NP * 64 * 4; }   // in floats (a uint4 = 8 16-bit pieces = 4 floats)
  enum : int {
    C_W1 = 0,                                  // K = 32 (12 padded), 8 tiles
    C_W2 = C_W1 + 8 * tile_floats(32),         // K = 128, 8 tiles
    C_WIH = C_W2 + 8 * tile_floats(128),       // 24 tiles: gate g (r, z, n), unit tile u -> tile 8 g + u
    C_WHH = C_WIH + 24 * tile_floats(128),     // 24 tiles
    C_WA = C_WHH + 24 * tile_floats(128),      // 10 tiles (columns 153..159 zero)
    C_B1 = C_WA + 10 * tile_floats(128), C_G1 = C_B1 + 128, C_BE1 = C_G1 + 128,
    C_B2 = C_BE1 + 128, C_G2 = C_B2 + 128, C_BE2 = C_G2 + 128,
    C_BIH = C_BE2 + 128, C_BHH = C_BIH + 384, C_G3 = C_BHH + 384, C_BE3 = C_G3 + 128,
    C_BA = C_BE3 + 128,                        // [160]
    C_END = C_BA + NHP
  };
};
__device__ __forceinline__ floatx4 splat4(float v) { floatx4 a = {v, v, v, v}; return a; }
template <int NP>
__device__ __forceinline__ floatx4 mf(const uint4& a, const uint4& b, floatx4 acc) {
  if constexpr (NP == 2)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(ctls::f16x8, a), __builtin_bit_cast(ctls::f16x8, b), acc, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(ctls::bf16x8, a), __builtin_bit_cast(ctls::bf16x8, b), acc, 0, 0, 0);
}
// result layout of a 16x16 tile: acc[i] is (row = 4 (lane / 16) + i, column = lane % 16)
__device__ __forceinline__ int c_row(int mt, int i, int lane) { return 16 * mt + 4 * (lane >> 4) + i; }

// A operands of one k-step for this lane: [M-tile][piece] = planes[piece][row = 16 mt + lane % 16][k = 32 s + 8 (lane / 16) .. + 7].
// MTL = M-tiles per wave: 2 (32 aircraft per workgroup) or 4 (64: the grids with more tiles than CUs, where a workgroup's fixed costs --
// first round trip, barriers, the latency-bound LayerNorm / gate / argmax phases -- are shared by twice the aircraft and every weight
// piece loaded feeds twice the matrix instructions).
template <int MTL>
struct Geo8 {
  static constexpr int R = 16 * MTL;               // aircraft per workgroup
  static constexpr int PLN = R * KS;               // fp16 per plane
  static constexpr int LSR = R + 1;                // row stride of the [feature][aircraft] buffers (odd: column writes spread over the banks)
  static constexpr int TPR = 512 / R;              // threads per aircraft in the row-wise phases (16 or 8)
  static constexpr int FPT = HID / TPR;            // features per thread there (8 or 16)
};
template <int MTL, int NP>
struct AF { uint4 a[MTL][NP]; };
template <int MTL, int NP>
__device__ __forceinline__ void load_af(const unsigned short* planes, int lane, int s, AF<MTL, NP>& A) {
  const unsigned short* base = planes + (lane & 15) * KS + 8 * (lane >> 4) + 32 * s;
#pragma unroll
  for (int mt = 0; mt < MTL; ++mt)
#pragma unroll
    for (int p = 0; p < NP; ++p) A.a[mt][p] = *reinterpret_cast<const uint4*>(base + p * Geo8<MTL>::PLN + 16 * mt * KS);
}
template <int NP>
struct BS { uint4 b[NP]; };   // one k-step of one 16-column tile: the pieces
template <int NP>
__device__ __forceinline__ void load_bs(const uint4* __restrict__ t4 /* tile + lane */, int s, BS<NP>& B) {
#pragma unroll
  for (int p = 0; p < NP; ++p) B.b[p] = t4[(s * NP + p) * 64];
}
template <int K, int NP>
struct BT { BS<NP> s[K / 32]; };
template <int K, int NP>
__device__ __forceinline__ void prefetch_bt(const float* __restrict__ tile, int lane, BT<K, NP>& B) {
  const uint4* t4 = reinterpret_cast<const uint4*>(tile) + lane;
#pragma unroll
  for (int s = 0; s < K / 32; ++s) load_bs<NP>(t4, s, B.s[s]);
}
// one k-step of one tile on two accumulation chains per M-tile: the leading term, and the others smallest first (two fp16 pieces: the two
// cross terms, 2^-11 of the product; three bf16 pieces: the three second-order terms, 2^-16, then the two first-order ones, 2^-8)
template <int MTL, int NP>
__device__ __forceinline__ void step2(floatx4 (&lo)[MTL], floatx4 (&acc)[MTL], const AF<MTL, NP>& A, const BS<NP>& B) {
  if constexpr (NP == 2) {
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) lo[mt] = mf<NP>(A.a[mt][1], B.b[0], lo[mt]);
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) acc[mt] = mf<NP>(A.a[mt][0], B.b[0], acc[mt]);
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) lo[mt] = mf<NP>(A.a[mt][0], B.b[1], lo[mt]);
  } else {
    constexpr int TI[5] = {2, 1, 0, 1, 0}, TJ[5] = {0, 1, 2, 0, 1};
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) lo[mt] = mf<NP>(A.a[mt][TI[0]], B.b[TJ[0]], lo[mt]);
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) acc[mt] = mf<NP>(A.a[mt][0], B.b[0], acc[mt]);
#pragma unroll
    for (int t = 1; t < 5; ++t)
#pragma unroll
      for (int mt = 0; mt < MTL; ++mt) lo[mt] = mf<NP>(A.a[mt][TI[t]], B.b[TJ[t]], lo[mt]);
  }
}
// a whole K = 128 layer for this wave's 16 columns: the weight tile is in registers (asked for a phase earlier), the A operands come
// from the planes one k-step ahead of their use (MTL = 2) or as they are needed (MTL = 4: registers)
template <int MTL, int NP>
__device__ __forceinline__ void layer128(const BT<HID, NP>& B, const unsigned short* planes, int lane, floatx4 (&acc)[MTL]) {
  floatx4 lo[MTL];
#pragma unroll
  for (int mt = 0; mt < MTL; ++mt) lo[mt] = splat4(0.0f);
  constexpr int NB = MTL == 2 ? 2 : 1;
  AF<MTL, NP> A[NB];
  load_af<MTL, NP>(planes, lane, 0, A[0]);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (NB == 2 && s + 1 < 4) load_af<MTL, NP>(planes, lane, s + 1, A[(s + 1) % NB]);
    __builtin_amdgcn_sched_barrier(0);
    step2<MTL, NP>(lo, acc, A[s % NB], B.s[s]);
    __builtin_amdgcn_sched_barrier(0);
    if (NB == 1 && s + 1 < 4) load_af<MTL, NP>(planes, lane, s + 1, A[0]);
  }
#pragma unroll
  for (int mt = 0; mt < MTL; ++mt)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[mt][i] += lo[mt][i];
}
// the GRU's k-steps: three gate tiles of this wave's 16 hidden units; one term of the products, all gates and M-tiles
template <int MTL, int NP>
__device__ __forceinline__ void gru_term(floatx4 (&a0)[MTL], floatx4 (&a1)[MTL], floatx4 (&a2)[MTL], const AF<MTL, NP>& A, int pa, const BS<NP> (&B)[3], int pb) {
#pragma unroll
  for (int mt = 0; mt < MTL; ++mt) {
    a0[mt] = mf<NP>(A.a[mt][pa], B[0].b[pb], a0[mt]); a1[mt] = mf<NP>(A.a[mt][pa], B[1].b[pb], a1[mt]); a2[mt] = mf<NP>(A.a[mt][pa], B[2].b[pb], a2[mt]);
  }
}
// the kept terms (three, or six) smallest first into one accumulator per (gate, M-tile)
template <int MTL, int NP>
__device__ __forceinline__ void gru_step(floatx4 (&a0)[MTL], floatx4 (&a1)[MTL], floatx4 (&a2)[MTL], const AF<MTL, NP>& A, const BS<NP> (&B)[3]) {
  if constexpr (NP == 2) {
    gru_term<MTL, NP>(a0, a1, a2, A, 1, B, 0); gru_term<MTL, NP>(a0, a1, a2, A, 0, B, 1); gru_term<MTL, NP>(a0, a1, a2, A, 0, B, 0);
  } else {
    gru_term<MTL, NP>(a0, a1, a2, A, 2, B, 0); gru_term<MTL, NP>(a0, a1, a2, A, 1, B, 1); gru_term<MTL, NP>(a0, a1, a2, A, 0, B, 2);
    gru_term<MTL, NP>(a0, a1, a2, A, 1, B, 0); gru_term<MTL, NP>(a0, a1, a2, A, 0, B, 1); gru_term<MTL, NP>(a0, a1, a2, A, 0, B, 0);
  }
}
template <int NP>
__device__ __forceinline__ void ring_load(const float* __restrict__ W, int w, int lane, int st, BS<NP> (&dst)[3]) {
  using L = Lay<NP>;
  const int TF = L::tile_floats(HID);
  const float* base = W + (st < 4 ? L::C_WIH : L::C_WHH);
#pragma unroll
  for (int g = 0; g < 3; ++g) load_bs<NP>(reinterpret_cast<const uint4*>(base + (8 * g + w) * TF) + lane, st & 3, dst[g]);
}
// eight consecutive features of one aircraft -> the NP planes (one 16-byte LDS store per plane)
template <int MTL, int NP>
__device__ __forceinline__ void write_planes8(unsigned short* planes, int row, int k0, const float* v) {
  if constexpr (NP == 2) {
    unsigned h[4], l[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) ctls::split2_pair(v[2 * q], v[2 * q + 1], h[q], l[q]);
    *reinterpret_cast<uint4*>(planes + 0 * Geo8<MTL>::PLN + row * KS + k0) = make_uint4(h[0], h[1], h[2], h[3]);
    *reinterpret_cast<uint4*>(planes + 1 * Geo8<MTL>::PLN + row * KS + k0) = make_uint4(l[0], l[1], l[2], l[3]);
  } else {
    unsigned p0[4], p1[4], p2[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) ctls::split3_pair(v[2 * q], v[2 * q + 1], p0[q], p1[q], p2[q]);
    *reinterpret_cast<uint4*>(planes + 0 * Geo8<MTL>::PLN + row * KS + k0) = make_uint4(p0[0], p0[1], p0[2], p0[3]);
    *reinterpret_cast<uint4*>(planes + 1 * Geo8<MTL>::PLN + row * KS + k0) = make_uint4(p1[0], p1[1], p1[2], p1[3]);
    *reinterpret_cast<uint4*>(planes + 2 * Geo8<MTL>::PLN + row * KS + k0) = make_uint4(p2[0], p2[1], p2[2], p2[3]);
  }
}
// Sum over the adjacent lanes of an aircraft (16 or 8), the same value in all of them, with data-parallel-primitive moves (a few cycles
// each; __shfl_xor compiles to ds_bpermute_b32, an LDS round trip of ~100 cycles, eight of them in a dependent chain per LayerNorm): pairs
// and quads by quad_perm, the two quads of a half row by row_half_mirror (lane i <-> 7 - i), the two halves by row_mirror (i <-> 15 - i).
// Every lane adds its own and its partner's partial sum, which are the same two numbers on both sides: all lanes end bit-identical.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int LANES>
__device__ __forceinline__ float group_sum(float v) {
  v += dpp_f<0xB1>(v);    // quad_perm [1, 0, 3, 2]
  v += dpp_f<0x4E>(v);    // quad_perm [2, 3, 0, 1]
  v += dpp_f<0x141>(v);   // row_half_mirror
  if (LANES == 16) v += dpp_f<0x140>(v);   // row_mirror
  return v;
}
// torch.nn.LayerNorm(128) (eps 1e-5, biased variance) of buf[row][k] (fp32, row stride RS) into the piece planes the next layer's
// A operands are read from. Thread = (aircraft = tid / TPR, part = tid % TPR) owns FPT consecutive features; the parts of an aircraft sit
// in adjacent lanes: mean and variance are a few DPP steps each, no partial sums through LDS. Scale / shift come from LDS (staged).
template <int MTL, int NP>
__device__ __forceinline__ void layer_norm_planes(const float* buf, unsigned short* planes, const float* g, const float* b, int tid) {
  constexpr int TPR = Geo8<MTL>::TPR, FPT = Geo8<MTL>::FPT;
  const int row = tid / TPR, part = tid % TPR;
  float x[FPT], gg[FPT], bb[FPT];
#pragma unroll
  for (int q = 0; q < FPT / 4; ++q) {
    const float4 xv = *reinterpret_cast<const float4*>(buf + row * RS + FPT * part + 4 * q);
    const float4 gv = *reinterpret_cast<const float4*>(g + FPT * part + 4 * q), bv = *reinterpret_cast<const float4*>(b + FPT * part + 4 * q);
    x[4 * q] = xv.x; x[4 * q + 1] = xv.y; x[4 * q + 2] = xv.z; x[4 * q + 3] = xv.w;
    gg[4 * q] = gv.x; gg[4 * q + 1] = gv.y; gg[4 * q + 2] = gv.z; gg[4 * q + 3] = gv.w;
    bb[4 * q] = bv.x; bb[4 * q + 1] = bv.y; bb[4 * q + 2] = bv.z; bb[4 * q + 3] = bv.w;
  }
  float sum = 0.0f;
#pragma unroll
  for (int q = 0; q < FPT / 8; ++q) sum += ((x[8 * q] + x[8 * q + 1]) + (x[8 * q + 2] + x[8 * q + 3])) + ((x[8 * q + 4] + x[8 * q + 5]) + (x[8 * q + 6] + x[8 * q + 7]));
  const float m = group_sum<TPR>(sum) * (1.0f / HID);
  float v = 0.0f;
#pragma unroll
  for (int q = 0; q < FPT; ++q) { x[q] -= m; v = fmaf(x[q], x[q], v); }
  const float is = rsqrtf(group_sum<TPR>(v) * (1.0f / HID) + 1e-5f);
  float y[FPT];
#pragma unroll
  for (int q = 0; q < FPT; ++q) y[q] = fmaf(x[q] * is, gg[q], bb[q]);
#pragma unroll
  for (int q = 0; q < FPT / 8; ++q) write_planes8<MTL, NP>(planes, row, FPT * part + 8 * q, y + 8 * q);
  __syncthreads();
}
// the fp32 GRU state of (aircraft row, unit): two fp16 pieces do not add up to it exactly, so an fp32 copy [aircraft][k] (row stride RS)
// sits behind the two planes of the state buffer for the gate algebra. Three bf16 pieces do (controller_pieces.hpp), and the LDS the
// copy would take is what keeps two 32-aircraft workgroups per CU (and a 64-aircraft one at all): the value is their sum.
template <int MTL, int NP>
__device__ __forceinline__ float state_value(const unsigned short* planes, int row, int unit) {
  if constexpr (NP == 2) {
    return reinterpret_cast<const float*>(planes + 2 * Geo8<MTL>::PLN)[row * RS + unit];
  } else {
    const int o = row * KS + unit;
    return (ctls::bf16_bits_to_f32(planes[o]) + ctls::bf16_bits_to_f32(planes[Geo8<MTL>::PLN + o])) + ctls::bf16_bits_to_f32(planes[2 * Geo8<MTL>::PLN + o]);
  }
}
}  // namespace ctl8
