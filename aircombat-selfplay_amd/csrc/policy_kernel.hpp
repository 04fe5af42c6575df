// The PPO rollout policy on the device (PPOPolicy.get_actions / .act of algorithms/ppo/ppo_policy.py): the actor (ppo_actor.py) and the
// critic (ppo_critic.py) of the reference's recurrent MLP policy for n rows in one launch, with the action heads' sampling and log-probs.
// Included by aircombat.hip behind the controller kernels, whose layer pieces it uses (mfma_layers.hpp, controller_pieces.hpp).
//
// Network (hidden sizes "128 128", one GRU layer of 128, ReLU), per row:
//   actor:  [LayerNorm(obs)] -> 2 x (Linear -> ReLU -> LayerNorm) -> GRU(h * mask) -> LayerNorm -> 2 x (Linear -> ReLU -> LayerNorm)
//           -> heads: MultiDiscrete logits (<= 160 in all) [+ four BetaShootBernoulli munition heads, Linear(128, 2) each]
//   critic: the same trunk (its own weights) -> value_out Linear(128, 1)
// Launch: grid (ceil(n / 32), 1 or 2): blockIdx.y = 0 the actor, 1 the critic; a workgroup = 32 rows x eight waves, wave w owning output
// columns 16 w .. 16 w + 15 of every 128-wide layer (the controller's shape, MTL = 2). The GEMMs are the controller's piece products:
// NP = 2 fp16 pieces (AC_CTL_FAST) or 3 bf16 pieces (AC_CTL_FP32).
//
// Packed weights of one network (Lay below): 16-column tiles of every matrix in the controller's B-operand tiling (controller8_kernel.hpp),
// then the fp32 vectors. The head tiles hold the logits in columns 0 .. sum(nvec) - 1 and munition head m's two outputs in columns
// 160 + 2 m, 161 + 2 m (the critic: the value in column 0).
//
// Sampling: deterministic = the mode (first maximum like torch.argmax; p > 0.5 for a munition head). Otherwise inverse-CDF with one
// uniform per (seed, counter, row, head) from the keyed generator policy_uniform, also compiled for the host (ac_policy_draw_host): a
// categorical head takes the first index whose running sum of exp(logit - max) exceeds u * total, a munition head fires when u >= 1 - p.
//
// The MAPPO form (policy_wide_kernel; struct Wide below): the same network with inputs up to 640 wide for both networks and a critic
// on cent_obs (explicit rows, or each env's observation block); policy_values_kernel is the PPO form's critic-only launch.
#pragma once
#include "keyed_uniform.hpp"

namespace pol {
using ctl::HID;
using ctls::KS; using ctls::RS;
constexpr int MTL = 2, R = 32;                  // M-tiles per wave, rows per workgroup
constexpr int MAXOBS = 32, MAXLOGITS = 160, MAXCAT = 8, NSHOOT = 4;
constexpr int HT = 11, HCOLS = 16 * HT;          // head tiles: 160 logit columns + 8 munition columns, padded to 176
constexpr int LSR = R + 1;

template <int NP>
struct Lay {
  static constexpr int T32 = ctl8::Lay<NP>::tile_floats(32), T128 = ctl8::Lay<NP>::tile_floats(HID);
  enum : int {
    W1 = 0,                    // obs_dim (<= 32) -> 128: 8 tiles, K = 32
    W2 = W1 + 8 * T32,         // 8 tiles
    WIH = W2 + 8 * T128,       // 24 tiles (gate-major r, z, n like torch)
    WHH = WIH + 24 * T128,     // 24 tiles
    W3 = WHH + 24 * T128,      // the action (critic: value) MLP, 8 tiles each
    W4 = W3 + 8 * T128,
    WO = W4 + 8 * T128,        // HT tiles
    F0G = WO + HT * T128, F0B = F0G + MAXOBS,   // LayerNorm(obs) (use_feature_normalization)
    B1 = F0B + MAXOBS, G1 = B1 + 128, BE1 = G1 + 128,
    B2 = BE1 + 128, G2 = B2 + 128, BE2 = G2 + 128,
    BIH = BE2 + 128, BHH = BIH + 384, GN = BHH + 384, BEN = GN + 128,
    B3 = BEN + 128, G3 = B3 + 128, BE3 = G3 + 128,
    B4 = BE3 + 128, G4 = B4 + 128, BE4 = G4 + 128,
    BO = BE4 + 128,            // [HCOLS]
    END = BO + HCOLS
  };
};

struct Args {
  const float* W[2];           // packed actor / critic (Lay<NP>)
  const float* obs;            // rows of obs_dim floats (env row order, below)
  const float* h_in[2];        // [n][128] GRU states in, actor / critic (may equal h_out)
  float* h_out[2];
  const float* masks;          // [n]
  float* actions;              // env rows of act_stride floats: heads at 0 .. n_cat + n_shoot - 1
  float* logp;                 // [n]
  float* values;               // [n] (critic)
  int n, obs_dim, act_stride;
  // row r of the call is env row (r / na) * A + a0 + r % na of the obs / action buffers (the agent range [a0, a0 + na) of an [E, A, .]
  // layout; a plain [n, .] layout is na = A = 1, a0 = 0)
  int na, A, a0;
  int obs_compact;             // get_actions launches (not the pool's): 1 = obs is a compact [n][obs_dim] array (a rollout buffer slot) while the actions keep the env rows
  int n_cat, n_shoot, use_fn, deterministic;
  int cat_off[MAXCAT], cat_cnt[MAXCAT];
  unsigned long long seed, counter;
};
// The wide form (the MAPPO policy: policy_wide_kernel): any input width 1 .. MAXWIDE per network, layer 1 streamed through the
// activation planes in 128-column K-blocks. Its W1 tiles (K = kpad) and feature-norm vectors sit behind the fixed part (WideLay); the
// fixed part's K = 32 W1 tiles and F0G / F0B stay zero. The critic's row r reads cin + (r / cna) * cstride: explicit rows (cna = 1,
// cstride = cent_dim), or env e = r / na's whole observation block (cin = the obs buffer, cna = na, cstride = A * obs_dim).
constexpr int MAXWIDE = 640;
struct Wide {
  const float* cin;
  long long cstride;
  int cna;
  int dim[2], kpad[2];         // input width and its padding to a multiple of 32, actor / critic
  int net0;                    // 1: a critic-only launch (get_values; grid y = 1), else 0
};
template <int NP>
struct WideLay {
  __host__ __device__ static constexpr int F0G(int kpad) { return Lay<NP>::END + 8 * ctl8::Lay<NP>::tile_floats(kpad); }
  __host__ __device__ static constexpr int END(int kpad) { return F0G(kpad) + 2 * kpad; }
};

// (the keyed counter-based generator policy_uniform: keyed_uniform.hpp)
// Where each tensor of one network sits in its fp32 source blob (float offsets; -1 = absent), from the blob order of policy.py
struct PackMap {
  int obs_dim;
  int w1, w2, wih, whh, w3, w4;                // row-major [out][in] like torch
  int f0g, f0b, b1, g1, be1, b2, g2, be2, bih, bhh, gn, ben, b3, g3, be3, b4, g4, be4;
  int orow[HCOLS], obias[HCOLS];               // the head (value) columns: source offset of the weight row / bias of each
};
// float f (counted from the first tile) of a run of 16-column weight tiles with K = kpad, as its two 16-bit pieces: output column j of
// tile row source roff + j * K (rows of them), or orow[j] when roff < 0 (the heads)
template <int NP>
__host__ __device__ inline unsigned policy_tile_bits(const float* src, const int* orow, int roff, int K, int kpad, int rows, int f) {
  const int per_tile = (kpad / 32) * NP * 512;
  unsigned bits = 0;
  for (int h = 0; h < 2; ++h) {
    const int e = 2 * f + h;
    const int c = e / per_tile, r = e % per_tile;
    const int st = r / (NP * 512), r2 = r % (NP * 512), pp = r2 / 512, lane = (r2 % 512) / 8, i = r2 % 8;
    const int k = 32 * st + 8 * (lane / 16) + i, j = 16 * c + lane % 16;
    const int ro = roff >= 0 ? (j < rows ? roff + j * K : -1) : (j < HCOLS ? orow[j] : -1);
    const float v = (ro >= 0 && k < K) ? src[ro + k] : 0.0f;
    unsigned pc[3];
    if (NP == 2) ctls::split2(v, pc[0], pc[1]);
    else ctls::split3(v, pc[0], pc[1], pc[2]);
    bits |= (pc[pp] & 0xFFFFu) << (16 * h);
  }
  return bits;
}
// packed float f of one network (Lay<NP>) as its bit pattern: the same code packs on the host (ac_policy_load) and on the device
// (ac_policy_load_device), so that both give the same bytes
template <int NP>
__host__ __device__ inline unsigned policy_pack_one(const float* src, const PackMap& m, int f) {
  using L = Lay<NP>;
  if (f < L::F0G) {   // a weight tile: two 16-bit pieces per float
    int base, K, kpad, rows, roff;
    if (f < L::W2) { base = L::W1; K = m.obs_dim; kpad = 32; rows = 128; roff = m.w1; }
    else if (f < L::WIH) { base = L::W2; K = 128; kpad = 128; rows = 128; roff = m.w2; }
    else if (f < L::WHH) { base = L::WIH; K = 128; kpad = 128; rows = 384; roff = m.wih; }
    else if (f < L::W3) { base = L::WHH; K = 128; kpad = 128; rows = 384; roff = m.whh; }
    else if (f < L::W4) { base = L::W3; K = 128; kpad = 128; rows = 128; roff = m.w3; }
    else if (f < L::WO) { base = L::W4; K = 128; kpad = 128; rows = 128; roff = m.w4; }
    else { base = L::WO; K = 128; kpad = 128; rows = HCOLS; roff = -1; }
    return policy_tile_bits<NP>(src, m.orow, roff, K, kpad, rows, f - base);
  }
  int o = -1, idx = 0;
  const int vb[22] = {L::F0G, L::F0B, L::B1, L::G1, L::BE1, L::B2, L::G2, L::BE2, L::BIH, L::BHH, L::GN, L::BEN,
                      L::B3, L::G3, L::BE3, L::B4, L::G4, L::BE4, L::BO, L::END, L::END, L::END};
  const int vs[19] = {m.f0g, m.f0b, m.b1, m.g1, m.be1, m.b2, m.g2, m.be2, m.bih, m.bhh, m.gn, m.ben, m.b3, m.g3, m.be3, m.b4, m.g4, m.be4, -2};
  for (int q = 0; q < 19; ++q)
    if (f >= vb[q] && f < vb[q + 1]) { idx = f - vb[q]; o = vs[q] == -2 ? (idx < HCOLS ? m.obias[idx] : -1) : (vs[q] >= 0 ? vs[q] + idx : -1); break; }
  if (o >= 0 && (f >= L::F0G && f < L::B1) && idx >= m.obs_dim) o = -1;
  const float v = o >= 0 ? src[o] : 0.0f;
  unsigned b;
  memcpy(&b, &v, 4);
  return b;
}
// packed float f of one network of the wide form (WideLay<NP>, m.obs_dim = this network's input width), for both load paths alike
template <int NP>
__host__ __device__ inline unsigned policy_pack_wide(const float* src, const PackMap& m, int f) {
  using L = Lay<NP>;
  const int kpad = (m.obs_dim + 31) / 32 * 32;
  if (f < L::W2 || (f >= L::F0G && f < L::B1)) return 0u;   // the fixed part's K = 32 layer 1 and feature norm: unused
  if (f < L::END) return policy_pack_one<NP>(src, m, f);
  f -= L::END;
  const int T = ctl8::Lay<NP>::tile_floats(kpad);
  if (f < 8 * T) return policy_tile_bits<NP>(src, m.orow, m.w1, m.obs_dim, kpad, 128, f);
  f -= 8 * T;
  const int o = f < kpad ? m.f0g : m.f0b, idx = f % kpad;
  const float v = (o >= 0 && idx < m.obs_dim) ? src[o + idx] : 0.0f;
  unsigned b;
  memcpy(&b, &v, 4);
  return b;
}
// The pool form (policy_pool_kernel, policy_pool_wide_kernel; csrc/policy_pool.hpp): one workgroup per tile of the plan, a tile being
// 1 .. 32 call rows of one member. Call row order[p] for p in [p0, p1); every row keeps its own positions in the buffers (the row
// indirection), and its draws are keyed by its call row as in the plain call.
struct Pool {
  const float* W0;             // member m's packed actor at W0 + m * stride
  long long stride;
  const int4* tiles;           // {member, p0, p1, 0}
  const int* order;            // the call rows, stably sorted by member
  const int* ntiles;           // tiles in the plan: workgroups past it exit
  int xcd;                     // 1: the tiles dealt so that a member's tiles share blockIdx.x % 8 (one XCD's L2; speed only)
};
// the tile of workgroup b (nt = none): the plain order, or the tile list cut into eight contiguous runs, run x taken by the workgroups
// b = x (mod 8) in order
__device__ __forceinline__ int pool_tile(int b, int nt, int xcd) {
  if (!xcd) return b;
  const int x = b & 7, j = b >> 3, q = nt >> 3, r = nt & 7;
  return j < q + (x < r ? 1 : 0) ? x * q + min(x, r) + j : nt;
}
__device__ __forceinline__ float softplus_t(float x) { return x > 20.0f ? x : log1pf(__expf(x)); }   // torch.nn.Softplus (threshold 20)

template <int NP>
__device__ __forceinline__ void ring_load(const float* __restrict__ W, int w, int lane, int st, ctl8::BS<NP> (&dst)[3]) {
  using L = Lay<NP>;
  const float* base = W + (st < 4 ? L::WIH : L::WHH);
#pragma unroll
  for (int g = 0; g < 3; ++g) ctl8::load_bs<NP>(reinterpret_cast<const uint4*>(base + (8 * g + w) * L::T128) + lane, st & 3, dst[g]);
}
// bias + ReLU of a 128-wide layer's outputs into the fp32 staging rows
__device__ __forceinline__ void relu_out(float* stg, const ctl8::floatx4 (&acc)[MTL], int w, int lane) {
  const int col = lane & 15;
#pragma unroll
  for (int mt = 0; mt < MTL; ++mt)
#pragma unroll
    for (int i = 0; i < 4; ++i) stg[ctl8::c_row(mt, i, lane) * RS + w * 16 + col] = fmaxf(acc[mt][i], 0.0f);
}
}  // namespace pol

// The PPO form's kernel (policy_kernel, at the end) is kept as it was written: the same body routed through this template compiles to a
// different schedule (224 -> 222 VGPRs for NP = 3), and its figures and results are pinned. This template is the body of the new kernels:
// WIDE = the wide input layer and the critic input of pol::Wide (policy_wide_kernel), else the PPO form's K = 32 one; VALUES = the PPO
// form's critic-only launch (policy_values_kernel; the wide form's is wx.net0); POOL = the actor of the plan's tile's member for the rows
// px.order lists (policy_pool_kernel / policy_pool_wide_kernel; the other instances compile as without it). Past layer 1 it is
// policy_kernel's code.
template <int NP, bool WIDE, bool VALUES, bool POOL = false>
__device__ __forceinline__ void policy_body(const pol::Args& a, const pol::Wide& wx, const pol::Pool& px = pol::Pool{}) {
  using namespace ctl8;
  using namespace pol;
  using ctl::sigmoid_f; using ctl::tanh_f;
  using L = pol::Lay<NP>;
  using G = Geo8<MTL>;
  constexpr int PLN = G::PLN;
  // the GRU state as piece planes (+ its fp32 copy behind them with two pieces: they do not add up to it exactly); the logits later
  constexpr int PHN = NP == 2 ? 2 * PLN + 2 * R * RS : 3 * PLN;
  __shared__ __attribute__((aligned(16))) unsigned short PA[NP * PLN];   // activations as piece planes [piece][row][k]
  __shared__ __attribute__((aligned(16))) unsigned short PH[PHN];
  __shared__ __attribute__((aligned(16))) float stg[R * RS];             // a layer's fp32 outputs [row][k] on their way to LayerNorm
  __shared__ float ab0[R][2];                                            // alpha0 / beta0 of the shoot prior
  __shared__ float lpart[R][MAXCAT + NSHOOT];                            // per-head log-probs
  static_assert(sizeof(unsigned short) * PHN >= sizeof(float) * HCOLS * LSR, "the logits reuse the GRU-state planes");
  float* lg = reinterpret_cast<float*>(PH);

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int net = POOL ? 0 : (WIDE ? blockIdx.y + wx.net0 : (VALUES ? 1 : blockIdx.y));   // 0 actor, 1 critic
  const int i0 = blockIdx.x * R;
  int4 tl = make_int4(0, 0, 0, 0);   // the pool form's tile: {member, p0, p1}
  if constexpr (POOL) {
    const int nt = *px.ntiles;
    const int t = pol::pool_tile(blockIdx.x, nt, px.xcd);
    if (t >= nt) return;
    tl = px.tiles[t];
  }
  const float* __restrict__ W = POOL ? px.W0 + tl.x * px.stride : a.W[net];
  const int col = lane & 15;
  const int srow = tid % R, spart = tid / R;   // staging: thread = (row, 8-feature part)
  // (a padding slot of a pool tile reads the member's last row)
  const int sn = POOL ? px.order[min(tl.y + srow, tl.z - 1)] : min(i0 + srow, a.n - 1);
  const long long senv = (long long)(sn / a.na) * a.A + a.a0 + sn % a.na;

  // ---- stage: the observation (LayerNorm'd when use_feature_normalization), the masked GRU state, the shoot prior
  BT<32, NP> b1;
  if constexpr (!WIDE) prefetch_bt<32, NP>(W + L::W1 + w * L::T32, lane, b1);
  BT<HID, NP> bt;
  if constexpr (!WIDE) prefetch_bt<HID, NP>(W + L::W2 + w * L::T128, lane, bt);
  const float mk = a.masks[sn];
  float hv[8];
  {
    const float4* hp = reinterpret_cast<const float4*>(a.h_in[net] + (size_t)sn * HID + 8 * spart);
    const float4 h0 = hp[0], h1 = hp[1];
    hv[0] = h0.x * mk; hv[1] = h0.y * mk; hv[2] = h0.z * mk; hv[3] = h0.w * mk;
    hv[4] = h1.x * mk; hv[5] = h1.y * mk; hv[6] = h1.z * mk; hv[7] = h1.w * mk;
  }
  if constexpr (!WIDE) {
    if (spart == 0) {
      const float* ob = a.obs + senv * a.obs_dim;
      float x[MAXOBS];
#pragma unroll
      for (int k = 0; k < MAXOBS; ++k) x[k] = k < a.obs_dim ? ob[k] : 0.0f;
      if (net == 0 && a.n_shoot) {   // ppo_actor.py: alpha0 3 / 6 (<= 12 km) / 10 (<= 8 km), beta0 10 / 6 (<= 45 deg) / 3 (<= 22.5 deg)
        const float ang = x[11] * 57.29577951308232f, dist = x[13] * 10000.0f;
        ab0[srow][0] = dist <= 8000.0f ? 10.0f : (dist <= 12000.0f ? 6.0f : 3.0f);
        ab0[srow][1] = ang <= 22.5f ? 3.0f : (ang <= 45.0f ? 6.0f : 10.0f);
      }
      if (a.use_fn) {   // torch.nn.LayerNorm(obs_dim): biased variance, eps 1e-5
        float m = 0.0f;
#pragma unroll
        for (int k = 0; k < MAXOBS; ++k) m += x[k];
        m /= (float)a.obs_dim;
        float v = 0.0f;
#pragma unroll
        for (int k = 0; k < MAXOBS; ++k) if (k < a.obs_dim) { x[k] -= m; v = fmaf(x[k], x[k], v); }
        const float is = rsqrtf(v / (float)a.obs_dim + 1e-5f);
#pragma unroll
        for (int k = 0; k < MAXOBS; ++k) x[k] = k < a.obs_dim ? fmaf(x[k] * is, W[L::F0G + k], W[L::F0B + k]) : 0.0f;
      }
#pragma unroll
      for (int q = 0; q < MAXOBS / 8; ++q) write_planes8<MTL, NP>(PA, srow, 8 * q, x + 8 * q);
    }
  }
  write_planes8<MTL, NP>(PH, srow, 8 * spart, hv);
  if constexpr (NP == 2) {
    float* hf = reinterpret_cast<float*>(PH + 2 * PLN);
    *reinterpret_cast<float4*>(hf + srow * RS + 8 * spart) = make_float4(hv[0], hv[1], hv[2], hv[3]);
    *reinterpret_cast<float4*>(hf + srow * RS + 8 * spart + 4) = make_float4(hv[4], hv[5], hv[6], hv[7]);
  }
  if constexpr (!WIDE) {
    __syncthreads();
    // ---- base MLP layer 1 (K = 32: one k-step)
    AF<MTL, NP> A;
    load_af<MTL, NP>(PA, lane, 0, A);
    floatx4 acc[MTL], lo[MTL];
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) { acc[mt] = splat4(W[L::B1 + w * 16 + col]); lo[mt] = splat4(0.0f); }
    step2<MTL, NP>(lo, acc, A, b1.s[0]);
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) acc[mt] += lo[mt];
    relu_out(stg, acc, w, lane);
  } else {
    // ---- the wide input: thread (row, part) stages columns 128 kb + 8 part .. + 7 of every 128-column K-block
    const int D = wx.dim[net], kp = wx.kpad[net], nst = kp / 32;
    const float* __restrict__ xin = net == 0 ? a.obs + (a.obs_compact ? (long long)sn : senv) * D : wx.cin + (long long)(sn / wx.cna) * wx.cstride;
    if (net == 0 && a.n_shoot && spart == 0) {   // the prior reads the actor's raw obs (ppo_actor.py; thresholds as above)
      const float ang = xin[11] * 57.29577951308232f, dist = xin[13] * 10000.0f;
      ab0[srow][0] = dist <= 8000.0f ? 10.0f : (dist <= 12000.0f ? 6.0f : 3.0f);
      ab0[srow][1] = ang <= 22.5f ? 3.0f : (ang <= 45.0f ? 6.0f : 10.0f);
    }
    const float* fg = W + WideLay<NP>::F0G(kp);
    const float* fb = fg + kp;
    float mean = 0.0f, is = 1.0f;
    if (a.use_fn) {   // LayerNorm(D) over the full width: the parts' sums through the staging rows (free until layer 1's output)
      float s = 0.0f;
      for (int c0 = 8 * spart; c0 < D; c0 += HID)
#pragma unroll
        for (int i = 0; i < 8; ++i) if (c0 + i < D) s += xin[c0 + i];
      stg[srow * RS + spart] = s;
      __syncthreads();
      s = 0.0f;
#pragma unroll
      for (int q = 0; q < 16; ++q) s += stg[srow * RS + q];
      mean = s / (float)D;
      float v = 0.0f;
      for (int c0 = 8 * spart; c0 < D; c0 += HID)
#pragma unroll
        for (int i = 0; i < 8; ++i) if (c0 + i < D) { const float d = xin[c0 + i] - mean; v = fmaf(d, d, v); }
      stg[srow * RS + 16 + spart] = v;
      __syncthreads();
      v = 0.0f;
#pragma unroll
      for (int q = 0; q < 16; ++q) v += stg[srow * RS + 16 + q];
      is = rsqrtf(v / (float)D + 1e-5f);
    }
    // ---- base MLP layer 1: K = kp in blocks of up to four k-steps, wave w's tile of W1 one block ahead of the staging
    const uint4* w1t = reinterpret_cast<const uint4*>(W + L::END + w * ctl8::Lay<NP>::tile_floats(kp)) + lane;
    floatx4 acc[MTL], lo[MTL];
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) { acc[mt] = splat4(W[L::B1 + w * 16 + col]); lo[mt] = splat4(0.0f); }
    for (int kb = 0; kb < nst; kb += 4) {
      BS<NP> bw[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) if (kb + s < nst) load_bs<NP>(w1t, kb + s, bw[s]);
      if (kb) __syncthreads();   // the previous block's A operands are read
      const int c0 = 32 * kb + 8 * spart;
      if (c0 < kp) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int c = c0 + i;
          v[i] = c < D ? (a.use_fn ? fmaf((xin[c] - mean) * is, fg[c], fb[c]) : xin[c]) : 0.0f;
        }
        write_planes8<MTL, NP>(PA, srow, 8 * spart, v);
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (kb + s < nst) {
          AF<MTL, NP> A;
          load_af<MTL, NP>(PA, lane, s, A);
          step2<MTL, NP>(lo, acc, A, bw[s]);
        }
    }
    prefetch_bt<HID, NP>(W + L::W2 + w * L::T128, lane, bt);
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) acc[mt] += lo[mt];
    relu_out(stg, acc, w, lane);
  }
  __syncthreads();
  layer_norm_planes<MTL, NP>(stg, PA, W + L::G1, W + L::BE1, tid);
  // ---- base MLP layer 2
  {
    floatx4 acc[MTL];
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) acc[mt] = splat4(W[L::B2 + w * 16 + col]);
    layer128<MTL, NP>(bt, PA, lane, acc);
    relu_out(stg, acc, w, lane);
  }
  constexpr int RING = 3;
  BS<NP> ring[RING][3];
#pragma unroll
  for (int st = 0; st < RING - 1; ++st) pol::ring_load<NP>(W, w, lane, st, ring[st]);
  __builtin_amdgcn_sched_barrier(0);
  __syncthreads();
  layer_norm_planes<MTL, NP>(stg, PA, W + L::G2, W + L::BE2, tid);
  // ---- GRU cell (gate order r, z, n) on the masked state: wave w owns hidden units 16 w .. 16 w + 15
  {
    const int unit = w * 16 + col;
    const float br = W[L::BIH + unit] + W[L::BHH + unit], bz = W[L::BIH + 128 + unit] + W[L::BHH + 128 + unit];
    const float bin = W[L::BIH + 256 + unit], bhn = W[L::BHH + 256 + unit];
    floatx4 gr[MTL], gz[MTL], in_[MTL], hn[MTL];
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) { gr[mt] = splat4(br); gz[mt] = splat4(bz); in_[mt] = splat4(bin); hn[mt] = splat4(bhn); }
    AF<MTL, NP> A[2];
    load_af<MTL, NP>(PA, lane, 0, A[0]);
#pragma unroll
    for (int st = 0; st < 8; ++st) {
      if (st + RING - 1 < 8) pol::ring_load<NP>(W, w, lane, st + RING - 1, ring[(st + RING - 1) % RING]);
      if (st + 1 < 8) load_af<MTL, NP>(st + 1 < 4 ? PA : PH, lane, (st + 1) & 3, A[(st + 1) % 2]);
      __builtin_amdgcn_sched_barrier(0);
      if (st < 4) gru_step<MTL, NP>(gr, gz, in_, A[st % 2], ring[st % RING]);
      else gru_step<MTL, NP>(gr, gz, hn, A[st % 2], ring[st % RING]);
      __builtin_amdgcn_sched_barrier(0);
    }
    prefetch_bt<HID, NP>(W + L::W3 + w * L::T128, lane, bt);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = c_row(mt, i, lane);
        const float rg = sigmoid_f(gr[mt][i]);
        const float zg = sigmoid_f(gz[mt][i]);
        const float ng = tanh_f(fmaf(rg, hn[mt][i], in_[mt][i]));
        stg[row * RS + unit] = fmaf(zg, state_value<MTL, NP>(PH, row, unit), (1.0f - zg) * ng);
      }
  }
  __syncthreads();
  {   // the new state goes out row-contiguous; every row of this workgroup was read into LDS above (in-place states are fine)
    const int n = POOL ? sn : i0 + srow;
    if (POOL ? tl.y + srow < tl.z : n < a.n) {
      float4* dst = reinterpret_cast<float4*>(a.h_out[net] + (size_t)n * HID + 8 * spart);
      dst[0] = *reinterpret_cast<const float4*>(stg + srow * RS + 8 * spart);
      dst[1] = *reinterpret_cast<const float4*>(stg + srow * RS + 8 * spart + 4);
    }
  }
  layer_norm_planes<MTL, NP>(stg, PA, W + L::GN, W + L::BEN, tid);
  // ---- action (value) MLP, two layers
  {
    floatx4 acc[MTL];
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) acc[mt] = splat4(W[L::B3 + w * 16 + col]);
    layer128<MTL, NP>(bt, PA, lane, acc);
    relu_out(stg, acc, w, lane);
  }
  prefetch_bt<HID, NP>(W + L::W4 + w * L::T128, lane, bt);
  __syncthreads();
  layer_norm_planes<MTL, NP>(stg, PA, W + L::G3, W + L::BE3, tid);
  {
    floatx4 acc[MTL];
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) acc[mt] = splat4(W[L::B4 + w * 16 + col]);
    layer128<MTL, NP>(bt, PA, lane, acc);
    relu_out(stg, acc, w, lane);
  }
  __syncthreads();
  layer_norm_planes<MTL, NP>(stg, PA, W + L::G4, W + L::BE4, tid);

  if (!POOL && net == 1) {   // ---- the critic: value_out = column 0 of tile 0 (wave 0)
    if (w == 0) {
      prefetch_bt<HID, NP>(W + L::WO, lane, bt);
      floatx4 acc[MTL];
#pragma unroll
      for (int mt = 0; mt < MTL; ++mt) acc[mt] = splat4(W[L::BO + col]);
      layer128<MTL, NP>(bt, PA, lane, acc);
      if (col == 0)
#pragma unroll
        for (int mt = 0; mt < MTL; ++mt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int n = i0 + c_row(mt, i, lane);
            if (n < a.n) a.values[n] = acc[mt][i];
          }
    }
    return;
  }
  // ---- the actor's heads: tile w, and tile 8 + w for waves 0..2; logits to lg [column][row] (over the GRU-state planes, last read
  // before three barriers)
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int tile = w + 8 * t;
    if (tile < HT) {
      prefetch_bt<HID, NP>(W + L::WO + tile * L::T128, lane, bt);
      floatx4 acc[MTL];
#pragma unroll
      for (int mt = 0; mt < MTL; ++mt) acc[mt] = splat4(W[L::BO + tile * 16 + col]);
      layer128<MTL, NP>(bt, PA, lane, acc);
#pragma unroll
      for (int mt = 0; mt < MTL; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) lg[(tile * 16 + col) * LSR + c_row(mt, i, lane)] = acc[mt][i];
    }
  }
  __syncthreads();
  // ---- sampling: thread = (head, row); log-probs of the chosen actions from an fp32 log-softmax (max first)
  const int nh = a.n_cat + a.n_shoot;
  if (tid < nh * R) {
    const int head = tid / R, row = tid % R, n = POOL ? px.order[min(tl.y + row, tl.z - 1)] : i0 + row;
    const float u = a.deterministic ? 0.0f : pol::policy_uniform(a.seed, a.counter, n, head);
    float act, lp;
    if (head < a.n_cat) {
      const int off = a.cat_off[head], cnt = a.cat_cnt[head];
      float m = lg[off * LSR + row];
      int am = 0;
      for (int j = 1; j < cnt; ++j) {
        const float v = lg[(off + j) * LSR + row];
        if (v > m) { m = v; am = j; }
      }
      float s = 0.0f;
      for (int j = 0; j < cnt; ++j) s += __expf(lg[(off + j) * LSR + row] - m);
      int pick = am;
      if (!a.deterministic) {
        const float target = u * s;
        float c = 0.0f;
        pick = -1;
        int last = 0;
        for (int j = 0; j < cnt; ++j) {
          const float e = __expf(lg[(off + j) * LSR + row] - m);
          if (e > 0.0f) last = j;
          c += e;
          if (pick < 0 && c > target) pick = j;
        }
        if (pick < 0) pick = last;   // u * s at or above the rounded total
      }
      act = (float)pick;
      lp = (lg[(off + pick) * LSR + row] - m) - __logf(s);
    } else {   // BetaShootBernoulli (distributions.py) with the prior of ppo_actor.py
      const int mh = head - a.n_cat;
      const float z0 = lg[(MAXLOGITS + 2 * mh) * LSR + row], z1 = lg[(MAXLOGITS + 2 * mh + 1) * LSR + row];
      const float al = 1.0f + (100.0f - softplus_t(100.0f - softplus_t(z0)));
      const float be = 1.0f + (100.0f - softplus_t(100.0f - softplus_t(z1)));
      const float aa = al + ab0[row][0];
      const float p = aa / (aa + be + ab0[row][1]);
      const bool fire = a.deterministic ? p > 0.5f : u >= 1.0f - p;
      // torch Bernoulli(probs).log_prob: probs clamped to [eps, 1 - eps] (eps = 2^-23)
      const float pc = fminf(fmaxf(p, 1.1920928955078125e-07f), 1.0f - 1.1920928955078125e-07f);
      act = fire ? 1.0f : 0.0f;
      lp = fire ? __logf(pc) : log1pf(-pc);
    }
    lpart[row][head] = lp;
    if (POOL ? tl.y + row < tl.z : n < a.n) {
      const long long env = (long long)(n / a.na) * a.A + a.a0 + n % a.na;
      a.actions[env * a.act_stride + head] = act;
    }
  }
  __syncthreads();
  if (tid < R && (POOL ? tl.y + tid < tl.z : i0 + tid < a.n)) {   // ACTLayer.forward: the heads' log-probs summed in head order
    float s = 0.0f;
    for (int h = 0; h < nh; ++h) s += lpart[tid][h];
    a.logp[POOL ? px.order[tl.y + tid] : i0 + tid] = s;
  }
}

template <int NP>
__global__ __launch_bounds__(512) void policy_values_kernel(pol::Args a) { policy_body<NP, false, true>(a, pol::Wide{}); }
// the MAPPO policy (wide inputs, a centralised critic): csrc/policy_host.hpp, ac_policy_get_actions_mappo / ac_policy_get_values
template <int NP>
__global__ __launch_bounds__(512) void policy_wide_kernel(pol::Args a, pol::Wide x) { policy_body<NP, true, false>(a, x); }

// the pool of actors (csrc/policy_pool.hpp, ac_policy_pool_act): grid = the plan's tiles (or a bound, past which workgroups exit)
template <int NP>
__global__ __launch_bounds__(512) void policy_pool_kernel(pol::Args a, pol::Pool p) { policy_body<NP, false, false, true>(a, pol::Wide{}, p); }
template <int NP>
__global__ __launch_bounds__(512) void policy_pool_wide_kernel(pol::Args a, pol::Wide x, pol::Pool p) { policy_body<NP, true, false, true>(a, x, p); }

template <int NP>
__global__ __launch_bounds__(512) void policy_kernel(pol::Args a) {
  using namespace ctl8;
  using namespace pol;
  using ctl::sigmoid_f; using ctl::tanh_f;
  using L = pol::Lay<NP>;
  using G = Geo8<MTL>;
  constexpr int PLN = G::PLN;
  // the GRU state as piece planes (+ its fp32 copy behind them with two pieces: they do not add up to it exactly); the logits later
  constexpr int PHN = NP == 2 ? 2 * PLN + 2 * R * RS : 3 * PLN;
  __shared__ __attribute__((aligned(16))) unsigned short PA[NP * PLN];   // activations as piece planes [piece][row][k]
  __shared__ __attribute__((aligned(16))) unsigned short PH[PHN];
  __shared__ __attribute__((aligned(16))) float stg[R * RS];             // a layer's fp32 outputs [row][k] on their way to LayerNorm
  __shared__ float ab0[R][2];                                            // alpha0 / beta0 of the shoot prior
  __shared__ float lpart[R][MAXCAT + NSHOOT];                            // per-head log-probs
  static_assert(sizeof(unsigned short) * PHN >= sizeof(float) * HCOLS * LSR, "the logits reuse the GRU-state planes");
  float* lg = reinterpret_cast<float*>(PH);

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int net = blockIdx.y;                  // 0 actor, 1 critic
  const int i0 = blockIdx.x * R;
  const float* __restrict__ W = a.W[net];
  const int col = lane & 15;
  const int srow = tid % R, spart = tid / R;   // staging: thread = (row, 8-feature part)
  const int sn = min(i0 + srow, a.n - 1);
  const long long senv = (long long)(sn / a.na) * a.A + a.a0 + sn % a.na;

  // ---- stage: the observation (LayerNorm'd when use_feature_normalization), the masked GRU state, the shoot prior
  BT<32, NP> b1;
  prefetch_bt<32, NP>(W + L::W1 + w * L::T32, lane, b1);
  BT<HID, NP> bt;
  prefetch_bt<HID, NP>(W + L::W2 + w * L::T128, lane, bt);
  const float mk = a.masks[sn];
  float hv[8];
  {
    const float4* hp = reinterpret_cast<const float4*>(a.h_in[net] + (size_t)sn * HID + 8 * spart);
    const float4 h0 = hp[0], h1 = hp[1];
    hv[0] = h0.x * mk; hv[1] = h0.y * mk; hv[2] = h0.z * mk; hv[3] = h0.w * mk;
    hv[4] = h1.x * mk; hv[5] = h1.y * mk; hv[6] = h1.z * mk; hv[7] = h1.w * mk;
  }
  if (spart == 0) {
    const float* ob = a.obs + (a.obs_compact ? (long long)sn : senv) * a.obs_dim;
    float x[MAXOBS];
#pragma unroll
    for (int k = 0; k < MAXOBS; ++k) x[k] = k < a.obs_dim ? ob[k] : 0.0f;
    if (net == 0 && a.n_shoot) {   // ppo_actor.py: alpha0 3 / 6 (<= 12 km) / 10 (<= 8 km), beta0 10 / 6 (<= 45 deg) / 3 (<= 22.5 deg)
      const float ang = x[11] * 57.29577951308232f, dist = x[13] * 10000.0f;
      ab0[srow][0] = dist <= 8000.0f ? 10.0f : (dist <= 12000.0f ? 6.0f : 3.0f);
      ab0[srow][1] = ang <= 22.5f ? 3.0f : (ang <= 45.0f ? 6.0f : 10.0f);
    }
    if (a.use_fn) {   // torch.nn.LayerNorm(obs_dim): biased variance, eps 1e-5
      float m = 0.0f;
#pragma unroll
      for (int k = 0; k < MAXOBS; ++k) m += x[k];
      m /= (float)a.obs_dim;
      float v = 0.0f;
#pragma unroll
      for (int k = 0; k < MAXOBS; ++k) if (k < a.obs_dim) { x[k] -= m; v = fmaf(x[k], x[k], v); }
      const float is = rsqrtf(v / (float)a.obs_dim + 1e-5f);
#pragma unroll
      for (int k = 0; k < MAXOBS; ++k) x[k] = k < a.obs_dim ? fmaf(x[k] * is, W[L::F0G + k], W[L::F0B + k]) : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < MAXOBS / 8; ++q) write_planes8<MTL, NP>(PA, srow, 8 * q, x + 8 * q);
  }
  write_planes8<MTL, NP>(PH, srow, 8 * spart, hv);
  if constexpr (NP == 2) {
    float* hf = reinterpret_cast<float*>(PH + 2 * PLN);
    *reinterpret_cast<float4*>(hf + srow * RS + 8 * spart) = make_float4(hv[0], hv[1], hv[2], hv[3]);
    *reinterpret_cast<float4*>(hf + srow * RS + 8 * spart + 4) = make_float4(hv[4], hv[5], hv[6], hv[7]);
  }
  __syncthreads();

  // ---- base MLP layer 1 (K = 32: one k-step)
  {
    AF<MTL, NP> A;
    load_af<MTL, NP>(PA, lane, 0, A);
    floatx4 acc[MTL], lo[MTL];
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) { acc[mt] = splat4(W[L::B1 + w * 16 + col]); lo[mt] = splat4(0.0f); }
    step2<MTL, NP>(lo, acc, A, b1.s[0]);
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) acc[mt] += lo[mt];
    relu_out(stg, acc, w, lane);
  }
  __syncthreads();
  layer_norm_planes<MTL, NP>(stg, PA, W + L::G1, W + L::BE1, tid);
  // ---- base MLP layer 2
  {
    floatx4 acc[MTL];
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) acc[mt] = splat4(W[L::B2 + w * 16 + col]);
    layer128<MTL, NP>(bt, PA, lane, acc);
    relu_out(stg, acc, w, lane);
  }
  constexpr int RING = 3;
  BS<NP> ring[RING][3];
#pragma unroll
  for (int st = 0; st < RING - 1; ++st) pol::ring_load<NP>(W, w, lane, st, ring[st]);
  __builtin_amdgcn_sched_barrier(0);
  __syncthreads();
  layer_norm_planes<MTL, NP>(stg, PA, W + L::G2, W + L::BE2, tid);
  // ---- GRU cell (gate order r, z, n) on the masked state: wave w owns hidden units 16 w .. 16 w + 15
  {
    const int unit = w * 16 + col;
    const float br = W[L::BIH + unit] + W[L::BHH + unit], bz = W[L::BIH + 128 + unit] + W[L::BHH + 128 + unit];
    const float bin = W[L::BIH + 256 + unit], bhn = W[L::BHH + 256 + unit];
    floatx4 gr[MTL], gz[MTL], in_[MTL], hn[MTL];
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) { gr[mt] = splat4(br); gz[mt] = splat4(bz); in_[mt] = splat4(bin); hn[mt] = splat4(bhn); }
    AF<MTL, NP> A[2];
    load_af<MTL, NP>(PA, lane, 0, A[0]);
#pragma unroll
    for (int st = 0; st < 8; ++st) {
      if (st + RING - 1 < 8) pol::ring_load<NP>(W, w, lane, st + RING - 1, ring[(st + RING - 1) % RING]);
      if (st + 1 < 8) load_af<MTL, NP>(st + 1 < 4 ? PA : PH, lane, (st + 1) & 3, A[(st + 1) % 2]);
      __builtin_amdgcn_sched_barrier(0);
      if (st < 4) gru_step<MTL, NP>(gr, gz, in_, A[st % 2], ring[st % RING]);
      else gru_step<MTL, NP>(gr, gz, hn, A[st % 2], ring[st % RING]);
      __builtin_amdgcn_sched_barrier(0);
    }
    prefetch_bt<HID, NP>(W + L::W3 + w * L::T128, lane, bt);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = c_row(mt, i, lane);
        const float rg = sigmoid_f(gr[mt][i]);
        const float zg = sigmoid_f(gz[mt][i]);
        const float ng = tanh_f(fmaf(rg, hn[mt][i], in_[mt][i]));
        stg[row * RS + unit] = fmaf(zg, state_value<MTL, NP>(PH, row, unit), (1.0f - zg) * ng);
      }
  }
  __syncthreads();
  {   // the new state goes out row-contiguous; every row of this workgroup was read into LDS above (in-place states are fine)
    const int n = i0 + srow;
    if (n < a.n) {
      float4* dst = reinterpret_cast<float4*>(a.h_out[net] + (size_t)n * HID + 8 * spart);
      dst[0] = *reinterpret_cast<const float4*>(stg + srow * RS + 8 * spart);
      dst[1] = *reinterpret_cast<const float4*>(stg + srow * RS + 8 * spart + 4);
    }
  }
  layer_norm_planes<MTL, NP>(stg, PA, W + L::GN, W + L::BEN, tid);
  // ---- action (value) MLP, two layers
  {
    floatx4 acc[MTL];
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) acc[mt] = splat4(W[L::B3 + w * 16 + col]);
    layer128<MTL, NP>(bt, PA, lane, acc);
    relu_out(stg, acc, w, lane);
  }
  prefetch_bt<HID, NP>(W + L::W4 + w * L::T128, lane, bt);
  __syncthreads();
  layer_norm_planes<MTL, NP>(stg, PA, W + L::G3, W + L::BE3, tid);
  {
    floatx4 acc[MTL];
#pragma unroll
    for (int mt = 0; mt < MTL; ++mt) acc[mt] = splat4(W[L::B4 + w * 16 + col]);
    layer128<MTL, NP>(bt, PA, lane, acc);
    relu_out(stg, acc, w, lane);
  }
  __syncthreads();
  layer_norm_planes<MTL, NP>(stg, PA, W + L::G4, W + L::BE4, tid);

  if (net == 1) {   // ---- the critic: value_out = column 0 of tile 0 (wave 0)
    if (w == 0) {
      prefetch_bt<HID, NP>(W + L::WO, lane, bt);
      floatx4 acc[MTL];
#pragma unroll
      for (int mt = 0; mt < MTL; ++mt) acc[mt] = splat4(W[L::BO + col]);
      layer128<MTL, NP>(bt, PA, lane, acc);
      if (col == 0)
#pragma unroll
        for (int mt = 0; mt < MTL; ++mt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int n = i0 + c_row(mt, i, lane);
            if (n < a.n) a.values[n] = acc[mt][i];
          }
    }
    return;
  }
  // ---- the actor's heads: tile w, and tile 8 + w for waves 0..2; logits to lg [column][row] (over the GRU-state planes, last read
  // before three barriers)
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int tile = w + 8 * t;
    if (tile < HT) {
      prefetch_bt<HID, NP>(W + L::WO + tile * L::T128, lane, bt);
      floatx4 acc[MTL];
#pragma unroll
      for (int mt = 0; mt < MTL; ++mt) acc[mt] = splat4(W[L::BO + tile * 16 + col]);
      layer128<MTL, NP>(bt, PA, lane, acc);
#pragma unroll
      for (int mt = 0; mt < MTL; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) lg[(tile * 16 + col) * LSR + c_row(mt, i, lane)] = acc[mt][i];
    }
  }
  __syncthreads();
  // ---- sampling: thread = (head, row); log-probs of the chosen actions from an fp32 log-softmax (max first)
  const int nh = a.n_cat + a.n_shoot;
  if (tid < nh * R) {
    const int head = tid / R, row = tid % R, n = i0 + row;
    const float u = a.deterministic ? 0.0f : pol::policy_uniform(a.seed, a.counter, n, head);
    float act, lp;
    if (head < a.n_cat) {
      const int off = a.cat_off[head], cnt = a.cat_cnt[head];
      float m = lg[off * LSR + row];
      int am = 0;
      for (int j = 1; j < cnt; ++j) {
        const float v = lg[(off + j) * LSR + row];
        if (v > m) { m = v; am = j; }
      }
      float s = 0.0f;
      for (int j = 0; j < cnt; ++j) s += __expf(lg[(off + j) * LSR + row] - m);
      int pick = am;
      if (!a.deterministic) {
        const float target = u * s;
        float c = 0.0f;
        pick = -1;
        int last = 0;
        for (int j = 0; j < cnt; ++j) {
          const float e = __expf(lg[(off + j) * LSR + row] - m);
          if (e > 0.0f) last = j;
          c += e;
          if (pick < 0 && c > target) pick = j;
        }
        if (pick < 0) pick = last;   // u * s at or above the rounded total
      }
      act = (float)pick;
      lp = (lg[(off + pick) * LSR + row] - m) - __logf(s);
    } else {   // BetaShootBernoulli (distributions.py) with the prior of ppo_actor.py
      const int mh = head - a.n_cat;
      const float z0 = lg[(MAXLOGITS + 2 * mh) * LSR + row], z1 = lg[(MAXLOGITS + 2 * mh + 1) * LSR + row];
      const float al = 1.0f + (100.0f - softplus_t(100.0f - softplus_t(z0)));
      const float be = 1.0f + (100.0f - softplus_t(100.0f - softplus_t(z1)));
      const float aa = al + ab0[row][0];
      const float p = aa / (aa + be + ab0[row][1]);
      const bool fire = a.deterministic ? p > 0.5f : u >= 1.0f - p;
      // torch Bernoulli(probs).log_prob: probs clamped to [eps, 1 - eps] (eps = 2^-23)
      const float pc = fminf(fmaxf(p, 1.1920928955078125e-07f), 1.0f - 1.1920928955078125e-07f);
      act = fire ? 1.0f : 0.0f;
      lp = fire ? __logf(pc) : log1pf(-pc);
    }
    lpart[row][head] = lp;
    if (n < a.n) {
      const long long env = (long long)(n / a.na) * a.A + a.a0 + n % a.na;
      a.actions[env * a.act_stride + head] = act;
    }
  }
  __syncthreads();
  if (tid < R && i0 + tid < a.n) {   // ACTLayer.forward: the heads' log-probs summed in head order
    float s = 0.0f;
    for (int h = 0; h < nh; ++h) s += lpart[tid][h];
    a.logp[i0 + tid] = s;
  }
}
