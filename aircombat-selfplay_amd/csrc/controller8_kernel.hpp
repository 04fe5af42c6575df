// The low-level controller kernel, eight-wave form (network, arguments: controller_common.hpp; the piece arithmetic -- every fp32
// product as three exact fp16 x fp16 terms accumulated in fp32 -- and its helpers: controller_pieces.hpp; the four-wave kernel of rounds
// 2-3 that this one replaced on every grid is in the history).
// Two forms share the body (controller8_body.hpp): the fast one (controller8_kernel, two fp16 pieces, three terms) and the
// reference-precision one (controller8x3_kernel, AC_CTL_FP32: three bf16 pieces, six terms); controller8_forward_kernel runs either on given
// inputs (ac_controller_forward).
//
// Why eight waves. The four-wave kernel put ONE wave on each SIMD of a CU: 378 registers of weight prefetch per wave, and a wave issues
// in order -- so every weight load, every LDS read and every LayerNorm / gate / argmax instruction was time the SIMD's matrix pipe stood
// idle (round 3's counters: pipe busy 12.9 k of a wave's 38.8 k cycles; sharing a weight stream between two tiles, two workgroups per CU
// in lockstep and a software pipeline of two tiles all measured within 3 % of it). Here a workgroup is still one 32-aircraft tile, but
// EIGHT waves, two per SIMD, each owning 16 of a layer's output columns (v_mfma_f32_16x16x32_f16: M = 16 aircraft x N = 16 columns x
// K = 32 per instruction, two M-tiles per wave): the two waves of a SIMD run the same phase on different columns, so one's load issue and
// LDS waits sit under the other's matrix instructions, and the vector phases (LayerNorm, gate algebra, argmax, staging) are spread over
// twice the lanes. A operands are read from the LDS planes per k-step (two M-tiles x two pieces = four ds_read_b128 per 18 matrix
// instructions of a GRU k-step) instead of living in registers, weight pieces stream through a three-stage ring of one k-step each:
// under 200 registers, no scratch.
//
// Weight tiles for this form (ac_load_controller): tile(c, K) = the 16 output columns 16 c .. 16 c + 15 of a layer = K/32 k-steps x
// 2 pieces x 64 lanes x 8 fp16; element (s, p, lane, i) = piece p of W[j = 16 c + lane % 16][k = 32 s + 8 (lane / 16) + i] (the B
// operand map of the 16x16x32 instruction: lane l holds B[k = 8 (l >> 4) + i][col = l & 15]).
#pragma once

#include "mfma_layers.hpp"   // namespace ctl8: the layer pieces (shared with policy_kernel.hpp)

// SCRIPTED: the handle has scripted opponents (`use_baseline`); their state -> pose code is compiled into that instantiation only.
// MTL: 16-row M-tiles per wave = aircraft per workgroup / 16 (2 or 4).
// The env path, fast form (two fp16 pieces) ...
template <bool SCRIPTED, int MTL>
__global__ __launch_bounds__(512) void controller8_kernel(ctl::Args a) {
  constexpr int NP = 2;
  constexpr bool XIN = false;
  const float* const __restrict__ xin = nullptr;
  float* const __restrict__ logits = nullptr;
#include "controller8_body.hpp"
}
// ... and reference-precision form (three bf16 pieces, AC_CTL_FP32)
template <bool SCRIPTED, int MTL>
__global__ __launch_bounds__(512) void controller8x3_kernel(ctl::Args a) {
  constexpr int NP = 3;
  constexpr bool XIN = false;
  const float* const __restrict__ xin = nullptr;
  float* const __restrict__ logits = nullptr;
#include "controller8_body.hpp"
}
// the standalone forward (ac_controller_forward): inputs xin[n][12], GRU state a.H [128][n], logits[n][153] (may be null), actions a.low [n][4]
template <int NP, int MTL>
__global__ __launch_bounds__(512) void controller8_forward_kernel(ctl::Args a, const float* __restrict__ xin, float* __restrict__ logits) {
  constexpr bool SCRIPTED = false;
  constexpr bool XIN = true;
#include "controller8_body.hpp"
}
