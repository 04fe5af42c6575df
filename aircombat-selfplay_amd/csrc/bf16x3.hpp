// The split-bf16 product of the training kernels (gru_train_split.hpp, gru_layer_train_split.hpp, mlp_train_split.hpp; DESIGN.md §5,
// "The split-bf16 product"): what AC_PRODUCTS_BF16X3 computes, in one place. The controller and policy kernels keep their own orders
// (mfma_layers.hpp) and do not come through here.
//
// Pieces. Every fp32 value is three bf16 pieces, x = b0 + b1 + b2 exactly (ctls::split3_pair, controller_pieces.hpp). A masked or
// padded value is +-0 and splits to three zero pieces.
// Terms. A product keeps the six terms b_i b_j with i + j <= 2, each an exact bf16 x bf16 product accumulated in fp32 by
// v_mfma_f32_16x16x32_bf16: good to about 2^-23 of itself, 24 instructions of 16 cycles per 128 k of a tile where the fp32 instruction
// takes 32 of 32 cycles. Within a k-step the terms run smallest first (TI / TJ), the controller's order (mfma_layers.hpp, gru_step).
// Operands. Lane l = 16 q + n of the instruction holds k = 8 q + e, e = 0 .. 7, of row n (A) or column n (B); result [i] is row
// 4 q + i of column n. Weights are read from the caller's fp32 tensor at every call and split in registers (12 VGPRs per k-step);
// nothing is kept between calls.
// Planes. A streamed operand is split by the thread that stores it into three bf16 planes in LDS, rows of K + 8 bf16 (80, 144, 272
// and 784 B: 4 banks mod 64 after every row, so the 16 rows of a lane quarter read distinct groups of banks), and read back as one
// ds_read_b128 per piece and k-step.
// k slots. Where the sum runs over a tile's 32 rows (the weight gradients), k slot 8 q + e of the instruction is row
// 16 (e / 4) + 4 q + e % 4: then a value in the result layout (rows 16 mt + 4 q + i of column n) IS the A operand, split in
// registers. The other operand is read from a transposed image [column][k slot] of rows of 32 + 8 bf16 (80 B: the 16 columns of a lane
// quarter cover the 64 banks once), in which a row pair 2 rp, 2 rp + 1 of one column is one 32-bit word.
#pragma once

namespace b3 {
using ctl8::floatx4;

__device__ __forceinline__ floatx4 mf(const uint4& a, const uint4& b, floatx4 acc) { return ctl8::mf<3>(a, b, acc); }
// the six kept terms (A piece, B piece), smallest first
constexpr int TI[6] = {2, 1, 0, 1, 0, 0}, TJ[6] = {0, 1, 2, 0, 1, 0};

// eight values along k -> one operand per piece
__device__ __forceinline__ void split8(const float (&v)[8], uint4 (&P)[3]) {
  unsigned a[4], b[4], c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) ctls::split3_pair(v[2 * j], v[2 * j + 1], a[j], b[j], c[j]);
  P[0] = make_uint4(a[0], a[1], a[2], a[3]); P[1] = make_uint4(b[0], b[1], b[2], b[3]); P[2] = make_uint4(c[0], c[1], c[2], c[3]);
}

// ------------------------------------------------------------------------------------------------ operands
// one operand of one k-step from the three planes (`pln` apart, in bf16): one ds_read_b128 per piece
__device__ __forceinline__ void read3(uint4 (&P)[3], const unsigned short* at, int pln) {
#pragma unroll
  for (int p = 0; p < 3; ++p) P[p] = *reinterpret_cast<const uint4*>(at + p * pln);
}
// eight adjacent fp32 (16-byte aligned) as two 16-byte loads
__device__ __forceinline__ void read8(float (&v)[8], const float* p) {
  const float4 v0 = *reinterpret_cast<const float4*>(p), v1 = *reinterpret_cast<const float4*>(p + 4);
  v[0] = v0.x; v[1] = v0.y; v[2] = v0.z; v[3] = v0.w; v[4] = v1.x; v[5] = v1.y; v[6] = v1.z; v[7] = v1.w;
}
// weight slices of lane quarter q: B[s] = the pieces of row[32 s + 8 q + e] (a row of W, 16-byte aligned), or of
// w[32 s + 8 q + e][col] (a column of W [.][ld])
template <int KSTEPS>
__device__ __forceinline__ void row_slice(uint4 (&B)[KSTEPS][3], const float* row, int q) {
#pragma unroll
  for (int s = 0; s < KSTEPS; ++s) {
    float v[8];
    read8(v, row + 32 * s + 8 * q);
    split8(v, B[s]);
  }
}
template <int KSTEPS>
__device__ __forceinline__ void col_slice(uint4 (&B)[KSTEPS][3], const float* w, int ld, int col, int q) {
#pragma unroll
  for (int s = 0; s < KSTEPS; ++s) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = w[(size_t)(32 * s + 8 * q + e) * ld + col];
    split8(v, B[s]);
  }
}

// ------------------------------------------------------------------------------------------------ the terms of one k-step
// One chain: all six terms, smallest first, into one accumulator per result. term(i, j) adds b_i(A) b_j(B) to every accumulator the
// caller keeps (acc = mf(A[i], B[j], acc) for each): the term loop is outermost, the accumulators innermost.
template <class F>
__device__ __forceinline__ void one_chain(F&& term) {
#pragma unroll
  for (int k = 0; k < 6; ++k) term(TI[k], TJ[k]);
}
// Three chains per result, closed by chain_sum. There are two assignments of the terms to the chains, and they are deliberately
// different: do not merge them, and choose by what happens to the result downstream.
//   pairs     c0 = (2,0), (1,0); c1 = (1,1), (0,1); c2 = (0,2), (0,0): two terms of every k-step each, the second-order terms lead.
//             The GRU's dh and dx (gru_seq_bwd_b3, gru_dx_b3).
//   by order  c0 = (2,0), (1,1), (0,2); c1 = (1,0), (0,1); c2 = (0,0): one chain per order i + j. The matrix instruction's
//             accumulation leans to one side by a small fraction of the accumulator's last place per step, so here only the b0 b0
//             steps run at the result's own magnitude. The MLP's dx (mlp_block_bwd_b3), which is summed over rows downstream (dbeta
//             and db of the block before): with all 24 terms in one chain it came out with a one-sided mean error (-0.044 of its rms
//             error at 4096 x 60, fp32 kernels +0.0002), and dbeta0 read 1.27 of its bound there.
__device__ __forceinline__ void chains_pairs(floatx4 (&c)[3], const uint4 (&A)[3], const uint4 (&B)[3]) {
  c[0] = mf(A[2], B[0], c[0]);
  c[1] = mf(A[1], B[1], c[1]);
  c[2] = mf(A[0], B[2], c[2]);
  c[0] = mf(A[1], B[0], c[0]);
  c[1] = mf(A[0], B[1], c[1]);
  c[2] = mf(A[0], B[0], c[2]);
}
__device__ __forceinline__ void chains_by_order(floatx4 (&c)[3], const uint4 (&A)[3], const uint4 (&B)[3]) {
  c[0] = mf(A[2], B[0], c[0]);
  c[1] = mf(A[1], B[0], c[1]);
  c[2] = mf(A[0], B[0], c[2]);
  c[0] = mf(A[1], B[1], c[0]);
  c[1] = mf(A[0], B[1], c[1]);
  c[0] = mf(A[0], B[2], c[0]);
}
// the chains of either form, added smallest first
__device__ __forceinline__ float chain_sum(const floatx4 (&c)[3], int i) { return (c[0][i] + c[1][i]) + c[2][i]; }

// ------------------------------------------------------------------------------------------------ split and store
// four adjacent values of a row -> their pieces as words w[pair][piece], and the words -> 8 bytes in each plane (`at` 8-byte aligned).
// Four is the one width the kernels store: a thread's float4 of a row.
__device__ __forceinline__ void split_row(unsigned (&w)[2][3], const float* v) {
  ctls::split3_pair(v[0], v[1], w[0][0], w[0][1], w[0][2]);
  ctls::split3_pair(v[2], v[3], w[1][0], w[1][1], w[1][2]);
}
__device__ __forceinline__ void store_words(unsigned short* at, int pln, const unsigned (&w)[2][3]) {
#pragma unroll
  for (int p = 0; p < 3; ++p) *reinterpret_cast<uint2*>(at + p * pln) = make_uint2(w[0][p], w[1][p]);
}
__device__ __forceinline__ void store_row(unsigned short* at, int pln, const float* v) {
  unsigned w[2][3];
  split_row(w, v);
  store_words(at, pln, w);
}
// this lane's four rows of one column (result layout) -> the three planes (row stride `ks` in bf16)
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

// ------------------------------------------------------------------------------------------------ k slots
// the k slot of row 2 rp of a 32-row tile (row 2 rp + 1 has the next): the inverse of "k slot 8 q + e is row 16 (e / 4) + 4 q + e % 4"
__device__ __forceinline__ int kslot(int rp) { return 8 * ((rp >> 1) & 3) + 4 * (rp >> 3) + 2 * (rp & 1); }
// a lane's result-layout values r[mt][i] (rows 16 mt + 4 q + i) as its eight k-slot values
__device__ __forceinline__ void to_kslots(float (&v)[8], const float (&r)[2][4]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = r[e >> 2][e & 3];
}
// the transposed image [column][k slot] (`kr` bf16 per column): b[p] = piece p of rows 2 rp (low half) and 2 rp + 1 of column `col`
__device__ __forceinline__ void store_pair(unsigned short* img, int pln, int kr, int col, int rp, const unsigned (&b)[3]) {
#pragma unroll
  for (int p = 0; p < 3; ++p) *reinterpret_cast<unsigned*>(img + p * pln + col * kr + kslot(rp)) = b[p];
}
}  // namespace b3
