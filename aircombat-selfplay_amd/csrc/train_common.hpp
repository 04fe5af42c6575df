// What the device training layers share (gru_train.hpp, mlp_train.hpp, act_train.hpp, ppo_update.hpp, gru_layer_train.hpp; DESIGN.md §5,
// "What the training layers share"). Included in aircombat.hip ahead of them (same library, same error channel): the sum of the partial
// sets that every backward's workgroups leave in the workspace, whose order depends on the number of sets alone (no floating-point
// atomics: results are bit-identical from run to run), and the host arithmetic every C entry point repeats.
#pragma once
#include <initializer_list>

namespace trn {
// element e of the sum of sets 0 .. S - 1 (set s at ws + s * nel): chain j adds sets j, j + 8, .. in ascending order from 0.0f, then
// ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7))
__device__ __forceinline__ float sum_sets(const float* __restrict__ ws, int S, size_t nel, int e) {
  float a[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  int s = 0;
  for (; s + 8 <= S; s += 8)
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += ws[(size_t)(s + j) * nel + e];
  for (int j = 0; s < S; ++s, ++j) a[j] += ws[(size_t)s * nel + e];
  return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

inline int tiles(int M, int RT) { return (M + RT - 1) / RT; }
// workgroups of a persistent loop over the tiles, `cap` at most (also the number of partial sets a backward writes)
inline int capped_tiles(int M, int RT, int cap) { return tiles(M, RT) < cap ? tiles(M, RT) : cap; }

// -1 with the message when element (M + slack) * width is past a 32-bit index (slack: the tile rows indexed beyond M before a bounds test)
inline int rows_fit_i32(const std::string& who, int32_t M, int width, int slack) {
  if ((int64_t)M * width > (int64_t)INT32_MAX - (int64_t)slack * width)
    return fail(who + ": M * " + std::to_string(width) + " exceeds the kernels' 32-bit index");
  return 0;
}

// -1 with the message unless `code` is one of the AC_PRODUCTS_ values; `word` names the argument: "products" or "dense products"
inline int products_ok(const char* who, const char* word, int32_t code) {
  if (code != AC_PRODUCTS_FP32 && code != AC_PRODUCTS_BF16X3)
    return fail(std::string(who) + ": unknown " + word + " " + std::to_string(code) + " (AC_PRODUCTS_FP32 or AC_PRODUCTS_BF16X3)");
  return 0;
}

__host__ __device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (!aligned16(p)) return false;
  return true;
}
}  // namespace trn
