// Late actions ("Step outputs and the host boundary"): the host half of a step whose action rows are copied into the mapped
// set AFTER the doorbell, under the launch. Plain C++, no HIP: aircombat.hip includes it for ac_step_host_actions, and
// tests/host/late_actions_main.cpp builds it alone under the sanitizers.
//
// A row is the four control indices of one aircraft, 16 bytes. Whether a row the kernel reads is this step's cannot be told by a flag
// beside the rows (two reads across PCIe may be served in either order), so every row carries a two-bit tag in the two lowest mantissa
// bits of its fourth element, the throttle index: 1 or 2, alternating per use of a host set, so that what the set still holds from its
// previous use never matches. The row is written with ONE aligned 16-byte store: a 16-byte load sees it entirely old or entirely new.
// A float whose two trailing mantissa bits are zero (every integer below 2^22, so every MultiDiscrete index) comes back bit-exact once
// the kernel has masked the tag; any other throttle index is rounded toward zero by at most 3 ulp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace late {
enum { HDR_TAG = 0,       // word 0 of a set's header block: 0 = plain rows, taken as they are; 1 / 2 = the tag every row must carry
       HDR_RETRIES = 1,   // word 1: re-issued row loads of the step, summed over the systems waves (written by the device)
       HDR_BUDGET = 2,    // word 2: how often a systems wave may ask again before it gives up (read by the device only when it has to)
       HDR_WORDS = 16 };  // (one 64-byte line behind the set's action rows)
constexpr uint32_t TAG_MASK = 3u;

// the tag of a set's next late use: 1, 2, 1, ...
inline uint32_t next_tag(uint32_t prev) { return prev == 1u ? 2u : 1u; }

typedef uint32_t u32x4 __attribute__((vector_size(16), may_alias));   // (stored over float rows)

// Rows [row0, row1) of `src` (any alignment) -> `dst` (16-byte aligned: the mapped action buffer), each tagged and written with one
// aligned 16-byte store.
inline void copy_tag_rows(float* dst, const float* src, size_t row0, size_t row1, uint32_t tag) {
  const u32x4 keep = {~0u, ~0u, ~0u, ~TAG_MASK}, put = {0u, 0u, 0u, tag & TAG_MASK};
  u32x4* d = reinterpret_cast<u32x4*>(dst);
  for (size_t r = row0; r < row1; ++r) {
    u32x4 v;
    memcpy(&v, src + 4 * r, sizeof v);
    d[r] = (v & keep) | put;
  }
}
// what the kernel decodes from a tagged row's fourth element
inline float untag(float w) {
  uint32_t b;
  memcpy(&b, &w, sizeof b);
  b &= ~TAG_MASK;
  memcpy(&w, &b, sizeof b);
  return w;
}
// rows copied in front of the doorbell when a share `f` (0 .. 1) of `rows` goes behind it
inline size_t rows_before(size_t rows, double f) {
  if (!(f > 0.0)) return rows;
  if (f >= 1.0) return 0;
  const size_t after = (size_t)((double)rows * f);
  return rows - (after > rows ? rows : after);
}
}  // namespace late
