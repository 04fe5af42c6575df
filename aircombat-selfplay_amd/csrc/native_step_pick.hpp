// Which result set a VecEnv.step writes into, and which inputs the native step takes itself: the rules of HipVecEnv._next_set and of
// the fast-path test in HipVecEnv.step (vec_env.py), in plain C++ -- no Python, no HIP. csrc/native_step.cpp applies them to live
// objects; tests/host/native_step_main.cpp builds this file alone under the sanitizers.
#pragma once
#include <cstddef>

namespace native_step {

constexpr int MAX_SETS = 8;     // AC_HOST_SETS (include/aircombat.h)
constexpr int MAX_ARRAYS = 5;   // obs, rewards, dones, info words and, for the share family, share_obs
constexpr int FALLBACK = -1;    // the caller's own path decides: grow the ring, or stage and copy

// copy=False: the other one of two sets, whoever holds what.
inline int pick_alternate(int cur) { return (cur == 0 || cur == 1) ? (cur ^ 1) : FALLBACK; }

// A set is held when any of its arrays counts more references than it did when only the VecEnv had it.
template <class Count>
inline bool held(const Count* now, const Count* baseline, int n_arrays) {
  for (int i = 0; i < n_arrays; ++i)
    if (now[i] != baseline[i]) return true;
  return false;
}

// Default mode: the next set of the ring after `cur` that nobody holds, `cur` itself last. FALLBACK when every set is held (or the
// arguments make no ring). `is_held(k)` is asked for the sets in ring order and for no set after the first free one.
template <class IsHeld>
inline int pick_ring(int cur, int n_sets, IsHeld is_held) {
  if (n_sets < 1 || n_sets > MAX_SETS || cur < 0 || cur >= n_sets) return FALLBACK;
  for (int i = 1; i <= n_sets; ++i) {
    const int k = (cur + i) % n_sets;
    if (!is_held(k)) return k;
  }
  return FALLBACK;
}

// The action batch the native step hands to the library as it is: C-contiguous (the caller asks the exporter for that) float32 in native
// byte order, exactly n_floats values. `format` is the buffer protocol's struct string, or null for "unsigned bytes".
inline bool fast_actions(const char* format, std::ptrdiff_t itemsize, std::ptrdiff_t len_bytes, std::size_t n_floats) {
  if (!format || itemsize != (std::ptrdiff_t)sizeof(float)) return false;
  if (format[0] == '@' || format[0] == '=' || format[0] == '<') ++format;   // (the library is built for little-endian hosts only)
  if (format[0] != 'f' || format[1] != '\0') return false;
  return len_bytes >= 0 && (std::size_t)len_bytes == n_floats * sizeof(float);
}

}  // namespace native_step
