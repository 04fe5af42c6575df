// Stand-alone check of the rules the native VecEnv.step applies (csrc/native_step_pick.hpp): which result set a step writes into for every
// hold pattern of every ring size, the two-set alternation, and which action buffers it takes as they are. Built with
// -fsanitize=address,undefined and run on the CPU by tests/test_native_step_host.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "native_step_pick.hpp"

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

using namespace native_step;

// the rule as HipVecEnv._next_set states it, kept apart from the header's loop: candidates in ring order after cur, cur last
static int reference_pick(int cur, const std::vector<bool>& held) {
  const int n = (int)held.size();
  std::vector<int> order;
  for (int k = cur + 1; k < n; ++k) order.push_back(k);
  for (int k = 0; k <= cur; ++k) order.push_back(k);
  for (int k : order)
    if (!held[k]) return k;
  return FALLBACK;
}

static void every_hold_pattern() {
  for (int n = 1; n <= MAX_SETS; ++n)
    for (unsigned pattern = 0; pattern < (1u << n); ++pattern) {
      std::vector<bool> h(n);
      for (int k = 0; k < n; ++k) h[k] = (pattern >> k) & 1u;
      for (int cur = 0; cur < n; ++cur) {
        std::vector<int> asked;
        const int got = pick_ring(cur, n, [&](int k) { asked.push_back(k); return (bool)h[k]; });
        CHECK(got == reference_pick(cur, h));
        // asked in ring order, every set at most once, nothing after the first free one
        CHECK((int)asked.size() <= n);
        for (size_t i = 0; i < asked.size(); ++i) {
          CHECK(asked[i] == (cur + 1 + (int)i) % n);
          CHECK(i + 1 == asked.size() || h[asked[i]]);
        }
        if (got != FALLBACK) CHECK(!asked.empty() && asked.back() == got);
      }
    }
}

static void rings_that_are_none() {
  auto never = [](int) { return false; };
  CHECK(pick_ring(0, 0, never) == FALLBACK);
  CHECK(pick_ring(0, MAX_SETS + 1, never) == FALLBACK);
  CHECK(pick_ring(-1, 4, never) == FALLBACK);
  CHECK(pick_ring(4, 4, never) == FALLBACK);
  CHECK(pick_ring(3, 4, never) == 0);
}

static void alternation() {
  CHECK(pick_alternate(0) == 1);
  CHECK(pick_alternate(1) == 0);
  CHECK(pick_alternate(2) == FALLBACK);
  CHECK(pick_alternate(-1) == FALLBACK);
  int cur = 0, ones = 0;
  for (int i = 0; i < 9; ++i) { cur = pick_alternate(cur); ones += cur; }
  CHECK(cur == 1 && ones == 5);
}

static void held_compares_every_count() {
  const long base[MAX_ARRAYS] = {3, 3, 3, 4, 2};
  for (int n = 1; n <= MAX_ARRAYS; ++n) {
    std::vector<long> now(base, base + n);       // exactly n entries: a read past them is the sanitizer's to catch
    CHECK(!held(now.data(), base, n));
    for (int i = 0; i < n; ++i) {
      now[i] += 1;
      CHECK(held(now.data(), base, n));
      now[i] -= 2;                               // (fewer than the baseline is not "free" either: something is off, stay away)
      CHECK(held(now.data(), base, n));
      now[i] += 1;
    }
  }
  const long more[MAX_ARRAYS] = {3, 3, 3, 4, 9};
  CHECK(!held(more, base, 4));                   // a count beyond n_arrays is not looked at
}

static void action_buffers() {
  const size_t n = 4096u * 2u * 4u;
  CHECK(fast_actions("f", 4, (std::ptrdiff_t)(n * 4), n));
  CHECK(fast_actions("<f", 4, (std::ptrdiff_t)(n * 4), n));
  CHECK(fast_actions("=f", 4, (std::ptrdiff_t)(n * 4), n));
  CHECK(fast_actions("@f", 4, (std::ptrdiff_t)(n * 4), n));
  CHECK(!fast_actions(nullptr, 4, (std::ptrdiff_t)(n * 4), n));
  CHECK(!fast_actions("", 4, (std::ptrdiff_t)(n * 4), n));
  CHECK(!fast_actions("<", 4, (std::ptrdiff_t)(n * 4), n));
  CHECK(!fast_actions(">f", 4, (std::ptrdiff_t)(n * 4), n));
  CHECK(!fast_actions("!f", 4, (std::ptrdiff_t)(n * 4), n));
  CHECK(!fast_actions("d", 8, (std::ptrdiff_t)(n * 8), n));
  CHECK(!fast_actions("i", 4, (std::ptrdiff_t)(n * 4), n));
  CHECK(!fast_actions("ff", 4, (std::ptrdiff_t)(n * 4), n));
  CHECK(!fast_actions("f", 8, (std::ptrdiff_t)(n * 4), n));
  CHECK(!fast_actions("f", 4, (std::ptrdiff_t)(n * 4 - 4), n));
  CHECK(!fast_actions("f", 4, (std::ptrdiff_t)(n * 4 + 4), n));
  CHECK(!fast_actions("f", 4, -1, n));
  CHECK(!fast_actions("f", 4, 0, n));
  char* fmt = new char[2];                       // a format string with nothing behind its terminator
  std::memcpy(fmt, "f", 2);
  CHECK(fast_actions(fmt, 4, 16, 4));
  delete[] fmt;
  char* lone = new char[1];
  lone[0] = '\0';
  CHECK(!fast_actions(lone, 4, 16, 4));
  delete[] lone;
}

int main() {
  every_hold_pattern();
  rings_that_are_none();
  alternation();
  held_compares_every_count();
  action_buffers();
  if (failures) {
    printf("%d native step pick checks FAILED\n", failures);
    return 1;
  }
  printf("native step pick checks ok\n");
  return 0;
}
