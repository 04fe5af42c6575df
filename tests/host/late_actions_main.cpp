// Stand-alone check of the host half of the late-actions step (csrc/late_actions.hpp): the copy-and-tag routine, the tag alternation and
// the split of a batch around the doorbell. Built with -fsanitize=address,undefined and run on the CPU by tests/test_late_actions_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "late_actions.hpp"

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

static uint32_t bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }

// a destination of `rows` rows with guard rows on either side: 32-byte aligned, or (`odd`) 16-byte aligned only
struct Dst {
  void* raw;
  float* p;
  size_t rows, lead;
  explicit Dst(size_t n, bool odd = false) : rows(n), lead(odd ? 3 : 2) {
    const size_t total = 16 * (n + lead + 2);
    raw = aligned_alloc(32, (total + 31) / 32 * 32);
    p = (float*)raw + 4 * lead;
    for (size_t i = 0; i < 4 * (n + lead + 2); ++i) ((float*)raw)[i] = -77.0f;
  }
  ~Dst() { free(raw); }
  bool guards_intact() const {
    for (size_t i = 0; i < 4 * lead; ++i)
      if (((float*)raw)[i] != -77.0f) return false;
    for (int i = 0; i < 8; ++i)
      if (p[4 * rows + i] != -77.0f) return false;
    return true;
  }
};

static void round_trip_integers() {
  // every MultiDiscrete index and every integer up to 2^22 - 1 in the fourth element comes back bit-exact after the mask, under both tags
  for (uint32_t tag = 1; tag <= 2; ++tag) {
    const size_t n = 4096;
    std::vector<float> src(4 * n);
    for (size_t r = 0; r < n; ++r) {
      src[4 * r] = (float)(r % 41); src[4 * r + 1] = (float)((r * 7) % 41); src[4 * r + 2] = (float)((r * 13) % 41);
      src[4 * r + 3] = r < 30 ? (float)r : (float)((r * 1021u) & ((1u << 22) - 1));
    }
    src[4 * 31 + 3] = (float)((1u << 22) - 1);
    Dst d(n);
    late::copy_tag_rows(d.p, src.data(), 0, n, tag);
    for (size_t r = 0; r < n; ++r) {
      CHECK(bits(d.p[4 * r]) == bits(src[4 * r]) && bits(d.p[4 * r + 1]) == bits(src[4 * r + 1]) && bits(d.p[4 * r + 2]) == bits(src[4 * r + 2]));
      CHECK((bits(d.p[4 * r + 3]) & late::TAG_MASK) == tag);
      CHECK(bits(late::untag(d.p[4 * r + 3])) == bits(src[4 * r + 3]));
    }
    CHECK(d.guards_intact());
  }
}

static void boundary_floats() {
  // the fourth element at the edges: zeros, the first integers that need the two low bits (2^22 + 1, 2^23 - 1, 2^24 - 1), non-integers
  // with a full mantissa, denormals, infinities: the first three elements pass untouched, the fourth loses its two low mantissa bits
  // and nothing else (toward zero, at most 3 ulp)
  const float w[] = {0.0f, -0.0f, 1.0f, 29.0f, (float)(1u << 22), (float)((1u << 22) + 1), (float)((1u << 23) - 1), (float)((1u << 24) - 1),
                     0.1f, 12.3f, 28.999998f, from_bits(0x00000003u), from_bits(0x00000001u), INFINITY, -INFINITY, from_bits(0x3f7fffffu), -5.7f};
  const size_t n = sizeof w / sizeof w[0];
  std::vector<float> src(4 * n);
  for (size_t r = 0; r < n; ++r) { src[4 * r] = from_bits(0xffffffffu - (uint32_t)r); src[4 * r + 1] = 0.3f; src[4 * r + 2] = from_bits(0x7fc00001u); src[4 * r + 3] = w[r]; }
  for (uint32_t tag = 1; tag <= 2; ++tag) {
    Dst d(n);
    late::copy_tag_rows(d.p, src.data(), 0, n, tag);
    for (size_t r = 0; r < n; ++r) {
      for (int k = 0; k < 3; ++k) CHECK(bits(d.p[4 * r + k]) == bits(src[4 * r + k]));
      CHECK((bits(d.p[4 * r + 3]) & late::TAG_MASK) == tag);
      const uint32_t got = bits(late::untag(d.p[4 * r + 3])), was = bits(w[r]);
      CHECK(got == (was & ~late::TAG_MASK));
      CHECK(was - got <= 3u);                                   // (sign-magnitude: fewer bits = toward zero)
      if ((was & late::TAG_MASK) == 0) CHECK(got == was);
    }
    CHECK(d.guards_intact());
  }
  CHECK(late::untag(from_bits(bits((float)((1u << 22) + 1)) | 2u)) == (float)(1u << 22));
}

static void tag_alternation() {
  // 1, 2, 1, 2 ... per set, each set on its own; what a set holds from its previous use never carries the tag of the next
  uint32_t tag[3] = {0, 0, 0};
  const int uses[] = {0, 0, 1, 0, 2, 2, 2, 1, 0, 1};
  uint32_t want[3] = {1, 1, 1};
  for (int u : uses) {
    const uint32_t prev = tag[u];
    tag[u] = late::next_tag(tag[u]);
    CHECK(tag[u] == want[u]);
    CHECK(tag[u] != prev && (tag[u] == 1 || tag[u] == 2));
    want[u] = want[u] == 1 ? 2 : 1;
  }
  // a set zeroed at allocation matches neither tag
  CHECK((bits(0.0f) & late::TAG_MASK) != 1 && (bits(0.0f) & late::TAG_MASK) != 2);
  // old rows against the new tag, row by row, while a copy is half done
  const size_t n = 37;
  std::vector<float> a(4 * n, 5.0f), b(4 * n, 6.0f);
  Dst d(n);
  late::copy_tag_rows(d.p, a.data(), 0, n, 1);
  late::copy_tag_rows(d.p, b.data(), 0, 20, 2);
  for (size_t r = 0; r < n; ++r) {
    const bool fresh = (bits(d.p[4 * r + 3]) & late::TAG_MASK) == 2;
    CHECK(fresh == (r < 20));
    CHECK(late::untag(d.p[4 * r + 3]) == (fresh ? 6.0f : 5.0f) && d.p[4 * r] == (fresh ? 6.0f : 5.0f));
  }
}

static void alignment_and_odd_sizes() {
  // sources at every 4-byte offset of a 16-byte line, row counts that are odd / prime / zero / one, and every split of the batch in
  // two calls the way the step makes it (rows_before); the guard rows around the destination stay untouched
  const size_t sizes[] = {0, 1, 2, 3, 5, 7, 16, 63, 64, 65, 80, 127, 1001};
  const double fractions[] = {0.0, 0.25, 0.5, 0.75, 1.0 / 3.0, 1.0};
  for (size_t n : sizes)
    for (int off = 0; off < 4; ++off)
      for (int k = 0; k < 12; ++k) {
        const double f = fractions[k % 6];
        const bool odd = k >= 6;
        std::vector<float> store(4 * n + 8);
        float* src = store.data() + off;                       // (vector storage is 16-byte aligned: off = 1 .. 3 is misaligned for a 16-byte load)
        for (size_t i = 0; i < 4 * n; ++i) src[i] = (float)(i % 29);
        Dst d(n, odd);
        CHECK((((uintptr_t)d.p & 31u) == 0) == !odd);
        const size_t nb = late::rows_before(n, f);
        CHECK(nb <= n);
        if (f == 0.0) CHECK(nb == n);
        if (f == 1.0) CHECK(nb == 0);
        late::copy_tag_rows(d.p, src, 0, nb, 2);
        late::copy_tag_rows(d.p, src, nb, n, 2);
        for (size_t r = 0; r < n; ++r) {
          for (int k = 0; k < 3; ++k) CHECK(d.p[4 * r + k] == src[4 * r + k]);
          CHECK((bits(d.p[4 * r + 3]) & late::TAG_MASK) == 2 && late::untag(d.p[4 * r + 3]) == src[4 * r + 3]);
        }
        CHECK(d.guards_intact());
        CHECK(((uintptr_t)d.p & 15u) == 0);
      }
  CHECK(late::rows_before(8192, 0.5) == 4096 && late::rows_before(8192, -1.0) == 8192 && late::rows_before(8192, 2.0) == 0);
  CHECK(late::rows_before(7, NAN) == 7);
}

int main() {
  round_trip_integers();
  boundary_floats();
  tag_alternation();
  alignment_and_odd_sizes();
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("late actions host checks ok\n");
  return 0;
}
