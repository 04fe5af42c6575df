/* A stand-in for ac_step_host_actions_begin / _wait with no GPU behind it (tests/test_native_step_host.py): it records what it was
 * called with, and "steps" by writing the step's number into the first observation of the set it was given. */
#include <stdint.h>
#include <stddef.h>
#include <time.h>

#define STUB_SETS 8

typedef struct {
  float* obs[STUB_SETS];        /* where the "kernel" writes, per set */
  int32_t begin_calls, wait_calls;
  int32_t last_set;
  const float* last_actions;
  size_t last_n;
  double first, last, sum;      /* of the batch, read inside begin: the array must be alive and complete there */
  int32_t begin_rc, wait_rc;    /* what the two calls return */
  int32_t wait_ms;              /* how long the wait sleeps */
  double wait_t0, wait_t1;      /* CLOCK_MONOTONIC around the sleep */
  void* last_handle;
} stub_t;

static stub_t g;

static double now_s(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

stub_t* stub_state(void) { return &g; }

int stub_begin(void* h, int32_t set, const float* actions, size_t n) {
  g.begin_calls += 1;
  g.last_handle = h;
  g.last_set = set;
  g.last_actions = actions;
  g.last_n = n;
  g.sum = 0.0;
  for (size_t i = 0; i < n; ++i) g.sum += actions[i];
  g.first = n ? actions[0] : 0.0;
  g.last = n ? actions[n - 1] : 0.0;
  return g.begin_rc;
}

int stub_wait(void* h) {
  g.wait_calls += 1;
  g.last_handle = h;
  g.wait_t0 = now_s();
  if (g.wait_ms > 0) {
    struct timespec d = {g.wait_ms / 1000, (long)(g.wait_ms % 1000) * 1000000L};
    nanosleep(&d, NULL);
  }
  g.wait_t1 = now_s();
  if (g.last_set >= 0 && g.last_set < STUB_SETS && g.obs[g.last_set]) g.obs[g.last_set][0] = (float)g.begin_calls;
  return g.wait_rc;
}
