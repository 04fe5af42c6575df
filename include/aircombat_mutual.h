/* aircombat_mutual.h -- C ABI of the mutual-support discriminator on the device: the intrinsic rewards of a whole rollout in one
 * launch, and the gather of its training mini-batches.
 *
 * The reference's Discriminator (R/algorithms/utils/discriminator.py, R = the reference repository) holds two three-layer nets,
 *   pred     Linear(128 + 2 C, 256) - ReLU - Linear(256, 256) - ReLU - Linear(256, D)
 *   pred_wo  Linear(128 + C, 256)   - ReLU - Linear(256, 256) - ReLU - Linear(256, D)
 * that predict an agent's next observation from agent 0's actor state and the actions of agents 0 and 1, with and without the
 * partner's action. Same library as aircombat.h (libaircombat_hip.so), same errors: 0 on success, -1 on failure with the message in
 * ac_last_error().
 *
 * The arrays are those of a shared rollout buffer (aircombat_buffer.h) with N = E * na columns in (env, agent) order and T steps:
 * OBS [T + 1][N][obs_dim], ACTIONS [T][N][act_dim], REWARDS [T][N], RNN_ACTOR [T + 1][N][128]. For step s and env e, with rows
 * r0 = e * na and r1 = e * na + 1:
 *   h = RNN_ACTOR[s][r0] (agent 0's actor state entering step s), a0 = ACTIONS[s][r0], a1 = ACTIONS[s][r1],
 *   tuple 0:  x = [h, a0, a1], target y = OBS[s + 1][r0];    tuple 1:  x = [h, a1, a0], target y = OBS[s + 1][r1]
 *   mse_with(j) = mean_d (pred(x_j) - y_j)^2,   mse_wo(j) = mean_d (pred_wo(first 128 + C columns of x_j) - y_j)^2
 *   score(j) = mse_wo(j) - mse_with(j);   r_int of agent 1 = score(0), of agent 0 = score(1), of agents >= 2: 0.
 * Accepted: act_dim 1 .. 12, obs_dim 1 .. 128, hidden 128, na >= 2, E >= 1. Everything else is refused with a message naming the value.
 * The weights are row-major [out][in] float32 (torch's parameter storage), read in place.
 */
#ifndef AIRCOMBAT_MUTUAL_H
#define AIRCOMBAT_MUTUAL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { AC_MI_HIDDEN = 128, AC_MI_WIDTH = 256, AC_MI_MAX_ACT = 12, AC_MI_MAX_OBS = 128 };

/* The scorer's arguments. Steps [s0, s0 + n) are scored: 0 <= s0, n >= 1, s0 + n <= T.
 * r_int [n][E][2] (may be NULL): entry [.][e][a] is the intrinsic reward of agent a. mse [n][E][2][2] (may be NULL): entry
 * [.][e][j][0] = mse_with(j), [.][e][j][1] = mse_wo(j). With add != 0, REWARDS[s][e * na + a] += ratio * r_int for a = 0, 1 (REWARDS
 * may be NULL otherwise); every (s, e, a) is written by one thread, once. */
typedef struct {
  int32_t E, na, T, obs_dim, act_dim, hidden, s0, n, add;
  float ratio;
  const float *OBS, *ACTIONS, *RNN_ACTOR;
  float* REWARDS;
  /* pred: layers.0, layers.1, last_fc; then pred_wo */
  const float *p_w0, *p_b0, *p_w1, *p_b1, *p_w2, *p_b2;
  const float *q_w0, *q_b0, *q_w1, *q_b1, *q_w2, *q_b2;
  float *r_int, *mse;
} ac_mi_score_t;

/* One launch on `stream` (a hipStream_t of the current device; NULL: its default stream), nothing waited for on the host. Every
 * pointer is device memory. Products and sums are float32 (v_mfma_f32_16x16x4_f32), no floating-point atomics: the results are
 * bit-identical from run to run. */
int ac_mi_score(const ac_mi_score_t* args, void* stream);
/* The same rule on host arrays (no GPU), float32 with every sum in plain index order. */
int ac_mi_score_host(const ac_mi_score_t* args);

/* The gather of one training mini-batch: for time indices times[0 .. m) it writes X [2 m E][128 + 2 C] and Y [2 m E][obs_dim]; row
 * (j * m + i) * E + e is tuple j of env e at step times[i]. It only copies. The device form reads `times` (device int32) when the
 * stream gets there and clamps every index into [0, T - 1]: memory safety, not validation. The host form refuses an index outside
 * that range. */
typedef struct {
  int32_t E, na, T, obs_dim, act_dim, hidden, m, pad_;
  const float *OBS, *ACTIONS, *RNN_ACTOR;
  const int32_t* times;
  float *X, *Y;
} ac_mi_gather_t;
int ac_mi_gather(const ac_mi_gather_t* args, void* stream);
int ac_mi_gather_host(const ac_mi_gather_t* args);

#ifdef __cplusplus
}
#endif
#endif
