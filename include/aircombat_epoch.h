/* aircombat_epoch.h -- C ABI of the stream-ordered hand-over from the rollout buffer to the PPO update: returns, advantages and a whole
 * epoch's mini-batches queued on the caller's stream, with no host wait.
 *
 * The calls of aircombat_buffer.h block: each ends with a wait for the buffer's own stream, so that host sources may be reused and
 * the results read at once. The calls below do the same device work for a caller that keeps everything on one stream (torch's
 * current stream): they queue on `caller` (a hipStream_t; NULL is the device's default stream) and return without waiting for the
 * device. Same library as aircombat.h (libaircombat_hip.so), same errors: 0 on success, -1 on failure with the message in
 * ac_last_error(). One caller thread per handle.
 *
 * Streams. On entry `caller` is made to wait for an event recorded on the buffer's own stream, so everything the blocking calls and
 * the collectors have queued there comes first; on return the buffer's stream is made to wait for an event recorded on `caller`, so
 * a later blocking call (insert, after_update, read, mini-batch) is ordered after the work queued here. The two events are created
 * once per buffer handle; nothing is waited for on the host. Refused by every call, with nothing queued: a NULL handle, and a buffer on
 * another device than the one `caller` belongs to (for a NULL `caller`: the calling thread's current device).
 */
#ifndef AIRCOMBAT_EPOCH_H
#define AIRCOMBAT_EPOCH_H
#include <stdint.h>
#include "aircombat_buffer.h"
#ifdef __cplusplus
extern "C" {
#endif

/* fields of a mini-batch in the order of ac_buffer_batch_t's members */
enum {
  AC_EPOCH_OBS = 0, AC_EPOCH_SHARE_OBS, AC_EPOCH_ACTIONS, AC_EPOCH_MASKS, AC_EPOCH_ACTIVE_MASKS, AC_EPOCH_LOGP, AC_EPOCH_ADVANTAGES,
  AC_EPOCH_RETURNS, AC_EPOCH_VALUES, AC_EPOCH_RNN_ACTOR, AC_EPOCH_RNN_CRITIC, AC_EPOCH_NFIELDS
};

/* ac_buffer_compute_returns with a device pointer, on `caller`: the same device-to-device put of next_value ([N] floats, read when
 * the stream gets there: it must stay valid until then) and the same kernel with the same grid. The kernel time that
 * ac_buffer_last_kernel_ms reports is neither updated nor waited for. */
int ac_buffer_compute_returns_on(ac_buffer_t* b, void* caller, const float* d_next_value);
/* ac_buffer_advantages on `caller`: the same three kernels into AC_BUF_ADVANTAGES */
int ac_buffer_advantages_on(ac_buffer_t* b, void* caller);

/* Where an epoch of n_minibatch mini-batches of mb chunks of chunk_len steps lies in ONE flat float array (host only, nothing is
 * queued). Field f of mini-batch i starts at float  offsets[f] + i * rows_f * dim_f,  rows_f = chunk_len * mb (mb for the two RNN
 * fields, one row per chunk), in the row order of a mini-batch of ac_buffer_minibatch: row l * mb + j = step l of chunk j.
 * offsets[f] is a multiple of 4 floats, or -1 for a field this buffer lacks (share_obs, active_masks without share_obs_dim);
 * *total_floats is the array's length: the fields' sizes, each padded to a multiple of 4 floats. The _for form takes the
 * constructor's arguments instead of a handle. Refused: a NULL argument, non-positive sizes,
 * n_minibatch * mb * chunk_len > T * N. */
int ac_buffer_epoch_layout(const ac_buffer_t* b, int32_t n_minibatch, int32_t mb, int32_t chunk_len, int64_t offsets[AC_EPOCH_NFIELDS],
                           int64_t* total_floats);
int ac_buffer_epoch_layout_for(const ac_buffer_config_t* cfg, int32_t n_minibatch, int32_t mb, int32_t chunk_len,
                               int64_t offsets[AC_EPOCH_NFIELDS], int64_t* total_floats);

/* One launch fills every field of every mini-batch of an epoch in d_out (device, total_floats floats, laid out as above). d_order is
 * a device int32 array of n_minibatch * mb chunk indices, read when the stream gets there; mini-batch i takes
 * d_order[i * mb : (i + 1) * mb]; chunk c covers rows [c * chunk_len, (c + 1) * chunk_len) of the column-major sequence view, as in
 * ac_buffer_minibatch. Refused on the host with nothing queued: a NULL argument, non-positive sizes,
 * n_minibatch * mb * chunk_len > T * N, a buffer on another device than `caller`'s.
 * The chunk indices cannot be checked without a wait, so the kernel clamps every index into [0, T * N / chunk_len - 1] before it is
 * used: whatever d_order holds, nothing outside the buffer's arrays is read. That is a memory-safety rule and no validation
 * service: an index out of range silently yields the rows of the first or last chunk. Check the order where it is made. */
int ac_buffer_gather_epoch(ac_buffer_t* b, void* caller, const int32_t* d_order, int32_t n_minibatch, int32_t mb, int32_t chunk_len,
                           float* d_out);

/* The kernel's row function on the host (no GPU, no handle): the source row  t * N + col  of step l of chunk `chunk` in a buffer of
 * T steps and N columns, with the clamp above applied to `chunk`; -1 for non-positive sizes, chunk_len > T * N or l outside
 * [0, chunk_len). */
int64_t ac_buffer_epoch_source_row_host(int32_t chunk, int32_t l, int32_t chunk_len, int32_t T, int32_t N);

/* ---- The list form: mini-batches cut from K buffers of one shape, as ReplayBuffer.recurrent_generator does for a list of buffers
 * (algorithms/utils/buffer.py:183-214). The buffers' column-major sequence views are stacked in the order of `bufs`: row R of the stack
 * is row R % (T * N) of buffer R / (T * N). Chunk c covers rows [c * chunk_len, (c + 1) * chunk_len) of the stack, so that a chunk may
 * straddle two columns and, where chunk_len does not divide T * N, two buffers; the RNN fields take the row of the chunk's first step,
 * from the buffer that row lies in. One permutation over the K * T * N / chunk_len chunks then mixes rows of every buffer in every
 * mini-batch. The advantages are each buffer's own (normalised per buffer, as the reference normalises them): queue them per handle
 * before the gather. The single-handle calls above are untouched by these; K = 1 gives what they give.
 *
 * Refused by every call below that takes `bufs`, with the cause named and nothing queued: a NULL `bufs` or handle, K outside
 * 1 .. AC_EPOCH_MAX_BUFFERS, the same handle twice, buffers that differ in buffer_size, n_envs, n_agents, a field's width or in
 * being shared (share_obs_dim > 0) or not, buffers on different devices, and (the gather) on another device than `caller`'s. */
#define AC_EPOCH_MAX_BUFFERS 8

/* The single form's layout rules over the stack's K * T * N rows. Refused as well: a NULL argument, non-positive sizes,
 * n_minibatch * mb > K * T * N / chunk_len, a stack of more than 2^31 - 1 chunks. */
int ac_buffers_epoch_layout(ac_buffer_t* const* bufs, int32_t K, int32_t n_minibatch, int32_t mb, int32_t chunk_len,
                            int64_t offsets[AC_EPOCH_NFIELDS], int64_t* total_floats);

/* One launch on `caller` for every field of every mini-batch of an epoch over the stack, into d_out as laid out above; d_order as in
 * the single form, its indices clamped into [0, K * T * N / chunk_len - 1] before use (memory safety, not validation). On entry
 * `caller` is made to wait for every buffer's own stream, on return every buffer's stream for `caller`; nothing is waited for on the
 * host. */
int ac_buffers_gather_epoch(ac_buffer_t* const* bufs, int32_t K, void* caller, const int32_t* d_order, int32_t n_minibatch, int32_t mb,
                            int32_t chunk_len, float* d_out);

/* The blocking form: one mini-batch of n_chunks chunks of the stack (host indices, checked: one outside the stack is refused) into the
 * arrays of `batch` (NULL members are skipped), host arrays or with on_device device arrays. It waits for every buffer's stream, runs
 * the same kernel on the first buffer's and returns when the arrays are complete. */
int ac_buffers_minibatch(ac_buffer_t* const* bufs, int32_t K, const int32_t* chunks, int32_t n_chunks, int32_t chunk_len,
                         const ac_buffer_batch_t* batch, int on_device);

/* The list kernel's row function on the host (no GPU, no handle): step l of chunk `chunk` of a stack of K buffers of T steps and N
 * columns lies in buffer *k at time-major source row *row = t * N + col, with the clamp applied to `chunk`. -1 for a NULL pointer,
 * non-positive sizes, K outside 1 .. AC_EPOCH_MAX_BUFFERS, chunk_len > K * T * N or l outside [0, chunk_len). */
int ac_buffers_epoch_source_host(int32_t chunk, int32_t l, int32_t chunk_len, int32_t T, int32_t N, int32_t K, int32_t* k, int64_t* row);

#ifdef __cplusplus
}
#endif
#endif
