// Stream-ordered hand-over from the rollout buffer to the PPO update (include/aircombat_epoch.h): compute_returns, the advantages
// and a whole epoch's mini-batches queued on the caller's stream, no host wait. Included after rollout_buffer.hpp (same library, same
// error channel); the returns and advantage launches are rollout_buffer.hpp's own helpers on another stream.
//
// epoch_gather_kernel: one launch per epoch instead of one gather_rows_kernel per field and mini-batch.
//   * An epoch's per-step fields are ONE run of G = n_minibatch * L * mb output rows each: mini-batch i's rows follow mini-batch
//     i - 1's, so output row g of field f lies at offsets[f] + g * dim_f. A workgroup takes ROWS consecutive rows g and, for each of
//     them ONCE, works out its source row (mini-batch, step, chunk -> d_order -> clamp -> column, time) into LDS; every field of the
//     tile then reads that table. The RNN states (one row per chunk) are tiles of their own over the n_minibatch * mb chunks.
//   * A field's part of a tile is contiguous in the output, so the threads sweep it in access units (a float, or a float4 where the
//     field's rows are 16-byte multiples and the output base is 16-byte aligned) with consecutive lanes on consecutive units: stores
//     are fully coalesced; loads are coalesced inside a source row and scattered between rows.
//   * unit -> (row of the tile, unit of the row) is a multiply-high by a reciprocal the host worked out, not a division.
// What bounds it: the scattered source rows. The arrays are time-major, adjacent output rows are different chunks, so every
// source row is fetched on its own: a scalar field (masks, advantages, returns, value_preds, PPO's log-probability) uses 4 bytes of
// each cache line it pulls in, and the L steps of one chunk are N * dim floats apart. The kernel is bound by the number of cache
// lines touched, not by the bytes it delivers ("Stream-ordered training data").
#pragma once
#include "../../include/aircombat_epoch.h"

namespace epoch {
constexpr int ROWS = 64, NT = 256, UNROLL = 4;

struct Field {
  const float* src;        // the buffer's array, time-major [slots][N][dim]; NULL: the buffer lacks the field
  int64_t out;             // offset of the field in the flat output, in floats
  uint32_t units;          // access units per row: dim, or dim / 4 with vec
  uint32_t magic;          // floor(2^32 / units) + 1; 0: units == 1, or too wide for the multiply-high (plain division then)
  int32_t vec;             // 1: float4 accesses
  int32_t first_only;      // 1: one row per chunk (its first step): the RNN states
};
struct Table { Field f[AC_EPOCH_NFIELDS]; };

// Memory safety, not validation: whatever the device array holds, the index used lies in [0, n_chunks - 1]
__host__ __device__ __forceinline__ int64_t clamp_chunk(int32_t chunk, int64_t n_chunks) {
  const int64_t c = chunk;
  return c < 0 ? 0 : (c >= n_chunks ? n_chunks - 1 : c);
}
// step l of chunk `chunk`: row = chunk * L + l of the column-major sequence view (buffer.py:33-34) -> time-major source row t * N + col.
// With chunk < T * N / L and l < L: row < T * N, so col < N and the result < T * N <= slots * N for every field.
__host__ __device__ __forceinline__ int64_t source_row(int32_t chunk, int l, int L, int T, int N) {
  const int64_t n_chunks = ((int64_t)T * N) / L;
  const int64_t row = clamp_chunk(chunk, n_chunks) * L + l;
  const int64_t col = row / T, t = row % T;
  return t * N + col;
}
// e / units for e < ROWS * units. With m = floor(2^32 / units) + 1, m * units = 2^32 + d, 0 < d <= units, and
// floor(e * m / 2^32) = floor(e / units + e * d / (units * 2^32)) = floor(e / units) as long as e * d < 2^32, which
// e * units < 2^32 guarantees: the host sets magic only where ROWS * units * units < 2^32.
__host__ __device__ __forceinline__ uint32_t unit_row(uint32_t e, uint32_t units, uint32_t magic) {
#if defined(__HIP_DEVICE_COMPILE__)
  return magic ? __umulhi(e, magic) : (units == 1 ? e : e / units);
#else
  return magic ? (uint32_t)(((uint64_t)e * magic) >> 32) : (units == 1 ? e : e / units);
#endif
}
static uint32_t magic_of(uint32_t units) {
  if (units < 2 || (uint64_t)ROWS * units * units >= (1ull << 32)) return 0;
  return (uint32_t)((1ull << 32) / units) + 1u;
}

template <class V>
__device__ __forceinline__ void copy_field(const Field& F, float* __restrict__ out, const int64_t* s_src, int64_t first_row, int rows) {
  const V* __restrict__ src = reinterpret_cast<const V*>(F.src);
  V* __restrict__ dst = reinterpret_cast<V*>(out + F.out) + first_row * (int64_t)F.units;
  const uint32_t total = (uint32_t)rows * F.units;
  for (uint32_t e0 = threadIdx.x; e0 < total; e0 += UNROLL * NT) {
    V v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {      // the loads of a pass are independent: all in flight before the first store
      // past the tile's end the last unit is read again (a valid address, never stored): every v[u] is assigned, so the array
      // stays in registers
      const uint32_t e = min(e0 + u * NT, total - 1);
      const uint32_t rr = unit_row(e, F.units, F.magic);
      v[u] = src[s_src[rr] * (int64_t)F.units + (e - rr * F.units)];
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const uint32_t e = e0 + u * NT;
      if (e < total) dst[e] = v[u];
    }
  }
}

// grid = step tiles (ceil(n_mb * L * mb / ROWS)) followed by RNN tiles (ceil(n_mb * mb / ROWS))
__global__ __launch_bounds__(NT) void epoch_gather_kernel(const Table tab, float* __restrict__ out, const int32_t* __restrict__ order,
                                                          int n_mb, int mb, int L, int T, int N, int step_tiles) {
  __shared__ int64_t s_src[ROWS];
  const bool rnn = (int)blockIdx.x >= step_tiles;
  const int64_t total_rows = rnn ? (int64_t)n_mb * mb : (int64_t)n_mb * mb * L;
  const int64_t first_row = (int64_t)(rnn ? blockIdx.x - step_tiles : blockIdx.x) * ROWS;
  const int rows = (int)(total_rows - first_row < ROWS ? total_rows - first_row : ROWS);
  if ((int)threadIdx.x < rows) {
    const int64_t g = first_row + threadIdx.x;
    int64_t q = g;            // index into `order`: i * mb + j
    int l = 0;
    if (!rnn) {
      const int64_t per_mb = (int64_t)L * mb, i = g / per_mb, r = g % per_mb;
      l = (int)(r / mb);
      q = i * mb + r % mb;
    }
    s_src[threadIdx.x] = source_row(order[q], l, L, T, N);
  }
  __syncthreads();
#pragma unroll 1      // one copy of the two sweeps, the field's entry read from the kernel arguments with a uniform index
  for (int k = 0; k < AC_EPOCH_NFIELDS; ++k) {
    const Field& F = tab.f[k];
    if (!F.src || (F.first_only != 0) != rnn) continue;
    if (F.vec) copy_field<float4>(F, out, s_src, first_row, rows);
    else copy_field<float>(F, out, s_src, first_row, rows);
  }
}
}  // namespace epoch

// buffer field of each mini-batch field, in the order of ac_buffer_batch_t
static const int kEpochField[AC_EPOCH_NFIELDS] = {AC_BUF_OBS, AC_BUF_SHARE_OBS, AC_BUF_ACTIONS, AC_BUF_MASKS, AC_BUF_ACTIVE_MASKS, AC_BUF_LOGP,
                                                  AC_BUF_ADVANTAGES, AC_BUF_RETURNS, AC_BUF_VALUES, AC_BUF_RNN_ACTOR, AC_BUF_RNN_CRITIC};

static int epoch_sizes_ok(const char* fn, int64_t T, int64_t N, int32_t n_mb, int32_t mb, int32_t L) {
  if (n_mb <= 0 || mb <= 0 || L <= 0) return fail(std::string(fn) + ": n_minibatch, mb and chunk_len must be positive");
  if ((int64_t)n_mb * mb > (T * N) / L)    // n_minibatch * mb * chunk_len > T * N, without the product's overflow
    return fail(std::string(fn) + ": n_minibatch * mb * chunk_len exceeds the buffer's T * N rows");
  return 0;
}

// dims of the mini-batch fields from the constructor's arguments (0: the buffer lacks the field), as ac_buffer_create lays them out
static void epoch_dims(const ac_buffer_config_t& c, int dim[AC_EPOCH_NFIELDS]) {
  const int hid = c.hidden_layers * c.hidden_size, shared = c.share_obs_dim > 0;
  const int d[AC_EPOCH_NFIELDS] = {c.obs_dim, c.share_obs_dim, c.act_dim, 1, shared ? 1 : 0, c.logp_dim, 1, 1, 1, hid, hid};
  for (int k = 0; k < AC_EPOCH_NFIELDS; ++k) dim[k] = d[k];
}

static int epoch_layout(const char* fn, const ac_buffer_config_t* cfg, int32_t n_mb, int32_t mb, int32_t L, int64_t* offsets, int64_t* total) {
  if (!cfg || !offsets || !total) return fail(std::string(fn) + ": null argument");
  if (cfg->buffer_size <= 0 || cfg->n_envs <= 0 || cfg->n_agents <= 0 || cfg->obs_dim <= 0 || cfg->act_dim <= 0 || cfg->logp_dim <= 0 ||
      cfg->share_obs_dim < 0 || cfg->hidden_layers <= 0 || cfg->hidden_size <= 0)
    return fail(std::string(fn) + ": the buffer's sizes must be positive (share_obs_dim may be 0)");
  if (epoch_sizes_ok(fn, cfg->buffer_size, (int64_t)cfg->n_envs * cfg->n_agents, n_mb, mb, L)) return -1;
  int dim[AC_EPOCH_NFIELDS];
  epoch_dims(*cfg, dim);
  int64_t at = 0;
  for (int k = 0; k < AC_EPOCH_NFIELDS; ++k) {
    if (dim[k] <= 0) { offsets[k] = -1; continue; }
    const bool first_only = k == AC_EPOCH_RNN_ACTOR || k == AC_EPOCH_RNN_CRITIC;
    const int64_t n = (int64_t)n_mb * mb * (first_only ? 1 : L) * dim[k];
    offsets[k] = at;
    at += (n + 3) / 4 * 4;
  }
  *total = at;
  return 0;
}

// the refusals every stream-ordered call shares, then the entry ordering: `caller` after the buffer's own stream
static int epoch_enter(const char* fn, ac_buffer* b, hipStream_t caller) {
  int dev = -1;
  if (caller) {
    hipDevice_t d;
    if (hipStreamGetDevice(caller, &d) != hipSuccess) return fail(std::string(fn) + ": the caller's stream is not a stream of any device");
    dev = (int)d;
  } else if (hipGetDevice(&dev) != hipSuccess) {
    return fail(std::string(fn) + ": no current HIP device");
  }
  if (dev != b->device) return fail(std::string(fn) + ": the buffer is on another device than the caller's stream");
  HIP_OK(hipSetDevice(b->device));
  HIP_OK(hipEventRecord(b->ev_in, b->stream));
  HIP_OK(hipStreamWaitEvent(caller, b->ev_in, 0));
  return 0;
}
// the exit ordering: the buffer's own stream after what was queued on `caller`. Queued whether the launches succeeded or not.
static int epoch_leave(const char* fn, ac_buffer* b, hipStream_t caller, int rc) {
  const hipError_t e0 = hipEventRecord(b->ev_out, caller);
  const hipError_t e1 = e0 == hipSuccess ? hipStreamWaitEvent(b->stream, b->ev_out, 0) : e0;
  if (rc) return rc;    // (the launch's own message stays in ac_last_error)
  if (e1 != hipSuccess) return fail(std::string(fn) + ": ordering after the launches: " + hipGetErrorString(e1));
  return 0;
}

extern "C" {

int ac_buffer_compute_returns_on(ac_buffer_t* b, void* caller, const float* d_next_value) {
  const char* fn = "ac_buffer_compute_returns_on";
  if (!b || !d_next_value) return fail(std::string(fn) + ": null argument");
  hipStream_t s = (hipStream_t)caller;
  if (epoch_enter(fn, b, s)) return -1;
  int rc = buf_put_next_value(b, d_next_value, 1, s);
  if (!rc) rc = buf_launch_returns(b, s);
  return epoch_leave(fn, b, s, rc);
}

int ac_buffer_advantages_on(ac_buffer_t* b, void* caller) {
  const char* fn = "ac_buffer_advantages_on";
  if (!b) return fail(std::string(fn) + ": null handle");
  hipStream_t s = (hipStream_t)caller;
  if (epoch_enter(fn, b, s)) return -1;
  return epoch_leave(fn, b, s, buf_launch_advantages(b, s));
}

int ac_buffer_epoch_layout_for(const ac_buffer_config_t* cfg, int32_t n_minibatch, int32_t mb, int32_t chunk_len, int64_t* offsets, int64_t* total_floats) {
  return epoch_layout("ac_buffer_epoch_layout_for", cfg, n_minibatch, mb, chunk_len, offsets, total_floats);
}

int ac_buffer_epoch_layout(const ac_buffer_t* b, int32_t n_minibatch, int32_t mb, int32_t chunk_len, int64_t* offsets, int64_t* total_floats) {
  if (!b) return fail("ac_buffer_epoch_layout: null argument");
  return epoch_layout("ac_buffer_epoch_layout", &b->cfg, n_minibatch, mb, chunk_len, offsets, total_floats);
}

int ac_buffer_gather_epoch(ac_buffer_t* b, void* caller, const int32_t* d_order, int32_t n_minibatch, int32_t mb, int32_t chunk_len, float* d_out) {
  const char* fn = "ac_buffer_gather_epoch";
  if (!b || !d_order || !d_out) return fail(std::string(fn) + ": null argument");
  int64_t offsets[AC_EPOCH_NFIELDS], total = 0;
  if (epoch_layout(fn, &b->cfg, n_minibatch, mb, chunk_len, offsets, &total)) return -1;
  epoch::Table tab;
  memset(&tab, 0, sizeof tab);
  const bool out_aligned = ((uintptr_t)d_out & 15) == 0;
  for (int k = 0; k < AC_EPOCH_NFIELDS; ++k) {
    const int fld = kEpochField[k];
    if (offsets[k] < 0 || !b->f[fld]) continue;
    epoch::Field& F = tab.f[k];
    const int dim = b->dim[fld];
    // 16-byte accesses only where every address is a 16-byte multiple: the arrays come from hipMalloc (256-byte aligned) and a row
    // starts at row * dim floats; the field's output starts at a multiple of 4 floats and a row at g * dim floats behind it
    F.vec = dim % 4 == 0 && out_aligned && ((uintptr_t)b->f[fld] & 15) == 0;
    F.src = b->f[fld];
    F.out = offsets[k];
    F.units = (uint32_t)(F.vec ? dim / 4 : dim);
    F.magic = epoch::magic_of(F.units);
    F.first_only = k == AC_EPOCH_RNN_ACTOR || k == AC_EPOCH_RNN_CRITIC;
  }
  const int64_t chunks = (int64_t)n_minibatch * mb;
  const int64_t step_tiles = (chunks * chunk_len + epoch::ROWS - 1) / epoch::ROWS, rnn_tiles = (chunks + epoch::ROWS - 1) / epoch::ROWS;
  if (step_tiles + rnn_tiles > 0x7fffffff) return fail(std::string(fn) + ": too many rows for one launch");
  hipStream_t s = (hipStream_t)caller;
  if (epoch_enter(fn, b, s)) return -1;
  hipLaunchKernelGGL(epoch::epoch_gather_kernel, dim3((unsigned)(step_tiles + rnn_tiles)), dim3(epoch::NT), 0, s, tab, d_out, d_order, n_minibatch, mb,
                     chunk_len, b->T, b->N, (int)step_tiles);
  const hipError_t e = hipGetLastError();
  const int rc = e == hipSuccess ? 0 : fail(std::string(fn) + ": " + hipGetErrorString(e));
  return epoch_leave(fn, b, s, rc);
}

int64_t ac_buffer_epoch_source_row_host(int32_t chunk, int32_t l, int32_t chunk_len, int32_t T, int32_t N) {
  if (T <= 0 || N <= 0 || chunk_len <= 0 || (int64_t)chunk_len > (int64_t)T * N || l < 0 || l >= chunk_len)
    return fail("ac_buffer_epoch_source_row_host: T, N and chunk_len must be positive, chunk_len <= T * N and 0 <= l < chunk_len");
  return epoch::source_row(chunk, l, chunk_len, T, N);
}

}  // extern "C"
