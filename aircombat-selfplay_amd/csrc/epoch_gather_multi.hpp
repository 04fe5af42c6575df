// The list form of the stream-ordered hand-over (include/aircombat_epoch.h, ac_buffers_*): an epoch's mini-batches cut from K rollout
// buffers of equal shape, as ReplayBuffer.recurrent_generator does for a list of buffers (algorithms/utils/buffer.py:183-214): the
// buffers' column-major sequence views are stacked (np.vstack) and ONE chunk permutation runs over the stack, so a mini-batch mixes
// rows of every buffer. Included after epoch_gather.hpp, whose kernel and calls are left as they are: this file adds to them.
//
// epoch_gather_multi_kernel is epoch_gather_kernel with K sources per field:
//   * row R of the stack lies in buffer k = R / (T * N) at local row r = R % (T * N), i.e. column r / T, time r % T, time-major source
//     row t * N + col of buffer k. Chunk c covers rows [c * L, (c + 1) * L) of the stack, so a chunk may straddle a column edge and, where
//     L does not divide T * N, the edge between two buffers: step l's source is worked out on its own, and the RNN fields take the row
//     of step 0, from the buffer that row lies in.
//   * a workgroup works out the pair (buffer, source row) ONCE per output row of its tile into LDS, packed into one 64-bit word
//     (buffer in the top byte); every field of the tile reads that table, and the field's K base pointers from a second LDS table that
//     the workgroup copies from the kernel arguments when it starts (a per-lane index into the arguments themselves makes the compiler
//     copy the table per thread).
//   * the stores are the single form's: a field's part of a tile is contiguous in the output, consecutive lanes on consecutive access
//     units, float4 units only where the rows are 16-byte multiples and the output AND all K sources of the field are 16-byte aligned;
//     unit -> (row, unit of the row) is the same multiply-high.
// What bounds it is what bounds the single form: every source row is a fetch of its own ("Stream-ordered training data").
#pragma once
#include "epoch_gather.hpp"

namespace epoch {
constexpr int MAX_SRC = AC_EPOCH_MAX_BUFFERS;
constexpr int SRC_SHIFT = 56;                                  // (buffer << 56) | source row: a source row is below 2^31 * 2^31 / 2^8
constexpr int64_t ROW_MASK = ((int64_t)1 << SRC_SHIFT) - 1;

struct MultiField {
  float* dst;              // where the field's first mini-batch starts; NULL: not asked for, or the buffers lack the field
  uint32_t units;          // access units per row: dim, or dim / 4 with vec
  uint32_t magic;          // as Field::magic
  int32_t vec;             // 1: float4 accesses
  int32_t first_only;      // 1: one row per chunk (its first step): the RNN states
};
struct MultiTable {
  MultiField f[AC_EPOCH_NFIELDS];
  const float* src[AC_EPOCH_NFIELDS][MAX_SRC];     // field f of buffer k, time-major [slots][N][dim]; entries k >= K are never read
};

// step l of chunk `chunk` of a stack of K buffers of T steps and N columns: the pair (buffer, time-major source row) packed as above.
// With the clamp chunk < K * T * N / L, so R = chunk * L + l < K * T * N: k < K, r < T * N, col < N and the row < T * N.
__host__ __device__ __forceinline__ int64_t multi_source(int32_t chunk, int l, int L, int T, int N, int K) {
  const int64_t per = (int64_t)T * N, n_chunks = (per * K) / L;
  const int64_t R = clamp_chunk(chunk, n_chunks) * L + l;
  const int64_t k = R / per, r = R % per;
  const int64_t col = r / T, t = r % T;
  return (k << SRC_SHIFT) | (t * N + col);
}

template <class V>
__device__ __forceinline__ void copy_field_multi(const MultiField& F, const float* const* s_ptr, const int64_t* s_src, int64_t first_row, int rows) {
  V* __restrict__ dst = reinterpret_cast<V*>(F.dst) + first_row * (int64_t)F.units;
  const uint32_t total = (uint32_t)rows * F.units;
  // as copy_field: the loads of a pass are independent and all in flight before the first store; past the tile's end the last unit is
  // read again (a valid address, never stored). Named values and no array: an array of float4 here was seen placed in LDS.
  static_assert(UNROLL == 4, "four named values per pass");
  const auto load = [&](uint32_t at) -> V {
    const uint32_t e = min(at, total - 1);
    const uint32_t rr = unit_row(e, F.units, F.magic);
    const int64_t p = s_src[rr];
    const V* src = reinterpret_cast<const V*>(s_ptr[p >> SRC_SHIFT]);
    return src[(p & ROW_MASK) * (int64_t)F.units + (e - rr * F.units)];
  };
  for (uint32_t e0 = threadIdx.x; e0 < total; e0 += UNROLL * NT) {
    const V v0 = load(e0), v1 = load(e0 + NT), v2 = load(e0 + 2 * NT), v3 = load(e0 + 3 * NT);
    if (e0 < total) dst[e0] = v0;
    if (e0 + NT < total) dst[e0 + NT] = v1;
    if (e0 + 2 * NT < total) dst[e0 + 2 * NT] = v2;
    if (e0 + 3 * NT < total) dst[e0 + 3 * NT] = v3;
  }
}

// grid = step tiles (ceil(n_mb * L * mb / ROWS)) followed by RNN tiles (ceil(n_mb * mb / ROWS)), as epoch_gather_kernel
__global__ __launch_bounds__(NT) void epoch_gather_multi_kernel(const MultiTable tab, const int32_t* __restrict__ order, int n_mb, int mb, int L,
                                                                int T, int N, int K, int step_tiles) {
  __shared__ int64_t s_src[ROWS];
  __shared__ const float* s_ptr[AC_EPOCH_NFIELDS * MAX_SRC];
  static_assert(MAX_SRC <= NT && ROWS <= NT, "one thread per table entry");
  const bool rnn = (int)blockIdx.x >= step_tiles;
  const int64_t total_rows = rnn ? (int64_t)n_mb * mb : (int64_t)n_mb * mb * L;
  const int64_t first_row = (int64_t)(rnn ? blockIdx.x - step_tiles : blockIdx.x) * ROWS;
  const int rows = (int)(total_rows - first_row < ROWS ? total_rows - first_row : ROWS);
  // the pointer table into LDS. The field index is uniform (a scalar load of the field's row of pointers from the kernel arguments) and
  // lane j picks entry j by selects: a per-lane index into the by-value struct would make the compiler copy the whole table per thread.
#pragma unroll 1
  for (int k = 0; k < AC_EPOCH_NFIELDS; ++k) {
    const float* p = nullptr;
#pragma unroll
    for (int j = 0; j < MAX_SRC; ++j) p = (int)threadIdx.x == j ? tab.src[k][j] : p;
    if (threadIdx.x < MAX_SRC) s_ptr[k * MAX_SRC + threadIdx.x] = p;
  }
  if ((int)threadIdx.x < rows) {
    const int64_t g = first_row + threadIdx.x;
    int64_t q = g;            // index into `order`: i * mb + j
    int l = 0;
    if (!rnn) {
      const int64_t per_mb = (int64_t)L * mb, i = g / per_mb, r = g % per_mb;
      l = (int)(r / mb);
      q = i * mb + r % mb;
    }
    s_src[threadIdx.x] = multi_source(order[q], l, L, T, N, K);
  }
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < AC_EPOCH_NFIELDS; ++k) {
    const MultiField& F = tab.f[k];
    if (!F.dst || (F.first_only != 0) != rnn) continue;
    if (F.vec) copy_field_multi<float4>(F, s_ptr + k * MAX_SRC, s_src, first_row, rows);
    else copy_field_multi<float>(F, s_ptr + k * MAX_SRC, s_src, first_row, rows);
  }
}
}  // namespace epoch

// the refusals every list call shares (nothing is queued by them): the handles, their number, their shapes, their device
static int buffers_check(const char* fn, ac_buffer_t* const* bufs, int32_t K) {
  const std::string f(fn);
  if (!bufs) return fail(f + ": null argument");
  if (K < 1 || K > AC_EPOCH_MAX_BUFFERS) return fail(f + ": K must be in 1 .. " + std::to_string(AC_EPOCH_MAX_BUFFERS) + " buffers, got " + std::to_string(K));
  for (int k = 0; k < K; ++k) {
    if (!bufs[k]) return fail(f + ": null handle (buffer " + std::to_string(k) + ")");
    for (int j = 0; j < k; ++j)
      if (bufs[j] == bufs[k]) return fail(f + ": the same handle twice (buffers " + std::to_string(j) + " and " + std::to_string(k) + ")");
  }
  const ac_buffer_config_t& a = bufs[0]->cfg;
  for (int k = 1; k < K; ++k) {
    const ac_buffer_config_t& c = bufs[k]->cfg;
    const char* what = nullptr;
    if ((a.share_obs_dim > 0) != (c.share_obs_dim > 0)) what = "shared versus unshared";
    else if (a.buffer_size != c.buffer_size) what = "buffer_size";
    else if (a.n_envs != c.n_envs) what = "n_envs";
    else if (a.n_agents != c.n_agents) what = "n_agents";
    else if (a.obs_dim != c.obs_dim) what = "obs_dim";
    else if (a.share_obs_dim != c.share_obs_dim) what = "share_obs_dim";
    else if (a.act_dim != c.act_dim) what = "act_dim";
    else if (a.logp_dim != c.logp_dim) what = "logp_dim";
    else if (a.hidden_layers * a.hidden_size != c.hidden_layers * c.hidden_size) what = "the RNN state's width";
    if (what) return fail(f + ": buffers 0 and " + std::to_string(k) + " differ in " + what + " (a list takes buffers of one shape)");
    if (bufs[k]->device != bufs[0]->device)
      return fail(f + ": buffers 0 and " + std::to_string(k) + " are on different devices (" + std::to_string(bufs[0]->device) + ", " +
                  std::to_string(bufs[k]->device) + ")");
  }
  return 0;
}
// the stack's sizes and where its fields lie: epoch_layout's rules over K * T * N rows
static int buffers_layout(const char* fn, ac_buffer_t* const* bufs, int32_t K, int32_t n_mb, int32_t mb, int32_t L, int64_t* offsets, int64_t* total) {
  const std::string f(fn);
  if (!offsets || !total) return fail(f + ": null argument");
  if (n_mb <= 0 || mb <= 0 || L <= 0) return fail(f + ": n_minibatch, mb and chunk_len must be positive");
  const ac_buffer* b = bufs[0];
  const int64_t n_chunks = ((int64_t)b->T * b->N * K) / L;
  if (n_chunks > 0x7fffffff) return fail(f + ": the stack's K * T * N / chunk_len chunks do not fit a 32-bit index");
  if ((int64_t)n_mb * mb > n_chunks) return fail(f + ": n_minibatch * mb * chunk_len exceeds the stack's K * T * N rows");
  if ((int64_t)b->T * K > 0x7fffffff) return fail(f + ": the stack's K * T steps do not fit a 32-bit index");
  ac_buffer_config_t stack = b->cfg;
  stack.buffer_size = b->T * K;
  return epoch_layout(fn, &stack, n_mb, mb, L, offsets, total);
}
// the device `caller` belongs to (NULL: the calling thread's current device) against the buffers', before anything is queued
static int buffers_caller_ok(const char* fn, ac_buffer_t* const* bufs, hipStream_t caller) {
  int dev = -1;
  if (caller) {
    hipDevice_t d;
    if (hipStreamGetDevice(caller, &d) != hipSuccess) return fail(std::string(fn) + ": the caller's stream is not a stream of any device");
    dev = (int)d;
  } else if (hipGetDevice(&dev) != hipSuccess) {
    return fail(std::string(fn) + ": no current HIP device");
  }
  if (dev != bufs[0]->device) return fail(std::string(fn) + ": the buffers are on another device than the caller's stream");
  return 0;
}
// the kernel's table: field k written at dst[k] (NULL: not asked for)
static int buffers_table(const char* fn, ac_buffer_t* const* bufs, int32_t K, float* const dst[AC_EPOCH_NFIELDS], epoch::MultiTable* tab) {
  memset(tab, 0, sizeof *tab);
  for (int k = 0; k < AC_EPOCH_NFIELDS; ++k) {
    const int fld = kEpochField[k];
    if (!dst[k]) continue;
    if (!bufs[0]->f[fld]) return fail(std::string(fn) + ": these buffers have no such field");
    epoch::MultiField& F = tab->f[k];
    const int dim = bufs[0]->dim[fld];
    // 16-byte accesses only where every address is a 16-byte multiple: a row starts at row * dim floats behind its array, whichever of
    // the K arrays it is, and behind the field's output
    bool vec = dim % 4 == 0 && ((uintptr_t)dst[k] & 15) == 0;
    for (int j = 0; j < K; ++j) {
      tab->src[k][j] = bufs[j]->f[fld];
      vec = vec && ((uintptr_t)bufs[j]->f[fld] & 15) == 0;
    }
    F.dst = dst[k];
    F.vec = vec;
    F.units = (uint32_t)(vec ? dim / 4 : dim);
    F.magic = epoch::magic_of(F.units);
    F.first_only = k == AC_EPOCH_RNN_ACTOR || k == AC_EPOCH_RNN_CRITIC;
  }
  return 0;
}
static int buffers_launch(const char* fn, ac_buffer_t* const* bufs, int32_t K, const epoch::MultiTable& tab, const int32_t* d_order, int32_t n_mb,
                          int32_t mb, int32_t L, hipStream_t s) {
  const int64_t chunks = (int64_t)n_mb * mb;
  const int64_t step_tiles = (chunks * L + epoch::ROWS - 1) / epoch::ROWS, rnn_tiles = (chunks + epoch::ROWS - 1) / epoch::ROWS;
  if (step_tiles + rnn_tiles > 0x7fffffff) return fail(std::string(fn) + ": too many rows for one launch");
  hipLaunchKernelGGL(epoch::epoch_gather_multi_kernel, dim3((unsigned)(step_tiles + rnn_tiles)), dim3(epoch::NT), 0, s, tab, d_order, n_mb, mb, L,
                     bufs[0]->T, bufs[0]->N, K, (int)step_tiles);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(std::string(fn) + ": " + hipGetErrorString(e));
}

extern "C" {

int ac_buffers_epoch_layout(ac_buffer_t* const* bufs, int32_t K, int32_t n_minibatch, int32_t mb, int32_t chunk_len, int64_t* offsets,
                            int64_t* total_floats) {
  const char* fn = "ac_buffers_epoch_layout";
  if (buffers_check(fn, bufs, K)) return -1;
  return buffers_layout(fn, bufs, K, n_minibatch, mb, chunk_len, offsets, total_floats);
}

int ac_buffers_gather_epoch(ac_buffer_t* const* bufs, int32_t K, void* caller, const int32_t* d_order, int32_t n_minibatch, int32_t mb,
                            int32_t chunk_len, float* d_out) {
  const char* fn = "ac_buffers_gather_epoch";
  if (buffers_check(fn, bufs, K)) return -1;
  if (!d_order || !d_out) return fail(std::string(fn) + ": null argument");
  int64_t offsets[AC_EPOCH_NFIELDS], total = 0;
  if (buffers_layout(fn, bufs, K, n_minibatch, mb, chunk_len, offsets, &total)) return -1;
  float* dst[AC_EPOCH_NFIELDS];
  for (int k = 0; k < AC_EPOCH_NFIELDS; ++k) dst[k] = offsets[k] < 0 ? nullptr : d_out + offsets[k];
  epoch::MultiTable tab;
  if (buffers_table(fn, bufs, K, dst, &tab)) return -1;
  hipStream_t s = (hipStream_t)caller;
  if (buffers_caller_ok(fn, bufs, s)) return -1;
  int entered = 0, rc = 0;
  while (entered < K && !rc) {
    rc = epoch_enter(fn, bufs[entered], s);
    if (!rc) ++entered;
  }
  if (!rc) rc = buffers_launch(fn, bufs, K, tab, d_order, n_minibatch, mb, chunk_len, s);
  for (int k = 0; k < entered; ++k) rc = epoch_leave(fn, bufs[k], s, rc);
  return rc;
}

int ac_buffers_minibatch(ac_buffer_t* const* bufs, int32_t K, const int32_t* chunks, int32_t n_chunks, int32_t chunk_len, const ac_buffer_batch_t* out,
                         int on_device) {
  const char* fn = "ac_buffers_minibatch";
  if (buffers_check(fn, bufs, K)) return -1;
  if (!chunks || !out) return fail(std::string(fn) + ": null argument");
  int64_t offsets[AC_EPOCH_NFIELDS], total = 0;
  if (buffers_layout(fn, bufs, K, 1, n_chunks, chunk_len, offsets, &total)) return -1;
  ac_buffer* b = bufs[0];
  const int64_t rows = (int64_t)b->T * b->N * K;
  for (int j = 0; j < n_chunks; ++j)
    if (chunks[j] < 0 || ((int64_t)chunks[j] + 1) * chunk_len > rows) return fail(std::string(fn) + ": chunk index outside the stack");
  float* const asked[AC_EPOCH_NFIELDS] = {out->obs, out->share_obs, out->actions, out->masks, out->active_masks, out->action_log_probs, out->advantages,
                                          out->returns, out->value_preds, out->rnn_states_actor, out->rnn_states_critic};
  for (int k = 0; k < AC_EPOCH_NFIELDS; ++k)
    if (asked[k] && !b->f[kEpochField[k]]) return fail(std::string(fn) + ": these buffers have no such field");
  HIP_OK(hipSetDevice(b->device));
  // a blocking call: what the K streams hold is waited for here, the gather runs on the first buffer's stream with its scratch
  for (int k = 0; k < K; ++k) HIP_OK(hipStreamSynchronize(bufs[k]->stream));
  if (n_chunks > b->chunks_cap) {
    if (b->d_chunks) HIP_OK(hipFree(b->d_chunks));
    b->d_chunks = nullptr; b->chunks_cap = 0;
    HIP_OK(hipMalloc(&b->d_chunks, (size_t)n_chunks * sizeof(int32_t)));
    b->chunks_cap = n_chunks;
  }
  HIP_OK(hipMemcpyAsync(b->d_chunks, chunks, (size_t)n_chunks * sizeof(int32_t), hipMemcpyHostToDevice, b->stream));
  if (!on_device && total > b->stage_cap) {   // host outputs: the whole mini-batch is staged in the flat layout, then copied out field by field
    if (b->d_stage) HIP_OK(hipFree(b->d_stage));
    b->d_stage = nullptr; b->stage_cap = 0;
    HIP_OK(hipMalloc(&b->d_stage, (size_t)total * sizeof(float)));
    b->stage_cap = total;
  }
  float* dst[AC_EPOCH_NFIELDS];
  for (int k = 0; k < AC_EPOCH_NFIELDS; ++k) dst[k] = !asked[k] ? nullptr : (on_device ? asked[k] : b->d_stage + offsets[k]);
  epoch::MultiTable tab;
  if (buffers_table(fn, bufs, K, dst, &tab)) return -1;
  if (buffers_launch(fn, bufs, K, tab, b->d_chunks, 1, n_chunks, chunk_len, b->stream)) return -1;
  if (!on_device)
    for (int k = 0; k < AC_EPOCH_NFIELDS; ++k) {
      if (!asked[k]) continue;
      const bool first_only = k == AC_EPOCH_RNN_ACTOR || k == AC_EPOCH_RNN_CRITIC;
      const size_t n = (size_t)n_chunks * (first_only ? 1 : chunk_len) * b->dim[kEpochField[k]];
      HIP_OK(hipMemcpyAsync(asked[k], dst[k], n * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    }
  HIP_OK(hipStreamSynchronize(b->stream));
  return 0;
}

int ac_buffers_epoch_source_host(int32_t chunk, int32_t l, int32_t chunk_len, int32_t T, int32_t N, int32_t K, int32_t* k, int64_t* row) {
  const char* fn = "ac_buffers_epoch_source_host";
  if (!k || !row) return fail(std::string(fn) + ": null argument");
  if (T <= 0 || N <= 0 || chunk_len <= 0 || K < 1 || K > AC_EPOCH_MAX_BUFFERS || (int64_t)chunk_len > (int64_t)T * N * K || l < 0 || l >= chunk_len)
    return fail(std::string(fn) + ": T, N and chunk_len must be positive, K in 1 .. " + std::to_string(AC_EPOCH_MAX_BUFFERS) +
                ", chunk_len <= K * T * N and 0 <= l < chunk_len");
  if (((int64_t)T * N * K) / chunk_len > 0x7fffffff) return fail(std::string(fn) + ": the stack's K * T * N / chunk_len chunks do not fit a 32-bit index");
  const int64_t p = epoch::multi_source(chunk, l, chunk_len, T, N, K);
  *k = (int32_t)(p >> epoch::SRC_SHIFT);
  *row = p & epoch::ROW_MASK;
  return 0;
}

}  // extern "C"
