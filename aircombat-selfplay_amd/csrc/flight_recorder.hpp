// The device flight recorder (include/aircombat_record.h): what an ACMI frame needs, captured behind every step of a handle for a chosen
// set of envs. Included from aircombat.hip after launch_reset: launch_step, host_step and ac_reset call recorder_hook, declared ahead of them.
//
// recorder_capture_kernel is a streaming kernel: one lane per selected aircraft (S * A lanes in 64-lane waves), no cross-lane work, no
// atomics, no device-side counter. A lane reads its aircraft as entity_kernel does (load_state, f16::locate, f16::body_frame, make_props),
// its munition slots from MI and MD or MF and the two extension words, and writes each value to its column of the frame's ring slot:
// column [F][count][S * A], so a wave's store of one value is one contiguous run. The slot index comes in as an argument -- every
// capture is queued by a host call, which is where the frame count lives.
#pragma once
#include "../../include/aircombat_record.h"

// ac_get_entity's twelve values of aircraft n (BaseSimulator.log's inputs and the NED velocity / NEU position next to them); `t` returns the
// aircraft's task record, which the capture kernel also needs. One body for entity_kernel and recorder_capture_kernel: the same
// operations on the same loaded words in both, so a recorded entity is ac_get_entity's to the last bit (tests/test_gpu_recorder.py
// compares them as raw bytes; should a compiler ever contract the two inlined copies differently, make this __noinline__).
__device__ __forceinline__ void entity_values(const DevPtrs& P, const DevCfg& c, int n, double* out, Task& t) {
  State s; Derived d; Props pr;
  load_state(P.F, P.I, P.D, c.N, n, s, t);
  f16::locate(s, d); f16::body_frame(s, d);
  make_props(s, d, c, pr);
  const double R2D = 180.0 / 3.14159265358979323846;
  out[0] = atan2(d.sLon64, d.cLon64) * R2D; out[1] = atan2(d.sLat64, d.cLat64) * R2D; out[2] = pr.alt_m;
  out[3] = atan2f(pr.sphi, pr.cphi); out[4] = asinf(pr.stht);
  float psi = atan2f(pr.m12, pr.m11); if (psi < 0.0f) psi += 2.0f * f16::kPi;
  out[5] = psi; out[6] = pr.vn; out[7] = pr.ve; out[8] = pr.vd; out[9] = pr.n; out[10] = pr.e; out[11] = pr.u;
}

namespace rec {
enum { C_cur_step, C_flags, C_status, C_entity, C_msl_status, C_msl_model, C_msl_pose, C_ext, NCOL };
static_assert(NCOL == AC_REC_MAX_COLUMNS, "ac_recorder_layout_t holds every column");
constexpr int kPose = 5;   // px, py, pz, theta, psi

// the table of a shape, and where its columns start in a ring of F frames of SA lanes (multiples of 256 bytes)
struct Layout {
  int ncol, bytes_af;
  int id[NCOL], size[NCOL], count[NCOL];
};
inline Layout layout_of(int msl_slots, bool ext) {
  Layout L{};
  auto add = [&](int id, int size, int count) {
    if (count < 1) return;
    L.id[L.ncol] = id; L.size[L.ncol] = size; L.count[L.ncol] = count; ++L.ncol;
    L.bytes_af += size * count;
  };
  add(C_cur_step, 4, 1); add(C_flags, 4, 1); add(C_status, 4, 1); add(C_entity, 8, 12);
  add(C_msl_status, 4, msl_slots); add(C_msl_model, 4, msl_slots); add(C_msl_pose, 8, kPose * msl_slots);
  add(C_ext, 4, ext ? 2 : 0);
  return L;
}
inline const char* column_name(int id) {
  static const char* names[NCOL] = {"cur_step", "flags", "status", "entity", "msl_status", "msl_model", "msl_pose", "ext"};
  return names[id];
}
// device addresses of the ring's columns by column id (null where the shape has none)
struct Ring {
  int* cur_step; int* flags; int* status; double* entity;
  int* msl_status; int* msl_model; double* msl_pose; int* ext;
};
// what the extract kernel walks: the shape's columns in table order, in 32-bit words
struct Cols {
  int ncol;
  int count[NCOL], words[NCOL];
  const unsigned* base[NCOL];
};
}  // namespace rec

// lane i = (position in the selection) * A + agent. slot: the frame's ring slot; sa = S * A; flags0: AC_REC_AFTER_RESET or 0. K = the
// handle's munition slots, a template parameter so that the slot loops unroll: every load of the lane is issued before the entity
// arithmetic and every store after it, instead of one load-to-store round trip per slot and value.
template <int K>
__global__ __launch_bounds__(64) void recorder_capture_kernel(DevPtrs P, DevCfg c, const int* __restrict__ XI, const int* __restrict__ sel, rec::Ring R,
                                                              int sa, int slot, int flags0) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sa) return;
  const int A = c.A;
  const int e = sel ? sel[i / A] : i / A;
  const int n = e * A + i % A;
  const size_t N = (size_t)c.N, SA = (size_t)sa, f = (size_t)slot;
  constexpr int pose_field[rec::kPose] = {MF_px, MF_py, MF_pz, MF_theta, MF_psi};
  constexpr int KK = K > 0 ? K : 1;
  int m_status[KK], m_recede[KK], w0 = 0, w1 = 0;
  double m_pose[KK][rec::kPose];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    m_status[k] = P.MI[((size_t)k * NMI + MI_status) * N + n];
    m_recede[k] = P.MI[((size_t)k * NMI + MI_recede) * N + n];
#pragma unroll
    for (int q = 0; q < rec::kPose; ++q) {
      const size_t w = ((size_t)k * NMF + pose_field[q]) * N + n;
      m_pose[k][q] = P.MD ? P.MD[w] : (double)P.MF[w];
    }
  }
  if (XI) { w0 = XI[(size_t)XI_w0 * N + n]; w1 = XI[(size_t)XI_w1 * N + n]; }
  const int done = P.done[n];
  Task t;
  double ent[12];
  entity_values(P, c, n, ent, t);
  R.cur_step[f * SA + i] = t.cur_step;
  R.flags[f * SA + i] = flags0 | ((flags0 & AC_REC_AFTER_RESET) ? 0 : (done ? AC_REC_DONE : 0));
  R.status[f * SA + i] = t.status;
#pragma unroll
  for (int j = 0; j < 12; ++j) R.entity[(f * 12 + j) * SA + i] = ent[j];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    R.msl_status[(f * K + k) * SA + i] = m_status[k];
    // (ac_get_missile's out[11]: the scenario family names its munitions, the 1v1 missile tasks fly the AIM-9L)
    R.msl_model[(f * K + k) * SA + i] = (P.MD && c.task != AC_TASK_DODGE_MISSILE) ? 1 + ((m_recede[k] >> 9) & 1) : 0;
#pragma unroll
    for (int q = 0; q < rec::kPose; ++q) R.msl_pose[((f * K + k) * rec::kPose + q) * SA + i] = m_pose[k][q];
  }
  if (XI) {
    R.ext[(f * 2 + 0) * SA + i] = w0;
    R.ext[(f * 2 + 1) * SA + i] = w1;
  }
}

// Frames [f0, f0 + n) of the env at position `pos` of the selection, one thread per (frame, agent), every column's words copied to
// out: column after column, column c as [n][count][A] elements.
__global__ __launch_bounds__(64) void recorder_extract_kernel(rec::Cols C, int sa, int A, int F, int pos, long long f0, int n, unsigned* __restrict__ out) {
  const int item = blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= n * A) return;
  const int r = item / A, a = item % A;
  const size_t slot = (size_t)((f0 + r) % F), SA = (size_t)sa, lane = (size_t)pos * A + a;
  size_t o = 0;
  for (int c = 0; c < C.ncol; ++c) {
    const size_t cnt = (size_t)C.count[c], w = (size_t)C.words[c];
    for (size_t j = 0; j < cnt; ++j)
      for (size_t q = 0; q < w; ++q)
        out[o + (((size_t)r * cnt + j) * A + a) * w + q] = C.base[c][((slot * cnt + j) * SA + lane) * w + q];
    o += (size_t)n * cnt * A * w;
  }
}

struct ac_recorder {
  ac_env* env;                  // null once the handle has been destroyed
  int device, A, S, F, K;
  bool ext, attached;
  long long count;              // captures queued so far
  rec::Layout lay;
  size_t col_off[rec::NCOL];    // by table position
  size_t ring_bytes, staging_bytes;
  std::vector<int> sel;         // the selection (all envs spelled out), for ac_recorder_read's lookup
  char* d_ring;
  int* d_sel;                   // null: all envs
  unsigned* d_staging;          // F * A aircraft-frames
  rec::Ring ring;
};

namespace rec {
inline size_t ring_bytes_of(const Layout& L, size_t F, size_t SA, size_t* off) {
  size_t b = 0;
  for (int c = 0; c < L.ncol; ++c) {
    if (off) off[c] = b;
    b += (F * (size_t)L.count[c] * SA * (size_t)L.size[c] + 255) / 256 * 256;
  }
  return b;
}
// "" when (sel, S, F) is a usable selection for a handle of E envs
inline std::string selection_error(int E, const int32_t* sel, int S, int F) {
  if (F < 1) return "the capacity F must be at least 1 frame (got " + std::to_string(F) + ")";
  if (!sel) return "";
  if (S < 1 || S > E) return "S must be in 1 .. E = " + std::to_string(E) + " (got " + std::to_string(S) + ")";
  for (int i = 0; i < S; ++i) {
    if (sel[i] < 0 || sel[i] >= E) return "env index " + std::to_string(sel[i]) + " out of range (E = " + std::to_string(E) + ")";
    if (i && sel[i] == sel[i - 1]) return "env index " + std::to_string(sel[i]) + " appears twice";
    if (i && sel[i] < sel[i - 1]) return "the selection is not sorted (" + std::to_string(sel[i]) + " after " + std::to_string(sel[i - 1]) + ")";
  }
  return "";
}
}  // namespace rec

// one frame of `r` queued on the handle's stream (the caller has passed host_entry or is a step path)
static int recorder_capture(ac_recorder* r, int after_reset) {
  ac_env* h = r->env;
  const int sa = r->S * r->A;
  auto* kernel = r->K == 0 ? recorder_capture_kernel<0> : (r->K == 2 ? recorder_capture_kernel<2> : recorder_capture_kernel<AC_MAX_MISSILES_PER_AGENT>);
  hipLaunchKernelGGL(kernel, dim3((sa + 63) / 64), dim3(64), 0, h->stream, h->dp, h->dc, r->ext ? h->d_XI : nullptr, r->d_sel, r->ring, sa,
                     (int)(r->count % r->F), after_reset ? (int)AC_REC_AFTER_RESET : 0);
  HIP_OK(hipGetLastError());
  h->stream_dirty = true;
  r->count += 1;
  return 0;
}
static int recorder_hook(ac_env* h, int after_reset) { return h->rec ? recorder_capture(h->rec, after_reset) : 0; }
static void recorder_env_gone(ac_env* h) {   // ac_destroy: the recorder outlives its handle only as something to destroy
  if (h->rec) { h->rec->attached = false; h->rec->env = nullptr; h->rec = nullptr; }
}

extern "C" {

int ac_recorder_layout(int32_t task, int32_t A, int32_t msl_slots, int32_t has_ext, ac_recorder_layout_t* out) {
  if (!out) return fail("ac_recorder_layout: null argument");
  if (task < AC_TASK_HEADING || task > AC_TASK_MANEUVER || A < 1 || A > AC_MAX_AGENTS || msl_slots < 0 || msl_slots > AC_MAX_MISSILES_PER_AGENT)
    return fail("ac_recorder_layout: task, A (1 .. 8) or msl_slots (0 .. 4) out of range");
  const rec::Layout L = rec::layout_of(msl_slots, has_ext != 0);
  memset(out, 0, sizeof *out);
  out->n_columns = L.ncol; out->bytes_per_aircraft_frame = L.bytes_af;
  for (int c = 0; c < L.ncol; ++c) {
    snprintf(out->columns[c].name, sizeof out->columns[c].name, "%s", rec::column_name(L.id[c]));
    out->columns[c].elem_size = L.size[c]; out->columns[c].count = L.count[c];
  }
  return 0;
}

int ac_recorder_bytes(ac_env_t* env, int32_t S, int32_t F, int64_t* bytes) {
  if (!env || !bytes) return fail("ac_recorder_bytes: null argument");
  if (S < 1 || S > env->E || F < 1) return fail("ac_recorder_bytes: S must be in 1 .. E and F at least 1");
  const rec::Layout L = rec::layout_of(env->dc.msl_slots, env->d_XI != nullptr);
  const size_t A = (size_t)env->A;
  *bytes = (int64_t)(rec::ring_bytes_of(L, (size_t)F, (size_t)S * A, nullptr) + sizeof(int) * (size_t)S + (size_t)F * A * L.bytes_af);
  return 0;
}

int ac_recorder_destroy(ac_recorder_t* r) {
  if (!r) return 0;
  (void)hipSetDevice(r->device);
  if (r->env) {
    (void)aql_settle(r->env);
    (void)hipStreamSynchronize(r->env->stream);   // no capture may still be writing into the ring
    if (r->env->rec == r) r->env->rec = nullptr;
  }
  for (void* q : {(void*)r->d_ring, (void*)r->d_sel, (void*)r->d_staging})
    if (q) (void)hipFree(q);
  delete r;
  return 0;
}

int ac_recorder_create(ac_env_t* env, const int32_t* sel, int32_t S, int32_t F, ac_recorder_t** out) {
  if (!env || !out) return fail("ac_recorder_create: null argument");
  *out = nullptr;
  const std::string bad = rec::selection_error(env->E, sel, S, F);
  if (!bad.empty()) return fail("ac_recorder_create: " + bad);
  if (host_entry(env)) return -1;
  HIP_OK(hipSetDevice(env->device));
  ac_recorder* r = new ac_recorder();
  r->env = env; r->device = env->device; r->A = env->A; r->S = sel ? S : env->E; r->F = F; r->K = env->dc.msl_slots;
  r->ext = env->d_XI != nullptr; r->attached = false; r->count = 0;
  if (r->K != 0 && r->K != 2 && r->K != AC_MAX_MISSILES_PER_AGENT) { delete r; return fail("ac_recorder_create: no capture kernel for this many munition slots"); }
  r->lay = rec::layout_of(r->K, r->ext);
  r->sel.resize(r->S);
  for (int i = 0; i < r->S; ++i) r->sel[i] = sel ? sel[i] : i;
  const size_t SA = (size_t)r->S * r->A;
  r->ring_bytes = rec::ring_bytes_of(r->lay, (size_t)F, SA, r->col_off);
  r->staging_bytes = (size_t)F * r->A * r->lay.bytes_af;
  r->d_ring = nullptr; r->d_sel = nullptr; r->d_staging = nullptr;
  hipError_t err = hipMalloc((void**)&r->d_ring, r->ring_bytes);
  if (err == hipSuccess) err = hipMalloc((void**)&r->d_staging, r->staging_bytes);
  if (err == hipSuccess && sel) err = hipMalloc((void**)&r->d_sel, sizeof(int) * (size_t)S);
  if (err == hipSuccess) err = hipMemsetAsync(r->d_ring, 0, r->ring_bytes, env->stream);
  if (err == hipSuccess && sel) err = hipMemcpyAsync(r->d_sel, r->sel.data(), sizeof(int) * (size_t)S, hipMemcpyHostToDevice, env->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(env->stream);
  if (err != hipSuccess) {
    (void)hipGetLastError();   // (an allocation the runtime refuses leaves its error behind for the next hipGetLastError)
    const size_t want = r->ring_bytes + r->staging_bytes;
    ac_recorder_destroy(r);
    return fail(std::string("ac_recorder_create: ") + hipGetErrorString(err) + " (a ring of " + std::to_string(want) + " bytes)");
  }
  void* base[rec::NCOL] = {};
  for (int c = 0; c < r->lay.ncol; ++c) base[r->lay.id[c]] = r->d_ring + r->col_off[c];
  r->ring = rec::Ring{(int*)base[rec::C_cur_step], (int*)base[rec::C_flags], (int*)base[rec::C_status], (double*)base[rec::C_entity],
                      (int*)base[rec::C_msl_status], (int*)base[rec::C_msl_model], (double*)base[rec::C_msl_pose], (int*)base[rec::C_ext]};
  *out = r;
  return 0;
}

int ac_recorder_attach(ac_env_t* env, ac_recorder_t* r) {
  if (!env || !r) return fail("ac_recorder_attach: null argument");
  if (r->env != env) return fail("ac_recorder_attach: the recorder was made for another handle");
  if (env->rec == r) return 0;
  if (env->rec) return fail("ac_recorder_attach: the handle already has a recorder attached (ac_recorder_detach first)");
  if (host_entry(env)) return -1;   // (a host step in flight on the AQL queue ends before the first hooked one)
  env->rec = r; r->attached = true;
  return 0;
}
int ac_recorder_detach(ac_env_t* env) {
  if (!env) return fail("ac_recorder_detach: null handle");
  if (env->rec) { env->rec->attached = false; env->rec = nullptr; }
  return 0;
}

int ac_recorder_capture(ac_recorder_t* r, int32_t after_reset) {
  if (!r) return fail("ac_recorder_capture: null handle");
  if (!r->env) return fail("ac_recorder_capture: the recorder's handle has been destroyed");
  if (host_entry(r->env)) return -1;
  HIP_OK(hipSetDevice(r->device));
  return recorder_capture(r, after_reset);
}
int64_t ac_recorder_count(ac_recorder_t* r) { return r ? (int64_t)r->count : -1; }

int ac_recorder_info(ac_recorder_t* r, ac_recorder_info_t* out) {
  if (!r || !out) return fail("ac_recorder_info: null argument");
  if (!r->env) return fail("ac_recorder_info: the recorder's handle has been destroyed");
  out->task = r->env->cfg.task; out->A = r->A; out->msl_slots = r->K; out->has_ext = r->ext ? 1 : 0;
  out->E = r->env->E; out->S = r->S; out->F = r->F; out->attached = r->attached ? 1 : 0;
  out->count = r->count; out->bytes = (int64_t)(r->ring_bytes + r->staging_bytes + (r->d_sel ? sizeof(int) * (size_t)r->S : 0));
  return 0;
}

int ac_recorder_read(ac_recorder_t* r, int32_t env, int64_t f0, int32_t n, void* host_out) {
  if (!r || !host_out) return fail("ac_recorder_read: null argument");
  if (!r->env) return fail("ac_recorder_read: the recorder's handle has been destroyed");
  const auto it = std::lower_bound(r->sel.begin(), r->sel.end(), (int)env);
  if (it == r->sel.end() || *it != env) return fail("ac_recorder_read: env " + std::to_string(env) + " is not among the recorded envs");
  const long long oldest = std::max(0LL, r->count - r->F);
  if (n < 1) return fail("ac_recorder_read: n must be at least 1");
  if (f0 < oldest)
    return fail("ac_recorder_read: frame " + std::to_string(f0) + " has been overwritten (readable: " + std::to_string(oldest) + " .. " +
                std::to_string(r->count - 1) + ")");
  if (f0 + n > r->count)
    return fail("ac_recorder_read: frame " + std::to_string(f0 + n - 1) + " has not been captured (readable: " + std::to_string(oldest) + " .. " +
                std::to_string(r->count - 1) + ")");
  ac_env* h = r->env;
  if (host_entry(h)) return -1;
  HIP_OK(hipSetDevice(r->device));
  rec::Cols C{};
  C.ncol = r->lay.ncol;
  for (int c = 0; c < r->lay.ncol; ++c) {
    C.count[c] = r->lay.count[c]; C.words[c] = r->lay.size[c] / 4;
    C.base[c] = reinterpret_cast<const unsigned*>(r->d_ring + r->col_off[c]);
  }
  const int items = n * r->A;   // n <= F: within the staging buffer
  hipLaunchKernelGGL(recorder_extract_kernel, dim3((items + 63) / 64), dim3(64), 0, h->stream, C, r->S * r->A, r->A, r->F, (int)(it - r->sel.begin()),
                     (long long)f0, (int)n, r->d_staging);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(host_out, r->d_staging, (size_t)items * r->lay.bytes_af, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int ac_recorder_device_ptr(ac_recorder_t* r, int32_t column, void** ptr, int64_t* elements) {
  if (!r || !ptr || !elements) return fail("ac_recorder_device_ptr: null argument");
  if (column < 0 || column >= r->lay.ncol) return fail("ac_recorder_device_ptr: no such column (ac_recorder_layout lists them)");
  *ptr = r->d_ring + r->col_off[column];
  *elements = (int64_t)r->F * r->lay.count[column] * r->S * r->A;
  return 0;
}

}  // extern "C"
