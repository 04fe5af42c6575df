// Whole-batch snapshot / restore and per-env clone of the env state (include/aircombat.h: ac_snapshot_*, ac_clone_envs).
//
// A snapshot is every array a later step reads that a reset does not rebuild from the config, in the order snap_sections lists
// them, each section at a 256-byte boundary behind a fixed 1024-byte header (AcSnapHeader). The arrays keep their device layout
// ([row][N] with N = E * A, rows of 4, 8 or 16 bytes per aircraft; the outputs as the step writes them, without the padding rows),
// so a whole-batch save / load is one copy per section. What does not change between steps -- reset template, tables, controller
// weights, config, kernel form -- is not copied; the header carries a digest of it (snap_config_hash), and a load refuses a
// snapshot whose digest, shape or library version differ from the handle's.
//
// Per env, every section is E chunks of A consecutive aircraft (the output rows and the info words likewise: chunk = the env's
// rows), so moving env s to env d is `rows` copies of `chunk` contiguous bytes. clone_envs_kernel does that for a list of (s, d)
// pairs: one thread per (pair, 16 / 8 / 4 / 1-byte piece of the chunk), the pieces of one pair in consecutive lanes and the pairs
// after each other, so a wave reads and writes whole runs of the row when the indices are sorted; blockIdx.y walks the rows of
// every section. No LDS, one load and one store per thread.

enum { AC_SNAP_MAGIC = 0x4e534341u /* "ACSN" */, AC_SNAP_FORMAT = 1, AC_SNAP_HDR = 1024, AC_SNAP_MAX_SECTIONS = 32, AC_SNAP_ALIGN = 256 };

struct AcSnapHeader {                     // little-endian, 1024 bytes; aircombat-selfplay_amd/snapshot.py decodes the same layout
  uint32_t magic, format;
  char version[64];                       // ac_version() of the library that wrote it
  int32_t task, E, A, msl_slots, obs_dim, act_dim, act_low, ctl_precision, hierarchical, n_sections, reserved0, reserved1;
  uint64_t config_hash;                   // snap_config_hash
  uint64_t total_bytes;                   // header + sections
  uint64_t offset[AC_SNAP_MAX_SECTIONS], bytes[AC_SNAP_MAX_SECTIONS];
  uint8_t pad[AC_SNAP_HDR - 136 - 16 * AC_SNAP_MAX_SECTIONS];
};
static_assert(sizeof(AcSnapHeader) == AC_SNAP_HDR, "snapshot header is 1024 bytes");

struct SnapSection {
  char* dev;                              // the handle's array
  size_t bytes;                           // of the whole section
  uint32_t rows, row_stride, chunk;       // rows of row_stride bytes; env e's part of a row: `chunk` bytes at e * chunk
};

static std::vector<SnapSection> snap_sections(const ac_env* h) {
  const uint32_t N = (uint32_t)h->N, A = (uint32_t)h->A, E = (uint32_t)h->E;
  const uint32_t ms = h->dc.msl_slots > 0 ? (uint32_t)h->dc.msl_slots : 1;   // (ac_create allocates one slot when there are none)
  std::vector<SnapSection> s;
  auto rows = [&](void* p, uint32_t n_rows, uint32_t elem) {
    if (p) s.push_back({(char*)p, (size_t)n_rows * N * elem, n_rows, N * elem, A * elem});
  };
  auto per_env = [&](void* p, uint32_t chunk) { s.push_back({(char*)p, (size_t)E * chunk, 1, E * chunk, chunk}); };
  rows(h->dp.F, NSG, 16);                                 // 19 groups of four words (ints aliased through dp.I)
  rows(h->dp.D, 1, 16);                                   // (rx, ry) pairs
  rows((char*)h->dp.D + (size_t)16 * N, 1, 8);            // rz
  rows(h->dp.MF, ms * NMF, 4);                            // munition slots, [slot][field][N]
  rows(h->dp.MI, ms * NMI, 4);
  rows(h->dp.MD, ms * NMF, 8);                            // scenario tasks: the fp64 slots
  rows(h->d_XF, NXF, 4);                                  // scenario extension state
  rows(h->d_XI, NXI, 4);
  rows(h->hp.HD, NHD, 8);                                 // HeadingTask: targets, clocks, turn counts, numpy PCG64 states
  rows(h->hp.HF, NHF, 4);
  rows(h->hp.HI, 1, 4);
  rows(h->hp.HR, 4, 8);
  rows(h->dp.H, 128, 4);                                  // hierarchical tasks: GRU state, last low-level action, scripted opponents
  if (h->d_low) per_env(h->d_low, A * (uint32_t)h->act_low * 4);
  rows(h->dp.man_step, 1, 4);
  rows(h->dp.man_h0, 1, 4);
  per_env(h->dp.obs, A * (uint32_t)h->obs_dim * 4);      // the last outputs
  rows(h->dp.rew, 1, 4);
  rows(h->dp.done, 1, 1);
  per_env(h->dp.info, 16);
  return s;
}

// Digest of what a step reads that is NOT in a snapshot: the device config (the decoy seed only where a kernel reads it: the
// scenario family), the heading task's constants, the task's form (hierarchical, scripted opponents, controller precision and
// weights, action widths, the kernel form ac_create picked) and the reset template as the init kernel built it.
static int snap_config_hash(ac_env* h, uint64_t* out) {
  if (!h->tmpl_hash) {
    const int A = h->A;
    std::vector<float> tf((size_t)NSW * A + (size_t)A * h->dc.tobs);
    std::vector<double> td((size_t)ND * A);
    HIP_OK(hipStreamSynchronize(h->stream));
    if (h->cfg.task != AC_TASK_HEADING) {   // (the heading task has no template: its resets draw in the kernel)
      HIP_OK(hipMemcpy(tf.data(), h->d_tF, sizeof(float) * tf.size(), hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(td.data(), h->d_tD, sizeof(double) * td.size(), hipMemcpyDeviceToHost));
    }
    uint64_t t = fnv1a(0xCBF29CE484222325ULL, tf.data(), sizeof(float) * tf.size());
    h->tmpl_hash = fnv1a(t, td.data(), sizeof(double) * td.size()) | 1ULL;
  }
  DevCfg c = h->dc;
  if (!h->d_XF) c.chaff_seed = 0;
  uint64_t x = fnv1a(0xCBF29CE484222325ULL, &c, sizeof c);
  if (h->cfg.task == AC_TASK_HEADING) x = fnv1a(x, &h->hc, sizeof h->hc);
  const int32_t form[10] = {h->cfg.hierarchical, h->cfg.use_baseline, h->cfg.controller_precision, h->act_dim, h->act_low, h->obs_dim,
                            (int32_t)h->split_waves, (int32_t)h->quad_waves, h->ctl_rows, h->E};
  x = fnv1a(x, form, sizeof form);
  x = fnv1a(x, &h->tmpl_hash, sizeof h->tmpl_hash);
  x = fnv1a(x, &h->ctl_hash, sizeof h->ctl_hash);
  *out = x;
  return 0;
}

static int snap_header(ac_env* h, AcSnapHeader* hd) {
  memset(hd, 0, sizeof *hd);
  hd->magic = AC_SNAP_MAGIC; hd->format = AC_SNAP_FORMAT;
  strncpy(hd->version, ac_version(), sizeof hd->version - 1);
  hd->task = h->cfg.task; hd->E = h->E; hd->A = h->A; hd->msl_slots = h->dc.msl_slots; hd->obs_dim = h->obs_dim; hd->act_dim = h->act_dim;
  hd->act_low = h->act_low; hd->ctl_precision = h->cfg.controller_precision; hd->hierarchical = h->cfg.hierarchical;
  if (snap_config_hash(h, &hd->config_hash)) return -1;
  const std::vector<SnapSection> s = snap_sections(h);
  if (s.size() > AC_SNAP_MAX_SECTIONS) return fail("snapshot: too many sections");
  hd->n_sections = (int32_t)s.size();
  uint64_t off = AC_SNAP_HDR;
  for (size_t k = 0; k < s.size(); ++k) {
    hd->offset[k] = off; hd->bytes[k] = s[k].bytes;
    off = (off + s[k].bytes + AC_SNAP_ALIGN - 1) / AC_SNAP_ALIGN * AC_SNAP_ALIGN;
  }
  hd->total_bytes = off;
  return 0;
}

// a snapshot header against the handle's: the first field that differs, named
static int snap_check(ac_env* h, const AcSnapHeader& got, const char* who) {
  AcSnapHeader want;
  if (snap_header(h, &want)) return -1;
  char msg[256];
  auto bad = [&](const char* what, long long a, long long b) {
    snprintf(msg, sizeof msg, "%s: snapshot %s is %lld, this handle's is %lld", who, what, a, b);
    return fail(msg);
  };
  if (got.magic != AC_SNAP_MAGIC) return fail(std::string(who) + ": not an env snapshot (bad magic word)");
  if (got.format != AC_SNAP_FORMAT) return bad("format version", got.format, want.format);
  if (strncmp(got.version, want.version, sizeof want.version))
    return fail(std::string(who) + ": snapshot written by '" + std::string(got.version, strnlen(got.version, sizeof got.version)) + "', this library is '" + want.version + "'");
  if (got.task != want.task) return bad("task", got.task, want.task);
  if (got.E != want.E) return bad("number of envs", got.E, want.E);
  if (got.A != want.A) return bad("number of agents", got.A, want.A);
  if (got.msl_slots != want.msl_slots) return bad("munition slot count", got.msl_slots, want.msl_slots);
  if (got.obs_dim != want.obs_dim) return bad("obs_dim", got.obs_dim, want.obs_dim);
  if (got.act_dim != want.act_dim) return bad("act_dim", got.act_dim, want.act_dim);
  if (got.hierarchical != want.hierarchical) return bad("hierarchical flag", got.hierarchical, want.hierarchical);
  if (got.ctl_precision != want.ctl_precision) return bad("controller precision", got.ctl_precision, want.ctl_precision);
  if (got.config_hash != want.config_hash)
    return fail(std::string(who) + ": snapshot config digest differs (config, reset template, seed, controller weights or kernel form)");
  if (got.n_sections != want.n_sections || got.total_bytes != want.total_bytes ||
      memcmp(got.offset, want.offset, sizeof want.offset) || memcmp(got.bytes, want.bytes, sizeof want.bytes))
    return fail(std::string(who) + ": snapshot section layout differs");
  return 0;
}

// ------------------------------------------------------------------------------------------------ clone kernel
struct CloneSeg { char* dst; const char* src; uint32_t row_stride, chunk, row0, shift; };   // shift: log2 of the piece width
struct CloneTable { CloneSeg s[AC_SNAP_MAX_SECTIONS]; int32_t nseg; };

// (the table's pointers come out of memory, so the compiler cannot tell they are global: said here, for global_load / global_store
// instead of flat)
typedef int clone_v4 __attribute__((ext_vector_type(4)));
template <typename T>
__device__ __forceinline__ void clone_piece(char* d, const char* s) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef __attribute__((address_space(1))) T GT;
  *(GT*)d = *(const GT*)s;
#endif
}

// grid: x = (pair, piece) threads, y = row over all sections (CloneSeg.row0 is the section's first)
__global__ void __launch_bounds__(256) clone_envs_kernel(const CloneTable* __restrict__ T, const int32_t* __restrict__ src_env,
                                                         const int32_t* __restrict__ dst_env, int32_t n) {
  const uint32_t y = blockIdx.y;
  int k = 0;
  while (k + 1 < T->nseg && y >= T->s[k + 1].row0) ++k;   // (wave-uniform: scalar loads)
  const char* src = T->s[k].src;
  char* dst = T->s[k].dst;
  const uint32_t shift = T->s[k].shift, chunk = T->s[k].chunk;
  const size_t row = (size_t)(y - T->s[k].row0) * T->s[k].row_stride;
  const uint32_t pieces = chunk >> shift;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint32_t)n * pieces) return;
  const uint32_t p = t / pieces, v = (t - p * pieces) << shift;
  const char* s = src + row + (size_t)src_env[p] * chunk + v;
  char* d = dst + row + (size_t)dst_env[p] * chunk + v;
  switch (shift) {
    case 4: clone_piece<clone_v4>(d, s); break;
    case 3: clone_piece<long long>(d, s); break;
    case 2: clone_piece<int>(d, s); break;
    default: clone_piece<char>(d, s); break;
  }
}

// Full-state digest: every word of every section, mixed with (section, word index), summed (order-independent within a launch).
__global__ void snapshot_checksum_kernel(const uint32_t* __restrict__ w, size_t nw, uint32_t section, unsigned long long* out) {
  unsigned long long acc = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nw; i += (size_t)gridDim.x * blockDim.x) {
    unsigned long long z = ((unsigned long long)w[i] | ((unsigned long long)section << 32)) + 0x9E3779B97F4A7C15ULL * (i + 1);
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ULL; z ^= z >> 27; z *= 0x94D049BB133111EBULL; z ^= z >> 31;
    acc += z;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);
}

static int snap_scratch(ac_env* h, int32_t n) {   // the handle's index staging: pinned host + device, 2 x n words, grown on demand
  if (n <= h->idx_cap) return 0;
  if (h->h_idx) HIP_OK(hipHostFree(h->h_idx));
  if (h->d_idx) HIP_OK(hipFree(h->d_idx));
  h->h_idx = nullptr; h->d_idx = nullptr; h->idx_cap = 0;
  HIP_OK(hipHostMalloc((void**)&h->h_idx, sizeof(int32_t) * 2 * (size_t)n, hipHostMallocDefault));
  HIP_OK(hipMalloc(&h->d_idx, sizeof(int32_t) * 2 * (size_t)n));
  h->idx_cap = n;
  return 0;
}

// Indices from device or host memory (hipMemcpyDefault), copied on the handle's stream -- after whatever ac_order_after queued --
// and checked on the host: in range, and no env written twice. `src` may be null (partial restore: source = destination).
static int snap_stage_indices(ac_env* h, const int32_t* src, const int32_t* dst, int32_t n, const char* who) {
  if (n <= 0 || !dst) return fail(std::string(who) + ": need n > 0 env indices");
  if (n > h->E) return fail(std::string(who) + ": more destination envs than the handle has (a destination may appear once)");
  if (snap_scratch(h, n)) return -1;
  HIP_OK(hipStreamSynchronize(h->stream));   // (also: the previous call's uploads out of h_idx / h_clone_tab are done)
  int32_t* hs = h->h_idx; int32_t* hd = h->h_idx + n;
  auto fetch = [&](int32_t* to, const int32_t* from) -> int {
    hipPointerAttribute_t a;
    const bool on_device = hipPointerGetAttributes(&a, from) == hipSuccess && a.type == hipMemoryTypeDevice;
    (void)hipGetLastError();   // (an unregistered host pointer leaves an error behind)
    if (!on_device) { memcpy(to, from, sizeof(int32_t) * n); return 0; }
    HIP_OK(hipMemcpyAsync(to, from, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    return 0;
  };
  if (fetch(hd, dst) || (src && fetch(hs, src))) return -1;
  HIP_OK(hipStreamSynchronize(h->stream));
  if (!src) memcpy(hs, hd, sizeof(int32_t) * n);
  std::vector<uint8_t> seen(h->E, 0);
  char msg[192];
  for (int32_t k = 0; k < n; ++k) {
    if (hs[k] < 0 || hs[k] >= h->E || hd[k] < 0 || hd[k] >= h->E) {
      snprintf(msg, sizeof msg, "%s: env index out of range at position %d (src %d, dst %d; the handle has %d envs)", who, k, hs[k], hd[k], h->E);
      return fail(msg);
    }
    if (seen[hd[k]]++) {
      snprintf(msg, sizeof msg, "%s: destination env %d appears twice", who, hd[k]);
      return fail(msg);
    }
  }
  // one launch reads every source and writes every destination with no order between its blocks: an env that is written by the call
  // may not be read by another pair (a chain 0 -> 1 -> 2 or a swap 1 <-> 2 would tear rows). (A partial restore reads the snapshot.)
  // (a pair that copies an env onto itself rewrites the bytes it reads: other pairs may read that env)
  if (src) {
    std::vector<int32_t> writer(h->E, -1);   // the source each destination is written from
    for (int32_t k = 0; k < n; ++k) writer[hd[k]] = hs[k];
    for (int32_t k = 0; k < n; ++k)
      if (writer[hs[k]] >= 0 && writer[hs[k]] != hs[k]) {
        snprintf(msg, sizeof msg, "%s: env %d is both a source (position %d) and a destination of the same call; clone in two calls", who, hs[k], k);
        return fail(msg);
      }
  }
  HIP_OK(hipMemcpyAsync(h->d_idx, h->h_idx, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyHostToDevice, h->stream));
  return 0;
}

// every section's rows, from `src_base` (a snapshot: section k at offset[k]; null: the handle's own arrays) into the handle
static int snap_launch_clone(ac_env* h, const char* src_base, const AcSnapHeader* hd, int32_t n) {
  const std::vector<SnapSection> s = snap_sections(h);
  CloneTable t{};
  uint32_t row0 = 0;
  for (size_t k = 0; k < s.size(); ++k) {
    uint32_t shift = 4;
    while (shift && ((s[k].chunk | s[k].row_stride) & ((1u << shift) - 1))) --shift;
    if (shift == 1) shift = 0;   // (no 2-byte pieces: every section is 4-byte words but the dones)
    t.s[k] = CloneSeg{s[k].dev, src_base ? src_base + hd->offset[k] : s[k].dev, s[k].row_stride, s[k].chunk, row0, shift};
    row0 += s[k].rows;
  }
  t.nseg = (int32_t)s.size();
  if (!h->d_clone_tab) {
    HIP_OK(hipMalloc(&h->d_clone_tab, sizeof(CloneTable)));
    HIP_OK(hipHostMalloc(&h->h_clone_tab, sizeof(CloneTable), hipHostMallocDefault));
  }
  // (the table goes up with the indices, in the order of the stream; snap_stage_indices waited for the previous upload)
  memcpy(h->h_clone_tab, &t, sizeof t);
  HIP_OK(hipMemcpyAsync(h->d_clone_tab, h->h_clone_tab, sizeof t, hipMemcpyHostToDevice, h->stream));
  uint32_t max_pieces = 0;
  for (size_t k = 0; k < s.size(); ++k) max_pieces = std::max(max_pieces, s[k].chunk >> t.s[k].shift);
  const dim3 grid(((uint32_t)n * max_pieces + 255) / 256, row0);
  hipLaunchKernelGGL(clone_envs_kernel, grid, dim3(256), 0, h->stream, (const CloneTable*)h->d_clone_tab, h->d_idx, h->d_idx + n, n);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" {

int ac_snapshot_bytes(ac_env_t* h, int64_t* bytes) {
  if (!h || !bytes) return fail("ac_snapshot_bytes: null argument");
  if (host_entry(h)) return -1;
  AcSnapHeader hd;
  if (snap_header(h, &hd)) return -1;
  *bytes = (int64_t)hd.total_bytes;
  return 0;
}

int ac_snapshot_header(ac_env_t* h, void* out) {
  if (!h || !out) return fail("ac_snapshot_header: null argument");
  if (host_entry(h)) return -1;
  HIP_OK(hipSetDevice(h->device));
  AcSnapHeader hd;
  if (snap_header(h, &hd)) return -1;
  memcpy(out, &hd, sizeof hd);
  return 0;
}

static int snap_healthy(ac_env* h, const char* who) {
  if (h->err_host && *(volatile int*)h->err_host) h->err_sticky = *(volatile int*)h->err_host;
  if (h->err_sticky) return fail(std::string(who) + ": the handle's non-finite guard has fired; a snapshot of that state is refused (ac_reset clears it)");
  return 0;
}

int ac_snapshot_save(ac_env_t* h, void* d_dst) {
  if (!h || !d_dst) return fail("ac_snapshot_save: null argument");
  if (host_entry(h)) return -1;
  HIP_OK(hipSetDevice(h->device));
  if (snap_healthy(h, "ac_snapshot_save")) return -1;
  if (!h->snap_hdr_ok) {   // the header is constant per handle (until ac_load_controller): built and uploaded once
    AcSnapHeader hd;
    if (snap_header(h, &hd)) return -1;
    if (!h->d_snap_hdr) HIP_OK(hipMalloc(&h->d_snap_hdr, sizeof hd));
    HIP_OK(hipMemcpy(h->d_snap_hdr, &hd, sizeof hd, hipMemcpyHostToDevice));
    memcpy(h->snap_hdr, &hd, sizeof hd);
    h->snap_hdr_ok = true;
  }
  AcSnapHeader hd;
  memcpy(&hd, h->snap_hdr, sizeof hd);
  char* dst = (char*)d_dst;
  HIP_OK(hipMemcpyAsync(dst, h->d_snap_hdr, sizeof hd, hipMemcpyDeviceToDevice, h->stream));
  const std::vector<SnapSection> s = snap_sections(h);
  for (size_t k = 0; k < s.size(); ++k) HIP_OK(hipMemcpyAsync(dst + hd.offset[k], s[k].dev, s[k].bytes, hipMemcpyDeviceToDevice, h->stream));
  return 0;
}

int ac_snapshot_save_host(ac_env_t* h, void* dst, int64_t bytes) {
  if (!h || !dst) return fail("ac_snapshot_save_host: null argument");
  if (host_entry(h)) return -1;
  HIP_OK(hipSetDevice(h->device));
  AcSnapHeader hd;
  if (snap_header(h, &hd)) return -1;
  if (bytes < (int64_t)hd.total_bytes) return fail("ac_snapshot_save_host: buffer smaller than ac_snapshot_bytes");
  HIP_OK(hipStreamSynchronize(h->stream));
  if (snap_healthy(h, "ac_snapshot_save_host")) return -1;
  char* d = (char*)dst;
  memcpy(d, &hd, sizeof hd);
  const std::vector<SnapSection> s = snap_sections(h);
  for (size_t k = 0; k < s.size(); ++k) HIP_OK(hipMemcpyAsync(d + hd.offset[k], s[k].dev, s[k].bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

// the whole state replaced by a snapshot (which a save only takes of a healthy handle): the non-finite guard starts clear
static void snap_clear_guard(ac_env* h) { *(volatile int*)h->err_host = 0; h->err_sticky = 0; }

int ac_snapshot_load(ac_env_t* h, const void* d_src) {
  if (!h || !d_src) return fail("ac_snapshot_load: null argument");
  if (host_entry(h)) return -1;
  HIP_OK(hipSetDevice(h->device));
  AcSnapHeader got;
  HIP_OK(hipMemcpyAsync(&got, d_src, sizeof got, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));   // (also: no step in flight writes the error word after the clear below)
  if (snap_check(h, got, "ac_snapshot_load")) return -1;
  snap_clear_guard(h);
  const char* src = (const char*)d_src;
  const std::vector<SnapSection> s = snap_sections(h);
  for (size_t k = 0; k < s.size(); ++k) HIP_OK(hipMemcpyAsync(s[k].dev, src + got.offset[k], s[k].bytes, hipMemcpyDeviceToDevice, h->stream));
  return 0;
}

int ac_snapshot_load_host(ac_env_t* h, const void* src, int64_t bytes) {
  if (!h || !src) return fail("ac_snapshot_load_host: null argument");
  if (host_entry(h)) return -1;
  HIP_OK(hipSetDevice(h->device));
  if (bytes < (int64_t)sizeof(AcSnapHeader)) return fail("ac_snapshot_load_host: shorter than a snapshot header");
  AcSnapHeader got;
  memcpy(&got, src, sizeof got);
  if (snap_check(h, got, "ac_snapshot_load_host")) return -1;
  if (bytes < (int64_t)got.total_bytes) return fail("ac_snapshot_load_host: buffer shorter than the snapshot it holds");
  HIP_OK(hipStreamSynchronize(h->stream));
  snap_clear_guard(h);
  const char* s0 = (const char*)src;
  const std::vector<SnapSection> s = snap_sections(h);
  for (size_t k = 0; k < s.size(); ++k) HIP_OK(hipMemcpyAsync(s[k].dev, s0 + got.offset[k], s[k].bytes, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));   // (the source may be pageable memory the caller frees next)
  return 0;
}

int ac_clone_envs(ac_env_t* h, const int32_t* src, const int32_t* dst, int32_t n) {
  if (!h || !src || !dst) return fail("ac_clone_envs: null argument");
  if (host_entry(h)) return -1;
  HIP_OK(hipSetDevice(h->device));
  if (snap_stage_indices(h, src, dst, n, "ac_clone_envs")) return -1;
  return snap_launch_clone(h, nullptr, nullptr, n);
}

int ac_snapshot_load_envs(ac_env_t* h, const void* d_src, const int32_t* idx, int32_t n) {
  if (!h || !d_src || !idx) return fail("ac_snapshot_load_envs: null argument");
  if (host_entry(h)) return -1;
  HIP_OK(hipSetDevice(h->device));
  AcSnapHeader got;
  HIP_OK(hipMemcpyAsync(&got, d_src, sizeof got, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  if (snap_check(h, got, "ac_snapshot_load_envs")) return -1;
  if (snap_stage_indices(h, nullptr, idx, n, "ac_snapshot_load_envs")) return -1;
  return snap_launch_clone(h, (const char*)d_src, &got, n);
}

int ac_get_obs(ac_env_t* h, float* obs) {
  if (!h || !obs) return fail("ac_get_obs: null argument");
  if (host_entry(h)) return -1;
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipMemcpyAsync(obs, h->dp.obs, sizeof(float) * (size_t)h->N * h->obs_dim, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int ac_snapshot_checksum(ac_env_t* h, uint64_t* out) {
  if (!h || !out) return fail("ac_snapshot_checksum: null argument");
  if (host_entry(h)) return -1;
  HIP_OK(hipSetDevice(h->device));
  unsigned long long* d_out;
  HIP_OK(hipMalloc(&d_out, sizeof(unsigned long long)));
  HIP_OK(hipMemsetAsync(d_out, 0, sizeof(unsigned long long), h->stream));
  const std::vector<SnapSection> s = snap_sections(h);
  for (size_t k = 0; k < s.size(); ++k) {
    const size_t nw = s[k].bytes / 4;   // (the dones: N bytes; a tail of N % 4 is folded in by the host below)
    const unsigned blocks = (unsigned)std::min<size_t>(1024, (nw + 255) / 256);
    if (nw) hipLaunchKernelGGL(snapshot_checksum_kernel, dim3(blocks), dim3(256), 0, h->stream, (const uint32_t*)s[k].dev, nw, (uint32_t)k, d_out);
    HIP_OK(hipGetLastError());
  }
  HIP_OK(hipStreamSynchronize(h->stream));
  unsigned long long v = 0;
  HIP_OK(hipMemcpy(&v, d_out, sizeof v, hipMemcpyDeviceToHost));
  HIP_OK(hipFree(d_out));
  for (size_t k = 0; k < s.size(); ++k)
    if (s[k].bytes % 4) {
      unsigned char tail[4] = {0, 0, 0, 0};
      HIP_OK(hipMemcpy(tail, s[k].dev + s[k].bytes / 4 * 4, s[k].bytes % 4, hipMemcpyDeviceToHost));
      v = fnv1a(v, tail, sizeof tail);
    }
  *out = (uint64_t)v;
  return 0;
}

}  // extern "C"
