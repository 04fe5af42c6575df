// Host steps as raw AQL packets ("Step outputs and the host boundary").
//
// Every host step of a handle launches the same kernel(s) with the same grid and the same kernarg bytes for a given host set. The HIP
// runtime rebuilds and uploads those bytes on every launch and waits through its own stream machinery; here the handle owns one HSA
// queue, keeps one kernarg block per host set in device memory (written once, rewritten only when its bytes change), writes the
// 64-byte kernel-dispatch packet itself, rings the doorbell and busy-waits on the packet's completion signal. tools/micro/aql_dispatch.hip
// measured the difference (profiles/aql_dispatch.txt).
//
// The kernel objects are HIP's own: the first host step goes through hipLaunchKernel, which loads HIP's code object; the symbols are then
// looked up by name in the executables the HSA loader holds for the handle's agent. No second code object exists.
//
// Ordering between the handle's two queues (its HIP stream and this AQL queue):
//  - before an AQL dispatch, everything enqueued on h->stream must be complete: every entry point that enqueues there marks the stream
//    dirty (host_entry), and the dispatch synchronises the stream when it is;
//  - before an entry point touches h->stream or the state, an AQL step still in flight is waited for (host_entry -> aql_wait).
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <hsa/hsa_ven_amd_loader.h>

// One kernel launch of a step: the kernel's host stub, its grid, and its explicit arguments packed the way the AMDGPU kernarg segment lays
// them out (each at its own alignment, in declaration order). The HIP path passes pointers into these bytes to hipLaunchKernel, the AQL
// path copies them into its kernarg block, so both launch the same kernel with the same bytes.
struct KLaunch {
  static constexpr uint32_t kCap = 1024;
  const void* fn = nullptr;
  dim3 grid, block;
  alignas(16) unsigned char args[kCap];
  uint32_t size = 0;
  void* argv[8];
  int argc = 0;
  template <class T> void arg(const T& v) {
    static_assert(sizeof(T) <= kCap, "kernel argument larger than the kernarg block");
    size = (size + (uint32_t)alignof(T) - 1) & ~((uint32_t)alignof(T) - 1);
    if (argc == 8 || size + sizeof(T) > kCap) { size = kCap + 1; return; }   // (refused by step_plan)
    memcpy(args + size, &v, sizeof(T));
    argv[argc++] = args + size;
    size += (uint32_t)sizeof(T);
  }
};
struct StepPlan {
  KLaunch k[2];      // hierarchical handles: controller kernel, then the step kernel; else the step kernel alone
  int n = 0;
  bool late = false;          // the step kernel is the one that reads tagged rows: they may be copied behind the doorbell (late_actions.hpp)
  const void* twin = nullptr; // the other kernel of that pair (plain <-> late), which takes the same argument bytes; null: there is none
};

struct AqlState {   // (plain bytes: ac_create zeroes the handle, which is the PENDING state)
  enum { PENDING = 0, READY = 1, HIP = -1 };
  int mode = PENDING;                    // PENDING until the first host step, READY once the queue is set up, HIP: pinned or fallen back
  char why[256];                         // mode HIP: AIRCOMBAT_DISPATCH=hip, or why the set-up failed or the queue faulted
  void set_hip(const std::string& reason) { mode = HIP; snprintf(why, sizeof why, "%s", reason.c_str()); }
  bool hsa_up = false;
  hsa_agent_t agent{};
  hsa_queue_t* q = nullptr;
  hsa_signal_t sig{};
  bool sig_ok = false;
  volatile int qerr = HSA_STATUS_SUCCESS;  // written by the queue's error callback
  struct Kern { const void* fn; uint64_t object; uint32_t group, priv, kernarg; } kern[2]{};
  int nkern = 0;
  Kern twin{};                           // the plan's twin of the step kernel (StepPlan::twin), dispatched in its place when the plan names it
  unsigned char* d_args = nullptr;       // [AC_HOST_SETS][2][KLaunch::kCap] in device memory
  unsigned char cached[AC_HOST_SETS][2][KLaunch::kCap];   // what each block holds
  bool have_block[AC_HOST_SETS]{};
  bool in_flight = false;
};

// the resolved kernel behind entry i of a plan: the one the queue was set up with, or its twin
static const AqlState::Kern* aql_kern(const AqlState* a, int i, const void* fn) {
  if (a->kern[i].fn == fn) return &a->kern[i];
  if (i == a->nkern - 1 && a->twin.fn && a->twin.fn == fn) return &a->twin;
  return nullptr;
}
static void aql_queue_error(hsa_status_t s, hsa_queue_t*, void* data) { ((AqlState*)data)->qerr = (int)s; }

static std::string hsa_msg(const char* what, hsa_status_t s) {
  const char* m = nullptr;
  hsa_status_string(s, &m);
  return std::string(what) + ": " + (m ? m : "unknown HSA status");
}

struct AqlAgentFind { uint32_t domain, bdf; hsa_agent_t agent; bool found; };
static hsa_status_t aql_on_agent(hsa_agent_t a, void* d) {
  AqlAgentFind* f = (AqlAgentFind*)d;
  hsa_device_type_t t;
  if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS || t != HSA_DEVICE_TYPE_GPU) return HSA_STATUS_SUCCESS;
  uint32_t bdf = 0, dom = 0;
  if (hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
  if (hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &dom) != HSA_STATUS_SUCCESS) dom = f->domain;
  if (bdf != f->bdf || dom != f->domain) return HSA_STATUS_SUCCESS;
  f->agent = a;
  f->found = true;
  return HSA_STATUS_INFO_BREAK;
}

struct AqlSymFind { hsa_agent_t agent; const char* name; AqlState::Kern* k; int hits; };
static hsa_status_t aql_on_symbol(hsa_executable_t, hsa_agent_t, hsa_executable_symbol_t sym, void* d) {
  AqlSymFind* f = (AqlSymFind*)d;
  hsa_symbol_kind_t kind;
  if (hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_TYPE, &kind) != HSA_STATUS_SUCCESS || kind != HSA_SYMBOL_KIND_KERNEL) return HSA_STATUS_SUCCESS;
  uint32_t len = 0;
  if (hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_NAME_LENGTH, &len) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
  std::string name(len, '\0');
  if (hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_NAME, &name[0]) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
  const std::string want = f->name;
  if (name != want && name != want + ".kd") return HSA_STATUS_SUCCESS;    // (the loader names a kernel by its descriptor symbol)
  if (f->hits++) return HSA_STATUS_SUCCESS;
  hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_OBJECT, &f->k->object);
  hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_GROUP_SEGMENT_SIZE, &f->k->group);
  hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_PRIVATE_SEGMENT_SIZE, &f->k->priv);
  hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_KERNARG_SEGMENT_SIZE, &f->k->kernarg);
  return HSA_STATUS_SUCCESS;
}
static hsa_status_t aql_on_executable(hsa_executable_t exe, void* d) {
  hsa_executable_iterate_agent_symbols(exe, ((AqlSymFind*)d)->agent, aql_on_symbol, d);
  return HSA_STATUS_SUCCESS;
}

// Set-up at the first host step after that step has gone through HIP (its code object is loaded then). An empty string is success; any
// other is the reason the handle stays on HIP. The caller releases what was made on failure (aql_release).
static std::string aql_setup(AqlState* a, int device, const StepPlan& plan) {
  hsa_status_t s = hsa_init();
  if (s != HSA_STATUS_SUCCESS) return hsa_msg("hsa_init", s);
  a->hsa_up = true;
  char pci[64];
  if (hipDeviceGetPCIBusId(pci, sizeof pci, device) != hipSuccess) return "hipDeviceGetPCIBusId failed";
  unsigned dom = 0, bus = 0, dev = 0, fn = 0;
  if (sscanf(pci, "%x:%x:%x.%x", &dom, &bus, &dev, &fn) != 4) return std::string("unexpected PCI bus id ") + pci;
  AqlAgentFind af{dom, (bus << 8) | (dev << 3) | fn, {}, false};
  hsa_iterate_agents(aql_on_agent, &af);
  if (!af.found) return std::string("no HSA GPU agent with PCI bus id ") + pci;
  a->agent = af.agent;
  hsa_ven_amd_loader_1_03_pfn_t loader;
  s = hsa_system_get_major_extension_table(HSA_EXTENSION_AMD_LOADER, 1, sizeof loader, &loader);
  if (s != HSA_STATUS_SUCCESS) return hsa_msg("AMD loader extension", s);
  a->nkern = plan.n;
  a->twin = AqlState::Kern{};
  for (int i = 0; i < plan.n + (plan.twin ? 1 : 0); ++i) {
    const bool tw = i == plan.n;           // (the twin takes the last kernel's arguments)
    const void* fn = tw ? plan.twin : plan.k[i].fn;
    const char* name = hipKernelNameRefByPtr(fn, nullptr);
    if (!name) return "hipKernelNameRefByPtr found no name for a step kernel";
    AqlState::Kern& k = tw ? a->twin : a->kern[i];
    k.fn = fn;
    AqlSymFind sf{a->agent, name, &k, 0};
    loader.hsa_ven_amd_loader_iterate_executables(aql_on_executable, &sf);
    if (sf.hits != 1) return std::string("kernel symbol ") + name + (sf.hits ? " is loaded more than once" : " not found among the loaded executables");
    // the kernels read no hidden arguments (no blockDim / gridDim / printf): their kernarg segment ends with the explicit arguments. A
    // kernel that grew one would read garbage from a block filled like this, so that is refused here rather than dispatched.
    const uint32_t want = plan.k[tw ? plan.n - 1 : i].size;
    if (k.kernarg != want) {
      char m[256];
      snprintf(m, sizeof m, "kernel %s: kernarg segment %u B, explicit arguments %u B (hidden arguments are not filled on this path)", name, k.kernarg, want);
      return m;
    }
  }
  s = hsa_queue_create(a->agent, 64, HSA_QUEUE_TYPE_SINGLE, aql_queue_error, a, UINT32_MAX, UINT32_MAX, &a->q);
  if (s != HSA_STATUS_SUCCESS) { a->q = nullptr; return hsa_msg("hsa_queue_create", s); }
  s = hsa_signal_create(0, 1, &a->agent, &a->sig);   // one GPU consumer: a plain memory signal, no interrupt event
  if (s != HSA_STATUS_SUCCESS) return hsa_msg("hsa_signal_create", s);
  a->sig_ok = true;
  if (hipMalloc((void**)&a->d_args, (size_t)AC_HOST_SETS * 2 * KLaunch::kCap) != hipSuccess) { a->d_args = nullptr; return "hipMalloc of the kernarg blocks failed"; }
  return "";
}
static void aql_release(AqlState* a) {
  if (a->d_args) (void)hipFree(a->d_args);
  if (a->sig_ok) hsa_signal_destroy(a->sig);
  if (a->q) hsa_queue_destroy(a->q);
  if (a->hsa_up) hsa_shut_down();
  a->d_args = nullptr; a->sig_ok = false; a->q = nullptr; a->hsa_up = false; a->in_flight = false;
}

// Write the plan's packets (barrier bit on each, so the step kernel of a hierarchical handle waits for its controller kernel) and ring the
// doorbell. The kernarg block of the host set is rewritten only when its bytes differ from what it holds.
static std::string aql_dispatch(AqlState* a, const StepPlan& plan, int set) {
  if (plan.n != a->nkern) return "the step's kernels changed after the AQL set-up";
  unsigned char* blk = a->d_args + (size_t)set * 2 * KLaunch::kCap;
  for (int i = 0; i < plan.n; ++i)
    if (!aql_kern(a, i, plan.k[i].fn)) return "the step's kernels changed after the AQL set-up";
  bool same = a->have_block[set];
  for (int i = 0; i < plan.n && same; ++i) same = memcmp(a->cached[set][i], plan.k[i].args, plan.k[i].size) == 0;
  if (!same) {   // first use of the set, or a buffer behind it was reallocated
    for (int i = 0; i < plan.n; ++i) {
      if (hipMemcpy(blk + (size_t)i * KLaunch::kCap, plan.k[i].args, plan.k[i].size, hipMemcpyHostToDevice) != hipSuccess) return "hipMemcpy of a kernarg block failed";
      memcpy(a->cached[set][i], plan.k[i].args, plan.k[i].size);
    }
    a->have_block[set] = true;
  }
  hsa_queue_t* q = a->q;
  const uint64_t idx = hsa_queue_load_write_index_relaxed(q);
  while (idx + plan.n - hsa_queue_load_read_index_scacquire(q) > q->size) {}   // (one step in flight at most: never waits in practice)
  hsa_signal_store_relaxed(a->sig, 1);
  uint32_t hdr[2];
  for (int i = 0; i < plan.n; ++i) {
    const KLaunch& k = plan.k[i];
    const AqlState::Kern& kk = *aql_kern(a, i, plan.k[i].fn);
    hsa_kernel_dispatch_packet_t* p = (hsa_kernel_dispatch_packet_t*)q->base_address + ((idx + i) & (q->size - 1));
    memset((char*)p + 4, 0, sizeof *p - 4);   // (the header word stays INVALID until the body is complete)
    p->workgroup_size_x = (uint16_t)k.block.x; p->workgroup_size_y = 1; p->workgroup_size_z = 1;
    p->grid_size_x = k.grid.x * k.block.x; p->grid_size_y = 1; p->grid_size_z = 1;
    p->private_segment_size = kk.priv;      // (the two-waves-per-SIMD forms use scratch: the queue allocates it on demand)
    p->group_segment_size = kk.group;
    p->kernel_object = kk.object;
    p->kernarg_address = blk + (size_t)i * KLaunch::kCap;
    const bool last = i == plan.n - 1;
    if (last) p->completion_signal = a->sig;
    // system scope on the step's ends: the actions come from host memory, the outputs go to host memory a host thread reads next;
    // agent scope between the controller kernel and the step kernel, as between two kernels of one stream
    const int acq = i == 0 ? HSA_FENCE_SCOPE_SYSTEM : HSA_FENCE_SCOPE_AGENT, rel = last ? HSA_FENCE_SCOPE_SYSTEM : HSA_FENCE_SCOPE_AGENT;
    hdr[i] = (uint32_t)((HSA_PACKET_TYPE_KERNEL_DISPATCH << HSA_PACKET_HEADER_TYPE) | (1 << HSA_PACKET_HEADER_BARRIER) |
                        (acq << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) | (rel << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE)) |
             ((uint32_t)(1 << HSA_KERNEL_DISPATCH_PACKET_SETUP_DIMENSIONS) << 16);
  }
  hsa_queue_store_write_index_relaxed(q, idx + plan.n);
  for (int i = 0; i < plan.n; ++i)
    __atomic_store_n((uint32_t*)((hsa_kernel_dispatch_packet_t*)q->base_address + ((idx + i) & (q->size - 1))), hdr[i], __ATOMIC_RELEASE);
  hsa_signal_store_screlease(q->doorbell_signal, (hsa_signal_value_t)(idx + plan.n - 1));
  a->in_flight = true;
  return "";
}

// Busy-wait for the dispatched step against a wall-clock deadline. A deadline passed or a queue error is returned as a message; the queue
// is not used again after either.
static std::string aql_wait(AqlState* a, double deadline_s = 10.0) {
  if (!a->in_flight) return "";
  const auto t0 = std::chrono::steady_clock::now();
  unsigned spins = 0;
  while (hsa_signal_load_scacquire(a->sig) != 0) {
    if (a->qerr != HSA_STATUS_SUCCESS) { a->in_flight = false; return hsa_msg("AQL step queue error", (hsa_status_t)a->qerr); }
    if ((++spins & 1023) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > deadline_s) {
      a->in_flight = false;
      return "AQL step did not complete within 10 s";
    }
  }
  a->in_flight = false;
  return "";
}
