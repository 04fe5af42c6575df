// Micro-benchmark behind the AQL host-step dispatch: what does the HIP runtime's launch + hipStreamSynchronize cost
// per host step, against writing one AQL kernel-dispatch packet into a queue the program owns and busy-waiting on its completion signal?
// Same stand-in as host_io.hip: 8192 lanes, a dependent FMA chain of ~17 us, actions read from and outputs written to mapped host memory
// through the LDS-transposed stores.
//   (a) hipLaunchKernelGGL + hipStreamSynchronize                                   (the HIP path of ac_step_host)
//   (b) AQL packet on an HSA queue of our own, kernargs written once into device memory, active wait on the completion signal
//   (c) like (b), but the kernargs are rewritten (hipMemcpy) before every step    (separates the kernarg upload from the submission)
// Each is run with an empty body (iters = 0) and the ~17 us body, the variants alternating in rounds within one process.
//   hipcc --offload-arch=gfx950 -O3 -o aql_dispatch aql_dispatch.hip -lhsa-runtime64 && ./aql_dispatch [steps] [iters]
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <hsa/hsa_ven_amd_loader.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <string>
#include <algorithm>
#include <vector>
#define OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)
#define HOK(x) do { hsa_status_t s_ = (x); if (s_ != HSA_STATUS_SUCCESS) { const char* m_ = ""; hsa_status_string(s_, &m_); printf("%s: %s\n", #x, m_); exit(1); } } while (0)
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

constexpr int N = 8192, OBS = 15, ACT = 4;
__device__ __forceinline__ float spin(float x, int iters) { for (int i = 0; i < iters; ++i) x = x * 1.0000001f + 1e-9f; return x; }

__global__ void k_coalesced(const float4* act, float* obs, float* rew, unsigned char* done, int iters) {
  __shared__ float L[64 * OBS];
  int n = blockIdx.x * 64 + threadIdx.x;
  float4 a = act[n];
  float x = a.x + a.y + a.z + a.w;
  x = spin(x, iters);
  for (int k = 0; k < OBS; ++k) L[threadIdx.x * OBS + k] = x + k;
  __syncthreads();
  float4* o4 = reinterpret_cast<float4*>(obs + (size_t)blockIdx.x * 64 * OBS);
  const float4* l4 = reinterpret_cast<const float4*>(L);
  for (int i = threadIdx.x; i < 64 * OBS / 4; i += 64) o4[i] = l4[i];
  rew[n] = x;
  unsigned long long b = __ballot(x > 1e30f);
  if (threadIdx.x < 16) reinterpret_cast<unsigned*>(done + blockIdx.x * 64)[threadIdx.x] = (unsigned)((b >> (4 * threadIdx.x)) & 1);
}

struct Args { const float4* act; float* obs; float* rew; unsigned char* done; int iters; int pad; };
static_assert(sizeof(Args) == 40, "explicit kernarg layout of k_coalesced");

struct Find { std::string want; hsa_agent_t agent; uint64_t object = 0; uint32_t group = 0, priv = 0, kernarg = 0; };
static hsa_status_t on_symbol(hsa_executable_t, hsa_agent_t, hsa_executable_symbol_t sym, void* d) {
  Find* f = (Find*)d;
  hsa_symbol_kind_t kind;
  HOK(hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_TYPE, &kind));
  if (kind != HSA_SYMBOL_KIND_KERNEL) return HSA_STATUS_SUCCESS;
  uint32_t len = 0;
  HOK(hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_NAME_LENGTH, &len));
  std::string name(len, '\0');
  HOK(hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_NAME, &name[0]));
  if (name != f->want && name != f->want + ".kd") return HSA_STATUS_SUCCESS;
  HOK(hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_OBJECT, &f->object));
  HOK(hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_GROUP_SEGMENT_SIZE, &f->group));
  HOK(hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_PRIVATE_SEGMENT_SIZE, &f->priv));
  HOK(hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_KERNARG_SEGMENT_SIZE, &f->kernarg));
  return HSA_STATUS_INFO_BREAK;
}
static hsa_ven_amd_loader_1_03_pfn_t g_loader;
static hsa_status_t on_executable(hsa_executable_t exe, void* d) {
  Find* f = (Find*)d;
  hsa_status_t s = hsa_executable_iterate_agent_symbols(exe, f->agent, on_symbol, d);
  return s == HSA_STATUS_INFO_BREAK ? s : HSA_STATUS_SUCCESS;
}
struct AgentFind { uint32_t bdf; hsa_agent_t agent; bool found = false; };
static hsa_status_t on_agent(hsa_agent_t a, void* d) {
  AgentFind* f = (AgentFind*)d;
  hsa_device_type_t t;
  HOK(hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t));
  if (t != HSA_DEVICE_TYPE_GPU) return HSA_STATUS_SUCCESS;
  uint32_t bdf = 0;
  HOK(hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf));
  if (bdf != f->bdf) return HSA_STATUS_SUCCESS;
  f->agent = a; f->found = true;
  return HSA_STATUS_INFO_BREAK;
}
static void on_queue_error(hsa_status_t s, hsa_queue_t*, void*) { const char* m = ""; hsa_status_string(s, &m); printf("queue error: %s\n", m); exit(1); }

int main(int argc, char** argv) {
  const int R = argc > 1 ? atoi(argv[1]) : 3000;
  const int iters17 = argc > 2 ? atoi(argv[2]) : 1000;
  OK(hipSetDevice(0));
  hipStream_t s; OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  float *h_act, *h_obs, *h_rew; unsigned char* h_done;
  const unsigned flags = hipHostMallocMapped | hipHostMallocNonCoherent;
  OK(hipHostMalloc(&h_act, N * ACT * 4, flags)); OK(hipHostMalloc(&h_obs, N * OBS * 4, flags));
  OK(hipHostMalloc(&h_rew, N * 4, flags)); OK(hipHostMalloc(&h_done, N, flags));
  for (int i = 0; i < N * ACT; ++i) h_act[i] = (float)(i % 41) * 1e-3f;
  float *m_act, *m_obs, *m_rew; unsigned char* m_done;
  OK(hipHostGetDevicePointer((void**)&m_act, h_act, 0)); OK(hipHostGetDevicePointer((void**)&m_obs, h_obs, 0));
  OK(hipHostGetDevicePointer((void**)&m_rew, h_rew, 0)); OK(hipHostGetDevicePointer((void**)&m_done, h_done, 0));
  // first launch through HIP: loads HIP's code object, so its executable holds the kernel from here on
  hipLaunchKernelGGL(k_coalesced, dim3(N / 64), dim3(64), 0, s, (const float4*)m_act, m_obs, m_rew, m_done, 0);
  OK(hipStreamSynchronize(s));

  HOK(hsa_init());
  char pci[64];
  OK(hipDeviceGetPCIBusId(pci, sizeof pci, 0));
  unsigned dom = 0, bus = 0, dev = 0, fn = 0;
  if (sscanf(pci, "%x:%x:%x.%x", &dom, &bus, &dev, &fn) != 4) { printf("bad PCI id %s\n", pci); return 1; }
  AgentFind af; af.bdf = (bus << 8) | (dev << 3) | fn;
  hsa_iterate_agents(on_agent, &af);
  if (!af.found) { printf("no HSA agent with PCI id %s\n", pci); return 1; }
  HOK(hsa_system_get_major_extension_table(HSA_EXTENSION_AMD_LOADER, 1, sizeof g_loader, &g_loader));
  Find kf; kf.want = "_Z11k_coalescedPK15HIP_vector_typeIfLj4EEPfS3_Phi"; kf.agent = af.agent;
  g_loader.hsa_ven_amd_loader_iterate_executables(on_executable, &kf);
  if (!kf.object) { printf("kernel symbol %s not found among the loaded executables\n", kf.want.c_str()); return 1; }
  printf("PCI %s  kernel object %#llx  group %u B  private %u B  kernarg %u B\n", pci, (unsigned long long)kf.object, kf.group, kf.priv, kf.kernarg);
  if (kf.kernarg > sizeof(Args)) { printf("kernel reads hidden arguments (%u B kernarg segment), the stand-in does not fill them\n", kf.kernarg); return 1; }

  hsa_queue_t* q = nullptr;
  HOK(hsa_queue_create(af.agent, 64, HSA_QUEUE_TYPE_SINGLE, on_queue_error, nullptr, UINT32_MAX, UINT32_MAX, &q));
  hsa_signal_t sig;
  HOK(hsa_signal_create(0, 1, &af.agent, &sig));   // one GPU consumer: a plain memory signal, no interrupt event
  void* d_args = nullptr;
  OK(hipMalloc(&d_args, 256));

  auto dispatch = [&](int iters, bool rewrite) {
    if (rewrite) { Args a{(const float4*)m_act, m_obs, m_rew, m_done, iters, 0}; OK(hipMemcpy(d_args, &a, sizeof a, hipMemcpyHostToDevice)); }
    const uint64_t idx = hsa_queue_load_write_index_relaxed(q);
    while (idx - hsa_queue_load_read_index_scacquire(q) >= q->size) {}
    hsa_kernel_dispatch_packet_t* p = (hsa_kernel_dispatch_packet_t*)q->base_address + (idx & (q->size - 1));
    memset((char*)p + 4, 0, sizeof *p - 4);
    p->workgroup_size_x = 64; p->workgroup_size_y = 1; p->workgroup_size_z = 1;
    p->grid_size_x = N; p->grid_size_y = 1; p->grid_size_z = 1;
    p->private_segment_size = kf.priv; p->group_segment_size = kf.group;
    p->kernel_object = kf.object; p->kernarg_address = d_args; p->completion_signal = sig;
    hsa_signal_store_relaxed(sig, 1);
    const uint16_t header = (HSA_PACKET_TYPE_KERNEL_DISPATCH << HSA_PACKET_HEADER_TYPE) | (1 << HSA_PACKET_HEADER_BARRIER) |
                            (HSA_FENCE_SCOPE_SYSTEM << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) | (HSA_FENCE_SCOPE_SYSTEM << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE);
    const uint16_t setup = 1 << HSA_KERNEL_DISPATCH_PACKET_SETUP_DIMENSIONS;
    hsa_queue_store_write_index_relaxed(q, idx + 1);
    __atomic_store_n((uint32_t*)p, (uint32_t)header | ((uint32_t)setup << 16), __ATOMIC_RELEASE);
    hsa_signal_store_screlease(q->doorbell_signal, idx);
    const double dl = now() + 10.0;
    while (hsa_signal_load_scacquire(sig) != 0) if (now() > dl) { printf("AQL dispatch did not complete within 10 s\n"); exit(1); }
  };
  auto hip_step = [&](int iters) {
    hipLaunchKernelGGL(k_coalesced, dim3(N / 64), dim3(64), 0, s, (const float4*)m_act, m_obs, m_rew, m_done, iters);
    OK(hipStreamSynchronize(s));
  };

  // correctness: the AQL path writes what the HIP path writes
  std::vector<float> ref(N * OBS);
  hip_step(100); memcpy(ref.data(), h_obs, ref.size() * 4);
  memset(h_obs, 0, N * OBS * 4);
  dispatch(100, true);
  if (memcmp(ref.data(), h_obs, ref.size() * 4)) { printf("AQL outputs differ from the HIP outputs\n"); return 1; }

  const char* names[3] = {"(a) hipLaunchKernelGGL + hipStreamSynchronize", "(b) AQL packet, kernargs written once, spin on signal",
                          "(c) AQL packet, kernargs rewritten every step"};
  const int ROUNDS = 6, per = std::max(R / ROUNDS, 1);
  for (int body = 0; body < 2; ++body) {
    const int iters = body ? iters17 : 0;
    { Args a{(const float4*)m_act, m_obs, m_rew, m_done, iters, 0}; OK(hipMemcpy(d_args, &a, sizeof a, hipMemcpyHostToDevice)); }
    for (int v = 0; v < 3; ++v) for (int w = 0; w < 200; ++w) { if (v == 0) hip_step(iters); else dispatch(iters, v == 2); }
    std::vector<double> tot(3, 0.0);
    std::vector<std::vector<double>> rounds(3);
    for (int r = 0; r < ROUNDS; ++r)
      for (int v = 0; v < 3; ++v) {
        if (v == 1) { Args a{(const float4*)m_act, m_obs, m_rew, m_done, iters, 0}; OK(hipMemcpy(d_args, &a, sizeof a, hipMemcpyHostToDevice)); }
        const double t0 = now();
        for (int i = 0; i < per; ++i) { if (v == 0) hip_step(iters); else dispatch(iters, v == 2); }
        const double dt = now() - t0;
        tot[v] += dt; rounds[v].push_back(dt / per * 1e6);
      }
    printf("---- body: %s (iters %d), %d steps per variant in %d alternating rounds\n", body ? "~17 us FMA chain" : "empty", iters, per * ROUNDS, ROUNDS);
    for (int v = 0; v < 3; ++v) {
      std::sort(rounds[v].begin(), rounds[v].end());
      printf("%-56s %7.2f us/step  (rounds min %.2f max %.2f)\n", names[v], tot[v] / (per * ROUNDS) * 1e6, rounds[v].front(), rounds[v].back());
    }
    printf("(a) - (b) = %.2f us/step\n", (tot[0] - tot[1]) / (per * ROUNDS) * 1e6);
  }
  float chk = 0; for (int i = 0; i < N * OBS; ++i) chk += h_obs[i];
  printf("checksum %g\n", chk);
  HOK(hsa_signal_destroy(sig)); HOK(hsa_queue_destroy(q));
  OK(hipFree(d_args));
  OK(hipHostFree(h_act)); OK(hipHostFree(h_obs)); OK(hipHostFree(h_rew)); OK(hipHostFree(h_done));
  HOK(hsa_shut_down());
  return 0;
}
