// Test access to the two device missile integrators, one level above math_probe.hpp: one lane per row runs `ticks` consecutive calls of the
// production missile_run (no formula is restated here) from a caller-supplied launch row against a caller-supplied target table, with the
// handle's DevCfg, and writes the whole munition record after every tick, so that each tick can be held to a CPU reference
// (tests/missile_probe_util.py, tests/test_gpu_missile_probe.py). Row layouts, forms and models: include/aircombat.h.
// form 0 = MslT<float> (its arguments are cast to float as the 1v1 step kernel's are, its results widened exactly), form 1 = the MslD
// overload. Like the step kernels, a row that reports HIT on a live target sees that target dead from then on, and a finished missile
// keeps being run. Included by aircombat.hip.
#pragma once

__device__ __forceinline__ int probe_missile_tick(Msl& m, const MslParam& P, const double* t, bool alive, const DevCfg& c) {
  missile_run(m, P, (float)t[0], (float)t[1], (float)t[2], (float)t[3], (float)t[4], (float)t[5], alive, c);
  return -1;   // (the fp32 form reports nothing)
}
__device__ __forceinline__ int probe_missile_tick(MslD& m, const MslParam& P, const double* t, bool alive, const DevCfg& c) {
  return missile_run(m, P, t[0], t[1], t[2], t[3], t[4], t[5], alive, c) ? 1 : 0;
}
template <typename R>
__device__ __forceinline__ void probe_missile_row(const DevCfg& c, const MslParam& P, int n, int ticks, int row, const double* __restrict__ launch,
                                                  const double* __restrict__ target, double* __restrict__ out) {
  const double* L = launch + (size_t)row * AC_PROBE_MSL_IN;
  MslT<R> m;
  m.px = (R)L[0]; m.py = (R)L[1]; m.pz = (R)L[2]; m.vx = (R)L[3]; m.vy = (R)L[4]; m.vz = (R)L[5];
  m.theta = (R)L[6]; m.psi = (R)L[7]; m.t = (R)L[8]; m.m = (R)L[9]; m.dth = (R)L[10]; m.dph = (R)L[11]; m.dprev = (R)L[12];
  m.recede = (int)L[13]; m.status = (int)L[14]; m.order = 0; m.dpos = 0; m.model = 0;
  bool shot = false;   // this row's target went down to this row's missile
  for (int k = 0; k < ticks; ++k) {
    const double* t = target + ((size_t)k * n + row) * AC_PROBE_MSL_TGT;
    const bool alive = t[6] != 0.0 && !shot;
    const int moved = probe_missile_tick(m, P, t, alive, c);
    if (m.status == MSL_HIT && alive) shot = true;
    double* o = out + ((size_t)k * n + row) * AC_PROBE_MSL_OUT;
    o[0] = (double)m.status;
    o[1] = (double)m.px; o[2] = (double)m.py; o[3] = (double)m.pz; o[4] = (double)m.vx; o[5] = (double)m.vy; o[6] = (double)m.vz;
    o[7] = (double)m.theta; o[8] = (double)m.psi; o[9] = (double)m.t; o[10] = (double)m.m; o[11] = (double)m.dth; o[12] = (double)m.dph;
    o[13] = (double)m.dprev; o[14] = (double)m.recede; o[15] = (double)moved;
  }
}

__global__ void __launch_bounds__(64) missile_probe_kernel(DevCfg c, int form, int model, int n, int ticks, const double* __restrict__ launch,
                                                           const double* __restrict__ target, double* __restrict__ out) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const MslParam P = model == AC_PROBE_MSL_AIM120B ? aim120b() : aim9l();
  if (form == AC_PROBE_MSL_FP32) probe_missile_row<float>(c, P, n, ticks, row, launch, target, out);
  else probe_missile_row<double>(c, P, n, ticks, row, launch, target, out);
}

extern "C" int ac_probe_missile(ac_env_t* h, int32_t form, int32_t model, int32_t n, int32_t ticks, const double* launch, const double* target,
                                double* out) {
  // (the arguments first, the handle last: every refusal but the last can be seen without a GPU)
  if (!launch || !target || !out) return fail("ac_probe_missile: null argument");
  if (form != AC_PROBE_MSL_FP32 && form != AC_PROBE_MSL_FP64) return fail("ac_probe_missile: unknown form");
  if (model != AC_PROBE_MSL_AIM9L && model != AC_PROBE_MSL_AIM120B) return fail("ac_probe_missile: unknown model");
  if (form == AC_PROBE_MSL_FP32 && model == AC_PROBE_MSL_AIM120B) return fail("ac_probe_missile: no step kernel flies the AIM-120B set in fp32");
  if (n <= 0 || n > AC_PROBE_MSL_MAX_ROWS) return fail("ac_probe_missile: n out of range");
  if (ticks <= 0 || ticks > AC_PROBE_MSL_MAX_TICKS) return fail("ac_probe_missile: ticks out of range");
  if ((int64_t)n * ticks > AC_PROBE_MSL_MAX_CELLS) return fail("ac_probe_missile: n * ticks out of range");
  if (!h) return fail("ac_probe_missile: null handle");
  if (host_entry(h)) return -1;
  HIP_OK(hipSetDevice(h->device));
  const size_t cells = (size_t)n * (size_t)ticks;
  const size_t bl = sizeof(double) * AC_PROBE_MSL_IN * (size_t)n, bt = sizeof(double) * AC_PROBE_MSL_TGT * cells, bo = sizeof(double) * AC_PROBE_MSL_OUT * cells;
  double *dl = nullptr, *dt = nullptr, *dout = nullptr;
  hipError_t err = hipMalloc(&dl, bl);
  if (err == hipSuccess) err = hipMalloc(&dt, bt);
  if (err == hipSuccess) err = hipMalloc(&dout, bo);
  if (err == hipSuccess) err = hipMemcpyAsync(dl, launch, bl, hipMemcpyHostToDevice, h->stream);
  if (err == hipSuccess) err = hipMemcpyAsync(dt, target, bt, hipMemcpyHostToDevice, h->stream);
  if (err == hipSuccess) {
    hipLaunchKernelGGL(missile_probe_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, h->dc, (int)form, (int)model, (int)n, (int)ticks,
                       dl, dt, dout);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipMemcpyAsync(out, dout, bo, hipMemcpyDeviceToHost, h->stream);
  const hipError_t sync = hipStreamSynchronize(h->stream);   // (also on an error: nothing may still use the buffers when they are freed)
  if (err == hipSuccess) err = sync;
  if (dl) (void)hipFree(dl);
  if (dt) (void)hipFree(dt);
  if (dout) (void)hipFree(dout);
  if (err != hipSuccess) return fail(std::string("ac_probe_missile: ") + hipGetErrorString(err));
  return 0;
}
