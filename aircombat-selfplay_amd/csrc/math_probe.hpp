// Test access to the device math primitives the step kernels rest on: one kernel that calls the very inline functions the step kernels
// call (no formula is restated here) on rows of caller-supplied arguments, so that each can be held to its own accuracy bound against a
// high-precision reference (tests/math_probe_util.py, tests/test_gpu_math_probe.py). Row layout and ops: include/aircombat.h.
// fp32 ops cast their arguments to float (the tests pass float32-exact values) and widen their results exactly.
// Included by aircombat.hip.
#pragma once

__global__ void __launch_bounds__(256) math_probe_kernel(DevCfg c, int op, long long n, const double* __restrict__ in, double* __restrict__ out) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const double* x = in + row * AC_PROBE_IN;
  double* o = out + row * AC_PROBE_OUT;
  const double a0 = x[0], a1 = x[1], a2 = x[2], a3 = x[3], a4 = x[4];
  const float f0 = (float)a0, f1 = (float)a1, f2 = (float)a2, f3 = (float)a3, f4 = (float)a4;
  double r[AC_PROBE_OUT];
#pragma unroll
  for (int k = 0; k < AC_PROBE_OUT; ++k) r[k] = 0.0;
  switch (op) {
    case AC_PROBE_FX_RCP: r[0] = fx::rcp(a0); break;
    case AC_PROBE_FX_RSQRT: r[0] = fx::rsqrt(a0); break;
    case AC_PROBE_FX_SQRT: r[0] = fx::sqrt(a0); break;
    case AC_PROBE_FX_SQRT_BOTH: fx::sqrt_both(a0, &r[0], &r[1]); break;
    case AC_PROBE_FX_SINCOS: fx::sincos(a0, &r[0], &r[1]); break;
    case AC_PROBE_ATAN2_FAST: r[0] = (double)f16::atan2_fast(f0, f1); break;
    case AC_PROBE_ACOS_FAST: r[0] = (double)acos_fast(f0); break;
    case AC_PROBE_POW_POS: r[0] = (double)f16::pow_pos(f0, f1); break;
    case AC_PROBE_TANH_FAST: r[0] = (double)tanh_fast(f0); break;
    case AC_PROBE_ATANH_FAST: r[0] = (double)atanh_fast(f0); break;
    case AC_PROBE_SIGMOID_F: r[0] = (double)ctl::sigmoid_f(f0); break;
    case AC_PROBE_TANH_F: r[0] = (double)ctl::tanh_f(f0); break;
    case AC_PROBE_ATMOSPHERE: {
      const f16::Atmos A = f16::atmosphere(f0);
      r[0] = (double)A.T; r[1] = (double)A.P; r[2] = (double)A.rho; r[3] = (double)A.a;
    } break;
    case AC_PROBE_PITOT: r[0] = (double)f16::pitot_impact_pressure(f0, f1); break;
    case AC_PROBE_VCAS: r[0] = (double)f16::vcas_from_impact_pressure(f0); break;
    case AC_PROBE_IN_RANGE_DEG: r[0] = (double)in_range_deg_f(f0); break;
    case AC_PROBE_IN_RANGE_RAD: r[0] = (double)ctl::in_range_rad_f(f0); break;
    case AC_PROBE_SLEW: r[0] = (double)f16::slew(f0, f1, f2, f3, f4); break;
    case AC_PROBE_TEF_KINEMATIC: r[0] = (double)f16::tef_kinematic(f0, f1); break;
    case AC_PROBE_SEEK: r[0] = (double)f16::seek(f0, f1, f2, f3, f4); break;
    case AC_PROBE_POSTURE_FN: r[0] = (double)posture_fn(f0, f1, f2); break;
    case AC_PROBE_MISSILE_HEIGHT_F: r[0] = (double)missile_height(f0, f1, f2, c); break;
    case AC_PROBE_MISSILE_HEIGHT_D: r[0] = missile_height(a0, a1, a2, c); break;
    case AC_PROBE_NEU_HEIGHT64: r[0] = neu_height64(a0, a1, a2, c); break;
    case AC_PROBE_LOCATE:
    case AC_PROBE_LOCATE_FAST: {
      f16::State s = {};
      f16::Derived d = {};
      s.rx = a0; s.ry = a1; s.rz = a2; s.ticks = (int)a3;
      if (op == AC_PROBE_LOCATE) f16::locate(s, d); else f16::locate_fast(s, d);
      r[0] = (double)d.h_sl_ft;
#pragma unroll
      for (int k = 0; k < 3; ++k) { r[1 + k] = (double)d.n_eci[k]; r[4 + k] = (double)d.e_eci[k]; r[7 + k] = (double)d.d_eci[k]; }
    } break;
    default: break;
  }
#pragma unroll
  for (int k = 0; k < AC_PROBE_OUT; ++k) o[k] = r[k];
}

extern "C" int ac_probe_math(ac_env_t* h, int32_t op, int64_t n, const double* in, double* out) {
  if (!h) return fail("ac_probe_math: null handle");
  if (!in || !out) return fail("ac_probe_math: null argument");
  if (op < 0 || op >= AC_PROBE_NOPS) return fail("ac_probe_math: unknown op");
  if (n <= 0 || n > AC_PROBE_MAX_ROWS) return fail("ac_probe_math: n out of range");
  if (host_entry(h)) return -1;
  HIP_OK(hipSetDevice(h->device));
  const size_t bin = sizeof(double) * AC_PROBE_IN * (size_t)n, bout = sizeof(double) * AC_PROBE_OUT * (size_t)n;
  double *din = nullptr, *dout = nullptr;
  hipError_t err = hipMalloc(&din, bin);
  if (err == hipSuccess) err = hipMalloc(&dout, bout);
  if (err == hipSuccess) err = hipMemcpyAsync(din, in, bin, hipMemcpyHostToDevice, h->stream);
  if (err == hipSuccess) {
    hipLaunchKernelGGL(math_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->dc, (int)op, (long long)n, din, dout);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipMemcpyAsync(out, dout, bout, hipMemcpyDeviceToHost, h->stream);
  const hipError_t sync = hipStreamSynchronize(h->stream);   // (also on an error: nothing may still use the buffers when they are freed)
  if (err == hipSuccess) err = sync;
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  if (err != hipSuccess) return fail(std::string("ac_probe_math: ") + hipGetErrorString(err));
  return 0;
}
