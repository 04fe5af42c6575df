// fp64 primitives for the munition path and the geodetic reductions: the reference flies its missiles in Python floats, and a 5 m
// fuse against ~25 m of relative travel per tick makes hit-or-miss hinge on centimetres of a 300-tick integration, so those
// updates stay in fp64 on the device -- but the library's division / sqrt / exp / sin are correctly-rounded, special-case-proof
// sequences of 25-200 instructions each, and one munition update held ~20 of them. These forms keep a relative error of one or two
// ulp (the hardware seed refined by two Newton steps, a Cody-Waite reduction, Taylor polynomials on a small range) for the finite,
// ordinary arguments these call sites produce, at 5-15 instructions each. In units of 2^-53 = 1.1e-16, with exact fused multiply-adds
// (tests/math_probe_util.py): rcp 1.0, sqrt 1.0, rsqrt 2.1 relative for 1e-6 <= x <= 1e16; sincos 1.1 absolute and 1.9 relative for
// |x| <= 8 pi. tests/test_gpu_math_probe.py holds the device to twice these figures.
#pragma once

namespace fx {

__device__ __forceinline__ double rcp(double x) {          // v_rcp_f64 (>= 26 bits) + two Newton-Raphson steps
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  r = fma(fma(-x, r, 1.0), r, r);
  return r;
}
__device__ __forceinline__ double rsqrt(double x) {         // v_rsq_f64 + two Newton-Raphson steps (x > 0)
  double r = __builtin_amdgcn_rsq(x);
  const double h = 0.5 * x;
  r = r * fma(-h * r, r, 1.5);
  r = r * fma(-h * r, r, 1.5);
  return r;
}
__device__ __forceinline__ double sqrt(double x) {          // x >= 0
  const double r = rsqrt(x), s = x * r;
  const double y = fma(fma(-s, s, x), 0.5 * r, s);
  return x > 0.0 ? y : 0.0;
}
// sqrt(x) and 1 / sqrt(x) from the one refined seed (x > 0): the callers that divide by a length they also need
__device__ __forceinline__ void sqrt_both(double x, double* s_out, double* r_out) {
  const double r = rsqrt(x), s = x * r;
  *s_out = fma(fma(-s, s, x), 0.5 * r, s);
  *r_out = r;
}
// sin and cos together for |x| up to a few turns (a missile's pitch and heading): reduction by the nearest multiple of pi / 2 in two
// pieces, Taylor series on [-pi/4, pi/4] to y^17 and y^16 (the first terms left out are 8e-20 and 2e-18 at pi/4), quadrant swap
__device__ __forceinline__ void sincos(double x, double* sn, double* cs) {
  const double n = rint(x * 0.63661977236758134308);
  double y = fma(-n, 1.5707963267948965580, x);
  y = fma(-n, 6.1232339957367660e-17, y);
  const double t = y * y;
  double ps = 2.8114572543455206e-15;                       //  1/17!
  ps = fma(ps, t, -7.6471637318198164e-13);                 // -1/15!
  ps = fma(ps, t, 1.6059043836821613e-10);                  //  1/13!
  ps = fma(ps, t, -2.5052108385441720e-08);                 // -1/11!
  ps = fma(ps, t, 2.7557319223985893e-06);                  //  1/9!
  ps = fma(ps, t, -1.9841269841269841e-04);                 // -1/7!
  ps = fma(ps, t, 8.3333333333333332e-03);                  //  1/5!
  ps = fma(ps, t, -1.6666666666666666e-01);                 // -1/3!
  const double s0 = fma(y * t, ps, y);
  double pc = 4.7794773323873853e-14;                       //  1/16!  (1.0e-15 at |y| = pi/4: it cannot be dropped)
  pc = fma(pc, t, -1.1470745597729725e-11);                 // -1/14!
  pc = fma(pc, t, 2.0876756987868100e-09);                  //  1/12!
  pc = fma(pc, t, -2.7557319223985888e-07);                 // -1/10!
  pc = fma(pc, t, 2.4801587301587302e-05);                  //  1/8!
  pc = fma(pc, t, -1.3888888888888889e-03);                 // -1/6!
  pc = fma(pc, t, 4.1666666666666664e-02);                  //  1/4!
  pc = fma(pc, t, -0.5);
  const double c0 = fma(t, pc, 1.0);
  const long long q = (long long)n & 3;
  const double s1 = (q & 1) ? c0 : s0, c1 = (q & 1) ? s0 : c0;
  *sn = (q == 2 || q == 3) ? -s1 : s1;
  *cs = (q == 1 || q == 2) ? -c1 : c1;
}

}  // namespace fx
