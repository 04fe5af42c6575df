"""References, CPU twins, input sets and bounds for the device math primitives (ac_probe_math, include/aircombat.h).

For every op of capi.AC_PROBE_OPS this module holds

* a REFERENCE: plain float64 (or mpmath where float64 is not enough) written from the formula the op implements -- the 1976 standard
  atmosphere, JSBSim's pitot / Rayleigh relations and their 10-step inverse, the exact ellipsoidal height, utils.py's angle wraps,
  FGKinemat -- never from the kernel. Where the reference of an fp64 op has to be better than float64 it is a (hi, lo) pair.
* a CPU TWIN: the op's own operations in its own order and precision. Every fma is exact (fma64 / fma32 below); an expression of the
  form a * b + c is taken as one fma, which is what the device compiler makes of it (-ffp-contract=fast, the HIP default). Where the
  device uses a hardware approximation (v_rcp_f32, v_rsq_f32, v_sqrt_f32, v_log_f32, v_exp_f32, the fp32 divide, which the build's
  -fno-hip-fp32-correctly-rounded-divide-sqrt turns into v_rcp_f32 and a multiply, and the fp64 seeds v_rcp_f64 / v_rsq_f64) the twin
  uses the correctly rounded value; the fp64 seeds are rounded to float32 (two Newton steps erase the seed).
* an INPUT SET: seeded, small, the range the call sites produce plus the edges.
* a SCALE per row and output, so that |error| / scale is one figure per op and output: 1 for an absolute bound, |reference| for a relative
  one, a sensitivity where the op is ill-conditioned in part of its range.
* the BOUND  B = 2 x (the twin's worst figure over the input set) + A.  The twin's figure stands in TWIN below and is recomputed by
  tests/test_math_probe_host.py (the copy must be within 5 %). A is the allowance for the hardware approximations alone: 1 ulp each
  (the CDNA ISA guide's figure for V_RCP_F32, V_RSQ_F32, V_SQRT_F32, V_LOG_F32 and V_EXP_F32), i.e. at most U = 2^-23 relative,
  propagated through the formula on paper; each derivation stands beside its number. B never comes from what the device returns.

Ops that are IEEE add / multiply-add / compare / fmodf only (in_range_*, slew, seek) have no tolerance: device == twin bit for bit.
tef_kinematic divides and is held to the FGKinemat restatement at 2^-22.
"""
import functools
import math

import mpmath as mp
import numpy as np

U = 2.0 ** -23          # one ulp of a float32 result, relative (at most)
E53 = 2.0 ** -53
f32 = np.float32
PI = math.pi

# the ops in the order of include/aircombat.h's enum and capi.AC_PROBE_OPS (tests/test_math_probe_host.py holds the three together)
OPS = ("fx_rcp", "fx_rsqrt", "fx_sqrt", "fx_sqrt_both", "fx_sincos", "atan2_fast", "acos_fast", "pow_pos", "tanh_fast", "atanh_fast",
       "sigmoid_f", "tanh_f", "atmosphere", "pitot", "vcas", "in_range_deg", "in_range_rad", "slew", "tef_kinematic", "seek",
       "posture_fn", "missile_height_f", "missile_height_d", "neu_height64", "locate", "locate_fast")
EXACT_OPS = ("in_range_deg", "in_range_rad", "slew", "seek")
CENTER = (60.0, 120.0, 0.0)   # lat, lon [deg], alt [m] of the shipped battle-field centre (the configs' battle_field_center)


# ------------------------------------------------------------------------------------------------ exact multiply-add
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a
    h = c - (c - a)
    return h, a - h


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _add_round_to_odd(a, b):
    """a + b in float64 rounded to odd: the exact sum if it is a float64, else the neighbour whose last mantissa bit is set."""
    s, e = _two_sum(a, b)
    s = np.ascontiguousarray(s)
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0)
    return np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)


def _b64(*xs):
    return [np.ascontiguousarray(x, dtype=np.float64) + 0.0 for x in np.broadcast_arrays(*[np.asarray(x, dtype=np.float64) for x in xs])]


def fma64(a, b, c):
    """round(a * b + c) with one rounding, float64 (Boldo & Melquiond 2008: error-free product, error-free sum, the two error terms added
    with rounding to odd, one final rounding to nearest). Exact for every finite case without overflow or underflow."""
    a, b, c = _b64(a, b, c)
    ph, pl = _two_prod(a, b)
    th, tl = _two_sum(c, ph)
    return th + _add_round_to_odd(tl, pl)


def fma32(a, b, c):
    """round(a * b + c) with one rounding, float32: the product of two float32 is exact in float64, the sum is rounded to odd there, and
    53 >= 2 * 24 + 2 bits make the second rounding innocuous."""
    a, b, c = _b64(f32(a), f32(b), f32(c))
    return _add_round_to_odd(a * b, c).astype(f32)


def _f(x):
    return np.asarray(x, dtype=f32)


def _exp2_32(x):   # correctly rounded stand-in for v_exp_f32
    return np.exp2(_f(x).astype(np.float64)).astype(f32)


def _log2_32(x):   # correctly rounded stand-in for v_log_f32
    return np.log2(_f(x).astype(np.float64)).astype(f32)


def _expf(x):      # __expf: v_exp_f32(log2(e) * x)
    return _exp2_32(f32(1.4426950408889634) * _f(x))


def _logf(x):      # __logf: the compiler's natural log, good to an ulp
    return np.log(_f(x).astype(np.float64)).astype(f32)


def _neighbours32(v):
    v = _f(v)
    return np.concatenate([v, np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(-np.inf))])


def _neighbours64(v):
    v = np.asarray(v, dtype=np.float64)
    return np.concatenate([v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)])


def _mp_pair(vals):
    """A list of mpf as a float64 (hi, lo) pair."""
    hi = np.array([float(v) for v in vals])
    lo = np.array([float(v - mp.mpf(h)) for v, h in zip(vals, hi)])
    return hi, lo


# ------------------------------------------------------------------------------------------------ fp64 primitives (csrc/fp64_fast.hpp)
def _seed24(v):
    """v rounded to float32's 24-bit mantissa at any exponent: the stand-in for an fp64 hardware seed."""
    m, e = np.frexp(np.asarray(v, dtype=np.float64))
    return np.ldexp(m.astype(f32).astype(np.float64), e)


def twin_fx_rcp(x):
    r = _seed24(1.0 / x)
    for _ in range(2):
        r = fma64(fma64(-x, r, 1.0), r, r)
    return r


def twin_fx_rsqrt(x):
    r = _seed24(1.0 / np.sqrt(x))
    h = 0.5 * x
    for _ in range(2):
        r = r * fma64(-h * r, r, 1.5)
    return r


def twin_fx_sqrt_both(x):
    r = twin_fx_rsqrt(x)
    s = x * r
    return fma64(fma64(-s, s, x), 0.5 * r, s), r


def twin_fx_sqrt(x):
    x = np.asarray(x, dtype=np.float64)
    pos = x > 0.0
    y = twin_fx_sqrt_both(np.where(pos, x, 1.0))[0]
    return np.where(pos, y, 0.0)


SIN_COEF = (2.8114572543455206e-15, -7.6471637318198164e-13, 1.6059043836821613e-10, -2.5052108385441720e-08, 2.7557319223985893e-06,
            -1.9841269841269841e-04, 8.3333333333333332e-03, -1.6666666666666666e-01)
COS_COEF = (4.7794773323873853e-14, -1.1470745597729725e-11, 2.0876756987868100e-09, -2.7557319223985888e-07, 2.4801587301587302e-05,
            -1.3888888888888889e-03, 4.1666666666666664e-02, -0.5)


def twin_fx_sincos(x, fault=None):
    """fault: 'no_16' drops the 1/16! cosine term (the parent's body), 'coef' puts the 1/5! sine coefficient 1e-3 off, 'quadrant' negates the
    sine in quadrants 1 and 2 instead of 2 and 3."""
    x = np.asarray(x, dtype=np.float64)
    n = np.rint(x * 0.63661977236758134308)
    y = fma64(-n, 1.5707963267948965580, x)
    y = fma64(-n, 6.1232339957367660e-17, y)
    t = y * y
    sc = list(SIN_COEF)
    if fault == "coef":
        sc[6] *= 1.001
    ps = np.full_like(x, sc[0])
    for c in sc[1:]:
        ps = fma64(ps, t, c)
    s0 = fma64(y * t, ps, y)
    cc = COS_COEF[1:] if fault == "no_16" else COS_COEF
    pc = np.full_like(x, cc[0])
    for c in cc[1:]:
        pc = fma64(pc, t, c)
    c0 = fma64(t, pc, 1.0)
    q = n.astype(np.int64) & 3
    s1 = np.where(q & 1, c0, s0)
    c1 = np.where(q & 1, s0, c0)
    neg_s = ((q == 1) | (q == 2)) if fault == "quadrant" else ((q == 2) | (q == 3))
    return np.where(neg_s, -s1, s1), np.where((q == 1) | (q == 2), -c1, c1)


# ------------------------------------------------------------------------------------------------ fp32 primitives
ATAN_COEF = (0.0024489392526447773, -0.014364523813128471, 0.0397086925804615, -0.07227175682783127, 0.10494229197502136,
             -0.14159545302391052, 0.1998557597398758, -0.33332565426826477, 0.9999998807907104)


def twin_atan2_fast(y, x, fault=None):
    """fault: 'drop' leaves out the last (highest-degree) coefficient, 'coef' puts the t^2 coefficient 1e-3 off, 'quadrant' reflects
    for x > 0 instead of x < 0."""
    y, x = _f(y), _f(x)
    ax, ay = np.abs(x), np.abs(y)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    a = mn * (f32(1.0) / mx)
    t = a * a
    co = [f32(c) for c in ATAN_COEF]
    if fault == "drop":
        co = co[1:]
    if fault == "coef":
        co[-3] = f32(co[-3] * 1.001)
    p = np.full_like(a, co[0])
    for c in co[1:]:
        p = fma32(p, t, c)
    r = p * a
    r = np.where(ay > ax, f32(1.57079632679489662) - r, r)
    r = np.where((x > 0) if fault == "quadrant" else (x < 0), f32(3.14159265358979324) - r, r)
    return np.copysign(r, y).astype(f32)


def twin_acos_fast(x):
    x = _f(x)
    return twin_atan2_fast(np.sqrt((f32(1.0) - x) * (f32(1.0) + x)), x)


def twin_pow_pos(x, y):
    return _exp2_32(_f(y) * _log2_32(x))


def twin_tanh_fast(x):
    t = _expf(f32(2.0) * np.clip(_f(x), f32(-10.0), f32(10.0)))
    return (t - f32(1.0)) / (t + f32(1.0))


def twin_atanh_fast(x):
    x = _f(x)
    return f32(0.5) * _logf((f32(1.0) + x) / (f32(1.0) - x))


def twin_sigmoid_f(x):
    return f32(1.0) / (f32(1.0) + _expf(-_f(x)))


def twin_tanh_f(x):
    return f32(1.0) - f32(2.0) / (_expf(f32(2.0) * _f(x)) + f32(1.0))


def twin_atmosphere(h, fault=None):
    """fault: 'coef' puts the tropospheric lapse rate 1e-3 off."""
    h = _f(h)
    Re, R, kG0 = f32(20855531.5), f32(1716.557158), f32(32.174049)
    g0R = kG0 / R
    gp = h * Re / (Re + h)
    hb1, hb2 = f32(36089.2388), f32(65616.7979)
    tropo, strato1 = gp < hb1, gp < hb2
    L0 = (f32(389.97) - f32(518.67)) / hb1
    if fault == "coef":
        L0 = f32(L0 * 1.001)
    L2 = (f32(411.57) - f32(389.97)) / (f32(104986.8766) - hb2)
    T = np.where(tropo, fma32(L0, gp, f32(518.67)), np.where(strato1, f32(389.97), fma32(L2, gp - hb2, f32(389.97)))).astype(f32)
    inv_base = np.where(tropo, f32(1.0) / f32(518.67), f32(1.0) / f32(389.97)).astype(f32)
    ex_pow = -np.where(tropo, g0R / L0, g0R / L2).astype(f32) * _log2_32(T * inv_base)
    ex_iso = (-g0R * f32(1.44269504088896341) / f32(389.97)) * (gp - hb1)
    iso = ~tropo & strato1
    P = np.where(tropo, f32(2116.228), np.where(strato1, f32(472.680579), f32(114.344890))).astype(f32) * _exp2_32(np.where(iso, ex_iso, ex_pow))
    rho = P / (R * T)
    a = np.sqrt(f32(1.4) * R * T)
    return T, P, rho, a


def twin_pitot(mach, p):
    mach, p = _f(mach), _f(p)
    m2 = mach * mach
    x = fma32(f32(0.2), m2, f32(1.0))
    sub = x * x * x * np.sqrt(x)
    y = np.maximum(fma32(f32(7.0), m2, f32(-1.0)), f32(1.0))
    sup = f32(166.92158009316827) * (m2 * m2 * m2 * mach) / (y * y * np.sqrt(y))
    return fma32(p, np.where(mach < 1.0, sub, sup).astype(f32), -p)


def twin_vcas(qc):
    qc = _f(qc)
    psl, asl = f32(2116.228), f32(1116.448558)
    A = qc / psl + f32(1.0)
    M = np.sqrt(np.maximum(f32(0.0), f32(5.0) * (twin_pow_pos(A, f32(1.0) / f32(3.5)) - f32(1.0))))
    Ms = M.copy()
    sup = M > 1.0
    Ms[~sup] = f32(1.5)                                  # (not used: keeps the unused lanes finite)
    for _ in range(10):
        w = np.where(sup, f32(1.0) - f32(1.0) / (f32(7.0) * Ms * Ms), f32(1.0)).astype(f32)
        Ms = f32(0.8812848543473311) * np.sqrt(A * twin_pow_pos(w, f32(2.5)))
    return asl * np.where(sup, Ms, M).astype(f32)


def _ftz(x):
    """The build flushes fp32 denormals to zero (-fgpu-flush-denormals-to-zero): a denormal argument reads as a zero of its sign."""
    x = _f(x)
    return np.where(np.abs(x) < f32(2.0 ** -126), np.copysign(f32(0.0), x), x).astype(f32)


def twin_in_range_deg(a, fault=None):
    """fault: 'ge' wraps at a >= 180 instead of a > 180."""
    a = np.fmod(_ftz(a), f32(360.0))
    a = np.where(a < 0, a + f32(360.0), a).astype(f32)
    over = (a >= f32(180.0)) if fault == "ge" else (a > f32(180.0))
    return np.where(over, a - f32(360.0), a).astype(f32)


def twin_in_range_rad(a):
    a = np.fmod(_ftz(a), f32(6.283185307179586))
    a = np.where(a < 0, a + f32(6.283185307179586), a).astype(f32)
    return np.where(a > f32(3.14159265358979), a - f32(6.283185307179586), a).astype(f32)


KFCSDT = f32(1.0) / f32(120.0)


def twin_slew(out, inp, lo, hi, rate):
    out, inp, lo, hi, rate = (_f(v) for v in (out, inp, lo, hi, rate))
    inp = np.minimum(np.maximum(inp, lo), hi)
    step = rate * KFCSDT
    d = inp - out
    return np.where(np.abs(d) <= step, inp, out + np.copysign(step, d)).astype(f32)


def twin_seek(v, target, accel, decel, dt):
    v, target, accel, decel, dt = (_f(x) for x in (v, target, accel, decel, dt))
    down = np.maximum(fma32(-dt, decel, v), target)
    up = np.minimum(fma32(dt, accel, v), target)
    return np.where(v > target, down, np.where(v < target, up, v)).astype(f32)


def twin_tef_kinematic(out, inp, fault=None):
    """fault: 'lt' takes 0 < out for 0 <= out in the detent search of a rising input."""
    out, inp = _f(out).copy(), np.clip(_f(inp), f32(-1.0), f32(1.0))
    dt0 = np.full_like(out, KFCSDT)
    walking = np.ones(out.shape, dtype=bool)
    rate = f32(1.0) / f32(3.0)
    for _ in range(3):
        go = walking & (dt0 > 0) & (inp != out)
        rising_in_2 = (f32(0.0) < out) if fault == "lt" else (f32(0.0) <= out)
        ind = np.where(inp < out, np.where(f32(0.0) < out, 2, 1), np.where(rising_in_2, 2, 1))
        jump = ind == 1
        this_in = np.clip(inp, f32(0.0), f32(1.0))
        this_dt = np.abs((this_in - out) / rate)
        partial = dt0 < this_dt
        moved = np.where(out < inp, fma32(dt0, rate, out), fma32(-dt0, rate, out))
        out_n = np.where(jump, inp, np.where(partial, moved, this_in))
        dt_n = np.where(jump, dt0, np.where(partial, f32(0.0), dt0 - this_dt))
        out = np.where(go, out_n, out).astype(f32)
        dt0 = np.where(go, dt_n, dt0).astype(f32)
        walking = go & ~jump
    return out


def twin_posture_fn(AO, TA, Rkm, fault=None):
    """fault: 'coef' puts the range law's linear coefficient 1e-3 off."""
    AO, TA, R = _f(AO), _f(TA), _f(Rkm)
    kPi = f32(3.14159265358979)
    x = np.maximum(f32(1.0) - np.maximum(f32(2.0) * TA / kPi, f32(1e-4)), f32(-0.99999994))
    orn = f32(1.0) / (f32(50.0) * AO / kPi + f32(2.0)) + f32(0.5) + np.minimum(twin_atanh_fast(x) / (f32(2.0) * kPi), f32(0.0)) + f32(0.5)
    b = f32(0.284 * 1.001) if fault == "coef" else f32(0.284)
    quad = fma32(b, R, f32(-0.032) * R * R) + f32(0.38)
    rng = np.where(R < 5, f32(1.0), f32(0.0)) + np.where(R >= 5, np.clip(quad, f32(0.0), f32(1.0)), f32(0.0)) + \
        np.clip(_expf(f32(-0.16) * R), f32(0.0), f32(0.2))
    return (orn * rng).astype(f32)


# ------------------------------------------------------------------------------------------------ geodesy
WGS_A, WGS_B = 6378137.0, 6356752.314245179          # pymap3d's WGS84 [m]
KA, KB, KOMEGA = 20925646.32546, 20855486.5951, 0.00007292115   # JSBSim's ellipsoid [ft] and Earth rate


def geodetic_lat(p, Z, a, b):
    """Geodetic latitude of the point at distance p from the axis and Z above the equator: Bowring's iteration run to convergence."""
    e2, ep2 = 1.0 - (b / a) ** 2, (a / b) ** 2 - 1.0
    beta = np.arctan2(a * Z, b * p)
    for _ in range(6):
        phi = np.arctan2(Z + ep2 * b * np.sin(beta) ** 3, p - e2 * a * np.cos(beta) ** 3)
        beta = np.arctan2(b * np.sin(phi), a * np.cos(phi))
    return phi


def centre_constants(center=CENTER):
    """What ac_create puts into the device configuration for a battle-field centre (float64 origin and direction cosines, float32 radii)."""
    lat, lon, alt = center
    a, f = WGS_A, 1.0 / 298.257223563
    e2 = f * (2.0 - f)
    sl, cl, so, co = math.sin(math.radians(lat)), math.cos(math.radians(lat)), math.sin(math.radians(lon)), math.cos(math.radians(lon))
    w2 = 1.0 - e2 * sl * sl
    N = a / math.sqrt(w2)
    return dict(P0=((N + alt) * cl * co, (N + alt) * cl * so, (N * (WGS_B / WGS_A) ** 2 + alt) * sl), sl=sl, cl=cl, so=so, co=co,
                rn0=f32(N + alt), rm0=f32(a * (1.0 - e2) / (w2 * math.sqrt(w2)) + alt), h0=f32(alt))


def _neu_to_ecef64(n, e, u, center):
    c = centre_constants(center)
    t = c["cl"] * u - c["sl"] * n
    dz = c["sl"] * u + c["cl"] * n
    dx = c["co"] * t - c["so"] * e
    dy = c["so"] * t + c["co"] * e
    return c["P0"][0] + dx, c["P0"][1] + dy, c["P0"][2] + dz


def ref_neu_height(n, e, u, center=CENTER):
    """The exact ellipsoidal height of the NEU point (utils.py's NEU2LLA -> pymap3d.ned2geodetic), float64: good to ~1e-9 m."""
    X, Y, Z = _neu_to_ecef64(*(np.asarray(v, dtype=np.float64) for v in (n, e, u)), center)
    p = np.hypot(X, Y)
    phi = geodetic_lat(p, Z, WGS_A, WGS_B)
    e2 = 1.0 - (WGS_B / WGS_A) ** 2
    return p * np.cos(phi) + Z * np.sin(phi) - WGS_A * np.sqrt(1.0 - e2 * np.sin(phi) ** 2)


def ref_neu_height_mp(n, e, u, center=CENTER):
    """The same as a (hi, lo) pair: the point and the height formula in 100-bit arithmetic. The latitude comes from float64: the height is
    stationary in it (dh / dphi = 0 at the foot point), so its 1e-16 rad costs 1e-25 m."""
    mp.mp.prec = 100
    lat, lon, alt = (mp.mpf(v) for v in center)
    a, b = mp.mpf(WGS_A), mp.mpf(WGS_B)
    f = 1 / mp.mpf("298.257223563")
    e2c = f * (2 - f)
    sl, cl, so, co = mp.sin(mp.radians(lat)), mp.cos(mp.radians(lat)), mp.sin(mp.radians(lon)), mp.cos(mp.radians(lon))
    N = a / mp.sqrt(1 - e2c * sl * sl)
    P0 = ((N + alt) * cl * co, (N + alt) * cl * so, (N * (b / a) ** 2 + alt) * sl)
    e2 = 1 - (b / a) ** 2
    X64, Y64, Z64 = _neu_to_ecef64(*(np.asarray(v, dtype=np.float64) for v in (n, e, u)), center)
    phi = geodetic_lat(np.hypot(X64, Y64), Z64, WGS_A, WGS_B)
    out = []
    for ni, ei, ui, ph in zip(n, e, u, phi):
        ni, ei, ui, ph = mp.mpf(float(ni)), mp.mpf(float(ei)), mp.mpf(float(ui)), mp.mpf(float(ph))
        t = cl * ui - sl * ni
        Z = P0[2] + sl * ui + cl * ni
        X = P0[0] + co * t - so * ei
        Y = P0[1] + so * t + co * ei
        p = mp.sqrt(X * X + Y * Y)
        s = mp.sin(ph)
        out.append(p * mp.cos(ph) + Z * s - a * mp.sqrt(1 - e2 * s * s))
    return _mp_pair(out)


def twin_missile_height_f(n, e, u, center=CENTER):
    c = centre_constants(center)
    n, e, u = _f(n), _f(e), _f(u)
    return c["h0"] + u + n * n / (f32(2.0) * (c["rm0"] + u)) + e * e / (f32(2.0) * (c["rn0"] + u))


def twin_missile_height_d(n, e, u, center=CENTER, fault=None):
    """fault: 'drop' leaves out the east term."""
    c = centre_constants(center)
    n, e, u = (np.asarray(v, dtype=np.float64) for v in (n, e, u))
    h = float(c["h0"]) + u
    h = fma64(n * n, twin_fx_rcp(2.0 * (float(c["rm0"]) + u)), h)
    return h if fault == "drop" else fma64(e * e, twin_fx_rcp(2.0 * (float(c["rn0"]) + u)), h)


def _fukushima64(rxy, s0, ec):
    zc, c0 = ec * s0, ec * rxy
    c02, s02 = c0 * c0, s0 * s0
    return zc, c0, c02, s02, fma64(c0, c0, s02)


def twin_neu_height64(n, e, u, center=CENTER):
    c = centre_constants(center)
    n, e, u = (np.asarray(v, dtype=np.float64) for v in (n, e, u))
    t = fma64(c["cl"], u, -(c["sl"] * n))
    dz = fma64(c["sl"], u, c["cl"] * n)
    dx = fma64(c["co"], t, -(c["so"] * e))
    dy = fma64(c["so"], t, c["co"] * e)
    X, Y, Z = c["P0"][0] + dx, c["P0"][1] + dy, c["P0"][2] + dz
    a, b = WGS_A, WGS_B
    ec = b / a
    ec2 = ec * ec
    cc0 = a * (1.0 - ec2)
    rxy = np.sqrt(fma64(X, X, Y * Y))
    s0 = np.abs(Z)
    zc, c0, c02, s02, a02 = _fukushima64(rxy, s0, ec)
    a0 = np.sqrt(a02)
    a03 = a02 * a0
    s1 = fma64(zc, a03, cc0 * s02 * s0)
    c1 = fma64(rxy, a03, -(cc0 * c02 * c0))
    cs = cc0 * c0 * s0
    b0 = 1.5 * cs * fma64(fma64(rxy, s0, -(zc * c0)), a0, -cs)
    s1 = fma64(s1, a03, -(b0 * s0))
    cc = ec * fma64(c1, a03, -(b0 * c0))
    s12, cc2 = s1 * s1, cc * cc
    norm = np.sqrt(s12 + cc2)
    return (fma64(rxy, cc, s0 * s1) - a * np.sqrt(fma64(ec2, s12, cc2))) / norm


def ref_locate(rx, ry, rz):
    """FGLocation: altitude above the sea-level radius at the geocentric latitude, and the local north / east / down unit vectors (geodetic
    normal, inertial longitude) in ECI. Float64, latitude by an iteration run to convergence. Columns as the probe's output row."""
    rx, ry, rz = (np.asarray(v, dtype=np.float64) for v in (rx, ry, rz))
    p = np.hypot(rx, ry)
    rad = np.sqrt(rx * rx + ry * ry + rz * rz)
    ec2 = (KB / KA) ** 2
    cgc = p / rad
    slr = KB / np.sqrt(1.0 - (1.0 - ec2) * cgc * cgc)
    phi = geodetic_lat(p, rz, KA, KB)
    sLa, cLa, sLo, cLo = np.sin(phi), np.cos(phi), ry / p, rx / p
    z = np.zeros_like(p)
    return np.stack([rad - slr, -cLo * sLa, -sLo * sLa, cLa, -sLo, cLo, z, -cLo * cLa, -sLo * cLa, -sLa], axis=1)


def twin_locate(rx, ry, rz, ticks):
    rx, ry, rz = (np.asarray(v, dtype=np.float64) for v in (rx, ry, rz))
    epa = KOMEGA * np.asarray(ticks, dtype=np.float64) * (1.0 / 60.0)
    e2 = epa * epa
    ce = fma64(-e2, fma64(-e2, fma64(-e2, 1.0 / 720.0, 1.0 / 24.0), 0.5), 1.0)
    se = epa * fma64(-e2, fma64(-e2, fma64(-e2, 1.0 / 5040.0, 1.0 / 120.0), 1.0 / 6.0), 1.0)
    X, Y, Z = fma64(ce, rx, se * ry), fma64(-se, rx, ce * ry), rz
    rxy2 = fma64(X, X, Y * Y)
    rxy, rad = twin_fx_sqrt(rxy2), twin_fx_sqrt(fma64(Z, Z, rxy2))
    ec = KB / KA
    ec2 = ec * ec
    ee = 1.0 - ec2
    c = KA * ee
    s0 = np.abs(Z)
    zc, c0, c02, s02, a02 = _fukushima64(rxy, s0, ec)
    a0 = twin_fx_sqrt(a02)
    a03 = a02 * a0
    s1 = fma64(zc, a03, c * s02 * s0)
    c1 = fma64(rxy, a03, -(c * c02 * c0))
    cs = c * c0 * s0
    b0 = 1.5 * cs * fma64(fma64(rxy, s0, -(zc * c0)), a0, -cs)
    s1 = fma64(s1, a03, -(b0 * s0))
    cc = ec * fma64(c1, a03, -(b0 * c0))
    inv = twin_fx_rsqrt(fma64(s1, s1, cc * cc))
    sinLat, cosLat = np.where(Z >= 0, s1, -s1) * inv, cc * inv
    cgc = rxy * twin_fx_rcp(rad)
    slr = KA * ec * twin_fx_rsqrt(fma64(-ee * cgc, cgc, 1.0))
    h = (rad - slr).astype(f32)
    irxy = twin_fx_rcp(rxy)
    cLo, sLo = (X * irxy).astype(f32), (Y * irxy).astype(f32)
    cef, sef, sLa, cLa = ce.astype(f32), se.astype(f32), sinLat.astype(f32), cosLat.astype(f32)
    nx, ny, nz = -cLo * sLa, -sLo * sLa, cLa
    ex, ey = -sLo, cLo
    dx, dy, dz = -cLo * cLa, -sLo * cLa, -sLa
    rot = lambda vx, vy: (fma32(cef, vx, -(sef * vy)), fma32(sef, vx, cef * vy))   # noqa: E731
    n0, n1 = rot(nx, ny)
    e0, e1 = rot(ex, ey)
    d0, d1 = rot(dx, dy)
    return np.stack([h, n0, n1, nz, e0, e1, np.zeros_like(h), d0, d1, dz], axis=1).astype(np.float64)


def twin_locate_fast(rx, ry, rz):
    rx, ry, rz = (np.asarray(v, dtype=np.float64) for v in (rx, ry, rz))
    rad = np.sqrt(fma64(rz, rz, fma64(ry, ry, rx * rx)))
    ia = f32(1.0 / KA)
    px, py, z = rx.astype(f32) * ia, ry.astype(f32) * ia, rz.astype(f32) * ia
    p2 = fma32(px, px, py * py)
    irp = f32(1.0) / np.sqrt(p2)
    p = p2 * irp
    cLo, sLo = px * irp, py * irp
    ec, e2 = f32(KB / KA), f32(1.0 - (KB / KA) * (KB / KA))
    s0 = np.abs(z)
    zc, c0 = ec * s0, ec * p
    c02, s02 = c0 * c0, s0 * s0
    a02 = fma32(c0, c0, s02)
    a0 = np.sqrt(a02)
    a03 = a02 * a0
    s1 = fma32(zc, a03, e2 * s02 * s0)
    c1 = fma32(p, a03, -(e2 * c02 * c0))
    cs = e2 * c0 * s0
    b0 = f32(1.5) * cs * fma32(fma32(p, s0, -(zc * c0)), a0, -cs)
    s1 = fma32(s1, a03, -(b0 * s0))
    cc = ec * fma32(c1, a03, -(b0 * c0))
    inv = f32(1.0) / np.sqrt(fma32(s1, s1, cc * cc))
    sLa, cLa = np.copysign(s1, z) * inv, cc * inv
    cg2 = p2 / fma32(z, z, p2)
    x = e2 * cg2
    ser = x * fma32(x, fma32(x, fma32(x, f32(0.2734375), f32(0.3125)), f32(0.375)), f32(0.5))
    h = fma32(-f32(KB), ser, (rad - KB).astype(f32))
    zero = np.zeros_like(h)
    return np.stack([h, -cLo * sLa, -sLo * sLa, cLa, -sLo, cLo, zero, -cLo * cLa, -sLo * cLa, -sLa], axis=1).astype(np.float64)


# ------------------------------------------------------------------------------------------------ references of the fp32 ops
ATM_H = (0.0, 36089.2388, 65616.7979, 104986.8766)       # geopotential breakpoints [ft] and temperatures [R] of the 1976 atmosphere
ATM_T = (518.67, 389.97, 389.97, 411.57)
ATM_RE = 6356766.0 / 0.3048
ATM_R = (8.31432 * 0.06852168 / (1.8 * 0.3048 * 0.3048)) / (28.9645 * 0.06852168 / 1000.0)
ATM_G0 = 9.80665 / 0.3048
ATM_PSL = 2116.228


def ref_atmosphere(h):
    """The 1976 standard atmosphere on geopotential layers (FGStandardAtmosphere), float64: T [R], P [psf], rho [slug/ft3], a [ft/s]."""
    h = np.asarray(h, dtype=np.float64)
    gp = h * ATM_RE / (ATM_RE + h)
    lapse = [(ATM_T[b + 1] - ATM_T[b]) / (ATM_H[b + 1] - ATM_H[b]) for b in range(3)]
    pb = [ATM_PSL]
    for b in range(2):
        dH = ATM_H[b + 1] - ATM_H[b]
        pb.append(pb[b] * ((ATM_T[b] / (ATM_T[b] + lapse[b] * dH)) ** (ATM_G0 / (ATM_R * lapse[b])) if lapse[b] != 0.0
                           else math.exp(-ATM_G0 * dH / (ATM_R * ATM_T[b]))))
    layer = np.where(gp < ATM_H[1], 0, np.where(gp < ATM_H[2], 1, 2))
    Tb, Hb, L, Pb = (np.take(np.array(v), layer) for v in (ATM_T[:3], ATM_H[:3], lapse, pb))
    T = Tb + L * (gp - Hb)
    with np.errstate(divide="ignore", invalid="ignore"):
        P = np.where(L != 0.0, Pb * (Tb / T) ** (ATM_G0 / (ATM_R * np.where(L != 0.0, L, 1.0))), Pb * np.exp(-ATM_G0 * (gp - Hb) / (ATM_R * Tb)))
    return np.stack([T, P, P / (ATM_R * T), np.sqrt(1.4 * ATM_R * T)], axis=1)


def ref_pitot(mach, p):
    mach, p = np.asarray(mach, dtype=np.float64), np.asarray(p, dtype=np.float64)
    sub = (1.0 + 0.2 * mach * mach) ** 3.5
    sup = 166.92158009316827 * mach ** 7.0 / np.maximum(7.0 * mach * mach - 1.0, 1.0) ** 2.5
    return p * np.where(mach < 1.0, sub, sup) - p


def ref_mach_from_qc(qc, p=ATM_PSL):
    A = np.asarray(qc, dtype=np.float64) / p + 1.0
    M = np.sqrt(5.0 * (A ** (1.0 / 3.5) - 1.0))
    Ms = np.where(M > 1.0, M, 1.5)
    for _ in range(10):
        Ms = 0.8812848543473311 * np.sqrt(A * np.where(M > 1.0, 1.0 - 1.0 / (7.0 * Ms * Ms), 1.0) ** 2.5)
    return np.where(M > 1.0, Ms, M)


def ref_vcas(qc):
    return math.sqrt(1.4 * ATM_R * 518.67) * ref_mach_from_qc(qc)


def ref_in_range(a, period):
    """utils.py's in_range_deg / in_range_rad on the float32 value, in exact rational arithmetic of Python's % on floats."""
    a = np.asarray(a, dtype=np.float64)
    r = np.mod(a, period)
    return np.where(r > period / 2, r - period, r)


def ref_kinemat(out, inp, detents=(-1.0, 0.0, 1.0), times=(3.0, 0.0, 3.0), dt=1.0 / 120.0):
    """FGKinemat::Run, float64, one value. Returns (output, the smallest |remaining time - segment time| met: a tie there decides between
    two branches, and an fp32 device may fall on the other side of it)."""
    n = len(detents)
    inp = min(max(inp * detents[-1], detents[0]), detents[-1])
    dt0, tie = dt, math.inf
    while dt0 > 0.0 and not abs(inp - out) <= 2.0 * 2.220446049250313e-16 * max(abs(inp), abs(out)):
        ind = 1
        while (detents[ind] < out) if inp < out else (detents[ind] <= out):
            if ind >= n - 1:
                break
            ind += 1
        if times[ind] <= 0.0:
            out = inp
            break
        rate = (detents[ind] - detents[ind - 1]) / times[ind]
        this_in = min(max(inp, detents[ind - 1]), detents[ind])
        this_dt = abs((this_in - out) / rate)
        tie = min(tie, abs(dt0 - this_dt))
        if dt0 < this_dt:
            this_dt = dt0
            out = out + this_dt * rate if out < inp else out - this_dt * rate
        else:
            out = this_in
        dt0 -= this_dt
    return out, tie


def ref_posture(AO, TA, Rkm):
    """posture_reward.py's orientation v2 x range v3 in float64, with the documented floor of the atanh argument (1 - 2^-24 inside -1)."""
    AO, TA, R = (np.asarray(v, dtype=np.float64) for v in (AO, TA, Rkm))
    x = np.maximum(1.0 - np.maximum(2.0 * TA / PI, 1e-4), -(1.0 - 2.0 ** -24))
    orn = 1.0 / (50.0 * AO / PI + 2.0) + 0.5 + np.minimum(np.arctanh(x) / (2.0 * PI), 0.0) + 0.5
    rng = np.where(R < 5, 1.0, 0.0) + np.where(R >= 5, np.clip(-0.032 * R * R + 0.284 * R + 0.38, 0.0, 1.0), 0.0) + np.clip(np.exp(-0.16 * R), 0.0, 0.2)
    return orn * rng, orn, rng, x


# ------------------------------------------------------------------------------------------------ input sets
def _rng(name):
    return np.random.default_rng([0x6D617468, OPS.index(name)])


def _positive_inputs():
    g = _rng("fx_rcp")
    sq = np.arange(1.0, 200.0) ** 2
    edges = np.concatenate([2.0 ** np.arange(-40, 60), 4.0 ** np.arange(-20, 30), _neighbours64([1.0, 2.0, 4.0]), sq, _neighbours64(sq[:40]),
                            [4.0e13, WGS_A ** 2, KA ** 2, WGS_B ** 2, KB ** 2]])
    return np.concatenate([10.0 ** g.uniform(-6, 16, 14000), 1.0 + g.uniform(0, 3, 5000), edges])


def _box(name, L, nrand, cast=None):
    g = _rng(name)
    n, e, u = g.uniform(-L, L, nrand), g.uniform(-L, L, nrand), g.uniform(0.0, 20000.0, nrand)
    cn, ce, cu = np.meshgrid([-L, 0.0, L], [-L, 0.0, L], [0.0, 10000.0, 20000.0], indexing="ij")
    rows = np.stack([np.concatenate([n, cn.ravel()]), np.concatenate([e, ce.ravel()]), np.concatenate([u, cu.ravel()])], axis=1)
    return rows.astype(cast).astype(np.float64) if cast else rows


def _eci_inputs(name):
    """ECI positions at every latitude and longitude, altitudes 0 to 80 000 ft above the sea-level radius, with a tick count."""
    g = _rng(name)
    m = 30000
    lat = np.concatenate([np.arcsin(g.uniform(-1, 1, m - 200)), g.uniform(-1, 1, 100) * 1e-3, np.radians(g.uniform(89.0, 89.99, 50)),
                          -np.radians(g.uniform(89.0, 89.99, 50))])
    lon = g.uniform(-PI, PI, m)
    alt = np.concatenate([g.uniform(0.0, 80000.0, m - 400), np.zeros(200), np.full(200, 80000.0)])
    ec2 = (KB / KA) ** 2
    slr = KB / np.sqrt(1.0 - (1.0 - ec2) * np.cos(lat) ** 2)          # (lat used as the geocentric latitude)
    r = slr + alt
    ticks = g.integers(0, 60 * 1200, m).astype(np.float64)
    return np.stack([r * np.cos(lat) * np.cos(lon), r * np.cos(lat) * np.sin(lon), r * np.sin(lat), ticks], axis=1)


@functools.lru_cache(maxsize=None)
def inputs(op):
    """The input rows of `op`, float64 [n][k] (float32-exact for the fp32 ops)."""
    g = _rng(op)
    if op in ("fx_rcp", "fx_rsqrt", "fx_sqrt_both"):
        rows = _positive_inputs()
    elif op == "fx_sqrt":
        rows = np.concatenate([_positive_inputs(), [0.0]])
    elif op == "fx_sincos":
        k = np.arange(-32, 33) * (PI / 4)
        rows = np.concatenate([g.uniform(-8 * PI, 8 * PI, 18000), _neighbours64(k), g.uniform(-1e-3, 1e-3, 2000), [0.0]])
    elif op == "atan2_fast":
        # both arguments zero is outside atan2_fast's contract (finite, not both zero) and is left out
        r, th = 10.0 ** g.uniform(-3, 4, 40000), g.uniform(-PI, PI, 40000)
        y, x = _f(r * np.sin(th)), _f(r * np.cos(th))
        v = _f(10.0 ** g.uniform(-3, 4, 500))
        one = _neighbours32([1.0])
        ey = np.concatenate([0 * v, -0.0 * v, 0 * v, -0.0 * v, v, -v, v, -v, v, -v, np.tile(one, 4) * np.repeat(_f([1, 1, -1, -1]), 3)])
        ex = np.concatenate([v, v, -v, -v, 0 * v, 0 * v, v, v, -v, -v, np.tile(_f([1.0, 1.0, 1.0]), 4) * np.repeat(_f([1, -1, 1, -1]), 3)])
        rows = np.stack([np.concatenate([y, ey]), np.concatenate([x, ex])], axis=1)
    elif op == "acos_fast":
        one = f32(1.0)
        edges = _f([1.0, -1.0, np.nextafter(one, f32(0)), -np.nextafter(one, f32(0)), 0.0, -0.0])
        rows = np.concatenate([_f(g.uniform(-1, 1, 30000)), _f(np.cos(g.uniform(0, 3e-3, 3000))), -_f(np.cos(g.uniform(0, 3e-3, 3000))), edges])
    elif op == "pow_pos":
        # the call sites: A^(1/3.5), A in [1, 12] (vcas) and (1 - 1/7M^2)^2.5 in [0.6, 1]; then a wider fill
        x = np.concatenate([g.uniform(1.0, 12.0, 12000), g.uniform(0.6, 1.0, 12000), g.uniform(0.5, 16.0, 12000), [1.0, 1.0]])
        y = np.concatenate([np.full(12000, f32(1.0) / f32(3.5)), np.full(12000, 2.5), g.uniform(0.25, 3.0, 12000), [f32(1.0) / f32(3.5), 2.5]])
        rows = np.stack([_f(x), _f(y)], axis=1)
    elif op in ("tanh_fast", "tanh_f"):
        rows = np.concatenate([_f(g.uniform(-12, 12, 30000)), _f(g.uniform(-1e-3, 1e-3, 2000)), _neighbours32([0.0, 10.0, -10.0]), _f([-0.0])])
    elif op == "atanh_fast":
        # posture_fn's argument: 1 - max(2 TA / pi, 1e-4) floored at -(1 - 2^-24)
        rows = np.concatenate([_f(g.uniform(-1, 0.9999, 30000)), -_f(1.0 - 10.0 ** g.uniform(-7, -1, 4000)), _f([-0.99999994, 0.9999, 0.0])])
    elif op == "sigmoid_f":
        rows = np.concatenate([_f(g.uniform(-30, 30, 30000)), _f(g.uniform(-1e-3, 1e-3, 2000)), _f([0.0, -0.0])])
    elif op == "atmosphere":
        # geometric altitudes of the two layer boundaries: gp = h Re / (Re + h)  <=>  h = gp Re / (Re - gp)
        hb = [gp * ATM_RE / (ATM_RE - gp) for gp in ATM_H[1:3]]
        near = np.concatenate([b + g.uniform(-2.0, 2.0, 400) for b in hb])
        rows = np.concatenate([_f(g.uniform(-1000.0, 80000.0, 40000)), _f(near), _neighbours32(hb), _f([-1000.0, 0.0, 80000.0])])
    elif op == "pitot":
        m = np.concatenate([g.uniform(0.1, 2.2, 30000), 1.0 + g.uniform(-1e-3, 1e-3, 1000), _neighbours32([1.0]), [0.1, 2.2]])
        rows = np.stack([_f(m), _f(g.uniform(50.0, 2200.0, m.size))], axis=1)
    elif op == "vcas":
        m = np.concatenate([g.uniform(0.1, 2.2, 30000), 1.0 + g.uniform(-1e-3, 1e-3, 1000), [0.1, 1.0, 2.2]])
        rows = _f(ref_pitot(m, g.uniform(50.0, 2200.0, m.size)))     # (round trip: test_math_probe_host inverts these back)
    elif op in ("in_range_deg", "in_range_rad"):
        per = 360.0 if op == "in_range_deg" else float(f32(6.283185307179586))
        mult = np.arange(-8, 9) * per / 2
        rows = np.concatenate([_f(g.uniform(-4 * per, 4 * per, 20000)), _neighbours32(mult), _f([0.0, -0.0, 180.0, -180.0, 360.0, -360.0]),
                               _neighbours32([3.14159265358979, -3.14159265358979])])
    elif op == "slew":
        lo, hi, rate = (np.array(v)[g.integers(0, 4, 30000)] for v in ([-1.0, -1.0, -1.0, 0.0], [1.0, 1.0, 1.0, 60.0], [2 / 0.3, 2 / 0.3, 2 / 0.4, 60.0]))
        span = hi - lo
        out = lo + span * g.uniform(0, 1, 30000)
        inp = np.where(g.random(30000) < 0.5, out + span * g.uniform(-0.02, 0.02, 30000), lo + span * g.uniform(-0.2, 1.2, 30000))
        rows = np.stack([_f(out), _f(inp), _f(lo), _f(hi), _f(rate)], axis=1).astype(np.float64)
        step = rows[:, 4].astype(f32) * KFCSDT                           # |in - out| == step exactly, from both sides
        rows[:2000, 1] = (rows[:2000, 0].astype(f32) + np.where(np.arange(2000) % 2, step[:2000], -step[:2000])).astype(f32)
    elif op == "tef_kinematic":
        out = np.concatenate([g.uniform(-1, 1, 30000), g.uniform(-0.02, 0.02, 5000), [0.0, -0.1, 0.0, 0.0, 1.0, -1.0]])
        inp = np.concatenate([g.uniform(-1.2, 1.2, 30000), g.uniform(-0.02, 0.02, 5000), [-0.1, 0.9, 1.0, 0.0, 1.0, -1.0]])
        rows = np.stack([_f(out), _f(inp)], axis=1)
    elif op == "seek":
        v = g.uniform(0, 100, 30000)
        tgt = np.where(g.random(30000) < 0.5, v + g.uniform(-0.5, 0.5, 30000), g.uniform(0, 100, 30000))
        tgt[:500] = v[:500]
        rows = np.stack([_f(v), _f(tgt), _f(g.uniform(0.1, 60, 30000)), _f(g.uniform(0.1, 60, 30000)), np.full(30000, f32(1.0) / f32(60.0))], axis=1)
    elif op == "posture_fn":
        m = 30000
        AO = np.concatenate([g.uniform(0, PI, m), np.zeros(200), g.uniform(0, PI, 1200)])
        TA = np.concatenate([g.uniform(0, PI, m), g.uniform(0, PI, 200), np.full(100, f32(PI)), PI - 10.0 ** g.uniform(-7, -2, 500), g.uniform(0, PI, 600)])
        R = np.concatenate([g.uniform(0, 40, m), g.uniform(0, 40, 800), _neighbours32([5.0] * 100), 5.0 + g.uniform(-0.01, 0.01, 300)])
        rows = np.stack([_f(AO), np.minimum(_f(TA), f32(PI)), _f(R)], axis=1)
    elif op == "missile_height_f":
        rows = _box(op, 60000.0, 30000, cast=f32)
    elif op == "missile_height_d":
        rows = _box(op, 60000.0, 30000)
    elif op == "neu_height64":
        rows = _box(op, 60000.0, 20000)
    elif op in ("locate", "locate_fast"):
        rows = _eci_inputs(op)
    else:
        raise KeyError(op)
    rows = np.asarray(rows, dtype=np.float64)
    rows = rows.reshape(-1, 1) if rows.ndim == 1 else rows
    rows.setflags(write=False)
    return rows


# ------------------------------------------------------------------------------------------------ references, scales, twins per op
def _mp_map(fn, x, prec=120):
    mp.mp.prec = prec
    return _mp_pair([fn(mp.mpf(float(v))) for v in x])


@functools.lru_cache(maxsize=None)
def reference(op, center=CENTER):
    """(hi, lo): float64 [n][c] each (lo is zero where float64 is reference enough)."""
    X = inputs(op)
    c = [X[:, k] for k in range(X.shape[1])]
    pair = None
    if op == "fx_rcp":
        pair = _mp_map(lambda v: 1 / v, c[0])
    elif op == "fx_rsqrt":
        pair = _mp_map(lambda v: 1 / mp.sqrt(v), c[0])
    elif op == "fx_sqrt":
        pair = _mp_map(mp.sqrt, c[0])
    elif op == "fx_sqrt_both":
        a, b = reference("fx_sqrt"), reference("fx_rsqrt")
        n = X.shape[0]
        pair = (np.stack([a[0][:n, 0], b[0][:, 0]], axis=1), np.stack([a[1][:n, 0], b[1][:, 0]], axis=1))
    elif op == "fx_sincos":
        s, co = _mp_map(mp.sin, c[0]), _mp_map(mp.cos, c[0])
        pair = (np.stack([s[0], co[0]], axis=1), np.stack([s[1], co[1]], axis=1))
    elif op == "neu_height64":
        pair = ref_neu_height_mp(c[0], c[1], c[2], center)
    elif op == "atan2_fast":
        hi = np.arctan2(c[0], c[1])
    elif op == "acos_fast":
        hi = np.arccos(c[0])
    elif op == "pow_pos":
        hi = c[0] ** c[1]
    elif op in ("tanh_fast", "tanh_f"):
        hi = np.tanh(c[0])
    elif op == "atanh_fast":
        hi = np.arctanh(c[0])
    elif op == "sigmoid_f":
        hi = 1.0 / (1.0 + np.exp(-c[0]))
    elif op == "atmosphere":
        hi = ref_atmosphere(c[0])
    elif op == "pitot":
        hi = ref_pitot(c[0], c[1])
    elif op == "vcas":
        hi = ref_vcas(c[0])
    elif op == "in_range_deg":
        hi = ref_in_range(c[0], 360.0)
    elif op == "in_range_rad":
        hi = ref_in_range(c[0], 2 * PI)
    elif op == "tef_kinematic":
        hi = np.array([ref_kinemat(o, i)[0] for o, i in zip(c[0], c[1])])
    elif op == "posture_fn":
        hi = ref_posture(c[0], c[1], c[2])[0]
    elif op in ("missile_height_f", "missile_height_d"):
        hi = ref_neu_height(c[0], c[1], c[2], center)
    elif op in ("locate", "locate_fast"):
        hi = ref_locate(c[0], c[1], c[2])
    else:
        raise KeyError(op)   # slew and seek have no formula beyond their twin: they are held bit for bit
    if pair is None:
        hi = np.asarray(hi, dtype=np.float64)
        pair = (hi, np.zeros_like(hi))
    hi, lo = (np.asarray(v, dtype=np.float64) for v in pair)
    hi, lo = (v.reshape(-1, 1) if v.ndim == 1 else v for v in (hi, lo))
    hi.setflags(write=False)
    lo.setflags(write=False)
    return hi, lo


def twin(op, X=None, center=CENTER, fault=None):
    """The CPU twin's output rows, float64 [n][c]."""
    X = inputs(op) if X is None else np.asarray(X, dtype=np.float64)
    c = [X[:, k] for k in range(X.shape[1])]
    kw = {"fault": fault} if fault else {}
    if op == "fx_rcp":
        out = twin_fx_rcp(c[0])
    elif op == "fx_rsqrt":
        out = twin_fx_rsqrt(c[0])
    elif op == "fx_sqrt":
        out = twin_fx_sqrt(c[0])
    elif op == "fx_sqrt_both":
        out = twin_fx_sqrt_both(c[0])
    elif op == "fx_sincos":
        out = twin_fx_sincos(c[0], **kw)
    elif op == "atan2_fast":
        out = twin_atan2_fast(c[0], c[1], **kw)
    elif op == "acos_fast":
        out = twin_acos_fast(c[0])
    elif op == "pow_pos":
        out = twin_pow_pos(c[0], c[1])
    elif op == "tanh_fast":
        out = twin_tanh_fast(c[0])
    elif op == "atanh_fast":
        out = twin_atanh_fast(c[0])
    elif op == "sigmoid_f":
        out = twin_sigmoid_f(c[0])
    elif op == "tanh_f":
        out = twin_tanh_f(c[0])
    elif op == "atmosphere":
        out = twin_atmosphere(c[0], **kw)
    elif op == "pitot":
        out = twin_pitot(c[0], c[1])
    elif op == "vcas":
        out = twin_vcas(c[0])
    elif op == "in_range_deg":
        out = twin_in_range_deg(c[0], **kw)
    elif op == "in_range_rad":
        out = twin_in_range_rad(c[0])
    elif op == "slew":
        out = twin_slew(*c[:5])
    elif op == "tef_kinematic":
        out = twin_tef_kinematic(c[0], c[1], **kw)
    elif op == "seek":
        out = twin_seek(*c[:5])
    elif op == "posture_fn":
        out = twin_posture_fn(c[0], c[1], c[2], **kw)
    elif op == "missile_height_f":
        out = twin_missile_height_f(c[0], c[1], c[2], center)
    elif op == "missile_height_d":
        out = twin_missile_height_d(c[0], c[1], c[2], center, **kw)
    elif op == "neu_height64":
        out = twin_neu_height64(c[0], c[1], c[2], center)
    elif op == "locate":
        out = twin_locate(c[0], c[1], c[2], c[3])
    elif op == "locate_fast":
        out = twin_locate_fast(c[0], c[1], c[2])
    else:
        raise KeyError(op)
    out = np.stack([np.asarray(o, dtype=np.float64) for o in out], axis=1) if isinstance(out, tuple) else np.asarray(out, dtype=np.float64)
    return out.reshape(-1, 1) if out.ndim == 1 else out


N_OUT = {"fx_sqrt_both": 2, "fx_sincos": 2, "atmosphere": 4, "locate": 10, "locate_fast": 10}


@functools.lru_cache(maxsize=None)
def scale(op, center=CENTER):
    """What one unit of the op's figure is, per row and output, float64 [n][c] (see the module docstring)."""
    X = inputs(op)
    ref = reference(op, center)[0]
    one = np.ones_like(ref)
    if op in ("fx_rcp", "fx_rsqrt", "fx_sqrt", "fx_sqrt_both", "atmosphere"):
        s = np.abs(ref)
        if op == "atmosphere":
            # pressure (and density with it) by layer, from the derivation at ALLOWANCE["atmosphere"]
            gp = X[:, 0] * ATM_RE / (ATM_RE + X[:, 0])
            w = np.where(gp < ATM_H[1], 9.5, np.where(gp < ATM_H[2], 4.2, 39.6))
            s = s * np.stack([np.full_like(w, 0.34), w, w + 1.34, np.full_like(w, 1.2)], axis=1)
        if op == "fx_sqrt":
            s = np.where(ref == 0.0, 1.0, s)
        return s
    if op == "pow_pos":
        return np.abs(ref) * (1.0 + math.log(2.0) * np.abs(X[:, 1:2] * np.log2(X[:, 0:1])))
    if op == "atanh_fast":
        return 1.0 + 2.0 * np.abs(ref)
    if op == "pitot":
        return ref + X[:, 1:2]                              # the total pressure p x ratio: the impact pressure is a difference of it and p
    if op == "vcas":
        M = ref_mach_from_qc(X[:, 0:1])
        asl = math.sqrt(1.4 * ATM_R * 518.67)
        return asl * np.where(M > 1.0, 4.2 * M, 1.32 * 2.5 * (1.0 + 0.2 * M * M) / M + M)
    if op == "posture_fn":
        _, orn, rng, x = ref_posture(X[:, 0:1], X[:, 1:2], X[:, 2:3])
        return rng * (1.0 + 1.0 / (PI * (1.0 - x * x))) + np.abs(orn)
    return one


# Allowance for the hardware approximations, in units of `scale`, per output. U = 2^-23.
ALLOWANCE = {
    # v_rcp_f64 / v_rsq_f64 seeds: relative error e0 <= 2^-24 on the device (ISA: 2^29 ulp), as the twin's float32-rounded seed; a
    # Newton step squares it, so after two steps 2^-96 remains: nothing.
    "fx_rcp": (0.0,), "fx_rsqrt": (0.0,), "fx_sqrt": (0.0,), "fx_sqrt_both": (0.0, 0.0),
    # fma, multiply, rint and selects only: the device is IEEE here
    "fx_sincos": (0.0, 0.0, 0.0, 0.0),
    # a = mn * v_rcp(mx): relative U on a; d atan(a) = da / (1 + a^2) = a U / (1 + a^2) <= U / 2   [rad]
    "atan2_fast": (0.5 * U,),
    # y = v_sqrt(...): relative U, then the same reciprocal: relative 2 U on a -> 2 * U / 2 = U   [rad]
    "acos_fast": (U,),
    # exp2(y * log2 x): v_log relative U on L = log2 x -> the exponent moves by |y L| U -> relative ln2 |y L| U on the result; v_exp adds
    # U. The scale is |ref| (1 + ln2 |y log2 x|), so the allowance is U.
    "pow_pos": (U,),
    # t = v_exp(..): relative U; d((t - 1) / (t + 1)) = 2 t / (t + 1)^2 x U <= U / 2; the divide (v_rcp + multiply): U |result| <= U
    "tanh_fast": (1.5 * U,),
    # q = (1 + x) / (1 - x): the divide moves log q by U; the logarithm is good to U relative: U |log q|; halved:
    # U / 2 (1 + 2 |atanh x|), and the scale is 1 + 2 |ref|
    "atanh_fast": (0.5 * U,),
    # e = v_exp(-x): d(1 / (1 + e)) = s (1 - s) U <= U / 4; the divide: U s <= U
    "sigmoid_f": (1.25 * U,),
    # t = v_exp(2x): d(2 / (t + 1)) = 2 t / (t + 1)^2 U <= U / 2; the divide: U x 2 / (t + 1) <= 2 U
    "tanh_f": (2.5 * U,),
    # gp = h Re / (Re + h): the divide puts U on gp.
    #  T = 518.67 + L0 gp: |L0 gp| / T <= 128.7 / 390 = 0.33 (troposphere); 389.97 + L2 (gp - hb2): L2 gp U / T <= 43.7 / 398 = 0.11 -> 0.34 U.
    #  P = Pb exp2(-k log2(T / Tb)), k = g0R / L: v_log U on the logarithm, T / Tb carries T's 0.33 U (0.11 U) and a reciprocal's U; v_exp U.
    #    troposphere  k = 5.256, |k log2| <= 2.162:  ln2 2.162 U + 5.256 (0.33 + 1) U + U = 9.5 U
    #    upper layer  k = 34.16, |k log2| <= 0.967:  ln2 0.967 U + 34.16 (0.11 + 1) U + U = 39.6 U
    #    isothermal   P = Pb exp2(c (gp - hb1)), |c| gp <= 4.55:  ln2 4.55 U + U = 4.2 U
    #  rho = P / (R T): P's, T's 0.34 U and the divide's U.   a = v_sqrt(1.4 R T): 0.17 U + U = 1.2 U.
    # These weights are in `scale`; the allowance is U.
    "atmosphere": (U, U, U, U),
    # subsonic x^3 v_sqrt(x): U on the ratio; supersonic ... / (y^2 v_sqrt(y)): the square root's U and the divide's U. The scale is the
    # total pressure p x ratio.
    "pitot": (2.0 * U,),
    # A = qc / psl + 1: the divide moves A by (A - 1) U. pw = pow_pos(A, 1 / 3.5): U + ln(A) / 3.5 U + (A - 1) / (3.5 A) U <= 1.32 U for
    # A <= 1.893 (M = 1). M = v_sqrt(5 (pw - 1)): dM = 2.5 pw x 1.32 U / M, and the square root's U M: the subsonic scale.
    # Supersonic: M <- c sqrt(A w^2.5), w = 1 - 1 / (7 M^2). One pass: the divide puts U / (7 M^2 - 1) <= U / 6 on w; pow_pos:
    # U + 2.5 ln(1 / w) U + 2.5 U / 6 <= 1.81 U; halved by the root: 0.9 U, the root's own U, A's U / 2: 2.4 U. The map contracts by
    # M g' / g = 1.25 (2 / 7 M^2) / (1 - 1 / 7 M^2) <= 0.417, so the passes sum to 2.4 U / (1 - 0.417) = 4.2 U relative: the supersonic scale.
    "vcas": (U,),
    # x = 1 - 2 TA / pi: the divide puts 2 U on x, atanh' = 1 / (1 - x^2), / 2 pi: U / (pi (1 - x^2)), the scale's second term. The rest on
    # the orientation: atanh_fast's own U / 2 (1 + 2 x 8.7) / 2 pi = 1.46 U, its division by 2 pi: 8.7 U / 2 pi = 1.4 U, the two divides of
    # 1 / (50 AO / pi + 2): U; together 3.9 U x range factor. v_exp on the range factor: 0.2 U x |orientation|.
    "posture_fn": (4.0 * U,),
    # n^2 / (2 (rm0 + u)) and e^2 / (2 (rn0 + u)), each at most 60 km^2 / (2 x 6.36e6 m) = 283 m, each divide U of it   [m]
    "missile_height_f": (2 * 283.0 * U,),
    "missile_height_d": (0.0,), "neu_height64": (0.0,),
    "locate": (0.0,) * 10,
    # altitude: b x ser is up to a - b = 70 160 ft and carries the U of the divide in cos^2 = p2 / (p2 + z^2): 0.0084 ft.
    # unit vectors: the two v_rsq (and a v_sqrt whose error the normalisation cancels to e^2 x 3 U) put U on each of the two factors of a
    # component: 2.1 U.
    "locate_fast": (70160.0 * U,) + (2.1 * U,) * 9,
}

# The twin's worst |error| / scale over the op's input set (tests/test_math_probe_host.py recomputes each within 5 %).
TWIN = {
    "fx_rcp": (1.110e-16,),
    "fx_rsqrt": (2.292e-16,),
    "fx_sqrt": (1.110e-16,),
    "fx_sqrt_both": (1.110e-16, 2.292e-16),
    "fx_sincos": (1.211e-16, 1.246e-16, 2.013e-16, 2.071e-16),
    "atan2_fast": (2.910e-07,),
    "acos_fast": (3.066e-07,),
    "pow_pos": (7.910e-08,),
    "tanh_fast": (1.327e-07,),
    "atanh_fast": (5.389e-08,),
    "sigmoid_f": (8.897e-08,),
    "tanh_f": (1.756e-07,),
    "atmosphere": (2.689e-07, 1.259e-07, 1.050e-07, 1.107e-07),
    "pitot": (4.013e-07,),
    "vcas": (7.464e-08,),
    "posture_fn": (2.447e-07,),
    "missile_height_f": (4.038e-02,),
    "missile_height_d": (4.017e-02,),
    "neu_height64": (2.296e-09,),
    "locate": (3.904e-03, 1.267e-07, 1.388e-07, 2.980e-08, 8.330e-08, 1.086e-07, 0.000e+00, 1.085e-07, 1.462e-07, 2.980e-08),
    "locate_fast": (2.110e-02, 2.079e-07, 1.894e-07, 1.624e-07, 1.331e-07, 1.284e-07, 0.000e+00, 2.297e-07, 2.196e-07, 1.630e-07),
}
TEF_BOUND = 2.0 ** -22
TEF_TIE = 1e-6


def figures(op, got, center=CENTER):
    """|got - reference| / scale, float64 [n][c]."""
    hi, lo = reference(op, center)
    got = np.asarray(got, dtype=np.float64)[:, :hi.shape[1]]
    err = np.abs((got - hi) - lo)
    if op == "fx_sincos":   # held both ways: outputs 0, 1 absolute, 2, 3 relative
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.concatenate([err, np.where(err == 0.0, 0.0, err / np.abs(hi + lo))], axis=1)
    return err / scale(op, center)


def bound(op):
    return 2.0 * np.asarray(TWIN[op]) + np.asarray(ALLOWANCE[op])


@functools.lru_cache(maxsize=None)
def tef_keep():
    """Rows of tef_kinematic's input set whose FGKinemat walk is not within TEF_TIE of a tie in its remaining-time comparison."""
    X = inputs("tef_kinematic")
    return np.array([ref_kinemat(o, i)[1] for o, i in X]) >= TEF_TIE


def mismatches(op, got):
    """For an op that has no tolerance: which rows of `got` differ from the float32 twin in any bit, bool [n]."""
    g32, w32 = np.asarray(got, dtype=np.float64)[:, :1].astype(f32), twin(op).astype(f32)
    return (g32.view(np.uint32) != w32.view(np.uint32))[:, 0]


def ratios(op, got, center=CENTER):
    """figure / bound per row and output, float64 [n][c]: the op holds where every entry is <= 1."""
    fig = figures(op, got, center)
    if op == "tef_kinematic":
        fig, b = np.where(tef_keep()[:, None], fig, 0.0), np.array([TEF_BOUND])
    else:
        b = bound(op)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(fig == 0.0, 0.0, fig / b)
    if op == "fx_sqrt":   # sqrt(0) is 0 exactly
        r = np.where((inputs(op) == 0.0) & (np.asarray(got, dtype=np.float64)[:, :1] != 0.0), np.inf, r)
    return np.where(np.isnan(r), np.inf, r)


def compare(op, got, center=CENTER):
    """The GPU test's comparison: (ok, message). `got` [n][>= c] are the op's outputs on inputs(op)."""
    X = inputs(op)
    got = np.asarray(got, dtype=np.float64)
    if op in EXACT_OPS:
        bad = mismatches(op, got)
        if not bad.any():
            return True, f"{op}: {X.shape[0]} rows equal the float32 twin bit for bit"
        i = int(np.flatnonzero(bad)[0])
        return False, (f"{op}: {int(bad.sum())} rows differ from the float32 twin, first at row {i}: in {X[i].tolist()} got {got[i, 0]!r} "
                       f"want {twin(op)[i, 0]!r}")
    r = ratios(op, got, center)
    i, k = np.unravel_index(int(np.argmax(r)), r.shape)
    ref = reference(op, center)[0]
    c = k % ref.shape[1]
    return bool(r[i, k] <= 1.0), (f"{op}: worst error / bound = {r[i, k]:.3f} at row {i} output {k}: in {X[i].tolist()} got {got[i, c]!r} "
                                  f"reference {ref[i, c]!r}")
