"""Cases, reference, CPU twins and bounds for the device missile integrators (ac_probe_missile, include/aircombat.h).

One level above math_probe_util.py: there each device primitive is held to its own bound, here the whole missile tick is -- both
`missile_run` forms of csrc/aircombat.hip, run tick by tick by the probe kernel (csrc/missile_probe.hpp) and compared with the oracle's
`or_missile_run` (oracle/combat_env.c, through or_missile_raw_flyout at the handle's battle-field centre).

* CASES (`group(name)`): seeded and fixed. The reference's own fly-outs of tests/golden/missile.npz, a grid around the over-the-top
  starts (stored pitch past pi/2), launches from 1 km to 18 km in every heading quadrant and at steep dive angles, targets that die in
  flight, every ending (HIT, time-out of either parameter set, v_min, 300 receding ticks, target death), at four battle-field centres.
  `coverage()` derives what the cases reach from the ORACLE's runs alone.
* REFERENCE (`fly("ref", ...)`): simulatior.py:520-608 restated in plain float64 numpy, with the exact geodetic height. It is held to the
  oracle and to the fixture rows at the tolerances of test_oracle_golden.py::test_missile_flyouts (tests/test_missile_probe_host.py).
* TWINS (`fly("twin32", ...)`, `fly("twin64", ...)`): the device's arithmetic with correctly rounded elementary functions. twin32 is
  float32 throughout with the tick-count clock and the local-curvature height (form 0); twin64 keeps the state and the guidance in
  float64 and takes the drag side -- height, density, reference area, thrust minus drag, dv/dt -- in float32 (form 1).
* BOUND, per form, field, row and tick:  B = running max over the ticks of  2 x |twin - oracle| + A.  A is the allowance for what the
  device does differently from its twin in ONE tick -- the hardware approximations (v_rcp_f32, v_sqrt_f32, v_exp_f32: one ulp each,
  U = 2^-23, math_probe_util.py; sin_rate's 6e-8 truncation; the fp64 fx:: forms' 2 ulp), fused multiply-adds the twin does not
  make, and in form 0 the half-ulp roundings of an fp32 state -- summed over the ticks flown so far: what may err the same way at every
  tick linearly, the state's own roundings in quadrature at four sigma (`_allowance`, where each term's derivation stands). How a tick's
  error GROWS through the guidance loop is not in A: that is what the twin's own deviation from the oracle samples, doubled; in form 0
  it is the largest deviation of the twin and JITTERS jittered twins. B never comes from the device.
* COMPARISON (`compare`): the continuous fields while the oracle's missile is still closing, up to and including its first receding
  tick or its ending (the convention of open_loop_util.py: near a pass the demands hinge on centimetres), in form 0 also only until the
  stored pitch comes near the vertical (`Run.window`); the discrete facts -- status,
  hence the ending tick, the receding count, `moved`, and through the mass the burn-out tick -- at EVERY tick, except around a decision
  of the oracle's own (range against Rc, speed against v_min, range against the previous range) that lies within B of its threshold:
  there the device may rightly decide the other way, and `Run.plan` leaves out only the facts and ticks that decision touches (the
  count until it is reset, the status for the few ticks by which an ending may shift). A row whose ending itself is in doubt is cut
  short there; `EXCLUDE_CAP` limits those rows per group, with no group and no row exempt, and the host test holds the oracle to it.
"""
import ctypes as C
import functools
import math
import os

import numpy as np

import math_probe_util as MP

f32 = np.float32
U = MP.U                 # one ulp of a float32 result, relative
E = 2.0 ** -53
DT = 1.0 / 60.0
RECEDE_MAX = 300
LAUNCHED, HIT, MISS = 0, 1, 2
FP32, FP64 = 0, 1
AIM9L, AIM120B = 0, 1
# the probe's out row (include/aircombat.h)
O_STATUS, O_P, O_V, O_TH, O_PS, O_T, O_M, O_DTH, O_DPH, O_DPREV, O_REC, O_MOVED, N_OUT = 0, 1, 4, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16
FIELDS = {"pos": (1, 4), "vel": (4, 7), "theta": (7, 8), "psi": (8, 9), "t": (9, 10), "m": (10, 11), "dtheta": (11, 12), "dphi": (12, 13),
          "dprev": (13, 14)}
EXCLUDE_CAP = 0.02
JITTERS = 3
COS_MIN_F32 = 0.25
DEFAULT_CENTER = MP.CENTER                                   # lat, lon, alt
CENTERS = {"default": DEFAULT_CENTER, "equator": (0.0, 0.0, 0.0), "arctic": (85.0, 179.9, 0.0), "antarctic": (-75.0, -179.9, 0.0)}
# simulatior.py:421-433 (AIM-9L, MissileSimulator's defaults) and :659-672, :696-709 (the set AIM_9M and AIM_120B carry)
PARAMS = {
    AIM9L: dict(g=9.81, t_max=60.0, t_thrust=3.0, Isp=120.0, Length=2.87, Diameter=0.127, cD=0.4, m0=84.0, dm=6.0, K=3.0, nyz_max=30.0,
                Rc=300.0, v_min=150.0),
    AIM120B: dict(g=9.81, t_max=27.22, t_thrust=1.4, Isp=1837.0, Length=3.66, Diameter=0.18, cD=0.02, m0=152.0, dm=6.0, K=5.0, nyz_max=50.0,
                  Rc=5.0, v_min=150.0),
}
# what the step kernels fly: (form, model)
PRODUCTION = ((FP32, AIM9L), (FP64, AIM120B), (FP64, AIM9L))


def _tick_sum(limit, strict):
    """The first tick whose float64 running sum of 1/60 is >= limit (> limit when strict): the device's k_burnout / k_timeout."""
    t, k = 0.0, 0
    while True:
        t += 1.0 / 60.0
        k += 1
        if (t > limit) if strict else (t >= limit):
            return k


K_BURNOUT = {m: _tick_sum(PARAMS[m]["t_thrust"], False) for m in PARAMS}
K_TIMEOUT = {m: _tick_sum(PARAMS[m]["t_max"], True) for m in PARAMS}


# ------------------------------------------------------------------------------------------------ one integrator, three arithmetics
FAULTS = ("abs_cos", "burnout_late", "timeout_ge", "recede_noreset", "recede_nosat", "gain_no_max", "guidance_f32", "height_off",
          "dprev_frozen", "tvz_negated")


def _sin32(x):
    return np.sin(x.astype(np.float64)).astype(f32)


def fly(kind, model, launch, target, center=DEFAULT_CENTER, fault=None, want_allowance=False, jitter=None):
    """`ticks` missile ticks for every launch row. kind: "ref" (the reference's formulas, float64), "twin32", "twin64" (the device's
    arithmetic, module docstring). launch [n][>= 15], target [ticks][n][7] as ac_probe_missile takes them. Returns out [ticks][n][16]
    in the probe's layout, and with want_allowance the per-tick allowance A [ticks][n][16] beside it (twins only).
    fault (twins): one of FAULTS, planted to show that the comparison can fail.
    jitter (twin32): a seed. The speed's square root and the four sines and cosines that rebuild the velocity are moved by one ulp up
    or down, drawn per tick and row: what v_sqrt_f32 and sincosf may do on the device, so that the jittered twins sample how such
    per-tick errors grow through the flight."""
    assert kind in ("ref", "twin32", "twin64") and (fault is None or fault in FAULTS)
    P = PARAMS[model]
    R = f32 if kind == "twin32" else np.float64
    launch = np.asarray(launch, dtype=np.float64)
    n, ticks = launch.shape[0], target.shape[0]
    p = [launch[:, i].astype(R) for i in range(3)]
    v = [launch[:, 3 + i].astype(R) for i in range(3)]
    th, ps, t, m, dth, dph, dprev = (launch[:, i].astype(R) for i in range(6, 13))
    rec = launch[:, 13].astype(np.int64)
    status = launch[:, 14].astype(np.int64)
    k = np.rint(launch[:, 8] * 60.0).astype(np.int64)
    shot = np.zeros(n, dtype=bool)
    jit = np.random.default_rng(jitter) if jitter is not None and kind == "twin32" else None
    out = np.zeros((ticks, n, N_OUT))
    A = np.zeros((ticks, n, N_OUT)) if want_allowance else None
    acc = {key: np.zeros(n) for key in ("vs", "vr", "pv", "ths", "thr", "pss", "psr", "poss", "posr", "flown")}
    g, t_max = R(P["g"]), R(P["t_max"])
    dt = R(DT)
    kb, kt = K_BURNOUT[model] + (1 if fault == "burnout_late" else 0), K_TIMEOUT[model]
    old = np.seterr(all="ignore")
    try:
        for j in range(ticks):
            tg = target[j]
            alive = (tg[:, 6] != 0.0) & ~shot
            tp = [tg[:, i].astype(R) for i in range(3)]
            tv = [tg[:, 3 + i].astype(R) for i in range(3)]
            if fault == "tvz_negated":
                tv[2] = -tv[2]
            k = k + 1
            if kind == "ref":
                t = t + DT
                burning, timeout = t < P["t_thrust"], t > P["t_max"]
            else:
                t = k.astype(R) * dt
                burning = k < kb
                timeout = (t >= t_max) if fault == "timeout_ge" else (k >= kt)
            # ---- _guidance (:556-576)
            G = f32 if fault == "guidance_f32" else R
            gp, gv, gtp, gtv = ([x.astype(G) for x in q] for q in (p, v, tp, tv))
            hxy2 = gv[0] * gv[0] + gv[1] * gv[1]
            vm = np.sqrt(hxy2 + gv[2] * gv[2])
            if kind == "ref":
                cth = np.cos(np.arcsin(gv[2] / vm))
            elif kind == "twin32":
                cth = np.sqrt(np.maximum(G(0), G(1) - (gv[2] / vm) * (gv[2] / vm)))
            else:
                cth = np.sqrt(hxy2) / vm
            dd = [gtp[i] - gp[i] for i in range(3)]
            rv = [gtv[i] - gv[i] for i in range(3)]
            Rxy2 = dd[0] * dd[0] + dd[1] * dd[1]
            Rxy = np.sqrt(Rxy2)
            R2 = Rxy2 + dd[2] * dd[2]
            Rxyz = np.sqrt(R2)
            dbeta = (rv[1] * dd[0] - rv[0] * dd[1]) / Rxy2
            deps = (rv[2] * Rxy2 - dd[2] * (dd[0] * rv[0] + dd[1] * rv[1])) / (R2 * Rxy)
            Kg = G(P["K"]) * (G(P["t_max"]) - t.astype(G)) / G(P["t_max"])
            canc_ps = (np.abs(rv[1] * dd[0]) + np.abs(rv[0] * dd[1])) / Rxy2                        # the sizes of what cancels in the two demands
            canc_th = (np.abs(rv[2]) * Rxy2 + np.abs(dd[2]) * (np.abs(dd[0] * rv[0]) + np.abs(dd[1] * rv[1]))) / (R2 * Rxy)
            if fault != "gain_no_max":
                Kg = np.maximum(Kg, G(0))
            ny_raw, nz_raw = Kg * vm / G(P["g"]) * cth * dbeta, Kg * vm / G(P["g"]) * deps + cth
            ny = np.clip(ny_raw, -G(P["nyz_max"]), G(P["nyz_max"])).astype(R)
            nz = np.clip(nz_raw, -G(P["nyz_max"]), G(P["nyz_max"])).astype(R)
            vm, cth, Rxyz = vm.astype(R), cth.astype(R), Rxyz.astype(R)
            if jit is not None:
                vm = (vm * (f32(1.0) + f32(U) * jit.choice(np.float32([-1.0, 1.0]), n))).astype(R)
            # ---- run (:520-533)
            inc = Rxyz > dprev
            if fault == "recede_noreset":
                rec = np.where(inc, np.minimum(rec + 1, RECEDE_MAX), rec)
            elif fault == "recede_nosat" or kind == "ref":
                rec = np.where(inc, rec + 1, 0)          # (the reference's deque decides by sum >= maxlen: the count in a row)
            else:
                rec = np.where(inc, np.minimum(rec + 1, RECEDE_MAX), 0)
            dprev = np.where(status == LAUNCHED, Rxyz, dprev) if fault == "dprev_frozen" else Rxyz
            hit = (Rxyz < R(P["Rc"])) & alive & (status != MISS)
            miss = ~hit & (timeout | (vm < R(P["v_min"])) | (rec >= RECEDE_MAX) | ~alive)
            mv = ~hit & ~miss
            status = np.where(hit, HIT, np.where(miss, MISS, status))
            shot |= hit
            # ---- _state_trans (:578-608) for the rows that move
            if kind == "twin32":
                pn = [MP.fma32(dt, v[i], p[i]) for i in range(3)]
            else:
                pn = [p[i] + dt * v[i] for i in range(3)]
            st, ct = np.sin(th), np.cos(th)
            if kind == "ref":
                alt = MP.ref_neu_height(pn[0], pn[1], pn[2], center)
                Tt = np.where(burning, P["g"] * P["Isp"] * P["dm"], 0.0)
                S = math.pi * (P["Diameter"] / 2) ** 2 + np.hypot(np.sin(dth), np.sin(dph)) * P["Diameter"] * P["Length"]
                rho = 1.225 * np.exp(-alt / 9300)
                Dr = 0.5 * P["cD"] * S * rho * vm ** 2
                nx = (Tt - Dr) / (m * P["g"])
                dv = P["g"] * (nx - st)
            else:
                gf, D0, L0 = f32(P["g"]), f32(P["Diameter"]), f32(P["Length"])
                fvm = vm.astype(f32)
                alt = MP.twin_missile_height_f(pn[0].astype(f32), pn[1].astype(f32), pn[2].astype(f32), center)
                if fault == "height_off":
                    alt = alt + f32(100.0)
                Tt = np.where(burning, gf * f32(P["Isp"]) * f32(P["dm"]), f32(0.0))
                sd, sp = _sin32(dth.astype(f32)), _sin32(dph.astype(f32))
                root = np.sqrt(sd * sd + sp * sp)
                S = f32(math.pi) * f32(0.25) * D0 * D0 + root * D0 * L0
                rho = f32(1.225) * MP._expf(-alt * (f32(1.0) / f32(9300.0)))
                Dr = f32(0.5) * f32(P["cD"]) * S * rho * fvm * fvm
                nx = (Tt - Dr) / (m.astype(f32) * gf)
                dv = (gf * (nx - st.astype(f32))).astype(R)
            if fault == "abs_cos" and kind == "twin64":
                # the shortcut: sines and cosines of the current angles as ratios of the velocity components (cos(theta) = hxy / v >= 0),
                # the new ones by angle addition; the first tick after a launch evaluates the functions
                hxy = np.sqrt(v[0] * v[0] + v[1] * v[1])
                first = k == 1
                st, ct = np.where(first, st, v[2] / vm), np.where(first, ct, hxy / vm)
                cps, sps = np.where(first, np.cos(ps), v[0] / hxy), np.where(first, np.sin(ps), v[1] / hxy)
            ndph = g / vm * (ny / ct)
            ndth = g / vm * (nz - ct)
            if kind == "twin32":
                vn_, psn, thn = MP.fma32(dt, dv, vm), MP.fma32(dt, ndph, ps), MP.fma32(dt, ndth, th)
            else:
                vn_, psn, thn = vm + dt * dv, ps + dt * ndph, th + dt * ndth
            if fault == "abs_cos" and kind == "twin64":
                sa, ca, sb, cb = np.sin(dt * ndth), np.cos(dt * ndth), np.sin(dt * ndph), np.cos(dt * ndph)
                s2, c2, s3, c3 = st * ca + ct * sa, ct * ca - st * sa, sps * cb + cps * sb, cps * cb - sps * sb
            else:
                s2, c2, s3, c3 = np.sin(thn), np.cos(thn), np.sin(psn), np.cos(psn)
                if jit is not None:
                    s2, c2, s3, c3 = ((x * (f32(1.0) + f32(U) * jit.choice(np.float32([-1.0, 1.0]), n))).astype(R) for x in (s2, c2, s3, c3))
            vnew = [vn_ * c2 * c3, vn_ * c2 * s3, vn_ * s2]
            mn = np.where(burning, m - dt * R(P["dm"]), m)
            if want_allowance:
                _allowance(kind, P, acc, mv, k, dict(vm=vm, m=m, alt=alt, S=S, Dr=Dr, Tt=Tt, nx=nx, dv=dv, root=root, ny=ny, nz=nz, ct=ct,
                                                     dth=ndth, dph=ndph, p=pn, th=thn, ps=psn, Rxyz=Rxyz, D0L0=float(D0) * float(L0),
                                                     st=st, Kc_ps=np.maximum(Kg, 0) * canc_ps, Kc_th=np.maximum(Kg, 0) * canc_th, Kg=np.maximum(Kg, 0), cth=cth, Rxy=Rxy,
                                                     relv=np.sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]), ny_raw=ny_raw, nz_raw=nz_raw), A[j])
            p = [np.where(mv, pn[i], p[i]) for i in range(3)]
            v = [np.where(mv, vnew[i].astype(R), v[i]) for i in range(3)]
            th, ps, m = np.where(mv, thn, th), np.where(mv, psn, ps), np.where(mv, mn, m)
            dth, dph = np.where(mv, ndth, dth), np.where(mv, ndph, dph)
            o = out[j]
            o[:, O_STATUS] = status
            for i in range(3):
                o[:, O_P + i], o[:, O_V + i] = p[i], v[i]
            o[:, O_TH], o[:, O_PS], o[:, O_T], o[:, O_M], o[:, O_DTH], o[:, O_DPH], o[:, O_DPREV] = th, ps, t, m, dth, dph, dprev
            o[:, O_REC], o[:, O_MOVED] = rec, mv
    finally:
        np.seterr(**old)
    return (out, A) if want_allowance else out


def _allowance(kind, P, acc, mv, k, q, A):
    """A of one tick (module docstring): what the device's tick may differ from its twin's by, summed over the ticks flown.
    Everything below is per tick and per row, from the twin's own values; `acc` carries the sums. Two kinds of term are summed differently.
    What a hardware approximation or a fused operation does may err the same way at every tick: those terms add up linearly. The
    round-to-nearest roundings of the STATE (the speed rebuilt from its components, the two angle updates, the position update) are
    independent in sign from one tick to the next: their squares add, and four standard deviations of that sum are allowed -- after k
    ticks 4 sqrt(k) eps instead of k eps. This is a statistical allowance, not a worst case: 3600 half-ulp roundings of a 30 km coordinate
    all falling the same way would be 13 m, which no flight shows; four sigma is 0.9 m.

    drag side (float32 in both forms).  sd, sp: sin_rate truncates at 6e-8 and rounds its result (U / 2 of <= 1): 1.2e-7 each, so the
    root moves by at most hypot(1.2e-7, 1.2e-7) = 1.7e-7 and v_sqrt_f32's U; form 0 takes __sinf, v_sin_f32's 4e-7 (the figure beside
    sin_rate in aircombat.hip): 5.7e-7.  S = S0 + root D0 L0: two products and a sum that the compiler may fuse: 3 U of the second term.
    rho = 1.225 exp2(log2e x alt / 9300): v_exp_f32's U, a product's U, and the height's own allowance (math_probe_util's
    missile_height_f: the two divides, 2 x 283 m x U) plus one ulp of alt for the final sum, over 9300 m.  D = cD/2 S rho v^2: four
    products, 2 U more than the twin's.  nx = (T - D) / (m g): the difference may be fused (U of it), the divide is v_rcp_f32 and a
    multiply (1.5 U of nx).  dv = g (nx - sin(theta)): sin(theta) is a ratio of fp64 velocity components cast to float where the twin
    casts the sine (one ulp of <= 1: U), and a product: U of dv.
    speed:  v += dt dv.  Form 1: fx::sqrt_both's 2 ulp and the sum, 4 E v per tick.  Form 0: v_sqrt_f32, the sum of squares, the
    fused update and the three products that rebuild the velocity: 4 U v per tick.
    angles:  theta += dt dtheta, dtheta = g / v (nz - cos theta); psi likewise with ny / cos theta. The speed's allowance moves the rate by
    |rate| A_v / v. Form 1: fx::rcp and the products, 8 E of each term. Form 0: two v_rcp_f32 divides (3 U of the rate), sincosf's 2 U on
    cos theta and 10 U on the fp32 guidance demand (its quotients and square roots), all times g / v; and U / 2 of the angle for the update.
    Both demands are differences of products that all but cancel on a target dead ahead (dbeta, deps): a fused and an unfused evaluation differ
    by an ulp of the products' sizes, so 4 E (4 U) x K x those sizes comes on the rates. And the two rates read the pitch itself: d(dtheta) =
    g / v sin(theta) d(theta), d(dpsi) = dpsi tan(theta) d(theta) -- the pitch allowance so far goes through them, which is what lets the
    allowance grow where the flight passes near the vertical (ny / cos(theta)).
    The demands also read the missile's own velocity and position: the line-of-sight rates are (relative velocity) / range, so the SPEED
    allowance A_v -- what the fp32 drag side puts on the speed, the one error source that is no rounding of the guidance itself -- and the
    along-track position it integrates to, A_pv = sum dt A_v, come on the rates as K (A_v / R + 2 |v_rel| A_pv / R^2) (pitch: the elevation rate is |v_rel| / R across the line of sight) and
    K cos / cos (A_v / Rxy + 2 |v_rel| A_pv / Rxy^2) (heading). Both demands are clamped to +-nyz_max: of such a change only the part beyond the
    margin by which the unclamped demand exceeds the clamp gets through, and never more than the clamp's width (a target passing overhead
    takes Rxy through zero with the heading demand saturated). Only these two, which do not depend on the angles, are carried through
    the demands: feeding the angle allowances back through them as well would treat the guidance loop, which corrects such errors, as if it
    amplified them at K v / R per second.
    velocity components:  A_v + v (A_theta + |cos theta| A_psi) (near the vertical the heading is all but undefined and moves the velocity little), plus the rebuilt sines and cosines: 8 E v (form 1), 6 U v (form 0, sincosf 2 U each).
    position:  p += dt v: the sum of dt x the velocity allowance; form 0 adds an ulp of p per tick (U |p|), form 1 E |p|.
    range (dprev): sqrt(3) x the position allowance (three components), plus the root and the sum of squares: 3 U R (form 0), 4 E R.
    clock: k / 60 rounded once in both: nothing.  mass: m -= dt dm may be fused: E m (U / 2 m in form 0) per burning tick."""
    f = lambda x: np.asarray(x, dtype=np.float64)   # noqa: E731
    vm, m, g = f(q["vm"]), f(q["m"]), P["g"]
    one32 = kind == "twin32"
    ds = 5.7e-7 if one32 else 1.7e-7
    dS = q["D0L0"] * (ds + 4.0 * U * f(q["root"]))
    alt = f(q["alt"])
    dalt = MP.ALLOWANCE["missile_height_f"][0] + U * np.abs(alt)
    Dr = f(q["Dr"])
    dD = Dr * (dS / f(q["S"]) + 2.0 * U + dalt / 9300.0 + 2.0 * U)
    dnx = (dD + U * np.abs(f(q["Tt"]) - Dr)) / (m * g) + 1.5 * U * np.abs(f(q["nx"]))
    ddv = g * (dnx + U) + U * np.abs(f(q["dv"]))
    r = U if one32 else E
    flown = mv.astype(np.float64)
    acc["flown"] += flown
    # systematic parts add tick by tick; the roundings of the state, independent in sign from tick to tick, in quadrature, taken at four sigma
    acc["vs"] += flown * DT * ddv
    acc["vr"] += flown * (4.0 * r * vm) ** 2
    acc_v = acc["vs"] + 4.0 * np.sqrt(acc["vr"])
    acc_th, acc_ps = acc["ths"] + 4.0 * np.sqrt(acc["thr"]), acc["pss"] + 4.0 * np.sqrt(acc["psr"])
    dth, dph, ct = np.abs(f(q["dth"])), np.abs(f(q["dph"])), np.abs(f(q["ct"]))
    gv = g / vm
    tan = np.abs(f(q["st"])) / ct
    if one32:
        rate_th = dth * acc_v / vm + 3.0 * U * dth + gv * (2.0 * U + 10.0 * U * (np.abs(f(q["nz"])) + 1.0))
        rate_ps = dph * acc_v / vm + 3.0 * U * dph + gv / ct * (2.0 * U * np.abs(f(q["ny"])) + 10.0 * U * (np.abs(f(q["ny"])) + 1.0))
        upd_th, upd_ps = 0.5 * U * np.abs(f(q["th"])), 0.5 * U * np.abs(f(q["ps"]))
    else:
        rate_th = dth * acc_v / vm + 8.0 * E * (dth + gv * (np.abs(f(q["nz"])) + 1.0))
        rate_ps = dph * acc_v / vm + 8.0 * E * (dph + gv * np.abs(f(q["ny"])) / ct)
        upd_th, upd_ps = E * np.abs(f(q["th"])), E * np.abs(f(q["ps"]))
    Kg, Rr, Rxy, relv, nyz = f(q["Kg"]), f(q["Rxyz"]), f(q["Rxy"]), f(q["relv"]), P["nyz_max"]
    d_ny = vm / g * f(q["cth"]) * (4.0 * r * f(q["Kc_ps"]) + Kg * (acc_v / Rxy + 2.0 * relv * acc["pv"] / (Rxy * Rxy)))
    d_nz = vm / g * (4.0 * r * f(q["Kc_th"]) + Kg * (acc_v / Rr + 2.0 * relv * acc["pv"] / (Rr * Rr)))
    d_ny = np.clip(d_ny - np.maximum(np.abs(f(q["ny_raw"])) - nyz, 0.0), 0.0, 2.0 * nyz)      # (what of it gets through the clamp)
    d_nz = np.clip(d_nz - np.maximum(np.abs(f(q["nz_raw"])) - nyz, 0.0), 0.0, 2.0 * nyz)
    d_ny, d_nz = np.where(np.isfinite(d_ny), d_ny, 2.0 * nyz), np.where(np.isfinite(d_nz), d_nz, 2.0 * nyz)
    rate_th = rate_th + gv * d_nz + gv * np.abs(f(q["st"])) * acc_th
    rate_ps = rate_ps + gv / ct * d_ny + dph * tan * acc_th
    acc["pv"] += flown * DT * acc_v
    acc["ths"] += flown * DT * rate_th
    acc["thr"] += flown * upd_th ** 2
    acc["pss"] += flown * DT * rate_ps
    acc["psr"] += flown * upd_ps ** 2
    acc_th, acc_ps = acc["ths"] + 4.0 * np.sqrt(acc["thr"]), acc["pss"] + 4.0 * np.sqrt(acc["psr"])
    a_vel = acc_v + vm * (acc_th + np.minimum(ct + acc_th, 1.0) * acc_ps) + (6.0 * U if one32 else 8.0 * E) * vm
    pmax = np.maximum.reduce([np.abs(f(x)) for x in q["p"]])
    acc["poss"] += flown * DT * a_vel
    acc["posr"] += flown * (r * pmax) ** 2
    acc_pos = acc["poss"] + 4.0 * np.sqrt(acc["posr"])
    A[:, O_P:O_P + 3] = acc_pos[:, None]
    A[:, O_V:O_V + 3] = a_vel[:, None]
    A[:, O_TH], A[:, O_PS] = acc_th, acc_ps
    A[:, O_DTH], A[:, O_DPH] = rate_th, rate_ps
    A[:, O_DPREV] = math.sqrt(3.0) * acc_pos + (3.0 * U if one32 else 4.0 * E) * f(q["Rxyz"])
    A[:, O_M] = (0.5 * U if one32 else E) * m * np.minimum(acc["flown"], 200.0)
    A[:, O_T] = 0.0


# ------------------------------------------------------------------------------------------------ the oracle
def oracle_fly(model, launch, target, center=DEFAULT_CENTER):
    """or_missile_run for every launch row against the target table at battle-field centre `center` (lat, lon, alt), in the probe's
    out layout [ticks][n][16]; the receding count is the oracle's own, which does not saturate."""
    from oracle import oracle as O
    L = O.lib()
    launch = np.asarray(launch, dtype=np.float64)
    target = np.ascontiguousarray(target, dtype=np.float64)
    n, ticks = launch.shape[0], target.shape[0]
    st = np.zeros((n, 20))
    st[:, 0] = launch[:, 14]
    st[:, 1:14] = launch[:, 0:13]
    st[:, 14] = launch[:, 13]
    raw = np.zeros((ticks, n, 20))
    dp = C.POINTER(C.c_double)
    L.or_missile_raw_flyout(st.ctypes.data_as(dp), n, ticks, int(model), target.ctypes.data_as(dp), float(center[1]), float(center[0]),
                            float(center[2]), raw.ctypes.data_as(dp))
    out = np.zeros((ticks, n, N_OUT))
    out[:, :, 0:14] = raw[:, :, 0:14]
    out[:, :, O_REC] = raw[:, :, 14]
    # moved = run() took _state_trans: the position changed (at 150 m/s and more it always does). A MISS entry moves again whenever
    # none of the MISS conditions holds at a later tick (:528-533), e.g. once the receding count has reset: its status stays MISS.
    before = np.concatenate([launch[None, :, 0:3], raw[:-1, :, 1:4]], axis=0)
    out[:, :, O_MOVED] = (raw[:, :, 1:4] != before).any(axis=2)
    return out


# ------------------------------------------------------------------------------------------------ cases
def launch_row(pos, speed, theta, psi, model, vel=None):
    """A launch as MissileSimulator.launch leaves it (:493-514): velocity along (theta, psi) unless given, clock 0, full mass, no turn
    rates, previous range inf, empty receding record."""
    row = np.zeros(16)
    row[0:3] = pos
    row[3:6] = vel if vel is not None else (speed * math.cos(theta) * math.cos(psi), speed * math.cos(theta) * math.sin(psi), speed * math.sin(theta))
    row[6], row[7], row[8], row[9], row[12] = theta, psi, 0.0, PARAMS[model]["m0"], np.inf
    return row


def target_track(ticks, p0, speed, heading, climb=0.0, turn=0.0, dies_at=None):
    """[ticks][7]: a target at p0 (NEU) flying `speed` m/s over the ground on `heading`, turning `turn` rad/s and climbing `climb` m/s. The
    velocity record is the pose's (north, east, DOWN) one (simulatior.py:249-252), which the reference's guidance reads as it stands."""
    tt = (np.arange(ticks) + 1.0) * DT
    h = heading + turn * tt
    if turn != 0.0:
        pn = p0[0] + speed / turn * (np.sin(h) - math.sin(heading))
        pe = p0[1] - speed / turn * (np.cos(h) - math.cos(heading))
    else:
        pn, pe = p0[0] + speed * math.cos(heading) * tt, p0[1] + speed * math.sin(heading) * tt
    tr = np.zeros((ticks, 7))
    tr[:, 0], tr[:, 1], tr[:, 2] = pn, pe, p0[2] + climb * tt
    tr[:, 3], tr[:, 4], tr[:, 5] = speed * np.cos(h), speed * np.sin(h), -climb
    tr[:, 6] = 1.0
    if dies_at is not None:
        tr[dies_at:, 6] = 0.0
    return tr


# the four over-the-top starts: (north, up) of the target from the launch point, launch pitch, target's northward speed
OVER_THE_TOP_STARTS = ((1000.0, 3000.0, 0.8, -300.0), (600.0, 3000.0, 1.45, -300.0), (300.0, 3000.0, 1.45, -150.0), (1500.0, 5000.0, 0.8, -300.0))


def _golden_group(model):
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "missile.npz"))
    ids = [c for c in range(int(g["n"][0])) if int(g[f"c{c}_model"][0]) == model]
    ticks = max(len(g[f"c{c}_rows"]) for c in ids)
    launch, target = [], np.zeros((ticks, len(ids), 7))
    for r, c in enumerate(ids):
        par, rows = g[f"c{c}_parent"], g[f"c{c}_rows"]
        launch.append(launch_row(par[3:6], 0.0, par[10], par[11], model, vel=par[6:9]))      # exactly as test_missile_flyouts launches
        target[:len(rows), r, 0:6] = rows[:, 3:9]
        target[:len(rows), r, 6] = rows[:, 1]
        # (the shorter fly-outs: the target flies on along its last velocity record, so that the range keeps changing)
        last, more = target[len(rows) - 1, r], np.arange(1, ticks - len(rows) + 1)[:, None] * DT
        target[len(rows):, r] = last
        target[len(rows):, r, 0:3] = last[0:3] + more * (np.array([last[3], last[4], -last[5]]) + np.array([0.0, 0.0, 1e-3]))
    return np.array(launch), target, ids


def _over_top_group(model):
    ticks, launch, tracks = 700, [], []
    starts = list(OVER_THE_TOP_STARTS)
    for north in (300.0, 600.0, 1000.0, 1500.0, 2500.0):
        for up in (2000.0, 3000.0, 5000.0):
            for pitch in (0.8, 1.15, 1.45):
                for tvn in (-150.0, -300.0):
                    if (north, up, pitch, tvn) not in starts:
                        starts.append((north, up, pitch, tvn))
    for north, up, pitch, tvn in starts:
        launch.append(launch_row((0.0, 0.0, 6000.0), 400.0, pitch, 0.0, model))
        tracks.append(target_track(ticks, (north, 50.0, 6000.0 + up), abs(tvn), math.pi if tvn < 0 else 0.0))
    return np.array(launch), np.stack(tracks, axis=1)


def _envelope_group(model, n, ticks, seed):
    g = np.random.default_rng(seed)
    launch, tracks = [], []
    pitches = (-1.35, -1.0, -0.5, 0.0, 0.3, 0.9)
    for r in range(n):
        alt = (1000.0, 18000.0)[r] if r < 2 else g.uniform(1000.0, 18000.0)
        psi = (r % 4) * (math.pi / 2) - math.pi + g.uniform(0.1, math.pi / 2 - 0.1)      # every quadrant in turn
        pitch = pitches[(r // 4) % len(pitches)]
        close = r % 3 == 1                        # a third of the rows start near the origin with the target in short reach: what fp32 can decide
        span = 4000.0 if close else 35000.0
        pos = (g.uniform(-span, span), g.uniform(-span, span), alt)
        launch.append(launch_row(pos, g.uniform(250.0, 500.0), pitch, psi, model))
        rng_, brg = (g.uniform(1200.0, 3500.0), psi + g.uniform(-0.4, 0.4)) if close else (g.uniform(3000.0, 18000.0), psi + g.uniform(-1.0, 1.0))
        talt = float(np.clip(alt + rng_ * math.tan(pitch * 0.6) + g.uniform(-2000.0, 2000.0), 500.0, 18000.0))
        tp0 = (pos[0] + rng_ * math.cos(brg), pos[1] + rng_ * math.sin(brg), talt)
        dies = int(g.integers(60, 400)) if r % 9 == 4 else None
        tracks.append(target_track(ticks, tp0, g.uniform(150.0, 400.0), g.uniform(-math.pi, math.pi), climb=g.uniform(-30.0, 30.0),
                                   turn=(0.0 if r % 3 == 0 else g.uniform(-0.15, 0.15)), dies_at=dies))
    return np.array(launch), np.stack(tracks, axis=1)


def _endings_group(model, ticks, reps):
    """Every way a fly-out ends, `reps` rows each, one of each kind in turn.
    Time-out: a distant target that flees slower than the missile coasts, at altitude.
    v_min: a missile late in its flight, motor out, slow and climbing after a target far above (from a launch neither set decays to
    150 m/s early enough for fp32 to decide the tick: the AIM-120B's motor adds 1000 m/s, the AIM-9L needs 40 s).
    Receding: a faster target flying away from the first tick; the count runs to 300 and stays there.
    Target death: the alive flag drops in flight; the target flies straight away, so the range to the stopped missile keeps growing.
    HIT: head-on and crossing targets in reach."""
    g = np.random.default_rng(101 + model)
    launch, tracks = [], []
    far = 45000.0 if model == AIM9L else 52000.0
    for i in range(reps):
        alt, psi = g.uniform(14000.0, 18000.0), g.uniform(-math.pi, math.pi)                                        # time-out
        pos = (-28000.0 * math.cos(psi), -28000.0 * math.sin(psi), alt)
        launch.append(launch_row(pos, g.uniform(400.0, 480.0), 0.02, psi, model))
        tracks.append(target_track(ticks, (pos[0] + far * math.cos(psi), pos[1] + far * math.sin(psi), alt + 500.0), g.uniform(240.0, 310.0), psi + g.uniform(-0.1, 0.1)))
        alt, psi = g.uniform(1000.0, 4000.0), g.uniform(-math.pi, math.pi)                                          # v_min
        pos = (g.uniform(-9000.0, 9000.0), g.uniform(-9000.0, 9000.0), alt)
        row = launch_row(pos, g.uniform(158.0, 175.0), g.uniform(0.7, 1.0), psi, model)
        burnt = K_BURNOUT[model] - 1
        row[8], row[9] = (20.0, 12.0)[model], PARAMS[model]["m0"] - burnt * DT * PARAMS[model]["dm"]
        launch.append(row)
        tracks.append(target_track(ticks, (pos[0] + 4000.0 * math.cos(psi), pos[1] + 4000.0 * math.sin(psi), alt + 16000.0), 200.0, psi))
        alt, psi = g.uniform(3000.0, 12000.0), g.uniform(-math.pi, math.pi)                                         # receding from the start
        pos = (g.uniform(-3000.0, 3000.0), g.uniform(-3000.0, 3000.0), alt)
        launch.append(launch_row(pos, 300.0, 0.0, psi, model))
        tracks.append(target_track(ticks, (pos[0] + 9000.0 * math.cos(psi), pos[1] + 9000.0 * math.sin(psi), alt), 900.0, psi))
        alt, psi = g.uniform(5000.0, 14000.0), g.uniform(-math.pi, math.pi)                                         # target death
        pos = (g.uniform(-8000.0, 8000.0), g.uniform(-8000.0, 8000.0), alt)
        launch.append(launch_row(pos, 350.0, 0.1, psi, model))
        tracks.append(target_track(ticks, (pos[0] + 12000.0 * math.cos(psi), pos[1] + 12000.0 * math.sin(psi), alt + 800.0), 250.0, psi + g.uniform(-0.2, 0.2),
                                   dies_at=int(g.integers(40, 300))))
        alt, psi = g.uniform(3000.0, 12000.0), g.uniform(-math.pi, math.pi)                                         # HIT
        pos = (g.uniform(-2000.0, 2000.0), g.uniform(-2000.0, 2000.0), alt)
        launch.append(launch_row(pos, 380.0, 0.05, psi, model))
        reach = g.uniform(2000.0, 4000.0)
        tracks.append(target_track(ticks, (pos[0] + reach * math.cos(psi + 0.1), pos[1] + reach * math.sin(psi + 0.1), alt + 300.0), 260.0,
                                   psi + (math.pi, 2.0, -2.2, 3.0)[i % 4]))
    return np.array(launch), np.stack(tracks, axis=1)


class Run:
    """A set of launch rows with its target table, centre and parameter set; the oracle's fly-outs, the twins' and the bounds, each
    computed once and shared read-only."""

    def __init__(self, launch, target, center, model):
        self.launch, self.target, self.center, self.model = launch, target, center, model
        self.ora = oracle_fly(model, launch, target, center)
        for a in (self.launch, self.target, self.ora):
            a.setflags(write=False)
        status = self.ora[:, :, O_STATUS].astype(int)
        self.flying = np.vstack([launch[None, :, 14].astype(int), status[:-1]]) == LAUNCHED     # the tick was run on a missile in flight
        moved = self.ora[:, :, O_MOVED] != 0.0
        self.still = ~self.flying & ~np.maximum.accumulate(moved & ~self.flying, axis=0)        # finished and not moved since
        self._twin, self._B, self._plan = {}, {}, {}

    def twin(self, form):
        """(the twin's fly-outs, the allowance A) in form `form`."""
        if form not in self._twin:
            out, A = fly("twin32" if form == FP32 else "twin64", self.model, self.launch, self.target, self.center, want_allowance=True)
            out.setflags(write=False)
            A.setflags(write=False)
            self._twin[form] = (out, A)
        return self._twin[form]

    def bounds(self, form):
        """B [ticks][n][16]: the running maximum over the ticks of 2 x |twin - oracle| + A (form 0: the largest deviation of four twins)."""
        if form not in self._B:
            tw, A = self.twin(form)
            with np.errstate(invalid="ignore"):
                dev = np.abs(tw - self.ora)
                # form 0: every elementary result on the device is a hardware approximation, an ulp off at every tick, and where a flight is
                # ill-conditioned (ny / cos(theta) near the vertical) ONE twin is one sample of how that grows. The deviation is the largest
                # over the twin and JITTERS jittered twins (fly's `jitter`).
                for seed in range(JITTERS if form == FP32 else 0):
                    dev = np.maximum(dev, np.abs(fly("twin32", self.model, self.launch, self.target, self.center, jitter=1000 + seed) - self.ora))
            dev[~np.isfinite(dev)] = 0.0                   # (inf - inf of the previous range before the first tick's: equal)
            self._B[form] = np.maximum.accumulate(2.0 * dev + A, axis=0)
            self._B[form].setflags(write=False)
        return self._B[form]

    def window(self, form=FP64):
        """[ticks][n] bool: the ticks at which the continuous fields are compared -- while the oracle's missile is still closing, up to
        and including its first receding tick or its ending. In form 0 also only until the stored pitch first comes within COS_MIN_F32 of
        the vertical: the heading rate is g / v ny / cos(theta), an ulp of an fp32 cosine of 0.25 is 5e-7 of it at every tick, and past that
        point two correctly rounded fp32 arithmetics an ulp apart fly metres apart (tests/test_missile_probe_host.py shows it with the
        jittered twins), so no bound taken from one of them holds the other. The discrete facts are compared past that point all the same."""
        stop = (self.ora[:, :, O_REC] > 0) | (self.ora[:, :, O_STATUS] != LAUNCHED)
        steep = np.zeros_like(stop)
        if form == FP32:
            th = np.vstack([self.launch[None, :, 6], self.ora[:-1, :, O_TH]])
            steep = (np.abs(np.cos(th)) < COS_MIN_F32) | (np.abs(np.cos(self.ora[:, :, O_TH])) < COS_MIN_F32)
        stop = stop | steep
        before = np.vstack([np.zeros((1, stop.shape[1]), dtype=bool), np.maximum.accumulate(stop, axis=0)[:-1]])
        return self.flying & ~before & ~steep

    def near(self, form):
        """([ticks][n] bool) x 3: the ticks at which a decision of the oracle's own lies within B of its threshold -- range against Rc
        (in flight), speed against v_min, range against the previous range (at every tick: the receding count runs on after the ending).
        The last one is the sign of dR = R_k - R_k-1, two ranges whose errors are all but equal, so it is held to the bound of dR itself:
        with a = T_k - p_k, b = T_k-1 - p_k-1 and a position error e common to both, | |a - e| - |b - e| - (|a| - |b|) | <= |e| |a - b| /
        min(|a|, |b|) (the gradient of |a - e| - |b - e| is the difference of two unit vectors); to that come what one tick adds -- dt x the
        velocity bound and the growth of the position bound over the tick -- and the rounding of the two ranges themselves."""
        P, launch, ora, fl = PARAMS[self.model], self.launch, self.ora, self.flying
        B = self.bounds(form)
        rng, Br = ora[:, :, O_DPREV], B[:, :, O_DPREV]
        prev_rng = np.vstack([launch[None, :, 12], rng[:-1]])
        speed = np.linalg.norm(np.vstack([launch[None, :, 3:6], ora[:-1, :, O_V:O_V + 3]]), axis=2)
        Bv = np.vstack([np.zeros((1, rng.shape[1])), np.sqrt(3.0) * B[:-1, :, O_V]])
        pos = np.concatenate([launch[None, :, 0:3], ora[:, :, O_P:O_P + 3]], axis=0)        # pos[k] is the position BEFORE tick k's move
        los = self.target[:, :, 0:3] - pos[:-1]                                              # what tick k's range is taken of
        step = np.linalg.norm(np.diff(los, axis=0), axis=2)
        Bp = np.sqrt(3.0) * B[:, :, O_P]
        with np.errstate(invalid="ignore", divide="ignore"):
            BdR = np.zeros_like(rng)
            BdR[1:] = Bp[:-1] * step / np.minimum(rng[1:], rng[:-1]) + DT * np.sqrt(3.0) * B[:-1, :, O_V] + (Bp[1:] - Bp[:-1]) \
                + 2.0 * (3.0 * U if form == FP32 else 4.0 * E) * rng[1:]
            turn = np.abs(rng - prev_rng) <= BdR
            turn[0] = False                                                                  # (nothing recedes from the launch's inf)
            return fl & (np.abs(rng - P["Rc"]) <= Br), np.abs(speed - P["v_min"]) <= Bv, turn

    def plan(self, form):
        """Which discrete facts are compared at which tick. Everything is, except around a decision of the oracle's that lies within B of
        its threshold, where the device may rightly decide the other way:

        * a receding decision (`turn`): the device's count may differ from the tick of the doubt until both counts are reset (the oracle's
          is 0 at a tick without doubt) or both stand at 300; the COUNT is not compared in between, everything else is. If the oracle's
          count comes within the number u of doubtful ticks of 300 in between while the target lives, the MISS by receding itself may come
          u ticks sooner or later: the status is not compared for 2 u + 3 ticks and must agree again afterwards; `moved`, the count, the
          mass and the recorded range are not compared from there on (the entry rests a few ticks' flight from the oracle's).
        * an ending decision in flight (range against Rc, speed against v_min) over ticks T..T2: the device may end a tick sooner or later.
          If the oracle ends inside T..T2+1, status, `moved` and mass are not compared from T until two ticks after, and must agree again
          from then on (a HIT turns MISS on the next tick, the target being dead, and neither a HIT nor a v_min MISS ever moves again); the
          count and the recorded range, which belong to a resting place a tick's flight apart, and the mass are not compared after T.
          If the oracle does not end there (a pass grazing the fuse), or the doubt is about a finished entry's v_min, the row is cut at T.

        Returns dict(status, rec, mass, late: [ticks][n] bool of what is compared; cut [n]: rows cut short, which EXCLUDE_CAP limits;
        windowed [n]: rows with an ending window)."""
        if form in self._plan:
            return self._plan[form]
        near_rc, near_v, turn = self.near(form)
        ticks, n = near_rc.shape
        st, rec = self.ora[:, :, O_STATUS].astype(int), self.ora[:, :, O_REC]
        hit = np.maximum.accumulate(self.flying & (st == HIT), axis=0)
        alive = (self.target[:, :, 6] != 0.0) & ~np.vstack([np.zeros((1, n), dtype=bool), hit[:-1]])
        cs, cr, cm, cv = (np.ones((ticks, n), dtype=bool) for _ in range(4))
        cl = self.still.copy()
        cut, windowed = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        why_cut = {}
        for r in range(n):
            def cut_at(j, why=""):
                cut[r] = True
                why_cut[r] = (why, j)
                cs[j:, r] = cv[j:, r] = cr[j:, r] = cm[j:, r] = cl[j:, r] = False
            end_near = near_rc[:, r] | near_v[:, r]
            idx = np.nonzero(end_near)[0]
            limit = ticks
            if idx.size:
                T = int(idx[0])
                T2 = T
                while T2 + 1 < ticks and end_near[T2 + 1] and self.flying[T2 + 1, r]:
                    T2 += 1
                ended = np.nonzero(self.flying[:, r] & (st[:, r] != LAUNCHED))[0]
                E = int(ended[0]) if ended.size else None
                limit = T
                if not self.flying[T, r] or E is None or not (T <= E <= T2 + 1) or st[E, r] == MISS and rec[E, r] >= RECEDE_MAX:
                    cut_at(T, "ending")
                else:
                    windowed[r] = True
                    hi = min(ticks, max(T2, E) + 3)
                    cs[T:hi, r] = False
                    cr[T:, r] = cm[T:, r] = cl[T:, r] = False
            active, u = False, 0
            tt = np.nonzero(turn[:limit, r])[0]
            for j in range(int(tt[0]), limit) if tt.size else ():
                if turn[j, r]:
                    active, u = True, u + 1
                if not active:
                    continue
                o = rec[j, r]
                if alive[j, r] and RECEDE_MAX - u <= o <= RECEDE_MAX + u:
                    # the MISS by 300 receding ticks (or a MISS entry's standing still) may come up to u ticks sooner or later
                    if self.flying[j, r]:
                        windowed[r] = True
                        cs[j:min(ticks, j + 2 * u + 3), r] = False
                    cv[j:, r] = cr[j:, r] = cm[j:, r] = cl[j:, r] = False
                    break
                cr[j, r] = False
                if not turn[j, r] and (o == 0 or o > RECEDE_MAX + u):
                    active, u = False, 0
                    cr[j, r] = True
        self._plan[form] = dict(status=cs, moved=cs & cv, rec=cr, mass=cm, late=cl, cut=cut, windowed=windowed, why=why_cut)
        return self._plan[form]

    def undecided(self, form):
        """[n] bool: the rows whose discrete comparison is cut short (plan)."""
        return self.plan(form)["cut"]


# A pass that grazes the fuse -- the oracle's missile goes by at 5.9 m of a 5 m fuse, within B -- leaves the ending itself in doubt, and
# the row's discrete comparison has to be cut there (Run.plan). EXCLUDE_CAP allows 2 % of a group's rows to be cut. The generated groups
# are therefore CHOSEN: their builders make candidates, and the first `pick` that no form flown cuts short are the cases (the oracle and
# the twins decide that, never the device). The fixture's fly-outs are taken as they are, and the four named over-the-top starts lead
# their groups; run() asserts that none of them is cut.
# group name -> (builder, centre name, (form, model) combinations, pick); every group is ONE probe launch per combination
def _groups():
    G = {}
    for model, tag in ((AIM9L, "9l"), (AIM120B, "120b")):
        combos = tuple(c for c in PRODUCTION if c[1] == model)
        G[f"golden_{tag}"] = (lambda model=model: _golden_group(model)[:2], "default", combos, None)
        G[f"over_top_{tag}"] = (lambda model=model: _over_top_group(model), "default", combos, 72)
        G[f"envelope_{tag}"] = (lambda model=model: _envelope_group(model, 192, 900, 11 + model), "default", combos, 160)
        G[f"endings_{tag}"] = (lambda model=model: _endings_group(model, 4200 if model == AIM9L else 1800, 5), "default", combos, None)
    for i, cname in enumerate(("equator", "arctic", "antarctic")):
        model = (AIM120B, AIM9L, AIM120B)[i]
        G[f"centre_{cname}"] = (lambda model=model, i=i: _envelope_group(model, 80, 700, 31 + i), cname, tuple(c for c in PRODUCTION if c[1] == model), 64)
    G["centre_arctic_120b"] = (lambda: _over_top_group(AIM120B), "arctic", ((FP64, AIM120B),), 72)
    return G


GROUPS = _groups()
OVER_THE_TOP_GROUPS = ("over_top_9l", "over_top_120b", "centre_arctic_120b")
FIXTURE_GROUPS = ("golden_9l", "golden_120b")
NAMED_STARTS = {"over_top_120b": 4, "centre_arctic_120b": 4}


@functools.lru_cache(maxsize=None)
def run(name):
    build, cname, combos, pick = GROUPS[name]
    launch, target = build()
    model = combos[0][1]
    if pick is not None:
        cand = Run(launch, target, CENTERS[cname], model)
        cut = np.zeros(launch.shape[0], dtype=bool)
        for form, _ in combos:
            cut |= cand.plan(form)["cut"]
        assert not cut[:NAMED_STARTS.get(name, 0)].any(), (name, "a named start is cut short")
        keep = np.nonzero(~cut)[0]
        assert keep.size >= pick, (name, keep.size, pick)
        keep = keep[:pick]
        launch, target = np.ascontiguousarray(launch[keep]), np.ascontiguousarray(target[:, keep])
    return Run(launch, target, CENTERS[cname], model)


def group(name):
    """(launch [n][16], target [ticks][n][7], center (lat, lon, alt), combos ((form, model), ...)) of a case group."""
    r = run(name)
    return r.launch, r.target, r.center, GROUPS[name][2]


def oracle_run(name):
    return run(name).ora


def twin_run(name, form):
    return run(name).twin(form)


# ------------------------------------------------------------------------------------------------ what the cases reach
def facts(ora, launch, model):
    """Per row, from the oracle's run alone: the ending and its cause, and the properties coverage() asks for."""
    ticks, n = ora.shape[:2]
    P = PARAMS[model]
    status = ora[:, :, O_STATUS].astype(int)
    prev_status = np.vstack([launch[None, :, 14].astype(int), status[:-1]])
    flying = prev_status == LAUNCHED                                # the tick was run on a missile still in flight
    th = np.vstack([launch[None, :, 6], ora[:, :, O_TH]])
    ps = np.vstack([launch[None, :, 7], ora[:, :, O_PS]])
    speed_before = np.linalg.norm(np.vstack([launch[None, :, 3:6], ora[:-1, :, O_V:O_V + 3]]), axis=2)
    t = ora[:, :, O_T]
    out = []
    for r in range(n):
        ended = np.nonzero(flying[:, r] & (status[:, r] != LAUNCHED))[0]
        end = int(ended[0]) if ended.size else None
        cause = None
        if end is not None:
            if status[end, r] == HIT:
                cause = "hit"
            elif t[end, r] > P["t_max"]:
                cause = "timeout"
            elif speed_before[end, r] < P["v_min"]:
                cause = "v_min"
            elif ora[end, r, O_REC] >= RECEDE_MAX:
                cause = "recede"
            else:
                cause = "target_death"
        fl = flying[:, r]
        mass = np.concatenate([[launch[r, 9]], ora[:, r, O_M]])
        burn = np.nonzero(np.diff(mass) < 0)[0]
        out.append(dict(end=end, cause=cause,
                        max_dtheta=float(np.abs(np.diff(th[:, r]))[fl].max(initial=0.0)), max_dpsi=float(np.abs(np.diff(ps[:, r]))[fl].max(initial=0.0)),
                        max_theta=float(np.abs(th[1:, r])[fl].max(initial=0.0)),
                        burnout_tick=(int(burn[-1]) + 2 if burn.size and (end is None or end > burn[-1] + 1) else None),
                        max_recede=int(ora[:, r, O_REC].max())))
    return out


@functools.lru_cache(maxsize=None)
def coverage():
    """What the case groups reach, from the oracle's own runs (so that coverage does not depend on the device)."""
    cov = dict(causes={AIM9L: set(), AIM120B: set()}, burnout={}, fallback_rows=0, over_top_hits=0, saturated=0, altitudes=[], quadrants=set(),
               steep_dives=0, dies_in_flight=0, centers=set())
    for name in GROUPS:
        launch, target, center, combos = group(name)
        model = combos[0][1]
        ora = oracle_run(name)
        cov["centers"].add(center)
        for r, fa in enumerate(facts(ora, launch, model)):
            if fa["cause"]:
                cov["causes"][model].add(fa["cause"])
            if fa["burnout_tick"] is not None:
                cov["burnout"].setdefault(model, set()).add(fa["burnout_tick"])
            cov["fallback_rows"] += max(fa["max_dtheta"], fa["max_dpsi"]) > 0.05
            cov["over_top_hits"] += fa["max_theta"] > math.pi / 2 and fa["cause"] == "hit"
            cov["saturated"] += fa["cause"] == "recede" and fa["max_recede"] > RECEDE_MAX
            cov["altitudes"].append(float(launch[r, 2]))
            cov["quadrants"].add((launch[r, 3] > 0, launch[r, 4] > 0))
            cov["steep_dives"] += launch[r, 6] < -0.9
            alive = target[:, r, 6]
            if fa["end"] is not None and fa["cause"] == "target_death" and alive[0] != 0.0:
                cov["dies_in_flight"] += 1
    return cov


# ------------------------------------------------------------------------------------------------ bounds and the comparison
def bounds(name, form):
    return run(name).bounds(form)


def window(name, form=FP64):
    return run(name).window(form)


def undecided(name, form):
    return run(name).undecided(form)


def plan(name, form):
    return run(name).plan(form)


def REFUSALS(capi):
    """(what, index into ac_probe_missile's arguments, the bad value): every call the probe refuses before it touches the device."""
    return (("unknown form", 1, 2), ("negative form", 1, -1), ("unknown model", 2, 2), ("fp32 with the AIM-120B set", 1, FP32), ("n = 0", 3, 0),
            ("n < 0", 3, -3), ("n too large", 3, capi.AC_PROBE_MSL_MAX_ROWS + 1), ("ticks = 0", 4, 0),
            ("ticks too large", 4, capi.AC_PROBE_MSL_MAX_TICKS + 1), ("null launch", 5, None), ("null target", 6, None), ("null output", 7, None),
            ("null handle", 0, None))


DISCRETE = (("status", O_STATUS), ("recede", O_REC), ("moved", O_MOVED))


def compare(name, form, got):
    """Hold `got` [ticks][n][16] (the device's, or a twin's with a planted fault) to the oracle under the module's rules.
    Returns (ok, worst, message): worst maps each continuous field to the largest fraction of its bound used."""
    launch, _, _, combos = group(name)
    ora = oracle_run(name)
    B = bounds(name, form)
    win = window(name, form)
    pl = plan(name, form)
    skip = pl["cut"]
    problems, worst = [], {}
    if not np.isfinite(got[:, :, :O_DPREV]).all():
        problems.append("non-finite values")
    for field, (a, b) in FIELDS.items():
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(got[:, :, a:b] - ora[:, :, a:b])
            frac = np.where(err == 0.0, 0.0, err / B[:, :, a:b])
        frac = np.where(np.isnan(frac), np.inf, frac)
        if field == "dprev":                                   # (inf before the first tick on both sides)
            frac = np.where(np.isinf(got[:, :, a:b]) & np.isinf(ora[:, :, a:b]), 0.0, frac)
        frac = np.where(win[:, :, None], frac, 0.0)
        worst[field] = float(frac.max())
        if worst[field] > 1.0:
            j, r, _ = np.unravel_index(np.argmax(frac), frac.shape)
            problems.append(f"{field}: {worst[field]:.3g} of its bound at tick {j + 1}, row {r} (|error| {err[j, r].max():.3g}, bound {B[j, r, a]:.3g})")
    ref = ora.copy()
    ref[:, :, O_REC] = np.minimum(ref[:, :, O_REC], RECEDE_MAX)     # (the device's count saturates at the deciding value)
    for what, col in DISCRETE:
        if what == "moved" and form == FP32:
            if not (got[:, :, col] == -1.0).all():
                problems.append("moved: the fp32 form reports -1")
            continue
        bad = (got[:, :, col] != ref[:, :, col]) & pl[{"recede": "rec", "moved": "moved"}.get(what, "status")]
        if bad.any():
            j, r = np.argwhere(bad)[0]
            problems.append(f"{what}: {got[j, r, col]:g} against the oracle's {ref[j, r, col]:g} at tick {j + 1}, row {r} ({int(bad.any(axis=0).sum())} rows differ)")
    # a finished missile that has not moved again stands where it ended while run() goes on recording its range: held at every such tick
    with np.errstate(invalid="ignore"):
        late = pl["late"] & ~(np.abs(got[:, :, O_DPREV] - ora[:, :, O_DPREV]) <= B[:, :, O_DPREV])
    if late.any():
        j, r = np.argwhere(late)[0]
        problems.append(f"dprev: {got[j, r, O_DPREV]:.6g} against the oracle's {ora[j, r, O_DPREV]:.6g} on the finished missile of row {r} at tick {j + 1}")
    # the burn-out tick, through the mass: it falls at exactly the ticks at which the oracle's falls
    fell_ref = np.diff(np.concatenate([launch[None, :, 9], ora[:, :, O_M]]), axis=0) < 0
    fell_got = np.diff(np.concatenate([launch[None, :, 9], got[:, :, O_M]]), axis=0) < 0
    bad = (fell_ref != fell_got) & pl["mass"]
    if bad.any():
        j, r = np.argwhere(bad)[0]
        problems.append(f"burn-out: the mass {'falls' if fell_got[j, r] else 'stands'} at tick {j + 1}, row {r}, against the oracle")
    msg = (f"{name} form {form}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f" of the bound; {int(skip.sum())}/{skip.size} rows cut short, {int(pl['windowed'].sum())} with an ending window"
           + ("; " + "; ".join(problems) if problems else ""))
    return not problems, worst, msg


# The twins' worst deviation from the oracle inside the comparison window, per group and form: position [m], velocity [m/s], pitch and
# heading [rad] (tests/test_missile_probe_host.py recomputes each within 5 %).
TWIN = {
    ("golden_9l", FP32): (0.005828, 0.001221, 4.132e-06, 4.197e-06),
    ("golden_9l", FP64): (2.786e-05, 8.752e-06, 5.694e-10, 2.891e-08),
    ("over_top_9l", FP32): (0.01571, 0.00529, 2.552e-05, 4.98e-05),
    ("over_top_9l", FP64): (0.0004373, 0.001695, 4.009e-06, 8.292e-06),
    ("envelope_9l", FP32): (0.04579, 0.009664, 1.761e-05, 2.672e-05),
    ("envelope_9l", FP64): (0.0003533, 4.905e-05, 4.682e-08, 1.106e-07),
    ("endings_9l", FP32): (0.1546, 0.008481, 9.259e-06, 1.335e-05),
    ("endings_9l", FP64): (0.0004234, 1.547e-05, 3.474e-10, 7.393e-09),
    ("golden_120b", FP64): (0.0006603, 0.0001978, 1.576e-07, 8.27e-08),
    ("over_top_120b", FP64): (0.03615, 4.186, 0.001925, 0.03183),
    ("envelope_120b", FP64): (0.001074, 0.001379, 1.036e-06, 8.339e-07),
    ("endings_120b", FP64): (0.001896, 7.522e-05, 4.277e-09, 1.239e-08),
    ("centre_equator", FP64): (0.0008938, 0.0009342, 2.365e-07, 6.944e-07),
    ("centre_arctic", FP32): (0.1467, 0.009911, 1.348e-05, 3.986e-05),
    ("centre_arctic", FP64): (0.0002619, 3.968e-05, 4.065e-08, 1.519e-07),
    ("centre_antarctic", FP64): (0.0009247, 0.0004668, 2.544e-07, 4.174e-07),
    ("centre_arctic_120b", FP64): (0.03614, 4.185, 0.001925, 0.03182),
}


def twin_figures(name, form):
    ora = oracle_run(name)
    tw, _ = twin_run(name, form)
    win = window(name, form)
    fig = []
    for field in ("pos", "vel", "theta", "psi"):
        a, b = FIELDS[field]
        fig.append(float(np.where(win[:, :, None], np.abs(tw[:, :, a:b] - ora[:, :, a:b]), 0.0).max()))
    return tuple(fig)
