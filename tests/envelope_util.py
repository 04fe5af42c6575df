"""Teacher-forced comparison across the envelope of initial conditions, shared by tests/test_envelope_twin.py (CPU: the oracle against a
second oracle) and tests/test_gpu_envelope.py (the device against the oracle).

Every other parity test starts where the shipped YAMLs spawn (60 N, 120 E, 20 000 ft, Mach 0.77). Here the battle-field centre moves to
LOCATIONS (both hemispheres, the equator, all four longitude quadrants, the prime meridian, next to the antimeridian, |lat| up to 85) and
every env of a location flies its own cell (altitude 3 000 - 80 000 ft with values on either side of both atmosphere layer boundaries,
250 - 2 000 ft/s, body v / w, body rates, heading). One device handle serves one location: the centre is per handle.

A Reference is the oracle's own run, computed once per (task, location, seed) and shared: per step the state every aircraft had BEFORE
the step (what both sides are teacher-forced to), the action, and the oracle's observation, reward, done flags and stored record after
it. A side under test (DeviceSide, or OracleUnderTest with an optional transform of the imported state: the fp32 twin, planted faults)
is played against it by compare(), which holds every sample to the suite's existing one-step bounds -- parity_util.obs_bounds and
RewardBound at scale 1, `done` equal, the stored record field by field with the bounds of
test_gpu_parity.py::test_singlecombat_kernel_forms_teacher_forced, the reported pose (geodetic position, attitude, NED velocity, NEU
position) with the first step of the free-flight envelope -- and returns the fraction of each bound used per sample, so that
the worst fraction can be printed per location, atmosphere layer and Mach band. A step on which the oracle ends the episode is compared
on `done` and reward only (both sides reset, to different initial conditions where the cells differ; the next step's
re-synchronisation repairs that)."""
import ctypes as C

import numpy as np

from parity_util import RewardBound, obs_bounds, team_max

OMEGA = 0.00007292115           # rad/s, Earth rotation (f16_fdm.h)
RE_FT = 20855531.5              # 6 356 766 m: the radius of the geopotential altitude (FGStandardAtmosphere)
LAYER_GP_FT = (36089.2388, 65616.7979)


def geometric_ft(gp_ft):
    return gp_ft * RE_FT / (RE_FT - gp_ft)


# (name, centre latitude, centre longitude, offset of the second team in latitude and longitude)
LOCATIONS = (
    ("75S 179.9W", -75.0, -179.9, 0.05, 0.03),      # next to the antimeridian from the west side, not across it
    ("33S 90W", -33.0, -90.0, 0.05, 0.03),
    ("0N 0E", 0.0, 0.0, -0.05, 0.03),               # on the equator and the prime meridian exactly; the second team sits south of the equator
    ("0.01N 0.02E", 0.01, 0.02, 0.05, 0.03),
    ("45N 120E", 45.0, 120.0, 0.05, 0.03),
    ("85N 179.9E", 85.0, 179.9, 0.05, 0.03),        # next to the antimeridian from the east side
    ("85S 90E", -85.0, 90.0, -0.05, 0.03),
    ("33N 45W", 33.0, -45.0, 0.05, 0.03),
    ("0N 120W", 0.0, -120.0, 0.05, 0.03),
    ("60N 0E", 60.0, 0.0, 0.05, -0.03),             # the second team sits west of the prime meridian
)
LOCATION_IDS = [l[0].replace(" ", "_") for l in LOCATIONS]
RAGGED = 4                      # index of the location whose handle has 70 envs (140 lanes: a ragged last workgroup)
ENVS, ENVS_RAGGED, STEPS, HOLD = 16, 70, 12, 4
SEED = 20251019
NVN_LOCATIONS = (0, 2, 7, 5)    # southern + western + antimeridian, equator / prime meridian, north-western, far north

# ft above sea level: 40 ft on either side of both layer boundaries (geometric 36 151.8 and 65 823.9 ft), and the issue's grid around them
ALTITUDES = (3000.0, 12000.0, 30000.0, geometric_ft(LAYER_GP_FT[0]) - 40.0, geometric_ft(LAYER_GP_FT[0]) + 40.0, 45000.0,
             geometric_ft(LAYER_GP_FT[1]) - 40.0, geometric_ft(LAYER_GP_FT[1]) + 40.0, 72000.0, 80000.0)
SPEEDS = (250.0, 500.0, 800.0, 1100.0, 1500.0, 2000.0)
ALTITUDE_LIMIT = -500.0

# The stored accelerations, load factors and the PID words that read them are differences of FORCES, and every aerodynamic force is
# dynamic pressure x area x a coefficient: fp32 rounding of the coefficient and of the flow angles (half an ulp of a 3 000 ft/s inertial
# velocity component is 6e-8 rad of sideslip) therefore grows with the dynamic pressure. Their bounds were stated where the suite
# flies, 800 ft/s at 20 000 ft, 405 lbf/ft^2; here the cells reach ten times that (2 000 ft/s at 3 000 ft). For these words only,
# the bound is the existing one x max(1, qbar / Q_REF), qbar = 0.7 P M^2 of the oracle's state before the step: the fp32 twin needs it
# (rounding vz alone moves `pin_y` by 0.7 of its plain bound at Mach 1.86 and 12 000 ft, 3 600 lbf/ft^2). Observations, rewards,
# positions, velocities, attitude, air data, engine and control-surface words keep the plain bounds.
Q_REF = 405.0
Q_FIELDS = ("ha1x", "ha1y", "ha1z", "wdx", "wdy", "wdz", "aix", "aiy", "aiz", "bax", "bay", "baz", "npx", "npy", "npz",
            "pin_r", "pin_p", "pin_y", "pi_r", "pi_p", "pi_y")

MACH_BANDS = ("M<0.4", "0.4-0.9", "0.9-1.2", "M>1.2")
LAYERS = ("troposphere", "isothermal", "upper gradient")


def draw_cell(rng):
    return dict(h_sl_ft=float(rng.choice(ALTITUDES)), u_fps=float(rng.choice(SPEEDS)), v_fps=float(rng.uniform(-60, 60)),
                w_fps=float(rng.uniform(-80, 150)), p_rad_sec=float(rng.uniform(-1, 1)), q_rad_sec=float(rng.uniform(-0.3, 0.3)),
                r_rad_sec=float(rng.uniform(-0.2, 0.2)), psi_deg=float(rng.uniform(0, 360)))


def location_config(pkg, task, loc, cells, per_side=1):
    """The task's default config moved to `loc`: centre, aircraft positions (team 0 at the centre, team 1 offset; team mates 0.013 deg
    apart in longitude, away from the antimeridian), the altitude limit lowered so that low cells fly, and one cell per aircraft."""
    _, lat, lon, dlat, dlon = loc
    if task in ("multiplecombat", "scenario_nvn"):
        cfg = pkg.default_nvn_config(per_side, task=task)
    else:
        cfg = pkg.default_config(task)
    A = cfg.n_agents
    cfg.center_lon, cfg.center_lat = lon, lat
    cfg.altitude_limit = ALTITUDE_LIMIT
    for a in range(A):
        side, k = (0, a) if a < max(1, A // 2) else (1, a - A // 2)
        ic = cfg.init[a]
        ic.lat_geod_deg = lat + dlat * side + 0.004 * k
        ic.lon_deg = lon + dlon * side + (0.013 if dlon > 0 else -0.013) * k
        for key, v in cells[a].items():
            setattr(ic, key, v)
    return cfg


def set_oracle_cell(ocfg, a, cell):
    ic = ocfg.init[a]
    ic.h_sl_ft, ic.u_fps, ic.v_fps, ic.w_fps, ic.psi_deg = cell["h_sl_ft"], cell["u_fps"], cell["v_fps"], cell["w_fps"], cell["psi_deg"]
    ic.p, ic.q, ic.r = cell["p_rad_sec"], cell["q_rad_sec"], cell["r_rad_sec"]


def body_velocity(st):
    """u, v, w (ft/s, relative to the rotating Earth) of a state vector, and the rotation ECI -> body."""
    q0, q1, q2, q3 = st[6:10]
    T = np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 + q0 * q3), 2 * (q1 * q3 - q0 * q2)],
                  [2 * (q1 * q2 - q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 + q0 * q1)],
                  [2 * (q1 * q3 + q0 * q2), 2 * (q2 * q3 - q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])
    rv = np.array([st[3] + OMEGA * st[1], st[4] - OMEGA * st[0], st[5]])
    return T @ rv, T


class Reference:
    """The oracle's run at one location: `E` envs, each with its own cell per aircraft when `per_env` (else every env flies the
    handle's cells, so that both sides reset to the same initial conditions), random control indices held HOLD steps, weapon bits 0."""

    def __init__(self, pkg, oracle, loc_index, E=None, task="singlecombat", per_side=1, per_env=True, steps=STEPS, seed=SEED, chaff_seed=None):
        self.loc = LOCATIONS[loc_index]
        self.name, self.task, self.steps = self.loc[0], task, steps
        self.E = E = E if E is not None else (ENVS_RAGGED if loc_index == RAGGED else ENVS)
        rng = np.random.default_rng([seed, loc_index])
        A = 2 * per_side
        # the handle's own cells (the device's reset template; env 0 of the oracle): altitude and speed walk through the grids, so that the
        # ten locations' resets reach every altitude of ALTITUDES (both upper layers) and every speed (supersonic ones)
        handle_cells = [dict(draw_cell(rng), h_sl_ft=ALTITUDES[(loc_index + 5 * a) % len(ALTITUDES)], u_fps=SPEEDS[(loc_index + 3 * a) % len(SPEEDS)])
                        for a in range(A)]
        self.cfg = location_config(pkg, task, self.loc, handle_cells, per_side)
        self.A = A = self.cfg.n_agents
        base = oracle.config_from_ac(self.cfg)
        self.ocfgs = []
        for e in range(E):
            c = oracle.copy_config(base)
            if chaff_seed is not None:
                c.chaff_seed = chaff_seed + e
            if per_env and e > 0:       # env 0 flies the handle's own cells: the ones the device's reset template holds
                for a in range(A):
                    set_oracle_cell(c, a, draw_cell(rng))
            self.ocfgs.append(c)
        envs = [oracle.OracleEnv(c) for c in self.ocfgs]
        self.act_dim = envs[0].act_dim
        self.reset_obs = np.stack([env.reset() for env in envs])
        self.reset_state = np.array([[env.export_state(a) for a in range(A)] for env in envs])
        K = steps
        self.pre = np.zeros((K, E, A, oracle.STATE_LEN)); self.post = np.zeros_like(self.pre)
        self.pose = np.zeros((K, E, A, 12)); self.post_pose = np.zeros((K, E, A, 12))
        self.act = np.zeros((K, E, A, self.act_dim), dtype=np.float32)
        self.obs = np.zeros((K, E, A, envs[0].obs_dim)); self.rew = np.zeros((K, E, A, 1))
        self.done = np.zeros((K, E, A, 1), dtype=bool); self.ended = np.zeros((K, E), dtype=bool)
        self.beta = np.zeros((K, E, A))
        for k in range(K):
            if k % HOLD == 0:
                ctl = np.stack([rng.integers(0, n, size=(E, A)) for n in (41, 41, 41, 30)], axis=-1).astype(np.float32)
            self.act[k, ..., :4] = ctl
            for e, env in enumerate(envs):
                for a in range(A):
                    st = self.pre[k, e, a] = env.export_state(a)
                    self.pose[k, e, a] = env.pose(a)
                    uvw, _ = body_velocity(st)
                    self.beta[k, e, a] = np.arctan2(uvw[1], np.hypot(uvw[0], uvw[2]))
                for a in range(A):      # the reference starts from the exported vector too (import rebuilds the derived quantities: not bit for bit)
                    env.import_state(a, self.pre[k, e, a])
                o, r, d, info = env.step(self.act[k, e])
                self.ended[k, e] = bool(info[3])
                if info[3]:
                    o = env.reset()
                self.obs[k, e], self.rew[k, e, :, 0], self.done[k, e, :, 0] = o, r, d
                for a in range(A):
                    self.post[k, e, a] = env.export_state(a)
                    self.post_pose[k, e, a] = env.pose(a)
        assert np.isfinite(self.obs).all() and np.isfinite(self.rew).all(), self.name
        # the groups of a sample, from the state before the step
        h_ft = self.pose[..., 2] / 0.3048
        gp = h_ft * RE_FT / (RE_FT + h_ft)
        self.layer = (gp >= LAYER_GP_FT[0]).astype(int) + (gp >= LAYER_GP_FT[1]).astype(int)
        self.mach = self.pre[..., 46]
        self.band = (self.mach >= 0.4).astype(int) + (self.mach >= 0.9).astype(int) + (self.mach > 1.2).astype(int)
        self.alpha_deg = np.degrees(self.pre[..., 45])
        L = oracle.lib()
        out = [C.c_double() for _ in range(5)]
        P = np.zeros(h_ft.shape)
        for i, h in np.ndenumerate(h_ft):
            L.f16_atmosphere(float(h), *[C.byref(o) for o in out])
            P[i] = out[1].value
        self.qbar = 0.7 * P * self.mach ** 2
        self.qscale = np.maximum(1.0, self.qbar / Q_REF)
        self.aug = (self.pre[..., 66].astype(int) & 64) != 0

    def live(self):
        """[K, E, A] samples compared in full (the oracle did not end the episode on that step)."""
        return np.broadcast_to(~self.ended[..., None], self.layer.shape)


_REFERENCES = {}


def reference(pkg, oracle, loc_index, **kw):
    key = (loc_index,) + tuple(sorted(kw.items()))
    if key not in _REFERENCES:
        _REFERENCES[key] = Reference(pkg, oracle, loc_index, **kw)
    return _REFERENCES[key]


# ---- sides under test
TASK_FIELDS = ("bloods", "pre_posture", "pre_altitude", "pre_event", "pre_shoot", "status", "die_flag", "remaining", "pre_remaining",
               "shoot_action", "last_missile", "last_shoot_time", "lock_bits", "lock_pos", "cur_step")


def field_index(pkg):
    names = pkg.load_library().state_field_names()
    return {nm: k for k, nm in enumerate(names) if nm}


def fdm_fields(ix):
    return np.array(sorted(k for nm, k in ix.items() if not nm.startswith("x_") and nm not in TASK_FIELDS))


class DeviceSide:
    """HipVecEnv (HipShareVecEnv for the NvN families) at the reference's location. fdm_only: overwrite the flight-model fields and
    keep the task's own bookkeeping (test_gpu_parity.py::test_heading_task_numpy_stream_on_device does the same)."""

    def __init__(self, pkg, ref, ix, share=False, fdm_only=False, seed=0):
        self.env = (pkg.HipShareVecEnv if share else pkg.HipVecEnv)(ref.cfg, ref.E, seed=seed)
        self.share, self.fdm = share, (fdm_fields(ix) if fdm_only else None)
        self.n = len(ref.pre[0, 0, 0])

    def reset(self):
        out = self.env.reset()
        return out[0] if self.share else out

    def sync(self, k, e, a, st):
        if self.fdm is not None:
            v = self.env.get_state(e, a)
            v[self.fdm] = st[self.fdm]
            st = v
        self.env.set_state(e, a, st)

    def step(self, act):
        out = self.env.step(act)
        return (out[0], out[2], out[3]) if self.share else out[:3]

    def state(self, e, a):
        return self.env.get_state(e, a)

    def pose(self, e, a):
        return self.env.get_entity(e, a)

    def close(self):
        self.env.close()


class OracleUnderTest:
    """A second oracle with the reference's own per-env configs. `transform(st, k, e, a)` edits the state vector at import: the
    identity is the control, rounding is the fp32 twin, the planted faults are below."""

    def __init__(self, oracle, ref, transform=None):
        self.envs = [oracle.OracleEnv(c) for c in ref.ocfgs]
        self.transform = transform
        self.A = ref.A
        self.reset()

    def reset(self):
        return np.stack([env.reset() for env in self.envs])

    def sync(self, k, e, a, st):
        if self.transform is not None:
            st = self.transform(st.copy(), k, e, a)
        self.envs[e].import_state(a, st)

    def step(self, act):
        obs, rew, done = [], [], []
        for env, a in zip(self.envs, act):
            o, r, d, info = env.step(a)
            if info[3]:
                o = env.reset()
            obs.append(o); rew.append(r); done.append(d)
        return np.stack(obs), np.stack(rew)[..., None], np.stack(done)[..., None]

    def state(self, e, a):
        return self.envs[e].export_state(a)

    def pose(self, e, a):
        return self.envs[e].pose(a)

    def close(self):
        pass


def fp32_twin(st, k, e, a):
    """What a correct fp32 implementation starts a step from: entries vx..tank1 rounded, the position fp64 (open_loop_util.Fp32Twin)."""
    st[3:61] = st[3:61].astype(np.float32)
    return st


# ---- planted faults (the second oracle only)
def lost_hemisphere(st, k, e, a):
    st[2] = abs(st[2])              # the sign of rz lost: acts in southern cells only
    return st


def lost_longitude_sign(st, k, e, a):
    st[1] = -st[1]
    return st


def altitude_300ft_off(st, k, e, a):
    st[0:3] *= 1.0 + 300.0 / np.linalg.norm(st[0:3])
    return st


class StaleAirData:
    """The alpha and Mach words of the step before."""

    def __init__(self):
        self.prev = {}

    def __call__(self, st, k, e, a):
        old = self.prev.get((e, a))
        self.prev[(e, a)] = st[45:47].copy()
        if old is not None:
            st[45:47] = old
        return st


def v_w_exchanged(st, k, e, a):
    uvw, T = body_velocity(st)
    rv = T.T @ np.array([uvw[0], uvw[2], uvw[1]])
    st[3], st[4], st[5] = rv[0] - OMEGA * st[1], rv[1] + OMEGA * st[0], rv[2]
    return st


# ---- the stored record: the bounds of test_gpu_parity.py::test_singlecombat_kernel_forms_teacher_forced, as (field, relative, floor, absolute)
RECORD_BOUNDS = {}
for _f in ("tef", "ail", "elev", "sbdeg", "pi_r", "pi_p", "pi_y", "pin_r", "pin_p", "pin_y", "n1", "n2", "n2norm", "tank0", "tank1",
           "alpha", "mach", "qc", "vg", "vx", "vy", "vz", "wp", "wq", "wr"):
    RECORD_BOUNDS[_f] = (2e-5, 1.0, 1e-6)
RECORD_BOUNDS["ff"] = (5e-4, 1.0, 1e-6)         # fuel flow = thrust x a sqrt-of-temperature factor, both fp32 on the device
for _f in ("q0", "q1", "q2", "q3"):
    RECORD_BOUNDS[_f] = (0.0, 1.0, 2e-5)
for _f in ("rx", "ry", "rz"):
    RECORD_BOUNDS[_f] = (0.0, 1.0, 0.05)
for _f in ("da", "de", "dr", "thr"):
    RECORD_BOUNDS[_f] = (0.0, 1.0, 1e-6)
for _f, _tol, _floor in (("ap", 3e-6, 1.0), ("aq", 3e-6, 1.0), ("ar", 3e-6, 1.0), ("npx", 1.5e-5, 1.0), ("npy", 1.5e-5, 1.0), ("npz", 1.5e-5, 1.0),
                         ("hv1x", 1e-5, 32.0), ("hv1y", 1e-5, 32.0), ("hv1z", 1e-5, 32.0), ("hv2x", 1e-5, 32.0), ("hv2y", 1e-5, 32.0), ("hv2z", 1e-5, 32.0),
                         ("ha1x", 1.2e-5, 32.0), ("ha1y", 1.2e-5, 32.0), ("ha1z", 1.2e-5, 32.0), ("wdx", 3e-5, 1.0), ("wdy", 3e-5, 1.0), ("wdz", 3e-5, 1.0),
                         ("aix", 1.2e-5, 32.0), ("aiy", 1.2e-5, 32.0), ("aiz", 1.2e-5, 32.0), ("bax", 1.5e-5, 32.0), ("bay", 1.5e-5, 32.0), ("baz", 1.5e-5, 32.0)):
    RECORD_BOUNDS[_f] = (_tol, _floor, 0.0)
EXACT_FIELDS = ("eng", "ticks")
TASK_EXACT = ("bloods", "status", "die_flag", "cur_step")
TASK_BOUNDS = {"pre_posture": 5e-3, "pre_altitude": 1e-4, "pre_event": 1e-6}
RECORD_CLASSES = {"fcs": ("tef", "ail", "elev", "sbdeg", "pi_r", "pi_p", "pi_y", "pin_r", "pin_p", "pin_y", "da", "de", "dr", "thr"),
                  "engine": ("n1", "n2", "n2norm", "ff", "tank0", "tank1", "eng"),
                  "air data": ("alpha", "mach", "qc", "vg", "ap", "aq", "ar", "npx", "npy", "npz"),
                  "velocity": ("vx", "vy", "vz", "wp", "wq", "wr", "hv1x", "hv1y", "hv1z", "hv2x", "hv2y", "hv2z"),
                  "attitude": ("q0", "q1", "q2", "q3"), "position": ("rx", "ry", "rz"),
                  "acceleration": ("ha1x", "ha1y", "ha1z", "wdx", "wdy", "wdz", "aix", "aiy", "aiz", "bax", "bay", "baz"),
                  "task": TASK_EXACT + tuple(TASK_BOUNDS) + ("ticks",)}
QUANTITIES = ("obs", "rew", "pose") + tuple(RECORD_CLASSES)

# The reported pose (ac_get_entity: lon, lat deg | alt m | roll, pitch, yaw rad | v NED m/s | NEU m about the centre) one step after an
# identical state: the free-flight envelope at its first step (open_loop_util.envelope: 0.02 m, 2e-4 rad, 0.01 m/s), not its 8x.
# Longitude and latitude are held to the same 0.02 m on the ground: 0.02 / 111 195 deg of latitude, and that over cos(lat) of longitude.
POSE_POS_M, POSE_ATT_RAD, POSE_VEL_MS, M_PER_DEG = 0.02, 2e-4, 0.01, 111195.0


def pose_fraction(got, want):
    dlon = (got[0] - want[0] + 180.0) % 360.0 - 180.0
    datt = (got[3:6] - want[3:6] + np.pi) % (2 * np.pi) - np.pi
    return max(abs(dlon) * M_PER_DEG * np.cos(np.radians(want[1])) / POSE_POS_M, abs(got[1] - want[1]) * M_PER_DEG / POSE_POS_M,
               abs(got[2] - want[2]) / POSE_POS_M, float(np.abs(datt).max()) / POSE_ATT_RAD,
               float(np.linalg.norm(got[6:9] - want[6:9])) / POSE_VEL_MS, float(np.linalg.norm(got[9:12] - want[9:12])) / POSE_POS_M)


def record_fractions(got, want, ix, ended, qscale=1.0):
    """Fraction of its bound that every stored word uses (inf: a word that must be equal is not), by field name. qscale: Q_FIELDS."""
    out = {}
    for f, (rel, floor, ab) in RECORD_BOUNDS.items():
        w = want[ix[f]]
        out[f] = abs(got[ix[f]] - w) / ((rel * max(floor, abs(w)) + ab) * (qscale if f in Q_FIELDS else 1.0))
    for f in EXACT_FIELDS:
        out[f] = 0.0 if got[ix[f]] == want[ix[f]] else np.inf
    if not ended:
        for f in TASK_EXACT:
            out[f] = 0.0 if got[ix[f]] == want[ix[f]] else np.inf
        for f, tol in TASK_BOUNDS.items():
            out[f] = abs(got[ix[f]] - want[ix[f]]) / (tol * max(1.0, abs(want[ix[f]])))
    return out


class Report:
    """Fractions of the bounds used, [K, E, A] per quantity (nan: not compared), and the violations [(step, env, aircraft, what, ...)]."""

    def __init__(self, ref):
        self.ref = ref
        self.frac = {q: np.full(ref.layer.shape, np.nan) for q in QUANTITIES}
        self.worst_field = {}
        self.violations = []
        self.force_plain = ("", 0.0)        # the most that a Q_FIELDS word uses of its PLAIN bound (not asserted: what the qbar widening is for)

    def used(self, mask=None):
        out = {}
        for q, f in self.frac.items():
            v = f if mask is None else np.where(mask, f, np.nan)
            if np.isfinite(v).any() or np.isinf(v).any():
                out[q] = float(np.nanmax(v))
        return out

    def by_group(self):
        ref = self.ref
        g = {"location " + ref.name: None}
        for i, nm in enumerate(LAYERS):
            g[nm] = ref.layer == i
        for i, nm in enumerate(MACH_BANDS):
            g[nm] = ref.band == i
        return {nm: self.used(m) for nm, m in g.items() if m is None or m.any()}

    def first_violation_step(self, mask=None):
        ks = [v[0] for v in self.violations if mask is None or mask[v[0], v[1], v[2]]]
        return min(ks) if ks else None


def compare(ref, side, ix, record=True, strict=True, posture_scale=None, pose=True):
    """Plays `side` against the reference, teacher-forced before every step. strict: assert on the first violation (after the whole
    step has been measured); else they are collected in the report."""
    K, E, A = ref.layer.shape
    rep = Report(ref)
    scale = ref.cfg.posture_scale if posture_scale is None else posture_scale
    half = A // 2
    bound = RewardBound(scale, 9 + 6 * (half - 1), half, 1.0)
    bound(np.zeros((E, A, 1)), ref.reset_obs)               # the reset's geometry is the first step's "previous" one
    for k in range(K):
        for e in range(E):
            for a in range(A):
                side.sync(k, e, a, ref.pre[k, e, a])
        obs, rew, done = side.step(ref.act[k])
        robs, rrew, rdone, ended = ref.obs[k], ref.rew[k], ref.done[k], ref.ended[k]
        bad = done != rdone
        for e, a in np.argwhere(bad[..., 0]):
            rep.violations.append((k, int(e), int(a), "done", bool(done[e, a, 0]), bool(rdone[e, a, 0])))
        tol, free = obs_bounds(robs, 1.0)
        fo = np.where(free, 0.0, np.abs(obs - robs) / tol)
        fo = np.where(np.isfinite(obs), fo, np.inf).max(axis=-1)
        rt = bound(rrew, robs)
        if A > 2:
            rt = team_max(rt, A)
        fr = (np.abs(rew - rrew) / rt)[..., 0]
        fr = np.where(np.isfinite(rew[..., 0]), fr, np.inf)
        rep.frac["obs"][k] = np.where(ended[:, None], np.nan, fo)
        rep.frac["rew"][k] = fr
        for e, a in np.argwhere(np.nan_to_num(rep.frac["obs"][k], nan=0.0) > 1.0):
            j = int(np.argmax(np.where(free[e, a], 0.0, np.abs(obs[e, a] - robs[e, a]) / tol[e, a])))
            rep.violations.append((k, int(e), int(a), "obs", j, float(obs[e, a, j]), float(robs[e, a, j]), float(tol[e, a, j])))
        for e, a in np.argwhere(fr > 1.0):
            rep.violations.append((k, int(e), int(a), "rew", float(rew[e, a, 0]), float(rrew[e, a, 0]), float(rt[e, a, 0])))
        if record or pose:
            for e in range(E):
                if ended[e]:
                    continue                                # both sides hold their own reset state now
                for a in range(A):
                    if pose:
                        got_pose = side.pose(e, a)
                        v = rep.frac["pose"][k, e, a] = pose_fraction(got_pose, ref.post_pose[k, e, a]) if np.isfinite(got_pose).all() else np.inf
                        if not v <= 1.0:
                            rep.violations.append((k, e, a, "pose", got_pose.tolist(), ref.post_pose[k, e, a].tolist()))
                    if not record:
                        continue
                    fr_rec = record_fractions(side.state(e, a), ref.post[k, e, a], ix, False, ref.qscale[k, e, a])
                    f = max(Q_FIELDS, key=lambda nm: fr_rec[nm])
                    if fr_rec[f] * ref.qscale[k, e, a] > rep.force_plain[1]:
                        rep.force_plain = (f, float(fr_rec[f] * ref.qscale[k, e, a]))
                    for cls, fields in RECORD_CLASSES.items():
                        f = max(fields, key=lambda nm: fr_rec.get(nm, 0.0))
                        v = fr_rec.get(f, 0.0)
                        rep.frac[cls][k, e, a] = v
                        if v > rep.worst_field.get(cls, ("", -1.0))[1]:
                            rep.worst_field[cls] = (f, v)
                        if not v <= 1.0:
                            rep.violations.append((k, e, a, "record", f, float(side.state(e, a)[ix[f]]), float(ref.post[k, e, a][ix[f]])))
        assert not (strict and rep.violations), (ref.name, ref.task, rep.violations[:6], describe(ref, rep.violations[:6]))
    return rep


def describe(ref, violations):
    """The cell behind a violation: altitude ft, Mach, alpha deg, layer, before the step."""
    return [dict(step=v[0], env=v[1], ac=v[2], qbar=round(float(ref.qbar[v[0], v[1], v[2]])), h_ft=round(float(ref.pose[v[0], v[1], v[2], 2] / 0.3048)), mach=round(float(ref.mach[v[0], v[1], v[2]]), 3),
                 alpha_deg=round(float(ref.alpha_deg[v[0], v[1], v[2]]), 2), layer=LAYERS[ref.layer[v[0], v[1], v[2]]]) for v in violations]


def merge_used(tables):
    """Worst fraction per group and quantity over several reports' by_group() tables."""
    out = {}
    for t in tables:
        for g, used in t.items():
            o = out.setdefault(g, {})
            for q, v in used.items():
                o[q] = max(o.get(q, 0.0), v)
    return out


def print_used(title, table):
    print(title + ": worst fraction of each bound used, per cell group")
    for g, used in table.items():
        print(f"  {g:28s} " + ", ".join(f"{q} {v:.3f}" for q, v in used.items()))


def coverage(refs):
    """Sample counts of the conditions the envelope must reach, from the oracle's own states (samples compared in full only)."""
    c = {}
    def add(name, mask, live):
        c[name] = c.get(name, 0) + int((mask & live).sum())
    for ref in refs:
        live = ref.live()
        for i, nm in enumerate(LAYERS):
            add(nm, ref.layer == i, live)
        add("Mach < 0.4", ref.mach < 0.4, live); add("Mach > 1.2", ref.mach > 1.2, live)
        add("alpha > 25 deg", ref.alpha_deg > 25.0, live); add("alpha < -10 deg", ref.alpha_deg < -10.0, live)
        add("|beta| > 8 deg", np.abs(np.degrees(ref.beta)) > 8.0, live)
        add("northern", ref.pre[..., 2] > 0, live); add("southern", ref.pre[..., 2] < 0, live)
        lon = ref.pose[..., 0]
        for lo in (-180, -90, 0, 90):
            add(f"longitude {lo}..{lo + 90}", (lon >= lo) & (lon < lo + 90), live)
        add("augmentation on", ref.aug, live); add("augmentation off", ~ref.aug, live)
    return c


def skipped_fraction(refs):
    return sum(int(r.ended.sum()) for r in refs) / sum(r.ended.size for r in refs)
