"""Free-flight comparison harness shared by tests/test_gpu_open_loop.py, tests/test_open_loop_twin.py and tools/diag/open_loop.py: two
implementations of the step from the same initial conditions under the same actions, with NO state injection, and the per-step
differences north_star names (position, attitude, velocity, reward), the munitions in flight and every weapon decision.

The two sides stand behind one small interface (DeviceSide wraps HipVecEnv, OracleSide wraps OracleVecEnv; the CPU tests pair the
oracle with a second oracle):

    step(act) -> obs, rew, done, reset_flags        state(e, a)   in the ac_state_field_name layout        pose(e, a)
    munitions(e, agents=None) -> records            counters(e, a) -> weapon bookkeeping by name           in_flight() -> int

The FIRST side is the one under test, the SECOND the reference: munitions are matched from the reference's list.

Every kernel form a BASELINE config launches flies through here: the task picks the kernel family, the environment variables
AIRCOMBAT_SPLIT / AIRCOMBAT_QUAD (set by the caller BEFORE the pair is built: ac_create reads them per handle) pin the form.
`substeps` = agent_interaction_steps: 6 is every shipped YAML's; 1 makes an env step ONE FDM tick, so that the discrete decisions of
the flight control system are compared after every tick instead of after every sixth."""
import ctypes as C

import numpy as np

KTSTOFPS = 1.68781

# (psi A, psi B, h_sl ft A, h_sl ft B, u fps A, u fps B): eight starts around the shipped one (WVR_selfplay.yaml:15-40: 20 000 ft, 800 fps, head-on)
STARTS = ((0.0, 180.0, 20000.0, 20000.0, 800.0, 800.0), (35.0, 200.0, 24000.0, 18000.0, 700.0, 900.0), (90.0, 270.0, 16000.0, 26000.0, 950.0, 650.0),
          (310.0, 140.0, 28000.0, 22000.0, 600.0, 1000.0), (180.0, 0.0, 19000.0, 21000.0, 850.0, 750.0), (225.0, 45.0, 30000.0, 15000.0, 1000.0, 600.0),
          (10.0, 170.0, 22000.0, 22500.0, 780.0, 820.0), (270.0, 100.0, 17500.0, 27000.0, 900.0, 700.0))

# task -> (config factory arguments, straight-and-level action row): the reference's straight-fly control indices [20, 19, 20, 0]
# (model/baseline.py:168), every weapon / shoot bit 0 (nothing is ever launched: what is compared is the FLIGHT of these kernel forms)
STRAIGHT = {"singlecombat": [20, 19, 20, 0], "singlecombat_shoot": [20, 19, 20, 0, 0], "multiplecombat": [20, 19, 20, 0],
            "scenario_nvn": [20, 19, 20, 0, 0, 0, 0, 0], "scenario1": [20, 19, 20, 0, 0, 0, 0, 0]}

TASK_DODGE, TASK_SHOOT, TASK_SCENARIO1, TASK_SCENARIO_NVN = 2, 3, 5, 6
# Munition records. Both sides use ONE set of status codes (combat_env.h OR_MSL_*, aircombat.hip MSL_*): -1 never launched, 0 in flight,
# 1 hit, 2 miss. Both keep the velocity in the frame of the aircraft pose's entries 6..8 (vN, vE, vDOWN: a launch copies the parent's
# velocity record as it stands, and the guidance then reads the third entry as a climb rate, simulatior.py:497-514 and :556-576, on both
# sides alike), the position in NEU like pose entries 9..11. The pair CHECKS this at the step of every launch, on each side against that
# side's own parent pose: task.step launches after the step's last tick, so at that step the record has t = 0, the parent's position and
# the parent's velocity -- a record in another frame, or a launch from the pose of the tick before (4 m behind at 250 m/s), fails there.
MSL_INACTIVE, MSL_LAUNCHED, MSL_HIT, MSL_MISS = -1, 0, 1, 2
LAUNCH_POS_TOL = {False: 1e-6, True: 0.02}    # m: fp64 record against fp64 pose; where the slot OR the pose (ac_get_entity's NEU) is fp32, half an ulp of a 150 km coordinate is 0.008 m
LAUNCH_VEL_TOL = 1e-3                         # m/s: the pose reports the velocity through ft/s and a clip, the slot holds it in fp32
WEAPON_NAMES = ("remaining", "last_shoot_time", "shoot_action")
LOCK_NAMES = ("lock_bits", "lock_pos")
SCENARIO_NAMES = ("rem_gun", "rem_9m", "rem_120b", "rem_chaff", "n_ch")


def wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


def envelope(k):
    """The frozen free-flight envelope of straight flight (tests/test_gpu_open_loop.py's docstring), k = env steps since the episode began."""
    x = np.asarray(k, dtype=np.float64) / 600.0
    return {"pos_m": 0.02 + 15.0 * x ** 3, "att_rad": 2e-4 + 0.015 * x ** 2, "vel_ms": 0.01 + 0.8 * x ** 2, "obs": 2e-4 + 0.015 * x ** 2,
            "rew": 5e-3 + 0.02 * x ** 2}


def make_config(pkg, task, per_side, start, substeps):
    if task in ("multiplecombat", "scenario_nvn"):
        cfg = pkg.default_nvn_config(per_side, task=task)
    else:
        cfg = pkg.default_config(task)
    A = cfg.n_agents
    for a in range(A):
        side, k = (0, a) if a < A // 2 else (1, a - A // 2)
        cfg.init[a].psi_deg, cfg.init[a].h_sl_ft, cfg.init[a].u_fps = start[side] + 3.0 * k, start[2 + side] + 400.0 * k, start[4 + side] + 15.0 * k
        if A > 2:   # the shipped NvN YAMLs put both teams on one meridian, exactly head-on: stagger them like the parity suite does
            cfg.init[a].lon_deg += 0.013 * (a % 3) + (0.03 if side else 0.0)
    cfg.agent_interaction_steps = substeps
    cfg.max_steps = 9000 * 6 // substeps
    return cfg


def weapon_names(task):
    names = WEAPON_NAMES
    if task == TASK_DODGE:
        names = names + LOCK_NAMES
    if task in (TASK_SCENARIO1, TASK_SCENARIO_NVN):
        names = names + SCENARIO_NAMES
    return names


class OracleSide:
    """OracleVecEnv behind the pair's interface. Subclasses that stand for another implementation (the fp32 twin, planted faults)
    override step(); `self.k` counts the steps taken."""
    msl_fp32 = pose_fp32 = False

    def __init__(self, oracle, ocfg, per, ix, chaff_seed=77):
        self.vec = oracle.OracleVecEnv(ocfg, per, chaff_seed=chaff_seed)
        self.cfg, self.ix, self.per, self.k = ocfg, ix, per, 0
        self.task, self.A = int(ocfg.task), ocfg.n_aircraft

    def reset(self):
        return self.vec.reset()

    def step(self, act):
        self.k += 1
        obs, rew, done, info = self.vec.step(act)
        return obs, rew, done, info[:, 3] != 0

    def state(self, e, a):
        return self.vec.envs[e].export_state(a)

    def pose(self, e, a):
        return self.vec.envs[e].pose(a)

    def munitions(self, e, agents=None):
        env = self.vec.envs[e]
        out = []
        for k, (m, x) in enumerate(zip(env.missiles(), env.missiles_ext())):
            if agents is not None and int(m[11]) not in agents:
                continue
            out.append({"agent": int(m[11]), "slot": k, "status": int(m[0]), "pos": m[1:4], "vel": m[4:7], "theta": m[7], "psi": m[8], "t": m[9],
                        "mass": m[10], "target": int(m[12]), "model": int(x[0]), "recede": int(x[3])})
        return out

    def in_flight(self):
        return sum(int(m[0]) == MSL_LAUNCHED for env in self.vec.envs for m in env.missiles())

    def chaff(self, e):
        """Positions of the decoy clouds still burning."""
        return [c[:3] for c in self.vec.envs[e].chaff() if int(c[4]) == 0]

    def counters(self, e, a, state=None):
        st = self.state(e, a) if state is None else state
        rec = {nm: int(round(st[self.ix[nm]])) for nm in weapon_names(self.task) if nm in self.ix}
        if self.task in (TASK_SCENARIO1, TASK_SCENARIO_NVN):
            env = self.vec.envs[e]
            cnt = env.counters(a)
            rec.update(rem_gun=int(cnt[0]), rem_9m=int(cnt[1]), rem_120b=int(cnt[2]), rem_chaff=int(cnt[3]))
            # release EVENTS of this aircraft (one event releases a cloud per incoming munition: the device stores a multiplicity)
            rec["n_ch"] = len({round(float(c[3]), 6) for c in env.chaff() if int(c[5]) == a})
        return rec

    def close(self):
        pass


class Fp32Twin(OracleSide):
    """The oracle with its flight state rounded to float32 after every env step (entries vx..tank1 of the state vector; the position stays
    fp64), and its munitions too where the device keeps its slots in fp32: what a correct fp32 implementation may differ by."""

    def __init__(self, oracle, ocfg, per, ix):
        super().__init__(oracle, ocfg, per, ix)
        self.msl_fp32 = self.task in (TASK_DODGE, TASK_SHOOT) and self.A == 2      # as DeviceSide: fp32 munition slots in the 1v1 missile tasks

    def step(self, act):
        out = super().step(act)
        for env in self.vec.envs:
            for a in range(self.A):
                st = env.export_state(a)
                st[3:61] = st[3:61].astype(np.float32)
                env.import_state(a, st)
            if self.msl_fp32:
                env.round_missiles_f32()
        return out


class DeviceSide:
    """HipVecEnv behind the pair's interface."""
    pose_fp32 = True        # ac_get_entity reports the NEU position rounded to fp32 (Props.n / e / u)

    def __init__(self, pkg, cfg, per, ix, seed=77):
        self.env = pkg.HipVecEnv(cfg, per, seed=seed)
        self.ix, self.per, self.k = ix, per, 0
        self.task, self.A = int(cfg.task), cfg.n_agents
        self.slots = self.env.snapshot_header()["msl_slots"]
        self.msl_fp32 = self.task in (TASK_DODGE, TASK_SHOOT) and self.A == 2   # the 1v1 missile tasks keep their slots in fp32 (aircombat.hip MslT<float>)
        self.lib = self.env.lib
        self._sig, self._slots = {}, {}     # per (env, aircraft): its launch counters, and the slots found in use when they last changed

    def reset(self):
        return self.env.reset()

    def step(self, act):
        self.k += 1
        obs, rew, done, info = self.env.step(act)
        return obs, rew, done, None

    def state(self, e, a):
        return self.env.get_state(e, a)

    def pose(self, e, a):
        return self.env.get_entity(e, a)

    def munitions(self, e, agents=None):
        out = []
        for a in (range(self.A) if agents is None else sorted(agents)):
            # a slot never launched into stays so until a launch, and a launch spends a round: all slots are read when the aircraft's launch
            # counters (counters()) have changed, else those found in use then. (A launch that spends nothing shows in in_flight().)
            sig, known = self._sig.get((e, a)), self._slots.get((e, a))
            scan = range(self.slots) if sig is None or known is None or known[0] != sig else known[1]
            used = []
            for k in scan:
                m = self.env.get_missile(e, a, k)
                if int(m[0]) == MSL_INACTIVE:
                    continue
                used.append(k)
                # ac_get_missile's model code names the weapon (0 AIM-9L, 1 AIM-120B, 2 AIM-9M); the oracle's is the PARAMETER set, which the two
                # scenario weapons share (simulatior.py:659-709): which of the two was launched is held by rem_9m / rem_120b
                out.append({"agent": a, "slot": k, "status": int(m[0]), "pos": m[1:4], "vel": m[4:7], "theta": m[7], "psi": m[8], "t": m[9], "mass": m[10],
                            "target": self.env.get_missile_target(e, a, k), "model": min(int(m[11]), 1), "recede": None})
            self._slots[(e, a)] = (sig, used)
        return out

    def in_flight(self):
        return self.env.munitions_in_flight()

    def chaff(self, e):
        out, ix = [], self.ix
        for a in range(self.A):
            st = self.state(e, a)
            for q in range(int(st[ix["x_n_ch"]])):
                if int(st[ix[f"x_ch_status{q}"]]) == 0:
                    out.append(np.array([st[ix[f"x_c{q}x"]], st[ix[f"x_c{q}y"]], st[ix[f"x_c{q}z"]]]))
        return out

    def counters(self, e, a, state=None):
        st = self.state(e, a) if state is None else state
        rec = {}
        for nm in weapon_names(self.task):
            rec[nm] = int(round(st[self.ix[nm if nm in WEAPON_NAMES + LOCK_NAMES else "x_" + nm]]))
        self._sig[(e, a)] = tuple(rec.get(nm) for nm in ("remaining", "rem_9m", "rem_120b"))
        return rec

    def close(self):
        self.env.close()


class OpenLoopPair:
    """len(STARTS) handles x (E / len(STARTS)) envs of `task`, each next to its twin. `sides(cfg, ocfg, per, ix)` -> (side under test,
    reference side); the default pairs the device with the oracle."""

    def __init__(self, pkg, oracle, E, spread=True, task="singlecombat", per_side=1, substeps=6, n_starts=None, sides=None):
        self.L = oracle.lib()
        self.L.f16_vcas_from_qc.restype = C.c_double
        self.L.f16_vcas_from_qc.argtypes = [C.c_double]
        starts = STARTS if spread else STARTS[:1]
        if n_starts is not None:
            starts = starts[:n_starts]
        per = max(1, E // len(starts))
        self.parts = []
        self.task, self.substeps = task, substeps
        names = pkg.load_library().state_field_names()
        self.ix = {nm: k for k, nm in enumerate(names) if nm}
        if sides is None:
            def sides(cfg, ocfg, per, ix):
                return DeviceSide(pkg, cfg, per, ix), OracleSide(oracle, ocfg, per, ix)
        for s in starts:
            cfg = make_config(pkg, task, per_side, s, substeps)
            ocfg = oracle.config_from_ac(cfg)
            env, ref = sides(cfg, ocfg, per, self.ix)
            obs, robs = env.reset(), ref.reset()
            assert obs.shape == robs.shape, (obs.shape, robs.shape)
            assert np.abs(obs - robs).max() < 2e-3, np.abs(obs - robs).max()
            self.parts.append((env, ref, per))
        self.A = self.parts[0][0].A
        self.cfg = ocfg
        self.task_id = int(ocfg.task)
        self.tick = 1.0 / ocfg.sim_freq
        self.altitude_limit = float(cfg.altitude_limit)
        self.E = per * len(starts)
        self.k = 0
        self.age = np.zeros(self.E, dtype=np.int64)                 # env steps since the episode began (the envelope's argument)
        self.horizon = np.full(self.E, 1 << 30, dtype=np.int64)     # first step at which a discrete decision differed (never: huge)
        self.reason = [""] * self.E
        self.done_mismatch = np.zeros(self.E, dtype=bool)
        self.unexplained = []                               # done flags and weapon decisions that differ and that neither an earlier decision nor a threshold explains
        self.last_reset = np.zeros(self.E, dtype=bool)      # envs whose episode ended (and restarted) in the last step()
        # munitions: per env, reference index -> what is remembered of a munition while it flies
        self.track = [dict() for _ in range(self.E)]
        self.prev_fly = [set() for _ in range(self.E)]      # aircraft whose reference twin had a munition in flight after the step before
        self.handle_ok = [True] * len(self.parts)           # the per-handle in-flight count is compared while every env of the handle is inside its horizon
        self.flown = np.zeros(self.E, dtype=bool)           # a munition was in flight at some step, inside the env's horizon
        self.msl_flown = self.msl_ended = 0                 # munitions launched / that reached a terminal status inside an env's horizon
        self.worst_msl = {"closing": {"pos_m": 0.0, "vel_ms": 0.0}, "after the pass": {"pos_m": 0.0, "vel_ms": 0.0}}   # fractions of the 8x envelope

    def straight_action(self):
        return np.tile(np.array(STRAIGHT[self.task], dtype=np.float32), (self.E, self.A, 1))

    def discrete(self, st):
        """The decisions the next tick's flight control system takes from this state (f16.xml:325-335,814-832: gear stays down, so the
        leading-edge flap is 0.262 rad above alpha 0.0873, else -0.0349 above Mach 0.9; trailing-edge flap 0.349 rad below 250 kt,
        -0.0349 above Mach 0.9), the turbine's phase word and the aircraft status. The weapon decisions (counters() of the two sides,
        the munitions' status, target, model and number in flight) are compared next to these after every step: step()."""
        ix = self.ix
        alpha, mach, qc = st[ix["alpha"]], st[ix["mach"]], st[ix["qc"]]
        vc_kts = self.L.f16_vcas_from_qc(float(qc)) / KTSTOFPS
        lef = 2 if alpha > 0.0873 else (1 if mach > 0.9 else 0)
        tef = 2 if vc_kts < 250.0 else (1 if mach > 0.9 else 0)
        return ("lef", lef), ("tef", tef), ("engine", int(st[ix["eng"]])), ("status", int(st[ix["status"]]))

    def near_a_threshold(self, st, pose, k):
        """A done flag that differs with every EARLIER decision equal is legitimate only where a continuous quantity sits on its
        threshold: the side that did NOT terminate must be within a hair of LowAltitude's limit (the other side's altitude is
        within the position envelope of it and just across) or of Overload / ExtremeState's load factor 10. Anything else (a
        timeout, SafeReturn, an altitude a hundred metres off the limit) is a termination bug. `st`, `pose`: the state and pose of
        the aircraft on the side whose done flag is False.

        A WEAPON decision that differs is held to the same rule by weapon_threshold(); the thresholds it knows, all of oracle/combat_env.c,
        each taken on the side that did not act and within the 8x free-flight envelope at the env's episode age (a range: 2 x 8 x the
        position envelope, two objects; an angle: that range over the distance plus 8 x the velocity envelope over the speed):
          kill radius Rc, `distance < m->Rc` (:239; Rc = 300 m :201, 5 m :204);
          a munition's own termination limits (:241): flight time `m->t > m->t_max`, speed `< m->v_min` (150 m/s, :198), the recede count
            reaching `recede_max` (5 s of ticks, :206: the count differs by the tick at which the range turns, so it is taken as "within two
            ticks of the limit on the reference"), a decoy cloud at 300 m (:892);
          lock angle `ang < max_attack_angle` (:842) and `dist <= max_attack_distance` (:847) of the rule-based launch;
          the scenario tasks' weapon zones (:756-758): range 3 / 37 / 7 km, off-boresight angle 5 / 90 / 90 deg, and the choice of the FARTHEST
            enemy as the target (:743: two enemies at the same range);
          the decoy release range of 1000 m to an incoming munition (:791)."""
        ix = self.ix
        margin = 1.0 + 8.0 * (0.02 + 15.0 * (k * self.substeps / 3600.0) ** 3)
        if 0.0 <= pose[2] - self.altitude_limit <= margin:
            return "altitude"
        for nm, off in (("npx", 0.0), ("npy", 0.0), ("npz", 1.0)):
            if 0.0 <= 10.0 - abs(st[ix[nm]] + off) <= 0.1:
                return "load factor"
        return None

    # ---- weapon decisions
    def margins(self, g):
        env = envelope(self.age[g] * self.substeps / 6.0)
        return 2.0 * 8.0 * float(env["pos_m"]), 8.0 * float(env["vel_ms"])

    def geometry(self, poses, s, a, j, g):
        """Range and off-boresight angle (deg) from aircraft a to aircraft j on side s, and the angle that the envelope subtends there."""
        rm, vm = self.margins(g)
        d = poses[j][s][9:12] - poses[a][s][9:12]
        v = poses[a][s][6:9]
        dist, sp = np.linalg.norm(d), np.linalg.norm(v)
        ang = np.degrees(np.arccos(np.clip(d @ v / (dist * sp + 1e-8), -1, 1)))
        return dist, ang, np.degrees(rm / max(dist, 1.0) + vm / max(sp, 1.0))

    def enemies(self, a):
        h = self.A // 2
        return list(range(h, self.A)) if a < h else list(range(0, h))

    def launch_threshold(self, poses, s, a, g):
        """A launch (or a gun burst) that one side made and side s did not: a zone limit on side s's geometry."""
        rm, _ = self.margins(g)
        foes = self.enemies(a)
        if self.task_id in (TASK_SCENARIO1, TASK_SCENARIO_NVN):
            rng = sorted(self.geometry(poses, s, a, j, g)[0] for j in foes)
            if len(rng) > 1 and rng[-1] - rng[-2] <= rm:
                return "farthest enemy"
            tg = max(foes, key=lambda j: self.geometry(poses, s, a, j, g)[0])
            dist, ang, am = self.geometry(poses, s, a, tg, g)
            if min(abs(dist - 3000.0), abs(dist - 37000.0), abs(dist - 7000.0)) <= rm:
                return "weapon zone range"
            if min(abs(ang - 5.0), abs(ang - 90.0)) <= am:
                return "weapon zone angle"
        elif self.task_id == TASK_DODGE:
            dist, ang, am = self.geometry(poses, s, a, foes[0], g)
            if abs(dist - self.cfg.max_attack_distance) <= rm:
                return "max_attack_distance"
            if abs(ang - self.cfg.max_attack_angle) <= am:
                return "max_attack_angle"
        return None   # singlecombat_shoot launches on the action bit alone (:857): no threshold can make the two sides differ

    def status_threshold(self, g, tr, s, acted, rec, ref_rec, poses, sides, e):
        """A munition that ended on one side (status `acted`) and still flies on side s, whose record of it is `rec`."""
        rm, vm = self.margins(g)
        fuse = 300.0 if rec["model"] == 0 else 5.0
        t_max = 60.0 if rec["model"] == 0 else 27.22
        if acted == MSL_HIT:
            # closest approach inside the step on side s: the chord between its records before and after the step, munition relative to target;
            # a chord misses the arc by at most a T^2 / 8 (50 g + 10 g over 0.1 s of substeps: 0.75 m)
            r1 = rec["pos"] - poses[rec["target"]][s][9:12]
            r0 = tr["rel"][s]
            if r0 is None:
                return None
            w = r1 - r0
            u = np.clip(-(r0 @ w) / max(w @ w, 1e-12), 0.0, 1.0)
            dmin = np.linalg.norm(r0 + u * w)
            return "kill radius" if dmin - fuse <= rm + 0.75 * (self.substeps / 6.0) ** 2 else None
        if acted == MSL_MISS:
            if abs(rec["t"] - t_max) <= self.tick + 1e-3:
                return "t_max"
            if abs(np.linalg.norm(rec["vel"]) - 150.0) <= vm:
                return "v_min"
            if ref_rec is not None and ref_rec["recede"] is not None and ref_rec["recede"] >= int(5.0 / self.tick) - 2:
                return "recede count"
            for c in sides[s].chaff(e):
                if abs(np.linalg.norm(c - rec["pos"]) - 300.0) <= rm:
                    return "decoy range"
        return None

    def check_launch_pose(self, g, name, rec, pose, fp32):
        dp, dv = np.linalg.norm(rec["pos"] - pose[9:12]), np.linalg.norm(rec["vel"] - pose[6:9])
        if dp > LAUNCH_POS_TOL[fp32] or dv > LAUNCH_VEL_TOL:
            self.unexplained.append((g, self.k, "launch pose: a munition with t = 0 is not at its parent's pose", name, rec["agent"], float(dp), float(dv)))

    def weapons(self, g, e, sides, states, poses, msl):
        """Weapon bookkeeping and munitions of env g after this step: returns the differing decisions [(name, aircraft, tested, reference)]
        with their explanation (None: unexplained)."""
        dev, ref = sides
        diffs = []
        for a in range(self.A):
            cd, cr = dev.counters(e, a, states[a][0]), ref.counters(e, a, states[a][1])
            for nm, y in cr.items():
                if cd[nm] != y:
                    s = 0 if cd[nm] > y else 1    # a count that is higher has not been spent: that side did not act
                    why = None
                    if nm in ("remaining", "last_shoot_time", "rem_gun", "rem_9m", "rem_120b"):
                        why = self.launch_threshold(poses, s, a, g)
                    elif nm == "lock_bits" and self.task_id == TASK_DODGE:
                        dist, ang, am = self.geometry(poses, 0, a, self.enemies(a)[0], g)
                        why = "max_attack_angle" if abs(ang - self.cfg.max_attack_angle) <= am else None
                    elif nm in ("rem_chaff", "n_ch"):
                        rm, _ = self.margins(g)
                        for m in sides[s].munitions(e):
                            if m["target"] == a and abs(np.linalg.norm(m["pos"] - poses[a][s][9:12]) - 1000.0) <= rm:
                                why = "decoy release range"
                    diffs.append(((nm, a, cd[nm], y), why))
        rmsl = ref.munitions(e)
        fly = {m["agent"] for m in rmsl if m["status"] == MSL_LAUNCHED}
        agents = fly | self.prev_fly[g]
        self.prev_fly[g] = fly
        if fly:
            self.flown[g] = True
        dmsl = dev.munitions(e, agents) if agents else []
        by_slot = {(d["agent"], d["slot"]): d for d in dmsl}
        tol_t = 1e-3 if dev.msl_fp32 else self.tick
        track = self.track[g]
        b = self.margins(g)
        b = (b[0] / 2.0, b[1])                          # a munition against its twin: ONE object's position envelope
        secondary = []
        for j, m in enumerate(rmsl):
            tr = track.get(j)
            if m["status"] == MSL_LAUNCHED:
                cands = [d for d in dmsl if d["agent"] == m["agent"] and d["status"] == MSL_LAUNCHED and abs(d["t"] - m["t"]) <= tol_t]
                if tr is None:
                    tr = track[j] = {"slot": None, "receded": False, "range": None, "rel": [None, None]}
                    self.msl_flown += 1
                if len(cands) != 1:
                    d = by_slot.get(tr["slot"])
                    if d is not None and d["status"] in (MSL_HIT, MSL_MISS):      # it ended on the side under test and flies on here
                        diffs.append((("msl_status", m["agent"], d["status"], m["status"]),
                                      self.status_threshold(g, tr, 1, d["status"], m, m, poses, sides, e)))
                    else:
                        secondary.append(("msl_match", m["agent"], len(cands), 1))
                    continue
                d = cands[0]
                tr["slot"] = (d["agent"], d["slot"])
                if m["t"] == 0.0:                       # the step of the launch: frame and launch pose, each side against its own parent
                    self.check_launch_pose(g, "reference", m, poses[m["agent"]][1], ref.msl_fp32 or ref.pose_fp32)
                    self.check_launch_pose(g, "tested", d, poses[d["agent"]][0], dev.msl_fp32 or dev.pose_fp32)
                if d["target"] != m["target"]:
                    rng = sorted(self.geometry(poses, 0, m["agent"], j2, g)[0] for j2 in self.enemies(m["agent"]))
                    tie = len(rng) > 1 and rng[-1] - rng[-2] <= 2.0 * b[0] and m["t"] == 0.0
                    diffs.append((("msl_target", m["agent"], d["target"], m["target"]), "farthest enemy" if tie else None))
                    continue
                if d["model"] != m["model"]:
                    diffs.append((("msl_model", m["agent"], d["model"], m["model"]), None))
                rel = [d["pos"] - poses[d["target"]][0][9:12], m["pos"] - poses[m["target"]][1][9:12]]
                rng = float(np.linalg.norm(rel[1]))
                if tr["range"] is not None and rng > tr["range"]:
                    tr["receded"] = True                # from its first receding step on only the munition's discrete facts are compared
                tr["range"], tr["rel"] = rng, rel
                dp, dv = float(np.linalg.norm(d["pos"] - m["pos"])), float(np.linalg.norm(d["vel"] - m["vel"]))
                phase = "after the pass" if tr["receded"] else "closing"
                w = self.worst_msl[phase]
                w["pos_m"], w["vel_ms"] = max(w["pos_m"], dp / b[0]), max(w["vel_ms"], dv / b[1])
                if not tr["receded"]:
                    msl["msl_pos_m"][g], msl["msl_vel_ms"][g] = max(msl["msl_pos_m"][g], dp), max(msl["msl_vel_ms"][g], dv)
            elif tr is not None and not tr.get("ended"):    # in flight after the step before, ended in this one
                tr["ended"] = True
                d = by_slot.get(tr["slot"])
                if d is not None and d["status"] == MSL_LAUNCHED and d["t"] == 0.0:
                    self.msl_ended += 1                 # the slot was launched into again in this very step: the ended status is gone
                elif d is not None and d["status"] == m["status"]:
                    self.msl_ended += 1
                elif d is not None and d["status"] == MSL_LAUNCHED:
                    diffs.append((("msl_status", m["agent"], d["status"], m["status"]), self.status_threshold(g, tr, 0, m["status"], d, m, poses, sides, e)))
                else:
                    diffs.append((("msl_status", m["agent"], None if d is None else d["status"], m["status"]), None))
        for a in agents:
            nd = sum(d["agent"] == a and d["status"] == MSL_LAUNCHED for d in dmsl)
            nr = sum(m["agent"] == a and m["status"] == MSL_LAUNCHED for m in rmsl)
            if nd != nr:
                secondary.append(("msl_in_flight", a, nd, nr))
        # a munition that cannot be matched, or a differing number in flight, FOLLOWS from a launch or an ending that differs: explained exactly
        # when such a primary difference stands beside it and is itself explained
        follows = "follows" if diffs and all(w is not None for _, w in diffs) else None
        diffs += [(s, follows) for s in secondary]
        return diffs

    def others_of(self, a):
        """The aircraft behind the relative-geometry blocks of agent a's observation, in block order: partners, then enemies."""
        A, h = self.A, self.A // 2
        team = range(0, h) if a < h else range(h, A)
        foes = range(h, A) if a < h else range(0, h)
        return [j for j in team if j != a] + list(foes)

    def side_flags_free(self, poses):
        """[A, A-1] bool: the side flag of a block is the sign of the HORIZONTAL cross product v_ego x (p_other - p_ego)
        (utils.py:58-83): undefined where the other aircraft is dead ahead or astern in plan view -- here to within the angle the
        free-flight position envelope subtends at that range (oracle poses: lon lat alt | rpy | v NED | NEU)."""
        pos_env = 0.02 + 15.0 * (self.k * self.substeps / 3600.0) ** 3
        free = np.zeros((self.A, self.A - 1), dtype=bool)
        for a in range(self.A):
            pa, va = poses[a][1][9:11], poses[a][1][6:8]
            for b, j in enumerate(self.others_of(a)):
                d = poses[j][1][9:11] - pa
                nd, nv = np.linalg.norm(d), np.linalg.norm(va)
                s2 = abs(va[0] * d[1] - va[1] * d[0]) / max(nd * nv, 1e-9)
                free[a, b] = s2 < 2e-3 + 4.0 * pos_env / max(nd, 100.0)
        return free

    def obs_difference(self, obs, robs, free):
        """max |d observation| per aircraft, with the two conditioning rules of the relative-geometry blocks [du, dh, AO, TA, R / 1e4,
        side] (tests/parity_util.py): the side flag where it is undefined (side_flags_free), and acos turning an fp32 rounding of its
        argument into 3e-7 / sin(angle)."""
        d = np.abs(obs - robs)
        for b in range(self.A - 1):
            o = 9 + 6 * b
            if o + 5 >= obs.shape[-1]:
                break
            d[..., o + 5] = np.where(free[..., b], 0.0, d[..., o + 5])
            for col in (o + 2, o + 3):
                d[..., col] = np.maximum(0.0, d[..., col] - 3e-7 / np.maximum(np.sin(robs[..., col]), 1e-4))
        return d.max(axis=-1)

    def step(self, act):
        """One env step of every handle and twin. Returns per-aircraft differences [E, A], per-env munition differences [E] (the largest
        over the munitions still closing on their targets) and `live` [E]: envs still inside their horizon (no discrete decision has
        differed yet, dones agree)."""
        self.k += 1
        self.age += 1
        A = self.A
        out = {k: [] for k in ("pos_m", "att_rad", "vel_ms", "obs", "rew")}
        msl = {"msl_pos_m": np.zeros(self.E), "msl_vel_ms": np.zeros(self.E)}
        e0 = 0
        for h, (env, ref, per) in enumerate(self.parts):
            a = act[e0:e0 + per]
            obs, rew, done, _ = env.step(a)
            robs, rrew, rdone, rreset = ref.step(a)
            self.last_reset[e0:e0 + per] = rreset
            pos, att, vel = np.zeros((per, A)), np.zeros((per, A)), np.zeros((per, A))
            free = np.zeros((per, A, A - 1), dtype=bool)
            for e in range(per):
                g = e0 + e
                if rreset[e]:                               # a new episode: its munitions are gone
                    self.track[g], self.prev_fly[g] = {}, set()
                states = None
                if self.horizon[g] > self.k:
                    states = [(env.state(e, ag), ref.state(e, ag)) for ag in range(A)]
                poses = [(env.pose(e, ag), ref.pose(e, ag)) for ag in range(A)]
                free[e] = self.side_flags_free(poses)
                for ag in range(A):
                    ge, oe = poses[ag]
                    pos[e, ag] = np.linalg.norm(ge[9:12] - oe[9:12])
                    att[e, ag] = np.abs(wrap(ge[3:6] - oe[3:6])).max()
                    vel[e, ag] = np.linalg.norm(ge[6:9] - oe[6:9])
                if states is not None:                      # decisions first: a status that differs explains a done flag that differs
                    for ag in range(A):
                        dg, do = self.discrete(states[ag][0]), self.discrete(states[ag][1])
                        for (nm, x), (_, y) in zip(dg, do):
                            if x != y and self.horizon[g] > self.k:
                                self.horizon[g], self.reason[g] = self.k, nm
                if states is not None and self.horizon[g] > self.k:
                    diffs = self.weapons(g, e, (env, ref), states, poses, msl)
                    if diffs:                               # the first differing weapon decision of this env: a threshold has to explain it
                        if any(w is None for _, w in diffs):
                            self.unexplained.append((g, self.k, "weapon decision", [(d, w or "unexplained") for d, w in diffs]))
                        self.horizon[g] = self.k
                        self.reason[g] = diffs[0][0][0] + " (" + ", ".join(sorted({w or "unexplained" for _, w in diffs})) + ")"
                        msl["msl_pos_m"][g] = msl["msl_vel_ms"][g] = 0.0
                if (done[e] != rdone[e]).any() and not self.done_mismatch[g]:
                    self.done_mismatch[g] = True
                    if self.horizon[g] >= self.k:           # no decision differed BEFORE this step: a threshold has to explain it
                        why = []
                        for ag in np.argwhere(done[e, :, 0] != rdone[e, :, 0])[:, 0]:
                            if done[e, ag, 0]:              # the device terminated this aircraft, the oracle flies on: look at the oracle's
                                why.append(self.near_a_threshold(ref.state(e, ag), poses[ag][1], self.k))
                            else:
                                why.append(self.near_a_threshold(env.state(e, ag), poses[ag][0], self.k))
                        if any(w is None for w in why):
                            self.unexplained.append((g, self.k, done[e, :, 0].tolist(), rdone[e, :, 0].tolist()))
                        self.horizon[g], self.reason[g] = self.k, "done (" + ", ".join(w or "unexplained" for w in why) + ")"
            # a launch on the side under test by an aircraft whose twin has nothing in flight is not seen slot by slot: the handle's count is
            if self.handle_ok[h] and (self.horizon[e0:e0 + per] > self.k).all():
                nd, nr = env.in_flight(), ref.in_flight()
                if nd != nr:
                    self.unexplained.append((f"handle {h}", self.k, "munitions in flight", nd, nr))
                    self.handle_ok[h] = False
            else:
                self.handle_ok[h] = False
            out["pos_m"].append(pos); out["att_rad"].append(att); out["vel_ms"].append(vel)
            out["obs"].append(self.obs_difference(obs, robs, free)); out["rew"].append(np.abs(rew - rrew)[..., 0])
            e0 += per
        res = {k: np.concatenate(v, axis=0) for k, v in out.items()}
        res.update(msl)
        res["live"] = self.horizon > self.k
        self.age[self.last_reset] = 0
        return res

    def reason_counts(self):
        c = {}
        for r in self.reason:
            if r:
                c[r] = c.get(r, 0) + 1
        return c

    def close(self):
        for env, _, _ in self.parts:
            env.close()


# ---- random-action free flight in every kernel form (tests/test_gpu_open_loop.py on the device, tests/test_open_loop_twin.py on the fp32 twin)
# (id, task, aircraft per side, environment that pins the kernel form, envs, seed). 300 steps each: divergence and munition fly-outs need the 30 s.
# The seeds were chosen with the fp32 twin (test_open_loop_twin.py), never with the device.
RANDOM_STEPS = 300
SHOOT_PROBABILITY = 0.05
RANDOM_FORMS = [
    ("C2 three-wave", "singlecombat", 1, {"AIRCOMBAT_SPLIT": "1"}, 32, 20250401),
    ("C2 one-wave (every batch above 32 768 aircraft)", "singlecombat", 1, {"AIRCOMBAT_SPLIT": "0"}, 32, 20250402),
    ("C3 quad form: three FDM waves + environment wave", "singlecombat_shoot", 1, {"AIRCOMBAT_QUAD": "1"}, 32, 20250403),
    ("C3 pair form: one flight wave + environment wave", "singlecombat_shoot", 1, {"AIRCOMBAT_QUAD": "0"}, 32, 20250404),
    ("C4 legacy multiplecombat 2v2, three-wave", "multiplecombat", 2, {"AIRCOMBAT_SPLIT": "1"}, 16, 20250405),
    ("C4 legacy multiplecombat 2v2, one-wave", "multiplecombat", 2, {"AIRCOMBAT_SPLIT": "0"}, 16, 20250406),
    ("C4 scenario_nvn 2v2, pair form (RAW pose reduced on the environment wave)", "scenario_nvn", 2, {}, 16, 20250407),
    ("C5 scenario_nvn 4v4, pair form", "scenario_nvn", 4, {}, 8, 20250408),
    ("scenario1 quad form", "scenario1", 1, {"AIRCOMBAT_QUAD": "1"}, 32, 20250409),
    ("scenario1 pair form", "scenario1", 1, {"AIRCOMBAT_QUAD": "0"}, 32, 20250410),
]
RANDOM_FORM_IDS = [f[0].split(":")[0].split(" (")[0].replace(" ", "_").replace(",", "") for f in RANDOM_FORMS]


def random_actions(task, E, A, steps, seed):
    """Control indices uniform, redrawn every 5 steps; every weapon / shoot column Bernoulli(0.05), redrawn every step. One stream for the
    controls and one for the weapon bits: the flight of a form does not depend on its action width."""
    rc, rw = np.random.default_rng([seed, 0]), np.random.default_rng([seed, 1])
    W = len(STRAIGHT[task]) - 4
    for k in range(steps):
        if k % 5 == 0:
            ctl = np.stack([rc.integers(0, n, size=(E, A)) for n in (41, 41, 41, 30)], axis=-1).astype(np.float32)
        bits = (rw.random((E, A, W)) < SHOOT_PROBABILITY).astype(np.float32)
        yield np.concatenate([ctl, bits], axis=-1)


def fly(pair, actions, name, strict=True):
    """Flies `pair` through `actions` and holds every env inside its horizon to the 8x envelope in its episode age (aircraft: all five
    quantities; munitions still closing: position and velocity) and to `not pair.unexplained`, after every step. strict: assert; else
    the violations [(what, step, value, bound)] are returned with the figures."""
    E = pair.E
    age = np.zeros(E, dtype=np.int64)
    worst, violations, steps = {}, [], 0
    for act in actions:
        m = pair.step(act)
        steps += 1
        age += 1
        live = m["live"]
        env = envelope(age * pair.substeps / 6.0)
        for key, bound in env.items():
            b = 8.0 * bound[:, None]
            ok = (m[key] <= b) | ~live[:, None]
            if not ok.all():
                bad = np.argwhere(~ok)[:4]
                rec = (key, pair.k, bad.tolist(), m[key][~ok][:4].tolist(), b[bad[:, 0], 0].tolist(), age[bad[:, 0]].tolist())
                assert not strict, (name,) + rec
                violations.append(rec)
            worst[key] = max(worst.get(key, 0.0), float((m[key] / b)[live].max()) if live.any() else 0.0)
        for key in ("pos_m", "vel_ms"):
            b, v = 8.0 * env[key], m["msl_" + key]
            ok = (v <= b) | ~live
            if not ok.all():
                bad = np.argwhere(~ok)[:4, 0]
                rec = ("msl_" + key, pair.k, bad.tolist(), v[bad].tolist(), b[bad].tolist(), age[bad].tolist())
                assert not strict, (name,) + rec
                violations.append(rec)
        assert not (strict and pair.unexplained), (name, pair.unexplained)
        age[pair.last_reset] = 0
    h = np.minimum(pair.horizon, steps)
    r3 = lambda d: {k: round(v, 3) for k, v in d.items()}
    print(f"random actions [{name}]: envs still comparable after {steps} steps {int((pair.horizon > steps).sum())}/{E}; horizon min {int(h.min())}, "
          f"p10 {np.percentile(h, 10):.0f}, median {np.median(h):.0f}; first differing decision: {pair.reason_counts()}; "
          f"worst fraction of the 8x envelope used: aircraft {r3(worst)}, munitions closing {r3(pair.worst_msl['closing'])}, "
          f"after the pass (not asserted) {r3(pair.worst_msl['after the pass'])}; munitions flown {pair.msl_flown} in {int(pair.flown.sum())}/{E} envs, "
          f"ended {pair.msl_ended}")
    return {"worst": worst, "violations": violations, "steps": steps}


def assert_random_flight_conditions(pair, task, steps):
    """What a random-action flight must have exercised for its comparison to mean something (conditions, not measurements)."""
    assert not pair.unexplained, pair.unexplained
    assert (pair.horizon > 100).mean() >= 0.9, pair.reason_counts()      # the regime with a stated tolerance is the common case, not the exception
    if len(STRAIGHT[task]) > 4:                                            # the forms with weapon columns
        assert pair.flown.mean() >= 0.5, (int(pair.flown.sum()), pair.E)  # a munition was in flight at some step in at least half of the envs
        assert pair.msl_ended >= 1                                         # and at least one reached a terminal status inside an env's horizon
