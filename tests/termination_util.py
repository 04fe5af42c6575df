"""Terminations and done codes at their thresholds, shared by tests/test_termination_twin.py (CPU: the oracle against a second oracle,
planted faults) and tests/test_gpu_terminations.py (the device against the oracle, every family and kernel form).

A Lattice is one (family, config): the family's default config with some limits lowered, and a list of cases. A case is one env: the
state every aircraft has before the step (an export_state vector, task record included: status, die_flag, cur_step and ticks travel in
it), one action, and the oracle's outcome for that step and the two steps after it. Both sides are teacher-forced to the oracle's state
before every step, so one `step` of a handle with as many envs as cases evaluates the whole lattice.

The lattice "msl" (SafeReturn's missile clause; singlecombat_shoot, singlecombat_dodge_missile, scenario1, scenario_nvn 2v2) is a chain
of 40 steps instead: the launch comes through the task's own rule at the step read off the oracle's run (step 0 by a weapon bit, step 9 by
dodge_missile's lock window), the launcher's whole team is killed before the next step, munitions fly open-loop on both sides. The range
at which the oracle's missile ends, and its last range while flying, must be MARGIN_X x MSL_BOUND_M from the fuse radius (margins());
MSL_BOUND_M rests on a measurement of the fp32 twins of missile_probe_util, not on a bound held on the device.

The oracle alone decides which cases exist. Builders make candidates by moving the imported position (altitude), the imported body
acceleration words (with agent_interaction_steps = 1 the evaluation reads the load factors that tick 1 computes from them), `ticks`
and `cur_step`, and in the heading task by importing another stream's spawn (its heading against this env's target); a candidate
becomes a case only if, at every compared step, every deciding quantity of every aircraft is at least
MARGIN_X times the suite's existing one-step bound for that quantity away from every threshold of the config (margins() below). No case
is ever dropped because of what a side under test returns. coverage() reports, from the oracle's outcomes only, the closest case on
either side of every threshold and the done codes, case groups and walk cases present.

compare() holds, per case and step: `done` per agent and the whole info row [current_step, done code, heading_turn_counts, env-reset
flag] equal; of every aircraft status, die_flag, bloods, cur_step and ticks equal and pre_event to 1e-6 (after an episode end these are
the reset template's: current_step restarts, the Overload gate closes again); rewards and observations (the auto-reset observation
included) with parity_util's RewardBound / obs_bounds at the scale of the family's existing teacher-forced test. A failure names the
family, the form, the case's label, the step, the agent and both rows."""
import ctypes as C

import numpy as np

from parity_util import TASK_FIELDS, RewardBound, obs_bounds, team_max

MARGIN_X = 5.0
ALT_BOUND_M = 0.02              # the reported pose one step after an identical state (envelope_util.POSE_POS_M)
NP_BOUND = 1.5e-5               # x max(1, |np|) x max(1, qbar / 405): test_singlecombat_kernel_forms_teacher_forced, envelope_util.Q_FIELDS
RATE_BOUND = 3e-6               # x max(1, |x|): ap, aq, ar
Q_REF = 405.0
G0 = 32.174                     # ft/s^2 per g: d(np) / d(imported body acceleration) at tick 1, measured on the oracle and refined per case
STEPS = 3                       # the decision and the two steps after it
SEED = 5
ALT_LIMIT = 6090.0              # m, exactly a float32; the shipped spawn is 20 000 ft = 6096 m
ACC_LIMIT = 2.5
ALT_WINDOW_M, NP_WINDOW = 1.0, 0.01
ALIVE, CRASH, SHOTDOWN = 0, 1, 2
# done codes (include/aircombat.h): 1 LowAltitude, 2 ExtremeState, 3 Overload, 4 / 5 / 6 SafeReturn's shot down / crashed / mission complete,
# 7 Timeout, 8 UnreachHeading

# family -> task, aircraft per side (0: a single-aircraft task), HipShareVecEnv, SafeReturn in the list, (observation, reward) scale of
# the family's existing teacher-forced test, kernel form pins that exist for it
FAMILIES = {
    "singlecombat": dict(task="singlecombat", per_side=1, share=False, safe_return=True, scale=(1.0, 1.0), forms=({"AIRCOMBAT_SPLIT": "0"}, {"AIRCOMBAT_SPLIT": "1"})),
    "singlecombat_shoot": dict(task="singlecombat_shoot", per_side=1, share=False, safe_return=True, scale=(3.0, 3.0), forms=({"AIRCOMBAT_QUAD": "0"}, {"AIRCOMBAT_QUAD": "1"})),
    "scenario1": dict(task="scenario1", per_side=1, share=False, safe_return=True, scale=(4.0, 4.0), forms=({"AIRCOMBAT_QUAD": "0"}, {"AIRCOMBAT_QUAD": "1"})),
    "singlecombat_dodge_missile": dict(task="singlecombat_dodge_missile", per_side=1, share=False, safe_return=True, scale=(4.0, 4.0), forms=({},)),
    "wvr_lowlevel": dict(task="wvr_lowlevel", per_side=1, share=False, safe_return=False, scale=(1.0, 3.0), forms=({},)),
    "multiplecombat 2v2": dict(task="multiplecombat", per_side=2, share=True, safe_return=True, scale=(2.0, 2.0), forms=({"AIRCOMBAT_SPLIT": "0"}, {"AIRCOMBAT_SPLIT": "1"})),
    "multiplecombat 4v4": dict(task="multiplecombat", per_side=4, share=True, safe_return=True, scale=(2.0, 2.0), forms=({"AIRCOMBAT_SPLIT": "0"}, {"AIRCOMBAT_SPLIT": "1"})),
    "scenario_nvn 2v2": dict(task="scenario_nvn", per_side=2, share=True, safe_return=True, scale=(4.0, 4.0), forms=({},)),
    "scenario_nvn 4v4": dict(task="scenario_nvn", per_side=4, share=True, safe_return=True, scale=(4.0, 4.0), forms=({},)),
    # the controller runs before the step ([3, 5, 3] -> BaselineActor -> control indices); the decision must not care
    "hierarchical_singlecombat": dict(task="hierarchical_singlecombat", per_side=1, share=False, safe_return=True, scale=(2.0, 4.0), forms=({},), hier=True),
    "heading": dict(task="heading", per_side=0, share=False, safe_return=False, scale=(2.0, 1.0), forms=({},)),
    "approach": dict(task="approach", per_side=0, share=False, safe_return=False, scale=(2.0, 1.0), forms=({},)),
}
RAGGED = {"singlecombat": 70}   # this family's altitude lattice is padded to 70 envs: 140 lanes, a ragged last workgroup
CONFIGS = ("alt", "g1", "g6", "time1", "time2", "time3")
HEADING_BOUND_DEG = float(np.degrees(2e-4))     # attitude, 2e-4 rad (envelope_util.POSE_ATT_RAD)
HEADING_WINDOW_DEG = 1.0
MSL_LAUNCHED = 0
# SafeReturn's missile clause: latitude offset (deg) of the second team's spawn, from a scan of the oracle alone: the nearest spawn at which
# the launcher's missile ends by a hit well inside the fuse radius before step 37
MSL_SPAWN = {"singlecombat_shoot": 0.022, "singlecombat_dodge_missile": 0.017, "scenario1": 0.035, "scenario_nvn 2v2": 0.03}
MSL_FAMILIES = tuple(MSL_SPAWN)
MSL_BOUND_M = 0.2               # NOT an existing suite bound (none exists for a munition's position after a fly-out): set here, above the
                                # fp32 twins' measured worst deviation of 0.155 m (missile_probe_util.TWIN)
FLIP_GAP = 1e-4                 # top-two logit gap of the oracle's controller below which the device's argmax may differ (test_gpu_parity.FLIP_GAP)


def configs(fam):
    """The lattices of a family: "hdg" / "hdg1" lower UnreachHeading's check interval, so that a check time falls inside the chain;
    "msl" is the missile tasks' chain."""
    keys = CONFIGS
    if fam == "singlecombat_dodge_missile":     # its lock window holds at most 31 steps per second: ac_create refuses one-substep steps
        keys = tuple(k for k in keys if k != "g1")
    if FAMILIES[fam].get("hier"):               # (Lattice.stale_observation_margin: the pull-up's states are far from the reset's observation)
        keys = tuple(k for k in keys if k != "g6")
    return keys + (("hdg", "hdg1") if fam == "heading" else ()) + (("msl",) if fam in MSL_FAMILIES else ())


def nvn(fam):
    return FAMILIES[fam]["per_side"] >= 2


def family_config(pkg, fam, key, acc_z6=None):
    """The family's default config with the limits of lattice `key`. Every limit given here is exactly a float32."""
    F = FAMILIES[fam]
    if nvn(fam):
        cfg = pkg.default_nvn_config(F["per_side"], task=F["task"])
        A = cfg.n_agents
        for i in range(A):      # off the shipped exactly-head-on geometry, where PostureReward's atanh is singular (test_gpu_parity.py)
            cfg.init[i].lon_deg += 0.013 * (i % 3) + (0.02 if i >= A // 2 else 0.0)
            cfg.init[i].psi_deg = (7.0 + 3.0 * i) if i < A // 2 else (171.0 + 2.0 * i)
    else:
        cfg = pkg.default_config(F["task"])
    cfg.altitude_limit = ALT_LIMIT
    if key == "msl":            # close and nose-on (test_one_wave_and_three_wave_forms_agree's spawn, nearer: the chain stays under 40 steps)
        cfg.altitude_limit = 2500.0
        dlat = MSL_SPAWN[fam]
        if nvn(fam):
            for i in range(cfg.n_agents // 2, cfg.n_agents):
                cfg.init[i].lat_geod_deg = 60.0 + dlat
        else:
            cfg.init[0].psi_deg = 9.0
            cfg.init[1].lon_deg, cfg.init[1].lat_geod_deg, cfg.init[1].psi_deg = 120.0 + 0.27 * dlat, 60.0 + dlat, 171.0
        if fam == "singlecombat_dodge_missile":     # the rule launches once the 10-step lock window is full; one missile each
            cfg.min_attack_interval = 100
    elif key == "g1":
        cfg.agent_interaction_steps = 1
        cfg.acc_limit_x = cfg.acc_limit_y = cfg.acc_limit_z = ACC_LIMIT
    elif key == "g6":
        cfg.acc_limit_z = float(np.float32(acc_z6))
    elif key.startswith("time"):
        cfg.max_steps = int(key[4:])
    elif key == "hdg":          # checks at the first step (0.1 s >= 0) and the third (0.3 s >= 0.25 s), none at the second
        cfg.check_interval = 0.25
    elif key == "hdg1":         # one tick per step: a check at tick 1, none at tick 2, and tick 3 is the check time itself (3 / 60 s against 0.05)
        cfg.agent_interaction_steps = 1
        cfg.check_interval = 0.05
    for v in (cfg.altitude_limit, cfg.acc_limit_x, cfg.acc_limit_y, cfg.acc_limit_z):
        assert float(np.float32(v)) == float(v), (fam, key, v)
    return cfg


class Case:
    def __init__(self, label, group, pre, act, tags=(), edits=None):
        self.label, self.group, self.pre0, self.act, self.tags = label, group, np.array(pre), np.array(act, dtype=np.float32), tuple(tags)
        self.edits = edits      # {step: edit(pre)}: changes to the state a later step starts from (part of the oracle's recorded pre[k])


# ---- the oracle's run of one case
class Outcome:
    """pre[k], obs[k], rew[k], done[k], info[k] of the three steps; post[k] / alt[k]: the record and geodetic altitude at the
    evaluation (before any reset); after[k]: the record the next step starts from; hdg[k]: the heading error UnreachHeading looked
    at (None: it did not look); rnn[k] / gap[k]: hierarchical tasks, the controller's GRU state before the step and the smallest
    top-two logit gap of its call."""


def new_oracle_env(oracle, lat, e, ocfg=None):
    ocfg = lat.ocfg if ocfg is None else ocfg
    if lat.single:          # env i of a handle owns numpy's PCG64 stream of seed + 1000 i (HipVecEnv._seed_heading)
        return oracle.OracleEnv(ocfg, pcg64_state=np.random.PCG64(SEED + 1000 * e).state)
    return oracle.OracleEnv(ocfg)


def play(oracle, lat, e, pre0, act, steps=None, transform=None, env=None, edits=None):
    """The oracle's outcome of one case. transform(st, k, a) edits what is imported (planted faults); edits[k](pre) changes the state
    that step k starts from on BOTH sides (it is part of the recorded pre[k]); act may be one action or one per step."""
    env = env or new_oracle_env(oracle, lat, e)
    env.reset()
    steps = lat.steps if steps is None else steps
    act = np.asarray(act)
    A = lat.A
    out = Outcome()
    out.pre, out.obs, out.rew, out.done, out.info, out.post, out.alt, out.after, out.hdg = [], [], [], [], [], [], [], [], []
    pre = np.array(pre0)
    unreach = lat.single and not lat.cfg.approach
    out.rnn, out.gap, out.msl = [], [], []
    for k in range(steps):
        if edits and k in edits:
            edits[k](pre)
        out.pre.append(pre.copy())
        if lat.hier:
            out.rnn.append(np.array([env.get_rnn(a)[0] for a in range(A)]))
        for a in range(A):
            st = pre[a] if transform is None else transform(pre[a].copy(), k, a)
            env.import_state(a, st)
        if unreach:
            target, _, _, check_time, _ = heading_get(env)
        o, r, d, info = env.step(act[k] if act.ndim == 3 else act)
        out.msl.append([(int(m[0]), float(x[4]), float(x[5]), int(m[11]), int(m[12])) for m, x in zip(env.missiles(), env.missiles_ext())])   # status, last range, fuse radius, parent, target
        err = None
        if unreach and sim_time(env.export_state(0)[lat.ix["ticks"]]) >= check_time:     # UnreachHeading looked at the heading error
            err = abs((target - np.degrees(env.pose(0)[5]) + 180.0) % 360.0 - 180.0)
        out.hdg.append(err)
        out.gap.append(min(float(env.ctl_gaps(a).min()) for a in range(A)) if lat.hier else None)
        out.post.append(np.array([env.export_state(a) for a in range(A)]))
        out.alt.append(np.array([env.pose(a)[2] for a in range(A)]))
        if info[3]:
            o = env.reset()
        out.obs.append(o); out.rew.append(r.copy()); out.done.append(d.copy()); out.info.append(info.copy())
        pre = np.array([env.export_state(a) for a in range(A)])
        out.after.append(pre.copy())
    return out


def heading_get(env):
    """Target heading deg, altitude ft, speed m/s, next check time s, turn counts of the oracle's heading task."""
    out = np.zeros(8)
    env.L.or_env_heading_get(env.p, out.ctypes.data_as(C.POINTER(C.c_double)))
    return out[:5]


def sim_time(ticks):
    """The clock after `ticks` ticks: the running fp64 sum of 1/60 that both implementations compare with the check time."""
    t = 0.0
    for _ in range(int(ticks)):
        t += 1.0 / 60.0
    return t


def qscale(oracle, st, ix, alt_m):
    out = [C.c_double() for _ in range(5)]
    oracle.lib().f16_atmosphere(float(alt_m / 0.3048), *[C.byref(o) for o in out])
    return max(1.0, 0.7 * out[1].value * st[ix["mach"]] ** 2 / Q_REF)


def thresholds(lat, st, ix, alt_m, hdg_err=None):
    """(name, deciding quantity, threshold, the suite's one-step bound for the quantity) of one aircraft at one evaluation."""
    c = lat.cfg
    qs = lat.qs(st, alt_m)
    out = [("altitude", alt_m, c.altitude_limit, ALT_BOUND_M)]
    for ax, lim in (("npx", c.acc_limit_x), ("npy", c.acc_limit_y)):
        v = abs(st[ix[ax]])
        b = NP_BOUND * max(1.0, v) * qs
        out.append((ax + " extreme", v, 10.0, b))
        out.append((ax + " overload", v, lim, b))
    z = st[ix["npz"]]
    b = NP_BOUND * max(1.0, abs(z)) * qs
    out.append(("npz extreme", abs(z), 10.0, b))
    out.append(("npz overload", abs(z + 1.0), c.acc_limit_z, b))
    rate = float(np.sqrt(st[ix["ap"]] ** 2 + st[ix["aq"]] ** 2 + st[ix["ar"]] ** 2))
    out.append(("body rate", rate, 1000.0, RATE_BOUND * max(1.0, rate)))
    if hdg_err is not None:
        out.append(("heading error", hdg_err, 10.0, HEADING_BOUND_DEG))
    return out


def margins(lat, outcome, ix):
    """Smallest distance from a threshold in units of its bound, over the steps and aircraft of a case; the candidate is a case only if
    it is at least MARGIN_X."""
    worst = np.inf
    for k in range(len(outcome.post)):
        for j, (status, rng, rc, _, _) in enumerate(outcome.msl[k]):     # the step at which a munition ends is a decision inside ITS bound
            before = outcome.msl[k - 1][j] if k > 0 and j < len(outcome.msl[k - 1]) else None
            if before is not None and before[0] == MSL_LAUNCHED and np.isfinite(before[1]):
                worst = min(worst, abs(before[1] - rc) / MSL_BOUND_M)      # the last range of a step in which it still flew
            if status != MSL_LAUNCHED and before is not None and before[0] == MSL_LAUNCHED:
                worst = min(worst, abs(rng - rc) / MSL_BOUND_M)            # the range it ended at
        if lat.hier:            # a near-tie of the oracle's own controller logits: the control indices themselves are not decided there
            worst = min(worst, outcome.gap[k] / FLIP_GAP)
        for a in range(lat.A):
            for _, v, thr, b in thresholds(lat, outcome.post[k][a], ix, outcome.alt[k][a], outcome.hdg[k]):
                worst = min(worst, abs(v - thr) / b)
    return worst


# ---- builders
def shifted_altitude(st, d_m):
    st = st.copy()
    r = st[0:3]
    st[0:3] = r + (d_m / 0.3048) * r / np.linalg.norm(r)
    return st


class Lattice:
    def __init__(self, pkg, oracle, ix, fam, key):
        self.fam, self.key, self.ix, self.oracle = fam, key, ix, oracle
        F = FAMILIES[fam]
        self.single, self.hier = F["per_side"] == 0, bool(F.get("hier"))
        self.steps = STEPS
        acc_z6 = None
        if key == "g6":
            self._pulls = {}
            self.pull = lambda e: self._pulls.setdefault(e if self.single else 0, pull_up(pkg, oracle, ix, fam, e if self.single else 0))
            v = self.pull(0)[0]
            k = max(range(3, 8), key=lambda j: abs(v[j + 1] - v[j]))
            acc_z6 = 0.5 * (v[k] + v[k + 1])        # between the |npz + 1| of two consecutive evaluations of the pull-up
        self.cfg = family_config(pkg, fam, key, acc_z6)
        self.ocfg = oracle.config_from_ac(self.cfg)
        self.A = self.cfg.n_agents
        env = oracle.OracleEnv(self.ocfg)
        self.act_dim, self.obs_dim = env.act_dim, env.obs_dim
        self.level = np.zeros((self.A, self.act_dim), dtype=np.float32)
        if self.hier:
            self.level[:, :3] = (1, 2, 1)       # no change of altitude, heading, speed
        else:
            self.level[:, :4] = (20, 18.6, 20, 15)
        self.cases, self.outcomes, self.drops = [], [], []     # drops: (label, env, margin) of the candidates the oracle refused
        self._qs, self._spawn = {}, {}

    def qs(self, st, alt_m):
        key = (round(float(alt_m), 1), round(float(st[self.ix["mach"]]), 4))
        if key not in self._qs:
            self._qs[key] = qscale(self.oracle, st, self.ix, alt_m)
        return self._qs[key]

    def base(self, e):
        """The reset state of env `e` of a handle (the single-aircraft tasks draw their spawn per env)."""
        env = new_oracle_env(self.oracle, self, e)
        env.reset()
        return np.array([env.export_state(a) for a in range(self.A)])

    def stick(self, v, what):
        """The level action with aircraft v's elevator index (hierarchical: its altitude command) set to descend / climb / pull."""
        act = self.level.copy()
        if self.hier:
            act[v, 0] = {"descending": 2.0, "climbing": 0.0, "pull": 0.0}[what]
        else:
            act[v, 1] = {"descending": 30.0, "climbing": 8.0, "pull": 0.0}[what]
        return act

    def spawn(self, e):
        """(reset state, spawn heading deg) of the env that owns stream e (single-aircraft tasks)."""
        if e not in self._spawn:
            env = new_oracle_env(self.oracle, self, e)
            env.reset()
            self._spawn[e] = (np.array([env.export_state(0)]), float(heading_get(env)[0]))
        return self._spawn[e]

    def foreign(self, e, want_deg, target=None, pool=range(1000, 2200)):
        """The spawn state of another stream whose heading is nearest to want_deg short of `target` (default: env e's own spawn heading,
        the target of its first UnreachHeading check)."""
        target = self.spawn(e)[1] if target is None else target
        err = lambda j: abs((target - self.spawn(j)[1] - want_deg + 180.0) % 360.0 - 180.0)
        return self.spawn(min(pool, key=err))[0].copy()

    def place(self, e, pre, act, alt=None, nps=None):
        """Moves the imported position / body accelerations so that the oracle's evaluation of step 0 finds aircraft a at altitude
        alt[a] (m) and load factor nps[(a, axis)]: two rounds against the oracle's own outcome."""
        pre = np.array(pre)
        for _ in range(2):
            out = play(self.oracle, self, e, pre, act, steps=1)
            for a, want in (alt or {}).items():
                pre[a] = shifted_altitude(pre[a], want - out.alt[0][a])
            for (a, ax), want in (nps or {}).items():
                pre[a][self.ix["ba" + ax]] += (want - out.post[0][a][self.ix["np" + ax]]) * G0
        return pre

    def stale_observation_margin(self, e, act, out):
        """Hierarchical tasks: the device's controller reads the observation the previous step (or the reset) returned, which an
        imported state does not refresh, while the oracle observes the imported state itself. A candidate is a case only if the
        oracle's own controller, fed the reset's observation instead, gives the same four control indices at step 0 with the
        same margin on its top-two logit gaps. Returns the smallest gap / FLIP_GAP (0: the indices differ)."""
        env = new_oracle_env(self.oracle, self, e)
        robs = env.reset()
        d_alt, d_vel = (0.1, 0.0, -0.1), (0.05, 0.0, -0.05)
        d_hdg = (-np.pi / 6, -np.pi / 12, 0.0, np.pi / 12, np.pi / 6)
        for a in range(self.A):
            env.import_state(a, out.pre[0][a])
        env.step(act)           # (no reset after it: the controller's last output is read below)
        worst = np.inf
        for a in range(self.A):
            x = np.concatenate([[d_alt[int(act[a, 0])], d_hdg[int(act[a, 1])], d_vel[int(act[a, 2])]], robs[a, :9]])
            low, _, logits = self.oracle.actor_forward(x, np.zeros(128))
            if (low != env.get_rnn(a)[1]).any():
                return 0.0
            for lo, hi in ((0, 41), (41, 82), (82, 123), (123, 153)):
                top = np.sort(logits[lo:hi])
                worst = min(worst, (top[-1] - top[-2]) / FLIP_GAP)
        return worst

    def add(self, label, group, pre, act=None, tags=(), edits=None):
        """A candidate: it becomes a case if the oracle's outcome keeps every margin. Its env index is its place in the handle."""
        e = len(self.cases)
        act = self.level if act is None else act
        out = play(self.oracle, self, e, pre, act, edits=edits)
        m = margins(self, out, self.ix) if all(np.isfinite(o).all() for o in out.obs) else -1.0
        if self.hier and m >= MARGIN_X:
            m = min(m, self.stale_observation_margin(e, act, out))
        if m < MARGIN_X:
            self.drops.append((label, e, m))        # (-1: the oracle's own observation was not finite)
            return False
        self.cases.append(Case(label, group, pre, act, tags, edits))
        self.outcomes.append(out)
        return True

    def candidate(self, label, group, tags=(), act=None, alt=None, nps=None, edit=None, hdg_err=None, retry=1):
        """Builds a candidate for the env index it would get: base state, `edit(pre)` (status, ticks, cur_step ...), then placement.
        The single-aircraft tasks draw their spawn altitude: there the aircraft is always placed, 6 m above the limit by default."""
        e, alt_arg = len(self.cases), alt
        pre = self.base(e) if hdg_err is None else self.foreign(e, hdg_err)
        act = self.level if act is None else act
        if edit is not None:
            edit(pre)
        if self.single and not alt:
            alt = {0: ALT_LIMIT + 6.0}
        if alt or nps:
            pre = self.place(e, pre, act, alt, nps)
        if self.add(label, group, pre, act, tags):
            return True
        if self.single and retry > 0:       # the spawn this stream draws (now or after the episode's end) sits on a threshold: the next stream's may not
            refused = self.drops.pop()
            if self.candidate(f"level flight, stream {e}", "padding", retry=0):
                return self.candidate(label, group, tags, act, alt_arg, nps, edit, hdg_err, retry - 1)
            self.drops.append(refused)
        return False

    def pad(self, n):
        """Level-flight cases up to n envs (a ragged last workgroup)."""
        while len(self.cases) < n:
            assert self.candidate(f"level flight, padding env {len(self.cases)}", "padding")

    @property
    def E(self):
        return len(self.cases)

    @property
    def dropped(self):
        return len(self.drops)


def _set(pre, ix, a, **kw):
    for f, v in kw.items():
        pre[a][ix[f]] = v


def dead(ix, a, status, latched):
    """Aircraft a already CRASH / SHOTDOWN before the step; latched: since the step before (die_flag set, the -200 already paid)."""
    def edit(pre):
        _set(pre, ix, a, status=status)
        if latched:
            _set(pre, ix, a, die_flag=1, pre_event=-200.0)
    return edit


def both(*edits):
    def edit(pre):
        for f in edits:
            f(pre)
    return edit


def ticks_edit(ix, A, ticks):
    def edit(pre):
        for a in range(A):
            _set(pre, ix, a, ticks=ticks)
    return edit


def step_edit(ix, A, cur):
    def edit(pre):
        for a in range(A):
            _set(pre, ix, a, cur_step=cur)
    return edit


LADDER_M = (-1.0, -0.75, -0.5, -0.25, 0.25, 0.5, 0.75, 1.0)
LADDER_G = (-0.02, -0.005, 0.005, 0.02)
LOW = ALT_LIMIT - 2.0
OPEN = 700                      # a `ticks` word past the Overload gate


def build_alt(lat):
    """Config "alt": LowAltitude's ladder, the agent walk, aircraft that were dead already."""
    ix, A, half = lat.ix, lat.A, max(1, lat.A // 2)
    victims = sorted({0, A - 1})
    for v in victims:
        for d in LADDER_M:
            lat.candidate(f"low-altitude ladder, aircraft {v} at limit {d:+.2f} m", "altitude", alt={v: ALT_LIMIT + d})
    for v, name in zip(victims * 2, ("descending", "climbing")):
        act = lat.stick(v, name)
        for d in (-0.5, -0.25, 0.25, 0.5):
            lat.candidate(f"low-altitude ladder, aircraft {v} {name}, at limit {d:+.2f} m", "altitude", act=act, alt={v: ALT_LIMIT + d})
    if A == 1:
        unreach = not lat.cfg.approach
        if unreach:         # the imported state is another stream's spawn: its heading against this env's target at the first check
            for sign in (1.0, -1.0):
                for d in (-0.7, -0.3, 0.3, 0.7):
                    lat.candidate(f"unreach-heading ladder: heading error about {sign * (10.0 + d):+.1f} deg at the first check", "heading", hdg_err=sign * (10.0 + d))
        what = "UnreachHeading" if unreach else "a heading error of 40 deg (no UnreachHeading in this task)"
        lat.candidate(f"pair: {what} + LowAltitude", "pair", ("pair",), alt={0: LOW}, hdg_err=40.0)
        lat.candidate(f"heading error of 40 deg alone", "heading", hdg_err=40.0)
        return
    low = lambda *acs: {a: LOW for a in acs}
    t0, t1 = list(range(half)), list(range(half, A))
    if A == 2:
        lat.candidate("walk: agent 0 crashes", "walk", ("walk",), alt=low(0))
        lat.candidate("walk: agent 1 crashes", "walk", ("walk",), alt=low(1))
        lat.candidate("walk: both crash", "walk", ("walk", "asymmetric"), alt=low(0, 1))
    else:
        n = f"nvn{half}"
        lat.candidate(f"walk: {n} team0 all low-altitude", "walk", ("walk", "asymmetric"), alt=low(*t0))
        lat.candidate(f"walk: {n} team1 all low-altitude", "walk", ("walk", "asymmetric"), alt=low(*t1))
        lat.candidate(f"walk: {n} everybody low-altitude", "walk", ("walk", "asymmetric"), alt=low(*t0, *t1))
        for nm, team in (("team0", t0), ("team1", t1)):
            lat.candidate(f"walk: {n} last survivor of {nm} crashes", "walk", ("walk",), alt=low(team[-1]),
                          edit=both(*[dead(ix, a, CRASH, True) for a in team[:-1]]))
            lat.candidate(f"walk: {n} {nm} dead since the step before", "walk", ("walk",), edit=both(*[dead(ix, a, CRASH if a % 2 else SHOTDOWN, True) for a in team]))
        lat.candidate(f"walk: {n} one aircraft per team crashes", "walk", ("walk",), alt=low(0, half))
        lat.candidate(f"walk: {n} the second of each team crashes", "walk", ("walk",), alt=low(1, half + 1))
    for a in victims:
        for status, nm in ((CRASH, "CRASH"), (SHOTDOWN, "SHOTDOWN")):
            for latched in (False, True):
                when = "since the step before" if latched else "set before this step"
                lat.candidate(f"walk: aircraft {a} already {nm} ({when})", "walk", ("walk",), edit=dead(ix, a, status, latched))
            lat.candidate(f"pair: aircraft {a} already {nm} and below the altitude limit", "pair", ("pair",), alt=low(a), edit=dead(ix, a, status, True))


def build_g1(lat):
    """Config "g1": one substep, acc limits 2.5: ExtremeState and Overload on every axis and sign, `npz + 1`, the tick gate, pairs."""
    ix, A = lat.ix, lat.A
    victims = sorted({0, A - 1})
    opened = ticks_edit(ix, A, OPEN)
    for ax in "xyz":
        for sign in (1.0, -1.0):
            for d in LADDER_G:
                v = victims[0] if ax != "z" else victims[-1]
                lat.candidate(f"extreme ladder, aircraft {v} np{ax} = {sign * (10.0 + d):+.3f} (gate closed)", "extreme", nps={(v, ax): sign * (10.0 + d)})
                if ax != "z":
                    lat.candidate(f"overload ladder, aircraft {v} np{ax} = {sign * (ACC_LIMIT + d):+.3f}", "overload", nps={(v, ax): sign * (ACC_LIMIT + d)}, edit=opened)
                else:       # |npz + 1| against the limit on both signs: npz near +1.5 is inside |npz| < 2.5 and must fire, npz near -3.5 outside
                    lat.candidate(f"overload ladder, aircraft {v} npz = {-1.0 + sign * (ACC_LIMIT + d):+.3f}", "overload", nps={(v, "z"): -1.0 + sign * (ACC_LIMIT + d)}, edit=opened)
    v = victims[0]
    for d in LADDER_G:      # |npz| near the limit itself decides nothing: -2.5 +- d is |npz + 1| = 1.5
        lat.candidate(f"overload: aircraft {v} npz = {-(ACC_LIMIT + d):+.3f} is not over the limit", "overload", nps={(v, "z"): -(ACC_LIMIT + d)}, edit=opened)
    for t in (597, 598, 599, 600, 601):
        lat.candidate(f"overload gate: evaluated at tick {t + 1}, npz = -4.5", "gate", ("gate",), nps={(v, "z"): -4.5}, edit=ticks_edit(ix, A, t))
    low = {v: LOW}
    lat.candidate("pair: LowAltitude + Overload", "pair", ("pair",), alt=low, nps={(v, "z"): -4.5}, edit=opened)
    lat.candidate("pair: LowAltitude + ExtremeState", "pair", ("pair",), alt=low, nps={(v, "x"): 11.0})
    lat.candidate("pair: ExtremeState + Overload", "pair", ("pair",), nps={(v, "x"): 11.0}, edit=opened)
    lat.candidate("pair: LowAltitude + ExtremeState + Overload", "pair", ("pair",), alt=low, nps={(v, "y"): -11.0}, edit=opened)
    if A > 1:
        w = victims[-1]
        lat.candidate(f"pair: aircraft {v} Overload, aircraft {w} LowAltitude", "pair", ("pair", "walk"), alt={w: LOW}, nps={(v, "z"): -4.5}, edit=opened)
        lat.candidate(f"pair: aircraft {v} LowAltitude, aircraft {w} ExtremeState", "pair", ("pair", "walk"), alt=low, nps={(w, "z"): 10.5})


def build_g6(lat):
    """Config "g6": the default six substeps with acc_limit_z lowered: the load factor that counts is the last tick's; the env steps
    on either side of tick 600."""
    ix, A = lat.ix, lat.A
    act = lat.stick(0, "pull")
    for k in range(8):
        lat.add(f"six substeps: pull-up step {k}, gate open", "overload6", lat.pull(lat.E)[1][k], act)
    for t in (588, 593, 594, 599, 600):
        p = lat.pull(lat.E)[1][-1].copy()
        for a in range(A):
            p[a][ix["ticks"]] = t
        lat.add(f"overload gate, six substeps: evaluated at tick {t + 6}, limit exceeded", "gate", p, act, ("gate",))


_PULL_LAT = {}


def pull_up(pkg, oracle, ix, fam, e):
    """Aircraft 0 of env e pulls from the reset with six substeps and the gate open: |npz + 1| at the nine evaluations, and the states
    before steps 1..8."""
    if fam not in _PULL_LAT:
        _PULL_LAT[fam] = Lattice(pkg, oracle, ix, fam, "alt")
    lat = _PULL_LAT[fam]
    act = lat.stick(0, "pull")
    pre = lat.base(e)
    if lat.single:
        pre = lat.place(e, pre, act, alt={0: ALT_LIMIT + 300.0})
    for a in range(lat.A):
        pre[a][ix["ticks"]] = OPEN
    out = play(oracle, lat, e, pre, act, steps=9)
    return [abs(p[0][ix["npz"]] + 1.0) for p in out.post], [out.pre[j] for j in range(1, 9)]


def build_hdg(lat):
    """Configs "hdg" / "hdg1" (heading): the first step's check passes and draws a new target, the second step is before the next
    check time and must not look at the heading, the third is at it. The imported state is another stream's spawn, chosen so that
    the heading error against the NEW target is near +-10 deg; an env whose draw leaves no such choice flies its own spawn."""
    wants = [s * (10.0 + d) for d in (-0.7, -0.3, 0.3, 0.7) for s in (1.0, -1.0)] * 5
    for want in wants:
        e = lat.E
        env = new_oracle_env(lat.oracle, lat, e)
        env.reset()
        env.step(lat.level)
        new_target, own = float(heading_get(env)[0]), lat.spawn(e)[1]
        first = abs((own - (new_target - want) + 180.0) % 360.0 - 180.0)         # the heading error the first check would see
        if first < 9.0:
            pre = lat.place(e, lat.foreign(e, want, target=new_target), lat.level, alt={0: ALT_LIMIT + 6.0})
            if lat.add(f"check-time chain: heading error about {want:+.1f} deg at the second check, none looked at between", "heading", pre, tags=("check",)):
                continue
        lat.candidate(f"check-time chain: own spawn, stream {e}", "heading", tags=("check",))


def build_msl(lat):
    """Config "msl" (SafeReturn's missile clause): aircraft L launches through the task's own rule -- the shoot bit, the AIM-9M bit of the
    scenario tasks, the lock-window rule of dodge_missile -- and its whole team is given CRASH or SHOTDOWN before the next step. The
    target must stay not-done while the missile flies and ends at the step at which the oracle's missile ends; an aircraft of its team
    that has no missile coming ends with mission complete at once. Munitions fly open-loop on both sides, the aircraft are
    teacher-forced. The launch step is read off the oracle's own run."""
    ix, A, half = lat.ix, lat.A, max(1, lat.A // 2)
    lat.steps = 40
    launchers = (0,) if lat.fam == "scenario1" else (0, half)      # Scenario1 refreshes the ego team's weapon bits only
    for L in launchers:
        act = np.repeat(lat.level[None], lat.steps, axis=0)
        if lat.act_dim == 5:
            act[0, L, 4] = 1.0
        elif lat.act_dim == 8:
            act[0, L, 6] = 1.0          # [gun, AIM-9M, AIM-120B, chaff]
        probe = play(lat.oracle, lat, lat.E, lat.base(lat.E), act)
        launch = next((k for k in range(lat.steps) if any(m[3] == L for m in probe.msl[k])), None)
        if launch is None:
            lat.drops.append((f"missile clause: aircraft {L} never launches", lat.E, -1.0))
            continue
        team = [a for a in range(A) if (a < half) == (L < half)] if A > 1 else [L]
        for status, nm in ((CRASH, "CRASH"), (SHOTDOWN, "SHOTDOWN"), (ALIVE, "alive (the control)")):
            def kill(pre, team=team, status=status):
                for a in team:
                    _set(pre, ix, a, status=status)
            lat.add(f"missile clause: aircraft {L} launches at step {launch}, then its team is {nm} while its missile flies", "missile", lat.base(lat.E), act,
                    ("missile",), edits={launch + 1: kill} if status != ALIVE else None)


def build_time(lat):
    """Configs "time1" .. "time3": cur_step on either side of max_steps, and a crash condition together with Timeout."""
    ix, A, m = lat.ix, lat.A, lat.cfg.max_steps
    for cur in range(max(0, m - 3), m + 1):
        lat.candidate(f"timeout: max_steps {m}, evaluated at current_step {cur + 1}", "timeout", ("timeout",), edit=step_edit(ix, A, cur))
    lat.candidate(f"pair: LowAltitude + Timeout (max_steps {m})", "pair", ("pair",), alt={0: LOW}, edit=step_edit(ix, A, m - 1))
    if A > 1:
        lat.candidate(f"pair: aircraft {A - 1} already CRASH + Timeout (max_steps {m})", "pair", ("pair",),
                      edit=both(step_edit(ix, A, m - 1), dead(ix, A - 1, CRASH, True)))


_LATTICES = {}      # per process: pkg, oracle and ix are the session's one library, one oracle and its field index


def lattice(pkg, oracle, ix, fam, key):
    """The lattice of (family, config), built once and shared; nothing changes it afterwards."""
    if (fam, key) not in _LATTICES:
        lat = Lattice(pkg, oracle, ix, fam, key)
        {"alt": build_alt, "g1": build_g1, "g6": build_g6, "hdg": build_hdg, "hdg1": build_hdg, "msl": build_msl}.get(key, build_time)(lat)
        if key == "alt" and fam in RAGGED:
            lat.pad(RAGGED[fam])
        assert 0 < lat.E <= 96, (fam, key, lat.E)
        _LATTICES[(fam, key)] = lat
    return _LATTICES[(fam, key)]


def field_index(pkg):
    names = pkg.load_library().state_field_names()
    return {nm: k for k, nm in enumerate(names) if nm}


# ---- coverage, from the oracle's outcomes only
def coverage(lats):
    """closest[(threshold name)] = [closest case below, closest case above] as (distance, distance / bound, label), over the decision
    step of every case; codes: the done codes seen in info rows and how often; groups / labels: the cases per group."""
    closest, codes, groups, labels, n = {}, {}, {}, [], 0
    for lat in lats:
        for case, out in zip(lat.cases, lat.outcomes):
            n += 1
            groups[case.group] = groups.get(case.group, 0) + 1
            labels.append(case.label)
            for k in range(lat.steps):
                c = int(out.info[k][1])
                codes[c] = codes.get(c, 0) + 1
            for a in range(lat.A):
                for name, v, thr, b in [t for k in range(lat.steps) for t in thresholds(lat, out.post[k][a], lat.ix, out.alt[k][a], out.hdg[k]) if k == 0 or t[0] == "heading error"]:
                    if name.endswith("overload") and out.post[0][a][lat.ix["ticks"]] < 600:
                        continue            # the gate is closed: the limit decides nothing there
                    side = 0 if v <= thr else 1
                    cur = closest.setdefault(name, [None, None])
                    if cur[side] is None or abs(v - thr) < cur[side][0]:
                        cur[side] = (abs(v - thr), abs(v - thr) / b, case.label)
    return dict(closest=closest, codes=codes, groups=groups, labels=labels, cases=n, dropped=sum(l.dropped for l in lats))


def print_coverage(title, cov):
    print(f"{title}: {cov['cases']} cases, done codes {dict(sorted(cov['codes'].items()))}, groups {cov['groups']}")
    for name, (lo, hi) in sorted(cov["closest"].items()):
        f = lambda s: "none" if s is None else f"{s[0]:.4g} = {s[1]:.1f} bounds"
        print(f"  {name:16s} closest case not above the threshold: {f(lo)}; above: {f(hi)}")


# ---- sides under test
class OracleSide:
    """A second oracle. transform(st, k, e, a) edits what it imports, cfg_edit(ocfg) its config: the planted faults."""

    def __init__(self, oracle, lat, transform=None, cfg_edit=None, after=None):
        self.lat, self.after = lat, after       # after(env, k): a change to the second oracle's env after step k (planted faults)
        ocfg = oracle.copy_config(lat.ocfg)
        if cfg_edit is not None:
            cfg_edit(ocfg)
        self.envs = [new_oracle_env(oracle, lat, e, ocfg) for e in range(lat.E)]
        self.transform = transform
        for env in self.envs:
            env.reset()

    def sync(self, k, e, a, st):
        if self.transform is not None:
            st = self.transform(st.copy(), k, e, a)
        self.envs[e].import_state(a, st)

    def sync_rnn(self, e, a, h):
        self.envs[e].set_rnn(a, h)

    def step(self, act, k=0):
        obs, rew, done, infos = [], [], [], []
        for env, a in zip(self.envs, act):
            o, r, d, info = env.step(a)
            if info[3]:
                o = env.reset()
            if self.after is not None:
                self.after(env, k)
            obs.append(o); rew.append(r); done.append(d); infos.append(info)
        return np.stack(obs), np.stack(rew)[..., None], np.stack(done)[..., None], np.stack(infos), None

    def state(self, e, a):
        return self.envs[e].export_state(a)

    def close(self):
        pass


class DeviceSide:
    """HipVecEnv / HipShareVecEnv with as many envs as the lattice has cases. The info rows are read from the device buffers
    (device_tensors()[4]); the packed host words of the same step are returned next to them."""

    def __init__(self, pkg, lat, envs=None):
        """envs: the size of the handle where it is larger than the lattice (the large-grid kernel variants): the cases are its first
        envs, the others fly level from their reset."""
        F = FAMILIES[lat.fam]
        self.share, self.E, self.level = F["share"], lat.E, lat.level
        self.env = (pkg.HipShareVecEnv if self.share else pkg.HipVecEnv)(lat.cfg, envs or lat.E, seed=SEED)
        self.env.reset()
        # with munitions in flight the weapon bookkeeping (slots, remaining, last missile) stays the device's own, as in the existing
        # weapon tests: the flight state and the status word are imported
        self.words = None
        if lat.key == "msl":
            self.words = np.array(sorted(k for nm, k in lat.ix.items() if not nm.startswith("x_") and (nm not in TASK_FIELDS or nm == "status")))

    def sync(self, k, e, a, st):
        if self.words is not None:
            v = self.env.get_state(e, a)
            v[self.words] = st[self.words]
            st = v
        self.env.set_state(e, a, st)

    def sync_rnn(self, e, a, h):
        self.env.set_controller_state(e, a, h)

    def step(self, act, k=0):
        E = self.E
        if self.env.num_envs > E:
            act = np.concatenate([act, np.broadcast_to(self.level, (self.env.num_envs - E,) + self.level.shape)])
        out = self.env.step(act)
        obs, rew, done = [x[:E] for x in ((out[0], out[2], out[3]) if self.share else out[:3])]
        words = out[-1]._codes[:E].astype(np.int64) & 0xFFFFFFFF
        rows = self.env.device_tensors()[4][:E].cpu().numpy().copy()
        host = np.stack([words & 0xFFFF, (words >> 16) & 0xFF, (words >> 24) & 0x7F, words >> 31], axis=-1)
        return np.array(obs), np.array(rew), np.array(done), rows, host

    def state(self, e, a):
        return self.env.get_state(e, a)

    def close(self):
        self.env.close()


TASK_EXACT = ("status", "die_flag", "bloods", "cur_step", "ticks")


def compare(lat, side, form="", host_words=False, strict=True):
    """Plays `side` against the lattice's oracle outcomes. Returns the failures as (label, group, step, what, agent, got, want); strict:
    asserts that there are none, naming family, form and the first of them."""
    F, ix, A, E = FAMILIES[lat.fam], lat.ix, lat.A, lat.E
    half = max(1, A // 2)
    bound = RewardBound(lat.cfg.posture_scale, 9 + 6 * (half - 1), half if A > 1 else 0, F["scale"][1])
    fails = []

    def fail(e, k, what, a, got, want):
        fails.append((lat.cases[e].label, lat.cases[e].group, k, what, a, got, want))

    for k in range(lat.steps):
        act = np.stack([c.act[k] if c.act.ndim == 3 else c.act for c in lat.cases])
        for e in range(E):
            for a in range(A):
                side.sync(k, e, a, lat.outcomes[e].pre[k][a])
                if lat.hier:
                    side.sync_rnn(e, a, lat.outcomes[e].rnn[k][a])
        obs, rew, done, rows, host = side.step(act, k)
        robs = np.stack([o.obs[k] for o in lat.outcomes])
        rrew = np.stack([o.rew[k] for o in lat.outcomes])[..., None]
        rdone = np.stack([o.done[k] for o in lat.outcomes])[..., None]
        rinfo = np.stack([o.info[k] for o in lat.outcomes])
        tol, free = obs_bounds(robs, F["scale"][0])
        rt = bound(rrew, robs)
        if A > 2:
            rt = team_max(rt, A)
        for e in range(E):
            if (np.asarray(rows[e]) != rinfo[e]).any():
                fail(e, k, "info row", None, np.asarray(rows[e]).tolist(), rinfo[e].tolist())
            if host_words and host is not None and (host[e] != rinfo[e]).any():
                fail(e, k, "host info word", None, host[e].tolist(), rinfo[e].tolist())
            for a in range(A):
                if bool(done[e, a, 0]) != bool(rdone[e, a, 0]):
                    fail(e, k, "done", a, done[e, :, 0].astype(int).tolist(), rdone[e, :, 0].astype(int).tolist())
                bad = ~free[e, a] & ~(np.abs(obs[e, a] - robs[e, a]) <= tol[e, a])
                if bad.any():
                    j = int(np.argmax(bad))
                    fail(e, k, f"obs[{j}]", a, float(obs[e, a, j]), float(robs[e, a, j]))
                if not abs(rew[e, a, 0] - rrew[e, a, 0]) <= rt[e, a, 0]:
                    fail(e, k, "reward", a, float(rew[e, a, 0]), float(rrew[e, a, 0]))
                got, want = side.state(e, a), lat.outcomes[e].after[k][a]
                for f in TASK_EXACT:
                    if got[ix[f]] != want[ix[f]]:
                        fail(e, k, f, a, float(got[ix[f]]), float(want[ix[f]]))
                if not abs(got[ix["pre_event"]] - want[ix["pre_event"]]) <= 1e-6:
                    fail(e, k, "pre_event", a, float(got[ix["pre_event"]]), float(want[ix["pre_event"]]))
    assert not (strict and fails), (f"{lat.fam} [{lat.key}] {form}: {len(fails)} differences from the oracle; the first: "
                                    + "; ".join(f"case '{f[0]}' step {f[2]} agent {f[4]} {f[3]}: got {f[5]}, oracle {f[6]}" for f in fails[:4]))
    return fails


def failed_groups(fails):
    return sorted({f[1] for f in fails})
