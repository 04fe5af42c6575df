"""The termination lattice (tests/termination_util.py) held to account without a GPU: the oracle against a second oracle, teacher-forced,
on the very cases that tests/test_gpu_terminations.py sets the device.

control         the oracle against itself over the whole lattice: no difference at all;
coverage        from the oracle's outcomes alone: every termination kind a family has appears as a done code; both sides of every
                threshold are present and the closest case on each side lies inside the window the lattice promises (altitude 1 m,
                load factors 0.01 g, heading error 1 deg; the integer gates have both neighbouring values by construction: ticks 598..602,
                current_step max_steps - 2 .. max_steps + 1); every pair-of-conditions and agent-walk case exists; every kept case is
                at least 5 bounds away from every threshold;
planted faults  a second oracle with one change each. The harness must report it in the case groups where the fault acts and in no
                other: the altitude limit moved by one ladder step, acc_limit_z moved by 0.01, Overload reading npz without the + 1
                (the imported baz shifted by one g), max_steps off by one, the tick gate at 601 (the imported ticks word one less), an
                UnreachHeading check one step early, the launcher's missile made harmless, and the ordering fault: the aircraft permuted in the
                second oracle's env."""
import pytest

import termination_util as T

FAMILY_IDS = [f.replace(" ", "_") for f in T.FAMILIES]


@pytest.fixture(scope="module")
def ix(pkg):
    return T.field_index(pkg)


def lattices(pkg, oracle, ix, fam):
    return [T.lattice(pkg, oracle, ix, fam, key) for key in T.configs(fam)]


@pytest.mark.parametrize("fam", list(T.FAMILIES), ids=FAMILY_IDS)
def test_control_oracle_against_itself_is_exact(pkg, oracle, ix, fam):
    for lat in lattices(pkg, oracle, ix, fam):
        fails = T.compare(lat, T.OracleSide(oracle, lat), strict=False)
        assert not fails, (fam, lat.key, fails[:4])
        for case, out in zip(lat.cases, lat.outcomes):          # bit for bit, not only inside the bounds
            env_out = T.play(oracle, lat, lat.cases.index(case), case.pre0, case.act, edits=case.edits)
            for k in range(lat.steps):
                assert (env_out.obs[k] == out.obs[k]).all() and (env_out.rew[k] == out.rew[k]).all() and (env_out.info[k] == out.info[k]).all(), (fam, case.label, k)


def expected_codes(fam):
    F = T.FAMILIES[fam]
    codes = {0, 1, 2, 3, 7}
    if F["safe_return"]:
        codes |= {4, 5, 6}
    if fam == "heading":
        codes |= {8}
    if "g1" not in T.configs(fam):
        codes -= {2, 3}         # ExtremeState is placed through one-substep steps only; the six-substep Overload is aircraft 0's, and the row carries aircraft 1's message
    return codes


@pytest.mark.parametrize("fam", list(T.FAMILIES), ids=FAMILY_IDS)
def test_coverage(pkg, oracle, ix, fam):
    lats = lattices(pkg, oracle, ix, fam)
    cov = T.coverage(lats)
    T.print_coverage(fam, cov)
    assert set(cov["codes"]) == expected_codes(fam), (fam, cov["codes"])        # every kind the family has, and no kind it has not
    windows = {"altitude": T.ALT_WINDOW_M, "heading error": T.HEADING_WINDOW_DEG}
    g1 = "g1" in T.configs(fam)
    ladders = ("npx extreme", "npy extreme", "npz extreme", "npx overload", "npy overload", "npz overload") if g1 else ()
    for name in ("altitude",) + ladders + (("heading error",) if fam == "heading" else ()):
        lo, hi = cov["closest"][name]
        w = windows.get(name, T.NP_WINDOW)
        assert lo is not None and hi is not None and lo[0] <= w and hi[0] <= w, (fam, name, lo, hi)
        assert lo[1] >= T.MARGIN_X and hi[1] >= T.MARGIN_X, (fam, name, lo, hi)
    for lat in lats:                                                            # the margin holds for every case, at every step
        for case, out in zip(lat.cases, lat.outcomes):
            assert T.margins(lat, out, ix) >= T.MARGIN_X, (fam, case.label)
    labels = cov["labels"]
    has = lambda text: any(text in l for l in labels)
    for t in (598, 599, 600, 601, 602) if g1 else ():
        assert has(f"overload gate: evaluated at tick {t},"), (fam, t)
    g6 = "g6" in T.configs(fam)
    for t in (594, 599, 600, 605, 606) if g6 else ():
        assert has(f"six substeps: evaluated at tick {t},"), (fam, t)
    for m in (1, 2, 3):
        for cur in range(max(1, m - 2), m + 2):
            assert has(f"timeout: max_steps {m}, evaluated at current_step {cur}"), (fam, m, cur)
        assert has(f"pair: LowAltitude + Timeout (max_steps {m})"), fam
    for pair in ("pair: LowAltitude + Overload", "pair: LowAltitude + ExtremeState", "pair: ExtremeState + Overload", "pair: LowAltitude + ExtremeState + Overload") if g1 else ():
        assert has(pair), (fam, pair)
    assert cov["groups"].get("overload6", 0) >= 6 or not g6, cov["groups"]
    A = lats[0].A
    if A == 1:
        assert has("pair: UnreachHeading + LowAltitude") == (fam == "heading") and has("+ LowAltitude") and has("heading error of 40 deg alone")
        if fam == "heading":
            assert sum("at the second check" in l for l in labels) >= 8
        return
    walk = ["already CRASH (set before this step)", "already CRASH (since the step before)", "already SHOTDOWN (set before this step)",
            "already SHOTDOWN (since the step before)", "already CRASH and below the altitude limit", "already SHOTDOWN and below the altitude limit",
            ] + (["Overload, aircraft", "LowAltitude, aircraft"] if g1 else [])
    if A == 2:
        walk += ["walk: agent 0 crashes", "walk: agent 1 crashes", "walk: both crash"]
    else:
        walk += ["team0 all low-altitude", "team1 all low-altitude", "everybody low-altitude", "last survivor of team0 crashes", "last survivor of team1 crashes",
                 "team0 dead since the step before", "team1 dead since the step before", "one aircraft per team crashes"]
    for w in walk:
        assert has(w), (fam, w)
    for a in (0, A - 1):
        assert has(f"aircraft {a} already CRASH") and has(f"aircraft {a} already SHOTDOWN"), (fam, a)


def test_the_asymmetric_whole_team_outcomes_are_the_oracles(pkg, oracle, ix):
    """The rule the walk cases exist for, read off the oracle's outcomes: in a 2v2 where team 0 crashes at this evaluation team 1 ends
    with mission complete in the same step; where team 1 crashes team 0 is not done at this step. In 1v1 an aircraft that was
    already CRASH and sits below the limit becomes a LowAltitude crash again (code 1); in NvN it stays what it was (code 5 / 4)."""
    lat = T.lattice(pkg, oracle, ix, "multiplecombat 2v2", "alt")
    by = {c.label: o for c, o in zip(lat.cases, lat.outcomes)}
    t0, t1 = by["walk: nvn2 team0 all low-altitude"], by["walk: nvn2 team1 all low-altitude"]
    assert t0.done[0].tolist() == [True] * 4 and t0.info[0].tolist() == [1, 6, 0, 1]
    assert t1.done[0].tolist() == [False, False, True, True] and t1.info[0].tolist() == [1, 1, 0, 0]
    assert by["pair: aircraft 3 already CRASH and below the altitude limit"].info[0][1] == 5
    assert by["pair: aircraft 3 already SHOTDOWN and below the altitude limit"].info[0][1] == 4
    one = T.lattice(pkg, oracle, ix, "singlecombat", "alt")
    by = {c.label: o for c, o in zip(one.cases, one.outcomes)}
    assert by["pair: aircraft 1 already CRASH and below the altitude limit"].info[0][1] == 1
    wvr = T.lattice(pkg, oracle, ix, "wvr_lowlevel", "alt")
    by = {c.label: o for c, o in zip(wvr.cases, wvr.outcomes)}
    assert by["walk: agent 0 crashes"].done[0].tolist() == [True, False]      # no SafeReturn: a dead enemy ends nothing


# ---- planted faults: (name, lattice keys, the change, groups that must fail, groups that may)
def _limit(name, delta):
    def edit(ocfg):
        setattr(ocfg, name, getattr(ocfg, name) + delta)
    return edit


def _shift(field, delta, ix_holder):
    def transform(st, k, e, a):
        if k == 0:
            st[ix_holder[field]] += delta
        return st
    return transform


FAULT_FAMILIES = ["singlecombat", "wvr_lowlevel", "multiplecombat 2v2", "scenario_nvn 2v2", "heading", "approach"]


def run_fault(pkg, oracle, ix, fam, keys, cfg_edit=None, transform=None, ignore=()):
    groups, labels = set(), []
    for key in keys:
        lat = T.lattice(pkg, oracle, ix, fam, key)
        fails = [f for f in T.compare(lat, T.OracleSide(oracle, lat, transform=transform, cfg_edit=cfg_edit), strict=False) if f[3] not in ignore]
        groups |= set(T.failed_groups(fails))
        labels += [f[0] for f in fails]
    return groups, labels


@pytest.mark.parametrize("fam", FAULT_FAMILIES, ids=[f.replace(" ", "_") for f in FAULT_FAMILIES])
def test_planted_faults_are_caught_where_they_act(pkg, oracle, ix, fam):
    keys = T.configs(fam)
    # 1. the altitude limit a ladder step higher (0.3 m: past the cases 0.25 m above it, which now crash); nothing else sits that close
    groups, labels = run_fault(pkg, oracle, ix, fam, keys, cfg_edit=_limit("altitude_limit", 0.3))
    assert groups == {"altitude"} and any("+0.25 m" in l for l in labels), (fam, groups, labels[:4])
    # 2. acc_limit_z 0.01 higher: the npz ladder's cases 0.005 above the limit no longer fire
    groups, labels = run_fault(pkg, oracle, ix, fam, ("g1",), cfg_edit=_limit("acc_limit_z", 0.01))
    assert groups == {"overload"} and all("npz" in l for l in labels) and len(set(labels)) >= 2, (fam, groups, labels[:4])
    #    ... and Overload reading npz where it should read npz + 1: the imported baz one g lower shifts what it sees by -1
    groups, labels = run_fault(pkg, oracle, ix, fam, ("g1",), transform=_shift("baz", -T.G0, ix))
    assert "overload" in groups and any("is not over the limit" in l for l in labels) and any("npz = +1.5" in l for l in labels), (fam, groups, labels[:4])
    # 3. max_steps one more
    groups, labels = run_fault(pkg, oracle, ix, fam, ("time1", "time2", "time3"), cfg_edit=_limit("max_steps", 1))
    assert "timeout" in groups and groups <= {"timeout", "pair"}, (fam, groups, labels[:4])
    assert all("Timeout" in l or "timeout" in l for l in labels), labels
    # 4. the gate one tick late (ticks imported one less; the stored ticks word itself is then off everywhere and is not what is looked for)
    groups, labels = run_fault(pkg, oracle, ix, fam, ("g1", "g6"), transform=_shift("ticks", -1, ix), ignore=("ticks",))
    assert groups == {"gate"} and sorted(set(labels)) == sorted({"overload gate: evaluated at tick 600, npz = -4.5",
                                                                   "overload gate, six substeps: evaluated at tick 600, limit exceeded"}), (fam, groups, labels)
    if fam == "heading":
        # UnreachHeading's 10 deg moved by half a degree cannot be planted through the config; its check interval can: a check one
        # step early looks at a heading error that must not be looked at
        for key, delta in (("hdg", -0.1), ("hdg1", -0.02)):
            groups, labels = run_fault(pkg, oracle, ix, fam, (key,), cfg_edit=_limit("check_interval", delta))
            assert groups == {"heading"} and len(set(labels)) >= 8, (fam, key, groups, labels[:4])


class PermutedOracle(T.OracleSide):
    """The ordering fault: a second oracle whose env lists the aircraft in another order (the teams swapped in the config, the states
    imported permuted, every output permuted back). Whatever does not depend on the walk over the agents in env order is unchanged."""

    def __init__(self, oracle, lat):
        A, half = lat.A, lat.A // 2
        self.perm = list(range(half, A)) + list(range(half))           # slot p holds aircraft perm[p]
        self.inv = [self.perm.index(a) for a in range(A)]

        def swap(ocfg):
            init = [type(ocfg.init[0]).from_buffer_copy(ocfg.init[i]) for i in range(A)]
            nm = [ocfg.num_missiles[i] for i in range(A)]
            for p in range(A):
                ocfg.init[p], ocfg.num_missiles[p] = init[self.perm[p]], nm[self.perm[p]]
        super().__init__(oracle, lat, cfg_edit=swap)

    def sync(self, k, e, a, st):
        self.envs[e].import_state(self.inv[a], st)

    def step(self, act, k=0):
        obs, rew, done, infos, _ = super().step(act[:, self.perm], k)
        return obs[:, self.inv], rew[:, self.inv], done[:, self.inv], infos, None

    def state(self, e, a):
        return self.envs[e].export_state(self.inv[a])


NVN_ORDER = (["walk: nvn2 team0 all low-altitude", "walk: nvn2 team1 all low-altitude", "walk: nvn2 last survivor of team0 crashes",
              "walk: nvn2 last survivor of team1 crashes"], ["walk: nvn2 one aircraft per team crashes", "walk: nvn2 the second of each team crashes"])
ORDER = {   # family -> (cases the walk decides: must differ, cases it does not: must not)
    # ("walk: both crash" in 1v1 does NOT change: both messages are LowAltitude, code 1 either way; the case with two different messages
    #  in one row, Overload + LowAltitude, is the one that resolves which agent's message the row keeps)
    "singlecombat": (["walk: agent 0 crashes", "walk: agent 1 crashes", "pair: aircraft 0 Overload, aircraft 1 LowAltitude"], ["walk: both crash"]),
    "wvr_lowlevel": (["pair: aircraft 0 Overload, aircraft 1 LowAltitude"], ["walk: agent 0 crashes", "walk: agent 1 crashes", "walk: both crash"]),
    "multiplecombat 2v2": NVN_ORDER,
    "scenario_nvn 2v2": NVN_ORDER,
}
# scenario_nvn's observations and rewards depend on the order of the aircraft in other ways than the walk (in every case): under the
# permutation only the decision itself is compared there
DECISION_ONLY = {"scenario_nvn 2v2": ("done", "info row", "status", "die_flag")}


@pytest.mark.parametrize("fam", list(ORDER), ids=[f.replace(" ", "_") for f in ORDER])
def test_the_ordering_fault_changes_the_walk_cases_and_nothing_else(pkg, oracle, ix, fam):
    """5. The agents of the second oracle permuted. It must change the asymmetric cases -- a whole team or a team's last survivor crashing
    at this evaluation, one aircraft's crash in 1v1 (the other's mission complete comes in the same step or the next), two different
    messages in one row -- and no case in which every aircraft stays alive through the three steps: the lattice resolves the walk."""
    must, must_not = ORDER[fam]
    changed = set()
    for key in (k for k in T.configs(fam) if k != "msl"):     # (the weapon bits and targets of a chain are not permuted)
        lat = T.lattice(pkg, oracle, ix, fam, key)
        fails = T.compare(lat, PermutedOracle(oracle, lat), strict=False)
        if fam in DECISION_ONLY:
            fails = [f for f in fails if f[3] in DECISION_ONLY[fam]]
        changed |= {f[0] for f in fails}
        somebody_dead = {c.label for c, o in zip(lat.cases, lat.outcomes) if any((p[:, ix["status"]] != T.ALIVE).any() for p in o.post)}
        assert {f[0] for f in fails} <= somebody_dead, (fam, key, sorted({f[0] for f in fails} - somebody_dead)[:4])
    for label in must:
        assert label in changed, (fam, label)
    for label in must_not:
        assert label not in changed, (fam, label)


@pytest.mark.parametrize("fam", list(T.MSL_FAMILIES), ids=[f.replace(" ", "_") for f in T.MSL_FAMILIES])
def test_a_harmless_missile_ends_the_target_early_and_is_caught(pkg, oracle, ix, fam):
    """6. SafeReturn's missile clause, in all four missile tasks: every launcher the task's rule allows produces its three cases (from the
    oracle: the missile is launched, flies at least 10 steps, ends by a hit inside the chain with two steps to follow, and while it
    flies the target of a dead launcher team is not done). In the second oracle every missile is made harmless as soon as it is
    launched (set_missile_status: a miss). The target then gets its mission complete at the step the launcher's team dies instead of
    staying not-done: every missile case differs, the killed-launcher ones from that step on, and nothing else does."""
    MISS = 2
    lat = T.lattice(pkg, oracle, ix, fam, "msl")
    assert lat.E == (3 if fam == "scenario1" else 6) and lat.steps <= 40 and not lat.drops, (fam, lat.E, lat.drops)
    kills = {}
    for case, out in zip(lat.cases, lat.outcomes):
        L = int(case.label.split("aircraft ")[1][0])
        flown = [k for k in range(lat.steps) if any(m[3] == L and m[0] == T.MSL_LAUNCHED for m in out.msl[k])]
        assert flown and len(flown) >= 10 and flown[-1] < lat.steps - 3, (case.label, flown)      # it flew for a while; two steps follow its end
        target = next(m[4] for m in out.msl[flown[0]] if m[3] == L)
        if case.edits:
            kill = kills[case.label] = min(case.edits)
            for k in range(kill, flown[-1] + 1):                                                 # launcher done, target not, while the missile flies
                assert out.done[k][L] and not out.done[k][target], (case.label, k, out.done[k])
            assert out.done[flown[-1] + 1].all() and out.info[flown[-1] + 1][3] == 1, case.label   # and the episode ends when it ends

    def harmless(env, k):
        for j, m in enumerate(env.missiles()):
            if int(m[0]) == T.MSL_LAUNCHED:
                env.set_missile_status(j, MISS)
    fails = T.compare(lat, T.OracleSide(oracle, lat, after=harmless), strict=False)
    assert T.failed_groups(fails) == ["missile"] and {f[0] for f in fails} == {c.label for c in lat.cases}, (fam, fails[:3])
    for label, kill in kills.items():
        assert any(f[0] == label and f[2] == kill and f[3] == "done" for f in fails), (fam, label)
    # the other lattices of the family never launch: the fault changes nothing there
    for key in ("alt", "time3"):
        other = T.lattice(pkg, oracle, ix, fam, key)
        assert not T.compare(other, T.OracleSide(oracle, other, after=harmless), strict=False), (fam, key)


def test_body_rate_at_1000_is_an_extreme_load_factor_already(pkg, oracle, ix):
    """Why the lattice has no ladder around the body-rate norm of 1000 rad/s: with such a roll rate imported (one substep) the oracle's
    step is finite, but the pilot-station load factor is far beyond 10 on BOTH sides of 1000 rad/s, so ExtremeState fires either way
    and the comparison against 1000 decides nothing."""
    lat = T.lattice(pkg, oracle, ix, "singlecombat", "g1")
    for wp in (999.5, 1000.5, -999.5, -1000.5):
        pre = lat.base(0)
        pre[0][ix["wp"]] += wp
        out = T.play(oracle, lat, 0, pre, lat.level, steps=1)
        post = out.post[0][0]
        rate = (post[ix["ap"]] ** 2 + post[ix["aq"]] ** 2 + post[ix["ar"]] ** 2) ** 0.5
        assert all(map(lambda v: v == v and abs(v) < 1e300, post)) and abs(rate - abs(wp)) < 0.1, (wp, rate)
        assert abs(post[ix["npz"]]) > 1e4 and out.done[0][0], (wp, post[ix["npz"]], out.done[0])
