"""The free-flight harness (tests/open_loop_util.py) held to account without a GPU: the oracle against a second oracle.

control        the oracle against itself: every difference is exactly 0 and no horizon ends;
fp32 twin      the second oracle's flight state is rounded to float32 after every env step (export_state -> entries vx..tank1, indices
               3-60, cast; position stays fp64 -> import_state), and its munitions too where the device keeps its slots in fp32 (the 1v1
               missile tasks): it stands for a correct fp32 implementation, and must meet every condition that
               tests/test_gpu_open_loop.py::test_random_actions_open_loop_every_form sets the device, with that test's own tasks, sizes,
               seeds, step count and shoot probability (open_loop_util.RANDOM_FORMS);
planted faults five faults injected into the second oracle only, each of which the harness must catch, and in the stated way.

Sensitivity limit. The 8x envelope is a chaos bound, not a decode check: a THROTTLE index off by one for one 5-step hold sits at its edge
(test_throttle_off_by_one_is_at_the_limit_of_the_envelope prints the fraction used: 1.31 of the velocity envelope for the hold at episode
age 50, where the envelope is still tight, 0.38 for the hold at age 150), where an aileron index off by one uses 39 times the attitude
envelope within two steps. That the stored commands are the decoded action is held by
tests/test_gpu_open_loop.py::test_stored_commands_are_the_decoded_action_in_every_form."""
import numpy as np
import pytest

from open_loop_util import (MSL_HIT, MSL_LAUNCHED, RANDOM_FORM_IDS, RANDOM_FORMS, RANDOM_STEPS, Fp32Twin, OpenLoopPair, OracleSide,
                            assert_random_flight_conditions, fly, random_actions)


def pair_of(pkg, oracle, second, task, per_side, E, **kw):
    def sides(cfg, ocfg, per, ix):
        return second(oracle, ocfg, per, ix), OracleSide(oracle, ocfg, per, ix)
    return OpenLoopPair(pkg, oracle, E, spread=True, task=task, per_side=per_side, sides=sides, **kw)


@pytest.mark.parametrize("task,per_side,E", [("singlecombat_shoot", 1, 8), ("scenario_nvn", 2, 8)])
def test_control_oracle_against_itself_is_exact(pkg, oracle, task, per_side, E):
    pair = pair_of(pkg, oracle, OracleSide, task, per_side, E)
    for act in random_actions(task, pair.E, pair.A, 200, 11):
        m = pair.step(act)
        for key, v in m.items():
            assert key == "live" or (v == 0.0).all(), (key, pair.k)
        assert m["live"].all() and not pair.unexplained, (pair.k, pair.reason, pair.unexplained)
    assert pair.msl_flown > 0 and pair.msl_ended > 0          # the exact comparison covered munitions from launch to their end
    assert pair.worst_msl == {"closing": {"pos_m": 0.0, "vel_ms": 0.0}, "after the pass": {"pos_m": 0.0, "vel_ms": 0.0}}


@pytest.mark.parametrize("form", RANDOM_FORMS, ids=RANDOM_FORM_IDS)
def test_fp32_twin_meets_the_gpu_tests_conditions(pkg, oracle, form):
    name, task, per_side, _, E, seed = form
    pair = pair_of(pkg, oracle, Fp32Twin, task, per_side, E)
    fly(pair, random_actions(task, pair.E, pair.A, RANDOM_STEPS, seed), "fp32 twin, inputs of " + name)
    assert_random_flight_conditions(pair, task, RANDOM_STEPS)


# ---- planted faults: the second oracle only
FAULT_AT = 50       # env step (1-based) at which a fault begins: the start of a 5-step hold of random_actions


class ControlIndexOff(OracleSide):
    column, at = 0, FAULT_AT          # aileron

    def step(self, act):
        if self.at <= self.k + 1 < self.at + 5:
            act = act.copy()
            act[:, 0, self.column] = np.where(act[:, 0, self.column] < (40 if self.column < 3 else 29), act[:, 0, self.column] + 1, act[:, 0, self.column] - 1)
        return super().step(act)


class ThrottleIndexOff(ControlIndexOff):
    column = 3


class ThrottleIndexOffLate(ThrottleIndexOff):
    at = 150


def shifted_hold_actions(task, E, A, steps, seed):
    """random_actions whose 5-step holds begin at steps 1, 6, ... FAULT_AT - 4 + 5 n: unchanged, FAULT_AT = 50 is NOT a boundary (holds begin at
    1-based steps 1, 6, .., 46, 51), so the fault classes above are given a stream cut to put one there."""
    it = random_actions(task, E, A, steps + 1, seed)
    next(it)
    return it


def test_aileron_off_by_one_leaves_the_envelope_within_two_steps(pkg, oracle):
    pair = pair_of(pkg, oracle, ControlIndexOff, "singlecombat", 1, 8)
    rep = fly(pair, shifted_hold_actions("singlecombat", pair.E, pair.A, FAULT_AT + 10, 5), "planted: aileron index + 1", strict=False)
    assert rep["violations"], "an aileron index off by one for a whole hold went unnoticed"
    first = min(v[1] for v in rep["violations"])
    assert FAULT_AT <= first <= FAULT_AT + 1, (first, rep["violations"][:3])      # nothing before the fault, and within two steps of it


@pytest.mark.parametrize("fault", [ThrottleIndexOff, ThrottleIndexOffLate], ids=["at_step_50", "at_step_150"])
def test_throttle_off_by_one_is_at_the_limit_of_the_envelope(pkg, oracle, fault):
    pair = pair_of(pkg, oracle, fault, "singlecombat", 1, 8)
    rep = fly(pair, shifted_hold_actions("singlecombat", pair.E, pair.A, fault.at + 100, 5), f"sensitivity limit: throttle index + 1 for the hold at step {fault.at}", strict=False)
    frac = max(rep["worst"].values())
    print(f"sensitivity limit: a throttle index off by one for the hold at step {fault.at} uses", round(frac, 3), "of the 8x envelope at most")
    assert 0.0 < frac < 4.0      # seen, but at the envelope's edge (the aileron's figure is 39): the module docstring says what holds the decode instead


class ShootBitLate(OracleSide):
    """Every shoot bit reaches the env one step late."""

    def step(self, act):
        late = act.copy()
        late[..., 4] = self.prev if self.k else 0.0
        self.prev = act[..., 4].copy()
        return super().step(late)


def test_shoot_bit_a_step_late_is_an_unexplained_weapon_decision(pkg, oracle):
    pair = pair_of(pkg, oracle, ShootBitLate, "singlecombat_shoot", 1, 8)
    acts = list(random_actions("singlecombat_shoot", pair.E, pair.A, 120, 7))
    fly(pair, iter(acts), "planted: shoot bit one step late", strict=False)
    first_bit = [1 + min(k for k, a in enumerate(acts) if a[e, :, 4].any()) for e in range(pair.E)]
    caught = {u[0]: u for u in reversed(pair.unexplained)}
    for e in range(pair.E):
        g, k, what, diffs = caught[e]
        assert k == first_bit[e] and what == "weapon decision", (e, first_bit[e], caught[e])
        assert any(d[0] == "shoot_action" for d, _ in diffs), diffs


class TargetSwapped(OracleSide):
    """Every munition is aimed at the OTHER enemy at its launch."""

    def step(self, act):
        out = super().step(act)
        for env in self.vec.envs:
            for k, m in enumerate(env.missiles()):
                if int(m[0]) == MSL_LAUNCHED and m[9] == 0.0:
                    foes = [j for j in range(self.A) if (j < self.A // 2) != (int(m[11]) < self.A // 2)]
                    env.set_missile_target(k, foes[1 - foes.index(int(m[12]))])
        return out


def test_swapped_target_is_a_target_mismatch(pkg, oracle):
    pair = pair_of(pkg, oracle, TargetSwapped, "scenario_nvn", 2, 8)
    fly(pair, random_actions("scenario_nvn", pair.E, pair.A, 200, 7), "planted: target swapped at launch", strict=False)
    assert pair.msl_flown > 0
    hits = [u for u in pair.unexplained if u[2] == "weapon decision" and any(d[0] == "msl_target" and w == "unexplained" for d, w in u[3])]
    assert len(hits) == int(pair.flown.sum()) > 0, pair.unexplained     # in every env that launched, at its first launch


class ForcedCrash(OracleSide):
    def step(self, act):
        if self.k + 1 == FAULT_AT:
            self.vec.envs[0].set_status(0, 1)       # OR_CRASH
        return super().step(act)


def test_forced_crash_200_m_above_the_limit_is_an_unexplained_done(pkg, oracle):
    seen = {}

    def sides(cfg, ocfg, per, ix):
        # the altitude limit 250 m under the start: after 5 s of level flight the aircraft is still some 200 m and more above it
        ocfg.altitude_limit = cfg.altitude_limit = cfg.init[0].h_sl_ft * 0.3048 - 250.0
        seen["limit"] = ocfg.altitude_limit
        return ForcedCrash(oracle, ocfg, per, ix), OracleSide(oracle, ocfg, per, ix)
    pair = OpenLoopPair(pkg, oracle, 1, spread=False, task="singlecombat", sides=sides)
    act = pair.straight_action()
    for k in range(1, FAULT_AT + 1):
        m = pair.step(act)
        assert m["live"].all() == (k < FAULT_AT), (k, pair.reason)
    above = pair.parts[0][0].pose(0, 0)[2] - seen["limit"]
    assert 200.0 <= above <= 300.0, above
    assert len(pair.unexplained) == 1 and pair.unexplained[0][:2] == (0, FAULT_AT), pair.unexplained
    assert pair.unexplained[0][2][0] and not pair.unexplained[0][3][0]         # done on the faulty side, not on the reference
    assert pair.reason[0] == "done (unexplained, unexplained)"     # the crashed aircraft, and its opponent's SafeReturn after it


class FalseHit(OracleSide):
    """The first munition of env 0 is declared a hit three steps after its launch."""

    def step(self, act):
        out = super().step(act)
        env = self.vec.envs[0]
        ms = env.missiles()
        if ms and not getattr(self, "fired", False) and int(ms[0][0]) == MSL_LAUNCHED and ms[0][9] > 0.25:
            self.miss_distance = float(np.linalg.norm(ms[0][1:4] - env.pose(int(ms[0][12]))[9:12]))
            env.set_missile_status(0, MSL_HIT)
            self.fired = self.k
        return out


def test_false_hit_outside_twice_the_kill_radius_is_unexplained(pkg, oracle):
    pair = pair_of(pkg, oracle, FalseHit, "singlecombat_shoot", 1, 8, n_starts=1)
    fly(pair, random_actions("singlecombat_shoot", pair.E, pair.A, 120, 7), "planted: false hit", strict=False)
    side = pair.parts[0][0]
    assert side.miss_distance > 2 * 300.0, side.miss_distance
    mine = [u for u in pair.unexplained if u[0] == 0]
    assert len(mine) == 1 and mine[0][1] == side.fired and mine[0][2] == "weapon decision", pair.unexplained
    assert any(d[0] == "msl_status" and d[2] == MSL_HIT and d[3] == MSL_LAUNCHED and w == "unexplained" for d, w in mine[0][3]), mine
