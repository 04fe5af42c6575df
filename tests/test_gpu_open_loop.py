"""The stated fp32 tolerance of FREE FLIGHT (north_star: "per-step state (position / attitude / velocity) and reward within a stated
fp32 tolerance ... on identical initial conditions and action sequences"): the HIP step (fp32, fp64 position) and the float64 oracle
start from the same initial conditions, take the same actions, and nothing is ever re-synchronised. The envelopes below were read off a
first run (tools/diag/open_loop.py, curves in DESIGN.md section 8) and then frozen at 4-5x what that run showed; k = env steps (0.1 s
each) since the episode began.

    position  |d NEU|        <= 0.02 m     + 15 m      (k / 600)^3
    attitude  max |d rpy|    <= 2e-4 rad   + 0.015 rad (k / 600)^2
    velocity  |d v_NED|      <= 0.01 m/s   + 0.8 m/s   (k / 600)^2
    observation entries      <= 2e-4       + 0.015     (k / 600)^2
    reward                   <= 5e-3       + 0.02      (k / 600)^2

They hold as long as both sides take the same discrete decisions (the flap switches of the flight control system on alpha / Mach /
calibrated airspeed, the turbine's phase, terminations): an aircraft whose switch flips a tick apart on the two sides has left the
regime in which a tolerance can be stated, and is dropped from the comparison from that step on (its horizon is reported)."""
import numpy as np
import pytest

from open_loop_util import RANDOM_FORM_IDS, RANDOM_FORMS, RANDOM_STEPS, OpenLoopPair, assert_random_flight_conditions, envelope, fly, random_actions

pytestmark = pytest.mark.gpu


# every kernel form a BASELINE config launches: (id, task, aircraft per side, environment that pins the form)
FORMS = [
    ("C2 three-wave", "singlecombat", 1, {"AIRCOMBAT_SPLIT": "1"}),
    ("C2 one-wave (every batch above 32 768 aircraft)", "singlecombat", 1, {"AIRCOMBAT_SPLIT": "0"}),
    ("C3 quad form: three FDM waves + environment wave", "singlecombat_shoot", 1, {"AIRCOMBAT_QUAD": "1"}),
    ("C3 pair form: one flight wave + environment wave", "singlecombat_shoot", 1, {"AIRCOMBAT_QUAD": "0"}),
    ("C4 legacy multiplecombat 2v2, three-wave", "multiplecombat", 2, {"AIRCOMBAT_SPLIT": "1"}),
    ("C4 legacy multiplecombat 2v2, one-wave", "multiplecombat", 2, {"AIRCOMBAT_SPLIT": "0"}),
    ("C4 scenario_nvn 2v2, pair form (RAW pose reduced on the environment wave)", "scenario_nvn", 2, {}),
    ("C5 scenario_nvn 4v4, pair form", "scenario_nvn", 4, {}),
]


FORM_IDS = [f[0].split(":")[0].split(" (")[0].replace(" ", "_").replace(",", "") for f in FORMS]
assert [f[:4] for f in RANDOM_FORMS[:len(FORMS)]] == [tuple(f) for f in FORMS]     # the random-action cases fly these forms, and scenario1's two


@pytest.mark.parametrize("form", FORMS + [("hierarchical C2: commands from the controller kernel", "hierarchical_singlecombat", 1, {})], ids=FORM_IDS + ["C2_hierarchical"])
def test_stored_commands_are_the_decoded_action_in_every_form(pkg, monkeypatch, form):
    """fcs/*-cmd-norm of the stored state after a step (ac_get_state: da, de, dr, thr) = normalize_action of the control indices the step
    was given (singlecombat_task.py:141-153), whichever wave of the form decodes the action row: in the three-wave and quad forms only the
    systems wave ever sees the row, and the dynamics wave -- which stores the flight state -- gets the commands with the systems wave's fields."""
    from open_loop_util import make_config, STARTS
    name, task, per_side, pins = form
    for k, v in pins.items():
        monkeypatch.setenv(k, v)
    hier = task.startswith("hierarchical")
    cfg = pkg.default_config(task, hierarchical=True) if hier else make_config(pkg, task, per_side, STARTS[0], 6)
    A, E = cfg.n_agents, 70
    cls = pkg.HipShareVecEnv if A > 2 else pkg.HipVecEnv
    env = cls(cfg, E, seed=2)
    env.reset()
    ix = {nm: k for k, nm in enumerate(env.lib.state_field_names()) if nm}
    rng = np.random.default_rng(4)
    for step in range(3):
        if hier:
            act = np.stack([rng.integers(0, n, size=(E, A)) for n in (3, 5, 3)], axis=-1).astype(np.float32)
        else:
            act = np.stack([rng.integers(0, n, size=(E, A)) for n in (41, 41, 41, 30)], axis=-1).astype(np.float32)
            if env.act_dim > 4:
                act = np.concatenate([act, np.zeros((E, A, env.act_dim - 4), dtype=np.float32)], axis=-1)
        env.step(act)
        for e in (0, 1, 33, 63, 64, 69):
            for a in range(A):
                low = env.get_controller_state(e, a)[1][:4] if hier else act[e, a, :4]
                want = [np.clip(low[0] / 20.0 - 1.0, -1, 1), np.clip(low[1] / 20.0 - 1.0, -1, 1), np.clip(low[2] / 20.0 - 1.0, -1, 1), np.clip(low[3] / 58.0 + 0.4, 0, 0.9)]
                st = env.get_state(e, a)
                got = [st[ix["da"]], st[ix["de"]], st[ix["dr"]], st[ix["thr"]]]
                assert np.allclose(got, want, atol=1e-6), (name, step, e, a, got, want)
    env.close()


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_straight_flight_600_steps_open_loop(pkg, oracle, monkeypatch, form):
    """Eight sets of initial conditions (15 000 - 30 000 ft, 600 - 1000 ft/s, every quadrant of heading), every aircraft holds the
    reference's straight-fly action [20, 19, 20, 0] (model/baseline.py:168; weapon bits 0) for 600 env steps = 60 s = 3600 FDM ticks,
    in every kernel form a BASELINE config launches: the same frozen envelope for all of them."""
    name, task, per_side, pins = form
    for k, v in pins.items():
        monkeypatch.setenv(k, v)
    pair = OpenLoopPair(pkg, oracle, 8, spread=True, task=task, per_side=per_side)   # one env per start: with a held action the envs of a handle are identical
    act = pair.straight_action()
    worst = {}
    for k in range(1, 601):
        m = pair.step(act)
        assert m["live"].all(), (k, pair.reason)           # straight and level: no switch flips, nobody terminates
        env = envelope(k)
        for key, bound in env.items():
            assert (m[key] <= bound).all(), (name, key, k, float(m[key].max()), float(bound))
            worst[key] = max(worst.get(key, 0.0), float((m[key] / bound).max()))
    print(f"straight flight [{name}], final max: pos {m['pos_m'].max():.3f} m att {m['att_rad'].max():.2e} rad vel {m['vel_ms'].max():.3f} m/s; "
          f"worst fraction of the envelope used:", {k: round(v, 3) for k, v in worst.items()})
    pair.close()


@pytest.mark.parametrize("split", ["1", "0"])
def test_straight_flight_every_tick_compared(pkg, oracle, monkeypatch, split):
    """The same flight with agent_interaction_steps = 1: an env step is ONE FDM tick, so the discrete decisions of the flight control
    system (flap switches, turbine phase, status) are compared after EVERY tick — a switch that flips a tick apart inside a 6-tick env
    step and agrees again at its end cannot hide. Four starts x 1800 ticks (30 s), BASELINE C2's kernel in both forms; the envelope is
    the 6-tick one at k = ticks / 6."""
    monkeypatch.setenv("AIRCOMBAT_SPLIT", split)
    pair = OpenLoopPair(pkg, oracle, 4, spread=True, task="singlecombat", substeps=1, n_starts=4)
    act = pair.straight_action()
    worst = {}
    for tick in range(1, 1801):
        m = pair.step(act)
        assert m["live"].all(), (tick, pair.reason)
        env = envelope(tick / 6.0)
        for key, bound in env.items():
            assert (m[key] <= bound).all(), (key, tick, float(m[key].max()), float(bound))
            worst[key] = max(worst.get(key, 0.0), float((m[key] / bound).max()))
    print(f"per-tick comparison, AIRCOMBAT_SPLIT={split}: no decision differed in {pair.E * pair.A} aircraft x 1800 ticks; worst fraction of the "
          f"envelope used:", {k: round(v, 3) for k, v in worst.items()})
    pair.close()


def test_random_actions_open_loop_until_a_switch_differs(pkg, oracle):
    """32 envs, uniform random control indices redrawn every 5 steps (violent manoeuvring: episodes end in crashes and restart),
    300 steps (tools/diag/open_loop.py runs the same at 64 envs x 600 steps: DESIGN.md section 8). Every env is compared as long as its discrete decisions agree; the envelope is the straight-flight one widened 8x
    (a manoeuvring aircraft turns a position difference into an attitude difference and back), in episode age."""
    E, STEPS = 32, 300
    pair = OpenLoopPair(pkg, oracle, E, spread=True)
    rng = np.random.default_rng(20250321)
    age = np.zeros(E, dtype=np.int64)
    worst = {}
    act = None
    for k in range(STEPS):
        if k % 5 == 0:
            act = np.stack([rng.integers(0, n, size=(E, 2)) for n in (41, 41, 41, 30)], axis=-1).astype(np.float32)
        m = pair.step(act)
        age += 1
        live = m["live"]
        env = envelope(age)
        for key, bound in env.items():
            b = 8.0 * bound[:, None]
            ok = (m[key] <= b) | ~live[:, None]
            assert ok.all(), (key, k, np.argwhere(~ok)[:4].tolist(), m[key][~ok][:4], b[np.argwhere(~ok)[:4, 0], 0], age[np.argwhere(~ok)[:4, 0]])
            worst[key] = max(worst.get(key, 0.0), float((m[key] / b)[live].max()) if live.any() else 0.0)
        age[pair.last_reset] = 0
    h = np.minimum(pair.horizon, STEPS)
    print(f"random actions: envs still comparable after {STEPS} steps {int((pair.horizon > STEPS).sum())}/{E}; horizon min {int(h.min())}, "
          f"p10 {np.percentile(h, 10):.0f}, median {np.median(h):.0f}; first differing decision: {pair.reason_counts()}; "
          f"worst fraction of the 8x envelope used: { {k: round(v, 3) for k, v in worst.items()} }")
    # a done flag that differs without an EARLIER differing decision must sit on a termination threshold (altitude limit, load
    # factor 10): anything else is a termination bug, reported with the env, the step and both done rows
    assert not pair.unexplained, pair.unexplained
    assert (pair.horizon > 100).mean() >= 0.9          # the regime with a stated tolerance is the common case, not the exception
    pair.close()


@pytest.mark.parametrize("form", RANDOM_FORMS, ids=RANDOM_FORM_IDS)
def test_random_actions_open_loop_every_form(pkg, oracle, monkeypatch, form):
    """Random actions, free flight, munitions live, in EVERY kernel form (FORMS, and scenario1 in its quad and pair form): control indices
    uniform and redrawn every 5 steps, every weapon / shoot column Bernoulli(0.05) redrawn every step, one fixed seed per form
    (open_loop_util.RANDOM_FORMS: 32 envs of 1v1, 16 of 2v2, 8 of 4v4, 300 steps = 30 s each). After every step, for the envs inside their
    horizon: the aircraft inside the 8x envelope in episode age, every munition still closing on its target inside the same envelope in
    position and velocity against its twin (matched by parent and flight time; from its first receding step on only its discrete facts
    are compared: at a near miss the pass turns a millimetre of target difference into decimetres), and no done flag and no weapon decision
    (remaining rounds, shoot bookkeeping, scenario counters, a munition's status, target and model, the number in flight) that differs
    without a threshold to explain it (OpenLoopPair.near_a_threshold). At the end, conditions: nine envs in ten comparable past step 100; in
    the forms with weapon columns a munition flew in at least half of the envs and at least one ended inside an env's horizon. The fp32
    twin meets all of them with these inputs (tests/test_open_loop_twin.py), and the seeds were chosen there.

    Left out: the *_dodge_missile tasks (their rule-based launch never fires from STARTS under random actions, 0/32 in the twin: they stay
    with the teacher-forced tests) and the hierarchical forms (a controller argmax flip is a decision of its own kind and wants a test of
    its own)."""
    name, task, per_side, pins, E, seed = form
    for k, v in pins.items():
        monkeypatch.setenv(k, v)
    pair = OpenLoopPair(pkg, oracle, E, spread=True, task=task, per_side=per_side)
    fly(pair, random_actions(task, pair.E, pair.A, RANDOM_STEPS, seed), name)
    assert_random_flight_conditions(pair, task, RANDOM_STEPS)
    pair.close()
