"""The MAPPO rollout collector without a GPU: the share post-step kernel's row function (ac_share_rollout_post_step_host,
csrc/rollout_collect.hpp) against a numpy restatement, in this project's own words, of what the share runner's insert()
(runner/share_jsbsim_runner.py:196-223) followed by SharedReplayBuffer.insert (algorithms/utils/buffer.py:312-343) leave behind, bit for
bit; the new header against its ctypes mirror; the exports."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HID, ENV_ACT, BUF_ACT, T = 128, 7, 4, 3   # env.act_dim > buffer.act_dim
# (E, A, na, obs_dim): (5, 2, 1, 15) has A * obs_dim = 30, no multiple of 4 (the scalar share path); the others take the 16-byte one
SHAPES = [(1, 1, 1, 15), (5, 2, 2, 15), (5, 2, 1, 15), (3, 4, 2, 39), (3, 8, 4, 65), (3, 8, 8, 21)]
# the patterns of test_rollout_collect_host.py, and one more: with na < A, "one_agent" ends an opponent's agent, which no buffer row shows
PATTERNS = ["none", "all", "one_agent", "mixed", "one_learner_agent"]


def dones_for(pattern, E, A, rng):
    d = np.zeros((E, A, 1), dtype=bool)
    if pattern == "all":
        d[:] = True
    elif pattern == "one_agent":      # one agent of an env done: with A > 1 that is not an env-done
        d[0, A - 1] = True
    elif pattern == "one_learner_agent":
        d[0, 0] = True
    elif pattern == "mixed":          # whole envs done, others with some of their agents done
        d[:] = rng.random((E, A, 1)) < 0.5
        d[E - 1] = True
        if E > 1:
            d[0] = True
            d[0, 0] = A == 1
    return d


def share_runner_insert(buf, step, opp, obs, actions, rewards, dones, logp, values, h_a, h_c, na):
    """What one step of the share runner leaves behind, on copies of the inputs. An env counts as done when every one of its agents is
    (the opponent's included): its new GRU states (learner's and opponent's) restart from zero and its masks are 0, the others 1. An
    agent is inactive (active_masks 0) when it is done while its env goes on. share_obs of an agent is its env's whole observation
    block. Then the learner's share -- agents [0, na), the first BUF_ACT action columns -- goes into the buffer: obs, share_obs, masks,
    active_masks and states at slot step + 1; actions, rewards, values and the log-prob (the heads' sum, once per head column) at slot
    step. bad_masks is never passed on, so it stays."""
    buf = {k: v.copy() for k, v in buf.items()}
    E, A, D = obs.shape
    agent_done = dones[..., 0]                                         # [E, A]
    ended = agent_done.all(axis=1)                                     # [E]
    alive = (~ended).astype(np.float32)
    if opp is not None:
        opp = {"h": opp["h"].copy(), "masks": np.repeat(alive, A - na).reshape(-1, A - na, 1)}
        opp["h"][ended] = 0.0
    active = np.ones((E, A, 1), dtype=np.float32)
    active[agent_done & ~ended[:, None]] = 0.0
    share = np.broadcast_to(obs.reshape(E, 1, A * D), (E, A, A * D))
    new_slot = {"obs": obs[:, :na], "share_obs": share[:, :na], "masks": np.broadcast_to(alive[:, None, None], (E, na, 1)),
                "active_masks": active[:, :na],
                "rnn_states_actor": np.where(ended[:, None, None, None], np.float32(0), h_a),
                "rnn_states_critic": np.where(ended[:, None, None, None], np.float32(0), h_c)}
    this_slot = {"actions": actions[:, :na, :BUF_ACT], "rewards": rewards[:, :na], "action_log_probs": np.broadcast_to(logp, (E, na, BUF_ACT)),
                 "value_preds": values}
    for k, v in new_slot.items():
        buf[k][step + 1] = v
    for k, v in this_slot.items():
        buf[k][step] = v
    return buf, opp


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("E,A,na,D", SHAPES)
def test_row_function_matches_the_share_runners_insert(pkg, E, A, na, D, pattern):
    lib = pkg.load_library()
    capi = pkg.capi
    rng = np.random.default_rng(1000 * E + 100 * A + 10 * na + D)
    f = lambda *shape: rng.normal(0, 1, shape).astype(np.float32)
    for s in range(T):
        buf = {"obs": f(T + 1, E, na, D), "share_obs": f(T + 1, E, na, A * D), "actions": f(T, E, na, BUF_ACT), "rewards": f(T, E, na, 1),
               "masks": f(T + 1, E, na, 1), "bad_masks": f(T + 1, E, na, 1), "active_masks": f(T + 1, E, na, 1),
               "action_log_probs": f(T, E, na, BUF_ACT), "value_preds": f(T + 1, E, na, 1),
               "rnn_states_actor": f(T + 1, E, na, 1, HID), "rnn_states_critic": f(T + 1, E, na, 1, HID)}
        opp = {"h": f(E, A - na, 1, HID), "masks": f(E, A - na, 1)} if na < A else None
        obs, actions, rewards = f(E, A, D), f(E, A, ENV_ACT), f(E, A, 1)
        dones = dones_for(pattern, E, A, rng)
        # what the policy kernel has written before the post-step kernel runs: slot s of VALUES, slot s + 1 of the states, the scratch
        logp, values, h_a, h_c = f(E, na, 1), f(E, na, 1), f(E, na, 1, HID), f(E, na, 1, HID)
        want, want_opp = share_runner_insert(buf, s, opp, obs, actions, rewards, dones, logp, values, h_a, h_c, na)
        if pattern in ("one_agent", "one_learner_agent") and A > 1:   # no env-done; an active_masks 0 beside a masks 1
            assert dones.any() and not dones[..., 0].all(axis=-1).any()
            if pattern == "one_learner_agent" or na == A:
                ag = 0 if pattern == "one_learner_agent" else A - 1
                assert want["active_masks"][s + 1, 0, ag, 0] == 0.0 and want["masks"][s + 1, 0, ag, 0] == 1.0
                assert want["active_masks"][s + 1].sum() == E * na - 1
        got = {k: v.copy() for k, v in buf.items()}
        got["value_preds"][s] = values
        got["rnn_states_actor"][s + 1], got["rnn_states_critic"][s + 1] = h_a, h_c
        got_opp = {k: v.copy() for k, v in opp.items()} if opp else None
        d8 = np.ascontiguousarray(dones.astype(np.uint8))
        ptr = lambda a: a.ctypes.data
        st = capi.AcShareRolloutPostStep(E, A, na, D, ENV_ACT, BUF_ACT, HID, T, s, ptr(obs), ptr(rewards), ptr(actions), ptr(d8), ptr(logp),
                                         ptr(got["obs"]), ptr(got["share_obs"]), ptr(got["rewards"]), ptr(got["actions"]),
                                         ptr(got["action_log_probs"]), ptr(got["masks"]), ptr(got["active_masks"]),
                                         ptr(got["rnn_states_actor"]), ptr(got["rnn_states_critic"]),
                                         ptr(got_opp["h"]) if opp else None, ptr(got_opp["masks"]) if opp else None)
        assert lib.ac_share_rollout_post_step_host(C.byref(st)) == 0, lib.last_error()
        assert set(want) == set(buf)
        for k in want:     # every array bit for bit: slots s / s + 1 as insert() leaves them, every other slot untouched
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (k, s)
        assert np.array_equal(got["bad_masks"].view(np.uint32), buf["bad_masks"].view(np.uint32))
        if opp:
            for k in want_opp:
                assert np.array_equal(got_opp[k].view(np.uint32), want_opp[k].view(np.uint32)), (k, s)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("E,A,na,D", [sh for sh in SHAPES if sh[3] == 15])
def test_both_forms_write_the_common_arrays_alike(pkg, E, A, na, D, pattern):
    """The PPO form's row function (ac_rollout_post_step_host) and the share form's are one template: on the same env-side arrays and
    the same initial buffer contents, every array both forms have ends up byte for byte the same, at every slot."""
    lib = pkg.load_library()
    capi = pkg.capi
    rng = np.random.default_rng(2000 * E + 100 * A + 10 * na + D)
    f = lambda *shape: rng.normal(0, 1, shape).astype(np.float32)
    common = ("obs", "rewards", "actions", "masks", "rnn_states_actor", "rnn_states_critic")
    ptr = lambda a: a.ctypes.data
    for s in range(T):
        buf = {"obs": f(T + 1, E, na, D), "share_obs": f(T + 1, E, na, A * D), "actions": f(T, E, na, BUF_ACT), "rewards": f(T, E, na, 1),
               "masks": f(T + 1, E, na, 1), "active_masks": f(T + 1, E, na, 1), "action_log_probs": f(T, E, na, BUF_ACT),
               "rnn_states_actor": f(T + 1, E, na, 1, HID), "rnn_states_critic": f(T + 1, E, na, 1, HID)}
        opp = {"h": f(E, A - na, 1, HID), "masks": f(E, A - na, 1)} if na < A else None
        obs, actions, rewards, logp = f(E, A, D), f(E, A, ENV_ACT), f(E, A, 1), f(E, na, 1)
        d8 = np.ascontiguousarray(dones_for(pattern, E, A, rng).astype(np.uint8))
        ppo, share = ({k: v.copy() for k, v in buf.items()} for _ in range(2))
        ppo_opp, share_opp = ({k: v.copy() for k, v in opp.items()} if opp else None for _ in range(2))
        opp_ptrs = lambda o: (ptr(o["h"]), ptr(o["masks"])) if o else (None, None)
        st = capi.AcRolloutPostStep(E, A, na, D, ENV_ACT, BUF_ACT, HID, T, s, ptr(obs), ptr(rewards), ptr(actions), ptr(d8),
                                    ptr(ppo["obs"]), ptr(ppo["rewards"]), ptr(ppo["actions"]), ptr(ppo["masks"]),
                                    ptr(ppo["rnn_states_actor"]), ptr(ppo["rnn_states_critic"]), *opp_ptrs(ppo_opp))
        assert lib.ac_rollout_post_step_host(C.byref(st)) == 0, lib.last_error()
        st = capi.AcShareRolloutPostStep(E, A, na, D, ENV_ACT, BUF_ACT, HID, T, s, ptr(obs), ptr(rewards), ptr(actions), ptr(d8), ptr(logp),
                                         ptr(share["obs"]), ptr(share["share_obs"]), ptr(share["rewards"]), ptr(share["actions"]),
                                         ptr(share["action_log_probs"]), ptr(share["masks"]), ptr(share["active_masks"]),
                                         ptr(share["rnn_states_actor"]), ptr(share["rnn_states_critic"]), *opp_ptrs(share_opp))
        assert lib.ac_share_rollout_post_step_host(C.byref(st)) == 0, lib.last_error()
        for k in common:
            assert ppo[k].tobytes() == share[k].tobytes(), (k, s)
            if not k.startswith("rnn_"):                                # (and the step did write them; the states only where done)
                assert ppo[k].tobytes() != buf[k].tobytes(), (k, s)
        for k in ("share_obs", "active_masks", "action_log_probs"):     # the PPO form has no pointer to these
            assert ppo[k].tobytes() == buf[k].tobytes(), (k, s)
        if opp:
            for k in opp:
                assert ppo_opp[k].tobytes() == share_opp[k].tobytes(), (k, s)


def test_row_function_refusals(pkg):
    lib = pkg.load_library()
    PS = pkg.capi.AcShareRolloutPostStep
    a = np.zeros(4096, dtype=np.float32)
    p = a.ctypes.data
    # E, A, na, obs_dim, env_act_dim, act_dim, hidden, T, s; 14 arrays; opp_h, opp_masks
    ok = [2, 2, 2, 3, 4, 4, 8, 2, 0] + [p] * 14 + [None, None]
    assert lib.ac_share_rollout_post_step_host(C.byref(PS(*ok))) == 0
    cases = [(8, 2, "slot s"), (8, -1, "slot s"), (2, 3, "na"), (5, 5, "env_act_dim >= act_dim"), (6, 6, "multiple of 4"), (23, p, "go together"),
             (0, 0, "out of range")] + [(i, None, "null array") for i in range(9, 23)]
    for idx, val, what in cases:
        bad = list(ok)
        bad[idx] = val
        assert lib.ac_share_rollout_post_step_host(C.byref(PS(*bad))) == -1, (idx, val)
        assert what in lib.last_error(), (what, lib.last_error())
    bad = list(ok)
    bad[23] = bad[24] = p       # opponent arrays although the learner owns every agent
    assert lib.ac_share_rollout_post_step_host(C.byref(PS(*bad))) == -1 and "na = A" in lib.last_error()
    assert lib.ac_share_rollout_post_step_host(None) == -1


def test_header_and_bindings_agree(pkg, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "aircombat_rollout_share.h"\n'
                   'int main(){printf("%zu %zu", sizeof(ac_rollout_config_t), sizeof(ac_share_rollout_post_step_t));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a, b = map(int, subprocess.check_output([str(exe)], text=True).split())
    assert a == C.sizeof(pkg.capi.AcRolloutConfig) and b == C.sizeof(pkg.capi.AcShareRolloutPostStep)
    hdr = open(os.path.join(ROOT, "include", "aircombat_rollout_share.h")).read()
    declared = set(re.findall(r"^int (ac_[a-z0-9_]+)\s*\(", hdr, flags=re.M))      # (the comments name ac_last_error() too)
    assert declared == {"ac_share_rollout_create", "ac_share_rollout_destroy", "ac_share_rollout_opponent_state", "ac_share_rollout_collect",
                        "ac_share_rollout_post_step_host"}
    assert not any(d.startswith("ac_rollout_") for d in declared)
    lib = pkg.load_library()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib.path], text=True)
    for sym in declared:
        assert sym in pkg.capi.SIGNATURES and hasattr(lib, sym) and re.search(rf"\bT {sym}\b", exported), sym


def test_exports_and_null_handles(pkg):
    assert pkg.DeviceMAPPORollout.__name__ == "DeviceMAPPORollout" and "DeviceMAPPORollout" in pkg.__all__
    assert issubclass(pkg.DeviceMAPPORollout, pkg.DeviceRollout)       # the stream and view helpers are shared
    lib = pkg.load_library()
    out = C.c_void_p()
    assert lib.ac_share_rollout_create(None, None, None, None, None, C.byref(out)) == -1 and "null argument" in lib.last_error()
    assert lib.ac_share_rollout_collect(None, None, 1, 0, 0, 0, 0) == -1 and "null handle" in lib.last_error()
    assert lib.ac_share_rollout_opponent_state(None, None, None) == -1 and "null argument" in lib.last_error()
    assert lib.ac_share_rollout_destroy(None) == 0
