"""The rollout collector without a GPU: the post-step kernel's row function (ac_rollout_post_step_host, csrc/rollout_collect.hpp) against
a numpy restatement, in this project's own words, of what the two runners' insert() (runner/jsbsim_runner.py:122-133,
runner/selfplay_jsbsim_runner.py:103-124) followed by ReplayBuffer.insert (algorithms/utils/buffer.py:77-111) leave behind, bit for bit; the new header against its ctypes mirror; the exports."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HID, OBS_DIM, ENV_ACT, BUF_ACT, T = 128, 15, 7, 4, 3   # env.act_dim > buffer.act_dim
SHAPES = [(1, 1, 1), (5, 2, 2), (5, 2, 1), (3, 4, 2), (3, 8, 4)]
PATTERNS = ["none", "all", "one_agent", "mixed"]


def dones_for(pattern, E, A, rng):
    d = np.zeros((E, A, 1), dtype=bool)
    if pattern == "all":
        d[:] = True
    elif pattern == "one_agent":      # one agent of an env done: with A > 1 that is not an env-done
        d[0, A - 1] = True
    elif pattern == "mixed":          # whole envs done, others with some of their agents done
        d[:] = rng.random((E, A, 1)) < 0.5
        d[E - 1] = True
        if E > 1:
            d[0] = True
            d[0, 0] = A == 1
    return d


def runner_insert(buf, step, opp, obs, actions, rewards, dones, logp, values, h_a, h_c, na):
    """What one step of the two runners leaves behind, on copies of the inputs: an env counts as done when every one of its agents is
    (the opponent's included); the new GRU states of a done env (learner's and opponent's) restart from zero and its masks are 0, the
    others 1; then the learner's share -- agents [0, na), the first BUF_ACT action columns -- goes into the buffer: observations,
    masks and states at slot step + 1, actions, rewards, log-probs and values at slot step. bad_masks is not given, so it stays.
    ``actions`` is the env's action row (all agents, the env's width); log-probs, values and states are what the policy produced for
    the learner. The runner without self-play is na == A: there is no opponent share."""
    buf = {k: v.copy() for k, v in buf.items()}
    ended = dones[..., 0].all(axis=1)                                  # [E]
    alive = (~ended).astype(np.float32)
    if opp is not None:
        A = dones.shape[1]
        opp = {"h": opp["h"].copy(), "masks": np.repeat(alive, A - na).reshape(-1, A - na, 1)}
        opp["h"][ended] = 0.0
    new_slot = {"obs": obs[:, :na], "masks": np.broadcast_to(alive[:, None, None], (len(alive), na, 1)),
                "rnn_states_actor": np.where(ended[:, None, None, None], np.float32(0), h_a),
                "rnn_states_critic": np.where(ended[:, None, None, None], np.float32(0), h_c)}
    this_slot = {"actions": actions[:, :na, :BUF_ACT], "rewards": rewards[:, :na], "action_log_probs": logp, "value_preds": values}
    for k, v in new_slot.items():
        buf[k][step + 1] = v
    for k, v in this_slot.items():
        buf[k][step] = v
    return buf, opp


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("E,A,na", SHAPES)
def test_row_function_matches_the_runners_insert(pkg, E, A, na, pattern):
    lib = pkg.load_library()
    capi = pkg.capi
    rng = np.random.default_rng(1000 * E + 10 * A + na)
    f = lambda *shape: rng.normal(0, 1, shape).astype(np.float32)
    for s in range(T):
        buf = {"obs": f(T + 1, E, na, OBS_DIM), "actions": f(T, E, na, BUF_ACT), "rewards": f(T, E, na, 1), "masks": f(T + 1, E, na, 1),
               "bad_masks": f(T + 1, E, na, 1), "action_log_probs": f(T, E, na, 1), "value_preds": f(T + 1, E, na, 1),
               "rnn_states_actor": f(T + 1, E, na, 1, HID), "rnn_states_critic": f(T + 1, E, na, 1, HID)}
        opp = {"h": f(E, A - na, 1, HID), "masks": f(E, A - na, 1)} if na < A else None
        obs, actions, rewards = f(E, A, OBS_DIM), f(E, A, ENV_ACT), f(E, A, 1)
        dones = dones_for(pattern, E, A, rng)
        if pattern == "one_agent" and A > 1:
            assert dones.any() and not np.all(dones[..., 0], axis=-1).any()
        # what the policy kernel has written before the post-step kernel runs: slot s of LOGP / VALUES, slot s + 1 of the states
        logp, values, h_a, h_c = f(E, na, 1), f(E, na, 1), f(E, na, 1, HID), f(E, na, 1, HID)
        want, want_opp = runner_insert(buf, s, opp, obs, actions, rewards, dones, logp, values, h_a, h_c, na)
        got = {k: v.copy() for k, v in buf.items()}
        got["action_log_probs"][s], got["value_preds"][s] = logp, values
        got["rnn_states_actor"][s + 1], got["rnn_states_critic"][s + 1] = h_a, h_c
        got_opp = {k: v.copy() for k, v in opp.items()} if opp else None
        d8 = np.ascontiguousarray(dones.astype(np.uint8))
        ptr = lambda a: a.ctypes.data
        st = capi.AcRolloutPostStep(E, A, na, OBS_DIM, ENV_ACT, BUF_ACT, HID, T, s, ptr(obs), ptr(rewards), ptr(actions), ptr(d8),
                                    ptr(got["obs"]), ptr(got["rewards"]), ptr(got["actions"]), ptr(got["masks"]),
                                    ptr(got["rnn_states_actor"]), ptr(got["rnn_states_critic"]),
                                    ptr(got_opp["h"]) if opp else None, ptr(got_opp["masks"]) if opp else None)
        assert lib.ac_rollout_post_step_host(C.byref(st)) == 0, lib.last_error()
        for k in want:     # every array bit for bit: slots s / s + 1 as insert() leaves them, every other slot untouched
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (k, s)
        assert np.array_equal(got["bad_masks"], buf["bad_masks"])
        if opp:
            for k in want_opp:
                assert np.array_equal(got_opp[k].view(np.uint32), want_opp[k].view(np.uint32)), (k, s)


def test_row_function_refusals(pkg):
    lib = pkg.load_library()
    a = np.zeros(4096, dtype=np.float32)
    p = a.ctypes.data
    ok = [2, 2, 2, 3, 4, 4, 8, 2, 0] + [p] * 10 + [None, None]
    assert lib.ac_rollout_post_step_host(C.byref(pkg.capi.AcRolloutPostStep(*ok))) == 0
    for idx, val, what in ((8, 2, "slot s"), (8, -1, "slot s"), (2, 3, "na"), (5, 5, "env_act_dim >= act_dim"), (6, 6, "multiple of 4"),
                           (9, None, "null array"), (19, p, "go together"), (0, 0, "out of range")):
        bad = list(ok)
        bad[idx] = val
        assert lib.ac_rollout_post_step_host(C.byref(pkg.capi.AcRolloutPostStep(*bad))) == -1
        assert what in lib.last_error(), (what, lib.last_error())
    bad = list(ok)
    bad[19] = bad[20] = p       # opponent arrays although the learner owns every agent
    assert lib.ac_rollout_post_step_host(C.byref(pkg.capi.AcRolloutPostStep(*bad))) == -1 and "na = A" in lib.last_error()
    assert lib.ac_rollout_post_step_host(None) == -1


def test_header_and_bindings_agree(pkg, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "aircombat_rollout.h"\n'
                   'int main(){printf("%zu %zu", sizeof(ac_rollout_config_t), sizeof(ac_rollout_post_step_t));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a, b = map(int, subprocess.check_output([str(exe)], text=True).split())
    assert a == C.sizeof(pkg.capi.AcRolloutConfig) == 16 and b == C.sizeof(pkg.capi.AcRolloutPostStep)
    hdr = open(os.path.join(ROOT, "include", "aircombat_rollout.h")).read()
    declared = set(re.findall(r"\b(ac_rollout_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"ac_rollout_create", "ac_rollout_destroy", "ac_rollout_opponent_state", "ac_rollout_collect", "ac_rollout_post_step_host"}
    lib = pkg.load_library()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib.path], text=True)
    for sym in declared:
        assert sym in pkg.capi.SIGNATURES and hasattr(lib, sym) and re.search(rf"\bT {sym}\b", exported), sym
    assert (pkg.capi.AC_ROLLOUT_NO_OPPONENT, pkg.capi.AC_ROLLOUT_OPPONENT_POLICY, pkg.capi.AC_ROLLOUT_OPPONENT_POOL) == (0, 1, 2)


def test_exports_and_null_handles(pkg):
    assert pkg.DeviceRollout.__name__ == "DeviceRollout" and "DeviceRollout" in pkg.__all__
    lib = pkg.load_library()
    out = C.c_void_p()
    assert lib.ac_rollout_create(None, None, None, None, None, C.byref(out)) == -1 and "null argument" in lib.last_error()
    assert lib.ac_rollout_collect(None, None, 1, 0, 0, 0, 0) == -1 and "null handle" in lib.last_error()
    assert lib.ac_rollout_opponent_state(None, None, None) == -1
    assert lib.ac_rollout_destroy(None) == 0
