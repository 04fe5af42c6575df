"""Evaluation episodes of the reference's runners queued on the device, with a per-env episode log (include/aircombat_eval.h).

``DeviceEvaluator`` ties a ``HipVecEnv`` / ``HipShareVecEnv``, a ``DevicePolicy`` or ``DeviceMAPPOPolicy`` (only the actor is used) and,
for self-play, an actor-only policy of the same form or a ``DevicePolicyPool`` together. ``run(n)`` queues n steps of the runners'
``eval()`` loop -- runner/jsbsim_runner.py:136-172, runner/selfplay_jsbsim_runner.py:127-239, runner/share_jsbsim_runner.py:226-300 --
from C++ and returns without waiting: per step the learner's launch, the opponent's launch, the env's step kernel(s) and one post-step
kernel that does the loops' numpy bookkeeping (csrc/eval_collect.hpp): ``dones_env``, the cumulative rewards, the returns of the
episodes that ended, zeroed GRU rows and masks. GRU states, masks, running sums and the log stay in HBM; the results are bit for bit
those of the stepwise loop of INTEGRATION.md §5d / §5e on the same handles.

Every env logs its first ``episodes_per_env`` episodes. With a pool as the opponent, one pass evaluates against every assigned member
at once (``pool.assign_split``), and ``EvalResult.per_opponent`` with ``elo_update`` restate selfplay_jsbsim_runner.py:203-227.

ACMI recordings of evaluation episodes: attach a flight recorder to the env (``envs.record``, recorder.py) before the reset, and
``episode_frames`` / ``write_episode_acmi`` turn a logged episode into its frames or its Tacview file once the evaluation has ended.

Out of scope: ``MultiDeviceVecEnv`` (one evaluator per device), graph capture and the per-step ``infos`` history.
"""
import collections
import ctypes as C

import numpy as np

from .capi import AcEvalConfig, AcEvalState
from .policy import DevicePolicyPool, HID
from .rollout import device_view, opponent_kind, stream_of

_U64 = 2 ** 64 - 1

Episodes = collections.namedtuple("Episodes", "returns lengths end_steps envs")


class EvalResult:
    """Numpy copies of an evaluator's log: ``returns [E, K, A]`` float32 (every agent's episode return, the opponent's included),
    ``lengths [E, K]``, ``end_steps [E, K]`` (the evaluator's step index of the step that ended the episode), ``counts [E]`` (episodes
    finished, those beyond K included), ``members [E]`` (the pool's assignment, or zeros), ``steps`` (steps run since ``begin``) and
    ``num_learner_agents``. Slot k of env e is valid where ``k < min(counts[e], K)``."""

    def __init__(self, returns, lengths, end_steps, counts, members, steps, num_learner_agents):
        self.returns = np.asarray(returns, dtype=np.float32)
        self.lengths, self.end_steps = np.asarray(lengths, dtype=np.int32), np.asarray(end_steps, dtype=np.int32)
        self.counts, self.members = np.asarray(counts, dtype=np.int32), np.asarray(members, dtype=np.int32)
        self.steps, self.num_learner_agents = int(steps), int(num_learner_agents)
        E, K, A = self.returns.shape
        if self.lengths.shape != (E, K) or self.end_steps.shape != (E, K) or self.counts.shape != (E,) or self.members.shape != (E,):
            raise ValueError("EvalResult: returns [E, K, A], lengths / end_steps [E, K], counts / members [E] disagree")
        if not 1 <= self.num_learner_agents <= A:
            raise ValueError("EvalResult: num_learner_agents must be in 1 .. A")

    @property
    def logged(self):
        """bool [E, K]: the log slots that hold an episode"""
        K = self.returns.shape[1]
        return np.arange(K)[None, :] < np.minimum(self.counts, K)[:, None]

    def episodes(self, n=None):
        """The finished episodes in the order in which the reference's loops concatenate them: by the step at which they ended, then
        by env index. Returns ``Episodes(returns [n, A], lengths [n], end_steps [n], envs [n])``; with ``n``, the first n.

        The reference stops at the first ``eval_episodes`` episodes to finish over all envs, which favours short episodes: an env whose
        episodes are short contributes more of them. A fixed quota per env (``episodes_per_env``, all of ``episodes()``) is the
        unbiased form, and the one to prefer. The first n are the reference's only while no env has run out of log slots: with ``n``
        this raises ``ValueError`` when an env's log was full, and the env went on to finish episodes that were not logged, before the
        n-th episode ended, since one of those may belong among the first n."""
        e_idx, k_idx = np.nonzero(self.logged)
        order = np.lexsort((e_idx, self.end_steps[e_idx, k_idx]))
        e_idx, k_idx = e_idx[order], k_idx[order]
        if n is not None:
            n = int(n)
            if not 0 <= n <= len(e_idx):
                raise ValueError(f"episodes: {n} asked for, {len(e_idx)} logged")
            if n > 0:
                K = self.returns.shape[1]
                last = int(self.end_steps[e_idx[n - 1], k_idx[n - 1]])
                early = np.nonzero((self.counts > K) & (self.end_steps[:, K - 1] < last))[0]
                if early.size:
                    raise ValueError(f"episodes: env {int(early[0])} filled its {K} log slots at step {int(self.end_steps[early[0], K - 1])} and "
                                     f"finished further episodes; episode {n} ended at step {last}, so the first {n} to finish cannot be told "
                                     "from the log (raise episodes_per_env, or use the per-env quota)")
            e_idx, k_idx = e_idx[:n], k_idx[:n]
        return Episodes(self.returns[e_idx, k_idx], self.lengths[e_idx, k_idx], self.end_steps[e_idx, k_idx], e_idx.astype(np.int32))

    def per_opponent(self):
        """Per pool member present in ``members``: its logged episode count and the learner's and the opponent's average episode
        reward, as selfplay_jsbsim_runner.py:203-209 computes them with one split per member. An episode's reward is the float32 mean
        over the side's agents; the average over the member's logged episodes is taken in float64. Returns a dict of arrays, one entry
        per member in ascending order: ``members``, ``episodes``, ``learner``, ``opponent`` (NaN where a member has no logged
        episode, and for ``opponent`` when the learner owns every agent)."""
        na, A = self.num_learner_agents, self.returns.shape[2]
        ids = np.unique(self.members)
        logged = self.logged
        out = {"members": ids.astype(np.int32), "episodes": np.zeros(len(ids), dtype=np.int64),
               "learner": np.full(len(ids), np.nan), "opponent": np.full(len(ids), np.nan)}
        for i, m in enumerate(ids):
            sel = logged & (self.members == m)[:, None]
            eps = self.returns[sel]                                   # [episodes, A]
            out["episodes"][i] = len(eps)
            if len(eps):
                out["learner"][i] = eps[:, :na].mean(axis=-1).astype(np.float64).mean()
                if na < A:
                    out["opponent"][i] = eps[:, na:].mean(axis=-1).astype(np.float64).mean()
        return out


def elo_update(latest_elo, opponent_elos, learner_avg, opponent_avg, k=32.0, threshold=100.0):
    """The Elo update of selfplay_jsbsim_runner.py:212-227 for per-opponent vectors. Each opponent's actual score comes from
    ``opponent_avg - learner_avg``: 1 above ``threshold``, 0.5 strictly inside (-threshold, threshold) and 0 otherwise (the reference's
    open interval: a difference of exactly +threshold or -threshold scores 0). The gain ``k * (actual - expected)`` is added to the
    opponent's Elo and subtracted from the learner's, and the new ``latest_elo`` is the mean over opponents. Returns
    (latest_elo, opponent_elos). Vectors of different lengths and averages that are not finite are refused: ``per_opponent`` gives
    NaN for a member without a logged episode, which must not be scored as a loss; leave such a member out."""
    ratings = np.asarray(opponent_elos, dtype=np.float64)
    margin = np.asarray(opponent_avg, dtype=np.float64) - np.asarray(learner_avg, dtype=np.float64)
    if ratings.ndim != 1 or margin.shape != ratings.shape:
        raise ValueError("elo_update: opponent_elos, learner_avg and opponent_avg must be vectors with one entry per opponent")
    if not np.isfinite(margin).all():
        raise ValueError(f"elo_update: the average episode reward of opponent {int(np.nonzero(~np.isfinite(margin))[0][0])} is not finite "
                         "(a member with no logged episode?)")
    expected = 1.0 / (1.0 + np.power(10.0, (ratings - float(latest_elo)) / 400.0))
    actual = np.where(margin > threshold, 1.0, np.where(np.abs(margin) < threshold, 0.5, 0.0))
    gain = k * (actual - expected)
    return float(np.mean(float(latest_elo) - gain)), ratings + gain


class DeviceEvaluator:
    """``DeviceEvaluator(envs, policy, opponent=None, num_learner_agents=None, episodes_per_env=1)``: the learner ``policy`` (a
    ``DevicePolicy`` or ``DeviceMAPPOPolicy``, with or without a critic) owns agents ``[0, num_learner_agents)`` of every env
    (default: all of them without an opponent, the first half with one); ``opponent`` (an actor-only policy of the same form, or a
    ``DevicePolicyPool`` of that form with an assignment for the env's E) acts for the others. Both act in their mode unless
    ``deterministic`` / ``opponent_deterministic`` is False. Reset the env, then ``begin()`` and ``run(n)``, or ``evaluate(max_steps)``.
    The handles must stay open while the evaluator is. A refusal (sizes, devices or forms that do not fit, ``run`` before ``begin``)
    raises ``ValueError`` and changes nothing."""

    _VIEWS = {"states": ("lrn_h", "<f4"), "masks": ("lrn_masks", "<f4"), "opponent_states": ("opp_h", "<f4"), "opponent_masks": ("opp_masks", "<f4"),
              "cum": ("cum", "<f4"), "lengths": ("len", "<i4"), "counts": ("count", "<i4"), "log_returns": ("log_ret", "<f4"),
              "log_lengths": ("log_len", "<i4"), "log_end_steps": ("log_end", "<i4"), "remaining": ("remaining", "<i4")}

    def __init__(self, envs, policy, opponent=None, num_learner_agents=None, episodes_per_env=1, deterministic=True, opponent_deterministic=True):
        self.lib = envs.lib
        self.envs, self.policy, self.opponent = envs, policy, opponent
        kind, self.num_learner_agents = opponent_kind(opponent, num_learner_agents, envs.num_agents,
                                                      "a DevicePolicy / DeviceMAPPOPolicy (critic=False) or a DevicePolicyPool")
        self.episodes_per_env = int(episodes_per_env)
        self.device_id = int(policy.device_id)
        cfg = AcEvalConfig(self.num_learner_agents, kind, int(bool(deterministic)), int(bool(opponent_deterministic)), self.episodes_per_env)
        h = C.c_void_p()
        self._h = None
        if self.lib.ac_eval_create(envs._h, policy._h, None if opponent is None else opponent._h, C.byref(cfg), C.byref(h)) != 0:
            raise ValueError(self.lib.last_error())
        self._h = h
        self._last_stream = None

    def close(self):
        if getattr(self, "_h", None):
            self.lib.ac_eval_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _state(self):
        st = AcEvalState()
        self.lib.check(self.lib.ac_eval_state(self._h, C.byref(st)), "ac_eval_state")
        return st

    @property
    def steps(self):
        """steps queued since ``begin`` (-1 before the first ``begin``)"""
        return int(self._state().step)

    def view(self, name):
        """torch view of one of the evaluator's device arrays (it owns them; read them on the stream ``run`` was given, or after a
        synchronize): ``states`` [E * na, 1, 128], ``masks`` [E * na, 1], ``opponent_states`` / ``opponent_masks`` (None without an
        opponent), ``cum`` [E, A], ``lengths`` [E], ``counts`` [E], ``log_returns`` [E, K, A], ``log_lengths`` / ``log_end_steps``
        [E, K], ``remaining`` [1]."""
        field, typestr = self._VIEWS[name]
        st = self._state()
        E, A, na, K = st.E, st.A, st.na, st.K
        shape = {"states": (E * na, 1, HID), "masks": (E * na, 1), "opponent_states": (E * (A - na), 1, HID), "opponent_masks": (E * (A - na), 1),
                 "cum": (E, A), "lengths": (E,), "counts": (E,), "log_returns": (E, K, A), "log_lengths": (E, K), "log_end_steps": (E, K),
                 "remaining": (1,)}[name]
        ptr = getattr(st, field)
        return None if not ptr else device_view(ptr, shape, self.device_id, typestr)

    def begin(self, stream=None):
        """Queue the start of an evaluation: GRU states zero, masks one, running sums and the log cleared, every env with its whole
        quota to go. The env is not reset: reset it first, as the reference does before evaluating."""
        tstream, raw = stream_of(self.device_id, stream)
        if self.lib.ac_eval_begin(self._h, raw) != 0:
            raise ValueError(self.lib.last_error())
        self._last_stream = tstream
        rec = getattr(self.envs, "recorder", None)
        self._rec, self._rec_c0 = rec, (rec.count if rec is not None else None)   # step t of this evaluation is recorder frame c0 + t

    def run(self, n_steps, stream=None):
        """Queue ``n_steps`` evaluation steps and return without waiting. ``stream`` (a ``torch.cuda.Stream``, a raw ``hipStream_t``
        value; default torch's current stream) is ordered around the steps (include/aircombat_eval.h): every launch goes to the env's
        stream, which waits at entry for the work already queued on ``stream``, and ``stream`` waits at exit for the last kernel, with
        nothing waited for per step or on the host. What the steps read must have been queued on it (or be complete) before the call,
        and work queued on it afterwards sees their results. Step t
        draws with ``policy.counter + t`` (the opponent with its own); both counters advance by ``n_steps``. Returns ``n_steps``.
        Should the runtime refuse a launch part of the way, the counters advance by the steps that were queued before the error is
        raised."""
        n_steps = int(n_steps)
        tstream, raw = stream_of(self.device_id, stream)
        opp = self.opponent
        before = self.steps
        rc = self.lib.ac_eval_run(self._h, raw, n_steps, C.c_uint64(self.policy.seed & _U64), C.c_uint64(self.policy.counter & _U64),
                                  C.c_uint64((opp.seed if opp is not None else 0) & _U64),
                                  C.c_uint64((opp.counter if opp is not None else 0) & _U64))
        done = n_steps if rc == 0 else self.steps - before
        self.policy.counter += done
        if opp is not None:
            opp.counter += done
        if done:
            self._last_stream = tstream
        if rc != 0:
            raise ValueError(self.lib.last_error())
        return n_steps

    def remaining(self, stream=None):
        """The number of envs that have not finished ``episodes_per_env`` episodes yet: one 4-byte read that waits for ``stream``
        (default: the stream of the last ``begin`` / ``run``)."""
        import torch
        s = stream_of(self.device_id, stream)[0] if stream is not None else (self._last_stream or stream_of(self.device_id, None)[0])
        with torch.cuda.stream(s):
            return int(self.view("remaining").item())

    def evaluate(self, max_steps, chunk=64, stream=None):
        """``begin()``, then ``run(chunk)`` and one read of ``remaining`` in turn (the only host wait, once per chunk) until every env
        has finished its quota or ``max_steps`` steps have run. Returns the ``EvalResult``."""
        max_steps, chunk = int(max_steps), int(chunk)
        if max_steps < 1 or chunk < 1:
            raise ValueError("evaluate: max_steps and chunk must be at least 1")
        self.begin(stream)
        steps = 0
        while steps < max_steps:
            steps += self.run(min(chunk, max_steps - steps), stream)
            if self.remaining() == 0:
                break
        return self.result()

    def episode_frames(self, env, k):
        """(first, last): the recorder frames of the k-th logged episode of env ``env``, for ``FlightRecorder.frames`` / ``write_acmi``.
        Step t of the evaluation (counted from ``begin()``) is frame ``c0 + t`` of the recorder that was attached to the env at
        ``begin()``, ``c0`` its count then. An episode of length L whose last step was ``t_end`` is frames ``c0 + t_end - L`` ..
        ``c0 + t_end - 1``: the first of them shows the reset state (the captured ``reset()``, or the step that ended the previous
        episode and auto-reset the env), the last the state before the step that ended it; the frame of step ``t_end`` itself already
        shows the next episode, as ``render()`` does after an auto-reset. Raises ``ValueError`` where no recorder was attached at
        ``begin()``, the slot holds no episode, the episode started before recording did, or its frames have left the ring."""
        from .recorder import check_span
        rec, c0 = getattr(self, "_rec", None), getattr(self, "_rec_c0", None)
        if rec is None or rec._h is None:
            raise ValueError("episode_frames: no flight recorder was attached to the env at begin() (envs.record)")
        res = self.result()
        env, k = int(env), int(k)
        if not (0 <= env < res.lengths.shape[0] and 0 <= k < res.lengths.shape[1] and res.logged[env, k]):
            raise ValueError(f"episode_frames: env {env} has no logged episode {k}")
        if env not in rec.envs:
            raise ValueError(f"episode_frames: env {env} is not among the recorded envs")
        L, t_end = int(res.lengths[env, k]), int(res.end_steps[env, k])
        first, last = c0 + t_end - L, c0 + t_end - 1
        if first < 0:
            raise ValueError(f"episode_frames: episode {k} of env {env} started before recording did (record before the reset)")
        check_span(rec.count, rec.capacity, first, last)
        return first, last

    def write_episode_acmi(self, path, env, k):
        """Write the k-th logged episode of env ``env`` as a Tacview ACMI file (``FlightRecorder.write_acmi`` over ``episode_frames``).
        Returns the number of frames written, the episode's length."""
        first, last = self.episode_frames(env, k)
        return self._rec.write_acmi(path, env, first, last)

    def result(self):
        """The log so far as an ``EvalResult`` (waits for the stream of the last ``begin`` / ``run``)."""
        import torch
        s = self._last_stream or stream_of(self.device_id, None)[0]
        with torch.cuda.stream(s):
            got = [self.view(k).cpu().numpy() for k in ("log_returns", "log_lengths", "log_end_steps", "counts")]
            opp = self.opponent
            if isinstance(opp, DevicePolicyPool) and opp._members is not None:
                members = opp._members.cpu().numpy()
            else:
                members = np.zeros(self.envs.num_envs, dtype=np.int32)
        return EvalResult(*got, members, self.steps, self.num_learner_agents)
