"""Twins and helpers for the spawn-curriculum tests (test_spawn_host.py, test_gpu_spawn.py): a numpy float32 restatement of the
per-env rule of include/aircombat_spawn.h (steps 1-4), written from the header's text, with its own Python-integer copy of the keyed
generator, and the few lines the GPU tests share."""
import ctypes as C

import numpy as np

M64 = (1 << 64) - 1
FIELDS = ("stage", "spawned", "episode", "ret_acc", "wins", "played", "return_sum")


def _mix(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def uniform(seed, counter, row, head=0):
    """policy_uniform in Python integers: a float32 on [0, 1) in steps of 2^-24"""
    z = _mix((seed * 0x9E3779B97F4A7C15 + 0x6A09E667F3BCC909) & M64)
    z = _mix(z ^ ((counter * 0xD1B54A32D192ED03) & M64))
    z = _mix(z ^ ((((row << 8) & M64) | (head & 0xFF))))
    return np.float32(z >> 40) * np.float32(1.0 / 16777216.0)


def draw(seed, env, episode, stage):
    """the sample='upto' index of (seed, env, episode) for a clamped stage"""
    k = int(np.float32(uniform(seed, episode, env)) * np.float32(stage + 1))
    return min(k, stage)


class Twin:
    """The rule on numpy arrays, env by env in float32 / int32."""

    def __init__(self, E, K, n_ego, mode="fixed", sample="at", window=20, min_wins=18, win_return=0.0, seed=0):
        self.E, self.K, self.n_ego = E, K, n_ego
        self.auto, self.upto, self.window, self.min_wins, self.win_return, self.seed = mode == "auto", sample == "upto", window, min_wins, np.float32(win_return), seed
        self.stage, self.spawned, self.episode = np.zeros(E, np.int32), np.full(E, -1, np.int32), np.zeros(E, np.int32)
        self.wins, self.played = np.zeros(E, np.int32), np.zeros(E, np.int32)
        self.ret_acc, self.return_sum = np.zeros(E, np.float32), np.zeros(E, np.float32)

    def arrays(self):
        return {k: getattr(self, k) for k in FIELDS}

    def step(self, rewards, info, all_envs=False):
        """one step's outputs (rewards [E, A(, 1)], info [E, 4]) -> index [E]: the entry each env respawns from, -1 where it does not"""
        rewards = None if all_envs else np.asarray(rewards, dtype=np.float32).reshape(self.E, -1)
        index = np.full(self.E, -1, np.int32)
        mask = (1 << self.window) - 1
        for e in range(self.E):
            if not all_envs:
                s = rewards[e, 0]
                for j in range(1, self.n_ego):
                    s = np.float32(s + rewards[e, j])
                self.ret_acc[e] = np.float32(self.ret_acc[e] + np.float32(s / np.float32(self.n_ego)))
                if not info[e][3]:
                    continue
                self.played[e] += 1
                self.return_sum[e] = np.float32(self.return_sum[e] + self.ret_acc[e])
                w = ((int(self.wins[e]) & 0xFFFFFFFF) << 1 | int(self.ret_acc[e] >= self.win_return)) & 0xFFFFFFFF
                self.wins[e] = np.uint32(w).astype(np.int32)
            self.ret_acc[e] = 0
            if self.auto and self.played[e] >= self.window and bin(int(self.wins[e]) & mask).count("1") >= self.min_wins:
                self.stage[e] = min(int(self.stage[e]) + 1, self.K - 1)
                self.played[e], self.wins[e], self.return_sum[e] = 0, 0, 0
            self.episode[e] += 1
            s = min(max(int(self.stage[e]), 0), self.K - 1)
            self.spawned[e] = draw(self.seed, e, int(self.episode[e]), s) if self.upto else s
            index[e] = self.spawned[e]
        return index


def spawn_cfg(pkg, mode="fixed", sample="at", window=20, min_wins=18, win_return=0.0, seed=0):
    c = pkg.capi.AcSpawnConfig()
    c.mode, c.sample = {"fixed": 0, "auto": 1}[mode], {"at": 0, "upto": 1}[sample]
    c.window, c.min_wins, c.win_return, c.seed = window, min_wins, win_return, seed
    return c


def host_step(pkg, cfg, K, n_ego, rewards, info, arrays, all_envs=False):
    """ac_spawn_post_step_host on `arrays` (a dict of the seven per-env numpy arrays, changed in place) -> index [E]"""
    lib = pkg.load_library()
    E = len(arrays["stage"])
    p = pkg.capi.AcSpawnPostStep()
    rewards = np.ascontiguousarray(rewards, dtype=np.float32).reshape(E, -1)
    info = np.ascontiguousarray(info, dtype=np.int32)
    p.E, p.A, p.n_ego, p.K, p.all_envs, p.cfg = E, rewards.shape[1], n_ego, K, int(all_envs), cfg
    p.rewards, p.info = rewards.ctypes.data, info.ctypes.data
    for k in FIELDS:
        assert arrays[k].flags.c_contiguous and arrays[k].itemsize == 4
        setattr(p, k, arrays[k].ctypes.data)
    index = np.full(E, -7, np.int32)
    p.index = index.ctypes.data
    assert lib.ac_spawn_post_step_host(C.byref(p)) == 0, lib.last_error()
    return index


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[x.itemsize]) if x.dtype.kind in "fb" else x


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def random_actions(rng, E, A, act_dim):
    """control indices [41, 41, 41, 30] and, where the task has them, weapon bits"""
    act = np.zeros((E, A, act_dim), dtype=np.float32)
    for k, n in enumerate((41, 41, 41, 30)):
        act[..., k] = rng.integers(0, n, size=(E, A))
    if act_dim > 4:
        act[..., 4:] = rng.integers(0, 2, size=(E, A, act_dim - 4))
    return act
