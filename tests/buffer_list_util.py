"""What the list-form buffer tests share (tests/test_buffer_list_host.py, tests/test_gpu_buffer_list.py,
tests/golden/make_buffer_list_golden.py): the cases, the hash that fills the buffers, and the numpy restatement of what the
reference's ``ReplayBuffer.recurrent_generator([b0, ...])`` yields (algorithms/utils/buffer.py:183-268): the buffers' sequence views
stacked in the list's order, one chunk order over the stack.

Nothing here reads the reference tree or the GPU."""
import types

import numpy as np

# The golden's cases. Stack rows = K * T * threads * A; the generator counts threads * (T * K) // L chunks (the agent axis is not counted).
#   a: 90 rows, T * N = 30 and L = 4: chunk 7 is rows 28 .. 31, two of buffer 0 and two of buffer 1; 22 chunks, 2 mini-batches of 11.
#      Widths 5, 2 and 3: no field may take the 16-byte path.
#   b: 140 rows, T = 7 and L = 3: chunks straddle columns; 23 chunks, 3 mini-batches of 7, two chunks dropped. Widths 8, 4 and 8: the
#      16-byte path; two agents per thread.
CASES = {
    "a": dict(K=3, T=10, E=3, A=1, L=4, n_mb=2, obs=5, act=2, hidden=3, seed=101),
    "b": dict(K=2, T=7, E=5, A=2, L=3, n_mb=3, obs=8, act=4, hidden=8, seed=202),
}
GAMMA, LAMBDA = 0.99, 0.95
NAMES = ("obs", "actions", "masks", "action_log_probs", "advantages", "returns", "value_preds", "rnn_states_actor", "rnn_states_critic")
SHARED_NAMES = ("obs", "share_obs", "actions", "masks", "active_masks", "action_log_probs", "advantages", "returns", "value_preds",
                "rnn_states_actor", "rnn_states_critic")


def args_of(case, T=None, E=None, hidden=None):
    """The constructor's ``args`` of every buffer class (the reference's, the oracle has its own signature, the device's)."""
    return types.SimpleNamespace(buffer_size=case["T"] if T is None else T, n_rollout_threads=case["E"] if E is None else E, gamma=GAMMA,
                                 use_proper_time_limits=True, use_gae=True, gae_lambda=LAMBDA,
                                 recurrent_hidden_size=case["hidden"] if hidden is None else hidden, recurrent_hidden_layers=1)


def hashed(shape, *key):
    """float32 array of ``shape`` in [-1, 1), element i a function of (key, i) alone: a 64-bit mix (splitmix64's finaliser), top 24 bits."""
    n = int(np.prod(shape))
    x = np.arange(n, dtype=np.uint64)
    for j, k in enumerate(key):
        x = x + np.uint64((int(k) * 0x9E3779B97F4A7C15 + j * 0xBF58476D1CE4E5B9 + 1) & (2 ** 64 - 1))
        x ^= x >> np.uint64(30)
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x = x * np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return ((x >> np.uint64(40)).astype(np.float64) / 2.0 ** 23 - 1.0).astype(np.float32).reshape(shape)


def stream(case, k, T=None, E=None, A=None, hidden=None, share=0):
    """The inputs of buffer k of a case as arrays over time: what ``feed`` passes to insert(), step by step."""
    T, E, A = (case["T"] if T is None else T), (case["E"] if E is None else E), (case["A"] if A is None else A)
    H = case["hidden"] if hidden is None else hidden
    key = (case["seed"], k)
    s = dict(obs=hashed((T + 1, E, A, case["obs"]), *key, 0), actions=np.floor(hashed((T, E, A, case["act"]), *key, 1) * 8.0),
             rewards=hashed((T, E, A, 1), *key, 2), masks=(hashed((T, E, A, 1), *key, 3) > -0.8).astype(np.float32),
             action_log_probs=hashed((T, E, A, case["act"] if share else 1), *key, 4) - 2.0, value_preds=hashed((T, E, A, 1), *key, 5),
             rnn_states_actor=hashed((T + 1, E, A, 1, H), *key, 6), rnn_states_critic=hashed((T + 1, E, A, 1, H), *key, 7),
             bad_masks=(hashed((T, E, A, 1), *key, 8) > -0.9).astype(np.float32), next_value=hashed((E, A, 1), *key, 9))
    if share:
        s.update(share_obs=hashed((T + 1, E, A, share), *key, 10), active_masks=(hashed((T, E, A, 1), *key, 11) > -0.8).astype(np.float32))
    return s


def feed(buf, s, set0):
    """The stream through insert() and compute_returns(); ``set0(name, value)`` seeds slot 0 as the runners do after a reset."""
    shared = "share_obs" in s
    set0("obs", s["obs"][0]); set0("rnn_states_actor", s["rnn_states_actor"][0]); set0("rnn_states_critic", s["rnn_states_critic"][0])
    if shared:
        set0("share_obs", s["share_obs"][0])
    for t in range(s["actions"].shape[0]):
        kw = dict(obs=s["obs"][t + 1], actions=s["actions"][t], rewards=s["rewards"][t], masks=s["masks"][t],
                  action_log_probs=s["action_log_probs"][t], value_preds=s["value_preds"][t], rnn_states_actor=s["rnn_states_actor"][t + 1],
                  rnn_states_critic=s["rnn_states_critic"][t + 1], bad_masks=s["bad_masks"][t])
        if shared:
            kw.update(share_obs=s["share_obs"][t + 1], active_masks=s["active_masks"][t])
        buf.insert(**kw)
    buf.compute_returns(s["next_value"])


def oracle_buffers(case, T=None, E=None, A=None, hidden=None, share=0):
    """The K numpy buffers of a case (oracle.rollout_buffer), fed and with their returns computed."""
    from oracle.rollout_buffer import OracleRolloutBuffer
    T_, E_, A_ = (case["T"] if T is None else T), (case["E"] if E is None else E), (case["A"] if A is None else A)
    H = case["hidden"] if hidden is None else hidden
    out = []
    for k in range(case["K"]):
        b = OracleRolloutBuffer(T_, E_, A_, case["obs"], case["act"], 1, H, GAMMA, LAMBDA, True, True, share_dim=share)
        feed(b, stream(case, k, T, E, A, hidden, share), lambda name, v, b=b: getattr(b, name).__setitem__(0, v))
        out.append(b)
    return out


def source(chunk, l, L, T, N, K):
    """(buffer, time-major source row) of step l of chunk ``chunk`` of the stack, the chunk index clamped into the stack first."""
    n_chunks = K * T * N // L
    R = min(max(int(chunk), 0), n_chunks - 1) * L + l
    k, r = divmod(R, T * N)
    col, t = divmod(r, T)
    return k, t * N + col


def stacked(bufs, advantages=None):
    """name -> the vstack of the buffers' sequence views, in the list's order; ``advantages``: one array per buffer instead of the
    buffers' own property."""
    from oracle.rollout_buffer import OracleRolloutBuffer
    seq = OracleRolloutBuffer.sequence_rows
    adv = [b.advantages for b in bufs] if advantages is None else advantages
    cut = {"obs": 1, "share_obs": 1, "masks": 1, "active_masks": 1, "returns": 1, "value_preds": 1, "rnn_states_actor": 1, "rnn_states_critic": 1,
           "actions": 0, "action_log_probs": 0}
    names = SHARED_NAMES if bufs[0].shared else NAMES
    out = {}
    for name in names:
        if name == "advantages":
            out[name] = np.vstack([seq(a) for a in adv])
        else:
            out[name] = np.vstack([seq(getattr(b, name)[:-1] if cut[name] else getattr(b, name)) for b in bufs])
    return out


def minibatches(bufs, order, n_mb, L, advantages=None, data_chunks=None):
    """The mini-batches the reference's generator yields for a list of buffers when torch.randperm returns ``order``: tuples in the
    order of NAMES (SHARED_NAMES for shared buffers), rows step-major (row l * mb + j = step l of chunk order[i * mb + j]), the RNN
    states the row of each chunk's first step. ``data_chunks``: the reference's count unless given."""
    rows = stacked(bufs, advantages)
    b = bufs[0]
    if data_chunks is None:
        data_chunks = b.E * (b.T * len(bufs)) // L
    mb = data_chunks // n_mb
    order = np.asarray(order)
    for i in range(n_mb):
        first = order[i * mb:(i + 1) * mb].astype(np.int64) * L
        at = (first[None, :] + np.arange(L)[:, None]).reshape(-1)
        yield tuple(rows[name][first] if name.startswith("rnn_states") else rows[name][at] for name in rows)
