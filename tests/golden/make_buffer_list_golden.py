"""Generate tests/golden/buffer_list.npz from the REFERENCE's own ReplayBuffer (runs only where the reference tree exists).

algorithms/utils/buffer.py is imported from the reference with gymnasium stubbed (make_policy_golden.py's stub). For each case of
tests/buffer_list_util.CASES, K buffers are filled through insert() from the util's hash, compute_returns() is called on each, and the
reference's own ``ReplayBuffer.recurrent_generator([b0, ...], num_mini_batch, data_chunk_length)`` is run under a fixed
torch.manual_seed. Stored per case (keys ``<case>/<name>``), data only:

  perm                 the permutation the generator drew (torch.randperm under the same seed, drawn again to record it)
  batch<i>_<j>         entry j (in the order of buffer_list_util.NAMES) of mini-batch i, as yielded
  returns<k>, advantages<k>    buffer k's returns and its own normalised advantages

    python tests/golden/make_buffer_list_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import buffer_list_util as U  # noqa: E402
from make_policy_golden import stub_gymnasium  # noqa: E402


def main():
    sp = stub_gymnasium()
    from algorithms.utils.buffer import ReplayBuffer
    out = {}
    for name, case in U.CASES.items():
        bufs = []
        for k in range(case["K"]):
            b = ReplayBuffer(U.args_of(case), case["A"], sp.Box(low=-1.0, high=1.0, shape=(case["obs"],)), sp.MultiDiscrete([8] * case["act"]))
            U.feed(b, U.stream(case, k), lambda field, v, b=b: getattr(b, field).__setitem__(0, v))
            assert b.step == 0
            bufs.append(b)
            out[f"{name}/returns{k}"], out[f"{name}/advantages{k}"] = b.returns.copy(), b.advantages.astype(np.float32)
        data_chunks = case["E"] * (case["T"] * case["K"]) // case["L"]
        torch.manual_seed(case["seed"])
        batches = list(ReplayBuffer.recurrent_generator(bufs, case["n_mb"], case["L"]))
        torch.manual_seed(case["seed"])
        out[f"{name}/perm"] = torch.randperm(data_chunks).numpy().astype(np.int64)
        assert len(batches) == case["n_mb"]
        for i, batch in enumerate(batches):
            assert len(batch) == len(U.NAMES)
            for j, a in enumerate(batch):
                assert a.dtype == np.float32, (name, i, j, a.dtype)
                out[f"{name}/batch{i}_{j}"] = np.ascontiguousarray(a)
    path = os.path.join(HERE, "buffer_list.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
