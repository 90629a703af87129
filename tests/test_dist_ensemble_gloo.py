"""dist.merge_ensembles on CPU: two gloo processes each hold the ensemble statistics of their contiguous shard (the numpy reference of
f16_mpc_oop_py_amd/ensemble.py stands for the device call, which tests/test_gpu_ensemble.py holds equal to it); the merged result is
`combine` of the two ranks' statistics in rank order, exactly, on both ranks, and the exact statistic of the whole batch within the
bound of tests/test_ensemble_cpu.py `error_bounds` (group size 64 per rank: a merged group holds one wave of each rank, so W = 2)."""
import os
import socket
from fractions import Fraction

import numpy as np
import torch.multiprocessing as mp

from test_ensemble_cpu import error_bounds, exact_group, synthetic

B_RANK, S, GROUP = 130, 2, 64          # per rank: two full groups and a short one


def shard(rank):
    x = synthetic(B_RANK, S=S, seed=10 + rank)
    x[0, 2, 5 + rank] = np.nan
    x[:, :, 64:128] = np.inf if rank == 0 else x[:, :, 64:128]          # rank 0 brings an empty group 1
    return x


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        import torch
        import torch.distributed as dist
        from f16_mpc_oop_py_amd import dist as fdist
        from f16_mpc_oop_py_amd.ensemble import Ensemble, ensemble_reference
        fdist.init_from_env("gloo")
        mine = ensemble_reference(shard(rank), GROUP, envelope=False)
        # as F16Batch returns it: torch tensors, the four moments as [S, G, 18] views of [S, 18, G] storage
        as_env = Ensemble(torch.as_tensor(mine.count), *(torch.as_tensor(np.ascontiguousarray(v.transpose(0, 2, 1))).permute(0, 2, 1)
                                                         for v in mine.parts()[1:]), group=GROUP)
        merged = fdist.merge_ensembles(as_env)
        q.put((rank, [np.asarray(v) for v in merged.parts()]))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:      # surface the failure instead of a queue timeout
        q.put((rank, repr(e)))
        raise


def test_merge_is_the_fold_in_rank_order_world2():
    from f16_mpc_oop_py_amd.ensemble import combine, ensemble_reference
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = dict(q.get(timeout=120) for _ in range(2))
    [p.join(60) for p in procs]
    assert all(p.exitcode == 0 for p in procs), res
    parts = [ensemble_reference(shard(r), GROUP, envelope=False).parts() for r in range(2)]
    want = combine(parts[0], parts[1])
    for r in range(2):                                     # exactly the fold, the same on both ranks
        for got, w in zip(res[r], want):
            assert got.shape == w.shape and got.dtype == w.dtype and np.array_equal(got, w), r
    assert list(want[0][1]) == [64 + 64, 64, 2 + 2] and list(want[0][0]) == [63 + 63, 64, 4]          # (rank 0's group 1 is empty)
    assert np.array_equal(want[1][:, 1], parts[1][1][:, 1]) and np.array_equal(want[2][:, 1], parts[1][2][:, 1])
    # ... and the exact statistic of the two shards' aircraft together, within the bound (two waves per merged group)
    x = [shard(r) for r in range(2)]
    worst = 0.0
    for s_ in range(S):
        for g in range(3):
            cols = [xr[s_][:, g * GROUP:(g + 1) * GROUP] for xr in x]
            both = np.concatenate([c[:, np.isfinite(c).all(0)] for c in cols], 1)
            assert want[0][s_, g] == both.shape[1]
            for k in range(18):
                _, mean, m2, mn, mx = exact_group(both[k])
                bm, b2 = error_bounds(float(np.abs(both[k]).max()), mx - mn, float(m2), 2)
                em, e2 = abs(float(Fraction(float(want[1][s_, g, k])) - mean)), abs(float(Fraction(float(want[2][s_, g, k])) - m2))
                assert em <= bm and e2 <= b2 and want[3][s_, g, k] == mn and want[4][s_, g, k] == mx, (s_, g, k, em, bm, e2, b2)
                worst = max(worst, em / bm if bm else 0.0, e2 / b2 if b2 else 0.0)
    print(f"MEASURED merged against exact: largest error / bound {worst:.2e}")


def test_without_a_group_the_result_is_the_input():
    from f16_mpc_oop_py_amd import dist as fdist
    from f16_mpc_oop_py_amd.ensemble import ensemble_reference
    mine = ensemble_reference(shard(1), GROUP, envelope=False)
    for got, w in zip(fdist.merge_ensembles(mine).parts(), mine.parts()):
        assert np.array_equal(got, w)
