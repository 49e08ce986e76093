"""broadcast_packed carries the attribution state (gloo, world_size=2, CPU):
the per-node expected values and the base value travel when present, and a
model packed without them still broadcasts."""

from __future__ import annotations

import multiprocessing as mp
import os

import numpy as np
import pytest

pytestmark = pytest.mark.slow


def _worker(rank: int, world: int, port: int, npz_path: str, q):
    try:
        import torch.distributed as dist

        from creditcore.pack import PackedModel
        from creditcore.parallel import broadcast_packed

        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        packed = PackedModel.load(npz_path) if rank == 0 else None
        got = broadcast_packed(packed, device="cpu", src=0)
        nv = got.cls_node_value
        q.put(
            (
                rank,
                None if nv is None else (str(nv.dtype), nv.view(np.int32).tolist()),
                (float(got.cls_base_value), len(got.cls_nodes)),
            )
        )
        dist.destroy_process_group()
    except Exception as e:  # surface worker failures to the parent
        q.put((rank, f"ERROR: {type(e).__name__}: {e}", None))


def _run(npz_path: str, port: int) -> dict:
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, npz_path, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(2):
        rank, a, b = q.get(timeout=180)
        assert not (isinstance(a, str) and a.startswith("ERROR")), a
        results[rank] = (a, b)
    for p in procs:
        p.join(timeout=60)
    return results


def test_broadcast_carries_node_values(packed, tmp_path):
    path = str(tmp_path / "packed.npz")
    packed.save(path)
    res = _run(path, 29531)
    dtype, bits = res[1][0]
    assert dtype == "float32"
    assert bits == packed.cls_node_value.view(np.int32).tolist()  # bit-identical
    assert res[0][0] == res[1][0]
    assert res[0][1] == res[1][1] == (packed.cls_base_value, len(packed.cls_nodes))


def test_broadcast_without_node_values(packed, tmp_path):
    import dataclasses

    path = str(tmp_path / "old.npz")
    dataclasses.replace(packed, cls_node_value=None, cls_base_value=0.0).save(path)
    res = _run(path, 29532)
    assert res[0][0] is None and res[1][0] is None
    assert res[0][1] == res[1][1] == (0.0, len(packed.cls_nodes))
