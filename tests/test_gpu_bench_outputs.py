"""bench.py --dump-outputs on the device workload: GpuWorkload.outputs() hands over the MoveData
records of the last step() -- checked against the engine's own record view (the az_move_rec array
step() fetched) on a small net, one file round trip through dump_outputs."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.mark.gpu
def test_gpu_bench_workload_outputs_are_the_last_moves_records(tmp_path):
    import bench
    from az_amd import dist as azdist
    G = 6
    a = bench.parse(["--config", "c2", "--blocks", "2", "--sims", "24", "--global-games", str(G)])
    wl = bench.GpuWorkload(a, 0, azdist.shard_range(0, 1, G))
    try:
        wl.net.init_random(a.seed)
        wl.start()
        wl.step()
        first = wl.outputs()
        mv, _ = wl.step()
        recs, slots = wl.mcts.stepMoves(materialize=False)       # the engine's records as they are
        out = wl.outputs()
        assert mv == G and sorted(slots.tolist()) == list(range(G))
        assert sorted(out) == ["action", "n_children", "policy", "value"]
        assert out["policy"].shape == (G, 225) and out["policy"].dtype == np.float32
        for r, s in zip(recs, slots):
            k = int(r["n_children"])
            pol = np.ctypeslib.as_array(ctypes.cast(int(r["policy"]), ctypes.POINTER(ctypes.c_float)), shape=(k,))
            act = np.ctypeslib.as_array(ctypes.cast(int(r["child_actions"]), ctypes.POINTER(ctypes.c_int)), shape=(k,))
            assert out["action"][s] == r["action"] and out["n_children"][s] == k == 225 - 1     # the second ply
            assert out["value"][s].view(np.uint32) == r["value"].view(np.uint32)
            want = np.zeros(225, np.float32)
            want[act] = pol
            assert np.array_equal(out["policy"][s].view(np.uint32), want.view(np.uint32))
            assert abs(float(pol.sum()) - 1.0) < 1e-5 and pol[act == r["action"]] > 0
        assert not np.array_equal(first["action"], out["action"]) or not np.array_equal(first["policy"], out["policy"])
        bench.dump_outputs(str(tmp_path), out)
        assert all(np.array_equal(np.load(tmp_path / f"{k}.npy"), v) for k, v in out.items())
    finally:
        wl.close()
