"""The self_play binary on the GPU (cpp/tools/self_play_main.cpp, the reference's
src/selfplay/selfplay_main.cpp): its records against the oracle's playSingleGame records bit for
bit (RandomPolicyNetwork -> the device random evaluator, the reference main's MCTS settings: fpu
0.1, root noise on every search), its metadata file, and the communicator path (--dist-id-file:
RCCL init, shape + weight broadcast of a random-init 20-block trunk net, the job counters reduced)
on one GPU."""
import glob
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "alphazero-multi-game_amd", "build", "self_play")


def _bits(xs):
    return np.asarray(xs, np.float32).view(np.uint32).tolist()


@pytest.mark.gpu
def test_gpu_self_play_binary_matches_oracle(tmp_path):
    import az_oracle as O
    n, bs, sims = 4, 7, 32
    out = tmp_path / "games"
    r = subprocess.run([BIN, "--game", "gomoku", "--size", str(bs), "--num-games", str(n), "--simulations", str(sims),
                        "--batch-size", str(n), "--output-dir", str(out), "--threads", "4"],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    refs = O.play(seed_stride=1, bs=bs, sims=sims, eval_kind=O.EVAL_RANDOM, eval_seed=0, n_games=n, fpu=0.1,
                  noise_each_search=1)
    for g in range(n):
        files = glob.glob(str(out / f"{g:03d}_*.json"))
        assert len(files) == 1, g
        rec = json.load(open(files[0]))
        ref = refs[g]
        assert rec["board_size"] == bs and len(rec["moves"]) == len(ref["moves"]), g
        for ply, (mv, rm) in enumerate(zip(rec["moves"], ref["moves"])):
            assert mv["action"] == rm["action"], (g, ply)
            # JSON keeps no NaN payload (null): at T = 0 the reference's NaN entries are compared as NaNs
            rp = np.asarray(rm["probs"], np.uint32).view(np.float32)
            assert len(mv["policy"]) == len(rp) and all((p is None) == bool(np.isnan(r)) for p, r in zip(mv["policy"], rp))
            assert _bits([0.0 if p is None else p for p in mv["policy"]]) == \
                _bits(np.where(np.isnan(rp), np.float32(0.0), rp)), (g, ply)
            assert _bits([mv["value"]])[0] == rm["value"], (g, ply)
        assert rec["result"] == ref["result"], g
    md = [json.load(open(f)) for f in glob.glob(str(out / "metadata_*.json"))]
    assert len(md) == 1
    md = md[0]
    assert (md["game"], md["board_size"], md["num_games_requested"], md["num_games_completed"]) == ("gomoku", bs, n, n)
    assert md["total_moves"] == sum(len(x["moves"]) for x in refs) and md["threads"] == 4
    assert md["world"] == 1 and md["job_total_moves"] == -1


@pytest.mark.gpu
def test_gpu_self_play_binary_dist_path(tmp_path):
    """--dist-id-file on one GPU: rank 0 writes the id, inits a 20 x 256 net, broadcasts shape and
    weights through the engine's communicator, plays, reduces the job counters."""
    out = tmp_path / "games"
    r = subprocess.run([BIN, "--num-games", "8", "--simulations", "16", "--batch-size", "8", "--max-moves", "4",
                        "--net-blocks", "20", "--net-channels", "256", "--precision", "fp16", "--output-dir", str(out),
                        "--world", "1", "--rank", "0", "--dist-id-file", str(tmp_path / "id")],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.getsize(tmp_path / "id") == 128
    md = json.load(open(glob.glob(str(out / "metadata_*.json"))[0]))
    assert md["precision"] == "fp16" and md["fp16_used"] is True and md["world"] == 1
    assert md["job_total_moves"] == md["total_moves"] == 8 * 4 and md["job_games_completed"] == 8
    assert len(glob.glob(str(out / "0*_*.json"))) == 8
    assert "Job: 8 games, 32 moves" in r.stdout


@pytest.mark.gpu
def test_gpu_self_play_binary_with_net_matches_in_process(tmp_path):
    """The binary with a device network, played to completion: 7 games of 6x6 Gomoku on 3 slots
    (--batch-size 3) with a random-init 2 x 32 net in f32.  Its record files equal, game by game, the
    records of the same run made in-process -- HipNeuralNetwork.init_random(7) (net_oracle.init_blob,
    test_gpu_net_init_random_matches_numpy), SelfPlayManager with the binary's search settings (fpu
    0.1, root noise on every search, noise seed 42 + game id: shardGames(0, 1, 7, 42) and
    SelfPlayManager::setShard) -- the configuration whose oracle replay
    test_gpu_net_selfplay_run_matches_oracle_replay[binary-cfg] verifies."""
    import az_amd
    n, slots, bs, sims, seed = 7, 3, 6, 32, 7
    out = tmp_path / "games"
    r = subprocess.run([BIN, "--game", "gomoku", "--size", str(bs), "--num-games", str(n), "--batch-size", str(slots),
                        "--simulations", str(sims), "--net-blocks", "2", "--net-channels", "32", "--seed", str(seed),
                        "--precision", "f32", "--output-dir", str(out), "--threads", "4"],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    eng = az_amd.Engine(0)
    desc = az_amd.gomoku_net_desc(board_size=bs, channels=32, blocks=2, precision=az_amd.AZ_PREC_F32, max_batch=slots)
    net = az_amd.HipNeuralNetwork(eng, desc)
    net.init_random(seed)
    mgr = az_amd.SelfPlayManager(eng, net=net, numGames=slots, numSimulations=sims, board_size=bs, fpu_reduction=0.1,
                                 use_dirichlet_each_search=True, noise_seed=42, noise_seed_stride=1)
    try:
        twins = mgr.generateGames(totalGames=n)
    finally:
        mgr.mcts.close()
        net.close()
    assert [t.game_id for t in twins] == list(range(n))
    for g, twin in enumerate(twins):
        files = glob.glob(str(out / f"{g:03d}_*.json"))
        assert len(files) == 1, g
        rec = json.load(open(files[0]))
        assert rec["board_size"] == bs and len(rec["moves"]) == len(twin.moves) > 0, g
        for ply, (mv, tm) in enumerate(zip(rec["moves"], twin.moves)):
            assert mv["action"] == tm.action, (g, ply)
            # JSON keeps no NaN payload (null): the T = 0 NaN entries are compared as NaNs
            tp = np.asarray(tm.policy, np.float32)
            assert len(mv["policy"]) == len(tp) and all((p is None) == bool(np.isnan(t)) for p, t in zip(mv["policy"], tp)), \
                (g, ply)
            assert _bits([0.0 if p is None else p for p in mv["policy"]]) == \
                _bits(np.where(np.isnan(tp), np.float32(0.0), tp)), (g, ply)
            assert _bits([mv["value"]])[0] == _bits([tm.value])[0], (g, ply)
        assert rec["result"] == twin.result, g
    md = [json.load(open(f)) for f in glob.glob(str(out / "metadata_*.json"))]
    assert len(md) == 1
    md = md[0]
    assert (md["num_games_requested"], md["num_games_completed"]) == (n, n)
    assert md["total_moves"] == sum(len(t.moves) for t in twins)
    assert md["precision"] == "f32" and md["fp16_used"] is False and md["world"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [None, "fp16", "bf16x3"], ids=["default", "fp16", "bf16x3"])
def test_gpu_self_play_binary_c2_shape_net_matches_in_process(tmp_path, precision):
    """The binary on the C2 net's shape class (15x15, 64 filters: the fused k_smallnet kernels): it creates
    its random-init net at f32 and switches it to the run's precision afterwards -- with no --precision
    that is f16x3, the fp32-faithful fp16 pieces -- so the weight sets of the fused kernels must be on the
    device whatever precision the net was loaded at (tests/test_gpu_net_lifecycle.py).  Its records
    equal, move for move, those of the same run in-process with a net CREATED at that precision."""
    import az_amd
    n, slots, bs, sims, seed, max_moves = 2, 2, 15, 8, 7, 3
    want = precision or "f16x3"
    out = tmp_path / "games"
    cmd = [BIN, "--game", "gomoku", "--size", str(bs), "--num-games", str(n), "--batch-size", str(slots),
           "--simulations", str(sims), "--max-moves", str(max_moves), "--net-blocks", "2", "--net-channels", "64",
           "--seed", str(seed), "--output-dir", str(out), "--threads", "4"]
    if precision:
        cmd += ["--precision", precision]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    md = [json.load(open(f)) for f in glob.glob(str(out / "metadata_*.json"))]
    assert len(md) == 1
    md = md[0]
    assert md["precision"] == want
    assert (md["num_games_requested"], md["num_games_completed"]) == (n, n)
    prec = {"f16x3": az_amd.AZ_PREC_F16X3, "fp16": az_amd.AZ_PREC_FP16, "bf16x3": az_amd.AZ_PREC_BF16X3}[want]
    eng = az_amd.Engine(0)
    desc = az_amd.gomoku_net_desc(board_size=bs, channels=64, blocks=2, precision=prec, max_batch=slots)
    net = az_amd.HipNeuralNetwork(eng, desc)
    assert net.trunk_kernel().startswith("k_smallnet_g<15," if want == "fp16" else "k_smallnet_x3<15,")
    net.init_random(seed)
    mgr = az_amd.SelfPlayManager(eng, net=net, numGames=slots, numSimulations=sims, board_size=bs, fpu_reduction=0.1,
                                 use_dirichlet_each_search=True, noise_seed=42, noise_seed_stride=1)
    try:
        twins = mgr.generateGames(totalGames=n, max_moves=max_moves)
    finally:
        mgr.mcts.close()
        net.close()
    assert [t.game_id for t in twins] == list(range(n))
    for g, twin in enumerate(twins):
        files = glob.glob(str(out / f"{g:03d}_*.json"))
        assert len(files) == 1, g
        rec = json.load(open(files[0]))
        assert rec["board_size"] == bs and len(rec["moves"]) == len(twin.moves) == max_moves, g
        for ply, (mv, tm) in enumerate(zip(rec["moves"], twin.moves)):
            assert mv["action"] == tm.action, (g, ply)
            # JSON keeps no NaN payload (null): the T = 0 NaN entries are compared as NaNs
            tp = np.asarray(tm.policy, np.float32)
            assert len(mv["policy"]) == len(tp) and all((p is None) == bool(np.isnan(t)) for p, t in zip(mv["policy"], tp)), \
                (g, ply)
            assert _bits([0.0 if p is None else p for p in mv["policy"]]) == \
                _bits(np.where(np.isnan(tp), np.float32(0.0), tp)), (g, ply)
            assert _bits([mv["value"]])[0] == _bits([tm.value])[0], (g, ply)
        assert rec["result"] == twin.result, g
    assert md["total_moves"] == sum(len(t.moves) for t in twins)
