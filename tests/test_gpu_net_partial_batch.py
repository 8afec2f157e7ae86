"""The compacted network batch of the search (search_host.hip search_step: k_scan writes eval_slot /
eval_games / n_eval and the net runs with LeafRecs.identity = 0) on each of the three input stages
that consume the batch map (net_host.hip net_input_path):
  NET_IN_SMALL  k_smallnet_g / k_smallnet_x3 read the leaf records through gidx
  NET_IN_G8     az_launch_rec_to_g8(rec, gidx, ...) -- 15x15 (NG = 2), the other boards through in32
                (NG = 4), Go records
  NET_IN_GEMM   az_launch_rec_planes(..., eval_games, n_eval, ...) into a dense plane batch
A handle of 8 slots plays only slots 1, 4 and 6: slot 0 is idle, every live slot's batch position
differs from its slot number, idle slots lie between and after the live ones, and every simulation
batch holds n_eval <= 3 < G boards.  One live slot is logged and replayed through the CPU
restatement bit for bit; every logged output is checked against the fp32 reference network and,
bitwise, against a dense forward of the logged planes on the same net (the logged output belongs to
that leaf, not to a neighbour's batch row)."""
import numpy as np
import pytest

from replay_util import compare_roots, replay_eval_log, root_record

G, LIVE, SIMS, MOVES = 8, [1, 4, 6], 32, 3
TOL = 1e-4   # BASELINE.json north_star: every precision but plain bf16, init weights

G8 = ("conv3x3_v5<", "conv3x3_v6<", "conv3x3_v7<")   # the g8 trunk kernels (conv_bf16.hip g8_choice)

# id: (game, board, channels, blocks, precision, trunk kernel family at max_batch = 8, fp32 check)
CASES = {
    "gemm-f32":       ("gomoku", 7, 32, 2, "f32", ("gemm_f32",), True),
    "gemm-bf16x3":    ("gomoku", 7, 32, 2, "bf16x3", ("conv3x3_bf16<split>",), True),
    "small-fp16":     ("gomoku", 15, 64, 1, "fp16", ("k_smallnet_g<15,",), True),
    "small-bf16x3":   ("gomoku", 15, 64, 1, "bf16x3", ("k_smallnet_x3<15, 8, true, 1>",), True),
    "small-f16x3":    ("gomoku", 15, 64, 1, "f16x3", ("k_smallnet_x3<15, 8, true, 2>",), True),
    "g8-15-fp16":     ("gomoku", 15, 128, 1, "fp16", tuple(k + "2, 15" for k in G8), True),
    # plain bf16 is held to 1e-4 nowhere: the replay and the dense-forward bit check only
    "g8-15-bf16":     ("gomoku", 15, 128, 1, "bf16", tuple(k + "1, 15" for k in G8), False),
    "g8-in32-fp16":   ("gomoku", 9, 128, 1, "fp16", tuple(k + "2, 9" for k in G8), True),
    "g8-go-fp16":     ("go", 9, 128, 1, "fp16", tuple(k + "2, 9" for k in G8), True),
    # 128 channels take the v7x3 tile of the fp16-piece trunk (v9x3 is the 256-channel one)
    "x3-trunk-f16x3": ("gomoku", 15, 128, 1, "f16x3", ("conv3x3_v7x3<15, SLIM, f16>", "conv3x3_v9x3<15, SLIM, f16>"), True),
}


@pytest.fixture(scope="module")
def engine():
    import az_amd
    return az_amd.Engine(0)


@pytest.mark.gpu
@pytest.mark.parametrize("logged", [1, 6])
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_partial_batch_matches_oracle_replay(engine, case, logged):
    import az_amd
    import az_oracle as O
    import net_oracle
    game, bs, ch, blocks, prec, kernels, fp32 = CASES[case]
    go = game == "go"
    p = {"f32": az_amd.AZ_PREC_F32, "bf16x3": az_amd.AZ_PREC_BF16X3, "f16x3": az_amd.AZ_PREC_F16X3,
         "bf16": az_amd.AZ_PREC_BF16, "fp16": az_amd.AZ_PREC_FP16}[prec]
    desc = az_amd.NetDesc(bs, 8 if go else 11, ch, blocks, bs * bs + (1 if go else 0), 32, 8, 256, 1, 0, p, G)
    net = az_amd.HipNeuralNetwork(engine, desc)
    m = None
    try:
        name = net.trunk_kernel()
        assert name.startswith(kernels), name
        blob = net_oracle.init_blob(desc, seed=9)
        net.load_weights(blob)
        m = az_amd.ParallelMCTS(engine, n_games=G, board_size=bs, num_simulations=SIMS, evaluator=az_amd.AZ_EVAL_NET,
                                net=net, noise_seed=42, noise_seed_stride=1,
                                game=az_amd.AZ_GAME_GO if go else az_amd.AZ_GAME_GOMOKU)
        cap = (SIMS + 2) * (MOVES + 1)
        m.enableEvalLog(logged, cap)
        m.newGames(LIVE)
        m.addDirichletNoise(0.03, 0.25)
        idle = [g for g in range(G) if g not in LIVE]
        alive = list(LIVE)
        dev = []
        for ply in range(MOVES):
            m.search()
            act, val, probs, cact, nch = m.select(True, 1.0)
            # the precondition of the compacted branch: the five other slots are idle on every move
            assert [int(act[g]) for g in idle] == [m.none] * len(idle), (ply, act.tolist())
            assert all(int(act[g]) != m.none and nch[g] > 0 for g in alive), (ply, act.tolist())
            dev.append(root_record(m, logged, act, val, probs, nch))
            term, _ = m.updateWithMove(act)
            if ply % 2 == 0:
                m.addDirichletNoise(0.03, 0.25)
            # three stones end no Gomoku game; a Go game ends when both sides pass (with these init
            # weights after two plies), and a finished live slot joins the idle ones
            assert go or not term[alive].any(), (ply, term.tolist())
            idle += [g for g in alive if term[g]]
            alive = [g for g in alive if not term[g]]
            if logged not in alive:
                break
        assert len(dev) == MOVES or (go and len(dev) >= 2), len(dev)
        pol, valv, planes = m.readEvalLog(cap)
    finally:
        if m is not None:
            m.close()
    try:
        assert SIMS < len(pol) < cap and planes.shape[1] == desc.in_planes
        ref = replay_eval_log(pol, valv, planes, [(logged, len(dev))], bs=bs, sims=SIMS,
                              game=O.GAME_GO if go else O.GAME_GOMOKU)[0]
        compare_roots(dev, ref["moves"])
        # the logged value of every evaluation is bitwise the value a dense forward gives its planes
        dv = np.concatenate([net.forward(planes[i:i + G])[1] for i in range(0, len(planes), G)])
        same = dv.view(np.uint32) == valv.view(np.uint32)
        # every logged output against the fp32 reference network on the logged planes
        rl, rv = net_oracle.forward(desc, blob, planes)
        ev = float(np.abs(valv - rv).max())
        ep = float(np.abs(pol - net_oracle.softmax_policy(rl)).max())
        print(f"partial batch {case} slot {logged}: trunk {name}, {len(pol)} logged evaluations replayed, "
              f"{int(same.sum())} values bitwise a dense forward's, max|dvalue|={ev:.3e} max|dpolicy|={ep:.3e} vs fp32")
        assert same.all(), np.flatnonzero(~same).tolist()
        if fp32:
            assert ev <= TOL and ep <= TOL, (ev, ep)
    finally:
        net.close()
