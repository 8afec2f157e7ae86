#!/usr/bin/env python3
"""The closed training loop on one GPU at a small scale, without a host trip for positions or weights:

    self-play (SelfPlayManager, the net as evaluator) -> device replay ring (ReplayBuffer) ->
    ReplayBuffer.sample_into (torch tensors) -> one SGD step of a torch module ->
    az_amd.state_dict_blob -> HipNeuralNetwork.load_weights_device -> next round of self-play

The module is the caller's: any nn.Module whose state_dict is in the engine's blob order (az_net_num_params;
oracle/net_oracle.param_shapes names the entries).  ResNet below is the plain residual net the engine runs.
The loss is the policy cross-entropy against the visit distribution plus the value MSE against the outcome.
Prints one line per round; the last line is a JSON summary."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-multi-game_amd"))

import torch                     # noqa: E402  (before libaz_hip.so: one HIP runtime)
import torch.nn as nn            # noqa: E402
import torch.nn.functional as F  # noqa: E402

import az_amd                    # noqa: E402


class ResNet(nn.Module):
    """az_net_desc as a torch module; attribute names and order give the blob order."""

    def __init__(self, d):
        super().__init__()
        Fc, HC, PP = d.channels, d.head_channels, d.pool * d.pool
        bias = bool(d.conv_bias)
        self.pool, self.residual = d.pool, bool(d.residual)
        self.input_conv = nn.Conv2d(d.in_planes, Fc, 3, padding=1, bias=bias)
        self.input_bn = nn.BatchNorm2d(Fc)
        self.blocks = nn.ModuleList([nn.Sequential(nn.Conv2d(Fc, Fc, 3, padding=1, bias=bias), nn.BatchNorm2d(Fc), nn.ReLU(),
                                                   nn.Conv2d(Fc, Fc, 3, padding=1, bias=bias), nn.BatchNorm2d(Fc))
                                     for _ in range(d.blocks)])
        self.policy_conv = nn.Conv2d(Fc, HC, 1, bias=bias)
        self.policy_bn = nn.BatchNorm2d(HC)
        self.policy_fc = nn.Linear(HC * PP, d.action_size)
        self.value_conv = nn.Conv2d(Fc, HC, 1, bias=bias)
        self.value_bn = nn.BatchNorm2d(HC)
        self.value_fc1 = nn.Linear(HC * PP, d.fc_hidden)
        self.value_fc2 = nn.Linear(d.fc_hidden, 1)

    def forward(self, x):
        x = torch.relu(self.input_bn(self.input_conv(x)))
        for b in self.blocks:
            x = torch.relu(b(x) + x) if self.residual else torch.relu(b(x))
        x = F.adaptive_avg_pool2d(x, (self.pool, self.pool))
        pol = self.policy_fc(torch.relu(self.policy_bn(self.policy_conv(x))).flatten(1))
        v = torch.relu(self.value_fc1(torch.relu(self.value_bn(self.value_conv(x))).flatten(1)))
        return pol, torch.tanh(self.value_fc2(v)).reshape(-1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--games", type=int, default=32, help="games per round (one device slot each)")
    ap.add_argument("--sims", type=int, default=32)
    ap.add_argument("--max-moves", type=int, default=24, help="games are cut after this many plies")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=1, help="SGD steps per round")
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--random-opening-plies", type=int, default=0,
                    help="every game begins with this many random legal plies drawn on the device (each round under a "
                         "seed of its own); the replay buffer holds the searched positions only")
    args = ap.parse_args()

    eng = az_amd.Engine(0)
    desc = az_amd.gomoku_net_desc(board_size=args.board, channels=args.channels, blocks=args.blocks,
                                  precision=az_amd.AZ_PREC_F32, max_batch=args.games)
    net = az_amd.HipNeuralNetwork(eng, desc)
    torch.manual_seed(args.seed)
    model = ResNet(desc).cuda()
    blob = az_amd.state_dict_blob(model.state_dict())
    if blob.numel() != net.num_params:
        raise SystemExit(f"the module has {blob.numel()} parameters, the engine's net {net.num_params}")
    net.load_weights_device(blob)
    rb = az_amd.ReplayBuffer(eng, az_amd.GAME_GOMOKU, args.board, capacity=1 << 14, max_plies=args.max_moves)
    mgr = az_amd.SelfPlayManager(eng, net=net, numGames=args.games, numSimulations=args.sims, board_size=args.board,
                                 noise_seed=42 + args.seed, noise_seed_stride=1)
    mgr.mcts.attachReplay(rb)
    rb.seed(args.seed)
    opt = torch.optim.SGD(model.parameters(), lr=args.lr, momentum=0.9)
    st = torch.empty((args.batch, rb.C, args.board, args.board), dtype=torch.float32, device="cuda")
    po = torch.empty((args.batch, rb.NA), dtype=torch.float32, device="cuda")
    z = torch.empty(args.batch, dtype=torch.float32, device="cuda")
    log = []
    for rnd in range(args.rounds):
        t0 = time.perf_counter()
        if args.random_opening_plies:   # a round numbers its games from 0 again: another seed, other openings
            mgr.setOpenings(None, args.random_opening_plies, seed=(args.seed << 32) + rnd)
        mgr.generateGames(args.games, max_moves=args.max_moves)
        t1 = time.perf_counter()
        model.train()
        for _ in range(args.steps):
            rb.sample_into(st, po, z)
            logits, v = model(st)
            loss_p = -(po * torch.log_softmax(logits, 1)).sum(1).mean()
            loss_v = ((v - z) ** 2).mean()
            opt.zero_grad()
            (loss_p + loss_v).backward()
            opt.step()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        az_amd.state_dict_blob(model.state_dict(), out=blob)
        net.load_weights_device(blob)
        t3 = time.perf_counter()
        row = dict(round=rnd, positions=rb.info()["committed"], loss_policy=float(loss_p), loss_value=float(loss_v),
                   selfplay_ms=(t1 - t0) * 1e3, train_ms=(t2 - t1) * 1e3, publish_ms=(t3 - t2) * 1e3)
        log.append(row)
        print(f"round {rnd}: {row['positions']} positions, loss {row['loss_policy']:.4f} + {row['loss_value']:.4f}, "
              f"self-play {row['selfplay_ms']:.1f} ms, train {row['train_ms']:.1f} ms, publish {row['publish_ms']:.3f} ms")
    mgr.mcts.close()
    rb.close()
    net.close()
    print(json.dumps({"train_loop": log}))


if __name__ == "__main__":
    main()
