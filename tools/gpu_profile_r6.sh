#!/bin/bash
# Round-6 profile batch: PMC passes of the C3 trunk kernels (fp16 conv3x3_v7, F16X3 conv3x3_v9x3;
# tools/pmc_conv.sh), the rocprofv3 kernel-trace summary of a default bench run (the roofline's
# kernels, headline + parity_mode), then the tree PMC at one sync per 100 simulation steps with the
# crash reporter on (the round-5 profiler SIGSEGV; tools/tree_pmc.sh).  Each step under its own limit.
set -o pipefail
export TMPDIR=/tmp
O=${OUT:-profile_out}/r6prof       # OUT: where the batch writes (default profile_out/, git-ignored)
mkdir -p $O
# geometry A/Bs (conv flag sets, alternating rounds): 15x15 C3 SLIM (default 0x204) vs DENSE (0x20c);
# the C4 128-board shard's tiles: 128-row 3-slot ring (default) vs 64-row (0x30204) vs 64-row 3-slot (0xb0204)
${SKIP_AB:+true} timeout -k 10 300 python3 tools/net_bench.py --game gomoku15 --batch 2048 --flags 0x204,0x20c --rounds 3 --iters 6 > $O/c3_geo_ab.txt 2>&1 &&
${SKIP_AB:+true} timeout -k 10 300 python3 tools/net_bench.py --game go19 --batch 128 --flags 0x204,0x30204,0xb0204 --rounds 3 --iters 20 > $O/c4s_tile_ab.txt 2>&1 &&
${SKIP_PMC:+true} bash tools/pmc_conv.sh fp16 r6_fp16 &&
${SKIP_PMC:+true} bash tools/pmc_conv.sh f16x3 r6_f16x3 &&
${SKIP_TRACE:+true} timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace -o run -- \
    python3 bench.py --full --steps 2 --warmup 1 --cpu-baseline 0 > $O/bench.json 2> $O/bench.err &&
echo "profile steps ok" &&
{ [ -n "$SKIP_TREE" ] || SYNC=${SYNC:-100} TAG=r6tree bash tools/tree_pmc.sh; }
