// csrc/net_plan.h behind a C interface for tests/test_net_plan_cpu.py and tests/test_gpu_net_plan.py
// (ctypes).  With -DNET_PLAN_MAIN the same calls run over a grid of shapes as a stand-alone program
// (for a sanitizer build).
#include "../../alphazero-multi-game_amd/csrc/net_plan.h"

namespace {

// desc: the twelve ints of az_net_desc in declaration order
NetShape shape_of(const int* desc, int rw) {
    az_net_desc d;
    int* f[12] = {&d.board_size, &d.in_planes, &d.channels, &d.blocks, &d.action_size, &d.head_channels,
                  &d.pool, &d.fc_hidden, &d.residual, &d.conv_bias, &d.precision, &d.max_batch};
    for (int i = 0; i < 12; ++i) *f[i] = desc[i];
    return net_shape(d, rw != 0);
}

}  // namespace

extern "C" {

enum { NP_FIELDS = 10 };

// The plan of one (description, rw, precision) as az_diag_net_plan prints it; returns its status.
int np_plan_line(const int* desc, int rw, int precision, int flags, long lds_limit, char* out, int len) {
    const NetPlan p = net_plan(shape_of(desc, rw), precision, flags, (size_t)lds_limit);
    net_plan_line(p, out, len);
    return p.status;
}

// n plans at once: out[i] = {input, in32, trunk, tail_fused, head_conv_fused, heads, status,
// no_forward set, message length, packs (1 sm, 2 in16, 4 in32, 8 trunk16)}
void np_plan_many(const int* descs, const int* rw, const int* precision, int n, int flags, long lds_limit, int* out) {
    for (int i = 0; i < n; ++i) {
        const NetShape s = shape_of(descs + 12 * i, rw[i]);
        const NetPlan p = net_plan(s, precision[i], flags, (size_t)lds_limit);
        const NetPacks k = net_packs(s);
        int len = 0;
        while (p.message[len]) ++len;
        int* o = out + NP_FIELDS * i;
        o[0] = p.input; o[1] = p.in32; o[2] = p.trunk; o[3] = p.tail_fused; o[4] = p.head_conv_fused; o[5] = p.heads;
        o[6] = p.status; o[7] = p.no_forward != nullptr; o[8] = len;
        o[9] = (k.sm ? 1 : 0) | (k.in16 ? 2 : 0) | (k.in32 ? 4 : 0) | (k.trunk16 ? 8 : 0);
    }
}

int np_cin_pad(const int* desc, int rw) { return shape_of(desc, rw).cin_pad; }

}  // extern "C"

#ifdef NET_PLAN_MAIN
#include <vector>
// the axes of tests/test_net_plan_cpu.py's grid, every precision (and two outside the enum), both entry points
int main() {
    std::vector<int> descs, rws, precs;
    for (int board : {6, 7, 8, 9, 13, 15, 19})
        for (int planes : {3, 11, 16, 17, 111})
            for (int ch : {16, 32, 48, 64, 128, 192, 256})
                for (int blocks : {0, 1, 20, AZ_SMALLNET_MAX_BLOCKS + 1})
                    for (int cap : {1, 127, 128, 511, 512, 1023, 1024, 2048, 1 << 24})
                        for (int rw : {0, 1})
                            for (int prec : {-1, 0, 1, 2, 3, 4, 5}) {
                                const int d[12] = {board, planes, ch, blocks, board * board, 32, 8, 256, 1, 0, prec, cap};
                                descs.insert(descs.end(), d, d + 12);
                                rws.push_back(rw);
                                precs.push_back(prec);
                            }
    const int n = (int)rws.size();
    std::vector<int> out((size_t)n * NP_FIELDS);
    np_plan_many(descs.data(), rws.data(), precs.data(), n, 0x204, 160 * 1024, out.data());
    size_t chars = 0;
    for (int i = 0; i < n; ++i) {
        char line[8];                                   // a short buffer: the line is cut, never overrun
        char full[320];
        np_plan_line(&descs[12 * (size_t)i], rws[i], precs[i], 0x204 | 0x400000, 64 * 1024, line, sizeof line);
        np_plan_line(&descs[12 * (size_t)i], rws[i], precs[i], 0x08000000, 0, full, sizeof full);
        for (const char* c = full; *c; ++c) ++chars;
        if (np_cin_pad(&descs[12 * (size_t)i], rws[i]) % 16) return 1;
    }
    std::printf("net_plan ok (%d plans, %zu characters)\n", n, chars);
    return 0;
}
#endif
