// csrc/conv_plan.h behind a C interface for tests/test_conv_plan_cpu.py (ctypes).  With
// -DCONV_PLAN_MAIN the same calls run over the test's grid as a stand-alone program (for a sanitizer
// build).
#include "../../alphazero-multi-game_amd/csrc/conv_plan.h"

extern "C" {

enum { CP_IN = 8, CP_OUT = 20, CP_NAME = 64 };
// optional outputs / residuals of a row and the other fields a forward varies (CP_IN column 7)
enum { CP_CF = 1, CP_CLO = 2, CP_CQ = 4, CP_RQ = 8, CP_RHI = 16, CP_RLO = 32, CP_NO_RELU = 64, CP_SHORT_TAIL = 128 };

// n plans at once.  in[i] = {family (0 g8, 1 nhwc16, 2 x3), flags, H, C, N, boards, mode (x3: the pieces),
// CP_* bits}; out[i] = {kernel, mode, pt, board, geo, tm, ring, bm, bn, bnt, sched, boards, nt, var,
// stagger, rows, cols, grid, block, conv_plan_name's status}; names[i]: the label, or "none".
void cp_plan_many(const int* in, int n, int* out, char* names) {
    for (int i = 0; i < n; ++i) {
        const int* r = in + CP_IN * i;
        const int H = r[2], o = r[7];
        ConvShape s{};
        s.H = s.W = H; s.C = r[3]; s.N = r[4]; s.M = r[5] * H * H;
        s.rows_per_sample = H * H;
        s.a_tail = (size_t)s.M * s.C * 2 - ((o & CP_SHORT_TAIL) ? 2 : 0);
        s.relu = !(o & CP_NO_RELU);
        s.Cf = o & CP_CF; s.Clo = o & CP_CLO; s.Cq = o & CP_CQ; s.Rq = o & CP_RQ; s.Rhi = o & CP_RHI; s.Rlo = o & CP_RLO;
        s.pt = r[0] == 2 ? r[6] : 0;
        const ConvPlan p = r[0] == 0 ? conv_plan_g8(s, r[6], r[1]) : r[0] == 1 ? conv_plan_nhwc16(s, r[6], r[1]) : conv_plan_x3(s, r[1]);
        char* name = names + (size_t)CP_NAME * i;
        const int st = conv_plan_name(p, name, CP_NAME);
        if (st) snprintf(name, CP_NAME, "none");
        const int v[CP_OUT] = {p.kernel, p.mode, p.pt, p.board, p.geo, p.tm, p.ring, p.bm, p.bn, p.bnt, p.sched, p.boards, p.nt,
                               p.var, p.stagger, p.rows, p.cols, (int)p.grid, (int)p.block, st};
        for (int k = 0; k < CP_OUT; ++k) out[CP_OUT * i + k] = v[k];
    }
}

// the named flag bits in the order of conv_plan.h's table, then the default set
int cp_flags(int* out) {
    const int f[] = {CONV_F_V6_AT_15, CONV_F_DENSE_15, CONV_F_NO_V7, CONV_F_V7_ONLY_15, CONV_F_V7_PAD_15, CONV_F_V7_ANY_BATCH,
                     CONV_F_V6_SMALL, CONV_F_V7_PER_TAP, CONV_F_V7_OLD_TAIL, CONV_F_V7_TM, CONV_F_V7_RING3, CONV_F_KEEP_POOL,
                     CONV_F_FC_F32, CONV_F_V7X3, CONV_F_V9_TAP_BARRIER, CONV_F_V9_KEEP_FRAG, CONV_F_DEFAULT};
    const int n = sizeof f / sizeof f[0];
    for (int i = 0; i < n; ++i) out[i] = f[i];
    return n;
}

}  // extern "C"

#ifdef CONV_PLAN_MAIN
#include <vector>
// the axes of tests/test_conv_plan_cpu.py's grid, every family and mode (and one outside), every CP_* bit alone
int main() {
    std::vector<int> in;
    for (int fl : {0x204, 0x304, 0xa04, 0xe04, 0xa0c, 0x804, 0x10804, 0x20804, 0x30804, 0x40804, 0xa0804, 0xb0804, 0x20a0c, 0x2204,
                   0x4204, 0x1204, 0x10000204, 0x904, 0x20000204, 0x40000204, 0x60000204, 0x200, 0x20c, 0x30204, 0xb0204, 0, -1})
        for (int H : {6, 8, 9, 13, 15, 19})
            for (int C : {16, 32, 48, 64, 128, 256})
                for (int N : {64, 128, 192, 256})
                    for (int B : {1, 64, 128, 256, 400, 512, 768, 1023, 1024, 2048})
                        for (int fam : {0, 1, 2})
                            for (int mode : {0, 1, 2, 3})
                                for (int o : {0, 1, 2, 4, 8, 16, 32, 48, 64, 128}) {
                                    if (o && B != 400) continue;
                                    const int r[CP_IN] = {fam, fl, H, C, N, B, mode, o};
                                    in.insert(in.end(), r, r + CP_IN);
                                }
    const int n = (int)(in.size() / CP_IN);
    std::vector<int> out((size_t)n * CP_OUT);
    std::vector<char> names((size_t)n * CP_NAME);
    cp_plan_many(in.data(), n, out.data(), names.data());
    size_t chars = 0, none = 0;
    for (int i = 0; i < n; ++i) {
        for (const char* c = &names[(size_t)CP_NAME * i]; *c; ++c) ++chars;
        none += out[(size_t)CP_OUT * i] == CONV_NONE;
        ConvPlan p{};                                   // a short buffer: the label is cut, never overrun
        p.kernel = out[(size_t)CP_OUT * i]; p.geo = GEO_DENSE; p.ring = 3; p.tm = 128; p.board = 19; p.mode = 2;
        char cut[8];
        conv_plan_name(p, cut, sizeof cut);
    }
    int f[32];
    if (cp_flags(f) != 17 || f[16] != 0x204) return 1;
    std::printf("conv_plan ok (%d plans, %zu refused, %zu characters)\n", n, none, chars);
    return 0;
}
#endif
