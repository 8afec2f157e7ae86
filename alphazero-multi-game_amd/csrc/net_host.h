// net_host.h -- the device network as the other host units see it: the handle with its layers
// and buffers, and the forward that the search drives.  Internal to libaz_hip.so; dist.hip keeps to
// the accessors of engine_internal.h.
#pragma once
#include <mutex>
#include <utility>
#include <vector>

#include "engine_internal.h"
#include "net.h"
#include "randwire.h"

struct Layer {            // one implicit-GEMM layer, BN folded
    float* W = nullptr;   // [N][K] fp32
    uint16_t* Whi = nullptr; uint16_t* Wlo = nullptr;   // bf16 split copies (3x3 trunk)
    uint16_t* Wh16 = nullptr;                           // fp16 copy (3x3 trunk, AZ_PREC_FP16)
    uint16_t* Wbk_bf = nullptr; uint16_t* Wbk_h = nullptr;  // chunk-blocked bf16 / fp16 copies (v5 conv)
    uint16_t* Wbk_lo = nullptr;                         // chunk-blocked bf16 lo parts (conv3x3_v7x3, AZ_PREC_BF16X3)
    // AZ_PREC_F16X3: the weights of output channel o scaled by 2^s_o (max |W[o]| in [2^13, 2^14)) and
    // split into chunk-blocked fp16 hi / lo pieces; bx = b * 2^s (the accumulators' start), sx = 2^-s
    uint16_t* Wbk_fh = nullptr; uint16_t* Wbk_fl = nullptr;
    float* bx = nullptr; float* sx = nullptr;
    float* b = nullptr;   // [N]
    int N = 0, K = 0, Kpad = 0, taps = 1, C = 0;
};

// One DDW-RandWire node (row f4): its router (only used with >1 predecessors), the residual
// block's two 3x3 convs (BN folded) and the SE block's two linear layers.
struct RwNode {
    Layer router, c1, c2;
    const float** ins = nullptr;   // device: the predecessors' output buffers (the router's concat)
    float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;   // SE: [R][C], [R], [C][R], [C]
};
struct RwBlock {
    azrw::Plan plan;
    std::vector<RwNode> node;   // by node id
    Layer out_router;           // when the block has more than one sink
    const float** outs = nullptr;   // device: the sinks' output buffers
};

struct az_net {
    az_engine* e = nullptr;
    az_net_desc d{};
    int cin_pad = 16;         // NetShape::cin_pad (net_plan.h)
    int HW = 0, P2 = 0;
    size_t act_elems = 0;   // elements of every 16-bit activation buffer before its zeroed tail
    size_t nparams = 0;
    Layer in, pconv, vconv, pfc, vfc1, vfc2;
    // the input conv with its 16 input channels zero-padded to 32 (16-bit chunk-blocked copies only
    // used): boards other than 15x15 take it on conv3x3_v6 (32-channel chunks) instead of the f32
    // GEMM + fp32 -> g8 conversion (C4 Go, 128-board shard: ~98 -> ~15 us per forward)
    Layer in32;
    Layer hconv;              // [pconv; vconv] as one 1x1 conv (2 HC outputs): both heads in one GEMM
    float* hpv = nullptr;     // its output [B * P * P][2 HC] (policy channels, then value)
    std::vector<Layer> blk;   // 2 per block
    // activations (max_batch samples)
    float *x0 = nullptr, *h0 = nullptr, *h1 = nullptr, *t = nullptr, *pool = nullptr;
    uint16_t *hh[2] = {nullptr, nullptr}, *hl[2] = {nullptr, nullptr}, *th = nullptr, *tl = nullptr;
    float *pp = nullptr, *vp = nullptr, *v1 = nullptr, *logits = nullptr, *value = nullptr, *soft = nullptr;
    float* ws = nullptr;                                // split-K workspace of the FC layers
    float* in_nchw = nullptr;
    int* d_nb = nullptr;
    int* ovf = nullptr;         // set by the fp16 kernels when an activation leaves the fp16 range (sticky until read)
    uint16_t* zero = nullptr;   // 256 zero bytes: glds source for the board edge
    // k_smallnet (64-filter fp16 nets): [2*blocks+1][9][64][64] fp16 trunk weights incl. the input conv, biases
    uint16_t* sm_W = nullptr;
    uint16_t* sm_Wf = nullptr;                  // the same weights fragment-major (k_smallnet's register path)
    uint16_t* sm_Wfh = nullptr; uint16_t* sm_Wfl = nullptr;   // scaled fp16 pieces (k_smallnet_x3<.., 2>, AZ_PREC_F16X3)
    float* sm_bx = nullptr; float* sm_sx = nullptr;           // their biases * 2^s and scales 2^-s, [L][64]
    uint16_t* sm_Wxh = nullptr;                 // bf16 hi / lo parts, fragment-major (k_smallnet_x3, AZ_PREC_BF16X3)
    uint16_t* sm_Wxl = nullptr;
    uint16_t* fcx_hi = nullptr;                 // both FC layers' bf16 hi / lo rows (k_fc_heads_x3)
    uint16_t* fcx_lo = nullptr;
    uint16_t* fcf_hi = nullptr;                 // the same rows scaled by 2^s, fp16 hi / lo (k_fc_heads_x3<2>, F16X3)
    uint16_t* fcf_lo = nullptr;
    float* fcf_rs = nullptr;                    // [NC] 2^-s
    float* sm_b = nullptr;
    // DDW-RandWire trunk (az_net_create_randwire): d.blocks rand-wire blocks of 32 nodes
    bool rw = false;
    std::vector<RwBlock> rwb;
    std::vector<float*> rw_out;       // node outputs [B*HW][F], by node id
    float *rw_t2 = nullptr, *rw_in = nullptr;   // conv2 output, router output
    int rw_splits = 1;                // K slices of the node convs (from the capacity: batch-size independent)
    float* rw_ws = nullptr;           // their split-K partials [rw_splits][rows][F]
    bool loaded = false;
    std::vector<float> host_blob;   // canonical blob of the loaded weights (az_net_get_weights)
    // az_net_load_weights_device keeps the blob it loaded on the device (d_blob, in `blob`) and marks the
    // host copy stale; az_net_get_weights / net_host_blob fetch it when first asked (net_load.hip)
    float* d_blob = nullptr;
    bool host_stale = false;
    double pack_ms = -1.0;          // device time of the last device load's launches (profiling on), else -1
    // Device memory (dev_pool.h); the named pointers above and in the layers point into these.
    // weights: every weight buffer, in the loader's order (a load allocates what is missing and
    // rewrites the rest): what az_net_broadcast_weights sends.  acts: every activation / workspace
    // buffer (bytes before any zeroed tail): the poison diagnostic (az_diag_set_poison) overwrites
    // them before each forward.  misc: d_nb, ovf, zero, the router tables, the profile clock.
    // blob: d_blob alone -- kept out of `weights`, whose list a broadcast compares and sends.
    DevPool weights, acts, misc, blob;
    // profiling: HIP events bracketing the 3x3 trunk of every forward (on the launch stream)
    bool prof = false;
    ProfClock pc;                 // sampled trunk timing (az_net_profile)
    long long prof_launches = 0, prof_forwards = 0;
    long long prof_tick = 0, prof_sampled = 0;    // events on every prof_every()-th forward only
    std::mutex mu;
};

// The parameters of the net's canonical blob (net_load.hip: the plain or the rand-wire layout).
size_t net_blob_params(const az_net* n);

// How the forward reads its input planes: the plan's NET_IN_* (net_plan.h).
int net_input_path(const az_net* n);

struct LeafRecs {                 // the search's leaf records: sample b = record gidx[b] (n records)
    const uint8_t* rec; const int* gidx; int go; int n;
    int identity;                 // gidx[b] == b (the identity batch): the fused forward skips that load
};

// Forward of B samples (B = capacity; *nb = active samples, device side) from the
// NHWC16 input x0 -> logits [B][A], value [B].  lr (optional; only where
// net_input_path != NET_IN_GEMM): the planes come from leaf records instead of x0.
int net_forward(az_net* n, const float* x0, int B, const int* nb, float* logits, float* value, hipStream_t st,
                const LeafRecs* lr = nullptr);

// The fp16 range guard's flag of a net (sticky on the device until read here): AZ_ERR_RANGE once set.
int check_ovf(az_net* n, int ovf);
