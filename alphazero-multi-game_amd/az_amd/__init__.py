"""az_amd -- host-side Python mirror of the reference's self-play plugin surface,
over the C-ABI of libaz_hip.so (include/az_engine.h).

Reference surfaces mirrored (paths relative to the reference root):
  HipNeuralNetwork  alphazero::nn::NeuralNetwork  (include/alphazero/nn/neural_network.h:20-132):
                    predict(planes) / predictBatch(planes) with TorchNeuralNetwork::predictBatch
                    semantics (softmax over A, value [B]) (src/nn/torch_neural_network.cpp:224-363)
  ParallelMCTS      alphazero::mcts::ParallelMCTS (include/alphazero/mcts/parallel_mcts.h:131-201),
                    one tree per game, G games per device handle: search(), selectAction(),
                    getActionProbabilities(), getRootValue(), updateWithMove(), addDirichletNoise()
  SelfPlayManager   alphazero::selfplay::SelfPlayManager (src/selfplay/self_play_manager.cpp:47-240):
                    generateGames() with the playSingleGame move loop and temperature schedule.
  Dataset           alphazero::selfplay::Dataset (src/selfplay/dataset.cpp): extractExamples with the
                    8-fold augmentation on device, getBatch, shuffle, getRandomSubset, save/load.
Beyond the reference:
  ReplayBuffer      az_replay_*: a device-resident ring of action-space training targets that self-play
                    fills (ParallelMCTS.attachReplay) and a trainer samples.
"""
import ctypes
from dataclasses import dataclass, field

import numpy as np

from ._lib import (AZ_GO_RULES_SET, AZ_MAX_LEAVES, GomokuRules, AZ_SEL_PROGRESSIVE_BIAS, AZ_SEL_PUCT, AZ_SEL_RAVE, AZ_SEL_UCB, SearchOpts, AZ_EVAL_CALLBACK, AZ_EVAL_HASH, AZ_EVAL_NET, AZ_EVAL_RANDOM, AZ_EVAL_UNIFORM, EVAL_FN, AZ_PREC_BF16, AZ_PREC_BF16X3, AZ_PREC_F16X3, AZ_PREC_F32, AZ_PREC_FP16, AzError,
                   ARENA_SINK, ArenaCfg, ArenaSummary, ReplayCfg, GAME_SINK, PROGRESS_FN, MoveRec as _lib_MoveRec, NetDesc, SearchCfg, SelfPlayCfg, check, lib)

__all__ = ["Engine", "HipNeuralNetwork", "ParallelMCTS", "SelfPlayManager", "Arena", "ArenaGameRecord", "EloRating", "GameRecord", "MoveData", "AzError",
           "Dataset", "TrainingExample", "GAME_GOMOKU", "GAME_GO", "ReplayBuffer", "replay_sym_cell", "replay_sample_plan",
           "AZ_PREC_F32", "AZ_PREC_BF16X3", "AZ_PREC_F16X3", "AZ_PREC_BF16", "AZ_PREC_FP16", "AZ_EVAL_NET", "AZ_EVAL_HASH", "AZ_EVAL_RANDOM", "AZ_EVAL_UNIFORM", "AZ_EVAL_CALLBACK",
           "gomoku_net_desc", "state_dict_blob", "load_openings", "parse_openings"]

_f = ctypes.POINTER(ctypes.c_float)
_i = ctypes.POINTER(ctypes.c_int)


def _fp(a):
    return a.ctypes.data_as(_f)


def _ip(a):
    return a.ctypes.data_as(_i)


class Engine:
    """One HIP device (az_engine_create).  Raises if no GPU is present."""

    def __init__(self, device=0):
        h = ctypes.c_void_p()
        check(lib().az_engine_create(device, ctypes.byref(h)))
        self.h = h

    @property
    def device_name(self):
        buf = ctypes.create_string_buffer(256)
        check(lib().az_engine_device_name(self.h, buf, 256))
        return buf.value.decode()

    def close(self):
        if self.h:
            lib().az_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gomoku_net_desc(board_size=15, channels=256, blocks=20, precision=AZ_PREC_F32, max_batch=256, residual=1,
                    conv_bias=0, in_planes=11, head_channels=32, pool=8, fc_hidden=256):
    """Residual policy/value net of BASELINE.json (C2: 6x64, C3: 20x256) for Gomoku."""
    return NetDesc(board_size, in_planes, channels, blocks, board_size * board_size, head_channels, pool, fc_hidden,
                   residual, conv_bias, precision, max_batch)


def state_dict_blob(state_dict, out=None):
    """The canonical parameter blob of a torch module's state_dict: its entries flattened and concatenated in
    order, num_batches_tracked skipped, as one float32 tensor on the entries' device (or written into `out`, a
    contiguous float32 tensor of that many elements, which is returned).  HipNeuralNetwork.load_weights_device
    takes the result as it is; load_weights takes blob.cpu().numpy().  The module's state_dict must be in
    blob order (conv, BN weight / bias / running_mean / running_var, ... as az_net_num_params counts them)."""
    import torch
    parts = [v for k, v in state_dict.items() if not k.endswith("num_batches_tracked")]
    total = sum(int(v.numel()) for v in parts)
    if out is None:
        out = torch.empty(total, dtype=torch.float32, device=parts[0].device if parts else "cpu")
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != total:
        raise ValueError(f"out: need a contiguous float32 tensor of {total} elements")
    flat, off = out.view(-1), 0
    with torch.no_grad():
        for v in parts:
            n = int(v.numel())
            flat[off:off + n].copy_(v.reshape(-1))
            off += n
    return out


def randwire_net_desc(board_size=15, channels=128, blocks=20, in_planes=11, max_batch=256, action_size=None):
    """DDWRandWireResNet(in_planes, action_size, channels, blocks) of src/nn/ddw_randwire_resnet.cpp:387-468
    (the reference's defaults: 128 channels, 20 blocks; heads 32 channels, 8x8 pool, 256 hidden)."""
    return NetDesc(board_size, in_planes, channels, blocks, action_size or board_size * board_size, 32,
                   min(8, board_size), 256, 0, 0, AZ_PREC_F32, max_batch)


def createDDWRandWireResNet(engine, input_channels, output_size, channels=128, num_blocks=20, board_size=15,
                            max_batch=256):
    """TorchNeuralNetwork::createDDWRandWireResNet (torch_neural_network.cpp:799-814) on the device engine."""
    d = randwire_net_desc(board_size, channels, num_blocks, input_channels, max_batch, output_size)
    return HipNeuralNetwork(engine, d, randwire=True)


def randwire_graph(block):
    """Host-side wiring of rand-wire block `block` (az_randwire_graph): dict like the reference dump."""
    order, topo, ins, outs = ((ctypes.c_int * 32)() for _ in range(4))
    nin, nout = ctypes.c_int(), ctypes.c_int()
    off = (ctypes.c_int * 33)()
    preds = (ctypes.c_int * 256)()
    check(lib().az_randwire_graph(block, order, topo, ins, ctypes.byref(nin), outs, ctypes.byref(nout), off, preds, 256))
    return {"nodes": list(order), "topo": list(topo), "input_nodes": list(ins)[:nin.value],
            "output_nodes": list(outs)[:nout.value], "preds": {v: list(preds[off[v]:off[v + 1]]) for v in range(32)}}


class HipNeuralNetwork:
    """NeuralNetwork plugin on the MI355X ConvNet kernels."""

    def __init__(self, engine, desc, randwire=False, graphs=None):
        """randwire: the DDW-RandWire net with the reference C++ wiring; graphs: explicit wiring per
        block (dicts with "nodes" (registration order), "preds" {node: [...]}, "output_nodes")."""
        self.engine = engine
        self.desc = desc
        h = ctypes.c_void_p()
        if graphs is not None:
            flat = []
            for g in graphs[:desc.blocks]:
                n = len(g["nodes"])
                flat += [n] + list(g["nodes"])
                for v in range(n):
                    p = list(g["preds"][v])
                    flat += [len(p)] + p
                flat += [len(g["output_nodes"])] + list(g["output_nodes"])
            arr = (ctypes.c_int * max(1, len(flat)))(*flat)
            check(lib().az_net_create_randwire_graphs(engine.h, ctypes.byref(desc), arr, len(flat), ctypes.byref(h)))
        else:
            create = lib().az_net_create_randwire if randwire else lib().az_net_create
            check(create(engine.h, ctypes.byref(desc), ctypes.byref(h)))
        self.h = h
        n = ctypes.c_size_t()
        check(lib().az_net_num_params(self.h, ctypes.byref(n)))
        self.num_params = n.value

    def load_weights(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.float32).reshape(-1)
        check(lib().az_net_load_weights(self.h, _fp(blob), blob.size))

    def load_weights_device(self, t):
        """The same load from a contiguous float32 torch tensor of num_params elements on the engine's device
        (az_net_load_weights_device; state_dict_blob makes one): packed by kernels, no host trip.  Waits for
        torch's current stream first -- the engine stream does not order with it -- and returns when the net
        holds the new weights, so `t` may be overwritten."""
        if (not hasattr(t, "data_ptr") or not getattr(t, "is_cuda", False) or str(t.dtype) != "torch.float32"
                or not t.is_contiguous() or t.numel() != self.num_params):
            raise ValueError(f"need a contiguous float32 device tensor of {self.num_params} elements")
        import torch
        torch.cuda.current_stream(t.device).synchronize()
        check(lib().az_net_load_weights_device(self.h, ctypes.c_void_p(t.data_ptr()), t.numel()))

    def init_random(self, seed):
        check(lib().az_net_init_random(self.h, seed))

    def get_weights(self):
        """The loaded weights as the canonical fp32 blob (az_net_get_weights)."""
        blob = np.empty(self.num_params, np.float32)
        check(lib().az_net_get_weights(self.h, _fp(blob), blob.size))
        return blob

    def set_precision(self, precision):
        check(lib().az_net_set_precision(self.h, precision))
        self.desc.precision = precision

    def forward(self, planes):
        """planes [B, C_in, H, W] fp32 -> (logits [B, A], value [B])."""
        x = np.ascontiguousarray(planes, dtype=np.float32)
        B = x.shape[0]
        A = self.desc.action_size
        lo = np.zeros((B, A), np.float32)
        v = np.zeros(B, np.float32)
        check(lib().az_net_forward(self.h, _fp(x), B, _fp(lo), _fp(v)))
        return lo, v

    def predictBatch(self, planes):
        """TorchNeuralNetwork::predictBatch semantics: (softmax policy [B, A], value [B])."""
        x = np.ascontiguousarray(planes, dtype=np.float32)
        B = x.shape[0]
        A = self.desc.action_size
        p = np.zeros((B, A), np.float32)
        v = np.zeros(B, np.float32)
        check(lib().az_net_predict_batch(self.h, _fp(x), B, _fp(p), _fp(v)))
        return p, v

    def predict(self, planes):
        p, v = self.predictBatch(np.asarray(planes, np.float32)[None])
        return p[0], float(v[0])

    def profile(self, enable=True):
        check(lib().az_net_profile(self.h, int(enable)))

    def profile_read(self):
        """(trunk milliseconds, trunk conv launches, forwards) since profile(True)."""
        ms = ctypes.c_double()
        la = ctypes.c_int64()
        fw = ctypes.c_int64()
        check(lib().az_net_profile_read(self.h, ctypes.byref(ms), ctypes.byref(la), ctypes.byref(fw)))
        return ms.value, la.value, fw.value

    def trunk_kernel(self):
        """Name of the HIP kernel the 3x3 trunk convs dispatch at this net's max_batch."""
        buf = ctypes.create_string_buffer(128)
        check(lib().az_net_trunk_kernel(self.h, buf, 128))
        return buf.value.decode()

    def plan(self):
        """Diagnostic: how this net runs at its current precision (input stage, trunk family, tail, head FCs)."""
        buf = ctypes.create_string_buffer(256)
        check(lib().az_diag_net_plan(self.h, buf, 256))
        return buf.value.decode()

    def getBatchSize(self):
        return self.desc.max_batch

    def isGpuAvailable(self):
        return True

    def close(self):
        if self.h:
            lib().az_net_destroy(self.h)
            self.h = None


AZ_GAME_GOMOKU, AZ_GAME_GO, AZ_ACTION_NONE = 0, 1, -2


def _go_rules_fields(game, komi, chinese, superko):
    """az_search_cfg's go_rules / go_komi / go_chinese_rules / go_superko: a Gomoku handle with the
    default rules leaves them zero (the engine refuses any other rules on it)."""
    if game != AZ_GAME_GO and (komi, bool(chinese), bool(superko)) == (7.5, True, True):
        return 0, 0.0, 0, 0
    return AZ_GO_RULES_SET, komi, int(bool(chinese)), int(bool(superko))


SEARCH_OPT_DEFAULTS = dict(selection=AZ_SEL_PUCT, max_search_depth=1000, use_td=False, td_lambda=0.8, use_widening=False,
                           widening_min_visits=10, widening_base=2.0, widening_exponent=0.5)


def _search_opts_struct(opts):
    """az_search_opts from keyword arguments named as SEARCH_OPT_DEFAULTS (MCTSConfig's selectionStrategy,
    maxSearchDepth, useTemporalDifference, tdLambda, useProgressiveWidening, minVisitsForWidening,
    progressiveWideningBase / Exponent); the ones not named take their defaults."""
    unknown = set(opts) - set(SEARCH_OPT_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown search options {sorted(unknown)}")
    o = dict(SEARCH_OPT_DEFAULTS, **opts)
    return SearchOpts(int(o["selection"]), int(o["max_search_depth"]), int(bool(o["use_td"])), float(o["td_lambda"]),
                      int(bool(o["use_widening"])), int(o["widening_min_visits"]), float(o["widening_base"]),
                      float(o["widening_exponent"]))


def widening_table(base, exponent, n_actions):
    """The progressive-widening counts by visit count the device reads (az_search_widening_table;
    host only): the whole table as an int32 array."""
    n = ctypes.c_int()
    check(lib().az_search_widening_table(base, exponent, n_actions, None, 0, ctypes.byref(n)))
    out = np.zeros(n.value, np.int32)
    check(lib().az_search_widening_table(base, exponent, n_actions, _ip(out), out.size, ctypes.byref(n)))
    return out


def parse_openings(text, name="<openings>"):
    """An openings file as a list of move sequences: one opening per line, whitespace-separated actions (Go's
    pass is -1), `#` starts a comment, blank lines are ignored.  A malformed line raises ValueError with the
    file's name and the line's number."""
    book = []
    for no, line in enumerate(text.splitlines(), 1):
        words = line.split("#", 1)[0].split()
        if not words:
            continue
        try:
            seq = [int(w, 10) for w in words]
        except ValueError:
            raise ValueError(f"{name}:{no}: not a list of actions: {line.strip()!r}") from None
        if min(seq) < -1:
            raise ValueError(f"{name}:{no}: action {min(seq)} (the smallest is -1, Go's pass)")
        book.append(seq)
    return book


def load_openings(path):
    """parse_openings of a file: the sequences ParallelMCTS.new_games_moves takes."""
    with open(path) as f:
        return parse_openings(f.read(), str(path))


class ParallelMCTS:
    """G independent ParallelMCTS trees (Mode S semantics, setDeterministicMode) on one device."""

    def __init__(self, engine, n_games=1, board_size=15, num_simulations=800, c_puct=1.5, fpu_reduction=0.0,
                 virtual_loss=3, evaluator=AZ_EVAL_HASH, net=None, eval_seed=7, zobrist_seed=12345, noise_seed=42,
                 noise_seed_stride=0, use_dirichlet_each_search=False, dirichlet_alpha=0.03, dirichlet_eps=0.25,
                 tt_log2=20, node_capacity=0, prior_ring=0, game=0, callback=None, go_komi=7.5, go_chinese_rules=True,
                 go_superko=True, gomoku_renju=False, gomoku_omok=False, leaves=1, **search_opts):
        """game: AZ_GAME_GOMOKU (0) or AZ_GAME_GO (1) -- GoState(bs 9/13/19, go_komi, go_chinese_rules,
        go_superko), fixed for the handle's life; Go actions are -1 (pass) .. bs*bs-1 and finished games
        report AZ_ACTION_NONE.
        gomoku_renju / gomoku_omok: GomokuState(bs, use_renju, use_omok), put in force right after creation
        (az_search_set_gomoku_rules) for every game the handle plays; gomokuRules() reads them back.
        search_opts: selection (AZ_SEL_*), max_search_depth, use_td, td_lambda, use_widening,
        widening_min_visits, widening_base, widening_exponent (SEARCH_OPT_DEFAULTS), put in force right
        after creation (az_search_set_options); setSearchOptions changes them on the live handle.
        leaves: leaf parallelism K (az_search_set_leaves; setLeafParallelism changes it between searches): a
        simulation step makes K descents per game and evaluates their leaves as one batch of up to n_games x K.
        evaluator=AZ_EVAL_CALLBACK: callback(games [n], moves: per leaf the moves from the empty board,
        planes [n][C][bs][bs]) -> (policy [n][NA] as NeuralNetwork::predict returns it, value [n])."""
        self.G = n_games
        self.bs = board_size
        self.game = game
        self.A = board_size * board_size + (1 if game == AZ_GAME_GO else 0)     # action space
        self.none = AZ_ACTION_NONE if game == AZ_GAME_GO else -1
        cfg = SearchCfg(n_games, board_size, num_simulations, c_puct, fpu_reduction, virtual_loss, evaluator,
                        eval_seed, zobrist_seed, noise_seed, noise_seed_stride, int(use_dirichlet_each_search),
                        dirichlet_alpha, dirichlet_eps, tt_log2, node_capacity, prior_ring, game,
                        *_go_rules_fields(game, go_komi, go_chinese_rules, go_superko))
        self.cfg = cfg
        opts = _search_opts_struct(search_opts)
        h = ctypes.c_void_p()
        check(lib().az_search_create(engine.h, net.h if net is not None else None, ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        try:
            if search_opts:
                check(lib().az_search_set_options(h, ctypes.byref(opts)))
            if gomoku_renju or gomoku_omok:
                check(lib().az_search_set_gomoku_rules(h, ctypes.byref(GomokuRules(int(bool(gomoku_renju)), int(bool(gomoku_omok)), 0))))
            if leaves != 1:
                check(lib().az_search_set_leaves(h, int(leaves)))
        except AzError:
            self.close()
            raise
        self.engine, self.net = engine, net
        self._cb = None
        if evaluator == AZ_EVAL_CALLBACK:
            if callback is None:
                raise ValueError("AZ_EVAL_CALLBACK needs a callback")
            NA = self.A

            def _eval(_user, n, games, plen, moves, max_path, planes, n_planes, pol, val):
                try:
                    g = np.ctypeslib.as_array(games, shape=(n,)).copy()
                    ln = np.ctypeslib.as_array(plen, shape=(n,))
                    mv = np.ctypeslib.as_array(moves, shape=(n, max_path))
                    x = np.ctypeslib.as_array(planes, shape=(n, n_planes, board_size, board_size)).copy()
                    p, v = callback(g, [mv[i, :ln[i]].tolist() for i in range(n)], x)
                    p = np.ascontiguousarray(p, np.float32).reshape(n, NA)
                    v = np.ascontiguousarray(v, np.float32).reshape(n)
                    ctypes.memmove(pol, p.ctypes.data, p.nbytes)
                    ctypes.memmove(val, v.ctypes.data, v.nbytes)
                    return 0
                except Exception as e:  # surfaced as AZ_ERR_STATE
                    print("az_amd evaluator failed:", repr(e))
                    return 1

            self._cb = EVAL_FN(_eval)
            check(lib().az_search_set_evaluator(self.h, self._cb, None))

    def newGames(self, games=None, ids=None):
        """Start fresh games in the listed slots (all by default).  ids: each game's stream id for its
        evaluator / noise seeds (az_search_new_games_ids; default the slot index)."""
        games = np.arange(self.G, dtype=np.int32) if games is None else np.ascontiguousarray(games, np.int32)
        if ids is None:
            check(lib().az_search_new_games(self.h, _ip(games), games.size))
        else:
            ids = np.ascontiguousarray(ids, np.int32)
            assert ids.size == games.size
            check(lib().az_search_new_games_ids(self.h, games.ctypes.data, ids.ctypes.data, games.size))

    def new_games_moves(self, sequences, games=None, ids=None):
        """Fresh games in the listed slots (all by default), slot games[i] advanced by sequences[i] -- a list of
        actions, Go's pass is -1 -- in one launch (az_search_new_games_moves): the handle as after newGames on
        the same slots and ids and one updateWithMove per move.  An illegal move anywhere raises AzError
        (AZ_ERR_ARG, naming the entry, the ply and the reason) and leaves the handle as it was."""
        games = np.arange(self.G, dtype=np.int32) if games is None else np.ascontiguousarray(games, np.int32)
        seqs = [np.asarray(q, np.int32).reshape(-1) for q in sequences]
        if len(seqs) != games.size:
            raise ValueError(f"{len(seqs)} sequences for {games.size} slots")
        stride = max([q.size for q in seqs] + [1])
        mv = np.full((max(1, len(seqs)), stride), AZ_ACTION_NONE, np.int32)
        nm = np.zeros(max(1, len(seqs)), np.int32)
        for i, q in enumerate(seqs):
            mv[i, :q.size] = q
            nm[i] = q.size
        if ids is not None:
            ids = np.ascontiguousarray(ids, np.int32)
            assert ids.size == games.size
        check(lib().az_search_new_games_moves(self.h, games.ctypes.data, ids.ctypes.data if ids is not None else None,
                                              games.size, mv.ctypes.data, nm.ctypes.data, stride))

    def setOpenings(self, book=None, random_plies=0, seed=0):
        """The openings of the games the drivers start on this handle (az_search_set_openings): game `id` begins
        with book[id % len(book)] -- book: a list of move sequences, e.g. load_openings(path) -- then plays up to
        random_plies plies drawn on the device from the Philox stream (seed, id).  No book and no random plies:
        empty-board starts again.  newGames / new_games_moves are not affected."""
        from ._lib import OpeningsCfg
        seqs = [np.asarray(q, np.int32).reshape(-1) for q in (book or [])]
        if not seqs and not random_plies:
            check(lib().az_search_set_openings(self.h, None))
            return
        stride = max([q.size for q in seqs] + [1])
        mv = np.full((max(1, len(seqs)), stride), AZ_ACTION_NONE, np.int32)
        nm = np.zeros(max(1, len(seqs)), np.int32)
        for i, q in enumerate(seqs):
            mv[i, :q.size] = q
            nm[i] = q.size
        cfg = OpeningsCfg(_ip(mv), _ip(nm), len(seqs), stride, int(random_plies), int(seed) & (2 ** 64 - 1))
        check(lib().az_search_set_openings(self.h, ctypes.byref(cfg)))

    def openings(self):
        """(book size, random plies, seed) in force (az_search_openings); (0, 0, 0) with none."""
        n, r, sd = ctypes.c_int(), ctypes.c_int(), ctypes.c_uint64()
        check(lib().az_search_openings(self.h, ctypes.byref(n), ctypes.byref(r), ctypes.byref(sd)))
        return n.value, r.value, sd.value

    def setNet(self, net):
        """ParallelMCTS::setNeuralNetwork on every slot (az_search_set_net); ends per-slot nets."""
        check(lib().az_search_set_net(self.h, net.h))
        self.net, self._slot_nets = net, None

    def setSlotNets(self, nets, slot_net):
        """Slot g is evaluated by nets[slot_net[g]] from the next search on (az_search_set_slot_nets):
        up to 4 nets of the handle's shape, each with max_batch >= its number of slots."""
        sn = np.ascontiguousarray(slot_net, dtype=np.uint8).reshape(-1)
        if sn.size != self.G:
            raise ValueError(f"slot_net holds {sn.size} entries, the handle has {self.G} slots")
        arr = (ctypes.c_void_p * max(1, len(nets)))(*[n.h.value for n in nets])
        check(lib().az_search_set_slot_nets(self.h, arr, len(nets), sn.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        self._slot_nets = list(nets)      # kept alive with the handle

    def addDirichletNoise(self, alpha=0.03, epsilon=0.25, mask=None):
        if mask is None:
            check(lib().az_search_add_noise(self.h, alpha, epsilon))
        else:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            check(lib().az_search_add_noise_masked(self.h, alpha, epsilon,
                                                   m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))

    def search(self, mask=None):
        """One search of every playing game; mask [G]: only of the games it marks (az_search_run_masked),
        the other trees untouched."""
        if mask is None:
            check(lib().az_search_run(self.h))
        else:
            m = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.G)
            check(lib().az_search_run_masked(self.h, m.ctypes.data))

    def runSingleSimulation(self, n=1):
        """ParallelMCTS::runSingleSimulation (parallel_mcts.cpp:276-380), n times, every game."""
        check(lib().az_search_simulate(self.h, int(n)))

    def runBatchedSearch(self):
        """ParallelMCTS::runBatchedSearch (parallel_mcts.cpp:1531-1590): numSimulations single simulations."""
        check(lib().az_search_simulate(self.h, self.cfg.num_simulations))

    def releaseMemory(self, visitThreshold=10):
        """ParallelMCTS::releaseMemory (parallel_mcts.cpp:1481-1496): nodes pruned per game."""
        out = np.zeros(self.G, np.int64)
        check(lib().az_search_release(self.h, int(visitThreshold), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return out

    def selectActionFor(self, game, isTraining=False, temperature=1.0, legal=(), useBatchInference=True):
        """ParallelMCTS::selectAction of one game (parallel_mcts.cpp:987-1047); with useBatchInference
        off it draws on the game's rng_ (libstdc++ discrete / uniform_int distributions).  legal: the
        root state's getLegalMoves(), used when the root has no children."""
        lg = np.ascontiguousarray(legal, np.int32)
        a = ctypes.c_int()
        check(lib().az_search_select_action(self.h, int(game), int(bool(isTraining)), float(temperature),
                                            int(bool(useBatchInference)), _ip(lg), int(lg.size), ctypes.byref(a)))
        return a.value

    def select(self, is_training=True, temperature=1.0, mask=None):
        """(actions [G], root values [G], probs [G][A] child order, child actions [G][A], n_children [G]).
        mask [G]: the games outside it report no action (-1, Go: AZ_ACTION_NONE) and no children."""
        G, A = self.G, self.A
        act = np.zeros(G, np.int32)
        val = np.zeros(G, np.float32)
        probs = np.zeros((G, A), np.float32)
        cact = np.zeros((G, A), np.int32)
        nch = np.zeros(G, np.int32)
        check(lib().az_search_select(self.h, int(is_training), temperature, _ip(act), _fp(val), _fp(probs), _ip(cact),
                                     _ip(nch)))
        if mask is not None:
            off = ~np.asarray(mask, bool).reshape(G)
            act[off] = self.none
            nch[off] = 0
        return act, val, probs, cact, nch

    def selectAction(self, isTraining=False, temperature=1.0):
        return self.select(isTraining, temperature)[0]

    def getActionProbabilities(self, temperature=1.0):
        _, _, probs, _, nch = self.select(True, temperature)
        return [probs[g, :nch[g]].copy() for g in range(self.G)]

    def getRootValue(self):
        return self.select(True, 1.0)[1]

    def updateWithMove(self, actions):
        a = np.ascontiguousarray(actions, dtype=np.int32).reshape(self.G)
        term = np.zeros(self.G, np.int32)
        res = np.zeros(self.G, np.int32)
        check(lib().az_search_apply(self.h, _ip(a), _ip(term), _ip(res)))
        return term, res

    def rootChildren(self, game):
        A = self.A
        act = np.zeros(A, np.int32)
        N = np.zeros(A, np.int32)
        VL = np.zeros(A, np.int32)
        W = np.zeros(A, np.float32)
        Pp = np.zeros(A, np.float32)
        n = ctypes.c_int()
        check(lib().az_search_root_children(self.h, game, _ip(act), _ip(N), _ip(VL), _fp(W), _fp(Pp), ctypes.byref(n)))
        k = n.value
        return act[:k], N[:k], VL[:k], W[:k], Pp[:k]

    def goRules(self):
        """(komi, chinese_rules, superko) the handle plays (az_search_go_rules)."""
        k, c, sk = ctypes.c_float(), ctypes.c_int(), ctypes.c_int()
        check(lib().az_search_go_rules(self.h, ctypes.byref(k), ctypes.byref(c), ctypes.byref(sk)))
        return k.value, bool(c.value), bool(sk.value)

    def gomokuRules(self):
        """(renju, omok) the handle plays (az_search_gomoku_rules)."""
        r = GomokuRules()
        check(lib().az_search_gomoku_rules(self.h, ctypes.byref(r)))
        return bool(r.renju), bool(r.omok)

    def searchOptions(self):
        """The search options the handle plays (az_search_options), keyed as SEARCH_OPT_DEFAULTS."""
        o = SearchOpts()
        check(lib().az_search_options(self.h, ctypes.byref(o)))
        return dict(selection=o.selection, max_search_depth=o.max_search_depth, use_td=bool(o.use_td), td_lambda=o.td_lambda,
                    use_widening=bool(o.use_widening), widening_min_visits=o.widening_min_visits,
                    widening_base=o.widening_base, widening_exponent=o.widening_exponent)

    def setSearchOptions(self, **search_opts):
        """setSelectionStrategy / setConfig on the live handle, trees kept (az_search_set_options): the
        options named change, the others stay as they are."""
        opts = _search_opts_struct(dict(self.searchOptions(), **search_opts))
        check(lib().az_search_set_options(self.h, ctypes.byref(opts)))

    def setLeafParallelism(self, leaves):
        """K descents per game and simulation step, their leaves one evaluator batch (az_search_set_leaves);
        between searches, trees kept."""
        check(lib().az_search_set_leaves(self.h, int(leaves)))

    def getLeafParallelism(self):
        k = ctypes.c_int()
        check(lib().az_search_leaves(self.h, ctypes.byref(k)))
        return k.value

    def rootNode(self, game):
        N = ctypes.c_int()
        VL = ctypes.c_int()
        W = ctypes.c_float()
        check(lib().az_search_root_node(self.h, game, ctypes.byref(N), ctypes.byref(VL), ctypes.byref(W)))
        return N.value, VL.value, W.value

    def counters(self, game):
        out = (ctypes.c_int64 * 5)()
        check(lib().az_search_counters(self.h, game, out))
        return dict(zip(("evals", "tt_lookups", "tt_hits", "sims", "nodes"), list(out)))

    def enableEvalLog(self, game, capacity):
        check(lib().az_search_enable_eval_log(self.h, game, capacity))

    def readEvalLog(self, capacity):
        A = self.A
        pol = np.zeros((capacity, A), np.float32)
        val = np.zeros(capacity, np.float32)
        planes = np.zeros((capacity, 8 if self.game == AZ_GAME_GO else 11, self.bs, self.bs), np.float32)
        n = ctypes.c_int()
        check(lib().az_search_read_eval_log(self.h, _fp(pol), _fp(val), _fp(planes), ctypes.byref(n)))
        k = n.value
        return pol[:k], val[:k], planes[:k]

    def profile(self, enable=True):
        """Start (reset) / stop tree-kernel timing and byte counting (az_search_profile)."""
        check(lib().az_search_profile(self.h, int(enable)))

    def profile_read(self):
        """dict(select_ms, expand_ms, sim_steps, select_bytes, expand_bytes, fused_ms, fused_launches) since
        profile(True): the split kernels of the sampled steps, the fused k_expand_select of the others."""
        a, b = ctypes.c_double(), ctypes.c_double()
        n, sb, eb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        check(lib().az_search_profile_read(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n), ctypes.byref(sb),
                                           ctypes.byref(eb)))
        f, fl = ctypes.c_double(), ctypes.c_int64()
        check(lib().az_search_profile_read_fused(self.h, ctypes.byref(f), ctypes.byref(fl)))
        return {"select_ms": a.value, "expand_ms": b.value, "sim_steps": n.value, "select_bytes": sb.value,
                "expand_bytes": eb.value, "fused_ms": f.value, "fused_launches": fl.value}

    def tree_evictions(self):
        """Diagnostic: TreeDev slot evictions so far (each one a stream synchronisation)."""
        f = lib().az_diag_tree_evictions
        f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_void_p]
        return int(f(self.h))

    def selfplayStep(self, temp_drop_move=30, t_init=1.0, t_final=0.0, restart_finished=True):
        cfg = SelfPlayCfg(temp_drop_move, t_init, t_final, int(restart_finished))
        moves = ctypes.c_int64(0)
        evals = ctypes.c_int64(0)
        check(lib().az_selfplay_step(self.h, ctypes.byref(cfg), ctypes.byref(moves), ctypes.byref(evals)))
        return moves.value, evals.value

    def stepMoves(self, materialize=True):
        """MoveData of the last selfplayStep: [(slot, MoveData)] for every game that moved.
        materialize=False returns the engine's own records as they are (the C++-assembled
        az_move_rec array, as a numpy structured view valid until the next step, and the slots)
        without building Python objects."""
        mv = ctypes.POINTER(_lib_MoveRec)()
        sl = ctypes.POINTER(ctypes.c_int)()
        n = ctypes.c_int()
        check(lib().az_selfplay_step_moves(self.h, ctypes.byref(mv), ctypes.byref(sl), ctypes.byref(n)))
        if not materialize:
            if n.value == 0:
                return None, None
            import numpy as np
            R = _lib_MoveRec
            dt = np.dtype({"names": ["action", "value", "n_children", "policy", "child_actions", "thinking_time_ms"],
                           "formats": ["<i4", "<f4", "<i4", "<u8", "<u8", "<i8"],
                           "offsets": [R.action.offset, R.value.offset, R.n_children.offset, R.policy.offset,
                                       R.child_actions.offset, R.thinking_time_ms.offset],
                           "itemsize": ctypes.sizeof(R)})
            raw = (ctypes.c_char * (n.value * ctypes.sizeof(R))).from_address(ctypes.addressof(mv.contents))
            return np.frombuffer(raw, dtype=dt), np.ctypeslib.as_array(sl, shape=(n.value,))
        out = []
        for i in range(n.value):
            r = mv[i]
            k = r.n_children
            # pointer slices copy the k entries in one C-level call (per-element indexing is ~8 ms/move at C2)
            out.append((int(sl[i]), MoveData(int(r.action), r.policy[:k], float(r.value),
                                             int(r.thinking_time_ms), r.child_actions[:k])))
        return out

    def attachReplay(self, rb):
        """az_search_attach_replay: selfplayStep / az_selfplay_run stage every position they move from into
        `rb` and commit finished games; None detaches.  Staged positions are discarded either way."""
        check(lib().az_search_attach_replay(self.h, rb.h if rb is not None else None))
        self._replay = rb      # kept alive with the handle

    def close(self):
        if self.h:
            if not getattr(self, "_borrowed", False):
                lib().az_search_destroy(self.h)
            self.h = None


@dataclass
class MoveData:
    """include/alphazero/selfplay/game_record.h:21-33 (policy in CHILD order, not action-indexed;
    child_actions holds the matching actions, an extension the reference does not record)."""
    action: int
    policy: list
    value: float
    thinking_time_ms: int = 0
    child_actions: list = field(default_factory=list)


@dataclass
class GameRecord:
    board_size: int
    moves: list = field(default_factory=list)
    result: int = 0
    game_id: int = -1


class SelfPlayManager:
    """SelfPlayManager::generateGames over G device-resident games (playSingleGame loop,
    self_play_manager.cpp:151-234): initial noise, search, T = initial until
    temperatureDropMove then final, selectAction(true, T), record, makeMove +
    updateWithMove, noise after every even ply."""

    def __init__(self, engine, net=None, numGames=1, numSimulations=800, board_size=15, evaluator=None, **mcts_kw):
        ev = evaluator if evaluator is not None else (AZ_EVAL_NET if net is not None else AZ_EVAL_HASH)
        if mcts_kw.get("selection") == AZ_SEL_UCB:      # playSingleGame turns UCB into PUCT (self_play_manager.cpp:180-181)
            mcts_kw = dict(mcts_kw, selection=AZ_SEL_PUCT)
        self.mcts = ParallelMCTS(engine, n_games=numGames, board_size=board_size, num_simulations=numSimulations,
                                 evaluator=ev, net=net, **mcts_kw)
        self.numGames = numGames
        self.dirichletAlpha, self.dirichletEpsilon = 0.03, 0.25
        self.initialTemperature, self.temperatureDropMove, self.finalTemperature = 1.0, 30, 0.0
        self.progressCallback = None

    def setExplorationParams(self, dirichletAlpha, dirichletEpsilon, initialTemperature, temperatureDropMove,
                             finalTemperature):
        self.dirichletAlpha, self.dirichletEpsilon = dirichletAlpha, dirichletEpsilon
        self.initialTemperature, self.temperatureDropMove = initialTemperature, temperatureDropMove
        self.finalTemperature = finalTemperature

    def setProgressCallback(self, cb):
        self.progressCallback = cb

    def setOpenings(self, book=None, random_plies=0, seed=0):
        """Every game generateGames starts begins with an opening (ParallelMCTS.setOpenings); its plies head the
        game's record as MoveData with an empty policy."""
        self.mcts.setOpenings(book, random_plies, seed)

    def getTemperature(self, moveNum):
        return self.finalTemperature if moveNum >= self.temperatureDropMove else self.initialTemperature

    def generateGames(self, totalGames=None, max_moves=0, abort=None):
        """SelfPlayManager::generateGames through the engine's device driver (az_selfplay_run):
        totalGames games (default numGames) on the handle's slots; returns GameRecords by game id."""
        total = self.numGames if totalGames is None else int(totalGames)
        recs = [None] * total

        def sink(_user, gid, bs, n, moves, result):
            r = GameRecord(bs, result=int(result), game_id=int(gid))
            for i in range(n):
                mv = moves[i]
                k = mv.n_children
                r.moves.append(MoveData(int(mv.action), [float(mv.policy[j]) for j in range(k)], float(mv.value),
                                        int(mv.thinking_time_ms), [int(mv.child_actions[j]) for j in range(k)]))
            recs[gid] = r

        def progress(_user, gid, move, tg, tm):
            if self.progressCallback:
                self.progressCallback(int(gid), int(move), int(tg), int(tm))

        cfg = SelfPlayCfg(self.temperatureDropMove, self.initialTemperature, self.finalTemperature, 0)
        flag = ctypes.c_int(0) if abort is None else abort
        cb_sink, cb_prog = GAME_SINK(sink), PROGRESS_FN(progress)
        check(lib().az_selfplay_run(self.mcts.h, ctypes.byref(cfg), total, int(max_moves), cb_sink, cb_prog, None,
                                    ctypes.byref(flag)))
        return recs

    def generateGamesStepwise(self, max_moves=1 << 30, on_move=None):
        """The playSingleGame loop driven from the host through the per-call C-ABI (search /
        select / apply / noise), all numGames games in lock step -- the cross-check for
        generateGames."""
        m = self.mcts
        G = self.numGames
        m.newGames()
        m.addDirichletNoise(self.dirichletAlpha, self.dirichletEpsilon)
        records = [GameRecord(m.bs) for _ in range(G)]
        live = np.ones(G, bool)
        move = 0
        while live.any() and move < max_moves:
            m.search()
            T = self.getTemperature(move)
            act, val, probs, cact, nch = m.select(True, T)
            if on_move is not None:
                on_move(move, m)
            for g in range(G):
                if live[g]:
                    records[g].moves.append(MoveData(int(act[g]), probs[g, :nch[g]].tolist(), float(val[g]), 0,
                                                     cact[g, :nch[g]].tolist()))
                    if self.progressCallback:
                        self.progressCallback(g, move, G, move * G)
            act = np.where(live, act, -1).astype(np.int32)
            term, res = m.updateWithMove(act)
            for g in range(G):
                if live[g] and term[g]:
                    records[g].result = int(res[g])
                    live[g] = False
            if move % 2 == 0:
                m.addDirichletNoise(self.dirichletAlpha, self.dirichletEpsilon)
            move += 1
        return records


# ---------------------------------------------------------------------------- Arena
class EloRating:
    """python/alphazero/utils/elo.py EloRating (ratings in doubles through az_elo_update)."""

    def __init__(self, initial_rating=1500.0, k_factor=32.0):
        self.initial_rating, self.k_factor = float(initial_rating), float(k_factor)
        self.ratings = {}

    def getRating(self, player_id):
        return self.ratings.get(player_id, self.initial_rating)

    def addGameResult(self, player_id, opponent_id, score):
        a, b = ctypes.c_double(self.getRating(player_id)), ctypes.c_double(self.getRating(opponent_id))
        lib().az_elo_update(ctypes.byref(a), ctypes.byref(b), float(score), self.k_factor)
        self.ratings[player_id], self.ratings[opponent_id] = a.value, b.value
        return a.value


@dataclass
class ArenaGameRecord:
    """One finished arena game: moves as MoveData (root value and child-order visit distribution of the
    mover's tree), movers[i] 0 (net A) or 1 (net B), result a GameResult (0: cut at max_moves), score_a."""
    game_id: int
    board_size: int
    a_is_player1: bool
    moves: list
    movers: list
    result: int
    score_a: float
    evals_a: int = 0
    evals_b: int = 0


class Arena:
    """Net A against net B on `tables` boards in lock step (az_arena_*): the game loop of the reference's
    python/scripts/evaluate.py on one search handle whose slots 2i / 2i + 1 are A's / B's tree of table i."""

    def __init__(self, engine, net_a, net_b, tables, board_size=15, num_simulations=800, swap_colors=False,
                 temperature=0.1, sample_moves=0, noise_alpha=0.03, noise_eps=0.0, game=0, c_puct=1.5,
                 fpu_reduction=0.0, virtual_loss=3, zobrist_seed=12345, noise_seed=42, noise_seed_stride=1, tt_log2=20,
                 node_capacity=0, prior_ring=0, go_komi=7.5, go_chinese_rules=True, go_superko=True, gomoku_renju=False,
                 gomoku_omok=False, **search_opts):
        """search_opts: the search options of ParallelMCTS (SEARCH_OPT_DEFAULTS), played by both nets' trees.
        gomoku_renju / gomoku_omok: the Gomoku rule variant, set on the arena's handle right after creation."""
        self.tables, self.engine, self.nets = int(tables), engine, (net_a, net_b)
        self.cfg = SearchCfg(self.tables, board_size, num_simulations, c_puct, fpu_reduction, virtual_loss, AZ_EVAL_NET,
                             7, zobrist_seed, noise_seed, noise_seed_stride, 0, noise_alpha, noise_eps, tt_log2,
                             node_capacity, prior_ring, game,
                             *_go_rules_fields(game, go_komi, go_chinese_rules, go_superko))
        opts = _search_opts_struct(search_opts)
        self.acfg = ArenaCfg(int(bool(swap_colors)), temperature, int(sample_moves), noise_alpha, noise_eps)
        h = ctypes.c_void_p()
        check(lib().az_arena_create(engine.h, net_a.h, net_b.h, ctypes.byref(self.cfg), ctypes.byref(self.acfg),
                                    ctypes.byref(h)))
        self.h = h
        # the underlying handle as a ParallelMCTS view (rootChildren, counters, the evaluation log); not owned
        m = ParallelMCTS.__new__(ParallelMCTS)
        m.G, m.bs, m.game = 2 * self.tables, board_size, game
        m.A = board_size * board_size + (1 if game == AZ_GAME_GO else 0)
        m.none = AZ_ACTION_NONE if game == AZ_GAME_GO else -1
        m.h = ctypes.c_void_p(lib().az_arena_search(self.h))
        m.engine, m.net, m._cb, m._borrowed, m.cfg = engine, net_a, None, True, self.cfg
        self.search = m
        self.progressCallback = None
        try:
            if search_opts:                                   # both nets' trees: every slot of the arena's handle
                check(lib().az_search_set_options(m.h, ctypes.byref(opts)))
            if gomoku_renju or gomoku_omok:
                check(lib().az_search_set_gomoku_rules(m.h, ctypes.byref(GomokuRules(int(bool(gomoku_renju)), int(bool(gomoku_omok)), 0))))
        except AzError:
            self.close()
            raise

    def step(self):
        """One ply on every live table; returns the moves played."""
        n = ctypes.c_int64(0)
        check(lib().az_arena_step(self.h, ctypes.byref(n)))
        return n.value

    def setOpenings(self, book=None, random_plies=0, seed=0):
        """Every game begins with an opening, both trees of its table alike (ParallelMCTS.setOpenings on the
        arena's handle); with swap_colors games 2k and 2k + 1 play opening k with the colours swapped."""
        self.search.setOpenings(book, random_plies, seed)

    def tableGames(self):
        """The game id each table plays now (-1: idle)."""
        ids = np.zeros(self.tables, np.int32)
        check(lib().az_arena_table_games(self.h, _ip(ids)))
        return ids.tolist()

    def run(self, total_games, max_moves=0, abort=None):
        """total_games games from fresh tables; returns their ArenaGameRecords by game id.
        progressCallback(game_id, ply, total_games, total_moves), when set, is called for every move after
        it is chosen and before it is applied."""
        recs = [None] * int(total_games)

        def sink(_user, gp):
            g = gp.contents
            moves = []
            for i in range(g.n_moves):
                mv = g.moves[i]
                k = mv.n_children
                moves.append(MoveData(int(mv.action), mv.policy[:k], float(mv.value), int(mv.thinking_time_ms),
                                      mv.child_actions[:k]))
            recs[g.game_id] = ArenaGameRecord(int(g.game_id), int(g.board_size), bool(g.a_is_player1), moves,
                                              [int(g.mover[i]) for i in range(g.n_moves)], int(g.result),
                                              float(g.score_a), int(g.evals_a), int(g.evals_b))

        def progress(_user, gid, move, tg, tm):
            if self.progressCallback:
                self.progressCallback(int(gid), int(move), int(tg), int(tm))

        flag = ctypes.c_int(0) if abort is None else abort
        cb_sink, cb_prog = ARENA_SINK(sink), PROGRESS_FN(progress)
        check(lib().az_arena_run(self.h, int(total_games), int(max_moves), cb_sink, cb_prog, None, ctypes.byref(flag)))
        return recs

    def summary(self):
        """dict(games, wins_a, wins_b, draws, moves, evals_a, evals_b, elo_a, elo_b) of the games finished since
        the last run() began."""
        out = ArenaSummary()
        check(lib().az_arena_summary_read(self.h, ctypes.byref(out)))
        return {n: getattr(out, n) for n, _ in ArenaSummary._fields_}

    def close(self):
        if self.h:
            self.search.close()
            lib().az_arena_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------------------- Dataset (row f3)
GAME_GOMOKU, GAME_GO = 0, 1
_i64 = ctypes.POINTER(ctypes.c_int64)


def _json_number(x):
    """nlohmann::json's text for a float widened to double: shortest round-trip digits, NaN as null."""
    v = float(x)
    if v != v or v in (float("inf"), float("-inf")):
        return "null"
    return repr(v)


@dataclass
class TrainingExample:
    """selfplay::TrainingExample (include/alphazero/selfplay/dataset.h:21-28): state [planes][bs][bs],
    policy (the record's child-order visit distribution), value."""
    state: np.ndarray
    policy: np.ndarray
    value: float

    def toJson(self):
        # TrainingExample::toJson (src/selfplay/dataset.cpp:16-33): j.dump(), keys sorted
        st = "[" + ",".join("[" + ",".join("[" + ",".join(_json_number(v) for v in row) + "]" for row in pl) + "]"
                            for pl in np.asarray(self.state)) + "]"
        pol = "[" + ",".join(_json_number(v) for v in np.asarray(self.policy)) + "]"
        return '{"policy":' + pol + ',"state":' + st + ',"value":' + _json_number(self.value) + "}"

    @staticmethod
    def fromJson(s):
        import json
        j = json.loads(s) if isinstance(s, str) else s
        nan = float("nan")
        state = np.array([[[nan if v is None else v for v in row] for row in pl] for pl in j["state"]], np.float32)
        policy = np.array([nan if v is None else v for v in j["policy"]], np.float32)
        return TrainingExample(state, policy, float(nan if j["value"] is None else j["value"]))


class Dataset:
    """selfplay::Dataset (include/alphazero/selfplay/dataset.h:33-118, src/selfplay/dataset.cpp) over a
    device-resident example store (az_dataset_*): extractExamples replays every record on the GPU and
    writes each position's examples (original + 7 symmetries) straight into their shuffled slots;
    getBatch / getRandomSubset / shuffle are device gathers.  rng_ is the handle's std::mt19937,
    seeded from std::random_device as the reference does unless `seed` is given."""

    def __init__(self, engine, game_type=GAME_GOMOKU, board_size=15, seed=None):
        h = ctypes.c_void_p()
        check(lib().az_dataset_create(engine.h, int(game_type), int(board_size), ctypes.byref(h)))
        self.h = h
        self.engine = engine
        self.game_type, self.bs = int(game_type), int(board_size)
        if seed is not None:
            check(lib().az_dataset_seed(self.h, int(seed) & 0xFFFFFFFF))
        n, c, b, st = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib().az_dataset_info(self.h, ctypes.byref(n), ctypes.byref(c), ctypes.byref(b), ctypes.byref(st)))
        self.planes, self.policy_stride = c.value, st.value
        self.gameRecords = []

    def addGameRecord(self, record, useEnhancedFeatures=True):
        if record.board_size != self.bs:
            raise ValueError(f"record board {record.board_size} != dataset board {self.bs}")
        self.gameRecords.append(record)

    def _order(self, n):
        out = np.empty(n, np.int64)
        check(lib().az_dataset_shuffle_order(self.h, int(n), out.ctypes.data_as(_i64)))
        return out

    def extractExamples(self, includeAugmentations=True, shuffle=True):
        """Dataset::extractExamples (dataset.cpp:60-114); shuffle=False keeps the pre-shuffle order
        (record order, per position the original then augmentExample's 7)."""
        recs = self.gameRecords
        n_moves = np.array([len(r.moves) for r in recs], np.int32)
        actions = np.array([m.action for r in recs for m in r.moves], np.int32)
        nch = np.array([len(m.policy) for r in recs for m in r.moves], np.int32)
        pols = [np.asarray(m.policy, np.float32) for r in recs for m in r.moves]
        pol = np.concatenate(pols) if pols else np.zeros(0, np.float32)
        res = np.array([r.result for r in recs], np.int32)
        E = int(n_moves.sum()) * (8 if includeAugmentations else 1)
        order = self._order(E) if shuffle else None
        ne = ctypes.c_int64()
        check(lib().az_dataset_extract(self.h, len(recs), _ip(n_moves), _ip(actions), _ip(nch), _fp(pol), _ip(res),
                                       int(bool(includeAugmentations)),
                                       order.ctypes.data_as(_i64) if order is not None else None, ctypes.byref(ne)))
        return ne.value

    def size(self):
        n = ctypes.c_int64()
        check(lib().az_dataset_info(self.h, ctypes.byref(n), None, None, None))
        return n.value

    def gather(self, idx):
        """Examples idx as arrays: states [n][planes][bs][bs], policy [n][stride], policy_len [n], value [n]."""
        idx = np.ascontiguousarray(idx, np.int64)
        n = len(idx)
        st = np.empty((n, self.planes, self.bs, self.bs), np.float32)
        po = np.empty((n, self.policy_stride), np.float32)
        pl = np.empty(n, np.int32)
        va = np.empty(n, np.float32)
        if n:
            check(lib().az_dataset_gather(self.h, idx.ctypes.data_as(_i64), n, _fp(st), _fp(po), _ip(pl), _fp(va)))
        return st, po, pl, va

    def getBatch(self, batchSize):
        """Dataset::getBatch (dataset.cpp:120-145): std::shuffle of all indices, the first batchSize."""
        n = self.size()
        b = min(int(batchSize), n)
        st, po, pl, va = self.gather(self._order(n)[:b])
        return st, [po[i, :pl[i]].copy() for i in range(b)], va

    def shuffle(self):
        n = self.size()
        if n:
            check(lib().az_dataset_permute(self.h, self._order(n).ctypes.data_as(_i64)))

    def getRandomSubset(self, count):
        n = self.size()
        st, po, pl, va = self.gather(self._order(n)[:min(int(count), n)])
        return [TrainingExample(st[i], po[i, :pl[i]].copy(), float(va[i])) for i in range(len(va))]

    def examples(self):
        st, po, pl, va = self.gather(np.arange(self.size()))
        return [TrainingExample(st[i], po[i, :pl[i]].copy(), float(va[i])) for i in range(len(va))]

    def saveToFile(self, filename):
        """Dataset::saveToFile (dataset.cpp:151-186): {"examples":[...]} as j.dump()."""
        try:
            with open(filename, "w") as f:
                f.write('{"examples":[' + ",".join(e.toJson() for e in self.examples()) + "]}")
            return True
        except Exception:
            return False

    def loadFromFile(self, filename):
        """Dataset::loadFromFile (dataset.cpp:188-227); examples go to the device store."""
        import json
        try:
            with open(filename) as f:
                j = json.load(f)
            exs = [TrainingExample.fromJson(e) for e in j["examples"]]
        except Exception:
            return False
        n = len(exs)
        st = np.zeros((n, self.planes, self.bs, self.bs), np.float32)
        po = np.zeros((n, self.policy_stride), np.float32)
        pl = np.zeros(n, np.int32)
        va = np.zeros(n, np.float32)
        for i, e in enumerate(exs):
            st[i] = e.state
            pl[i] = len(e.policy)
            po[i, :pl[i]] = e.policy
            va[i] = e.value
        check(lib().az_dataset_upload(self.h, n, _fp(st), _fp(po), _ip(pl), _fp(va)))
        return True

    def profile_read(self):
        ms, by = ctypes.c_double(), ctypes.c_double()
        check(lib().az_dataset_profile_read(self.h, ctypes.byref(ms), ctypes.byref(by)))
        return ms.value, by.value

    def close(self):
        if self.h:
            lib().az_dataset_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------- ReplayBuffer
def replay_sym_cell(board_size, sym, cell):
    """az_replay_sym_cell: the cell `cell` maps to under symmetry `sym` (0 identity; the enumeration is in
    include/az_engine.h)."""
    c = lib().az_replay_sym_cell(int(board_size), int(sym), int(cell))
    if c < 0:
        raise ValueError(f"replay_sym_cell({board_size}, {sym}, {cell}): argument out of range")
    return c


def replay_sample_plan(seed, call, n, committed, augment=True):
    """az_replay_sample_plan: (idx int64 [n], sym int32 [n]) of sampling call `call` under `seed`."""
    idx = np.zeros(max(n, 1), np.int64)
    sym = np.zeros(max(n, 1), np.int32)
    check(lib().az_replay_sample_plan(int(seed), int(call), int(n), int(committed), int(bool(augment)),
                                      idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _ip(sym)))
    return idx[:n], sym[:n]


class ReplayBuffer:
    """A device-resident ring of training positions (az_replay_*): board record, visit counts by action, root
    value and outcome.  Attach it to a ParallelMCTS (attachReplay); selfplayStep / generateGames fill it."""

    def __init__(self, engine, game=GAME_GOMOKU, board_size=15, capacity=1 << 16, max_plies=None):
        self.bs, self.game = board_size, game
        self.A = board_size * board_size
        self.NA = self.A + (1 if game == GAME_GO else 0)
        self.C = 8 if game == GAME_GO else 11
        if max_plies is None:
            max_plies = 2 * self.A
        cfg = ReplayCfg(game, board_size, capacity, max_plies)
        h = ctypes.c_void_p()
        check(lib().az_replay_create(engine.h, ctypes.byref(cfg), ctypes.byref(h)))
        self.h, self.engine = h, engine

    def info(self):
        v = [ctypes.c_int64(0) for _ in range(5)]
        check(lib().az_replay_info(self.h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("committed", "total_committed", "games", "dropped", "skipped"), (int(x.value) for x in v)))

    def seed(self, seed):
        """The seed of sample / sample_into; the call counter restarts at 0."""
        check(lib().az_replay_seed(self.h, int(seed)))

    def _outs(self, n):
        m = max(n, 1)
        return (np.zeros((m, self.C, self.bs, self.bs), np.float32), np.zeros((m, self.NA), np.float32),
                np.zeros(m, np.float32), np.zeros(m, np.float32))

    def gather(self, idx, sym=None):
        """Ring slots idx under symmetries sym (None: identity): dict of states [n][C][bs][bs], policy [n][NA],
        z, q, game_id, ply."""
        idx = np.ascontiguousarray(idx, np.int64).reshape(-1)
        n = idx.size
        st, po, z, q = self._outs(n)
        gid, ply = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        sp = None
        if sym is not None:
            sym = np.ascontiguousarray(sym, np.int32).reshape(-1)
            if sym.size != n:
                raise ValueError("sym and idx differ in length")
            sp = _ip(sym)
        check(lib().az_replay_gather(self.h, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), sp, n, _fp(st), _fp(po),
                                     _fp(z), _fp(q), _ip(gid), _ip(ply)))
        return dict(states=st[:n], policy=po[:n], z=z[:n], q=q[:n], game_id=gid[:n], ply=ply[:n])

    def sample(self, n, augment=True):
        """One sampling call to host arrays: dict of states, policy, z, q and the plan's idx, sym."""
        st, po, z, q = self._outs(n)
        idx, sym = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int32)
        check(lib().az_replay_sample(self.h, n, int(bool(augment)), _fp(st), _fp(po), _fp(z), _fp(q),
                                     idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _ip(sym)))
        return dict(states=st[:n], policy=po[:n], z=z[:n], q=q[:n], idx=idx[:n], sym=sym[:n])

    def sample_into(self, states, policy, z=None, q=None, augment=True):
        """One sampling call straight into contiguous float32 torch tensors on the engine's device: states
        [n][C][bs][bs], policy [n][NA], optional z [n], q [n].  Returns when the tensors are written."""
        n = int(states.shape[0])
        want = {"states": (states, (n, self.C, self.bs, self.bs)), "policy": (policy, (n, self.NA)), "z": (z, (n,)),
                "q": (q, (n,))}
        ptr = {}
        for name, (t, shape) in want.items():
            if t is None:
                ptr[name] = None
                continue
            if tuple(t.shape) != shape or not t.is_contiguous() or str(t.dtype) != "torch.float32" or not t.is_cuda:
                raise ValueError(f"{name}: need a contiguous float32 device tensor of shape {shape}")
            ptr[name] = ctypes.c_void_p(t.data_ptr())
        check(lib().az_replay_sample_device(self.h, n, int(bool(augment)), ptr["states"], ptr["policy"], ptr["z"],
                                            ptr["q"]))

    def counts(self, idx):
        """The raw visit counts by action of ring slots idx: (counts int32 [n][NA], sum int32 [n])."""
        idx = np.ascontiguousarray(idx, np.int64).reshape(-1)
        n = idx.size
        c, s = np.zeros((max(n, 1), self.NA), np.int32), np.zeros(max(n, 1), np.int32)
        check(lib().az_replay_counts(self.h, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n, _ip(c), _ip(s)))
        return c[:n], s[:n]

    def clear(self):
        check(lib().az_replay_clear(self.h))

    def close(self):
        if self.h:
            lib().az_replay_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
