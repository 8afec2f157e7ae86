"""The host-only parts of the replay buffer (az_replay_*, include/az_engine.h), no GPU:
  - az_replay_sample_plan against a numpy restatement of Philox4x32-10 written here (itself anchored to the
    published known-answer vectors of the generator),
  - az_replay_sym_cell: eight distinct board symmetries, closed under composition,
  - the null-handle guards."""
import ctypes

import numpy as np
import pytest

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr uint32 [n][4], key (k0, k1) -> uint32 [n][4] (Salmon et al., SC'11, ten rounds)."""
    c = [ctr[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, 1).astype(np.uint32)


def plan_model(seed, call, n, committed, augment):
    ctr = np.zeros((n, 4), np.uint32)
    ctr[:, 0] = np.arange(n)
    ctr[:, 1], ctr[:, 2] = call & 0xFFFFFFFF, call >> 32
    out = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).astype(np.uint64)
    idx = ((out[:, 0] * np.uint64(committed)) >> np.uint64(32)).astype(np.int64)
    sym = (out[:, 1] & np.uint64(7)).astype(np.int32) if augment else np.zeros(n, np.int32)
    return idx, sym


def test_philox_restatement_known_answers():
    """The generator's published test vectors (Random123 kat_vectors, philox4x32 10)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox4x32_10(np.array([ctr], np.uint32), key)[0]
        assert [int(x) for x in got] == list(want), (ctr, key)


@pytest.mark.parametrize("seed", [0x0123456789ABCDEF, 7])
@pytest.mark.parametrize("call", [0, (3 << 32) | 5])
@pytest.mark.parametrize("committed", [1, 7, 1000])
def test_sample_plan_is_philox(seed, call, committed):
    import az_amd
    n = 64
    idx, sym = az_amd.replay_sample_plan(seed, call, n, committed, augment=True)
    widx, wsym = plan_model(seed, call, n, committed, True)
    assert np.array_equal(idx, widx) and np.array_equal(sym, wsym)
    assert idx.min() >= 0 and idx.max() < committed
    assert sym.min() >= 0 and sym.max() <= 7
    idx0, sym0 = az_amd.replay_sample_plan(seed, call, n, committed, augment=False)
    assert np.array_equal(idx0, idx) and not sym0.any()
    idx1, sym1 = az_amd.replay_sample_plan(seed, call + 1, n, committed, augment=True)
    assert not np.array_equal(sym1, sym)                    # another call: another plan
    if committed > 1:
        assert not np.array_equal(idx1, idx)
    if committed == 1000:
        assert len(set(sym.tolist())) == 8 and len(set(idx.tolist())) > 48


def test_sample_plan_guards():
    import az_amd
    for bad in (dict(n=-1, committed=5), dict(n=4, committed=0), dict(n=4, committed=1 << 32)):
        with pytest.raises(az_amd.AzError) as e:
            az_amd.replay_sample_plan(1, 0, bad["n"], bad["committed"])
        assert e.value.code == -1


@pytest.mark.parametrize("bs", [3, 6, 9])
def test_sym_cell_is_the_squares_symmetry_group(bs):
    import az_amd
    A = bs * bs
    maps = [tuple(az_amd.replay_sym_cell(bs, s, a) for a in range(A)) for s in range(8)]
    assert maps[0] == tuple(range(A))                        # 0: the identity
    for m in maps:
        assert sorted(m) == list(range(A))                   # a bijection
    assert len(set(maps)) == 8                               # pairwise distinct
    for a in maps:                                           # closed under composition
        for b in maps:
            assert tuple(b[a[x]] for x in range(A)) in maps
    # a board symmetry: cells that share an edge still do
    def adjacent(x, y):
        return abs(x // bs - y // bs) + abs(x % bs - y % bs) == 1
    for m in maps:
        for x in range(A):
            for y in (x + 1, x + bs):
                if y < A and adjacent(x, y):
                    assert adjacent(m[x], m[y])
    # the enumeration the header states: sym = k + 4 f, mirror the columns if f, then k quarter turns
    n = bs - 1
    want = [lambda r, c: (r, c), lambda r, c: (c, n - r), lambda r, c: (n - r, n - c), lambda r, c: (n - c, r),
            lambda r, c: (r, n - c), lambda r, c: (n - c, n - r), lambda r, c: (n - r, c), lambda r, c: (c, r)]
    for s in range(8):
        for x in range(A):
            r, c = want[s](x // bs, x % bs)
            assert maps[s][x] == r * bs + c
    for bad in ((bs, 8, 0), (bs, -1, 0), (bs, 0, A), (bs, 0, -1)):
        with pytest.raises(ValueError):
            az_amd.replay_sym_cell(*bad)


def test_null_handles_are_argument_errors():
    from az_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    cfg = _lib.ReplayCfg(0, 9, 64, 16)
    assert L.az_replay_create(None, ctypes.byref(cfg), ctypes.byref(h)) == _lib.AZ_ERR_ARG
    assert L.az_last_error()
    assert L.az_search_attach_replay(None, None) == _lib.AZ_ERR_ARG
    assert L.az_replay_info(None, None, None, None, None, None) == _lib.AZ_ERR_ARG
