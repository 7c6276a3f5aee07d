"""Scatter-gather batches on the CPU: tulips_csum_batch_sg_cpu against the
reference over the concatenated bytes.

Expected values: oracle/csum_oracle.c (pinned to the reference by
tests/test_oracle.py) over the concatenation of each segment's fragments, and
the reference's own outputs in tests/golden/adversarial.npz for that fixture
cut into fragments. Bar: bit-exact.
"""
import ctypes as C

import numpy as np
import pytest

import sg_util
import tulips_amd
from tulips_amd import csum
from oracle import FLAG_COMPLEMENT, MODE_INET, MODE_RAW, MODE_TCP

MODES = [MODE_RAW, MODE_INET, MODE_TCP, MODE_RAW | FLAG_COMPLEMENT,
         MODE_INET | FLAG_COMPLEMENT, MODE_TCP | FLAG_COMPLEMENT]


def _side(rng, n):
    seeds = rng.integers(0, 65536, n, dtype=np.uint32).astype(np.uint16)
    src = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    dst = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    return seeds, src, dst


@pytest.mark.parametrize("fill", [None, 0x00, 0xFF])
def test_random_plans_all_modes(oracle, fill):
    """0 to 6 fragments per segment, the edge lengths and random ones, every
    start alignment 0..15, all modes with and without seeds and COMPLEMENT,
    on random, all-zero and all-0xff arenas."""
    rng = np.random.default_rng(0x5347 + (fill or 7))
    n = 400
    arena, foffs, flens, first = sg_util.random_plan(rng, n, fill=fill)
    assert set((foffs % 16).tolist()) == set(range(16))
    seeds, src, dst = _side(rng, n)
    for mode in MODES:
        for use_seeds in (False, True):
            sd = seeds if use_seeds and (mode & 0xff) != MODE_TCP else None
            exp = sg_util.expected(oracle, arena, foffs, flens, first, seeds=sd, src=src,
                                   dst=dst, mode=mode)
            got = csum.batch_sg_cpu(arena, foffs, flens, first, seeds=sd, src=src, dst=dst,
                                    mode=mode)
            np.testing.assert_array_equal(got, exp, err_msg=f"mode {mode:#x} seeds {use_seeds}")
    if fill == 0x00:
        # zero iff all bytes are zero: INET 0xffff and RAW 0 with no seed
        assert not tulips_amd.batch_sg_cpu(arena, foffs, flens, first, mode=MODE_RAW).any()
        assert (csum.batch_sg_cpu(arena, foffs, flens, first, mode=MODE_INET) == 0xFFFF).all()
    if fill == 0xFF:
        # all-0xff bytes must not collapse to 0 (segments with any byte)
        _, _, lens = sg_util.concat(arena, foffs, flens, first)
        got = csum.batch_sg_cpu(arena, foffs, flens, first, mode=MODE_RAW)
        assert (got[lens > 0] != 0).all() and (got[(lens > 0) & (lens % 2 == 0)] == 0xFFFF).all()


def test_adversarial_fixture_cut_in_place(golden):
    """Every segment of the adversarial fixture cut at seeded points into 1
    to 5 fragments, still in place: the fixture's own reference outputs."""
    adv = golden.adversarial()
    rng = np.random.default_rng(0xAD5)
    foffs, flens, first = sg_util.cut(rng, adv["offsets"], adv["lengths"], 5)
    assert len(foffs) > len(adv["offsets"])
    for name, (kind, mode, use_seeds) in golden.ADV_CASES.items():
        got = csum.batch_sg_cpu(golden.adv_arena(adv, kind), foffs, flens, first,
                                seeds=adv["seeds"] if use_seeds else None, src=adv["src"],
                                dst=adv["dst"], mode=mode)
        np.testing.assert_array_equal(got, adv["expect_" + name], err_msg=name)


def test_concatenation_is_not_chaining(oracle):
    """Fragments {0x01} and {0x02} are the segment 01 02: RAW 0x0102. The
    reference call chained per fragment would give 0x0100 + 0x0200."""
    for o1, o2 in ((5, 32), (32, 5)):
        a = np.zeros(64, dtype=np.uint8)
        a[o1], a[o2] = 0x01, 0x02
        got = csum.batch_sg_cpu(a, [o1, o2], [1, 1], [0, 2])
        assert got.tolist() == [0x0102]
    assert oracle.checksum(0, b"\x01\x02") == 0x0102
    assert oracle.checksum(oracle.checksum(0, b"\x01"), b"\x02") == 0x0300


def test_bad_count_is_exact(oracle):
    """k corrupted segments among valid TCP segments: bad_count == k."""
    rng = np.random.default_rng(77)
    n, k = 200, 13
    lens = rng.integers(20, 1500, n).astype(np.uint16)
    offs = np.concatenate(([0], np.cumsum(lens.astype(np.int64) + 5)[:-1])).astype(np.uint64) + 3
    arena = rng.integers(0, 256, int(offs[-1]) + int(lens[-1]) + 64, dtype=np.uint8)
    _, src, dst = _side(rng, n)
    # make every segment verify: store the complemented checksum at bytes 16..17
    for i in range(n):
        o = int(offs[i])
        arena[o + 16:o + 18] = 0
    gen = oracle.batch(arena, offs, lens, src=src, dst=dst, mode=MODE_TCP | FLAG_COMPLEMENT)
    for i in range(n):
        o = int(offs[i])
        arena[o + 16:o + 18] = np.frombuffer(np.uint16(gen[i]).tobytes(), dtype=np.uint8)
    assert (oracle.batch(arena, offs, lens, src=src, dst=dst, mode=MODE_TCP) == 0xFFFF).all()
    for i in rng.choice(n, k, replace=False):
        arena[int(offs[i]) + int(rng.integers(0, lens[i]))] ^= 0x40
    foffs, flens, first = sg_util.cut(rng, offs, lens, 4)
    out, bad = csum.batch_sg_cpu(arena, foffs, flens, first, src=src, dst=dst, mode=MODE_TCP,
                                 with_bad=True)
    assert bad == k
    assert int(np.count_nonzero(out != 0xFFFF)) == k


def _raw_call(arena, foffs, flens, first, n, *, nfrags=None, out=True, bad=False, mode=MODE_RAW,
              src=None, dst=None):
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    foffs = np.ascontiguousarray(foffs, dtype=np.uint64)
    flens = np.ascontiguousarray(flens, dtype=np.uint16)
    first = np.ascontiguousarray(first, dtype=np.uint32)
    o = np.full(max(n, 1), 0xA5A5, dtype=np.uint16)
    b = np.full(1, 0xA5A5A5A5, dtype=np.uint32)
    rc = csum.lib.tulips_csum_batch_sg_cpu(
        arena.ctypes.data, foffs.ctypes.data, flens.ctypes.data,
        len(foffs) if nfrags is None else nfrags, first.ctypes.data, None,
        None if src is None else src.ctypes.data, None if dst is None else dst.ctypes.data,
        o.ctypes.data if out else None, b.ctypes.data if bad else None, n, mode)
    return rc, o, b


def test_broken_plan_is_invalid_argument():
    arena = np.arange(64, dtype=np.uint8)
    foffs, flens = [0, 8, 16], [4, 4, 4]
    assert _raw_call(arena, foffs, flens, [0, 1, 3], 2)[0] == csum.STATUS_OK
    # not monotone
    assert _raw_call(arena, foffs, flens, [0, 2, 1], 2)[0] == csum.STATUS_INVALID_ARGUMENT
    # past nfrags
    assert _raw_call(arena, foffs, flens, [0, 1, 4], 2)[0] == csum.STATUS_INVALID_ARGUMENT
    with pytest.raises(csum.InvalidArgument):
        csum.batch_sg_cpu(arena, foffs, flens, [0, 3, 2])


def test_argument_errors():
    arena = np.arange(64, dtype=np.uint8)
    foffs, flens, first = [0, 8], [4, 4], [0, 1, 2]
    inv = csum.STATUS_INVALID_ARGUMENT
    assert _raw_call(arena, foffs, flens, first, 2, mode=3)[0] == inv           # unknown mode
    assert _raw_call(arena, foffs, flens, first, 2, mode=0x200)[0] == inv       # unknown flag
    assert _raw_call(arena, foffs, flens, first, 2, mode=MODE_TCP)[0] == inv    # no src/dst
    assert _raw_call(arena, foffs, flens, first, 2, out=False)[0] == inv        # nothing to write
    rc = csum.lib.tulips_csum_batch_sg_cpu(arena.ctypes.data, None, None, 2, None, None, None,
                                           None, None, None, 2, MODE_RAW)
    assert rc == inv
    # the device entry points validate before any GPU call
    lib = csum.lib
    assert lib.tulips_csum_batch_sg(None, None, None, 0, None, None, None, None, None, 0, 0,
                                    None) == csum.STATUS_OK
    one = C.c_uint64(0)
    p = C.addressof(one)
    assert lib.tulips_csum_batch_sg(p, p, p, 1, p, None, None, None, None, 1, 0, None) == inv
    assert lib.tulips_csum_batch_sg(p, p, p, 1, None, None, None, None, p, 1, 0, None) == inv
    assert lib.tulips_csum_batch_sg(None, p, p, 1, p, None, None, None, p, 1, 0, None) == inv
    assert lib.tulips_csum_batch_sg(p, p, p, 1, p, None, None, None, p, 1, 7, None) == inv
    assert lib.tulips_csum_batch_sg(p, p, p, 1, p, None, None, None, p, 1, MODE_TCP,
                                    None) == inv
    assert lib.tulips_csum_verify_sg(p, p, p, 1, p, None, None, None, None, 1, MODE_INET,
                                     None) == inv                                # no counter
    assert lib.tulips_csum_verify_sg(p, p, p, 1, p, None, None, None, p, 1, MODE_RAW,
                                     None) == inv                                # RAW verify
    bad = csum.Tuning(group=7, unroll=4, kind=csum.KIND_DEFAULT)
    assert lib.tulips_csum_batch_sg_tuned(p, p, p, 1, p, None, None, None, p, 1, 0,
                                          C.byref(bad), None) == inv


def test_empty_batch_and_empty_segments():
    rc, o, b = _raw_call(np.zeros(1, np.uint8), [], [], [0], 0, bad=True)
    assert rc == csum.STATUS_OK and int(b[0]) == 0 and int(o[0]) == 0xA5A5
    assert len(csum.batch_sg_cpu(np.zeros(1, np.uint8), [], [], [0])) == 0
    # segments without fragments (and with only empty fragments) return their seed
    seeds = np.array([0x1234, 0, 0xFFFF, 7], dtype=np.uint16)
    got = csum.batch_sg_cpu(np.zeros(16, np.uint8), [3, 9], [0, 0], [0, 0, 0, 2, 2], seeds=seeds)
    assert got.tolist() == seeds.tolist()
    # nfrags == 0 with n > 0
    got = csum.batch_sg_cpu(np.zeros(1, np.uint8), [], [], [0, 0, 0], seeds=seeds[:2],
                            mode=MODE_INET)
    assert got.tolist() == [0x3412, 0xFFFF]
