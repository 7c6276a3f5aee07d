"""Scatter-gather batches on the GPU: tulips_csum_batch_sg / _verify_sg (every
shipped kernel instance) against the reference over the concatenated bytes.

Expected values: the reference's own outputs in tests/golden/adversarial.npz
for that fixture cut into fragments, and oracle/csum_oracle.c (pinned to the
reference by tests/test_oracle.py) over the concatenation of each segment's
fragments. Bar: bit-exact. Shapes are the smallest at which the kernel can go
wrong: fragments per segment around its 64-fragment metadata batch, segment
counts around the segments-per-wave boundary of every instance and the grid
tail, the four address / logical parity combinations, one-byte fragments
inside 0xff chunks, the 65535-byte total.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import FLAG_COMPLEMENT, MODE_INET, MODE_RAW, MODE_TCP  # noqa: E402

import sg_util  # noqa: E402
import tulips_amd  # noqa: E402
from tulips_amd import csum  # noqa: E402

DEV = "cuda:0"

# every shipped instance (segments per wave, windows per batch, nt loads), and
# the entry point's own choice
GEOMETRIES = [None] + [(s, u, nt) for (s, u) in csum.SG_GEOMETRIES for nt in (0, 1)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def d(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def u16(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint16)


def tuning(geom):
    if geom is None:
        return None
    s, u, nt = geom
    return csum.Tuning(kind=csum.KIND_DEFAULT, group=s, unroll=u, nontemporal=nt)


class Plan:
    """A plan on the device."""

    def __init__(self, arena, foffs, flens, first):
        self.h = (np.asarray(arena, np.uint8), np.asarray(foffs, np.uint64),
                  np.asarray(flens, np.uint16), np.asarray(first, np.uint32))
        self.n = len(first) - 1
        self.d = tuple(d(x) for x in self.h)

    def run(self, geom=None, **kw):
        kw = {k: (d(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        return u16(csum.batch_sg(*self.d, tuning=tuning(geom), **kw))

    def expect(self, oracle, **kw):
        return sg_util.expected(oracle, *self.h, **kw)


@pytest.fixture(scope="module")
def cut_fixture(golden):
    """The adversarial fixture cut into 1..5 fragments per segment: in place,
    and with every fragment copied to a seeded place in a 0xff-filled arena."""
    adv = golden.adversarial()
    rng = np.random.default_rng(0xAD5)
    foffs, flens, first = sg_util.cut(rng, adv["offsets"], adv["lengths"], 5)
    arena2, foffs2 = sg_util.relocate(rng, adv["arena"], foffs, flens, fill=0xFF)
    side = {k: d(adv[k]) for k in ("seeds", "src", "dst")}
    return {"adv": adv, "side": side, "nfrags": len(foffs),
            "in_place": lambda arena: Plan(arena, foffs, flens, first),
            "moved": Plan(arena2, foffs2, flens, first)}


def test_cut_fixture_all_modes(golden, cut_fixture):
    adv, side = cut_fixture["adv"], cut_fixture["side"]
    for name, (kind, mode, use_seeds) in golden.ADV_CASES.items():
        plans = [cut_fixture["in_place"](golden.adv_arena(adv, kind))]
        if kind == "arena":
            plans.append(cut_fixture["moved"])
        for p in plans:
            got = p.run(seeds=side["seeds"] if use_seeds else None, src=side["src"],
                        dst=side["dst"], mode=mode)
            np.testing.assert_array_equal(got, adv["expect_" + name], err_msg=name)


@pytest.mark.parametrize("geom", GEOMETRIES[1:])
def test_cut_fixture_every_instance(golden, cut_fixture, geom):
    adv, side = cut_fixture["adv"], cut_fixture["side"]
    for p in (cut_fixture["in_place"](adv["arena"]), cut_fixture["moved"]):
        got = p.run(geom, src=side["src"], dst=side["dst"], mode=MODE_TCP)
        np.testing.assert_array_equal(got, adv["expect_tcp"])
        got = p.run(geom, seeds=side["seeds"], mode=MODE_RAW)
        np.testing.assert_array_equal(got, adv["expect_raw_seed"])


def test_one_fragment_per_segment_is_batch(golden, oracle):
    """seg_first = 0..n over a plain batch: bit-identical to tulips_csum_batch
    on the same arrays (and to the reference)."""
    adv = golden.adversarial()
    n = len(adv["offsets"])
    p = Plan(adv["arena"], adv["offsets"], adv["lengths"], np.arange(n + 1, dtype=np.uint32))
    src, dst = d(adv["src"]), d(adv["dst"])
    for mode in (MODE_RAW, MODE_TCP | FLAG_COMPLEMENT):
        want = u16(tulips_amd.batch(p.d[0], p.d[1], p.d[2], src=src, dst=dst, mode=mode))
        np.testing.assert_array_equal(p.run(src=src, dst=dst, mode=mode), want)
    np.testing.assert_array_equal(p.run(src=src, dst=dst, mode=MODE_TCP), adv["expect_tcp"])


def test_parity_combinations(oracle):
    """An odd-length fragment first, then fragments at both address parities
    and both logical parities."""
    rng = np.random.default_rng(3)
    arena = rng.integers(1, 256, 8192, dtype=np.uint8)
    foffs, flens, first, seen = [], [], [0], set()
    at = 0
    for a0 in (0, 1):
        for l0 in (1, 3, 17):
            for a1 in (0, 1):
                for l1 in (2, 5, 16):
                    for a2 in (0, 1):
                        for ap, ln in ((a0, l0), (a1, l1), (a2, 7)):
                            at = (at + 34) & ~1
                            foffs.append(at + ap)
                            flens.append(ln)
                        seen.add((a1, l0 & 1))
                        seen.add((a2, (l0 + l1) & 1))
                        first.append(len(foffs))
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)} and at < 8100
    p = Plan(arena, foffs, flens, first)
    for geom in GEOMETRIES:
        np.testing.assert_array_equal(p.run(geom), p.expect(oracle), err_msg=str(geom))
    # the known answer: {0x01}, {0x02} is 01 02, not the chained 0x0300
    a = np.zeros(64, dtype=np.uint8)
    a[5], a[32] = 0x01, 0x02
    assert Plan(a, [5, 32], [1, 1], [0, 2]).run().tolist() == [0x0102]
    assert Plan(a, [32, 5], [1, 1], [0, 2]).run().tolist() == [0x0201]


FRAGS_PER_SEG = (0, 1, 2, 3, 63, 64, 65, 130)
# around the 8- and 16-segment wave boundaries (and twice that) and the grid tail
SEG_COUNTS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def boundary_plans(oracle):
    """One plan per segment count, its fragment counts cycling through
    FRAGS_PER_SEG (so segments cross the 64-fragment batch at every phase),
    with the oracle's RAW and TCP results."""
    rng = np.random.default_rng(0xB0)
    plans = []
    for n in SEG_COUNTS:
        counts = np.array([FRAGS_PER_SEG[(i + n) % len(FRAGS_PER_SEG)] for i in range(n)])
        nf = int(counts.sum())
        flens = rng.integers(0, 48, nf)
        first = np.concatenate(([0], np.cumsum(counts)))
        arena = rng.integers(0, 256, 8192, dtype=np.uint8)
        foffs = rng.integers(0, 8192 - 64, nf)
        src = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        dst = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        seeds = rng.integers(0, 65536, n, dtype=np.uint32).astype(np.uint16)
        p = Plan(arena, foffs, flens, first)
        plans.append((p, seeds, src, dst, p.expect(oracle, seeds=seeds),
                      p.expect(oracle, src=src, dst=dst, mode=MODE_TCP)))
    return plans


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_batch_and_wave_boundaries(boundary_plans, geom):
    for p, seeds, src, dst, e_raw, e_tcp in boundary_plans:
        np.testing.assert_array_equal(p.run(geom, seeds=seeds), e_raw, err_msg=f"n={p.n}")
        np.testing.assert_array_equal(p.run(geom, src=src, dst=dst, mode=MODE_TCP), e_tcp,
                                      err_msg=f"n={p.n}")


def test_one_byte_fragments_in_ff_chunks(oracle):
    """The worst edge-byte subtraction: one segment of 4096 one-byte
    fragments, each in the middle of its own 0xff-filled chunk."""
    rng = np.random.default_rng(5)
    arena = np.full(4096 * 16 + 16, 0xFF, dtype=np.uint8)
    foffs = np.arange(4096) * 16 + 7 + (np.arange(4096) % 2)
    arena[foffs] = rng.integers(0, 256, 4096)
    p = Plan(arena, foffs, np.ones(4096, np.uint16), [0, 4096])
    want = p.expect(oracle)
    for geom in GEOMETRIES:
        np.testing.assert_array_equal(p.run(geom), want, err_msg=str(geom))


def test_maximum_total(oracle):
    """One segment of 65535 bytes in five fragments (with neighbours)."""
    rng = np.random.default_rng(6)
    arena = rng.integers(0, 256, 200000, dtype=np.uint8)
    flens = [3, 20001, 12345, 33181, 1, 7, 65535, 0, 65535]
    assert sum(flens[1:6]) == 65535
    foffs = [9, 100003, 17, 40001, 77, 150002, 1001, 5, 70000]
    first = [0, 1, 6, 6, 7, 9]
    src = np.arange(5, dtype=np.uint32) * 0x01010101
    p = Plan(arena, foffs, flens, first)
    for geom in GEOMETRIES:
        for mode in (MODE_RAW, MODE_TCP):
            np.testing.assert_array_equal(p.run(geom, src=src, dst=src, mode=mode),
                                          p.expect(oracle, src=src, dst=src, mode=mode),
                                          err_msg=f"{geom} {mode}")


def test_identity_cases(oracle):
    rng = np.random.default_rng(8)
    for fill in (0x00, 0xFF):
        arena, foffs, flens, first = sg_util.random_plan(rng, 300, fill=fill)
        p = Plan(arena, foffs, flens, first)
        _, _, lens = sg_util.concat(*p.h)
        raw, inet = p.run(mode=MODE_RAW), p.run(mode=MODE_INET)
        np.testing.assert_array_equal(raw, p.expect(oracle))
        np.testing.assert_array_equal(inet, p.expect(oracle, mode=MODE_INET))
        if fill == 0:
            assert not raw.any() and (inet == 0xFFFF).all()
        else:
            assert (raw[lens > 0] != 0).all()
            assert (raw[(lens > 0) & (lens % 2 == 0)] == 0xFFFF).all()


def test_empty_plans():
    seeds = np.array([0x1234, 0, 0xFFFF], dtype=np.uint16)
    e = np.zeros(0, dtype=np.uint8)
    # nfrags == 0 with n > 0: every segment returns its seed
    p = Plan(e, e.astype(np.uint64), e.astype(np.uint16), [0, 0, 0, 0])
    assert p.run(seeds=seeds).tolist() == seeds.tolist()
    assert p.run(mode=MODE_INET).tolist() == [0xFFFF] * 3
    bad = csum.verify_sg(*p.d, mode=MODE_INET)
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    # n == 0
    p = Plan(e, e.astype(np.uint64), e.astype(np.uint16), [0])
    assert len(p.run()) == 0
    bad = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    csum.verify_sg(*p.d, mode=MODE_INET, bad=bad)
    torch.cuda.synchronize()
    assert int(bad.item()) == 0


def _verifying_plan(oracle, rng, n, k):
    """n TCP segments that verify, k of them then corrupted, cut into 1..4
    fragments; returns (plan, src, dst, expected results)."""
    lens = rng.integers(20, 1500, n).astype(np.uint16)
    offs = np.concatenate(([0], np.cumsum(lens.astype(np.int64) + 5)[:-1])).astype(np.uint64) + 3
    arena = rng.integers(0, 256, int(offs[-1]) + int(lens[-1]) + 64, dtype=np.uint8)
    src = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    dst = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    idx = offs.astype(np.int64) + 16
    arena[idx] = arena[idx + 1] = 0
    gen = oracle.batch(arena, offs, lens, src=src, dst=dst, mode=MODE_TCP | FLAG_COMPLEMENT)
    arena[idx], arena[idx + 1] = gen & 0xFF, gen >> 8
    for i in rng.choice(n, k, replace=False):
        arena[int(offs[i]) + int(rng.integers(0, lens[i]))] ^= 0x40
    exp = oracle.batch(arena, offs, lens, src=src, dst=dst, mode=MODE_TCP)
    assert int(np.count_nonzero(exp != 0xFFFF)) == k
    foffs, flens, first = sg_util.cut(rng, offs, lens, 4)
    return Plan(arena, foffs, flens, first), src, dst, exp


def test_verify_counts(oracle):
    rng = np.random.default_rng(9)
    for n, k in ((300, 0), (300, 13), (70, 70)):
        p, src, dst, exp = _verifying_plan(oracle, rng, n, k)
        bad = torch.full((1,), 99, dtype=torch.int32, device=DEV)
        csum.verify_sg(*p.d, src=d(src), dst=d(dst), mode=MODE_TCP, out=None, bad=bad)
        torch.cuda.synchronize()
        assert int(bad.item()) == k
        out = torch.zeros(n, dtype=torch.int16, device=DEV)
        bad = csum.verify_sg(*p.d, src=d(src), dst=d(dst), mode=MODE_TCP, out=out)
        assert int(bad.item()) == k
        np.testing.assert_array_equal(u16(out), exp)


def test_captured_graph_replays(oracle):
    """batch_sg and verify_sg captured on one stream into one graph, replayed
    twice with the data changed in between."""
    rng = np.random.default_rng(10)
    n = 500
    p, src, dst, exp = _verifying_plan(oracle, rng, n, 9)
    dsrc, ddst = d(src), d(dst)
    out = torch.zeros(n, dtype=torch.int16, device=DEV)
    out2 = torch.zeros(n, dtype=torch.int16, device=DEV)
    bad = torch.full((1,), 99, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        csum.batch_sg(*p.d, src=dsrc, dst=ddst, mode=MODE_TCP, out=out)
        csum.verify_sg(*p.d, src=dsrc, dst=ddst, mode=MODE_TCP, out=out2, bad=bad)
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(u16(out), exp)
    np.testing.assert_array_equal(u16(out2), exp)
    assert int(bad.item()) == 9
    # corrupt three more segments in the captured arena, replay
    arena = p.h[0].copy()
    good = np.nonzero(exp == 0xFFFF)[0][:3]
    for i in good:
        arena[int(p.h[1][p.h[3][i]])] ^= 0x01      # first byte of the first fragment
    p.d[0].copy_(torch.from_numpy(arena))
    exp2 = sg_util.expected(oracle, arena, *p.h[1:], src=src, dst=dst, mode=MODE_TCP)
    nbad2 = int(np.count_nonzero(exp2 != 0xFFFF))
    assert nbad2 == 12
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(u16(out), exp2)
    assert int(bad.item()) == nbad2
    torch.cuda.synchronize()
    del g
