"""Write confinement: every entry point of include/tulips_csum.h writes only
where its contract says.

The other tests take an output from the Python wrapper (torch.empty(n)) or
allocate exactly the bytes the contract names; the caching allocator rounds
each block up, so a store one result past out[n-1] or one slot past
out_capacity lands in slack nobody reads. Here every output is a view inside
a larger pattern-filled allocation (tests/guard_util.py) handed to the C ABI
by address, so no wrapper allocates anything, and each case asserts both

  (a) the result inside the view equals the oracle (a test that only looked
      at the bands would pass on a kernel that wrote nothing), and
  (b) both guard bands, every byte of the view the contract says is not
      written, and every "only read" / "not modified" input are unchanged.

Choice of n. A result is produced per subgroup, wave or window, and a ragged
last wave / workgroup / grid-stride round is where a store predicate goes
wrong. For every kernel instance the counts one wave and one workgroup handle
are derived from its geometry tuple (the *_counts functions next to each
geometry list below), and n runs over

  {1, per_wave - 1, per_wave, per_wave + 1, per_workgroup + 1}

plus one odd n of a few thousand (a prime, so with max_blocks = 7 the last
grid-stride round is ragged whatever the workgroup holds). A new instance in
one of the imported geometry lists gets its boundary n by construction.

Out of scope on purpose: the zero-copy / resident validation server
(tulips_csum_validate_frames_zc, tulips_csum_ctx_set_lowlat), the benchlib
ceilings, and reads outside the inputs (not observable without a fault).
"""
import numpy as np
import pytest

import guard_util
import sg_util
from guard_util import Registry, check, guarded
from oracle import FLAG_COMPLEMENT, MODE_INET, MODE_RAW, MODE_TCP
from test_frames import (FRAME_GEOMETRIES, counters_of, fields_of, frames_fixture, mutate,
                         scramble_fields)
from test_segment import pack as pack_super, super_frame

torch = pytest.importorskip("torch")

from tulips_amd import csum  # noqa: E402
from test_gpu_parity import GEOMETRIES as BATCH_GEOMETRIES  # noqa: E402
from test_sg_gpu import GEOMETRIES as SG_GEOMETRIES  # noqa: E402
from test_span import GEOMS as SPAN_GEOMS, tuning as span_tuning  # noqa: E402

DEV = "cuda:0"
L = csum.lib
BLOCK = 256                       # threads per workgroup in every tuned call here
N_BIG = 4099                      # odd, prime: ragged last round under max_blocks = 7
CAP = 7
# uint16 outputs: ≡ 14 (mod 16) (hence ≡ 2 (mod 4)) and ≡ 2 (mod 4) on its own:
# two results paired into a dword store, or a store rounded up to 16 bytes,
# leave the view at odd n
U16_AT = ((16, 14), (4, 2))
U32_AT = (16, 4)                  # uint32 outputs (bad_count, counters, fields, first)
U8_AT = (2, 1)                    # uint8 flags at an odd address
RAW_SEEDED, TCP_GEN = MODE_RAW, MODE_TCP | FLAG_COMPLEMENT
MODES = (RAW_SEEDED, TCP_GEN)

# captured graphs kept alive to the end of the process
_KEPT_GRAPHS = []


def boundary_ns(per_wave, per_wg, big=N_BIG):
    """The n at which a ragged last wave, workgroup or grid-stride round
    exists, from the counts one wave / one workgroup handles."""
    ns = {1, per_wave - 1, per_wave, per_wave + 1, per_wg + 1, big}
    return sorted(n for n in ns if n >= 1)


# -- geometry -> (segments per wave, segments per workgroup) ------------------
def batch_counts(geom, block=BLOCK):
    """tests/test_gpu_parity.py GEOMETRIES / PACKED, (kind, group, unroll, nt,
    sps). SUBGROUP: `group` lanes per segment, so 64 / group segments per wave
    and block / group per workgroup (csum_kernel: seg = block * groups_per_block
    + thread / G). PACKED: one wave per `group` segments, block / 64 waves."""
    kind, group = geom[0], geom[1]
    if kind == csum.KIND_SUBGROUP:
        return 64 // group, block // group
    assert kind == csum.KIND_PACKED
    return group, block // 64 * group


def sg_counts(geom, block=BLOCK):
    """tests/test_sg_gpu.py GEOMETRIES, (segments per wave, windows, nt) or
    None = the entry point's own 8 x 4: one wave per `s` segments."""
    s = 8 if geom is None else geom[0]
    return s, block // 64 * s


def frame_counts(group, sps, block=BLOCK):
    """tests/test_frames.py FRAME_GEOMETRIES (group lanes per frame, unroll):
    64 / group subgroups per wave, each with 1 frame in flight, 2 with sps 2,
    about 4 with sps 3 (frames.hip launch_one: per_block = block / G * {1,2,4})."""
    f = {0: 1, 1: 1, 2: 2, 3: 4}[sps]
    return 64 // group * f, block // group * f


def span_counts(geo, seg_bytes=64):
    """tests/test_span.py GEOMS, (chunks per lane, form[, tail percent]): a
    workgroup per 4 KiB * unroll of arena bytes, whatever the segment count;
    the segments that START in a range are finished by its workgroup. With
    `seg_bytes`-byte segments laid end to end a range holds 4096 * unroll /
    seg_bytes of them; a wave has no segment count of its own, so the per-wave
    entry is a quarter of the range (four waves per 256-thread workgroup)."""
    per_range = 4096 * geo[0] // seg_bytes
    return per_range // 4, per_range


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


def expect_all(g, want):
    """(b) bands intact with every element written, then (a) the values."""
    check(g, np.ones(g.nbytes, bool))
    np.testing.assert_array_equal(g.host(), np.asarray(want).astype(g.dtype))


def expect_none(g):
    """Nothing at all written: bands and the whole view hold the pattern."""
    check(g, np.zeros(g.nbytes, bool))


# =============================================================================
# tulips_csum_batch, _batch_arena, _batch_fixed and their _tuned forms
# =============================================================================
class VarBatch:
    """An in-order arena of n segments with gaps (so it serves the any-layout
    and the arena entries alike), side inputs, and the oracle's results; a
    prefix of it is a batch of its own."""

    def __init__(self, oracle, n, seed, uniform=0, big=6):
        rng = np.random.default_rng(seed)
        if uniform:
            lens = np.full(n, uniform, np.uint16)
            gaps = np.zeros(n, np.uint64)
        else:
            lens = rng.integers(0, 300, n).astype(np.uint16)
            lens[rng.random(n) < 0.1] = 0
            lens[rng.integers(0, n, big)] = rng.integers(3000, 20000, big)
            lens[[0, -1]] = (1, 0)
            gaps = rng.integers(0, 24, n).astype(np.uint64)
        ends = np.cumsum(lens.astype(np.uint64) + gaps)
        self.n = n
        self.lens = lens
        self.offs = (ends - lens.astype(np.uint64)).astype(np.uint64)
        self.arena_bytes = int(ends[-1])
        self.arena = rng.integers(0, 256, self.arena_bytes + 64, dtype=np.uint8)
        self.seeds = rng.integers(0, 65536, n, dtype=np.uint32).astype(np.uint16)
        self.src = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        self.dst = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        # RAW seeded and TCP generation for the batch entries; INET and TCP
        # without seeds for the verify entries (they take none)
        self.exp = {m: oracle.batch(self.arena, self.offs, lens, src=self.src, dst=self.dst,
                                    seeds=self.seeds if m in MODES else None, mode=m, nthreads=4)
                    for m in MODES + (MODE_INET, MODE_TCP)}
        self.d = None

    def end(self, n):
        """Arena bytes of the prefix batch [0, n)."""
        return int(self.offs[n - 1]) + int(self.lens[n - 1])

    def device(self, reg):
        """The inputs on the device, each registered read-only with `reg`."""
        d = {k: dev(getattr(self, k)) for k in ("arena", "lens", "seeds", "src", "dst")}
        d["offs"] = dev(self.offs.view(np.int64))
        for k, t in d.items():
            reg.ro(t, k)
        return {k: t.data_ptr() for k, t in d.items()}, d

    def host(self, reg):
        for k in ("arena", "offs", "lens", "seeds", "src", "dst"):
            reg.ro(getattr(self, k), k)
        return {k: getattr(self, k).ctypes.data for k in ("arena", "offs", "lens", "seeds",
                                                          "src", "dst")}


class FixedBatch:
    """n segments of `length` bytes every `stride` bytes from an odd base."""

    def __init__(self, oracle, n, length, seed):
        rng = np.random.default_rng(seed)
        self.n, self.length, self.stride, self.base_off = n, length, length + 3, 1
        self.arena = rng.integers(0, 256, self.base_off + n * self.stride + 64, dtype=np.uint8)
        self.seeds = rng.integers(0, 65536, n, dtype=np.uint32).astype(np.uint16)
        self.src = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        self.dst = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        self.exp = {m: oracle.batch(self.arena[self.base_off:], stride=self.stride,
                                    fixed_len=length, n=n, seeds=self.seeds, src=self.src,
                                    dst=self.dst, mode=m, nthreads=4) for m in MODES}

    def device(self, reg):
        d = {k: dev(getattr(self, k)) for k in ("arena", "seeds", "src", "dst")}
        for k, t in d.items():
            reg.ro(t, k)
        p = {k: t.data_ptr() for k, t in d.items()}
        p["arena"] += self.base_off
        return p, d


@pytest.fixture(scope="module")
def var_batch(oracle):
    return VarBatch(oracle, N_BIG, 0xC0F1)


@pytest.fixture(scope="module")
def fixed77(oracle):
    return FixedBatch(oracle, N_BIG, 77, 0xC0F2)


def side(p, mode):
    """(seeds, src, dst) arguments of a mode: RAW with seeds, TCP with src/dst."""
    return (p["seeds"], None, None) if mode == RAW_SEEDED else (None, p["src"], p["dst"])


def run_var(b, p, n, mode, tuning, at):
    out = guarded((n,), np.uint16, align=at[0], skew=at[1], device=DEV)
    args = (p["arena"], p["offs"], p["lens"], *side(p, mode), out.ptr, n, mode)
    rc = L.tulips_csum_batch(*args, stream()) if tuning is None else \
        L.tulips_csum_batch_tuned(*args, tuning, stream())
    assert rc == 0, (rc, n, mode, tuning)
    expect_all(out, b.exp[mode][:n])


def run_fixed(b, p, n, mode, tuning, at):
    out = guarded((n,), np.uint16, align=at[0], skew=at[1], device=DEV)
    args = (p["arena"], b.stride, b.length, *side(p, mode), out.ptr, n, mode)
    rc = L.tulips_csum_batch_fixed(*args, stream()) if tuning is None else \
        L.tulips_csum_batch_fixed_tuned(*args, tuning, stream())
    assert rc == 0, (rc, n, mode, tuning)
    expect_all(out, b.exp[mode][:n])


def run_arena(b, p, n, mode, tuning, at, arena_bytes=None):
    out = guarded((n,), np.uint16, align=at[0], skew=at[1], device=DEV)
    args = (p["arena"], b.end(n) if arena_bytes is None else arena_bytes, p["offs"], p["lens"],
            *side(p, mode), out.ptr, n, mode)
    rc = L.tulips_csum_batch_arena(*args, stream()) if tuning is None else \
        L.tulips_csum_batch_arena_tuned(*args, tuning, stream())
    assert rc == 0, (rc, n, mode, tuning)
    expect_all(out, b.exp[mode][:n])


@pytest.mark.gpu
@pytest.mark.parametrize("geom", BATCH_GEOMETRIES)
def test_gpu_batch_tuned_every_instance(var_batch, fixed77, geom):
    """tulips_csum_batch_tuned at every shipped instance (SUBGROUP and
    PACKED), tulips_csum_batch_fixed_tuned at every SUBGROUP one: out[n] at
    both uint16 placements, n at the instance's wave / workgroup boundaries
    and at 4099 with a grid cap of 7 workgroups."""
    kind, group, unroll, nt, sps = geom
    reg = Registry(DEV)
    pv, _kv = var_batch.device(reg)
    pf, _kf = fixed77.device(reg)
    for n in boundary_ns(*batch_counts(geom)):
        t = csum.Tuning(kind=kind, group=group, unroll=unroll, nontemporal=nt, sps=sps,
                        block=BLOCK, max_blocks=CAP if n == N_BIG else 0)
        for mode in MODES:
            for at in U16_AT:
                run_var(var_batch, pv, n, mode, t, at)
                if kind == csum.KIND_SUBGROUP:
                    run_fixed(fixed77, pf, n, mode, t, at)
    reg.check_inputs()


@pytest.fixture(scope="module")
def span_uniform(oracle):
    """64-byte segments end to end from arena byte 0: a span range of 4096 *
    unroll bytes holds exactly 64 * unroll of them."""
    return VarBatch(oracle, 2 * 64 * 8 + 1, 0xC0F3, uniform=64)


@pytest.mark.gpu
@pytest.mark.parametrize("geo", SPAN_GEOMS)
def test_gpu_batch_arena_tuned_every_span_instance(var_batch, span_uniform, geo):
    """tulips_csum_batch_arena_tuned at every span instance: 64-byte segments
    filling exactly one range less one, one range, one more, two ranges and
    one; then 4099 mixed segments with gaps (ranges that hold no segment
    start, segments crossing ranges)."""
    reg = Registry(DEV)
    pu, _ku = span_uniform.device(reg)
    pv, _kv = var_batch.device(reg)
    per_wave, per_range = span_counts(geo)
    for nt in (1, 3):                                     # nt loads; nt loads and stores
        t = span_tuning(geo, nt=nt)
        for n in boundary_ns(per_wave, per_range, big=2 * per_range + 1):
            for mode in MODES:
                run_arena(span_uniform, pu, n, mode, t, U16_AT[nt == 3])
        for mode in MODES:
            for at in U16_AT:
                run_arena(var_batch, pv, N_BIG, mode, t, at)
            # the whole arena declared, a short batch in it: ranges past the
            # last segment have nothing to write
            run_arena(var_batch, pv, 33, mode, t, U16_AT[0], arena_bytes=var_batch.arena_bytes)
    reg.check_inputs()


@pytest.mark.gpu
@pytest.mark.parametrize("length", [64, 1500, 9000])
def test_gpu_batch_fixed_default_tuning(oracle, length):
    """tulips_csum_batch_fixed with the geometry it picks itself for 64, 1500
    and 9000 bytes; the grid-capped ragged round through the _tuned form with
    that same geometry."""
    b = FixedBatch(oracle, N_BIG, length, 0xC100 + length)
    reg = Registry(DEV)
    p, _keep = b.device(reg)
    d = csum.default_tuning(length)
    geom = (d.kind, d.group, d.unroll, d.nontemporal, d.sps)
    for n in boundary_ns(*batch_counts(geom, d.block)):
        for mode in MODES:
            for at in U16_AT:
                run_fixed(b, p, n, mode, None, at)
    capped = csum.Tuning(kind=d.kind, group=d.group, unroll=d.unroll, nontemporal=d.nontemporal,
                         sps=d.sps, block=d.block, max_blocks=CAP)
    for mode in MODES:
        run_fixed(b, p, N_BIG, mode, capped, U16_AT[0])
    reg.check_inputs()


@pytest.mark.gpu
def test_gpu_batch_variable_default_tuning(var_batch):
    """tulips_csum_batch and tulips_csum_batch_arena untuned (PACKED 8 x 4,
    the default span form), plus the capped ragged round of the default."""
    reg = Registry(DEV)
    p, _keep = var_batch.device(reg)
    d = csum.default_tuning(0, variable=True)
    geom = (d.kind, d.group, d.unroll, d.nontemporal, d.sps)
    for n in boundary_ns(*batch_counts(geom, d.block)):
        for mode in MODES:
            for at in U16_AT:
                run_var(var_batch, p, n, mode, None, at)
                run_arena(var_batch, p, n, mode, None, at)
    capped = csum.Tuning(kind=d.kind, group=d.group, unroll=d.unroll, nontemporal=d.nontemporal,
                         sps=d.sps, block=d.block, max_blocks=CAP)
    for mode in MODES:
        run_var(var_batch, p, N_BIG, mode, capped, U16_AT[0])
    reg.check_inputs()


# =============================================================================
# tulips_csum_verify, _verify_arena: the single bad_count word
# =============================================================================
def bad_of(exp):
    return int(np.count_nonzero(exp != 0xFFFF))


@pytest.mark.gpu
def test_gpu_verify_bad_count_word_two_streams_and_replay(var_batch):
    """bad_count is 4 bytes: the words around it stay intact, with and without
    `out`, for direct calls queued on two streams and for one call captured
    and replayed on a single stream."""
    b = var_batch
    reg = Registry(DEV)
    p, _keep = b.device(reg)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    d = csum.default_tuning(0, variable=True)
    ns = boundary_ns(*batch_counts((d.kind, d.group, d.unroll, 1, d.sps), d.block))
    jobs = []
    for k, n in enumerate(ns):
        for mode, arena_form in ((MODE_INET, False), (MODE_TCP, True), (MODE_TCP, False),
                                 (MODE_INET, True)):
            st = (s1, s2)[len(jobs) % 2].cuda_stream
            bad = guarded(4, np.uint32, align=U32_AT[0], skew=U32_AT[1], device=DEV)
            out = guarded((n,), np.uint16, align=16, skew=14, device=DEV) if k % 2 else None
            optr = out.ptr if out is not None else None
            if arena_form:
                rc = L.tulips_csum_verify_arena(p["arena"], b.end(n), p["offs"], p["lens"],
                                                p["src"], p["dst"], optr, bad.ptr, n, mode, st)
            else:
                rc = L.tulips_csum_verify(p["arena"], p["offs"], p["lens"], p["src"], p["dst"],
                                          optr, bad.ptr, n, mode, st)
            assert rc == 0
            jobs.append((n, mode, bad, out))
    torch.cuda.synchronize()
    for n, mode, bad, out in jobs:
        expect_all(bad, [bad_of(b.exp[mode][:n])])
        if out is not None:
            expect_all(out, b.exp[mode][:n])
    # captured on one stream (no parallel branches), replayed twice
    for arena_form in (False, True):
        cap = torch.cuda.Stream()
        n = N_BIG
        bad = guarded(4, np.uint32, align=U32_AT[0], skew=U32_AT[1], device=DEV)
        out = guarded((n,), np.uint16, align=16, skew=14, device=DEV)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=cap):
            if arena_form:
                rc = L.tulips_csum_verify_arena(p["arena"], b.end(n), p["offs"], p["lens"],
                                                p["src"], p["dst"], out.ptr, bad.ptr, n,
                                                MODE_TCP, cap.cuda_stream)
            else:
                rc = L.tulips_csum_verify(p["arena"], p["offs"], p["lens"], p["src"], p["dst"],
                                          out.ptr, bad.ptr, n, MODE_TCP, cap.cuda_stream)
        assert rc == 0
        _KEPT_GRAPHS.append(g)
        expect_none(bad)                       # a capture runs nothing
        expect_none(out)
        for rep in range(2):
            g.replay()
            torch.cuda.synchronize()
            expect_all(bad, [bad_of(b.exp[MODE_TCP][:n])])
            expect_all(out, b.exp[MODE_TCP][:n])
    reg.check_inputs()


# =============================================================================
# tulips_csum_batch_sg, _verify_sg, _batch_sg_tuned
# =============================================================================
class SgPlan:
    """n segments of 0..5 fragments, the first and the last segment empty
    (n >= 3), a fragment count that is no multiple of 64, fragments anywhere
    in an 8 KiB arena."""

    def __init__(self, oracle, n, seed):
        rng = np.random.default_rng(seed)
        counts = rng.integers(0, 6, n)
        if n >= 3:
            counts[[0, -1]] = 0
            counts[n // 2] = max(counts[n // 2], 1)
            if counts.sum() % 64 == 0:
                counts[n // 2] += 1
        else:
            counts[:] = 3
        nf = int(counts.sum())
        assert nf % 64 != 0
        self.n, self.nf = n, nf
        self.first = np.concatenate(([0], np.cumsum(counts))).astype(np.uint32)
        self.flens = np.where(rng.random(nf) < 0.5, rng.choice([0, 1, 2, 15, 16, 17, 33], nf),
                              rng.integers(0, 200, nf)).astype(np.uint16)
        self.arena = rng.integers(0, 256, 8192, dtype=np.uint8)
        self.foffs = rng.integers(0, 8192 - 256, nf).astype(np.uint64)
        self.seeds = rng.integers(0, 65536, n, dtype=np.uint32).astype(np.uint16)
        self.src = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        self.dst = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        self.exp = {m: sg_util.expected(oracle, self.arena, self.foffs, self.flens, self.first,
                                        seeds=self.seeds if m in MODES else None, src=self.src,
                                        dst=self.dst, mode=m)
                    for m in MODES + (MODE_INET, MODE_TCP)}

    KEYS = ("arena", "foffs", "flens", "first", "seeds", "src", "dst")

    def device(self, reg):
        d = {k: dev(getattr(self, k).view(np.int64) if k == "foffs" else getattr(self, k))
             for k in self.KEYS}
        for k, t in d.items():
            reg.ro(t, k)
        return {k: t.data_ptr() for k, t in d.items()}, d

    def host(self, reg):
        for k in self.KEYS:
            reg.ro(getattr(self, k), k)
        return {k: getattr(self, k).ctypes.data for k in self.KEYS}


@pytest.fixture(scope="module")
def sg_plans(oracle):
    ns = sorted(set(n for g in SG_GEOMETRIES for n in boundary_ns(*sg_counts(g))))
    return {n: SgPlan(oracle, n, 0x5600 + n) for n in ns}


@pytest.mark.gpu
@pytest.mark.parametrize("geom", SG_GEOMETRIES)
def test_gpu_sg_every_instance(sg_plans, geom):
    """tulips_csum_batch_sg (geom None) / _batch_sg_tuned at every instance:
    out[n]; tulips_csum_verify_sg: out[n] and the bad_count word. (The grid of
    these kernels is not capped: tuning.max_blocks is ignored.)"""
    t = None if geom is None else csum.Tuning(kind=csum.KIND_DEFAULT, group=geom[0],
                                              unroll=geom[1], nontemporal=geom[2], block=BLOCK)
    for n in boundary_ns(*sg_counts(geom)):
        pl = sg_plans[n]
        reg = Registry(DEV)
        p, _keep = pl.device(reg)
        for mode in MODES:
            for at in U16_AT:
                out = guarded((n,), np.uint16, align=at[0], skew=at[1], device=DEV)
                args = (p["arena"], p["foffs"], p["flens"], pl.nf, p["first"], *side(p, mode),
                        out.ptr, n, mode)
                rc = L.tulips_csum_batch_sg(*args, stream()) if t is None else \
                    L.tulips_csum_batch_sg_tuned(*args, t, stream())
                assert rc == 0
                expect_all(out, pl.exp[mode][:n])
        if geom is None:
            for mode, with_out in ((MODE_INET, True), (MODE_TCP, False), (MODE_TCP, True)):
                bad = guarded(4, np.uint32, align=U32_AT[0], skew=U32_AT[1], device=DEV)
                out = guarded((n,), np.uint16, align=16, skew=14, device=DEV)
                assert L.tulips_csum_verify_sg(p["arena"], p["foffs"], p["flens"], pl.nf,
                                               p["first"], p["src"], p["dst"],
                                               out.ptr if with_out else None, bad.ptr, n, mode,
                                               stream()) == 0
                expect_all(bad, [bad_of(pl.exp[mode])])
                if with_out:
                    expect_all(out, pl.exp[mode])
                else:
                    expect_none(out)           # the absent array appears nowhere
        reg.check_inputs()


# =============================================================================
# tulips_rss_toeplitz_batch
# =============================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4097])
def test_gpu_rss_out_confined(n):
    """out[n] (uint32) on the 4-tuples-per-thread path (every array 16-byte
    aligned: n / 4 vector stores plus the n % 4 tail) and on the one-tuple
    path (out ≡ 4 (mod 16); or the inputs one element in)."""
    rng = np.random.default_rng(0x7055 + n)
    m = n + 1
    arrs = dict(saddr=rng.integers(0, 2**32, m, dtype=np.uint64).astype(np.uint32),
                daddr=rng.integers(0, 2**32, m, dtype=np.uint64).astype(np.uint32),
                sport=rng.integers(0, 65536, m, dtype=np.uint32).astype(np.uint16),
                dport=rng.integers(0, 65536, m, dtype=np.uint32).astype(np.uint16))
    key = rng.integers(0, 256, 40, dtype=np.uint8).tobytes()
    kp, _keep = csum._buf(key)
    reg = Registry(DEV)
    t = {k: reg.ro(dev(v), k) for k, v in arrs.items()}
    for shift, skew in ((0, 0), (0, 4), (1, 0), (1, 4)):
        want = [csum.toeplitz(int(arrs["saddr"][shift + j]), int(arrs["daddr"][shift + j]),
                              int(arrs["sport"][shift + j]), int(arrs["dport"][shift + j]), key,
                              0x1234567) for j in range(n)]
        out = guarded((n,), np.uint32, align=16, skew=skew, device=DEV)
        assert L.tulips_rss_toeplitz_batch(
            t["saddr"].data_ptr() + 4 * shift, t["daddr"].data_ptr() + 4 * shift,
            t["sport"].data_ptr() + 2 * shift, t["dport"].data_ptr() + 2 * shift, n, kp,
            len(key), 0x1234567, out.ptr, stream()) == 0
        expect_all(out, want)
    reg.check_inputs()


# =============================================================================
# frames: validate, generate_fields, generate_frames
# =============================================================================
class Frames:
    """The validation fixture (every frame kind, in order, never overlapping)
    with mutations; a prefix of n frames with the arena cut right behind its
    last frame is a batch of its own."""

    def __init__(self, oracle, seed):
        fx = frames_fixture()
        rng = np.random.default_rng(seed)
        self.offs, self.lens = fx["offsets"], fx["lengths"]
        self.arena = mutate(fx, rng, 1500)
        self.flags = oracle.validate_frames(self.arena, self.offs, self.lens)
        self.gen_src = scramble_fields(fx, rng)
        self.oracle = oracle
        self._gen = {}

    def end(self, n):
        return int(self.offs[n - 1]) + int(self.lens[n - 1])

    def generated(self, n):
        """(arena prefix after generation, flags, fields) of frames [0, n)."""
        if n not in self._gen:
            a, f = self.oracle.generate_frames(self.gen_src[:self.end(n)], self.offs[:n],
                                               self.lens[:n])
            self._gen[n] = (a, f, fields_of(a, self.offs[:n], self.lens[:n], f))
        return self._gen[n]


@pytest.fixture(scope="module")
def frames(oracle):
    return Frames(oracle, 0xF4A3)


N_FRAMES_BIG = 2999               # odd, prime, within the 3000-frame fixture

FRAME_INSTANCES = [(g, u, 0) for (g, u) in FRAME_GEOMETRIES] + [(16, 6, 2), (16, 6, 3)]


def frame_ns(group, sps):
    return boundary_ns(*frame_counts(group, sps), big=N_FRAMES_BIG)


def validate_case(fr, n, call):
    """flags + counters, flags only, counters only through `call(flags_ptr,
    counters_ptr)`; the array that is absent stays pattern."""
    flags = guarded((n,), np.uint8, align=U8_AT[0], skew=U8_AT[1], device=DEV)
    cnt = guarded((4,), np.uint32, align=U32_AT[0], skew=U32_AT[1], device=DEV)
    assert call(flags.ptr, cnt.ptr) == 0
    expect_all(flags, fr.flags[:n])
    expect_all(cnt, counters_of(fr.flags[:n]))
    flags.reset()
    cnt.reset()
    assert call(flags.ptr, None) == 0
    expect_all(flags, fr.flags[:n])
    expect_none(cnt)
    flags.reset()
    assert call(None, cnt.ptr) == 0
    expect_none(flags)
    expect_all(cnt, counters_of(fr.flags[:n]))


@pytest.mark.gpu
@pytest.mark.parametrize("inst", FRAME_INSTANCES)
def test_gpu_validate_frames_every_instance(frames, inst):
    """tulips_csum_frames_tuned op 0 at every FRAME_GEOMETRIES instance and
    both sps forms of 16 x 6: flags[n] at an odd address and counters[4]."""
    group, unroll, sps = inst
    reg = Registry(DEV)
    a, o, ln = (reg.ro(dev(x)) for x in (frames.arena, frames.offs.view(np.int64), frames.lens))
    for n in frame_ns(group, sps):
        t = csum.Tuning(group=group, unroll=unroll, nontemporal=1, sps=sps, block=BLOCK,
                        max_blocks=CAP if n == N_FRAMES_BIG else 0)
        validate_case(frames, n, lambda f, c: L.tulips_csum_frames_tuned(
            0, a.data_ptr(), o.data_ptr(), ln.data_ptr(), n, f, c, t, stream()))
    reg.check_inputs()


@pytest.mark.gpu
def test_gpu_validate_frames_default_entry(frames):
    """tulips_csum_validate_frames itself, at the boundary n of every form
    the 16-lane default could take."""
    reg = Registry(DEV)
    a, o, ln = (reg.ro(dev(x)) for x in (frames.arena, frames.offs.view(np.int64), frames.lens))
    for n in sorted(set(frame_ns(16, 0) + frame_ns(16, 2) + frame_ns(16, 3))):
        validate_case(frames, n, lambda f, c: L.tulips_csum_validate_frames(
            a.data_ptr(), o.data_ptr(), ln.data_ptr(), n, f, c, stream()))
    reg.check_inputs()


def fields_case(fr, n, call):
    _a, eflags, efields = fr.generated(n)
    for with_flags in (True, False):
        fields = guarded((n,), np.uint32, align=U32_AT[0], skew=U32_AT[1], device=DEV)
        flags = guarded((n,), np.uint8, align=U8_AT[0], skew=U8_AT[1], device=DEV)
        assert call(fields.ptr, flags.ptr if with_flags else None) == 0
        expect_all(fields, efields)
        if with_flags:
            expect_all(flags, eflags)
        else:
            expect_none(flags)


def generate_case(fr, n, call):
    """In place: the arena (cut right behind frame n - 1, so the band starts
    there) byte for byte against the oracle, gaps included; flags[n]."""
    earena, eflags, _f = fr.generated(n)
    for with_flags in (True, False):
        arena = guarded(fr.end(n), np.uint8, align=16, skew=3, device=DEV)
        arena.fill(fr.gen_src[:fr.end(n)])
        flags = guarded((n,), np.uint8, align=U8_AT[0], skew=U8_AT[1], device=DEV)
        assert call(arena.ptr, flags.ptr if with_flags else None) == 0
        check(arena)
        np.testing.assert_array_equal(arena.host(), earena)
        if with_flags:
            expect_all(flags, eflags)
        else:
            expect_none(flags)


@pytest.mark.gpu
@pytest.mark.parametrize("geo", FRAME_GEOMETRIES)
def test_gpu_generate_every_instance(frames, geo):
    """tulips_csum_frames_tuned op 2 (fields[n], flags[n]; the arena only
    read) and op 1 (the arena against oracle.generate_frames, flags[n]) at
    every FRAME_GEOMETRIES instance."""
    group, unroll = geo
    reg = Registry(DEV)
    a = reg.ro(dev(frames.gen_src), "arena")
    o, ln = (reg.ro(dev(x)) for x in (frames.offs.view(np.int64), frames.lens))
    for n in frame_ns(group, 0):
        t = csum.Tuning(group=group, unroll=unroll, nontemporal=1, block=BLOCK,
                        max_blocks=CAP if n == N_FRAMES_BIG else 0)
        fields_case(frames, n, lambda fields, flags: L.tulips_csum_frames_tuned(
            2, a.data_ptr(), o.data_ptr(), ln.data_ptr(), n, flags, fields, t, stream()))
        generate_case(frames, n, lambda arena, flags: L.tulips_csum_frames_tuned(
            1, arena, o.data_ptr(), ln.data_ptr(), n, flags, None, t, stream()))
    reg.check_inputs()


@pytest.mark.gpu
def test_gpu_generate_default_entries(frames):
    """tulips_csum_generate_fields and tulips_csum_generate_frames themselves."""
    reg = Registry(DEV)
    a = reg.ro(dev(frames.gen_src), "arena")
    o, ln = (reg.ro(dev(x)) for x in (frames.offs.view(np.int64), frames.lens))
    for n in frame_ns(16, 0):
        fields_case(frames, n, lambda fields, flags: L.tulips_csum_generate_fields(
            a.data_ptr(), o.data_ptr(), ln.data_ptr(), n, fields, flags, stream()))
        generate_case(frames, n, lambda arena, flags: L.tulips_csum_generate_frames(
            arena, o.data_ptr(), ln.data_ptr(), n, flags, stream()))
    reg.check_inputs()


# =============================================================================
# tulips_csum_segment_frames and _planned
# =============================================================================
DOFFS = (5, 8, 15)


def payloads(mss):
    return (0, 1, mss - 1, mss, mss + 1, 3 * mss + 5, 20000)


def round16(x):
    return (x + 15) // 16 * 16


class SegCase:
    """Super-frames of every payload x doff, and per segment the exact bytes
    the oracle makes (computed at a stride that fits every segment, so the
    expectation at a smaller stride or capacity is built here from the
    header's rule, not taken from the oracle's own handling of limits)."""

    def __init__(self, oracle, mss, reps=1):
        rng = np.random.default_rng(0x5E6 + mss)
        fr = [super_frame(oracle, rng, p, doff=d) for d in DOFFS for p in payloads(mss)] * reps
        self.arena, self.offs, self.lens = pack_super(fr, rng)
        self.n, self.mss = len(fr), mss
        self.fit = round16(94 + mss)                 # 14 + 20 + 60 header bytes at most
        self.tight = round16(54 + mss)               # fits doff 5 only
        first, out, ol = oracle.segment_frames(self.arena, self.offs, self.lens, mss, self.fit)
        self.first = first
        self.total = int(first[-1])
        self.segs = [out[j * self.fit:j * self.fit + int(ol[j])].copy()
                     for j in range(self.total)]
        assert max(len(s) for s in self.segs) > self.tight >= min(len(s) for s in self.segs)

    def device(self, reg):
        d = (dev(self.arena), dev(self.offs.view(np.int64)), dev(self.lens))
        for t, k in zip(d, ("super-frames", "in_offsets", "in_lengths")):
            reg.ro(t, k)
        return d


@pytest.fixture(scope="module", params=[536, 1460])
def seg_case(oracle, request):
    return SegCase(oracle, request.param)


def expect_slots(out, olens, segs, stride, upto, whole=False):
    """Slots [0, upto) as the header says, everything else pattern. `segs[j]`
    is the segment's bytes, or None for a planned segment its frame does not
    make (length 0, nothing written). The slot-tail rule of the device forms:
    a segment of L bytes is written as whole 16-byte chunks, zeros from L to
    the next 16-byte boundary and nothing past it; a segment longer than the
    stride leaves its slot untouched and gets length 0. `whole`: the rule of
    tulips_csum_segment_frames_host, whose slots travel back whole: every
    slot j < upto is written to its full stride, zeros past the segment (a
    too-long segment's slot all zeros, length 0)."""
    want = out.view_pattern().copy()
    mask = np.zeros(out.nbytes, bool)
    lwant = olens.view_pattern().copy()
    lmask = np.zeros(olens.nbytes // 2, bool)
    for j in range(upto):
        lmask[j] = True
        s = segs[j]
        at = j * stride
        if whole:
            want[at:at + stride] = 0
            mask[at:at + stride] = True
        if s is None or len(s) > stride:
            lwant[j] = 0
            continue
        n_ = len(s)
        lwant[j] = n_
        want[at:at + n_] = s
        want[at + n_:at + round16(n_)] = 0
        mask[at:at + round16(n_)] = True
    check(out, mask)
    check(olens, lmask)
    got = out.host()
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"slot bytes differ at {bad[:8]} (slot {bad[0] // stride}, "
                             f"byte {bad[0] % stride}): {got[bad[:8]]} != {want[bad[:8]]}")
    np.testing.assert_array_equal(olens.host(), lwant)


def seg_buffers(view_slots, stride, n, device=DEV):
    out = guarded(view_slots * stride, np.uint8, align=16, skew=0, slot=stride, device=device)
    olens = guarded((view_slots,), np.uint16, align=16, skew=14, device=device)
    first = guarded((n + 1,), np.uint32, align=U32_AT[0], skew=U32_AT[1], device=device)
    return out, olens, first


def seg_limits(c):
    """(stride, slots in the view, capacity passed) of the limit cases."""
    return [("capacity == total", c.fit, c.total, c.total),
            ("capacity below the total", c.fit, c.total, c.total // 2 + 1),
            ("capacity above the total", c.fit, c.total + 7, c.total + 7),
            ("stride too small for some", c.tight, c.total, c.total),
            ("capacity 0", c.fit, 4, 0)]


@pytest.mark.gpu
def test_gpu_segment_frames_confined(seg_case):
    """tulips_csum_segment_frames: the slot array, out_lengths[capacity] and
    out_first[n + 1], under every limit of the header."""
    c = seg_case
    reg = Registry(DEV)
    a, o, ln = c.device(reg)
    for what, stride, slots, capacity in seg_limits(c):
        out, olens, first = seg_buffers(slots, stride, c.n)
        assert L.tulips_csum_segment_frames(a.data_ptr(), o.data_ptr(), ln.data_ptr(), c.n, c.mss,
                                            out.ptr, stride, capacity, olens.ptr, first.ptr,
                                            stream()) == 0, what
        expect_all(first, c.first)                  # complete whatever the capacity
        expect_slots(out, olens, c.segs, stride, min(c.total, capacity))
    reg.check_inputs()


@pytest.mark.gpu
def test_gpu_segment_frames_planned_confined(seg_case):
    """tulips_csum_segment_frames_planned under the same limits (the plan is
    an input), and with a plan that promises frame 1 two segments more than
    its header makes: those get length 0 and pattern-only slots."""
    c = seg_case
    reg = Registry(DEV)
    a, o, ln = c.device(reg)
    plan = reg.ro(dev(c.first.view(np.int32)), "plan")
    for what, stride, slots, capacity in seg_limits(c):
        out, olens, _first = seg_buffers(slots, stride, c.n)
        assert L.tulips_csum_segment_frames_planned(
            a.data_ptr(), o.data_ptr(), ln.data_ptr(), c.n, c.mss, plan.data_ptr(), out.ptr,
            stride, capacity, olens.ptr, stream()) == 0, what
        expect_slots(out, olens, c.segs, stride, min(c.total, capacity))
    bad = c.first.astype(np.int64)
    bad[2:] += 2
    e1 = int(c.first[2])
    segs = c.segs[:e1] + [None, None] + c.segs[e1:]
    bad_plan = reg.ro(dev(bad.astype(np.int32)), "bad plan")
    for capacity in (c.total + 2, e1 + 1, c.total + 9):
        out, olens, _first = seg_buffers(c.total + 9, c.fit, c.n)
        assert L.tulips_csum_segment_frames_planned(
            a.data_ptr(), o.data_ptr(), ln.data_ptr(), c.n, c.mss, bad_plan.data_ptr(), out.ptr,
            c.fit, capacity, olens.ptr, stream()) == 0
        expect_slots(out, olens, segs, c.fit, min(c.total + 2, capacity))
    reg.check_inputs()


# =============================================================================
# host forms: numpy guarded arrays, several staging chunks
# =============================================================================
CHUNK = 1 << 17


@pytest.mark.gpu
def test_gpu_batch_host_confined(var_batch):
    """tulips_csum_batch_host: out[n] in host memory across several staging
    chunks (the chunk-wise copy-back)."""
    b = var_batch
    assert b.arena_bytes > 3 * CHUNK
    reg = Registry()
    p = b.host(reg)
    with csum.HostContext(0, chunk_bytes=CHUNK) as ctx:
        for n in (1, 2, 33, N_BIG):
            for mode in MODES:
                at = U16_AT[n % 2]
                out = guarded((n,), np.uint16, align=at[0], skew=at[1])
                assert L.tulips_csum_batch_host(ctx._h, p["arena"], p["offs"], p["lens"],
                                                *side(p, mode), out.ptr, n, mode) == 0
                expect_all(out, b.exp[mode][:n])
    reg.check_inputs()


@pytest.mark.gpu
def test_gpu_validate_frames_host_confined(frames):
    fr = frames
    reg = Registry()
    for x in (fr.arena, fr.offs, fr.lens):
        reg.ro(x)
    assert len(fr.arena) > 3 * CHUNK
    with csum.HostContext(0, chunk_bytes=CHUNK) as ctx:
        for n in (1, 17, N_FRAMES_BIG):
            for with_counters in (True, False):
                flags = guarded((n,), np.uint8, align=U8_AT[0], skew=U8_AT[1])
                cnt = guarded((4,), np.uint32, align=U32_AT[0], skew=U32_AT[1])
                assert L.tulips_csum_validate_frames_host(
                    ctx._h, fr.arena.ctypes.data, fr.offs.ctypes.data, fr.lens.ctypes.data, n,
                    flags.ptr, cnt.ptr if with_counters else None) == 0
                expect_all(flags, fr.flags[:n])
                if with_counters:
                    expect_all(cnt, counters_of(fr.flags[:n]))
                else:
                    expect_none(cnt)
    reg.check_inputs()


@pytest.mark.gpu
def test_gpu_generate_frames_host_confined(frames):
    """Only the 4 field bytes per frame come back into the arena: the whole
    arena against the oracle, the band right behind the last frame."""
    fr = frames
    reg = Registry()
    reg.ro(fr.offs)
    reg.ro(fr.lens)
    with csum.HostContext(0, chunk_bytes=CHUNK) as ctx:
        for n in (1, 17, N_FRAMES_BIG):
            earena, eflags, _f = fr.generated(n)
            for with_flags in (True, False):
                arena = guarded(fr.end(n), np.uint8, align=16, skew=3)
                arena.fill(fr.gen_src[:fr.end(n)])
                flags = guarded((n,), np.uint8, align=U8_AT[0], skew=U8_AT[1])
                assert L.tulips_csum_generate_frames_host(
                    ctx._h, arena.ptr, fr.offs.ctypes.data, fr.lens.ctypes.data, n,
                    flags.ptr if with_flags else None) == 0
                check(arena)
                np.testing.assert_array_equal(arena.host(), earena)
                if with_flags:
                    expect_all(flags, eflags)
                else:
                    expect_none(flags)
    reg.check_inputs()


@pytest.mark.gpu
def test_gpu_segment_frames_host_confined(oracle):
    """tulips_csum_segment_frames_host over several staging chunks: capacity
    equal to, below and far above the total (2^31 - 1 declared, the caller's
    arrays holding the real output only), a stride too small for some, and
    capacity 0. Slots j < min(total, capacity) come back whole (segment, then
    zeros to the stride); no other slot or length is touched."""
    c = SegCase(oracle, 1460, reps=4)
    assert len(c.arena) > 2 * CHUNK
    reg = Registry()
    for x in (c.arena, c.offs, c.lens):
        reg.ro(x)
    with csum.HostContext(0, chunk_bytes=CHUNK) as ctx:
        for stride, slots, capacity in ((c.fit, c.total, c.total),
                                        (c.fit, c.total, c.total // 2 + 1),
                                        (c.tight, c.total, c.total),
                                        (c.fit, c.total, (1 << 31) - 1),
                                        (c.fit, 4, 0)):
            out, olens, first = seg_buffers(slots, stride, c.n, device=None)
            assert L.tulips_csum_segment_frames_host(
                ctx._h, c.arena.ctypes.data, c.offs.ctypes.data, c.lens.ctypes.data, c.n, c.mss,
                out.ptr, stride, capacity, olens.ptr, first.ptr) == 0
            expect_all(first, c.first)
            expect_slots(out, olens, c.segs, stride, min(c.total, capacity), whole=True)
    reg.check_inputs()


# =============================================================================
# multi-device contexts on devices [0, 0]
# =============================================================================
def odd_bound_n(lens, start):
    """The largest odd n <= start whose byte-balanced two-shard bound is odd."""
    for n in range(start, start - 200, -2):
        if int(csum.shard_plan(lens[:n], 2)[1]) % 2 == 1:
            return n
    raise AssertionError("no n with an odd shard bound")


@pytest.mark.gpu
def test_gpu_mctx_host_confined(var_batch, frames):
    """tulips_csum_mctx_batch_host and _mctx_validate_frames_host scatter two
    shards' results into one caller array; the shard bound is odd."""
    b = var_batch
    reg = Registry()
    p = b.host(reg)
    n = odd_bound_n(b.lens, N_BIG)
    with csum.MultiContext([0, 0], chunk_bytes=CHUNK) as m:
        for mode in MODES:
            for at in U16_AT:
                out = guarded((n,), np.uint16, align=at[0], skew=at[1])
                assert L.tulips_csum_mctx_batch_host(m._h, p["arena"], p["offs"], p["lens"],
                                                     *side(p, mode), out.ptr, n, mode) == 0
                assert int(m.bounds()[1]) % 2 == 1
                expect_all(out, b.exp[mode][:n])
        fr = frames
        for x in (fr.arena, fr.offs, fr.lens):
            reg.ro(x)
        nf = odd_bound_n(fr.lens, N_FRAMES_BIG)
        for with_counters in (True, False):
            flags = guarded((nf,), np.uint8, align=U8_AT[0], skew=U8_AT[1])
            cnt = guarded((4,), np.uint32, align=U32_AT[0], skew=U32_AT[1])
            assert L.tulips_csum_mctx_validate_frames_host(
                m._h, fr.arena.ctypes.data, fr.offs.ctypes.data, fr.lens.ctypes.data, nf,
                flags.ptr, cnt.ptr if with_counters else None) == 0
            assert int(m.bounds()[1]) % 2 == 1
            expect_all(flags, fr.flags[:nf])
            if with_counters:
                expect_all(cnt, counters_of(fr.flags[:nf]))
            else:
                expect_none(cnt)
    reg.check_inputs()


def odd_cut_n(b, start):
    """The largest odd n <= start for which the first segment starting at or
    after the middle byte of the prefix arena (where the device form cuts it
    for two devices) has an odd index, with no segment start within 2 bytes
    of the cut."""
    offs = b.offs.astype(np.int64)
    for n in range(start, start - 400, -2):
        cut = b.end(n) // 2
        i = [int(np.searchsorted(offs[:n], cut + d, "left")) for d in (-2, 0, 2)]
        if i[0] == i[2] and i[1] % 2 == 1:
            return n
    raise AssertionError("no n with an odd cut")


@pytest.mark.gpu
def test_gpu_mctx_device_confined(var_batch, fixed77):
    """tulips_csum_mctx_batch_arena_device and _batch_fixed_device: the second
    logical device sends its results home into out[bound:]; the bound the
    context reports is odd for at least one n of each form (fixed: n / 2 of
    4099; arena: the n chosen by odd_cut_n)."""
    reg = Registry(DEV)
    pv, _kv = var_batch.device(reg)
    pf, _kf = fixed77.device(reg)
    odd = {"arena": False, "fixed": False}
    with csum.MultiContext([0, 0]) as m:
        for n in (N_BIG, odd_cut_n(var_batch, N_BIG - 2), 3, 1):
            for mode in MODES:
                at = U16_AT[mode == TCP_GEN]
                out = guarded((n,), np.uint16, align=at[0], skew=at[1], device=DEV)
                assert L.tulips_csum_mctx_batch_arena_device(
                    m._h, pv["arena"], var_batch.end(n), pv["offs"], pv["lens"],
                    *side(pv, mode), out.ptr, n, mode, stream()) == 0
                torch.cuda.synchronize()
                odd["arena"] |= int(m.bounds()[1]) % 2 == 1
                expect_all(out, var_batch.exp[mode][:n])
                out = guarded((n,), np.uint16, align=at[0], skew=at[1], device=DEV)
                assert L.tulips_csum_mctx_batch_fixed_device(
                    m._h, pf["arena"], fixed77.stride, fixed77.length, *side(pf, mode), out.ptr,
                    n, mode, stream()) == 0
                torch.cuda.synchronize()
                odd["fixed"] |= int(m.bounds()[1]) % 2 == 1
                expect_all(out, fixed77.exp[mode][:n])
    assert odd["arena"] and odd["fixed"], odd
    reg.check_inputs()


# =============================================================================
# CPU entries (no GPU involved)
# =============================================================================
def test_validate_frames_cpu_confined(frames):
    fr = frames
    reg = Registry()
    for x in (fr.arena, fr.offs, fr.lens):
        reg.ro(x)
    for n in (1, 2, 17, N_FRAMES_BIG):
        for want_flags, want_cnt in ((True, True), (True, False), (False, True)):
            flags = guarded((n,), np.uint8, align=U8_AT[0], skew=U8_AT[1])
            cnt = guarded((4,), np.uint32, align=U32_AT[0], skew=U32_AT[1])
            assert L.tulips_csum_validate_frames_cpu(
                fr.arena.ctypes.data, fr.offs.ctypes.data, fr.lens.ctypes.data, n,
                flags.ptr if want_flags else None, cnt.ptr if want_cnt else None) == 0
            if want_flags:
                expect_all(flags, fr.flags[:n])
            else:
                expect_none(flags)
            if want_cnt:
                expect_all(cnt, counters_of(fr.flags[:n]))
            else:
                expect_none(cnt)
    reg.check_inputs()


def test_batch_sg_cpu_confined(oracle):
    for n in (1, 3, 9, 257):
        pl = SgPlan(oracle, n, 0x5700 + n)
        reg = Registry()
        p = pl.host(reg)
        for mode in MODES + (MODE_TCP,):
            for want_out, want_bad in ((True, True), (True, False), (False, True)):
                out = guarded((n,), np.uint16, align=16, skew=14)
                bad = guarded(4, np.uint32, align=U32_AT[0], skew=U32_AT[1])
                assert L.tulips_csum_batch_sg_cpu(
                    p["arena"], p["foffs"], p["flens"], pl.nf, p["first"], *side(p, mode),
                    out.ptr if want_out else None, bad.ptr if want_bad else None, n, mode) == 0
                if want_out:
                    expect_all(out, pl.exp[mode])
                else:
                    expect_none(out)
                if want_bad:
                    ok = 0 if mode & FLAG_COMPLEMENT else 0xFFFF
                    expect_all(bad, [int(np.count_nonzero(pl.exp[mode] != ok))])
                else:
                    expect_none(bad)
        # a rejected plan writes nothing at all: seg_first decreasing, and
        # seg_first[n] past nfrags
        for broken in ("decreasing", "past nfrags"):
            first = pl.first.copy()
            if broken == "decreasing":
                if n < 3:
                    continue
                first[n // 2] = first[-1] + 1
            else:
                first[-1] = pl.nf + 1
            out = guarded((n,), np.uint16, align=16, skew=14)
            bad = guarded(4, np.uint32, align=U32_AT[0], skew=U32_AT[1])
            assert L.tulips_csum_batch_sg_cpu(
                p["arena"], p["foffs"], p["flens"], pl.nf, first.ctypes.data, p["seeds"], None,
                None, out.ptr, bad.ptr, n, MODE_RAW) == csum.STATUS_INVALID_ARGUMENT, broken
            expect_none(out)
            expect_none(bad)
        reg.check_inputs()


@pytest.mark.parametrize("mss", [536, 1460])
def test_segment_plan_host_confined(oracle, mss):
    c = SegCase(oracle, mss)
    reg = Registry()
    for x in (c.arena, c.offs, c.lens):
        reg.ro(x)
    for n in (1, 2, c.n):
        first = guarded((n + 1,), np.uint32, align=U32_AT[0], skew=U32_AT[1])
        assert L.tulips_csum_segment_plan_host(c.arena.ctypes.data, c.offs.ctypes.data,
                                               c.lens.ctypes.data, n, mss, first.ptr) == 0
        expect_all(first, c.first[:n + 1])
    reg.check_inputs()


def test_shard_plan_confined(oracle):
    lens = oracle.zipf_lengths(N_BIG)
    reg = Registry()
    reg.ro(lens)
    pre = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    for n in (0, 1, 2, N_BIG):
        for k in (1, 2, 3, 8, 64):
            bounds = guarded((k + 1,), np.uint32, align=U32_AT[0], skew=U32_AT[1])
            assert L.tulips_csum_shard_plan(lens.ctypes.data, n, k, bounds.ptr) == 0
            # shard j starts at the first segment whose prefix reaches j/k of the bytes
            total = int(pre[n])
            want = [min(int(np.searchsorted(pre[:n + 1], -(-total * j // k), "left")), n)
                    for j in range(k)] + [n]
            want[0] = 0
            expect_all(bounds, want)
    reg.check_inputs()
