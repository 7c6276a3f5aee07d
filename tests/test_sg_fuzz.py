"""Seeded, time-budgeted fuzz of the scatter-gather device entry points
(tulips_csum_batch_sg, every shipped instance, and tulips_csum_verify_sg)
against the oracle over the concatenated bytes, in the manner of
tests/test_fuzz.py.

Each case draws a segment count (0 to 6,000, log-uniform), a fragments-per-
segment mix (none, a few, runs past the 64-fragment batch), a length mix
(empty, tiny, MTU-like header + payload, up to the 65535 total), fragments at
any alignment that may overlap, an arena with all-0x00 / all-0xFF stretches,
a mode and a kernel instance. Bar: bit-exact.

TULIPS_FUZZ_SECONDS (default 2) bounds the run; TULIPS_FUZZ_SEED (default 1)
picks the sequence. A failure names its case seed; TULIPS_FUZZ_CASE=<case
seed> runs that case alone.
"""
import os
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import FLAG_COMPLEMENT, MODE_INET, MODE_RAW, MODE_TCP  # noqa: E402

import sg_util  # noqa: E402
from tulips_amd import csum  # noqa: E402

DEV = "cuda:0"
BYTES_MAX = 24 << 20    # fragment bytes per case


def _d(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def _counts(rng, n):
    kind = rng.integers(0, 4)
    if kind == 0:       # header + payload
        return np.full(n, 2)
    if kind == 1:       # a few
        return rng.integers(0, 6, n)
    if kind == 2:       # mostly one, some long runs across the fragment batch
        c = np.ones(n, dtype=np.int64)
        c[rng.random(n) < 0.05] = rng.integers(60, 200)
        return c
    c = rng.integers(0, 4, n)   # runs of empty segments
    if n > 70:
        s = int(rng.integers(0, n - 70))
        c[s:s + 70] = 0
    return c


def _frag_lengths(rng, counts):
    nf = int(counts.sum())
    kind = rng.integers(0, 4)
    if kind == 0:
        lens = rng.integers(0, 80, nf)
    elif kind == 1:
        lens = rng.integers(0, 1500, nf)
        lens[rng.random(nf) < 0.3] = 20
    elif kind == 2:
        lens = rng.integers(0, 65536, nf)
    else:
        lens = rng.integers(0, 3000, nf)
        lens[rng.random(nf) < 0.3] = 0
    lens = lens.astype(np.int64)
    first = np.concatenate(([0], np.cumsum(counts)))
    # every segment within 65535, the case within its byte budget
    seg_of = np.repeat(np.arange(len(counts)), counts)
    tot = np.bincount(seg_of, weights=lens, minlength=len(counts))
    over = tot[seg_of] > 65535
    lens[over] = (lens[over] * 65535 // np.maximum(tot[seg_of][over], 1)).astype(np.int64)
    if lens.sum() > BYTES_MAX:
        lens = lens * BYTES_MAX // int(lens.sum())
    return lens.astype(np.uint16), first.astype(np.uint32)


def _case(oracle, seed):
    rng = np.random.default_rng(seed)
    n = int(np.exp(rng.uniform(0, np.log(6001)))) - 1
    counts = _counts(rng, n).astype(np.int64)
    flens, first = _frag_lengths(rng, counts)
    nf = len(flens)
    nbytes = max(int(flens.astype(np.int64).sum()) // 2, 65536) + 65536 + 64
    arena = rng.integers(0, 256, nbytes, dtype=np.uint8)
    for _ in range(int(rng.integers(0, 4))):
        s = int(rng.integers(0, nbytes - 1))
        arena[s:s + int(rng.integers(1, 70000))] = 0xFF if rng.random() < 0.5 else 0
    foffs = rng.integers(0, nbytes - 65536, nf).astype(np.uint64)
    mode = [MODE_RAW, MODE_INET, MODE_TCP][int(rng.integers(0, 3))]
    if rng.random() < 0.3:
        mode |= FLAG_COMPLEMENT
    seeds = rng.integers(0, 65536, n, dtype=np.uint32).astype(np.uint16) \
        if rng.random() < 0.5 and (mode & 0xff) != MODE_TCP else None
    src = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    dst = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    geoms = [None] + [(s, u, nt) for (s, u) in csum.SG_GEOMETRIES for nt in (0, 1)]
    geom = geoms[int(rng.integers(0, len(geoms)))]
    tuning = None if geom is None else csum.Tuning(kind=csum.KIND_DEFAULT, group=geom[0],
                                                   unroll=geom[1], nontemporal=geom[2])
    what = f"case seed {seed}: n={n} nfrags={nf} mode={mode:#x} geometry={geom}"
    exp = sg_util.expected(oracle, arena, foffs, flens, first, seeds=seeds, src=src, dst=dst,
                           mode=mode)
    da, do, dl, df = _d(arena), _d(foffs), _d(flens), _d(first)
    dsrc, ddst = _d(src), _d(dst)
    got = csum.batch_sg(da, do, dl, df, seeds=None if seeds is None else _d(seeds), src=dsrc,
                        dst=ddst, mode=mode, tuning=tuning)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint16), exp,
                                  err_msg=f"batch_sg {what}")
    vmode = mode & 0xff
    if vmode in (MODE_INET, MODE_TCP):
        vexp = exp if (seeds is None and mode == vmode) else \
            sg_util.expected(oracle, arena, foffs, flens, first, src=src, dst=dst, mode=vmode)
        out = torch.zeros(max(n, 1), dtype=torch.int16, device=DEV)
        bad = csum.verify_sg(da, do, dl, df, src=dsrc, dst=ddst, mode=vmode,
                             out=out if rng.random() < 0.5 else None)
        torch.cuda.synchronize()
        assert int(bad.item()) == int(np.count_nonzero(vexp != 0xFFFF)), f"verify_sg {what}"


def test_fuzz_scatter_gather_vs_oracle(oracle):
    if os.environ.get("TULIPS_FUZZ_CASE"):
        _case(oracle, int(os.environ["TULIPS_FUZZ_CASE"]))
        return
    budget = float(os.environ.get("TULIPS_FUZZ_SECONDS", "2"))
    seed0 = int(os.environ.get("TULIPS_FUZZ_SEED", "1"))
    t0 = last = time.monotonic()
    done = 0
    while done == 0 or time.monotonic() - t0 < budget:
        _case(oracle, seed0 * 1_000_117 + done)
        done += 1
        if time.monotonic() - last > 20:
            last = time.monotonic()
            print(f"fuzz sg: {done} cases, {last - t0:.0f} s", flush=True)
    print(f"fuzz sg: {done} cases in {time.monotonic() - t0:.1f} s", flush=True)
    assert done >= 1
