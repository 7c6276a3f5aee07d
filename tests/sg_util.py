"""Helpers of the scatter-gather tests (tests/test_sg*.py): plans of
fragments, their concatenated form for the oracle, and fixtures cut into
fragments. Expected values always come from the oracle / the reference over
the concatenated bytes, never from the library."""
import numpy as np


def concat(arena, foffs, flens, first):
    """The contiguous batch a scatter-gather plan stands for: (arena, offsets,
    lengths) with segment i = the bytes of fragments first[i] .. first[i+1]-1
    in order."""
    arena = np.asarray(arena, dtype=np.uint8)
    foffs = np.asarray(foffs, dtype=np.uint64).astype(np.int64)
    flens = np.asarray(flens, dtype=np.uint16).astype(np.int64)
    first = np.asarray(first, dtype=np.uint32).astype(np.int64)
    n = len(first) - 1
    nf = int(first[-1]) if n >= 0 and len(first) else 0
    total = int(flens[:nf].sum())
    # gather index: for every byte of every fragment, its arena position
    starts = np.repeat(foffs[:nf], flens[:nf])
    fpos = np.concatenate(([0], np.cumsum(flens[:nf])))
    within = np.arange(total, dtype=np.int64) - np.repeat(fpos[:-1], flens[:nf])
    flat = arena[starts + within] if total else np.zeros(0, np.uint8)
    offs = fpos[first[:-1]].astype(np.uint64)
    lens = (fpos[first[1:]] - fpos[first[:-1]])
    assert lens.max(initial=0) <= 65535
    return np.concatenate((flat, np.zeros(8, np.uint8))), offs, lens.astype(np.uint16)


def expected(checker, arena, foffs, flens, first, *, seeds=None, src=None, dst=None, mode=0):
    """What `checker` (Oracle / Reference) gives over the concatenated bytes."""
    flat, offs, lens = concat(arena, foffs, flens, first)
    return checker.batch(flat, offs, lens, seeds=seeds, src=src, dst=dst, mode=mode, nthreads=4)


def cut(rng, offs, lens, max_frags):
    """Cut every segment [offs[i], offs[i] + lens[i]) at seeded points into 1
    to max_frags fragments, still in place (cut points may coincide: empty
    fragments). Returns (frag_offsets, frag_lengths, seg_first)."""
    foffs, flens, first = [], [], [0]
    for o, ln in zip(np.asarray(offs).astype(np.int64), np.asarray(lens).astype(np.int64)):
        k = int(rng.integers(1, max_frags + 1))
        cuts = np.sort(rng.integers(0, ln + 1, k - 1))
        edges = np.concatenate(([0], cuts, [ln]))
        foffs.extend((o + edges[:-1]).tolist())
        flens.extend(np.diff(edges).tolist())
        first.append(len(foffs))
    return (np.array(foffs, dtype=np.uint64), np.array(flens, dtype=np.uint16),
            np.array(first, dtype=np.uint32))


def relocate(rng, arena, foffs, flens, fill=0xFF):
    """Copy every fragment to a seeded offset and alignment in a second arena
    filled with `fill`, in a shuffled order with gaps, so that any neighbour
    byte leaking into a sum changes it. Returns (arena2, frag_offsets2)."""
    arena = np.asarray(arena, dtype=np.uint8)
    nf = len(foffs)
    order = rng.permutation(nf)
    gaps = rng.integers(1, 40, nf)
    ln = np.asarray(flens).astype(np.int64)
    pos = np.zeros(nf, dtype=np.int64)
    at = int(rng.integers(0, 16))
    for j, g in zip(order, gaps):
        pos[j] = at
        at += int(ln[j]) + int(g)
    out = np.full(at + 64, fill, dtype=np.uint8)
    for j in range(nf):
        o = int(foffs[j])
        out[pos[j]:pos[j] + ln[j]] = arena[o:o + ln[j]]
    return out, pos.astype(np.uint64)


def random_plan(rng, n, *, max_frags=6, special=(0, 1, 2, 3, 15, 16, 17, 31, 33, 1460),
                max_len=3000, fill=None):
    """A seeded plan: 0..max_frags fragments per segment, lengths from
    `special` or random, fragments at any alignment (each of 0..15 used in
    turn), possibly overlapping, in an arena of random bytes (or `fill`)."""
    counts = rng.integers(0, max_frags + 1, n)
    nf = int(counts.sum())
    flens = np.where(rng.random(nf) < 0.6, rng.choice(np.array(special), nf),
                     rng.integers(0, max_len, nf)).astype(np.int64)
    # keep every segment within 65535
    first = np.concatenate(([0], np.cumsum(counts))).astype(np.uint32)
    for i in range(n):
        s, e = int(first[i]), int(first[i + 1])
        while flens[s:e].sum() > 65535:
            flens[s:e] //= 2
    nbytes = max(int(flens.sum()) // 2, int(flens.max(initial=0))) + 4096
    foffs = rng.integers(0, (nbytes - flens.max(initial=0) - 16) // 16, nf) * 16 + \
        (np.arange(nf) % 16)
    if fill is None:
        arena = rng.integers(0, 256, nbytes, dtype=np.uint8)
    else:
        arena = np.full(nbytes, fill, dtype=np.uint8)
    return arena, foffs.astype(np.uint64), flens.astype(np.uint16), first
