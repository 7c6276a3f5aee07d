"""Guard-banded buffers for the write-confinement tests (tests/test_confinement.py).

The suite checks WHAT a kernel writes against the oracle; this module checks
WHERE. An output handed to the library is a view inside a larger allocation
whose every byte, view included, holds a seeded, position-dependent pattern.
After the call `check()` reads the whole allocation back: the bands on both
sides must still hold the pattern (a store before out[0] or past out[n-1]
lands there instead of in the allocator's unread slack), and so must every
byte of the view the contract says is not written. Inputs the header calls
"only read" / "not modified" are snapshotted and compared byte for byte.

Nothing here provokes a fault: a stray store of up to a band's width lands in
memory the test owns.
"""
import itertools

import numpy as np

# Each band is at least this many bytes, 64 elements, and (slot outputs) two
# whole slots.
MIN_BAND = 4096
# The pattern never holds these bytes, so a stray store of 0, 0xffff or of one
# of the poisons the suite used before (0xA5, 0xAB) differs from it at every
# byte, not with probability 255/256.
AVOID = (0x00, 0xFF, 0xA5, 0xAB)
_REMAP = 0x11                     # x ^ 0x11 maps AVOID onto bytes outside AVOID

_serial = itertools.count(1)


def pattern(nbytes, seed):
    """`nbytes` seeded bytes, different at every position and for every seed,
    none of them in AVOID."""
    p = np.random.default_rng([0x6A5D, int(seed)]).integers(0, 256, int(nbytes), dtype=np.uint8)
    for v in AVOID:
        p[p == v] = v ^ _REMAP
    return p


def _nbytes(nbytes_or_shape, itemsize):
    if isinstance(nbytes_or_shape, (tuple, list)):
        return int(np.prod(nbytes_or_shape, dtype=np.int64)) * itemsize
    return int(nbytes_or_shape)


class Guarded:
    """A view of `nbytes` inside a pattern-filled backing buffer.

    .view     the view: a uint8 torch tensor (device) or a numpy array of
              `dtype` (host); memory the library may write
    .ptr      address of its first element (what the C ABI takes)
    .host()   the view's current content as a numpy array of `dtype`
    .fill(a)  put `a` into the view (an in-place arena: generation)
    .reset()  the whole buffer back to the pattern, for another call
    .view_pattern()  what the view held before the call, as `dtype`
    """

    def __init__(self, backing, start, nbytes, dtype, pat, device):
        self.backing, self.start, self.nbytes = backing, start, nbytes
        self.dtype, self.pattern, self.device = np.dtype(dtype), pat, device
        if device is None:
            self.ptr = backing.ctypes.data + start
            self.view = backing[start:start + nbytes].view(self.dtype)
        else:
            self.ptr = backing.data_ptr() + start
            self.view = backing[start:start + nbytes]

    def _bytes(self):
        """The whole backing buffer as host bytes (after a synchronize)."""
        if self.device is None:
            return self.backing
        if self.backing.is_cuda:
            import torch
            torch.cuda.synchronize()
        return self.backing.cpu().numpy()

    def host(self):
        b = self._bytes()[self.start:self.start + self.nbytes]
        return np.array(b, copy=True).view(self.dtype)

    def fill(self, data):
        raw = np.ascontiguousarray(data).view(np.uint8).ravel()
        assert raw.size == self.nbytes, (raw.size, self.nbytes)
        if self.device is None:
            self.backing[self.start:self.start + self.nbytes] = raw
        else:
            import torch
            self.view.copy_(torch.from_numpy(raw.copy()))

    def reset(self):
        """Every byte, view included, back to the pattern (before another
        call into the same buffer)."""
        if self.device is None:
            self.backing[:] = self.pattern
        else:
            import torch
            self.backing.copy_(torch.from_numpy(self.pattern.copy()))

    def view_pattern(self):
        """The pattern the view held before the call, as `dtype`."""
        return self.pattern[self.start:self.start + self.nbytes].copy().view(self.dtype)


def guarded(nbytes_or_shape, dtype=np.uint8, *, align=16, skew=0, device=None, slot=0,
            seed=None):
    """A Guarded view of `nbytes_or_shape` (a byte count, or a shape of
    `dtype` elements) whose first element lies at an address ≡ `skew`
    (mod `align`), with a band of at least MIN_BAND bytes, 64 elements and two
    `slot`-byte slots on each side. `device` None = host (numpy), else a torch
    device. `align` is a power of two; `skew` keeps the element's natural
    alignment (a uint16 never sits at an odd address)."""
    dt = np.dtype(dtype)
    nbytes = _nbytes(nbytes_or_shape, dt.itemsize)
    assert align >= 1 and align & (align - 1) == 0 and 0 <= skew < align
    assert skew % min(dt.itemsize, align) == 0, "skew must keep the natural alignment"
    band = max(MIN_BAND, 64 * dt.itemsize, 2 * int(slot))
    total = band + align + nbytes + band
    pat = pattern(total, next(_serial) if seed is None else seed)
    if device is None:
        backing = pat.copy()
        base = backing.ctypes.data
    else:
        import torch
        backing = torch.from_numpy(pat.copy()).to(device)
        base = backing.data_ptr()
    start = band + (skew - (base + band)) % align
    g = Guarded(backing, start, nbytes, dt, pat, device)
    assert g.ptr % align == skew and start >= band and total - start - nbytes >= band
    return g


def _describe(idx, got, want, origin):
    idx = idx[:8]
    return ", ".join(f"{int(i) - origin:+d}: found 0x{int(got[i]):02x} (pattern 0x{int(want[i]):02x})"
                     for i in idx)


def check(g, written_mask=None):
    """After a synchronize: both bands of `g` still hold the pattern; with
    `written_mask` (True = the contract allows a write; one entry per byte or
    per element of the view) every other byte of the view does too. Raises
    AssertionError naming the first offending byte offsets relative to the
    view (negative: before it; >= nbytes: past it) and the bytes found."""
    now = g._bytes()
    pat = g.pattern
    s, e = g.start, g.start + g.nbytes
    problems = []
    bad = np.nonzero(now[:s] != pat[:s])[0]
    if bad.size:
        problems.append(f"{bad.size} byte(s) written BEFORE the view at " +
                        _describe(bad[::-1], now, pat, s))
    bad = np.nonzero(now[e:] != pat[e:])[0] + e
    if bad.size:
        problems.append(f"{bad.size} byte(s) written PAST the view ({g.nbytes} bytes) at " +
                        _describe(bad, now, pat, s))
    if written_mask is not None:
        m = np.asarray(written_mask, dtype=bool).ravel()
        if m.size * g.dtype.itemsize == g.nbytes and m.size != g.nbytes:
            m = np.repeat(m, g.dtype.itemsize)
        assert m.size == g.nbytes, (m.size, g.nbytes)
        bad = np.nonzero((now[s:e] != pat[s:e]) & ~m)[0] + s
        if bad.size:
            problems.append(f"{bad.size} byte(s) written INSIDE the view where the contract "
                            "forbids it at " + _describe(bad, now, pat, s))
    if problems:
        raise AssertionError("write confinement broken: " + "; ".join(problems))


class ReadOnly:
    """An input registered as read-only: a snapshot taken now, compared byte
    for byte by check_unchanged()."""

    def __init__(self, arr, name="input"):
        self.arr, self.name = arr, name
        self.snapshot = self._bytes().copy()

    def _bytes(self):
        a = self.arr
        if isinstance(a, np.ndarray):
            return np.ascontiguousarray(a).view(np.uint8).ravel()
        import torch
        if a.is_cuda:
            torch.cuda.synchronize()
        return a.contiguous().view(torch.uint8).cpu().numpy().ravel()


def check_unchanged(r):
    now = r._bytes()
    bad = np.nonzero(now != r.snapshot)[0]
    if bad.size:
        raise AssertionError(
            f"read-only {r.name} was modified: {bad.size} byte(s), first at " +
            ", ".join(f"+{int(i)}: 0x{int(r.snapshot[i]):02x} -> 0x{int(now[i]):02x}"
                      for i in bad[:8]))


class Registry:
    """The guarded outputs and read-only inputs of one test, checked
    together."""

    def __init__(self, device=None):
        self.device, self.inputs = device, []

    def out(self, nbytes_or_shape, dtype=np.uint8, **kw):
        kw.setdefault("device", self.device)
        return guarded(nbytes_or_shape, dtype, **kw)

    def ro(self, arr, name="input"):
        self.inputs.append(ReadOnly(arr, name))
        return arr

    def check_inputs(self):
        for r in self.inputs:
            check_unchanged(r)
