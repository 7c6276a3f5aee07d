"""The guard-band helper itself (tests/guard_util.py), on the CPU: a guard
that cannot fail is worth nothing, so every kind of stray write a kernel
could make is simulated here with numpy and CPU torch and must be flagged;
a correct write must pass. No GPU involved."""
import numpy as np
import pytest

import guard_util
from guard_util import check, check_unchanged, guarded

torch = pytest.importorskip("torch")

BACKENDS = [None, "cpu"]          # numpy host arrays, torch tensors


def raw(g):
    """The backing bytes of `g`, writable (the simulated kernel's memory)."""
    return g.backing if g.device is None else g.backing.numpy()


def store(g, elem, value):
    """Simulated kernel store of element `elem` (may be outside the view)."""
    b = np.array([value], dtype=g.dtype).view(np.uint8)
    at = g.start + elem * g.dtype.itemsize
    raw(g)[at:at + b.size] = b


# the placements the confinement tests rely on
PLACEMENTS = [(np.uint16, 4, 2), (np.uint16, 16, 14), (np.uint8, 2, 1), (np.uint8, 16, 15),
              (np.uint32, 16, 4), (np.uint8, 16, 0), (np.uint32, 16, 0)]


@pytest.mark.parametrize("device", BACKENDS)
@pytest.mark.parametrize("dtype,align,skew", PLACEMENTS)
def test_placement_and_bands(device, dtype, align, skew):
    for n in (1, 5, 4099):
        g = guarded((n,), dtype, align=align, skew=skew, device=device)
        assert g.ptr % align == skew
        assert g.nbytes == n * np.dtype(dtype).itemsize
        total = len(g.pattern)
        assert g.start >= guard_util.MIN_BAND and total - g.start - g.nbytes >= guard_util.MIN_BAND
        assert g.start >= 64 * np.dtype(dtype).itemsize
        # view included, everything holds the pattern, and no forbidden byte
        np.testing.assert_array_equal(g._bytes(), g.pattern)
        assert not np.isin(g.pattern, guard_util.AVOID).any()
        check(g, np.zeros(n, bool))
    # slot outputs: two whole slots on each side, the header's alignment kept
    g = guarded(3 * 9216, np.uint8, align=16, skew=0, slot=9216, device=device)
    assert g.ptr % 16 == 0 and g.start >= 2 * 9216
    assert len(g.pattern) - g.start - g.nbytes >= 2 * 9216


def test_pattern_is_position_dependent_and_seeded():
    a, b = guard_util.pattern(8192, 1), guard_util.pattern(8192, 2)
    assert len(np.unique(a)) > 200 and not np.array_equal(a, b)
    assert not np.array_equal(a[:4096], a[4096:])
    np.testing.assert_array_equal(a, guard_util.pattern(8192, 1))
    g1, g2 = guarded(64), guarded(64)
    assert not np.array_equal(g1.pattern, g2.pattern)     # a fresh pattern per buffer


@pytest.mark.parametrize("device", BACKENDS)
@pytest.mark.parametrize("dtype,align,skew", PLACEMENTS[:5])
def test_correct_write_passes(device, dtype, align, skew):
    n = 37
    g = guarded((n,), dtype, align=align, skew=skew, device=device)
    for i in range(n):
        store(g, i, i * 3 + 1)
    check(g)
    check(g, np.ones(n, bool))
    np.testing.assert_array_equal(g.host(), (np.arange(n) * 3 + 1).astype(dtype))
    # all but the last element written, as the mask says
    g = guarded((n,), dtype, align=align, skew=skew, device=device)
    for i in range(n - 1):
        store(g, i, 7)
    m = np.ones(n, bool)
    m[-1] = False
    check(g, m)
    assert g.host()[-1] == g.view_pattern()[-1]


@pytest.mark.parametrize("device", BACKENDS)
@pytest.mark.parametrize("dtype,align,skew", PLACEMENTS[:5])
@pytest.mark.parametrize("value", [0, 0xFF, 0xA5, 0xAB, 0xFFFF, 0xA5A5, 0xABAB, 0x1234])
def test_one_element_past_the_end_and_before_the_start(device, dtype, align, skew, value):
    """Whatever the value, the old constant poisons 0xA5 / 0xAB included."""
    n = 5
    value &= (1 << 8 * np.dtype(dtype).itemsize) - 1
    for elem, word in ((n, "PAST"), (-1, "BEFORE"), (n + 40, "PAST"), (-64, "BEFORE")):
        # (a fixed seed: the pattern under test is the same in every run)
        g = guarded((n,), dtype, align=align, skew=skew, device=device, seed=7000 + elem)
        for i in range(n):
            store(g, i, 1)
        store(g, elem, value)
        with pytest.raises(AssertionError, match=word) as ei:
            check(g)
        off = elem * np.dtype(dtype).itemsize
        assert f"{off:+d}: found 0x{value & 0xFF:02x}" in str(ei.value)


@pytest.mark.parametrize("device", BACKENDS)
@pytest.mark.parametrize("value", [0, 0xFFFF, 0xA5A5, 0xABAB, 0x0102])
def test_write_inside_the_view_where_the_mask_forbids_it(device, value):
    n = 9
    g = guarded((n,), np.uint16, align=16, skew=14, device=device, seed=7100)
    m = np.ones(n, bool)
    m[4] = False
    for i in range(n):
        store(g, i, value)
    check(g)                                   # the bands are intact ...
    with pytest.raises(AssertionError, match="INSIDE") as ei:
        check(g, m)                            # ... but element 4 was not to be written
    assert "+8: found" in str(ei.value) and "+9: found" in str(ei.value)
    # a byte mask names single bytes (slot tails)
    g = guarded(64, np.uint8, device=device)
    bm = np.zeros(64, bool)
    bm[:20] = True
    raw(g)[g.start:g.start + 32] = 0           # "zeros up to the next 16-byte boundary" ...
    with pytest.raises(AssertionError, match=r"\+20: found 0x00"):
        check(g, bm)                           # ... where only 20 bytes were allowed
    bm[:32] = True
    check(g, bm)


def test_paired_and_rounded_stores_are_caught_at_odd_n():
    """The kernel shapes the placements are for: two 16-bit results paired
    into one dword store, and a store rounded up to 16 bytes."""
    n = 5
    g = guarded((n,), np.uint16, align=4, skew=2)          # out ≡ 2 (mod 4)
    b = raw(g)
    for i in range(0, n, 2):                               # dword store of (i, i + 1)
        b[g.start + 2 * i:g.start + 2 * i + 4] = 0
    with pytest.raises(AssertionError, match=r"PAST.*\+10: found 0x00"):
        check(g)
    g = guarded((n,), np.uint16, align=16, skew=14)
    b = raw(g)
    lo = g.start - 14                                      # the enclosing 16-byte lines
    b[lo:lo + 32] = 0xFF
    with pytest.raises(AssertionError, match="BEFORE.*PAST"):
        check(g)


@pytest.mark.parametrize("device", BACKENDS)
def test_fill_and_readonly_inputs(device):
    g = guarded(100, np.uint8, skew=3, device=device)
    data = np.arange(100, dtype=np.uint8)
    g.fill(data)
    np.testing.assert_array_equal(g.host(), data)
    check(g)
    arr = np.arange(1000, dtype=np.uint32)
    if device is not None:
        arr = torch.from_numpy(arr.view(np.int32))
    r = guard_util.ReadOnly(arr, "lengths")
    check_unchanged(r)
    arr[777] ^= 0x100
    with pytest.raises(AssertionError, match=r"read-only lengths was modified.*\+3109"):
        check_unchanged(r)
    reg = guard_util.Registry(device)
    a = reg.ro(np.zeros(8, np.uint8) if device is None else torch.zeros(8, dtype=torch.uint8))
    reg.check_inputs()
    a[3] = 1
    with pytest.raises(AssertionError, match="modified"):
        reg.check_inputs()
