"""pack16 of the MSD hybrid: the last digit pass of a
full-width keys-only sort writes only the low 16 bits of every key (the bucket
index restates the high 16), and the bucket kernels, both fallback lists and
the host-level LSD fallback read that u16 array.  Forced hybrid, both digit
widths, against the oracle's sort.  The timing registry's "pack16" entry
(recorded beside the packed last pass, no launch of its own) says that the
mode ran, "pack16expand" that the host-level fallback rebuilt whole keys.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pylibsort
    import pylibsort.device as D
    assert pylibsort.gpu_ready(), pylibsort.last_error()
    return D


@pytest.fixture(params=[4, 8], ids=["digit4", "digit8"])
def bits(request, dev):
    import pylibsort
    prev = pylibsort.setDigitBits(request.param)
    yield request.param
    pylibsort.setDigitBits(prev)


@pytest.fixture(autouse=True)
def force(dev):
    import pylibsort
    prev = pylibsort.setHybrid("force")
    yield
    pylibsort.setHybrid(prev)


@pytest.fixture
def knob_on(monkeypatch):
    monkeypatch.setenv("LIBSORT_HYB_PACK16", "1")
    monkeypatch.delenv("LIBSORT_HYB_RESERVE", raising=False)


def _u32(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _tensor(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _run(dev, fn):
    """fn() with the registry on: its output and the launch counts of
    (pack16, pack16expand, bucketsort, tilepass)."""
    dev.timing_enable(True)
    dev.timing_reset()
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, tuple(dev.timing_query(k)[0] for k in ("pack16", "pack16expand", "bucketsort", "tilepass"))
    finally:
        dev.timing_enable(False)


def _check(dev, oracle_mod, x, **kw):
    out, counts = _run(dev, lambda: dev.sort_keys_u32(_tensor(x), **kw))
    np.testing.assert_array_equal(_u32(out), oracle_mod.sort_u32(x))
    return counts


SIZES = [1024, 1025, 4097, 65539, (1 << 20) + 3]


@pytest.mark.parametrize("n", SIZES)
def test_ragged_sizes(dev, oracle_mod, bits, knob_on, n):
    """65539 keys: ~1 per bucket, so every start parity meets lengths 0-3
    (2-byte stores only, dword loads of one or two elements); 1025: nearly
    every bucket empty."""
    p16, exp, nbs, npass = _check(dev, oracle_mod, oracle_mod.pcg(n, first=7 * n + bits))
    assert (p16, exp, nbs, npass) == (1, 0, 1, 16 // bits)


@functools.lru_cache(maxsize=1)
def _edge_base():
    """2^22 uniform keys with bucket B emptied (its keys moved one bucket up)
    and the positions, in random order, of the keys above bucket B + 1."""
    import oracle.oracle as o
    n = 1 << 22
    x = o.pcg(n, first=2222)
    b = np.uint32(EDGE_BUCKET)
    x[(x >> 16) == b] += np.uint32(1 << 16)
    rng = np.random.default_rng(22)
    pool = rng.permutation(np.nonzero((x >> 16) > b + 1)[0])
    return x, pool


EDGE_BUCKET = 0x5A31
EDGE_CAP1 = 2304  # 256 x 9: the first block's slots at 2^22 keys (mean bucket 64 + 3.5 sigma <= 256 x 9)


@pytest.mark.parametrize("parity", [0, 1], ids=["even_start", "odd_start"])
@pytest.mark.parametrize("extra", [-1, 0, 1], ids=["cap1-1", "cap1", "cap1+1"])
def test_block_capacity_edge(dev, oracle_mod, bits, knob_on, extra, parity):
    """One bucket of exactly cap1 - 1, cap1, cap1 + 1 keys, starting at an even
    and at an odd element (an odd start takes one slot more than the bucket's
    length: 2304 slots of keys, 5 dwords x 256 x 2 = 2560 loaded).  The first
    two fit the first launch's block, the third is listed for the 3-bit retry
    at the second size; which launch placed a bucket is not in the registry, so
    the result and the absence of any LSD fallback are what is asserted."""
    base, pool = _edge_base()
    x = base.copy()
    length = EDGE_CAP1 + extra
    rng = np.random.default_rng(100 + extra)
    b = np.uint32(EDGE_BUCKET)
    x[pool[:length]] = (b << 16) | rng.integers(0, 1 << 16, length).astype(np.uint32)
    if int(np.count_nonzero((x >> 16) < b)) % 2 != parity:
        x[pool[length]] &= np.uint32(0xFFFF)  # one key from above the bucket to below it
    assert int(np.count_nonzero((x >> 16) == b)) == length
    assert int(np.count_nonzero((x >> 16) < b)) % 2 == parity
    p16, exp, nbs, npass = _check(dev, oracle_mod, x)
    assert (p16, exp, nbs, npass) == (1, 0, 1, 16 // bits)


def _kind(kind, n, seed, bits):
    import oracle.oracle as o
    x = o.pcg(n, first=seed)
    if kind == "low16_const":  # every bucket all-equal keys: the LSD-step list takes them all
        return x & np.uint32(0xFFFF0000)
    if kind == "four":
        rng = np.random.default_rng(seed)
        return rng.integers(0, 4, n, dtype=np.uint64).astype(np.uint32) * np.uint32(0x40000001)
    if kind == "equal":
        return np.full(n, 0x9E3779B9, dtype=np.uint32)
    if kind == "deep_skew":
        # the top digit uniform, the prefix's other bits zero: RADIX buckets of
        # n / RADIX keys, over every block (test_gpu_hybrid's deep_skew is the
        # 4-bit form; at 8-bit digits that one has 16 of 256 top digits and is
        # abandoned at depth 0, before any last pass)
        return x & np.uint32(0xF000FFFF if bits == 4 else 0xFF00FFFF)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["low16_const", "four", "equal"])
def test_count_overflow_kinds(dev, oracle_mod, bits, knob_on, kind):
    """Duplicate-heavy buckets: the 2-bit and 3-bit counts wrap and the
    LSD-step list reads the packed input.  `four` and `equal` have a skewed top
    digit, which abandons the hybrid at depth 0 (no bucket sort, no last pass):
    wherever the bucket sort ran, the packed last pass ran before it."""
    x = _kind(kind, (1 << 22) + 17, 31 + bits, bits)
    p16, exp, nbs, npass = _check(dev, oracle_mod, x)
    assert exp == 0
    if kind == "low16_const":
        assert (p16, nbs, npass) == (1, 1, 16 // bits)
    else:
        assert p16 == nbs


def test_count_overflow_exact_repeats(dev, oracle_mod, bits, knob_on):
    """Uniform 2^20 keys, one value exactly 4 times (its 2-bit count wraps:
    the 3-bit retry list) and one exactly 8 times (the 3-bit count wraps too:
    the LSD-step list)."""
    n = 1 << 20
    x = oracle_mod.pcg(n, first=404 + bits).copy()
    v4, v8 = np.uint32(0x1234ABCD), np.uint32(0xC0DE0007)
    for v in (v4, v8):
        x[x == v] ^= np.uint32(1 << 20)
    x[1000:1004] = v4
    x[5000:5008] = v8
    assert int(np.count_nonzero(x == v4)) == 4 and int(np.count_nonzero(x == v8)) == 8
    p16, exp, nbs, npass = _check(dev, oracle_mod, x)
    assert (p16, exp, nbs, npass) == (1, 0, 1, 16 // bits)


def test_host_fallback_expands(dev, oracle_mod, bits, knob_on):
    """Buckets over every block: the host learns it after the packed last pass
    is queued, so whole keys are rebuilt in out (pack16expand) before the LSD
    sort of out in place."""
    x = _kind("deep_skew", (1 << 22) + 17, 53, bits)
    p16, exp, nbs, npass = _check(dev, oracle_mod, x)
    assert (p16, exp, nbs) == (1, 1, 0)
    assert npass > 16 // bits


def test_stale_buffers(dev, oracle_mod, bits, knob_on):
    """out and tmp hold 0xDEADBEEF; a 65539-key sort of other keys follows a
    2^22 + 5 one on the same workspace (whose u16 array, slices and lists are
    left over)."""
    for n, first in (((1 << 22) + 5, 11), (65539, 12345)):
        x = oracle_mod.pcg(n, first=first + bits)
        out = torch.full((n,), -559038737, dtype=torch.int32, device="cuda")  # 0xDEADBEEF
        tmp = out.clone()
        p16, exp, nbs, npass = _check(dev, oracle_mod, x, out=out, tmp=tmp)
        assert (p16, exp, nbs, npass) == (1, 0, 1, 16 // bits)


def test_off_in_place(dev, oracle_mod, bits, knob_on):
    x = oracle_mod.pcg((1 << 21) + 9, first=77)
    t = _tensor(x)
    tmp = torch.empty_like(t)
    _, (p16, exp, _, _) = _run(dev, lambda: dev.sort_keys_u32(t, out=t, tmp=tmp))
    np.testing.assert_array_equal(_u32(t), oracle_mod.sort_u32(x))
    assert (p16, exp) == (0, 0)


@pytest.mark.parametrize("reserve", ["0", "nomem", "short"])
def test_off_without_reserved_depth0(dev, oracle_mod, bits, knob_on, monkeypatch, reserve):
    """No reserved depth 0 (count pass instead), or its short-slice test mode
    (whose overflow sends the sort to the LSD passes over the untouched
    input): whole keys as before."""
    monkeypatch.setenv("LIBSORT_HYB_RESERVE", reserve)
    n = (1 << 22) + 5
    p16, exp, _, _ = _check(dev, oracle_mod, oracle_mod.pcg(n, first=n + 99))
    assert (p16, exp) == (0, 0)


def test_off_range_sort(dev, oracle_mod, bits, knob_on):
    n = (1 << 21) + 9
    lo = 0x12345678
    x = (oracle_mod.pcg(n, first=77) % np.uint32(0x5000000)) + np.uint32(lo)
    out, (p16, exp, _, _) = _run(dev, lambda: dev.sort_keys_range_u32(_tensor(x), lo, lo + 0x5000000))
    np.testing.assert_array_equal(_u32(out), oracle_mod.sort_u32(x))
    assert (p16, exp) == (0, 0)


@pytest.mark.parametrize("n", SIZES)
def test_knob_off(dev, oracle_mod, bits, monkeypatch, n):
    monkeypatch.setenv("LIBSORT_HYB_PACK16", "0")
    p16, exp, nbs, npass = _check(dev, oracle_mod, oracle_mod.pcg(n, first=7 * n + bits))
    assert (p16, exp, nbs, npass) == (0, 0, 1, 16 // bits)
