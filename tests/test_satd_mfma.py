"""The Hadamard half of the rough search on the matrix cores (kvz_mfma.hpp satd8_group_mfma, through kvz_hip_dev_satd8_blocks: the text the CTU pass calls, 32 pairs of
8x8 byte blocks per wavefront) against sum |H8 (P - O) H8| in numpy, exactly.  The block pairs are the ones that each catch one way the product can go wrong:
P = O (the bias and the -128 of both operands must cancel: 0), the largest coefficient (255 against 0: 16320), the 64 two-dimensional Walsh patterns and their
negatives (a (lane half, byte) slot that means one sample to the matrix and another to the samples spreads a one-coefficient spectrum and changes the sum),
asymmetric random blocks (P and O drawn separately, no transposition symmetry) and 0 / 255 noise (the largest totals).  The pool goes through in calls of 32 blocks
(one group), 96, and 77 (no multiple of 32: a group with dead columns), with guard words behind the sums."""
import numpy as np
import pytest

H2 = np.array([[1, 1], [1, -1]], dtype=np.int64)
H8 = np.kron(np.kron(H2, H2), H2)
GUARD = 0xDEADBEEF


def _pool():
    rng = np.random.default_rng(20240)
    p, o = [], []
    same = rng.integers(0, 256, (16, 8, 8))
    p += list(same); o += list(same)  # noqa: E702
    full, zero = np.full((8, 8), 255), np.zeros((8, 8), dtype=np.int64)
    p += [full, zero]; o += [zero, full]  # noqa: E702
    for u in range(8):
        for v in range(8):
            pat = np.outer(H8[u], H8[v])
            plus, minus = np.where(pat > 0, 255, 0), np.where(pat < 0, 255, 0)
            p += [plus, minus]; o += [minus, plus]  # noqa: E702
    p += list(rng.integers(0, 256, (48, 8, 8))); o += list(rng.integers(0, 256, (48, 8, 8)))  # noqa: E702
    p += list(rng.integers(0, 2, (24, 8, 8)) * 255); o += list(rng.integers(0, 2, (24, 8, 8)) * 255)  # noqa: E702
    p += [np.arange(64).reshape(8, 8) * 4, np.arange(64).reshape(8, 8)[::-1] * 3]; o += [np.arange(64).reshape(8, 8).T * 2, np.full((8, 8), 7)]  # noqa: E702
    return np.array(p, dtype=np.uint8), np.array(o, dtype=np.uint8)


def _want(p, o):
    d = p.astype(np.int64) - o.astype(np.int64)
    return np.abs(H8 @ d @ H8).sum(axis=(1, 2)).astype(np.uint32)


def test_pool_holds_the_cases():
    p, o = _pool()
    want = _want(p, o)
    assert len(p) == 16 + 2 + 128 + 48 + 24 + 2 and len(p) % 32 != 0
    assert not want[:16].any() and list(want[16:18]) == [64 * 255] * 2  # one coefficient of 64 x 255 = 16320 ...
    assert all(int(w) == 64 * 255 for w in want[18:146])                  # ... as for every Walsh pattern, whose spectrum is one coefficient too
    assert any(not np.array_equal(a, a.T) for a in p[146:194]) and want[194:218].max() > want[146:194].max()
    assert np.array_equal(_want(o, p), want)  # magnitudes: the sign of the difference does not show


@pytest.fixture(scope="module")
def dev():
    import kvazaar_amd
    from kvazaar_amd import dev as devapi
    return devapi.Dev(kvazaar_amd.load_library())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [32, 96, 77])
def test_device_group_sums_equal_numpy(dev, n):
    p, o = _pool()
    want = _want(p, o)
    dp, do = dev.empty(n * 64), dev.empty(n * 64)
    dout = dev.put(np.full(n + 8, GUARD, dtype=np.uint32))
    try:
        for at in range(0, len(p), n):
            k = min(n, len(p) - at)
            dev.copy_in(dp, p[at:at + k])
            dev.copy_in(do, o[at:at + k])
            dev.copy_in(dout, np.full(n + 8, GUARD, dtype=np.uint32))
            assert dev.lib.kvz_hip_dev_satd8_blocks(dp, do, k, dout) == 0
            dev.lib.kvz_hip_dev_sync()
            got = dev.get(dout, (n + 8,), np.uint32)
            bad = np.nonzero(got[:k] != want[at:at + k])[0]
            assert not len(bad), (n, at, [(int(at + i), int(got[i]), int(want[at + i])) for i in bad[:8]])
            assert (got[k:] == GUARD).all(), (n, at, k)
        assert dev.lib.kvz_hip_dev_satd8_blocks(dp, do, 0, dout) == 0 and dev.lib.kvz_hip_dev_satd8_blocks(dp, do, -1, dout) == -1
    finally:
        dev.free(dp, do, dout)
