"""The prediction half of the rough search of modes 2..33 on the device (kvz_hip_dev_rough_rows: the pass's own reference filter, extended references, edge bytes of
modes 10 / 26 and the packed, table-driven row generator kvz_mfma.hpp satd_rows_predict, in the pass's lane roles) against the oracle's intra prediction, exactly:
every mode and every 8x8 block of 8x8 and 16x16 CUs -- the pass-level tests only see the modes that win -- on the reference sets of rough_rows_common.py (50 random
ones, all 0, all 255, alternating 0 / 255 that take the edge samples into both ends of their clip).  An odd number of CUs, so that a half-filled workgroup occurs."""
import numpy as np
import pytest

import rough_rows_common as rr


def _dev():
    import kvazaar_amd
    from kvazaar_amd import dev as devapi
    return devapi.Dev(kvazaar_amd.load_library())


@pytest.mark.gpu
@pytest.mark.parametrize("log2w", [3, 4])
def test_device_rows_equal_the_oracle_prediction(oracle, log2w):
    tops, lefts = rr.ref_sets(log2w)
    n = 2 * (1 << log2w) + 1
    want = rr.oracle_blocks(oracle, log2w)
    order = np.arange(1 - len(tops) % 2, len(tops))  # (an even number of sets: without the first, a random one)
    count = len(order)
    assert count % 2 == 1 and count >= 50 + 6 - 1
    dev = _dev()
    per = want[0].size
    bufs = [dev.put(tops[order, :n]), dev.put(lefts[order, :n]), dev.put(np.full(per * (count + 1), 0xA5, np.uint8))]
    try:
        assert dev.lib.kvz_hip_dev_rough_rows(log2w, bufs[0], bufs[1], count, bufs[2]) == 0
        got = dev.get(bufs[2], (count + 1,) + want.shape[1:], np.uint8)
        assert (got[count] == 0xA5).all()  # nothing written past the last CU
        bad = np.argwhere((got[:count] != want[order]).any(axis=3))
        assert bad.size == 0, bad[:8]  # (set, mode - 2, block)
        assert dev.lib.kvz_hip_dev_rough_rows(5, bufs[0], bufs[1], 1, bufs[2]) == -1 and dev.lib.kvz_hip_dev_rough_rows(log2w, bufs[0], bufs[1], -1, bufs[2]) == -1
        assert dev.lib.kvz_hip_dev_rough_rows(log2w, bufs[0], bufs[1], 0, bufs[2]) == 0
    finally:
        dev.free(*bufs)
