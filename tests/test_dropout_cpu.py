"""Training-mode dropout of the VGG-16 head without a GPU: the numpy Philox4x32-10 mirror (tests/dropout_mirror.py) against
Random123's known-answer vectors, and the argument checks of frcnn_dropout / frcnn_dropout_relu_backward (they return before any
GPU work)."""
import ctypes as C
import math

import numpy as np
import pytest

from fasterrcnn_amd import _native as nv
from tests import dropout_mirror as DM


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    got = DM.philox4x32_10(*ctr, *key)
    assert [int(v) for v in got] == list(want)


def test_mirror_layout_and_keep_rule():
    seed, sid, rank = -0x123456789abcdef, 2, 3
    k0, k1 = DM.seed_words(seed)
    w = DM.random_words(11, seed, sid, rank)
    for g in range(3):
        words = DM.philox4x32_10(g, 0, sid, rank, k0, k1)
        for j in range(4):
            if 4 * g + j < 11:
                assert int(w[4 * g + j]) == int(words[j])
    assert DM.keep_mask(1000, 0.0, seed, sid, rank).all()
    assert not DM.keep_mask(1000, 1.0, seed, sid, rank).any()
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    assert np.array_equal(DM.keep_mask(11, 0.5, seed, sid, rank), (u < np.float32(0.5)).astype(np.uint8))
    assert DM.scale_of(0.5) == np.float32(2.0) and DM.scale_of(0.1) == np.float32(1.0 / 0.9)


def test_dropout_argument_validation_without_gpu():
    lib = nv.lib()
    buf = (C.c_float * 8)()
    seed = (C.c_uint64 * 1)()
    x, s = C.addressof(buf), C.addressof(seed)
    for p in (-0.1, 1.5, math.nan, math.inf):
        assert lib.frcnn_dropout(x, 8, p, 2.0, s, 1, 0, None, None) == -1, p
    for scale in (math.nan, math.inf, 0.5, -2.0):
        assert lib.frcnn_dropout(x, 8, 0.5, scale, s, 1, 0, None, None) == -1, scale
    assert lib.frcnn_dropout(None, 8, 0.5, 2.0, s, 1, 0, None, None) == -1
    assert lib.frcnn_dropout(x, 8, 0.5, 2.0, None, 1, 0, None, None) == -1
    assert lib.frcnn_dropout(None, 0, 0.5, 2.0, None, 1, 0, None, None) == 0          # n == 0: a no-op
    assert lib.frcnn_dropout(x, 8, 1.5, 2.0, s, 1, 0, None, None) == -1                # checked before n / pointers
    for scale in (math.nan, 0.5, 0.0):
        assert lib.frcnn_dropout_relu_backward(x, x, 8, scale, None) == -1, scale
    assert lib.frcnn_dropout_relu_backward(None, x, 8, 2.0, None) == -1
    assert lib.frcnn_dropout_relu_backward(x, None, 8, 2.0, None) == -1
    assert lib.frcnn_dropout_relu_backward(None, None, 0, 2.0, None) == 0
