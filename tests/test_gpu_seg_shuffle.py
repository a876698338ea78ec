"""The kernels' segment cross-lane helpers (``seg_up`` / ``seg_down`` / ``seg_xor``, their
``_nc`` variants, ``seg_bcast0``, ``seg_incl_scan``, ``seg_sum``, ``wave_sum``; DESIGN.md section
3c, round 9) move by DPP row operations exactly what the ``__shfl_*`` calls they replace move.

``nx_test_seg_shuffle`` runs, in one launch of one 1024-thread workgroup, every helper for
W = 4, 8, 16 and every power-of-two offset below W once by the helper and once by the plain
shuffle, on the same input: one double (and one int) per lane, all distinct, high and low
words both varying, with -0.0, a denormal, an infinity and a NaN with a payload among them.
The outputs are compared as integers, with no tolerance -- these are data moves: the checked
helpers on every lane, the ``_nc`` ones on the lanes their contract defines (the source lane
inside the segment)."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from networks_fenicsx_amd import _lib

pytestmark = pytest.mark.gpu

LANES = 1024
KINDS = ("up", "down", "xor", "up_nc", "down_nc")


def _slots():
    """(name, W, O) per output slot, in the order include/nxhip.h gives."""
    out = []
    for W in (4, 8, 16):
        O = 1
        while O < W:
            out += [(k, W, O) for k in KINDS]
            O *= 2
        out += [("bcast0", W, 0), ("scan", W, 0), ("sum", W, 0)]
    return out + [("wave_sum", 64, 0)]


def _inputs():
    rng = np.random.default_rng(20240917)
    bits = np.unique(rng.integers(0, 2**63, size=2 * LANES, dtype=np.uint64))[:LANES].copy()
    rng.shuffle(bits)
    # moderate exponents (2^-64 .. 2^63: the sums stay finite), random sign, random 52-bit mantissa
    mant = bits & np.uint64((1 << 52) - 1)
    expo = (np.uint64(1023 - 64) + (bits >> np.uint64(52)) % np.uint64(128)) << np.uint64(52)
    sign = (bits >> np.uint64(62)) << np.uint64(63)
    d = (sign | expo | mant).view(np.float64)
    special = np.array([0x8000000000000000,    # -0.0
                        0x0000000000abcdef,    # a denormal
                        0x7ff0000000000000,    # +inf
                        0x7ff8dead0000beef],   # a quiet NaN with a payload
                       dtype=np.uint64).view(np.float64)
    d[[5, 130, 517, 1001]] = special
    assert np.unique(d.view(np.uint64)).size == LANES
    hi, lo = d.view(np.uint64) >> np.uint64(32), d.view(np.uint64) & np.uint64(0xffffffff)
    assert np.unique(hi).size > LANES // 2 and np.unique(lo).size > LANES // 2
    i = rng.permutation(np.arange(LANES, dtype=np.int64) * 2097143 - 2**30).astype(np.int32)
    assert np.unique(i).size == LANES
    return np.ascontiguousarray(d), np.ascontiguousarray(i)


@pytest.fixture(scope="module")
def outputs():
    d, i = _inputs()
    cap = 64
    new_d, ref_d = np.zeros((cap, LANES)), np.ones((cap, LANES))
    new_i, ref_i = np.zeros((cap, LANES), np.int32), np.ones((cap, LANES), np.int32)
    n = C.c_int32(0)
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    _lib.check(_lib.lib().nx_test_seg_shuffle(
        d.ctypes.data_as(pd), i.ctypes.data_as(pi), cap, new_d.ctypes.data_as(pd),
        ref_d.ctypes.data_as(pd), new_i.ctypes.data_as(pi), ref_i.ctypes.data_as(pi), C.byref(n)))
    slots = _slots()
    assert n.value == len(slots)
    return d, i, slots, new_d.view(np.uint64), ref_d.view(np.uint64), new_i, ref_i


def _defined(kind, W, O):
    """Lanes on which the helper's contract defines the result."""
    l = np.arange(LANES) % W
    if kind == "up_nc":
        return l >= O
    if kind == "down_nc":
        return l + O < W
    return np.ones(LANES, bool)


def _host_move(v, kind, W, O):
    """What ``__shfl_*(v, O, W)`` returns, on the host (own value outside the segment)."""
    lane = np.arange(LANES)
    l = lane % W
    if kind in ("up", "up_nc"):
        src = np.where(l >= O, lane - O, lane)
    elif kind in ("down", "down_nc"):
        src = np.where(l + O < W, lane + O, lane)
    elif kind == "xor":
        src = lane ^ O
    else:
        src = lane - l
    return v[src]


def test_double_moves_and_sums_are_the_shuffles_bits(outputs):
    d, _, slots, new, ref, _, _ = outputs
    for s, (kind, W, O) in enumerate(slots):
        m = _defined(kind, W, O)
        bad = np.flatnonzero(m & (new[s] != ref[s]))
        assert bad.size == 0, (kind, W, O, bad[:8], new[s][bad[:8]], ref[s][bad[:8]])
        if kind in KINDS or kind == "bcast0":  # the shuffle itself moved what it should
            np.testing.assert_array_equal(ref[s][m], _host_move(d.view(np.uint64), kind, W, O)[m])


def test_int_moves_are_the_shuffles_bits(outputs):
    _, i, slots, _, _, new, ref = outputs
    for s, (kind, W, O) in enumerate(slots):
        if kind in ("scan", "sum", "wave_sum"):
            assert not new[s].any() and not ref[s].any()
            continue
        m = _defined(kind, W, O)
        bad = np.flatnonzero(m & (new[s] != ref[s]))
        assert bad.size == 0, (kind, W, O, bad[:8], new[s][bad[:8]], ref[s][bad[:8]])
        np.testing.assert_array_equal(ref[s][m], _host_move(i, kind, W, O)[m])
