"""The solves compute what they computed before the segment helpers went from ``__shfl*``
(``ds_bpermute``) to DPP row moves: the data moved is the
same, so is every result, bit for bit.

``seg_shuffle_cases.py`` lists the cases (one per lane shape a small N reaches) and their paths:
the fused step (storing, then -- at N = 15 -- the values-free ``k_dir_step_kv``), the separate
launches, one MINRES solve, one batch solve of two columns. ``golden/seg_shuffle_parent.npz``
holds the parent commit's solution, rhs, CSR values and reported residuals of each, recorded on
an MI355X. Expected difference: 0 bits, in every array of every case."""

from __future__ import annotations

import functools
from pathlib import Path

import numpy as np
import pytest

import seg_shuffle_cases as SC

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN / "seg_shuffle_parent.npz") as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("N", SC.NS)
def test_bit_equal_to_the_parent_build(N):
    gold = {k[len(f"N{N}_"):]: v for k, v in _golden().items() if k.startswith(f"N{N}_")}
    got = SC.run_case(N)
    assert sorted(got) == sorted(gold)
    if N == 15:
        assert got["fused2_kept"] == 1  # (the values-free step ran)
    bad = []
    for k in sorted(gold):
        a, b = np.asarray(got[k]), gold[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        same = a.tobytes() == b.tobytes()
        if not same:
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            bad.append((k, int(np.count_nonzero(d)), float(np.max(d))))
        print(f"N={N} {k}: shape {a.shape} bit-equal={same}")
    assert not bad, bad
