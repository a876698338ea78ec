"""The Woodbury correction of the cycle chains computes what it computed before its four
builders, nine kernels and four apply sites became one build, one apply and one kernel set
(DESIGN.md section 3d): the arithmetic and its order are the same, so is every result, bit
for bit.

``cyc_unify_cases.py`` lists the cases (one rank with the CSR's couplings, m > 256, the (k, 0)
route's auxiliary handle, in-process groups, the batch); ``golden/cyc_unify_parent.npz`` holds
the parent commit's solutions, reported residuals, pass counts and launch counts of each,
recorded on an MI355X. Expected difference: 0 bits, in every array of every case.

And a build that fails leaves the handle able to build again: its unit solves run the tree
solve alone, and that state must not outlive the build."""

from __future__ import annotations

import functools
from pathlib import Path

import numpy as np
import pytest

import cyc_unify_cases as CC
from cases import CYCLIC, p_y
from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh, _lib
from oracle import nx_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
SOL_TOL = 1e-10  # the direct solve's bar (tests/test_gpu_direct.py)


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN / "cyc_unify_parent.npz") as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("case", CC.CASES)
def test_bit_equal_to_the_parent_build(case):
    gold = {k[len(case) + 1:]: v for k, v in _golden().items() if k.startswith(case + "/")}
    assert gold, case
    got = CC.run_case(case)
    assert sorted(got) == sorted(gold)
    bad = []
    for k in sorted(gold):
        a, b = np.asarray(got[k]), gold[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        same = a.tobytes() == b.tobytes()
        if not same:
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            bad.append((k, int(np.count_nonzero(d)), float(np.max(d))))
        print(f"{case} {k}: shape {a.shape} bit-equal={same}")
    assert not bad, bad


def _set_cycles(h, rows):
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    h._pc_keep_y = rows
    _lib.check(_lib.lib().nx_set_cycles(h.ptr, int(rows.shape[0]), _lib._ptr(rows, _lib.C.c_int32)))


def test_a_failed_build_is_built_again():
    """A table that pairs a cycle chain's flux end with a multiplier row it has no entry
    with: the coupling read from the CSR is 0 and the build fails (``cyc_invert``: no coupling
    at its grounded end) after its unit solves ran. With the decomposition's table back the
    next solve builds the correction and meets the oracle -- nothing of the failed build (its
    tree-solve-alone state least of all) is left on the handle."""
    make, N = CYCLIC["lattice4x5_N6"]
    mesh = NetworkMesh(make(), N=N)
    asm = HydraulicNetworkAssembler(mesh)
    asm.compute_forms(p_bc_ex=p_y)
    asm.set_direct(True)
    h = asm.handle
    good = np.array(asm.tree_preconditioner.cyc_rows, dtype=np.int32).reshape(-1, 2)
    asm.assemble()
    rp, col, _ = h.csr()
    q = int(good[0, 0])
    taken = set(col[rp[q]:rp[q + 1]].tolist()) | set(good[:, 1].tolist())
    lam = next(r for r in range(asm.local_problem.n_edge_dofs, h.n_rows) if r not in taken)
    bad = good.copy()
    bad[0, 1] = lam
    _set_cycles(h, bad)
    asm.assemble()
    with pytest.raises(_lib.NxError, match="no coupling at its grounded end"):
        h.solve(1e-12, 100, 4)
    _set_cycles(h, good)
    asm.assemble()
    it, rr, conv = h.solve(1e-12, 100, 4)
    assert h.solver() == (1, 1) and conv and it in (1, 2) and rr <= 1e-12, (h.solver(), it, rr)
    src, dst = mesh.edges
    P = O.build_problem(mesh.node_coordinates, src, dst, N, mesh.edge_colors)
    A, b = O.assemble_reference(P, p_y)
    _, _, perm, _ = O.to_build_layout(P, A, b)
    x_ref = O.solve_reference(A, b)[perm]
    assert np.linalg.norm(h.solution() - x_ref) / np.linalg.norm(x_ref) <= SOL_TOL
    asm.close()
