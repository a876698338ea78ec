"""CPU model of the per-scenario cycle correction of the ensemble calls
(``nx_set_ensemble_cycles``; csrc/nxhip.hip ``k_e_cyc_*``), in the solve-again form

    K_j = C^{-1} + U^T A_g(R_j)^{-1} U,  x_g = A_g(R_j)^{-1} b,
    w = K_j^{-1} U^T x_g,                x = A_g(R_j)^{-1} (b - U w)

per row of ``tests/test_gpu_ensemble.py``'s ``ensemble_R`` (0 the resident R, 3 and 9 +-1 decade
per edge, 10 +-2 decades), against SuperLU of ``A(R_j)``. The 342-chain lattice is the GPU
tests': its dense model takes minutes. Three checks per graph and row, none of them refined
unless it says so:

1. *The form*, with an exact tree solve (SuperLU of ``A_g(R_j)``) standing in: one pass, held to
   1e-12, the bar ``test_cycle_rows_and_woodbury`` holds the ``Z w`` form to. Measured worst:
   see FORM_MEASURED.
2. *The form through the device's tree solve* (``tests/test_precond.py``'s ``direct_model``): one
   pass, held to the project's 1e-10 (SOL_TOL) and to FORM_FACTOR x the error of the handle's
   ``x_g - Z w`` form on the same right-hand side through the same tree solve. This Python tree
   solve's own error against SuperLU of ``A_g`` is 2e-14 to 6e-13, and K amplifies it: first
   pass, rows 0 / 3 / 9 / 10: edge_info_N10 2.5e-13 / 9.5e-14 / 5.3e-13 / 1.3e-12, lattice4x5_N6
   1.1e-13 / 6.2e-13 / 3.3e-13 / 5.3e-11 (cond(K) = 1.4e4), lattice6x6_N3 9.1e-14 / 6.2e-14 /
   5.0e-14 / 4.0e-13 -- above 1e-12 on two rows, and the ``Z w`` form's figures are the same
   (ratios 0.93 to 1.03), so that is the tree-solve model's error, not the form's.
3. *The device's per-column policy* (``batch_solve_cols``) on top of 2: true residual, one
   refinement pass through the same route where it is above the solver's default rtol = 1e-12;
   held to 1e-12.

It also checks that K_j is symmetric and that the couplings the cycle rows drop are the same
+-1 entries for every R. ``cyc_rows`` themselves come from the decomposition, which is built from
the graph alone and never sees R, so there is nothing to compare across R."""

from __future__ import annotations

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from cases import CYCLIC
from networks_fenicsx_amd import NetworkMesh
from networks_fenicsx_amd.layout import build_local_problem
from networks_fenicsx_amd.precond import build_tree_preconditioner, lumped_mass
from oracle import nx_oracle as O
from test_precond import direct_model

BAR = 1e-12
SOL_TOL = 1e-10  # the project's bar (tests/test_gpu_direct.py)
RTOL = 1e-12  # the solver's default ksp_rtol: a column above it takes the refinement pass
FORM_MEASURED = 2.6e-14  # check 1, worst over the cases (lattice4x5_N6 row 10; else <= 3.7e-15)
# check 2: both forms apply the same w (same K, same x_g) and differ by one more tree solve's
# rounding, small beside the error K puts into w: a factor of 2 between them is generous
# (measured ratios 0.93 to 1.03)
FORM_FACTOR = 2.0
ROWS_OF_R = (0, 3, 9, 10)


def ensemble_R(E):
    """tests/test_gpu_ensemble.py's rows (that module needs a GPU build to import)."""
    rng = np.random.default_rng(2024)
    R = np.empty((11, E))
    R[0] = 0.5 + (np.arange(E) % 3) / 2.0
    R[1] = 1.0
    R[2] = 3.7
    R[3:10] = 10.0 ** rng.uniform(-1.0, 1.0, size=(7, E))
    R[10] = 10.0 ** rng.uniform(-2.0, 2.0, size=E)
    return R


def capacitance(tree, rows, a, n):
    """Z = A_g^{-1} U through ``tree`` and K = C^{-1} + U^T Z."""
    eye = np.eye(n)
    Z = np.stack([tree(eye[r]) for r in rows], axis=1)
    K = Z[rows].copy()
    asym = np.abs(K - K.T).max() / np.abs(K).max()
    for i in range(a.size):
        K[2 * i, 2 * i + 1] += 1.0 / a[i]
        K[2 * i + 1, 2 * i] += 1.0 / a[i]
    return Z, K, asym


def solve_again(tree, K, rows, rhs):
    xg = tree(rhs)
    w = np.linalg.solve(K, xg[rows])
    b2 = rhs.copy()
    b2[rows] -= w
    return tree(b2)


@pytest.mark.parametrize("case", ["edge_info_N10", "lattice4x5_N6", "lattice6x6_N3"])
def test_solve_again_correction_per_R(case):
    make, N = CYCLIC[case]
    m = NetworkMesh(make(), N=N)
    src, dst = m.edges
    P = O.build_problem(m.node_coordinates, src, dst, N, m.edge_colors)
    lp = build_local_problem(m.node_coordinates, src, dst, m.degrees, N)
    # (built from the graph alone: it cannot differ between the rows of R)
    pc = build_tree_preconditioner(lp, src, dst, m.degrees, target_jobs=16)
    k = m.num_edges - m.num_nodes + 1
    assert not pc.tree_exact and pc.cyc_rows.shape == (k, 2)
    q, lam = pc.cyc_rows[:, 0].astype(np.int64), pc.cyc_rows[:, 1].astype(np.int64)
    rows = pc.cyc_rows.reshape(-1).astype(np.int64)
    mm = rows.size
    R = ensemble_R(m.num_edges)
    rng = np.random.default_rng(11)
    a0 = None
    for j in ROWS_OF_R:
        A, b = O.assemble_reference(P, lambda x: x[1], R=R[j])
        Ab, _, _, _ = O.to_build_layout(P, A, b)
        Ad = Ab.toarray()
        a = Ad[q, lam]
        assert np.all(np.abs(a) == 1.0) and np.array_equal(a, Ad[lam, q])
        if a0 is None:
            a0 = a
        np.testing.assert_array_equal(a, a0)  # the same couplings for every R
        Ag = Ad.copy()
        Ag[q, lam] = 0.0
        Ag[lam, q] = 0.0
        Ags = sp.csr_matrix(Ag)
        dq = lumped_mass(Ab, lp)
        n = Ab.shape[0]
        bvec = rng.standard_normal(n)
        x_ref = spla.splu(Ab.tocsc()).solve(bvec)

        def err_of(x):
            return float(np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref))

        # 1: the form, exact tree solve, one pass
        lu_g = spla.splu(Ags.tocsc())
        _, K_lu, asym_lu = capacitance(lu_g.solve, rows, a, n)
        form = err_of(solve_again(lu_g.solve, K_lu, rows, bvec))
        # 2: the form through the device's tree solve, one pass, beside the Z w form
        def tree(rhs):
            return direct_model(pc, lp, dq, Ags, rhs)

        Z, K, asym = capacitance(tree, rows, a, n)
        x = solve_again(tree, K, rows, bvec)
        first = err_of(x)
        xg = tree(bvec)
        zw = err_of(xg - Z @ np.linalg.solve(K, xg[rows]))
        # 3: the per-column policy of batch_solve_cols on top of 2
        relres = np.linalg.norm(bvec - Ab @ x) / np.linalg.norm(bvec)
        refined = relres > RTOL
        if refined:
            x = x + solve_again(tree, K, rows, bvec - Ab @ x)
        err = err_of(x)
        print(f"{case} row {j}: m {mm}, cond(K) {np.linalg.cond(K):.2e}, asymmetry {asym:.2e} "
              f"({asym_lu:.2e} exact) | 1 exact tree solve {form:.2e} | 2 direct_model first "
              f"pass {first:.2e}, Z w form {zw:.2e}, ratio {first / zw:.2f} | 3 residual "
              f"{relres:.2e}, refined {refined}, error {err:.2e}")
        assert asym <= 1e-12 and asym_lu <= 1e-12, (j, asym, asym_lu)  # K_j is symmetric
        assert form <= BAR, (j, form)
        assert first <= SOL_TOL, (j, first)
        assert first <= FORM_FACTOR * zw, (j, first, zw)
        assert err <= BAR, (j, err)
