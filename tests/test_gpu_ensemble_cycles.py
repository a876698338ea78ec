"""Ensembles on graphs with cycles: ``Solver(..., ensemble_cycles=True)`` /
``nx_set_ensemble_cycles`` -- a cycle correction per scenario in the solve-again form
(``k_e_cyc_unit`` / ``k_e_cyc_extract`` / ``k_e_cyc_factor`` / ``k_e_cyc_w`` / ``k_e_cyc_restore``).

Set-up, scenarios, rows of R and yardsticks are ``tests/test_gpu_ensemble.py``'s (B = 11, the
seven cycled scenarios with the zero column, per scenario the oracle's LU at that scenario's R
and, where f = 0, the analytic resistor network; the project's bar SOL_TOL = 1e-10 on every row,
row 10 with its +-2 decades included) on ``cases.CYCLIC``: edge_info_N10 (m = 2 n_cyc = 4),
lattice4x5_N6 (m = 24), lattice6x6_N3 (m = 50: 550 unit columns, 8 passes of 64 and one of 38,
passes straddle scenarios), lattice19x20_N2 (m = 684: the factorisation in global memory).

Launches (include/nxhip.h, "Launches with cycles"): with P = ceil(nc m / 64) per chunk of nc
scenarios, ``solve_ensemble`` 5 P + 13, ``gradient(R=...)`` 5 P + 24 (objective alone 5 P + 13),
``hessian_vector(R=...)`` 5 P + 48 (Gauss-Newton 5 P + 37), and 11 more per refinement pass.

The batched results are not bit-equal to the one-matrix path (``solve_many`` at the same R): the
correction solves again with ``b - U w`` where that path subtracts ``Z w``. Both are held to the
oracle.

Gradients and Hessian-vector products follow the project's convention (test_gpu_gradient.py,
test_gpu_hvp.py): the yardstick is the CPU adjoint / the CPU product at each R_j, the bar 10 x
the largest relative error measured on an MI355X over the cases below, rounded up, never above
1e-8. Measured: see GRAD_MEASURED_BY_CASE and HVP_MEASURED_BY_CASE.

Refinement (test_refinement_pass): lattice19x20_N2 at rtol = 1e-13, the setting
test_gpu_gradient.py's refinement test uses; see that test's docstring for the figures."""

from __future__ import annotations

import numpy as np
import pytest

from gradient_ref import AdjointRef
from networks_fenicsx_amd import Solver, _lib
from test_gpu_ensemble import (B, SOL_TOL, GradSetup, HandleState, Setup, check_against_oracle,
                               env, oracle, rel)
from test_gpu_hvp import G_NAMES, MODES, HvpSetup, assert_same_bits
from test_gpu_hvp import parity_errors as hvp_errors

pytestmark = pytest.mark.gpu

GRAD_MEASURED_BY_CASE = {  # worst figure of the case on an MI355X (test_gradient_at_many_R)
    "edge_info_N10": 3.680e-13, "lattice6x6_N3": 3.738e-14, "lattice19x20_N2": 5.452e-13}
GRAD_MEASURED = max(GRAD_MEASURED_BY_CASE.values())  # (dR, least squares, the resident R)
GRAD_BAR = 5.5e-12  # 10 x GRAD_MEASURED (rounded up); may never exceed 1e-8
assert 10 * GRAD_MEASURED <= GRAD_BAR <= 1e-8

HVP_MEASURED_BY_CASE = {  # worst figure of the case (test_hessian_vector_at_many_R)
    "edge_info_N10": 8.955e-13, "lattice6x6_N3": 2.329e-13}
HVP_MEASURED = max(HVP_MEASURED_BY_CASE.values())
HVP_BAR = 9.0e-12  # 10 x HVP_MEASURED (rounded up); may never exceed 1e-8
assert 10 * HVP_MEASURED <= HVP_BAR <= 1e-8

W = 64  # the workspace's columns on a handle that has opted in (kBatchChunkMax)


def m_of(s):
    """m = 2 n_cyc: two rows per independent cycle of the (connected) graph."""
    return 2 * (s.mesh.num_edges - s.mesh.num_nodes + 1)


def passes(nc, m):
    return -(-nc * m // W)


def solve_launches(chunks, m, refined_chunks=0):
    """include/nxhip.h: 5 P + 13 per chunk, 11 more for a chunk with a refinement pass."""
    return sum(5 * passes(nc, m) + 13 for nc in chunks) + 11 * refined_chunks


def cyc_solver(s, **opts):
    return Solver(s.asm, petsc_options=opts or None, ensemble_cycles=True)


# 1, 5 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge_info_N10", "lattice4x5_N6", "lattice6x6_N3"])
def test_parity_with_the_oracle_and_handle_untouched(name):
    s = Setup(name)
    try:
        solver = cyc_solver(s)
        state = HandleState(s, solver)
        h = s.asm.handle
        m = m_of(s)
        writes = h.values_kept()["writes"]
        res = solver.solve_ensemble(s.R, s.items, s.f)
        assert h.values_kept()["writes"] == writes
        info = h.ensemble_cycles_info()
        print(f"{name}: m {m}, info {res.info}, {info}")
        assert res.path == "batched" and res.info["fallback"] == 0
        assert res.info["chunk"] == B
        assert info == {"enabled": True, "unit_solves": B * m, "storage": 1}
        assert res.info["launches"] == solve_launches([B], m, int(res.info["refined"] > 0))
        assert res.x.shape == (B, h.n_rows)
        errs = check_against_oracle(s, res, range(B), s.R)
        print(f"{name}: worst {max(errs.values()):.3e} (row 10: {errs[10]:.3e})")
        # the handle's own cycle correction was neither used nor rebuilt: a solve_many now finds
        # everything current (9 launches per chunk with cycles, 8 more with a refinement pass)
        many = solver.solve_many(s.items[:3], s.f[:3])
        assert many.info["launches"] == 9 + 8 * int(many.info["refined"] > 0), many.info
        state.check()
    finally:
        s.close()


# 2 ---------------------------------------------------------------------------------------
def test_factorisation_in_global_memory():
    """m = 684: K_j (3.7 MB) does not fit a workgroup's LDS. B = 3 rows: the resident R, a +-1
    decade row, row 10; 3 x 684 = 2052 unit columns in 33 passes."""
    s = Setup("lattice19x20_N2")
    try:
        solver = cyc_solver(s)
        solver.assemble()
        solver.solve()
        cols = [0, 3, 10]
        m = m_of(s)
        assert m == 684
        res = solver.solve_ensemble(s.R[cols], [s.items[j] for j in cols], s.f[cols])
        info = s.asm.handle.ensemble_cycles_info()
        print(f"info {res.info}, {info}")
        assert res.path == "batched" and res.info["fallback"] == 0
        assert info == {"enabled": True, "unit_solves": 3 * m, "storage": 2}
        assert res.info["launches"] == solve_launches([3], m, int(res.info["refined"] > 0))
        check_against_oracle(s, res, cols, s.R[cols])
    finally:
        s.close()


def test_forced_global_memory_variant():
    """NXHIP_ENS_CYC_LDS=0: the same body with K_j in global memory, the same bars (and, the
    operations being the same, the LDS variant's bits)."""
    s = Setup("lattice6x6_N3")
    try:
        solver = cyc_solver(s)
        solver.assemble()
        solver.solve()
        lds = solver.solve_ensemble(s.R, s.items, s.f)
        assert s.asm.handle.ensemble_cycles_info()["storage"] == 1
        with env(NXHIP_ENS_CYC_LDS=0):
            res = solver.solve_ensemble(s.R, s.items, s.f)
        info = s.asm.handle.ensemble_cycles_info()
        assert res.path == "batched" and res.info["fallback"] == 0
        assert info == {"enabled": True, "unit_solves": B * m_of(s), "storage": 2}
        check_against_oracle(s, res, range(B), s.R)
        np.testing.assert_array_equal(res.x, lds.x)
    finally:
        s.close()


# 3 ---------------------------------------------------------------------------------------
def test_a_columns_bits_depend_on_the_column_alone():
    s = Setup("lattice4x5_N6")
    try:
        solver = cyc_solver(s)
        m = m_of(s)
        a = solver.solve_ensemble(s.R, s.items, s.f)
        assert a.path == "batched"
        with env(NXHIP_BATCH_CHUNK=4):  # chunks 4 + 4 + 3
            b = solver.solve_ensemble(s.R, s.items, s.f)
            assert b.info["chunk"] == 4
            assert b.info["launches"] == solve_launches(
                [4, 4, 3], m, sum(bool((b.iterations[c:c + 4] == 2).any()) for c in (0, 4, 8)))
            assert s.asm.handle.ensemble_cycles_info()["unit_solves"] == B * m
        c = solver.solve_ensemble(s.R[::-1], s.items[::-1], s.f[::-1])
        for other, sl in ((b, slice(None)), (c, slice(None, None, -1))):
            np.testing.assert_array_equal(other.x[sl], a.x)
            np.testing.assert_array_equal(other.iterations[sl], a.iterations)
            np.testing.assert_array_equal(other.residual_norms[sl], a.residual_norms)
    finally:
        s.close()


# 4 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge_info_N10", "lattice6x6_N3"])
def test_consistent_with_the_one_matrix_path(name):
    """Every row of R the resident one: solve_ensemble against solve_many. Both within SOL_TOL
    of the oracle and of each other; not bit-equal (x = A_g^{-1} (b - U w) is a different sum
    from x_g - Z w)."""
    s = Setup(name)
    try:
        solver = cyc_solver(s)
        R = np.tile(s.R0, (B, 1))
        many = solver.solve_many(s.items, s.f)
        ens = solver.solve_ensemble(R, s.items, s.f)
        assert many.path == ens.path == "batched"
        check_against_oracle(s, many, range(B), R)
        check_against_oracle(s, ens, range(B), R)
        for j in range(B):
            if many.x[j].any():
                d = rel(ens.x[j], many.x[j])
                print(f"{name} scenario {j}: ensemble vs solve_many {d:.3e}")
                assert d <= SOL_TOL, (j, d)
    finally:
        s.close()


# 6 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge_info_N10", "lattice6x6_N3", "lattice19x20_N2"])
def test_gradient_at_many_R(name):
    """value, dR, df, dp_bc of scenario j against the CPU adjoint at R_j, both kinds;
    derivatives=False gives the same value bits and no derivatives."""
    s = GradSetup(name)
    try:
        solver = cyc_solver(s)
        solver.assemble()
        solver.solve()
        m = m_of(s)
        P = passes(3, m)
        refs = [AdjointRef(s.P, s.R[j]) for j in range(3)]
        worst = 0.0
        for kind, data in (("linear", None), ("lsq", s.data)):
            g = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=data, R=s.R)
            assert g.converged.all() and g.converged.shape == (3, 2)
            assert g.info["fallback"] == 0
            assert g.info["launches"] == 5 * P + 24 + 11 * int(
                (g.iterations[:, 0] == 2).any()) + 11 * int((g.iterations[:, 1] == 2).any())
            assert s.asm.handle.ensemble_cycles_info()["unit_solves"] == 3 * m
            for j in range(3):
                r = refs[j].gradient(s.nodal[j], s.f[j], s.rows, s.w,
                                     None if data is None else data[j])
                errs = {"value": abs(g.value[j] - r["value"]) / abs(r["value"]),
                        "dR": rel(g.dR[j], r["dR"]), "df": rel(g.df[j], r["df"]),
                        "dp_bc": rel(g.dp_bc[j], r["dp_bc"])}
                print(f"{name} {kind} scenario {j}: "
                      + ", ".join(f"{k} {v:.2e}" for k, v in errs.items())
                      + f" (refined {g.info['refined']})")
                worst = max(worst, *errs.values())
            obj = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=data, R=s.R,
                                  derivatives=False)
            np.testing.assert_array_equal(obj.value, g.value)
            assert obj.dR is None and obj.df is None and obj.dp_bc is None
            assert obj.converged.all() and obj.info["launches"] == 5 * P + 13 + 11 * int(
                (obj.iterations == 2).any())
        print(f"{name}: worst {worst:.3e}")
        assert worst <= GRAD_BAR, worst
    finally:
        s.close()


# 7 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge_info_N10", "lattice6x6_N3"])
def test_hessian_vector_at_many_R(name):
    """Full mode (both kinds) and Gauss-Newton against the CPU product at each R_j =
    10^U(-1, 1); grad_* of the full call are gradient(R=...)'s bits."""
    s = HvpSetup(name)
    try:
        solver = cyc_solver(s)
        solver.assemble()
        solver.solve()
        R = 10.0 ** np.random.default_rng(5).uniform(-1.0, 1.0, (3, s.mesh.num_edges))
        P = passes(3, m_of(s))
        worst = 0.0
        for mode, lsq, gn in MODES:
            data = s.data if lsq else None
            hv = solver.hessian_vector(s.items, s.f, data=data, gauss_newton=gn, R=R, **s.kw,
                                       **s.dirs[0])
            assert hv.converged.all() and hv.info["fallback"] == 0
            n_ref = int((hv.iterations == 2).any(axis=0).sum())
            assert hv.info["launches"] == 5 * P + (37 if gn else 48) + 11 * n_ref, hv.info
            for j, errs in enumerate(hvp_errors(s, hv, data, s.dirs[0], gn, R=R)):
                print(f"{name} {mode} scenario {j}: "
                      + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
                worst = max(worst, *errs.values())
            if not gn:
                g = solver.gradient(s.items, s.f, data=data, R=R, **s.kw)
                assert_same_bits(hv, g, slice(None), slice(None), names=G_NAMES)
        print(f"{name}: worst {worst:.3e}")
        assert worst <= HVP_BAR, worst
    finally:
        s.close()


# 8 ---------------------------------------------------------------------------------------
def test_refinement_pass():
    """lattice19x20_N2, rtol = 1e-13 (what one pass of the direct solve does not reach there):
    the columns above it take the refinement pass through their own factors -- sweeps,
    k_e_cyc_w, sweeps, k_e_cyc_restore on the list of those columns -- and meet SOL_TOL; the
    launches follow the formula with its refinement term. The device's figures are read from
    the handle's call (no sequential fallback in between).

    Measured on an MI355X: iterations [1, 1, 2] -- row 10 is refined, from above 1e-13 to a
    relative residual of 3.4e-15 -- 189 = 5 x 33 + 13 + 11 launches; against the oracle 2.0e-13,
    1.3e-14, 2.9e-14."""
    s = Setup("lattice19x20_N2")
    try:
        solver = cyc_solver(s, ksp_rtol=1e-13, ksp_error_if_not_converged=False)
        solver.assemble()
        solver.solve()
        cols = [0, 3, 10]
        h = s.asm.handle
        bc, ef, fc = s.asm.scenario_coefficients([s.items[j] for j in cols], s.f[cols])
        eR = s.R[cols][:, s.asm._edge_ids]
        x, it, rr, cv = h.ensemble_solve(eR, bc, ef, fc, 1e-13)
        info = h.batch_info()
        print(f"iterations {it.tolist()}, relres {rr.tolist()}, converged {cv.tolist()}, {info}")
        assert info["refined"] > 0 and info["refined"] == int((it == 2).sum())
        assert info["launches"] == solve_launches([3], m_of(s), 1)
        for i, j in enumerate(cols):
            x_ref, _, _ = oracle(s, j, s.R[j])
            e = rel(x[i], x_ref)
            print(f"scenario {j}: vs oracle {e:.3e}")
            assert np.isfinite(x[i]).all() and e <= SOL_TOL, (j, e)
    finally:
        s.close()


# 9 ---------------------------------------------------------------------------------------
def test_off_by_default_and_abi():
    s = Setup("edge_info_N10")
    try:
        h = s.asm.handle
        solver = Solver(s.asm)
        solver.assemble()
        solver.solve()
        assert h.ensemble_cycles_info()["enabled"] is False
        assert h.batch_supported() and not h.ensemble_supported()
        res = solver.solve_ensemble(s.R[:2], s.items[:2], s.f[:2])
        assert res.path == "sequential"
        with pytest.raises(NotImplementedError):
            solver.gradient(s.items[:2], rows=np.array([0]), R=np.array([1.0, 2.0]))
        h.set_ensemble_cycles(True)
        assert h.ensemble_supported() and h.ensemble_cycles_info()["enabled"] is True
        h.set_ensemble_cycles(False)
        assert not h.ensemble_supported()
        L = _lib.lib()
        assert L.nx_set_ensemble_cycles(None, 1) == _lib.NX_ERR_ARG
        assert L.nx_get_ensemble_cycles(None, None, None, None) == _lib.NX_ERR_ARG
        assert L.nx_set_ensemble_cycles(h.ptr, 2) == _lib.NX_ERR_ARG
        assert L.nx_get_ensemble_cycles(h.ptr, None, None, None) == _lib.NX_OK
        assert L.nx_version() >= 10200
        # two solvers on one assembler: each call configures the handle for its own solver
        on = cyc_solver(s)
        assert on.solve_ensemble(s.R[:2], s.items[:2], s.f[:2]).path == "batched"
        assert solver.solve_ensemble(s.R[:2], s.items[:2], s.f[:2]).path == "sequential"
        with env(NXHIP_ENS_CYCLES=1):
            assert Solver(s.asm).solve_ensemble(s.R[:2], s.items[:2], s.f[:2]).path == "batched"
    finally:
        s.close()


def test_a_forest_is_unchanged_by_the_flag():
    s = Setup("tree5_N15")
    try:
        plain = Solver(s.asm)
        plain.assemble()
        plain.solve()  # (the calls below find the values assembled)
        off = plain.solve_ensemble(s.R, s.items, s.f)
        on = cyc_solver(s).solve_ensemble(s.R, s.items, s.f)
        assert off.path == on.path == "batched"
        assert on.info["launches"] == off.info["launches"]
        assert s.asm.handle.ensemble_cycles_info() == {"enabled": True, "unit_solves": 0,
                                                       "storage": 0}
        np.testing.assert_array_equal(on.x, off.x)
        np.testing.assert_array_equal(on.iterations, off.iterations)
        np.testing.assert_array_equal(on.residual_norms, off.residual_norms)
    finally:
        s.close()
