"""Direct tree solve on the device (``nx_set_solver(h, 1)``; ``Solver`` with the
reference's default ``ksp_type="preonly"`` + ``pc_type="lu"``, solver.py:58-65).

Tolerances: solution <= 1e-10 relative 2-norm against the oracle's sparse direct solve
(SuperLU, the MUMPS stand-in) and the analytic resistor-network answer; the reported true
residual <= 1e-12. Graphs with cycles (the reference's edge_info graph, grid networks) run
the direct solve too, with the Woodbury correction of their cycle-closing chains
(nx_set_cycles), to the same bar."""

from __future__ import annotations

import numpy as np
import pytest

from cases import CASES
from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh, Solver
from networks_fenicsx_amd import network_generation as ng
from oracle import nx_oracle as O
from tree_shapes import block_errors_oracle

pytestmark = pytest.mark.gpu

SOL_TOL = 1e-10


def _setup(case, **forms):
    make, N, strategy, pbc = CASES[case]
    mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
    asm = HydraulicNetworkAssembler(mesh)
    asm.compute_forms(p_bc_ex=pbc, **forms)
    src, dst = mesh.edges
    P = O.build_problem(mesh.node_coordinates, src, dst, N, mesh.edge_colors)
    A, b = O.assemble_reference(P, pbc, **forms)
    return mesh, asm, P, A, b, pbc


@pytest.mark.parametrize("case", sorted(CASES))
def test_direct_solve_matches_oracle(case):
    mesh, asm, P, A, b, pbc = _setup(case)
    solver = Solver(asm)  # reference defaults: preonly + lu
    solver.assemble()
    sol = solver.solve()
    assert solver.ksp.solver_used == "direct"  # trees and (one rank) graphs with cycles
    assert solver.ksp.getIterationNumber() in (1, 2)  # 2: one refinement step
    assert solver.ksp.getResidualNorm() <= 1e-12
    x_ref = O.solve_reference(A, b)
    got = np.concatenate([f.x.array for f in sol])  # the reference's block order
    assert np.linalg.norm(got - x_ref) / np.linalg.norm(x_ref) <= SOL_TOL
    # fluxes, pressures and multipliers each: the pressures carry the norm of x on these graphs
    assert max(block_errors_oracle(got, x_ref, P.p_offset, P.lm_offset)) <= SOL_TOL
    xa = O.resistor_network_solution(P, pbc)
    assert np.linalg.norm(got - xa) / np.linalg.norm(xa) <= SOL_TOL
    assert solver.true_residual() <= 1e-12


def test_direct_equals_minres_and_reassembles():
    """Same solution as preconditioned MINRES; the captured graph stays valid across
    reassembly with new coefficients (per-edge R and f) -- the factorisation is redone
    from each assembly inside the graph."""
    mesh, asm, P, A, b, pbc = _setup("arterial5_N40")
    direct = Solver(asm)
    direct.assemble()
    xd = np.concatenate([f.x.array for f in direct.solve()])
    it_solver = Solver(asm, petsc_options={"ksp_type": "minres"})
    xm = np.concatenate([f.x.array for f in it_solver.solve()])
    assert it_solver.ksp.solver_used == "minres" and it_solver.ksp.getIterationNumber() <= 4
    assert np.linalg.norm(xd - xm) / np.linalg.norm(xm) <= 1e-11
    R = 1.0 / mesh.edge_radius ** 4
    f = 0.1 + 0.02 * (np.arange(mesh.num_edges) % 5)
    asm.compute_forms(p_bc_ex=pbc, f=f, R=R)
    direct.assemble()
    x2 = np.concatenate([fn.x.array for fn in direct.solve()])
    assert direct.ksp.solver_used == "direct"
    A2, b2 = O.assemble_reference(P, pbc, f=f, R=R)
    x_ref = O.solve_reference(A2, b2)
    assert np.linalg.norm(x2 - x_ref) / np.linalg.norm(x_ref) <= SOL_TOL


def test_direct_needs_the_exact_preconditioner():
    mesh, asm, P, A, b, pbc = _setup("depth6_N40")
    lumped = Solver(asm, petsc_options={"pc_mass": "lumped"})
    lumped.assemble()
    lumped.solve()
    assert lumped.ksp.solver_used == "minres"
    plain = Solver(asm, petsc_options={"pc_type": "none"})
    plain.solve()
    assert plain.ksp.solver_used == "minres"
    back = Solver(asm)
    back.solve()
    assert back.ksp.solver_used == "direct"


@pytest.mark.parametrize("N", [300, 700, 1024])
def test_direct_long_edges(N):
    """Chain layouts (64, 8) / (64, 16) of N > 256 (demo_tree.py doubles N to 1024)."""
    mesh = NetworkMesh(ng.make_tree(3, 1, 1), N=N)
    asm = HydraulicNetworkAssembler(mesh)
    asm.compute_forms(p_bc_ex=lambda x: x[1])
    solver = Solver(asm)
    solver.assemble()
    solver.solve()
    assert solver.ksp.solver_used == "direct"
    src, dst = mesh.edges
    P = O.build_problem(mesh.node_coordinates, src, dst, N, mesh.edge_colors)
    A, b = O.assemble_reference(P, lambda x: x[1])
    _, _, perm, _ = O.to_build_layout(P, A, b)
    x_ref = O.solve_reference(A, b)
    x = solver.solution_vector()
    assert np.linalg.norm(x - x_ref[perm]) / np.linalg.norm(x_ref) <= SOL_TOL


@pytest.mark.parametrize("levels,N", [(15, 15), (12, 40)])
def test_direct_large_tree_analytic(levels, N):
    """C3 (make_tree(15), N = 15, 1,032,160 DoF) and a deep-N tree: analytic answer to
    1e-10 through the C ABI, repeated solves bit-identical (no state carried over)."""
    mesh = NetworkMesh(ng.make_tree(levels, levels, levels), N=N, color_strategy="smallest_last")
    asm = HydraulicNetworkAssembler(mesh)
    asm.compute_forms(p_bc_ex=lambda x: x[1])
    asm.set_direct(True)
    h = asm.handle
    asm.assemble()
    it, relres, conv = h.solve(1e-12, 100, 4)
    assert conv and it in (1, 2) and relres <= 1e-12 and h.solver() == (1, 1)
    x1 = h.solution()
    asm.assemble()
    h.solve(1e-12, 100, 4)
    np.testing.assert_array_equal(h.solution(), x1)
    src, dst = mesh.edges
    P = O.build_problem(mesh.node_coordinates, src, dst, N)
    xa = O.resistor_network_solution(P, lambda x: x[1])[O.build_permutation(P)[0]]
    assert np.linalg.norm(x1 - xa) / np.linalg.norm(xa) <= SOL_TOL
    asm.close()


def test_deferred_assembly_keeps_call_order():
    """nx_assemble is deferred on one rank (it heads the direct solve's graph), but every
    other call flushes it first: an assembly followed by new coefficients still holds the
    old ones, exactly as if it had run at once."""
    mesh, asm, P, A, b, pbc = _setup("depth6_N40")
    h = asm.handle
    asm.assemble()
    asm.compute_forms(p_bc_ex=pbc, R=2.0)  # uploads R = 2 after the pending assembly ran
    Ab, bb, _, _ = O.to_build_layout(P, A, b)
    np.testing.assert_array_equal(h.csr()[2], Ab.data)
    np.testing.assert_array_equal(h.rhs(), bb)
    asm.assemble()
    A2, b2 = O.assemble_reference(P, pbc, R=2.0)
    Ab2, bb2, perm, _ = O.to_build_layout(P, A2, b2)
    np.testing.assert_array_equal(h.csr()[2], Ab2.data)
    asm.assemble()  # deferred into the solve's graph
    asm.set_direct(True)
    it, relres, conv = h.solve(1e-12, 100, 4)
    assert conv and h.solver()[1] == 1
    x_ref = O.solve_reference(A2, b2)[perm]
    assert np.linalg.norm(h.solution() - x_ref) / np.linalg.norm(x_ref) <= SOL_TOL
    asm.assemble(assemble_lhs=False)  # rhs only: flushed, then the plain direct graph
    it, relres, conv = h.solve(1e-12, 100, 4)
    assert conv and np.linalg.norm(h.solution() - x_ref) / np.linalg.norm(x_ref) <= SOL_TOL


@pytest.mark.parametrize("case", ["depth6_N40", "arterial5_N40", "tree6_2d_N70", "Y_N4",
                                  "demo_tree_N1", "linear_alt_N3"])
def test_fused_residual_is_the_true_residual(case, monkeypatch):
    """The down sweep forms r = b - A x itself (PcArgs::fres; the top part's multiplier rows in
    k_dir_publish_fr): the reported residual is the true one (host SpMV of the assembled CSR)
    to 5%, the solution is bit-identical to the unfused check's (NXHIP_DIR_FRES=0), and a
    forced refinement step (rtol just under the first pass's residual) converges with the
    refined residual reported truthfully too."""
    mesh, asm, P, A, b, pbc = _setup(case)
    # the four-launch path's fused check (the fused step k_dir_step has its own tests,
    # tests/test_gpu_dstep.py, and forms other FMAs: ~1 ulp on some entries)
    monkeypatch.setenv("NXHIP_DIR_FUSED", "0")
    asm.set_direct(True)
    h = asm.handle
    asm.assemble()
    it, rr, conv = h.solve(1e-12, 100, 4)
    assert conv and it == 1 and h.solver() == (1, 1)
    x_fused = h.solution()
    true1 = h.true_residual()
    assert abs(rr - true1) <= 0.05 * true1 + 5e-16, (rr, true1)  # 5e-16: see below
    monkeypatch.setenv("NXHIP_DIR_FRES", "0")
    asm.set_direct(True)
    asm.set_preconditioner(True)
    asm.assemble()
    it0, rr0, _ = h.solve(1e-12, 100, 4)
    np.testing.assert_array_equal(h.solution(), x_fused)
    assert abs(rr0 - rr) <= 0.05 * rr0 + 5e-16
    monkeypatch.delenv("NXHIP_DIR_FRES")
    asm.set_preconditioner(True)
    if rr > 4e-15:  # room for a refinement step below it
        asm.assemble()
        it2, rr2, conv2 = h.solve(rr / 2, 100, 4)
        assert h.solver() == (1, 1) and it2 == 2 and conv2, (it2, rr2)
        true2 = h.true_residual()
        # at ~1e-16 the two evaluations (fused sweep / host CSR SpMV, different summation
        # orders) differ by their own rounding, eps ||A|| ||x|| / ||b|| ~ 5e-16
        assert rr2 <= rr / 2 and abs(rr2 - true2) <= 0.05 * true2 + 5e-16, (rr2, true2)
        x_ref = O.solve_reference(A, b)
        _, _, perm, _ = O.to_build_layout(P, A, b)
        assert np.linalg.norm(h.solution() - x_ref[perm]) / np.linalg.norm(x_ref) <= SOL_TOL


@pytest.mark.parametrize("case", ["edge_info_N10", "lattice4x5_N6", "lattice6x6_N3",
                                  "lattice19x20_N2"])
def test_direct_solve_with_cycles(case, monkeypatch):
    """Graphs with cycles: the tree solve of A without the cycle chains' grounded couplings
    plus the rank-2k Woodbury correction (k_cyc_*), checked with the CSR's true residual;
    <= 1e-10 vs the oracle's sparse direct solve (MUMPS stand-in). A forced refinement step
    (rtol under the first pass's residual) is corrected the same way, and a reassembly with
    new coefficients rebuilds the correction."""
    from test_precond import CYCLIC

    make, N = CYCLIC[case]
    mesh = NetworkMesh(make(), N=N)
    asm = HydraulicNetworkAssembler(mesh)
    pbc = lambda x: x[1]  # noqa: E731
    asm.compute_forms(p_bc_ex=pbc)
    asm.set_direct(True)
    h = asm.handle
    src, dst = mesh.edges
    P = O.build_problem(mesh.node_coordinates, src, dst, N, mesh.edge_colors)
    A, b = O.assemble_reference(P, pbc)
    _, _, perm, _ = O.to_build_layout(P, A, b)
    asm.assemble()
    it, rr, conv = h.solve(1e-12, 100, 4)
    assert h.solver() == (1, 1) and conv and it in (1, 2) and rr <= 1e-12, (h.solver(), it, rr)
    x_ref = O.solve_reference(A, b)[perm]
    assert np.linalg.norm(h.solution() - x_ref) / np.linalg.norm(x_ref) <= SOL_TOL
    true1 = h.true_residual()
    assert abs(rr - true1) <= 0.05 * true1 + 5e-16, (rr, true1)
    if rr > 4e-15:
        asm.assemble()
        it2, rr2, conv2 = h.solve(rr / 2, 100, 4)
        assert h.solver() == (1, 1) and it2 == 2 and conv2 and rr2 <= rr / 2, (it2, rr2)
        assert np.linalg.norm(h.solution() - x_ref) / np.linalg.norm(x_ref) <= SOL_TOL
    R = 1.0 + 0.5 * (np.arange(mesh.num_edges) % 3)
    asm.compute_forms(p_bc_ex=pbc, R=R)
    asm.assemble()
    it, rr, conv = h.solve(1e-12, 100, 4)
    assert h.solver() == (1, 1) and conv and rr <= 1e-12
    A2, b2 = O.assemble_reference(P, pbc, R=R)
    x2 = O.solve_reference(A2, b2)[perm]
    assert np.linalg.norm(h.solution() - x2) / np.linalg.norm(x2) <= SOL_TOL
    asm.close()
