"""Continuous pressure (k > m >= 1) on graphs with cycles, on the GPU: the node-condensed
direct solve with the chords' correction (``cycle_direct=True`` / ``NXHIP_CP_CYCLES=1``;
``nx_fe_cp_set_cycles``).

Tolerances: the solution <= 1e-10 relative 2-norm against the oracle's LU of its own
(independently integrated) system -- the direct solve's bar, as on forests; the reported
residual is the true one (<= 1e-12, the solve's rtol). On forests the switch changes no
launch: the same bits."""

from __future__ import annotations

import logging

import numpy as np
import pytest

from cases import CASES, CYCLIC, lattice_graph, p_y
from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh, Solver, _lib
from networks_fenicsx_amd.layout_fe import build_cp_tables, build_fe_layout
from oracle import nx_oracle as O
from oracle import nx_oracle_fe as OF
from test_gpu_fe_ranks import _gather, _reference, _run

pytestmark = pytest.mark.gpu

SOL_TOL = 1e-10
CHORDS = {"edge_info_N10": 2, "lattice4x5_N6": 12, "lattice6x6_N3": 25, "lattice19x20_N2": 342}


def _setup(case, km, f=None, R=None, cycle_direct=True):
    make, N = CYCLIC[case]
    mesh = NetworkMesh(make(), N=N)
    asm = HydraulicNetworkAssembler(mesh, flux_degree=km[0], pressure_degree=km[1],
                                    cycle_direct=cycle_direct)
    asm.compute_forms(p_bc_ex=p_y, f=f, R=R)
    src, dst = mesh.edges
    F = OF.build_problem_fe(mesh.node_coordinates, src, dst, N, *km, mesh.edge_colors)
    return mesh, asm, F


def _check_direct(asm, solver, F, f, R, pbc=p_y):
    """One assembled solve: direct, node-condensed, corrected, <= SOL_TOL of the oracle."""
    solver.assemble()
    sol = solver.solve()
    assert solver.ksp.solver_used == "direct" and solver.ksp.converged
    assert asm.handle.direct_path() == "node-condensed"
    assert 1 <= solver.ksp.iterations <= 3
    assert asm.handle.cp_cycles()["ran"]
    A, b = OF.assemble_reference_fe(F, pbc, f=f, R=R)
    x_ref = O.solve_reference(A, b)
    got = np.concatenate([fn.x.array for fn in sol])
    err = np.linalg.norm(got - x_ref) / np.linalg.norm(x_ref)
    tr = solver.true_residual()
    print(f"err {err:.2e} residual {tr:.2e} passes {solver.ksp.iterations}")
    assert err <= SOL_TOL
    assert tr <= 1e-12
    assert abs(solver.ksp.residual_estimate - tr) <= 1e-6 * tr + 1e-16


@pytest.mark.parametrize("case,km", [("edge_info_N10", (2, 1)), ("edge_info_N10", (3, 2)),
                                     ("edge_info_N10", (3, 1)), ("edge_info_N10", (4, 3)),
                                     ("lattice4x5_N6", (2, 1)), ("lattice4x5_N6", (3, 2)),
                                     ("lattice6x6_N3", (2, 1)), ("lattice6x6_N3", (3, 2))])
def test_cycles_direct(case, km):
    """The direct solve on a graph with cycles; a second solve with another per-edge R builds
    the capacitance matrix again, a third with only new boundary values and source does not."""
    E = len(CYCLIC[case][0]().edges())
    R = 1.0 + 0.5 * (np.arange(E) % 3)
    mesh, asm, F = _setup(case, km, f=0.4, R=R)
    assert asm.fe_direct_available
    assert np.asarray(asm._fe_cp.chord).size == CHORDS[case]
    solver = Solver(asm)
    _check_direct(asm, solver, F, 0.4, R)
    builds = asm.handle.cp_cycles()["builds"]
    assert builds == 1
    R2 = 2.0 - 0.25 * (np.arange(E) % 4)
    asm.compute_forms(p_bc_ex=p_y, f=0.1, R=R2)
    _check_direct(asm, solver, F, 0.1, R2)
    assert asm.handle.cp_cycles()["builds"] == builds + 1
    p2 = lambda x: 0.5 * x[0] - x[1] + 2.0  # noqa: E731
    asm.compute_forms(p_bc_ex=p2, f=0.7, R=R2)
    _check_direct(asm, solver, F, 0.7, R2, pbc=p2)
    assert asm.handle.cp_cycles()["builds"] == builds + 1


def test_cycles_direct_342_chords():
    case = "lattice19x20_N2"
    E = len(CYCLIC[case][0]().edges())
    R = 1.0 + 0.5 * (np.arange(E) % 3)
    mesh, asm, F = _setup(case, (2, 1), f=0.4, R=R)
    assert asm.fe_direct_available and np.asarray(asm._fe_cp.chord).size == 342
    _check_direct(asm, Solver(asm), F, 0.4, R)


@pytest.mark.parametrize("case", ["depth6_N40", "arterial5_N40"])
def test_forest_unchanged(case):
    make, N, strategy, pbc = CASES[case]
    E = len(make().edges())
    R = 1.0 + 0.5 * (np.arange(E) % 3)
    xs = []
    for flag in (True, None):
        mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
        kw = {} if flag is None else {"cycle_direct": flag}
        asm = HydraulicNetworkAssembler(mesh, flux_degree=2, pressure_degree=1, **kw)
        asm.compute_forms(p_bc_ex=pbc, f=0.4, R=R)
        solver = Solver(asm)
        solver.assemble()
        solver.solve()
        assert solver.ksp.solver_used == "direct"
        assert asm.handle.direct_path() == "node-condensed"
        assert asm.handle.cp_cycles() == {"ran": False, "builds": 0}
        xs.append(asm.handle.solution())
    np.testing.assert_array_equal(xs[0], xs[1])


def test_switch_off_overrides_environment(monkeypatch):
    monkeypatch.setenv("NXHIP_CP_CYCLES", "1")
    mesh, asm, F = _setup("edge_info_N10", (2, 1), cycle_direct=False)
    assert not asm.fe_direct_available
    solver = Solver(asm)
    solver.assemble()
    solver.solve()
    assert solver.ksp.solver_used == "minres" and solver.ksp.converged
    assert not asm.handle.cp_cycles()["ran"]


def test_environment_switches_on(monkeypatch):
    monkeypatch.setenv("NXHIP_CP_CYCLES", "1")
    mesh = NetworkMesh(CYCLIC["edge_info_N10"][0](), N=10)
    asm = HydraulicNetworkAssembler(mesh, flux_degree=2, pressure_degree=1)
    assert asm.fe_direct_available


def _n_slots(n):
    mesh = NetworkMesh(lattice_graph(n, n), N=2)
    src, dst = mesh.edges
    lay = build_fe_layout(np.asarray(mesh.node_coordinates, dtype=np.float64), src, dst,
                          mesh.degrees, 2, 2, 1)
    return mesh, np.asarray(build_cp_tables(lay, src, dst, cycles=True).cslot).size // 2


def test_past_the_cap_runs_minres(caplog):
    """The smallest square lattice with more border slots at chord ends than the cap: the
    assembler detaches the tables and warns once; nothing is solved."""
    n = 46
    assert _n_slots(n - 1)[1] <= _lib.MAX_CP_SLOTS
    mesh, ns = _n_slots(n)
    assert ns > _lib.MAX_CP_SLOTS
    with caplog.at_level(logging.WARNING):
        asm = HydraulicNetworkAssembler(mesh, flux_degree=2, pressure_degree=1,
                                        cycle_direct=True)
    assert not asm.fe_direct_available
    warned = [r for r in caplog.records if r.levelno >= logging.WARNING]
    assert len(warned) == 1
    assert "chords" in warned[0].getMessage() and "MINRES" in warned[0].getMessage()


def test_set_cycles_rejects_bad_tables():
    mesh, asm, F = _setup("edge_info_N10", (2, 1))
    tab = asm._fe_cp
    h = asm.handle
    from dataclasses import replace

    par = np.asarray(tab.parent).reshape(-1, 3)
    tree_edge = int(par[par[:, 1] >= 0, 1][0])
    for bad in (replace(tab, chord=np.array([10 ** 6], np.int32)),
                replace(tab, chord=np.array([tree_edge], np.int32)),
                replace(tab, cslot=np.asarray(tab.cslot)[::-1].copy()),
                replace(tab, cslot=np.asarray(tab.cslot)[2:])):
        with pytest.raises(_lib.NxError):
            h.fe_cp_set_cycles(bad)
    h.fe_cp_set_cycles(tab)  # (the tables themselves attach again)
    asm.compute_forms(p_bc_ex=p_y, f=0.4, R=None)
    _check_direct(asm, Solver(asm), F, 0.4, 1.0)


@pytest.mark.parametrize("P,km", [(2, (2, 1)), (3, (3, 2))])
def test_cycles_ranks(tmp_path, monkeypatch, P, km):
    """Several ranks (one process each, at most 3 on the GPU, the host transport): every
    rank forms the same capacitance matrix from the summed blocks."""
    monkeypatch.setenv("NXHIP_CP_CYCLES", "1")
    case = "edge_info_N10"
    ranks, data = _run(tmp_path, case, P, km[0], steps=2, m=km[1])
    x_ref = _reference(case, *km)
    for s in range(2):
        for r in range(P):
            st = ranks[r][s]
            assert st["direct_available"] and st["solver"] == "direct", (r, st)
            assert st["path"] == "node-condensed" and st["converged"], (r, st)
            assert st["relres"] == ranks[0][s]["relres"]
        x = _gather(data, s, x_ref.size)
        err = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
        print(f"step {s}: err {err:.2e} relres {ranks[0][s]['relres']:.2e}")
        assert err <= SOL_TOL, s
