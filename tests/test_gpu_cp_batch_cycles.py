"""``Solver(asm, batch_continuous=True, batch_continuous_cycles=True)`` /
``nx_set_cp_batch_cycles``: the batched node-condensed solve of a continuous-pressure system
(k > m >= 1) on a graph with cycles -- the single solve's chord correction per column, on the
batch's own factors and its own capacitance inverse.

Set-up, scenarios, reference and bars are tests/test_gpu_cp_batch.py's (``Setup`` with
``cycle_direct=True``, the 7 columns, SuperLU on ``assemble_reference_fe``, ``check_columns``:
every non-zero column <= 1e-10 against the oracle, the reported residual <= 1e-12 and within
5 % + 5e-16 of the host's, the zero column exact zeros). tests/test_cp_batch_cycles_host.py holds
the numpy model to 1e-12 after one pass and at most one refinement on every graph below, so no
column may fall back.

Why these graphs: edge_info_N10 -- 2 chords, 6 slots (one partial 64-row block of the
inverse), edges 0.1 and 0.3 long in ten cells (the grounded refinement's case);
lattice4x5_N6 (32 slots) and lattice6x6_N3 (60 slots) -- nodes shared by several chords, below
one 64-row block; lattice19x20_N2 -- 722 slots: two ``k_cp_zcols`` batches, twelve row blocks,
the last partial. B = 7 and B = 9 leave partial column tiles (tiles of 4)."""

from __future__ import annotations

import numpy as np
import pytest

from cases import CASES
from networks_fenicsx_amd import Solver, _lib
from networks_fenicsx_amd import network_generation as ng
from networks_fenicsx_amd.post_processing import terminal_conductance
from test_gpu_batch import N_SCEN, env, rel
from test_gpu_cp_batch import PAIRS, SOL_TOL, ZERO, Setup, check_columns

pytestmark = pytest.mark.gpu

SMALL = ["edge_info_N10", "lattice4x5_N6", "lattice6x6_N3"]
CASES_KM = [(n, km) for n in SMALL for km in PAIRS] + [("lattice19x20_N2", (2, 1))]
SLOTS = {"edge_info_N10": 6, "lattice4x5_N6": 32, "lattice6x6_N3": 60, "lattice19x20_N2": 722}
# include/nxhip.h, nx_cp_batch_solve on a graph with cycles: no level of these node forests
# holds more than 128 nodes, so U = D = 1: the factor stage is 1 + U launches, a chunk with its
# blocks gathered 10 + 3 (U + D), a refinement pass 8 + 3 (U + D); the call that builds the
# inverse adds ceil(ns / min(ns, 512)) + 2 ns + 2 (the unit columns' batches, k_cp_cap, a pivot
# and an elimination per column, k_gj_out)
FACTOR, PER_CHUNK, REFINE = 2, 16, 14


def build_launches(ns):
    return -(-ns // min(ns, 512)) + 2 * ns + 2


def cyc_solver(s, **opts):
    return Solver(s.asm, batch_continuous=True, batch_continuous_cycles=True,
                  petsc_options=opts or None)


def setup(name, km):
    return Setup(name, km, cycle_direct=True)


# 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,km", CASES_KM)
def test_batched_columns_match_oracle(name, km):
    s = setup(name, km)
    try:
        h = s.asm.handle
        res = cyc_solver(s).solve_many(s.items, s.f)
        info = h.cp_batch_cycles_info()
        print(res.info, info)
        assert res.path == "batched" and res.info["chunk"] == N_SCEN
        assert res.info["fallback"] == 0
        assert info == {"enabled": True, "applied": True, "builds": 1}
        check_columns(s, res)
    finally:
        s.close()


# 2 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,km", [("edge_info_N10", (4, 3)), ("lattice6x6_N3", (2, 1))])
def test_columns_do_not_depend_on_their_batch(name, km):
    s = setup(name, km)
    try:
        solver = cyc_solver(s)
        a = solver.solve_many(s.items, s.f)
        assert a.path == "batched" and a.info["fallback"] == 0
        with env(NXHIP_BATCH=1):  # column 2 alone
            d = solver.solve_many([s.items[2]], s.f[2:3])
            assert d.path == "batched" and d.info["chunk"] == 1
        np.testing.assert_array_equal(d.x[0], a.x[2])
        assert d.residual_norms[0] == a.residual_norms[2]
        c = solver.solve_many(s.items[::-1], s.f[::-1])
        np.testing.assert_array_equal(c.x[::-1], a.x)
        np.testing.assert_array_equal(c.residual_norms[::-1], a.residual_norms)
        with env(NXHIP_BATCH_CHUNK=4):
            b = solver.solve_many(s.items, s.f)
            assert b.path == "batched" and b.info["chunk"] == 4
        np.testing.assert_array_equal(b.x, a.x)
        np.testing.assert_array_equal(b.residual_norms, a.residual_norms)
        extra = [0, 2]  # B = 9: two tiles of 4 and one of 1
        nine = solver.solve_many(s.items + [s.items[j] for j in extra],
                                 np.concatenate([s.f, s.f[extra]]))
        assert nine.path == "batched" and nine.info["chunk"] == 9
        np.testing.assert_array_equal(nine.x[:N_SCEN], a.x)
        np.testing.assert_array_equal(nine.x[N_SCEN:], a.x[extra])
        np.testing.assert_array_equal(nine.residual_norms[:N_SCEN], a.residual_norms)
        assert s.asm.handle.cp_batch_cycles_info()["builds"] == 1
    finally:
        s.close()


# 3 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge_info_N10", "lattice6x6_N3"])
def test_one_pass_not_a_loop(name):
    """The documented launch counts (include/nxhip.h): the same at B = 1 and B = 7 in one
    chunk, growing per chunk only; the build's launches in the first call alone. rtol = 1e-9
    keeps the refinement pass out of the count (the one-pass residual of the model is below
    2e-12 on these graphs, tests/test_cp_batch_cycles_host.py)."""
    s = setup(name, (2, 1))
    try:
        solver = cyc_solver(s, ksp_rtol=1e-9)
        with env(NXHIP_BATCH=1):
            first = solver.solve_many(s.items[:1], s.f[:1])  # (it assembles, and builds)
            one = solver.solve_many(s.items[:1], s.f[:1])
        seven = solver.solve_many(s.items, s.f)
        for r in (first, one, seven):
            print(r.info)
            assert r.path == "batched" and r.info["fallback"] == 0 and r.info["refined"] == 0
        assert seven.info["chunk"] == N_SCEN
        assert one.info["launches"] == seven.info["launches"] == FACTOR + PER_CHUNK
        # (+ 1 only where that assembly was deferred and the call flushed it)
        assert (first.info["launches"] - one.info["launches"] - build_launches(SLOTS[name])
                in (0, 1))
        counts = []
        for chunk, n in ((7, 1), (4, 2), (2, 4)):
            with env(NXHIP_BATCH_CHUNK=chunk):
                r = solver.solve_many(s.items, s.f)
            assert r.info["chunk"] == chunk and r.info["refined"] == 0
            counts.append(r.info["launches"])
            assert r.info["launches"] == FACTOR + n * PER_CHUNK
        assert counts[1] - counts[0] == PER_CHUNK and counts[2] - counts[1] == 2 * PER_CHUNK
    finally:
        s.close()


def _tree_with_chords():
    """A depth-8 binary tree (511 edges; its last node levels hold 128 and 256 nodes) with two
    pairs of leaves joined: a node forest whose up and down passes take more than one launch."""
    G = ng.make_tree(9, 9, 9)
    leaves = sorted(n for n in G.nodes if G.out_degree(n) == 0)
    G.add_edge(leaves[0], leaves[1])
    G.add_edge(leaves[100], leaves[101])
    return G


def test_launch_formula_with_wide_levels(monkeypatch):
    """The '3 (U + D)' term of include/nxhip.h at U + D > 2: F = 1 + U from the first chunk,
    S = 10 + 3 (U + D) from the step between one and two chunks; the columns at the oracle's
    bar. rtol = 1e-9 keeps the refinement pass out of the count."""
    monkeypatch.setitem(CASES, "tree8_chords_N2", (_tree_with_chords, 2, "smallest_last",
                                                   CASES["Y_N4"][3]))
    s = setup("tree8_chords_N2", (2, 1))
    try:
        assert s.mesh.num_edges == 513
        h = s.asm.handle
        solver = cyc_solver(s, ksp_rtol=1e-9)
        solver.solve_many(s.items, s.f)  # (assembles and builds)
        one = solver.solve_many(s.items, s.f)
        with env(NXHIP_BATCH_CHUNK=4):
            two = solver.solve_many(s.items, s.f)
        with env(NXHIP_BATCH_CHUNK=2):
            four = solver.solve_many(s.items, s.f)
        for r in (one, two, four):
            print(r.info)
            assert r.path == "batched" and r.info["refined"] == 0 and r.info["fallback"] == 0
        assert h.cp_batch_cycles_info() == {"enabled": True, "applied": True, "builds": 1}
        S = two.info["launches"] - one.info["launches"]
        F = one.info["launches"] - S
        assert four.info["launches"] == F + 4 * S
        U, ud = F - 1, (S - 10) // 3
        print(f"F {F}, S {S}: U {U}, D {ud - U}")
        assert S == 10 + 3 * ud and ud > 2 and 1 <= U < ud
        check_columns(s, solver.solve_many(s.items, s.f))
    finally:
        s.close()


# 4 ---------------------------------------------------------------------------------------
def test_builds_follow_R_alone():
    s = setup("lattice4x5_N6", (2, 1))
    try:
        solver = cyc_solver(s)
        h = s.asm.handle
        a = solver.solve_many(s.items, s.f)
        b = solver.solve_many(s.items, s.f)
        assert h.cp_batch_cycles_info()["builds"] == 1
        np.testing.assert_array_equal(a.x, b.x)
        steady = FACTOR + PER_CHUNK + (REFINE if b.info["refined"] else 0)
        assert b.info["launches"] == steady
        assert a.info["launches"] - steady - build_launches(SLOTS["lattice4x5_N6"]) in (0, 1)
        # new p_bc / f alone: nothing is built
        s.asm.compute_forms(p_bc_ex=s.items[1], f=0.25, R=s.R)
        c = solver.solve_many(s.items, s.f)
        assert h.cp_batch_cycles_info()["builds"] == 1
        np.testing.assert_array_equal(c.x, a.x)
        # a new R: one more build, the new oracle
        R2 = 2.0 - 0.25 * (np.arange(s.mesh.num_edges) % 4)
        s.asm.compute_forms(p_bc_ex=s.pbc, R=R2)
        res = solver.solve_many(s.items, s.f)
        assert res.path == "batched" and res.info["fallback"] == 0
        assert h.cp_batch_cycles_info() == {"enabled": True, "applied": True, "builds": 2}
        check_columns(s, res, R=R2)
        again = solver.solve_many(s.items, s.f)
        assert h.cp_batch_cycles_info()["builds"] == 2
        np.testing.assert_array_equal(again.x, res.x)
    finally:
        s.close()


# 5 ---------------------------------------------------------------------------------------
def test_handle_left_as_it_was():
    """The batch builds its own inverse on its own factors: the single solve's bits, rhs,
    solution, and its own correction's figures do not move with the batched calls."""
    s = setup("lattice6x6_N3", (3, 2))
    try:
        solver = cyc_solver(s)
        solver.assemble()
        x_first = np.concatenate([f.x.array for f in solver.solve()])
        h = s.asm.handle
        cyc0 = h.cp_cycles()
        assert cyc0 == {"ran": True, "builds": 1}
        rhs0, xd0 = h.rhs(), h.solution()
        for _ in range(2):
            res = solver.solve_many(s.items, s.f)
            assert res.path == "batched" and res.info["fallback"] == 0
            np.testing.assert_array_equal(h.rhs(), rhs0)
            np.testing.assert_array_equal(h.solution(), xd0)
            assert h.cp_cycles() == cyc0
        assert h.cp_batch_cycles_info()["builds"] == 1
        x_after = np.concatenate([f.x.array for f in solver.solve()])
        np.testing.assert_array_equal(x_after, x_first)
        assert h.cp_cycles() == cyc0
        # ... and the other way round: a batched call first, then the single solve, on a fresh
        # handle, gives the same single-solve bits
        t = setup("lattice6x6_N3", (3, 2))
        try:
            other = cyc_solver(t)
            assert other.solve_many(t.items, t.f).path == "batched"
            other.assemble()
            x_other = np.concatenate([f.x.array for f in other.solve()])
            np.testing.assert_array_equal(x_other, x_first)
            assert t.asm.handle.cp_cycles() == cyc0
        finally:
            t.close()
    finally:
        s.close()


# 6 ---------------------------------------------------------------------------------------
def test_conductance_matches_the_loop():
    s = setup("lattice4x5_N6", (2, 1))
    try:
        h = s.asm.handle
        nodes, C = terminal_conductance(cyc_solver(s))
        info = h.batch_info()
        print(info, h.cp_batch_cycles_info())
        assert info["launches"] > 0 and info["chunk"] == min(nodes.size, 64)
        assert info["fallback"] == 0 and h.cp_batch_cycles_info()["applied"]
        cmax = np.abs(C).max()
        assert np.abs(C - C.T).max() <= SOL_TOL * cmax
        assert np.abs(C.sum(axis=0)).max() <= SOL_TOL * cmax
        nodes2, Cloop = terminal_conductance(Solver(s.asm, batch_continuous=True))
        assert not h.cp_batch_cycles_info()["enabled"] and not h.cp_batch_supported()
        np.testing.assert_array_equal(nodes2, nodes)
        assert np.abs(C - Cloop).max() <= SOL_TOL * np.abs(Cloop).max()
    finally:
        s.close()


# 7 ---------------------------------------------------------------------------------------
def test_refinement_and_fallback():
    """tests/test_gpu_cp_batch.py::test_refinement_and_fallback on a graph with cycles:
    rtol = 1e-17 is below what the refinement pass reaches, so the non-zero columns take it and
    then the single-column route (fe_cp_solve with the handle's own correction, MINRES capped
    at ksp_max_it = 20). The solutions stay at the oracle's bar, a second chunk after a
    fallback column is still the oracle's, and the handle's next solve() keeps its bits."""
    s = setup("edge_info_N10", (2, 1))
    try:
        base = cyc_solver(s)
        base.assemble()
        x0 = np.concatenate([f.x.array for f in base.solve()])
        h = s.asm.handle
        rhs0, xd0 = h.rhs(), h.solution()
        pick = [0, ZERO, 5]
        items, f = [s.items[j] for j in pick], s.f[pick]
        tight = cyc_solver(s, ksp_rtol=1e-17, ksp_max_it=20, ksp_error_if_not_converged=False)
        res = tight.solve_many(items, f)
        print(res.info, res.iterations, res.residual_norms, res.converged)
        assert res.path == "batched"
        assert res.info["refined"] == 2 and res.info["fallback"] == 2
        assert res.info["launches"] >= FACTOR + PER_CHUNK + REFINE
        assert not res.x[1].any() and res.converged[1] and res.iterations[1] == 1
        assert res.residual_norms[1] == 0.0
        x_ref = s.oracle()
        for j, kk in ((0, 0), (2, 5)):
            assert rel(res.x[j], x_ref[kk]) <= SOL_TOL
        np.testing.assert_array_equal(h.rhs(), rhs0)
        np.testing.assert_array_equal(h.solution(), xd0)
        np.testing.assert_array_equal(np.concatenate([f.x.array for f in base.solve()]), x0)
        with env(NXHIP_BATCH_CHUNK=2):
            res2 = tight.solve_many(items, f)
        assert res2.info["chunk"] == 2 and res2.info["fallback"] == 2
        assert rel(res2.x[2], x_ref[5]) <= SOL_TOL and rel(res2.x[0], x_ref[0]) <= SOL_TOL
        assert h.cp_batch_cycles_info()["builds"] == 1 and h.cp_batch_supported()
    finally:
        s.close()


# 8 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["alone", "no_cycle_direct", "env", "env_false", "minres"])
def test_switch(kind, monkeypatch):
    monkeypatch.delenv("NXHIP_CP_BATCH_CYCLES", raising=False)
    if kind in ("env", "env_false"):
        monkeypatch.setenv("NXHIP_CP_BATCH_CYCLES", "1")
    s = Setup("edge_info_N10", (2, 1), cycle_direct=kind != "no_cycle_direct")
    try:
        kw = {"alone": dict(batch_continuous_cycles=True),
              "no_cycle_direct": dict(batch_continuous=True, batch_continuous_cycles=True),
              "env": dict(batch_continuous=True),
              "env_false": dict(batch_continuous=True, batch_continuous_cycles=False),
              "minres": dict(batch_continuous=True, batch_continuous_cycles=True,
                             petsc_options={"ksp_type": "minres"})}[kind]
        res = Solver(s.asm, **kw).solve_many(s.items, s.f)
        h = s.asm.handle
        assert res.converged.all()
        if kind == "env":
            assert res.path == "batched" and res.info["fallback"] == 0
            assert h.cp_batch_cycles_info()["applied"]
            check_columns(s, res)
        else:
            assert res.path == "sequential"
            assert h.cp_batch_cycles_info()["builds"] == 0
            assert not h.cp_batch_cycles_info()["applied"]
        if kind == "env_false":
            assert not h.cp_batch_supported() and not h.cp_batch_cycles_info()["enabled"]
    finally:
        s.close()


def test_c_abi():
    s = setup("edge_info_N10", (2, 1))
    try:
        Solver(s.asm, batch_continuous=True)._configure()
        h, L = s.asm.handle, _lib.lib()
        assert h.cp_batch_cycles_info() == {"enabled": False, "applied": False, "builds": 0}
        assert not h.cp_batch_supported()
        h.set_cp_batch_cycles(True)
        assert h.cp_batch_supported() and h.cp_batch_cycles_info()["enabled"]
        h.set_cp_batch_cycles(False)
        assert not h.cp_batch_supported()
        assert L.nx_set_cp_batch_cycles(None, 1) == _lib.NX_ERR_ARG
        assert L.nx_get_cp_batch_cycles(None, None, None, None) == _lib.NX_ERR_ARG
        assert L.nx_set_cp_batch_cycles(h.ptr, 2) == _lib.NX_ERR_ARG
        assert L.nx_get_cp_batch_cycles(h.ptr, None, None, None) == _lib.NX_OK
    finally:
        s.close()
