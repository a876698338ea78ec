"""``Solver(asm, batch_continuous=True).solve_many`` / ``nx_cp_batch_solve``: many boundary and
source scenarios of a continuous-pressure system (k > m >= 1) on a forest in one batched pass of
its node-condensed direct solve -- factored once per call, the right-hand sides swept with a
column dimension -- and ``terminal_conductance`` on top of it.

Scenarios per graph: the 7 columns of tests/test_gpu_batch.py (the case's own p_bc, p_x, a
fixed-seed random nodal array, a unit terminal, an all-zero column, the first two again with
the per-edge source) against the matrix of a per-edge R = 0.5 + (e mod 3) / 2; the shapes of
tests/tree_shapes.py take their own coefficients (``tree_shapes.coefficients``) and ``p_xy``.

Reference: ``oracle.nx_oracle_fe.assemble_reference_fe`` (independently integrated reference
tensors) and one SuperLU factorisation per graph. Tolerances, the project's: every non-zero
column <= 1e-10 relative 2-norm against it (tests/test_gpu_fe.py holds the single solve to it on
the same degrees); the reported true residual <= 1e-12 and within 5 % + 5e-16 of a host
||b - A x|| / ||b|| from the device's CSR (tests/test_gpu_batch.py's bars). The batch has one
refinement pass where the single solve has two: tests/test_cp_batch_host.py holds the numpy
model to 1e-12 after one pass and one refinement on these graphs, so no column may fall back."""

from __future__ import annotations

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from cases import CASES
from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh, Solver, _lib
from networks_fenicsx_amd import network_generation as ng
from networks_fenicsx_amd.layout_fe import evaluate_terms
from networks_fenicsx_amd.post_processing import terminal_conductance
from oracle import nx_oracle as O
from oracle import nx_oracle_fe as OF
from test_gpu_batch import N_SCEN, _graph, edge_R, env, rel, scenarios
from tree_shapes import SHAPES, coefficients, p_xy

pytestmark = pytest.mark.gpu

SOL_TOL = 1e-10
ZERO = 4  # the all-zero column
PAIRS = [(2, 1), (3, 1), (3, 2), (4, 3)]
SMALL = ["demo_tree_N1", "Y_N4", "double_Y_N5", "linear_alt_N3"]
SHAPE_NAMES = ["hub3", "hub5", "hub70", "broom33", "rand200_s1"]
# include/nxhip.h, nx_cp_batch_solve: no level of these node forests holds more than 128 nodes,
# so the forest's up and down passes are one launch each (U = D = 1): the factor stage is
# 1 + U launches, a chunk with its blocks gathered 6 + U + D, a refinement pass 4 + U + D
FACTOR, PER_CHUNK, REFINE = 2, 8, 6


class Setup:
    def __init__(self, name, km, **asm_kw):
        k, m = km
        if name in SHAPES:
            make, N, _ = SHAPES[name]
            strategy, self.pbc = None, p_xy
        else:
            make, N, strategy, self.pbc = _graph(name)
        self.mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
        self.asm = HydraulicNetworkAssembler(self.mesh, flux_degree=k, pressure_degree=m,
                                             **asm_kw)
        E = self.mesh.num_edges
        if name in SHAPES:  # the shape's own coefficients (none: R = 1, f = 0)
            coef = coefficients(name, E)
            self.R = np.asarray(coef.get("R", np.ones(E)), dtype=np.float64)
            self.asm.compute_forms(p_bc_ex=self.pbc, R=self.R, **({"f": coef["f"]} if coef else {}))
        else:
            self.R = edge_R(self.mesh)
            self.asm.compute_forms(p_bc_ex=self.pbc, R=self.R)
        src, dst = self.mesh.edges
        self.F = OF.build_problem_fe(self.mesh.node_coordinates, src, dst, N, k, m,
                                     self.mesh.edge_colors)
        self.items, self.nodal, self.f = scenarios(self.mesh, self.pbc)
        self._ref = {}

    def oracle(self, R=None):
        """Reference solutions (7, n) in the reference block order; one LU per R."""
        R = self.R if R is None else R
        key = np.asarray(R, dtype=np.float64).tobytes()
        if key not in self._ref:
            A, bs = None, []
            for j in range(N_SCEN):
                A, b = OF.assemble_reference_fe(self.F, self.nodal[j], f=self.f[j], R=R)
                bs.append(b)
            lu = spla.splu(A.tocsc())
            self._ref[key] = np.stack([lu.solve(b) for b in bs])
        return self._ref[key]

    def close(self):
        self.asm.close()


def device_columns(s, res):
    """res.x (block order) in the device layout."""
    xdev = np.empty_like(res.x)
    xdev[:, s.asm.block_order_rows()] = res.x
    return xdev


def check_columns(s, res, R=None):
    """The oracle bar, the residual's bars, the zero column; no other column skipped."""
    x_ref = s.oracle(R)
    h = s.asm.handle
    rp, col, val = h.csr()
    Adev = sp.csr_matrix((val, col, rp), shape=(h.n_rows, h.n_cols))
    bc, ef, fc = s.asm.scenario_coefficients(s.items, s.f)
    bdev = h.cp_batch_rhs(bc, ef, fc)
    xdev = device_columns(s, res)
    assert res.x.shape == x_ref.shape
    for j in range(N_SCEN):
        if j == ZERO:
            assert not res.x[j].any() and res.residual_norms[j] == 0.0 and res.converged[j]
            continue
        assert np.linalg.norm(x_ref[j]) > 0
        e = rel(res.x[j], x_ref[j])
        host = np.linalg.norm(bdev[j] - Adev @ xdev[j]) / np.linalg.norm(bdev[j])
        print(f"column {j}: vs oracle {e:.3e}, relres {res.residual_norms[j]:.3e}, "
              f"host {host:.3e}, iterations {res.iterations[j]}")
        assert e <= SOL_TOL, (j, e)
        assert res.converged[j] and res.residual_norms[j] <= 1e-12
        assert abs(res.residual_norms[j] - host) <= 0.05 * host + 5e-16, (j, host)


# 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("km", [(2, 1), (3, 2)])
@pytest.mark.parametrize("struct", ["1", "0"])  # the edge templates (default) / the gather tables
def test_rhs_bit_exact(km, struct, monkeypatch):
    """nx_cp_batch_rhs column j == evaluate_terms on the host == h.rhs() after compute_forms +
    assemble of scenario j."""
    monkeypatch.setenv("NXHIP_FE_STRUCT", struct)
    s = Setup("Y_N4", km)
    try:
        asm, h = s.asm, s.asm.handle
        Solver(asm, batch_continuous=True)._configure()
        assert h.cp_batch_supported() and not h.batch_supported()
        assert not h.fe_batch_supported()
        bc, ef, fc = asm.scenario_coefficients(s.items, s.f)
        got = h.cp_batch_rhs(bc, ef, fc)
        _, hcell = O.cell_geometry(s.F.base)
        for j in range(N_SCEN):
            _, hr = evaluate_terms(asm.fe_layout, s.R, s.f[j], bc[j], hcell)
            np.testing.assert_array_equal(got[j], hr)
        for j in range(N_SCEN):
            asm.compute_forms(p_bc_ex=s.items[j], f=s.f[j] if s.f[j].any() else 0.0, R=s.R)
            asm.assemble()
            np.testing.assert_array_equal(got[j], h.rhs())
        # neither edge_f nor f_const: the handle's source (now the last scenario's)
        np.testing.assert_array_equal(h.cp_batch_rhs(bc[N_SCEN - 1:])[0], h.rhs())
    finally:
        s.close()


# 2 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize(
    "name,km",
    [(n, km) for n in SMALL for km in PAIRS] + [("depth6_N40", (2, 1)), ("depth6_N40", (4, 3))]
    + [(n, km) for n in SHAPE_NAMES for km in ((2, 1), (3, 2))])
def test_batched_columns_match_oracle(name, km):
    """N = 1 (both pressures of the one cell are border values), alternating edge directions
    on twelve one-node levels, a partly empty last wave and long edges (depth6_N40: 127 edges),
    a record exactly full (hub3), past the record caps (hub5, hub70, broom33: the lists), a
    random tree with hubs."""
    s = Setup(name, km)
    try:
        res = Solver(s.asm, batch_continuous=True).solve_many(s.items, s.f)
        print(res.info)
        assert res.path == "batched" and res.info["chunk"] == N_SCEN
        assert res.info["fallback"] == 0
        check_columns(s, res)
        fns = res.functions(2)  # scatter_solution's split of column 2
        np.testing.assert_array_equal(np.concatenate([f.x.array for f in fns]), res.x[2])
    finally:
        s.close()


def test_wide_level_without_records(monkeypatch):
    """Without node records (NXHIP_CP_NOREC) every node reads the lists, and a level of more
    than 2048 nodes goes to a grid launch (k_cp_b_level): a depth-12 binary tree, N = 2, whose
    last two levels hold 2048 and 4096 nodes."""
    monkeypatch.setenv("NXHIP_CP_NOREC", "1")
    monkeypatch.setitem(CASES, "depth12_N2", (lambda: ng.make_tree(13, 13, 13), 2,
                                             "smallest_last", CASES["Y_N4"][3]))
    s = Setup("depth12_N2", (2, 1))
    try:
        assert s.mesh.num_edges == 8191
        res = Solver(s.asm, batch_continuous=True).solve_many(s.items, s.f)
        print(res.info)
        assert res.path == "batched" and res.info["fallback"] == 0
        # the factor stage and the chunk's two passes each launch more than one run of levels
        assert res.info["launches"] > FACTOR + PER_CHUNK + (REFINE if res.info["refined"] else 0)
        check_columns(s, res)
    finally:
        s.close()


# 3 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,km", [("depth6_N40", (2, 1)), ("hub5", (3, 2))])
def test_columns_do_not_depend_on_their_batch(name, km):
    s = Setup(name, km)
    try:
        solver = Solver(s.asm, batch_continuous=True)
        a = solver.solve_many(s.items, s.f)
        assert a.path == "batched"
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
        # B = 9: a tile of 8 and one more (two tiles of 4 and one of 1)
        extra = [0, 2]
        nine = solver.solve_many(s.items + [s.items[j] for j in extra],
                                 np.concatenate([s.f, s.f[extra]]))
        assert nine.path == "batched" and nine.info["chunk"] == 9
        np.testing.assert_array_equal(nine.x[:N_SCEN], a.x)
        np.testing.assert_array_equal(nine.x[N_SCEN:], a.x[extra])
        np.testing.assert_array_equal(nine.residual_norms[:N_SCEN], a.residual_norms)
    finally:
        s.close()


# 4 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Y_N4", "depth6_N40"])
def test_one_pass_not_a_loop(name):
    """The documented launch counts (include/nxhip.h): the factor stage once per call, then
    the same count per chunk whatever its columns. rtol = 1e-9 keeps the refinement pass out of
    the count: the one-pass residual is below 1e-11 (tests/test_cp_batch_host.py's bar)."""
    s = Setup(name, (2, 1))
    try:
        solver = Solver(s.asm, batch_continuous=True, petsc_options={"ksp_rtol": 1e-9})
        with env(NXHIP_BATCH=1):
            first = solver.solve_many(s.items[:1], s.f[:1])  # (it assembles the matrix)
            one = solver.solve_many(s.items[:1], s.f[:1])
        seven = solver.solve_many(s.items, s.f)
        for r in (first, one, seven):
            print(r.info)
            assert r.path == "batched" and r.info["fallback"] == 0 and r.info["refined"] == 0
        assert seven.info["chunk"] == N_SCEN
        assert one.info["launches"] == seven.info["launches"] == FACTOR + PER_CHUNK
        # (+ 1 only where that assembly was deferred and the call flushed it)
        assert first.info["launches"] - one.info["launches"] in (0, 1)
        counts = []
        for chunk, n in ((7, 1), (4, 2), (2, 4)):
            with env(NXHIP_BATCH_CHUNK=chunk):
                r = solver.solve_many(s.items, s.f)
            assert r.info["chunk"] == chunk and r.info["refined"] == 0
            counts.append(r.info["launches"])
            assert r.info["launches"] == FACTOR + n * PER_CHUNK
        step = counts[1] - counts[0]
        assert step == PER_CHUNK > 0 and counts[2] - counts[1] == 2 * step
        assert counts[0] - step == FACTOR
    finally:
        s.close()


# 5 ---------------------------------------------------------------------------------------
def test_handle_untouched_and_new_R():
    s = Setup("depth6_N40", (2, 1))
    try:
        solver = Solver(s.asm, batch_continuous=True)
        solver.assemble()
        x_first = np.concatenate([f.x.array for f in solver.solve()])
        h = s.asm.handle
        rhs_before, xdev_before = h.rhs(), h.solution()
        res = solver.solve_many(s.items, s.f)
        assert res.path == "batched"
        np.testing.assert_array_equal(h.rhs(), rhs_before)
        np.testing.assert_array_equal(h.solution(), xdev_before)
        x_after = np.concatenate([f.x.array for f in solver.solve()])
        np.testing.assert_array_equal(x_after, x_first)
        # a new R: the next solve_many assembles the matrix itself, factors again and meets the
        # new oracle; a further call gives the same bits
        R2 = 2.0 - 0.25 * (np.arange(s.mesh.num_edges) % 4)
        s.asm.compute_forms(p_bc_ex=s.pbc, R=R2)
        res = solver.solve_many(s.items, s.f)
        assert res.path == "batched" and res.info["fallback"] == 0
        check_columns(s, res, R=R2)
        again = solver.solve_many(s.items, s.f)
        assert again.path == "batched" and again.info["fallback"] == 0
        check_columns(s, again, R=R2)
        np.testing.assert_array_equal(again.x, res.x)
        steady = FACTOR + PER_CHUNK + (REFINE if again.info["refined"] else 0)
        assert again.info["launches"] == steady
        assert again.info["refined"] == res.info["refined"]
        assert res.info["launches"] - steady in (0, 1)  # (a deferred assembly it flushed)
    finally:
        s.close()


# 6 ---------------------------------------------------------------------------------------
def test_refinement_and_fallback():
    """rtol = 1e-17 is below what the refinement pass reaches: the non-zero columns take it and
    then the single-column route (fe_cp_solve on the handle's own arrays, MINRES capped at
    ksp_max_it = 20); the zero column does neither. The solutions stay at the oracle's bar, the
    handle as before -- and the batch's factors intact: the column after a fallback column in
    the same chunk is still the oracle's."""
    s = Setup("double_Y_N5", (2, 1))
    try:
        base = Solver(s.asm, batch_continuous=True)
        base.assemble()
        x0 = np.concatenate([f.x.array for f in base.solve()])
        h = s.asm.handle
        rhs0, xd0 = h.rhs(), h.solution()
        pick = [0, ZERO, 5]
        items, f = [s.items[j] for j in pick], s.f[pick]
        tight = Solver(s.asm, batch_continuous=True,
                       petsc_options={"ksp_rtol": 1e-17, "ksp_max_it": 20,
                                      "ksp_error_if_not_converged": False})
        res = tight.solve_many(items, f)
        print(res.info, res.iterations, res.residual_norms, res.converged)
        assert res.path == "batched"
        assert res.info["refined"] == 2 and res.info["fallback"] == 2
        assert not res.x[1].any() and res.converged[1] and res.iterations[1] == 1
        assert res.residual_norms[1] == 0.0
        x_ref = s.oracle()
        for j, kk in ((0, 0), (2, 5)):
            assert rel(res.x[j], x_ref[kk]) <= SOL_TOL
        np.testing.assert_array_equal(h.rhs(), rhs0)
        np.testing.assert_array_equal(h.solution(), xd0)
        np.testing.assert_array_equal(np.concatenate([f.x.array for f in base.solve()]), x0)
        # two chunks, a fallback column in the first: the second chunk sweeps on the call's
        # factors after fe_cp_solve ran on the handle's
        with env(NXHIP_BATCH_CHUNK=2):
            res2 = tight.solve_many(items, f)
        assert res2.info["chunk"] == 2 and res2.info["fallback"] == 2
        assert rel(res2.x[2], x_ref[5]) <= SOL_TOL and rel(res2.x[0], x_ref[0]) <= SOL_TOL
    finally:
        s.close()


# 7 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["off", "degrees_only", "minres", "env0", "cycles"])
def test_where_it_must_not_engage(kind):
    if kind == "cycles":
        s = Setup("edge_info_N10", (2, 1), cycle_direct=True)
    else:
        s = Setup("Y_N4", (2, 1))
    try:
        opts = {"ksp_type": "minres"} if kind == "minres" else None
        kw = {"off": {}, "degrees_only": {"batch_degrees": True}}.get(
            kind, {"batch_continuous": True})
        solver = Solver(s.asm, petsc_options=opts, **kw)
        with env(NXHIP_BATCH="0" if kind == "env0" else ""):
            res = solver.solve_many(s.items, s.f)
        assert res.path == "sequential" and res.converged.all()
        if kind == "cycles":
            assert not s.asm.handle.cp_batch_supported()
    finally:
        s.close()


# 8 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("degrees", [(2, 0), (1, 0)])
def test_refused_handles(degrees):
    make, N, strategy, pbc = _graph("Y_N4")
    mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
    asm = HydraulicNetworkAssembler(mesh, flux_degree=degrees[0], pressure_degree=degrees[1])
    try:
        asm.compute_forms(p_bc_ex=pbc)
        solver = Solver(asm, batch_continuous=True)
        solver.assemble()
        solver.solve()
        h = asm.handle
        assert not h.cp_batch_supported()
        items, _, f = scenarios(mesh, pbc)
        bc, ef, fc = asm.scenario_coefficients(items, f)
        with pytest.raises(_lib.NxError, match=f"libnxhip error {_lib.NX_ERR_STATE}:.*"
                                               "nx_cp_batch_supported"):
            h.cp_batch_solve(bc, ef, fc)
        with pytest.raises(_lib.NxError, match="nx_cp_batch_supported"):
            h.cp_batch_rhs(bc, ef, fc)
        # (the option changes nothing for these degrees)
        assert solver.solve_many(items, f).path == ("batched" if degrees == (1, 0)
                                                    else "sequential")
    finally:
        asm.close()


# 9 ---------------------------------------------------------------------------------------
def test_conductance_matches_oracle_and_resistor_network():
    s = Setup("depth6_N40", (2, 1))
    try:
        h = s.asm.handle
        nodes, C = terminal_conductance(Solver(s.asm, batch_continuous=True))
        info = h.batch_info()
        print(info)
        assert info["launches"] > 0 and info["chunk"] == min(nodes.size, 64)
        assert info["fallback"] == 0
        cmax = np.abs(C).max()
        assert np.abs(C - C.T).max() <= 1e-10 * cmax
        assert np.abs(C.sum(axis=0)).max() <= 1e-10 * cmax
        src, dst = s.mesh.edges
        k, N = 2, s.mesh.N
        Cref = np.empty_like(C)
        lu = None
        for t, nt in enumerate(nodes):
            pbc = np.zeros(s.mesh.num_nodes)
            pbc[nt] = 1.0
            A, b = OF.assemble_reference_fe(s.F, pbc, f=0.0, R=s.R)
            lu = lu or spla.splu(A.tocsc())
            x = lu.solve(b)
            for i, ns in enumerate(nodes):
                e_t, e_s = np.flatnonzero(dst == ns), np.flatnonzero(src == ns)
                Cref[i, t] = (x[s.F.flux_offset[e_t[0]] + k * N] if e_t.size
                              else -x[s.F.flux_offset[e_s[0]]])
        assert np.abs(C - Cref).max() <= 1e-10 * np.abs(Cref).max()
        # the resistor network: edge conductances 1 / (R_e L_e), the graph Laplacian's Schur
        # complement onto the terminals (f = 0: the exact solution lies in the discrete spaces)
        Cnet = resistor_schur(s.mesh, s.R, nodes)
        assert np.abs(C - Cnet).max() <= 1e-10 * np.abs(Cnet).max()
    finally:
        s.close()


def resistor_schur(mesh, R, nodes):
    """``terminal_conductance``'s matrix from the resistor network: with the graph Laplacian L
    of the conductances 1 / (R_e L_e), the terminals T and the other nodes I,
    L_TT - L_TI L_II^-1 L_IT in the order of ``nodes``."""
    src, dst = mesh.edges
    pos = np.asarray(mesh.node_coordinates, dtype=np.float64)
    g = 1.0 / (np.asarray(R) * np.linalg.norm(pos[dst] - pos[src], axis=1))
    n = mesh.num_nodes
    L = np.zeros((n, n))
    for e in range(src.size):
        a, b = int(src[e]), int(dst[e])
        L[a, a] += g[e]
        L[b, b] += g[e]
        L[a, b] -= g[e]
        L[b, a] -= g[e]
    T = np.asarray(nodes, dtype=np.int64)
    inner = np.setdiff1d(np.arange(n), T)
    return L[np.ix_(T, T)] - L[np.ix_(T, inner)] @ np.linalg.solve(L[np.ix_(inner, inner)],
                                                                  L[np.ix_(inner, T)])
