"""``Solver(asm, batch_degrees=True).solve_many`` / ``nx_fe_batch_solve``: many boundary and
source scenarios of a flux-degree-k / DG0 system in one batched pass of its condensed direct
solve, and ``terminal_conductance`` on top of it.

Scenarios per graph: the 7 columns of tests/test_gpu_batch.py (the case's own p_bc, p_x, a
fixed-seed random nodal array, a unit terminal, an all-zero column, the first two again with
the per-edge source) against the matrix of a per-edge R = 0.5 + (e mod 3) / 2.

Reference: ``oracle.nx_oracle_fe.assemble_reference_fe`` (independently integrated reference
tensors) and one SuperLU factorisation per graph. Tolerances: every non-zero column <= 1e-10
relative 2-norm against it -- the project's bar, held by the single solve on the same graphs
and degrees (tests/test_gpu_fe.py::test_fe_direct_condensed); the reported true residual
<= 1e-12 and within 5 % + 5e-16 of a host ||b - A x|| / ||b|| from the device's CSR
(tests/test_gpu_batch.py's bars)."""

from __future__ import annotations

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from cases import CYCLIC
from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh, Solver, _lib
from networks_fenicsx_amd.layout_fe import evaluate_terms
from networks_fenicsx_amd.post_processing import terminal_conductance
from oracle import nx_oracle as O
from oracle import nx_oracle_fe as OF
from test_gpu_batch import N_SCEN, _graph, edge_R, env, rel, scenarios

pytestmark = pytest.mark.gpu

SOL_TOL = 1e-10
ZERO = 4  # the all-zero column


class Setup:
    def __init__(self, name, k, m=0, R="edge"):
        make, N, strategy, self.pbc = _graph(name)
        self.mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
        self.asm = HydraulicNetworkAssembler(self.mesh, flux_degree=k, pressure_degree=m)
        self.R = edge_R(self.mesh) if isinstance(R, str) else R
        self.asm.compute_forms(p_bc_ex=self.pbc, R=self.R)
        src, dst = self.mesh.edges
        self.F = OF.build_problem_fe(self.mesh.node_coordinates, src, dst, N, k, m,
                                     self.mesh.edge_colors)
        self.items, self.nodal, self.f = scenarios(self.mesh, self.pbc)
        self.cyclic = name in CYCLIC
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

    @property
    def jobs(self):
        return int(self.asm._fe_aux_pc.n_jobs)

    def close(self):
        self.asm.close()


def steady_launches(s, info, chunks=1):
    """The documented launches (include/nxhip.h, nx_fe_batch_solve) of a call that found
    everything current, blocks gathered: per chunk rhs, condense, [up,] top, [down,] expand,
    residual, norms, gather and the cycle correction's two kernels; a refinement pass adds
    condense, the sweeps (and the two), expand, residual and norms."""
    sweeps = 3 if s.jobs > 0 else 1
    cyc = 2 if s.cyclic else 0
    per = 6 + sweeps + cyc
    ref = (4 + sweeps + cyc) if info["refined"] else 0
    return chunks * per + ref


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
    bdev = h.fe_batch_rhs(bc, ef, fc)
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
@pytest.mark.parametrize("name", ["Y_N4", "edge_info_N10"])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("struct", ["1", "0"])  # the edge templates (default) / the gather tables
def test_rhs_bit_exact(name, k, struct, monkeypatch):
    """nx_fe_batch_rhs column j == evaluate_terms on the host == h.rhs() after compute_forms +
    assemble of scenario j."""
    monkeypatch.setenv("NXHIP_FE_STRUCT", struct)
    s = Setup(name, k)
    try:
        asm, h = s.asm, s.asm.handle
        Solver(asm, batch_degrees=True)._configure()
        assert h.fe_batch_supported() and not h.batch_supported()
        bc, ef, fc = asm.scenario_coefficients(s.items, s.f)
        got = h.fe_batch_rhs(bc, ef, fc)
        _, hcell = O.cell_geometry(s.F.base)
        for j in range(N_SCEN):
            _, hr = evaluate_terms(asm.fe_layout, s.R, s.f[j], bc[j], hcell)
            np.testing.assert_array_equal(got[j], hr)
        # scalars per column, and the handle's own source (None)
        fs = np.linspace(-0.5, 1.0, N_SCEN)
        got_c = h.fe_batch_rhs(bc, None, fs)
        for j in (0, 3, 6):
            _, hr = evaluate_terms(asm.fe_layout, s.R, float(fs[j]), bc[j], hcell)
            np.testing.assert_array_equal(got_c[j], hr)
        for j in range(N_SCEN):
            asm.compute_forms(p_bc_ex=s.items[j], f=s.f[j] if s.f[j].any() else 0.0, R=s.R)
            asm.assemble()
            np.testing.assert_array_equal(got[j], h.rhs())
        # neither edge_f nor f_const: the handle's source (now the last scenario's)
        np.testing.assert_array_equal(h.fe_batch_rhs(bc[N_SCEN - 1:])[0], h.rhs())
    finally:
        s.close()


# 2 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("Y_N4", 2), ("Y_N4", 3), ("Y_N4", 4), ("double_Y_N5", 2),
                                    ("double_Y_N5", 3), ("double_Y_N5", 4), ("depth6_N40", 2),
                                    ("tree6_2d_N70", 2)])
def test_batched_columns_match_oracle(name, k):
    """One subtree job (Y_N4), several, several cells per lane (depth6_N40), N >= 64."""
    s = Setup(name, k)
    try:
        res = Solver(s.asm, batch_degrees=True).solve_many(s.items, s.f)
        assert res.path == "batched" and res.info["chunk"] == N_SCEN
        assert res.info["fallback"] == 0
        check_columns(s, res)
        fns = res.functions(2)  # scatter_solution's split of column 2
        np.testing.assert_array_equal(np.concatenate([f.x.array for f in fns]), res.x[2])
    finally:
        s.close()


# 3 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge_info_N10", "lattice4x5_N6"])
def test_batched_cycles(name):
    """2 and 12 cycle chains. The first call after compute_forms assembles the matrix and
    builds the auxiliary correction itself; the second reports the steady launches alone and
    the same bits; a later solve() still meets the bar."""
    s = Setup(name, 2)
    try:
        solver = Solver(s.asm, batch_degrees=True)
        res = solver.solve_many(s.items, s.f)
        assert res.path == "batched" and res.info["fallback"] == 0
        check_columns(s, res)
        res2 = solver.solve_many(s.items, s.f)
        np.testing.assert_array_equal(res2.x, res.x)
        m = np.asarray(s.asm._fe_aux_pc.cyc_rows).size
        assert m in (4, 24)
        steady = steady_launches(s, res2.info)
        print(f"launches: first {res.info['launches']}, second {res2.info['launches']}, m {m}")
        assert res2.info["launches"] == steady
        assert res2.info["refined"] == res.info["refined"]
        assert res.info["launches"] >= steady + 1 + 4 * m + 3
        solver.assemble()
        sol = np.concatenate([f.x.array for f in solver.solve()])
        assert rel(sol, s.oracle()[0]) <= SOL_TOL
    finally:
        s.close()


# 4 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["depth6_N40", "edge_info_N10"])
def test_columns_do_not_depend_on_their_batch(name):
    s = Setup(name, 2)
    try:
        solver = Solver(s.asm, batch_degrees=True)
        a = solver.solve_many(s.items, s.f)
        assert a.path == "batched"
        with env(NXHIP_BATCH_CHUNK=2):
            b = solver.solve_many(s.items, s.f)
            assert b.path == "batched" and b.info["chunk"] == 2
        c = solver.solve_many(s.items[::-1], s.f[::-1])
        with env(NXHIP_BATCH=1):
            for j in range(N_SCEN):
                d = solver.solve_many([s.items[j]], s.f[j:j + 1])
                assert d.path == "batched"
                np.testing.assert_array_equal(d.x[0], a.x[j])
                assert d.residual_norms[0] == a.residual_norms[j]
        np.testing.assert_array_equal(b.x, a.x)
        np.testing.assert_array_equal(c.x[::-1], a.x)
        np.testing.assert_array_equal(b.residual_norms, a.residual_norms)
        np.testing.assert_array_equal(c.residual_norms[::-1], a.residual_norms)
    finally:
        s.close()


# 5 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["depth6_N40", "Y_N4"])
def test_one_pass_not_a_loop(name):
    """The documented launch counts: 9 per chunk on a forest (both graphs have subtree jobs),
    + 7 for a chunk with a refinement pass; the same for B = 1, 5, 7; two chunks: twice."""
    s = Setup(name, 2)
    try:
        solver = Solver(s.asm, batch_degrees=True)
        with env(NXHIP_BATCH=1):
            first = solver.solve_many(s.items[:1], s.f[:1])  # (it assembles the matrix)
            one = solver.solve_many(s.items[:1], s.f[:1])
        five = solver.solve_many(s.items[:5], s.f[:5])
        seven = solver.solve_many(s.items, s.f)
        per = 9 if s.jobs > 0 else 7
        assert s.jobs >= 1 and (name != "Y_N4" or s.jobs == 1)  # (Y_N4: one up / down workgroup)
        for r in (first, one, five, seven):
            assert r.path == "batched" and r.info["fallback"] == 0
            print(r.info)
        assert one.info["launches"] == per + ((per - 2) if one.info["refined"] else 0)
        assert one.info["launches"] == steady_launches(s, one.info)
        # (+ 1 only where that assembly was deferred and the call flushed it)
        assert first.info["launches"] - steady_launches(s, first.info) in (0, 1)
        assert five.info["launches"] == steady_launches(s, five.info)
        assert seven.info["launches"] == steady_launches(s, seven.info)
        if not (one.info["refined"] or five.info["refined"] or seven.info["refined"]):
            assert one.info["launches"] == five.info["launches"] == seven.info["launches"] == per
        with env(NXHIP_BATCH_CHUNK=3):
            six = solver.solve_many(s.items[:6], s.f[:6])
        assert six.info["chunk"] == 3 and six.info["fallback"] == 0
        if not six.info["refined"]:
            assert six.info["launches"] == 2 * per
        else:  # (one or both chunks took a refinement pass)
            assert six.info["launches"] in (2 * per + (per - 2), 2 * per + 2 * (per - 2))
    finally:
        s.close()


# 6 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["depth6_N40", "edge_info_N10"])
def test_handle_untouched_and_new_R(name):
    s = Setup(name, 2)
    try:
        solver = Solver(s.asm, batch_degrees=True)
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
        # a new R: the next solve_many assembles the matrix itself, rebuilds the auxiliary mass
        # (and the correction) and meets the new oracle; a further call rebuilds nothing
        R2 = 2.0 - 0.25 * (np.arange(s.mesh.num_edges) % 4)
        s.asm.compute_forms(p_bc_ex=s.pbc, R=R2)
        res = solver.solve_many(s.items, s.f)
        assert res.path == "batched" and res.info["fallback"] == 0
        check_columns(s, res, R=R2)
        again = solver.solve_many(s.items, s.f)
        np.testing.assert_array_equal(again.x, res.x)
        steady = steady_launches(s, again.info)
        assert again.info["launches"] == steady
        assert again.info["refined"] == res.info["refined"]
        if s.cyclic:
            m = np.asarray(s.asm._fe_aux_pc.cyc_rows).size
            assert res.info["launches"] >= steady + 1 + 4 * m + 3
        else:  # (+ 1 only where the assembly was deferred and the call flushed it)
            assert res.info["launches"] - steady in (0, 1)
    finally:
        s.close()


# 7 ---------------------------------------------------------------------------------------
def test_refinement_and_fallback():
    """rtol = 1e-17 is below what the refinement pass reaches: the non-zero columns take it and
    then the single-column route (fe_solve_direct, MINRES capped at ksp_max_it = 20, which ends
    unconverged and worse: the refined column stands); the zero column does neither. The
    solutions stay at the oracle's bar, the handle as before."""
    s = Setup("double_Y_N5", 2)
    try:
        base = Solver(s.asm, batch_degrees=True)
        base.assemble()
        x0 = np.concatenate([f.x.array for f in base.solve()])
        h = s.asm.handle
        rhs0, xd0 = h.rhs(), h.solution()
        pick = [0, ZERO, 5]
        items, f = [s.items[j] for j in pick], s.f[pick]
        tight = Solver(s.asm, batch_degrees=True,
                       petsc_options={"ksp_rtol": 1e-17, "ksp_max_it": 20,
                                      "ksp_error_if_not_converged": False})
        res = tight.solve_many(items, f)
        print(res.info, res.iterations, res.residual_norms, res.converged)
        assert res.path == "batched"
        assert res.info["refined"] == int((res.iterations != 1).sum())
        assert not res.x[1].any() and res.converged[1] and res.iterations[1] == 1
        assert res.residual_norms[1] == 0.0
        if res.residual_norms.any():
            assert res.info["fallback"] >= 1
        x_ref = s.oracle()
        for j, kk in ((0, 0), (2, 5)):
            assert rel(res.x[j], x_ref[kk]) <= SOL_TOL
        np.testing.assert_array_equal(h.rhs(), rhs0)
        np.testing.assert_array_equal(h.solution(), xd0)
        np.testing.assert_array_equal(np.concatenate([f.x.array for f in base.solve()]), x0)
    finally:
        s.close()


# 8 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["off", "fe21", "minres", "env0"])
def test_where_it_must_not_engage(kind):
    m = 1 if kind == "fe21" else 0
    s = Setup("Y_N4", 2, m=m)
    try:
        opts = {"ksp_type": "minres"} if kind == "minres" else None
        solver = Solver(s.asm, petsc_options=opts, batch_degrees=kind != "off")
        with env(NXHIP_BATCH="0" if kind == "env0" else ""):
            res = solver.solve_many(s.items, s.f)
        assert res.path == "sequential" and res.converged.all()
    finally:
        s.close()


def test_p1_handle_is_refused():
    make, N, strategy, pbc = _graph("Y_N4")
    mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
    asm = HydraulicNetworkAssembler(mesh)
    try:
        asm.compute_forms(p_bc_ex=pbc)
        solver = Solver(asm, batch_degrees=True)
        solver.assemble()
        solver.solve()
        h = asm.handle
        assert not h.fe_batch_supported()
        items, _, f = scenarios(mesh, pbc)
        bc, ef, fc = asm.scenario_coefficients(items, f)
        with pytest.raises(_lib.NxError, match=f"libnxhip error {_lib.NX_ERR_STATE}:"):
            h.fe_batch_solve(bc, ef, fc)
        assert solver.solve_many(items, f).path == "batched"  # (nx_batch_solve, as before)
    finally:
        asm.close()


# 9 ---------------------------------------------------------------------------------------
def test_conductance_matches_oracle():
    s = Setup("depth6_N40", 2)
    try:
        h = s.asm.handle
        nodes, C = terminal_conductance(Solver(s.asm, batch_degrees=True))
        info = h.batch_info()
        print(info)
        assert info["launches"] > 0 and info["chunk"] == min(nodes.size, 64)
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
    finally:
        s.close()
