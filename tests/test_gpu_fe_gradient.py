"""``Solver(asm, batch_degrees=True).gradient`` / ``nx_fe_batch_gradient``: adjoint gradients of
an observed-row objective for flux degree k >= 2 with DG0 pressure, in two batched passes of the
condensed direct solve and one contraction with the degree-k element mass.

Set-up per graph (tests/test_gpu_gradient.py's with ``flux_degree=k, pressure_degree=0``):
per-edge R = 0.5 + (e mod 3) / 2; B = 3 scenarios -- the case's own p_bc, p_x and a fixed-seed
random nodal array -- each with the per-edge source f = 0.1 + 0.02 (e mod 5); about 12 observed
rows drawn from the vertex-flux, the INTERIOR-flux, the pressure and the multiplier rows (a
wrong sign or a wrong row map on a block is an O(1) error), weights in [0.5, 1.5); both kinds of
objective (linear, and least squares against random data).

Yardstick: the CPU adjoint of tests/gradient_ref_fe.py (SuperLU on the oracle's A and A^T,
itself held to central finite differences in tests/test_gradient_ref_fe.py). ``value``, ``dR``,
``df`` and ``dp_bc`` of every scenario are compared as relative 2-norms.

The parity bar: each figure is a product of two solves held to 1e-10 each, so the bar is set
from a measurement -- 10x the largest error over all the cases below on an MI355X (margin for
machine-to-machine rounding of the sweeps' order), and never above 1e-8 (any formula or sign
error is O(1)). Measured worst figure per case (both kinds, all scenarios and quantities):
demo_tree_N1 k=2 3.0e-15, Y_N4 k=2 5.0e-15, Y_N4 k=3 4.6e-15, Y_N4 k=4 1.2e-14, tree5_N15 k=2
2.0e-14, tree5_N16 k=2 3.9e-14, tree5_3d_N31 k=3 7.2e-14, tree6_2d_N70 k=2 5.1e-13, depth6_N40
k=2 3.1e-13, edge_info_N10 k=2 1.4e-13, lattice6x6_N3 k=2 1.4e-14; the largest is
PARITY_MEASURED = 5.110e-13, the bar 5.2e-12."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from cases import CYCLIC
from gradient_ref_fe import AdjointRefFe, objective
from networks_fenicsx_amd import Solver, _lib
from oracle import nx_oracle_fe as OF
from test_gpu_gradient import Setup as P1Setup
from test_gpu_gradient import assert_same_bits, env, rel

pytestmark = pytest.mark.gpu

PARITY_MEASURED = 5.110e-13  # the largest error over test_parity_with_cpu_adjoint's cases
PARITY_BAR = 5.2e-12  # 10 x PARITY_MEASURED (rounded up); may never exceed 1e-8
assert 10 * PARITY_MEASURED <= PARITY_BAR <= 1e-8

# (case, k): why it is there
PARITY_CASES = [("demo_tree_N1", 2),   # one cell per edge, no neighbour lane
                ("Y_N4", 2), ("Y_N4", 3), ("Y_N4", 4),  # a hard-coded k or mass size
                ("tree5_N15", 2), ("tree5_N16", 2),  # the 16-lane / 32-lane segment boundary
                ("tree5_3d_N31", 3),   # the last 32-lane segment
                ("tree6_2d_N70", 2),   # two 64-cell chunks per wave
                ("depth6_N40", 2),     # auxiliary subtree jobs: several
                ("edge_info_N10", 2), ("lattice6x6_N3", 2)]  # cycles: the adjoint's correction


class Setup(P1Setup):
    """tests/test_gpu_gradient.py's set-up at degrees (k, 0): the same R, scenarios and
    sources; the oracle's (k, 0) problem; rows from all four kinds of row."""

    def __init__(self, name, k, **asm_kw):
        super().__init__(name, flux_degree=k, pressure_degree=0, **asm_kw)
        self.k = k
        src, dst = self.mesh.edges
        N = self.mesh.N
        self.F = F = OF.build_problem_fe(self.mesh.node_coordinates, src, dst, N, k, 0,
                                         self.mesh.edge_colors)
        assert F.n_dofs == self.asm.handle.n_rows
        rng = np.random.default_rng(11)
        # reference block order: every edge's k N + 1 flux nodes along the edge (a node is a
        # cell vertex iff its position is a multiple of k), then pressure, then multipliers
        flux = np.arange(F.p_offset)
        vertex = (flux % (k * N + 1)) % k == 0
        groups = [(flux[vertex], 3), (flux[~vertex], 3),
                  (np.arange(F.p_offset, F.lm_offset), 4), (np.arange(F.lm_offset, F.n_dofs), 3)]
        picks = [rng.choice(g, size=min(n, g.size), replace=False) for g, n in groups]
        assert all(p.size > 0 for p in picks), "every kind of row is observed"
        self.rows = np.concatenate(picks)
        interior = self.rows[self.rows < F.p_offset]
        assert ((interior % (k * N + 1)) % k != 0).any(), "an interior flux row is observed"
        self.w = 0.5 + rng.random(self.rows.size)
        self.data = rng.standard_normal((3, self.rows.size))

    @property
    def jobs(self):
        return int(self.asm._fe_aux_pc.n_jobs)


_REFS = {}


def cpu_adjoint(s, R=None):
    """The CPU adjoint's operators for the graph and k (computed once per graph, k and R)."""
    key = (s.name, s.k, None if R is None else np.asarray(R, dtype=np.float64).tobytes())
    if key not in _REFS:
        _REFS[key] = AdjointRefFe(s.F, s.R if R is None else R)
    return _REFS[key]


def parity_errors(s, g, data, R=None):
    """The relative errors of every scenario's value, dR, df, dp_bc against the CPU adjoint; no
    column and no quantity skipped, and no reference norm zero."""
    ref = cpu_adjoint(s, R)
    out = []
    for j in range(len(g)):
        r = ref.gradient(s.nodal[j], s.f[j], s.rows, s.w, None if data is None else data[j])
        for name in ("dR", "df", "dp_bc"):
            assert np.linalg.norm(r[name]) > 0, name
        assert abs(r["value"]) > 0
        out.append({"value": abs(g.value[j] - r["value"]) / abs(r["value"]),
                    "dR": rel(g.dR[j], r["dR"]), "df": rel(g.df[j], r["df"]),
                    "dp_bc": rel(g.dp_bc[j], r["dp_bc"])})
    return out


def worst_error(s, g, data, R=None, tag=""):
    worst = 0.0
    for j, errs in enumerate(parity_errors(s, g, data, R)):
        print(f"{s.name} k={s.k} {tag} scenario {j}: "
              + ", ".join(f"{k} {v:.2e}" for k, v in errs.items())
              + f" (refined {g.info['refined']})")
        worst = max(worst, *errs.values())
    return worst


def steady_launches(s, linear, chunks=1):
    """include/nxhip.h, nx_fe_batch_gradient: P = s + 4 launches per solve pass (condense, s
    sweeps, expand, residual, norms), s + 6 with cycles."""
    P = (3 if s.jobs > 0 else 1) + 4 + (2 if s.name in CYCLIC else 0)
    if linear:
        return (1 + P) + chunks * (1 + P + 1 + 1)
    return chunks * (1 + P + 1 + P + 1)


# 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", PARITY_CASES)
def test_parity_with_cpu_adjoint(name, k):
    s = Setup(name, k)
    try:
        if name == "tree6_2d_N70":
            assert s.mesh.N >= 32  # one wave per edge
        if name == "depth6_N40":
            assert s.jobs > 0
        solver = Solver(s.asm, batch_degrees=True)
        worst = 0.0
        for kind, data in (("linear", None), ("lsq", s.data)):
            g = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=data)
            assert g.converged.all() and g.info["fallback"] == 0
            assert g.value.shape == (3,) and g.dR.shape == (3, s.mesh.num_edges)
            assert g.df.shape == g.dR.shape and g.dp_bc.shape == (3, s.mesh.num_nodes)
            worst = max(worst, worst_error(s, g, data, tag=kind))
        print(f"{name} k={k}: worst {worst:.3e}")
        assert worst <= PARITY_BAR, worst
    finally:
        s.close()


# 2 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("tree5_N16", 2), ("edge_info_N10", 3)])
def test_value_is_the_objective_of_solve_many(name, k):
    """``value`` against the objective evaluated on the host from solve_many's columns of the
    same solver: 1e-12 relative for the linear kind (one sum in another order), 1e-10 for least
    squares (two solves' bar)."""
    s = Setup(name, k)
    try:
        solver = Solver(s.asm, batch_degrees=True)
        res = solver.solve_many(s.items, s.f)
        assert res.path == "batched"
        for data, bar in ((None, 1e-12), (s.data, 1e-10)):
            g = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=data)
            for j in range(3):
                J = objective(res.x[j], s.rows, s.w, None if data is None else data[j])
                err = abs(g.value[j] - J) / abs(J)
                print(f"{name} k={k} {'linear' if data is None else 'lsq'} scenario {j}: {err:.2e}")
                assert abs(J) > 0 and err <= bar, (j, err)
    finally:
        s.close()


# 3 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["depth6_N40", "edge_info_N10"])
def test_batch_independence(name):
    """A scenario's bits are the same alone (B = 1), at another position in a batch of 3, and
    under NXHIP_BATCH_CHUNK=2 (chunks of 2 and 1: one scenario sits in the partial last chunk)."""
    s = Setup(name, 2)
    try:
        solver = Solver(s.asm, batch_degrees=True)
        order = [1, 2, 0]
        items3, f3, data3 = [s.items[i] for i in order], s.f[order], s.data[order]
        for lsq in (False, True):
            kw = dict(rows=s.rows, weights=s.w)
            three = solver.gradient(items3, f3, data=data3 if lsq else None, **kw)
            with env(NXHIP_BATCH_CHUNK=2):
                chunked = solver.gradient(items3, f3, data=data3 if lsq else None, **kw)
            assert chunked.info["chunk"] == 2 and three.info["chunk"] == 3
            for pos, j in enumerate(order):
                with env(NXHIP_BATCH=1):
                    alone = solver.gradient(s.items[j:j + 1], s.f[j:j + 1],
                                            data=s.data[j:j + 1] if lsq else None, **kw)
                assert alone.info["chunk"] == 1
                assert_same_bits(alone, three, 0, pos)
                assert_same_bits(alone, chunked, 0, pos)
                assert alone.dR.any() and alone.df.any() and alone.dp_bc.any()
    finally:
        s.close()


# 4 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["depth6_N40", "Y_N4", "edge_info_N10"])
def test_launch_counts_and_one_linear_adjoint(name):
    """One pass, not a loop: a call that finds everything current launches the documented
    steady count, whatever B is inside a chunk -- a forest with several subtree jobs, with one,
    and a graph with cycles (the tree decomposition gives every graph at least one job, so
    s = 1 of the formula is not reachable from the assembler); the first call after
    compute_forms reports more (the assembly it flushed, the cycle correction it built); the
    linear kind solves ONE adjoint column per call."""
    s = Setup(name, 2)
    try:
        solver = Solver(s.asm, batch_degrees=True)
        kw = dict(rows=s.rows, weights=s.w)
        first = solver.gradient(s.items, s.f, **kw)  # (makes everything current)
        second = solver.gradient(s.items, s.f, **kw)
        print(f"{name}: first {first.info}, second {second.info}")
        assert second.info["refined"] == 0 and second.info["chunk"] == 3
        assert second.info["launches"] == steady_launches(s, True)
        if name in CYCLIC:
            m = np.asarray(s.asm._fe_aux_pc.cyc_rows).size
            assert first.info["launches"] >= steady_launches(s, True) + 4 * m + 3
        else:  # (+ 1 only where the assembly was deferred and the call flushed it)
            assert first.info["launches"] - steady_launches(s, True) in (0, 1)
        assert_same_bits(first, second, slice(None), slice(None))
        for B in (1, 3):
            lin = solver.gradient(s.items[:B], s.f[:B], **kw)
            lsq = solver.gradient(s.items[:B], s.f[:B], data=s.data[:B], **kw)
            print(f"{name} B={B}: linear {lin.info}, lsq {lsq.info}")
            assert lin.info["refined"] == 0 and lsq.info["refined"] == 0
            assert lin.info["launches"] == steady_launches(s, True)
            assert lsq.info["launches"] == steady_launches(s, False)
            assert lin.info["chunk"] == B and lsq.info["chunk"] == B
            assert lin.info["fallback"] == 0 and lsq.info["fallback"] == 0
            # the one adjoint column's figures, repeated for every scenario
            assert (lin.residual_norms[:, 1] == lin.residual_norms[0, 1]).all()
        with env(NXHIP_BATCH_CHUNK=2):
            lin = solver.gradient(s.items, s.f, **kw)
            lsq = solver.gradient(s.items, s.f, data=s.data, **kw)
        assert lin.info["refined"] == 0 and lsq.info["refined"] == 0
        assert lin.info["chunk"] == 2 and lin.info["launches"] == steady_launches(s, True, 2)
        assert lsq.info["launches"] == steady_launches(s, False, 2)
    finally:
        s.close()


# 5 ---------------------------------------------------------------------------------------
def test_handle_untouched_and_new_R():
    """The handle's rhs, solution and last-solve figures are bit-identical after a gradient
    call and solver.solve() returns the bits it returned before. After compute_forms with a new
    R the next gradient matches the CPU adjoint at the new R (the auxiliary lumped mass and the
    cycle correction were rebuilt), and the call after it rebuilds nothing."""
    s = Setup("edge_info_N10", 2)
    try:
        solver = Solver(s.asm, batch_degrees=True)
        solver.assemble()
        x0 = np.concatenate([fn.x.array for fn in solver.solve()])
        h = s.asm.handle
        before = (h.rhs(), h.solution(), h.solver(), h.true_residual(), solver.ksp.iterations)
        kw = dict(rows=s.rows, weights=s.w)
        for data in (None, s.data):
            g1 = solver.gradient(s.items, s.f, data=data, **kw)
            after = (h.rhs(), h.solution(), h.solver(), h.true_residual(), solver.ksp.iterations)
            np.testing.assert_array_equal(after[0], before[0])
            np.testing.assert_array_equal(after[1], before[1])
            assert after[2:] == before[2:]
        x1 = np.concatenate([fn.x.array for fn in solver.solve()])
        np.testing.assert_array_equal(x1, x0)
        R2 = 2.0 * s.R[::-1].copy()
        s.asm.compute_forms(p_bc_ex=s.pbc, R=R2)
        g2 = solver.gradient(s.items, s.f, data=s.data, **kw)
        g3 = solver.gradient(s.items, s.f, data=s.data, **kw)
        m = np.asarray(s.asm._fe_aux_pc.cyc_rows).size
        steady = steady_launches(s, False)
        print(f"launches: {g1.info['launches']}, {g2.info['launches']}, {g3.info['launches']}")
        assert g2.info["refined"] == 0 and g3.info["refined"] == 0
        assert g2.info["launches"] >= steady + 1 + 4 * m + 3
        assert g3.info["launches"] == steady
        assert_same_bits(g2, g3, slice(None), slice(None))
        assert rel(g2.dR, g1.dR) > 1e-2
        worst = worst_error(s, g2, s.data, R=R2, tag="new R")
        assert worst <= PARITY_BAR, worst
    finally:
        s.close()


# 6 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["solve_many", "gradient"])
def test_workspace_grows_in_both_orders(first):
    """solve_many then gradient (a workspace allocated without the gradient's part must be
    allocated again with it, not overrun), and gradient then solve_many, on one handle: both
    results hold their bars, and a second round has the first round's bits."""
    s = Setup("tree5_N16", 2)
    try:
        solver = Solver(s.asm, batch_degrees=True)
        A, bs = None, []
        for j in range(3):
            A, b = OF.assemble_reference_fe(s.F, s.nodal[j], f=s.f[j], R=s.R)
            bs.append(b)
        x_ref = np.stack([cpu_adjoint(s).lu.solve(b) for b in bs])

        def many():
            res = solver.solve_many(s.items, s.f)
            assert res.path == "batched" and res.converged.all()
            for j in range(3):
                assert rel(res.x[j], x_ref[j]) <= 1e-10, j
            return res.x.copy()

        def grad():
            g = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=s.data)
            assert g.converged.all()
            assert worst_error(s, g, s.data, tag=first + " first") <= PARITY_BAR
            return g

        if first == "solve_many":
            x, g = many(), grad()
        else:
            g, x = grad(), many()
        np.testing.assert_array_equal(many(), x)
        assert_same_bits(grad(), g, slice(None), slice(None))
        # more columns than the workspace holds: both parts grow together
        items7 = (s.items * 3)[:7]
        f7 = np.tile(s.f, (3, 1))[:7]
        g7 = solver.gradient(items7, f7, rows=s.rows, weights=s.w, data=np.tile(s.data, (3, 1))[:7])
        assert g7.info["chunk"] == 7
        assert_same_bits(g7, g, 6, 0)
        np.testing.assert_array_equal(solver.solve_many(items7, f7).x[3:6], x)
    finally:
        s.close()


# 7 ---------------------------------------------------------------------------------------
def test_where_it_must_not_engage():
    s = Setup("Y_N4", 2)
    try:
        with pytest.raises(NotImplementedError, match="degrees") as err:
            Solver(s.asm).gradient(s.items, s.f, rows=s.rows)
        assert "batch_degrees" in str(err.value)
        solver = Solver(s.asm, batch_degrees=True)
        with pytest.raises(NotImplementedError, match="ensemble"):
            solver.gradient(s.items, s.f, rows=s.rows, R=np.ones((3, s.mesh.num_edges)))
        with pytest.raises(NotImplementedError, match="degrees"):
            solver.hessian_vector(s.items, s.f, rows=s.rows, v_R=np.ones(s.mesh.num_edges))
    finally:
        s.close()
    s = P1Setup("Y_N4", flux_degree=2, pressure_degree=1)
    try:
        with pytest.raises(NotImplementedError):
            Solver(s.asm, batch_degrees=True).gradient(s.items, s.f, rows=np.array([0, 1]))
    finally:
        s.close()


def _c_call(h, bc, value, gR, n_cols=1, kind=0, rows=(0, 1), w=(1.0, 1.0), d=None, n_obs=None,
            maxit=100, no_rows=False, no_w=False):
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rows = np.asarray(rows, dtype=np.int32)
    w = np.asarray(w, dtype=np.float64)
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
    return _lib.lib().nx_fe_batch_gradient(
        h.ptr, n_cols, p(bc, pd), None, None, 1e-12, maxit, kind,
        rows.size if n_obs is None else n_obs, None if no_rows else p(rows, pi),
        None if no_w else p(w, pd), p(d, pd), p(value, pd), p(gR, pd), None, None, None, None,
        None)


def test_c_abi_errors():
    """nx_fe_batch_gradient's NX_ERR_ARG cases and NX_ERR_STATE on a P1/DG0 handle, through the
    ctypes binding."""
    s = Setup("Y_N4", 2)
    try:
        solver = Solver(s.asm, batch_degrees=True)
        solver.gradient(s.items, s.f, rows=s.rows)  # (the handle configured and assembled)
        h = s.asm.handle
        E, n = h.n_edges, h.n_rows
        edge_bc, _, _ = s.asm.scenario_coefficients(s.items[:1], None)
        bc = np.ascontiguousarray(edge_bc)
        value, gR = np.zeros(1), np.zeros(E)
        call = lambda **kw: _c_call(h, kw.pop("bc", bc), kw.pop("value", value),  # noqa: E731
                                    kw.pop("gR", gR), **kw)
        assert call() == _lib.NX_OK  # (grad_bc, grad_f and the status arrays may be NULL)
        assert call(n_cols=0) == _lib.NX_ERR_ARG
        assert call(n_obs=0) == _lib.NX_ERR_ARG
        assert call(rows=(0, n)) == _lib.NX_ERR_ARG
        assert call(rows=(-1, 0)) == _lib.NX_ERR_ARG
        assert call(rows=(3, 3)) == _lib.NX_ERR_ARG
        assert call(kind=2) == _lib.NX_ERR_ARG
        assert call(kind=1, d=None) == _lib.NX_ERR_ARG
        assert call(bc=None) == _lib.NX_ERR_ARG
        assert call(value=None) == _lib.NX_ERR_ARG
        assert call(gR=None) == _lib.NX_ERR_ARG
        assert call(no_rows=True) == _lib.NX_ERR_ARG
        assert call(no_w=True) == _lib.NX_ERR_ARG
        assert call(maxit=0) == _lib.NX_ERR_ARG
        assert call(kind=1, d=np.zeros(2)) == _lib.NX_OK
    finally:
        s.close()
    s = P1Setup("Y_N4")
    try:
        Solver(s.asm).gradient(s.items, s.f, rows=s.rows)
        h = s.asm.handle
        edge_bc, _, _ = s.asm.scenario_coefficients(s.items[:1], None)
        rc = _c_call(h, np.ascontiguousarray(edge_bc), np.zeros(1), np.zeros(h.n_edges))
        assert rc == _lib.NX_ERR_STATE
    finally:
        s.close()


# 8 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tree5_N16", "edge_info_N10"])
def test_zero_columns(name):
    """A scenario with p_bc = 0 and f = 0: the zero solution's value and exact-zero dR (both
    kinds; least squares still has an adjoint there, so df and dp_bc are not zero). A linear
    objective whose weights are all zero: a zero adjoint, reported converged, every derivative
    exactly zero."""
    s = Setup(name, 2)
    try:
        solver = Solver(s.asm, batch_degrees=True)
        items = [s.items[0], np.zeros(s.mesh.num_nodes)]
        f = np.stack([s.f[0], np.zeros(s.mesh.num_edges)])
        kw = dict(rows=s.rows, weights=s.w)
        lin = solver.gradient(items, f, **kw)
        lsq = solver.gradient(items, f, data=s.data[:2], **kw)
        assert lin.value[1] == 0.0 and not lin.dR[1].any()
        J0 = objective(np.zeros(s.F.n_dofs), s.rows, s.w, s.data[1])
        assert lsq.value[1] == pytest.approx(J0, rel=1e-14) and not lsq.dR[1].any()
        assert lsq.df[1].any() and lsq.dp_bc[1].any()
        for g in (lin, lsq):
            assert g.converged.all() and g.residual_norms[1, 0] == 0.0
            assert g.dR[0].any()
        g = solver.gradient(items, f, rows=s.rows, weights=np.zeros(s.rows.size))
        assert g.converged.all() and not g.residual_norms[:, 1].any()
        assert not g.value.any() and not g.dR.any() and not g.df.any() and not g.dp_bc.any()
    finally:
        s.close()
