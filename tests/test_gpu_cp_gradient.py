"""``Solver(asm, batch_continuous=True).gradient`` / ``nx_cp_batch_gradient``: adjoint gradients
of an observed-row objective for continuous pressure (k > m >= 1) on a forest -- one factor
stage of the node-condensed solve per call, two batched passes on its factors and one
contraction over the (k, m) rows (``k_cp_b_edge_form``).

Set-up per graph (tests/test_gpu_fe_gradient.py's with ``flux_degree=k, pressure_degree=m``):
per-edge R = 0.5 + (e mod 3) / 2; B = 3 scenarios -- the case's own p_bc, p_x and a fixed-seed
random nodal array -- each with the per-edge source f = 0.1 + 0.02 (e mod 5); about 12 observed
rows drawn from every kind of row: cell-vertex flux nodes, INTERIOR flux nodes, edge-interior
pressure nodes, pressure DoFs at graph nodes shared by several edges, multipliers (a wrong sign
or a wrong row on a block is an O(1) error); weights in [0.5, 1.5); both kinds of objective
(linear, and least squares against random data).

Yardstick: the CPU adjoint of tests/gradient_ref_fe.py (SuperLU on the oracle's A and A^T,
itself held to central finite differences at m >= 1 in tests/test_gradient_ref_cp.py).
``value``, ``dR``, ``df`` and ``dp_bc`` of every scenario are compared as relative 2-norms.

The parity bar: each figure is a product of two solves held to 1e-10 each, so the bar is set
from a measurement against the CPU adjoint -- 10x the largest error over all the cases below on
an MI355X (margin for machine-to-machine rounding of the sweeps' order), and never above 1e-8
(any formula, sign or row error is O(1)). Measured worst figure per case (both kinds, all
scenarios and quantities): demo_tree_N1 (2,1) 3.1e-14, Y_N4 (2,1) 1.2e-14, Y_N4 (3,1) 2.1e-14,
Y_N4 (3,2) 1.8e-14, Y_N4 (4,3) 1.7e-14, linear_alt_N3 (2,1) 6.8e-14, tree5_N15 (2,1) 5.5e-13,
tree5_N16 (2,1) 2.5e-13, tree5_3d_N31 (3,2) 6.6e-13, tree6_2d_N70 (2,1) 4.6e-13, depth6_N40
(2,1) 1.01e-11, depth6_N40 (4,3) 9.99e-12 (dR of the case's own p_bc on both; its df and dp_bc
are below 1e-12); the largest is PARITY_MEASURED = 1.008e-11, the bar 1.1e-10."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from gradient_ref_fe import AdjointRefFe, objective
from networks_fenicsx_amd import Solver, _lib
from oracle import nx_oracle_fe as OF
from test_gpu_gradient import Setup as P1Setup
from test_gpu_gradient import assert_same_bits, env, rel

pytestmark = pytest.mark.gpu

PARITY_MEASURED = 1.008e-11  # the largest error over test_parity_with_cpu_adjoint's cases
PARITY_BAR = 1.1e-10  # 10 x PARITY_MEASURED (rounded up); may never exceed 1e-8
assert 10 * PARITY_MEASURED <= PARITY_BAR <= 1e-8

# (case, (k, m)): why it is there
PARITY_CASES = [("demo_tree_N1", (2, 1)),  # N = 1: no interior pressure row
                ("Y_N4", (2, 1)), ("Y_N4", (3, 1)), ("Y_N4", (3, 2)), ("Y_N4", (4, 3)),
                ("linear_alt_N3", (2, 1)),  # alternating edge orientation
                ("tree5_N15", (2, 1)), ("tree5_N16", (2, 1)),  # the 16 / 32-lane boundary
                ("tree5_3d_N31", (3, 2)),  # the last 32-lane segment
                ("tree6_2d_N70", (2, 1)),  # two 64-cell chunks per wave
                ("depth6_N40", (2, 1)), ("depth6_N40", (4, 3))]  # 127 edges: a partly empty wave


class Setup(P1Setup):
    """tests/test_gpu_gradient.py's set-up at degrees (k, m): the same R, scenarios and
    sources; the oracle's (k, m) problem; rows from every kind of row."""

    def __init__(self, name, km, **asm_kw):
        k, m = km
        super().__init__(name, flux_degree=k, pressure_degree=m, **asm_kw)
        self.k, self.m = k, m
        src, dst = self.mesh.edges
        N = self.mesh.N
        self.F = F = OF.build_problem_fe(self.mesh.node_coordinates, src, dst, N, k, m,
                                         self.mesh.edge_colors)
        assert F.n_dofs == self.asm.handle.n_rows
        rng = np.random.default_rng(11)
        # reference block order: every edge's k N + 1 flux nodes along the edge (a node is a
        # cell vertex iff its position is a multiple of k), then the pressure of the graph
        # nodes, the edges' interior pressure nodes, then the multipliers
        flux = np.arange(F.p_offset)
        vertex = (flux % (k * N + 1)) % k == 0
        shared = F.p_offset + np.flatnonzero(F.base.degree[F.p_nodes] > 1)
        p_int = np.arange(F.p_offset + F.p_nodes.size, F.lm_offset)
        self.kinds = {"vertex flux": (flux[vertex], 2), "interior flux": (flux[~vertex], 3),
                      "edge-interior pressure": (p_int, 3), "shared node pressure": (shared, 2),
                      "multiplier": (np.arange(F.lm_offset, F.n_dofs), 2)}
        picks = {key: rng.choice(g, size=min(n, g.size), replace=False)
                 for key, (g, n) in self.kinds.items()}
        for key, (g, _) in self.kinds.items():  # every kind of row the graph has is observed
            assert picks[key].size > 0 or g.size == 0, key
        # (only N = 1 with m = 1 has no edge-interior pressure node)
        assert all(p.size > 0 for key, p in picks.items()
                   if not (key == "edge-interior pressure" and m * N == 1)), "every kind"
        self.rows = np.concatenate(list(picks.values()))
        assert np.unique(self.rows).size == self.rows.size
        self.w = 0.5 + rng.random(self.rows.size)
        self.data = rng.standard_normal((3, self.rows.size))


_REFS = {}


def cpu_adjoint(s, R=None):
    """The CPU adjoint's operators for the graph and (k, m) (computed once per graph, pair and
    R; shared by the tests of the module and left unchanged)."""
    key = (s.name, s.k, s.m, None if R is None else np.asarray(R, dtype=np.float64).tobytes())
    if key not in _REFS:
        _REFS[key] = AdjointRefFe(s.F, s.R if R is None else R)
    return _REFS[key]


def parity_errors(s, g, data, R=None, nodal=None, f=None, cols=None):
    """The relative errors of every scenario's value, dR, df, dp_bc against the CPU adjoint; no
    column and no quantity skipped (``cols``: the scenarios with a non-zero right-hand side of
    a test that has a zero scenario too), and no reference norm zero."""
    ref = cpu_adjoint(s, R)
    nodal = s.nodal if nodal is None else nodal
    f = s.f if f is None else f
    out = []
    for j in (range(len(g)) if cols is None else cols):
        r = ref.gradient(nodal[j], f[j], s.rows, s.w, None if data is None else data[j])
        for name in ("dR", "df", "dp_bc"):
            assert np.linalg.norm(r[name]) > 0, name
        assert abs(r["value"]) > 0
        out.append({"value": abs(g.value[j] - r["value"]) / abs(r["value"]),
                    "dR": rel(g.dR[j], r["dR"]), "df": rel(g.df[j], r["df"]),
                    "dp_bc": rel(g.dp_bc[j], r["dp_bc"])})
    return out


def worst_error(s, g, data, tag="", **kw):
    worst = 0.0
    for j, errs in enumerate(parity_errors(s, g, data, **kw)):
        print(f"{s.name} ({s.k},{s.m}) {tag} scenario {j}: "
              + ", ".join(f"{k} {v:.2e}" for k, v in errs.items())
              + f" (refined {g.info['refined']})")
        worst = max(worst, *errs.values())
    return worst


# 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,km", PARITY_CASES)
def test_parity_with_cpu_adjoint(name, km):
    s = Setup(name, km)
    try:
        if name == "tree6_2d_N70":
            assert s.mesh.N > 64  # one wave per edge, two chunks of cells
        if name == "depth6_N40":
            assert s.mesh.num_edges == 127
        solver = Solver(s.asm, batch_continuous=True)
        worst = 0.0
        for kind, data in (("linear", None), ("lsq", s.data)):
            g = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=data)
            assert g.converged.all() and g.info["fallback"] == 0
            assert g.value.shape == (3,) and g.dR.shape == (3, s.mesh.num_edges)
            assert g.df.shape == g.dR.shape and g.dp_bc.shape == (3, s.mesh.num_nodes)
            worst = max(worst, worst_error(s, g, data, tag=kind))
        print(f"PARITY {name} {km}: worst {worst:.3e}")
        assert worst <= PARITY_BAR, worst
    finally:
        s.close()


# 2 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,km", [("tree5_N16", (2, 1)), ("Y_N4", (3, 2))])
def test_value_is_the_objective_of_solve_many(name, km):
    """``value`` against the objective evaluated on the host from solve_many's columns of the
    same solver: 1e-12 relative for the linear kind (one sum in another order), 1e-10 for least
    squares (two solves' bar)."""
    s = Setup(name, km)
    try:
        solver = Solver(s.asm, batch_continuous=True)
        res = solver.solve_many(s.items, s.f)
        assert res.path == "batched"
        for data, bar in ((None, 1e-12), (s.data, 1e-10)):
            g = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=data)
            for j in range(3):
                J = objective(res.x[j], s.rows, s.w, None if data is None else data[j])
                err = abs(g.value[j] - J) / abs(J)
                print(f"{name} {km} {'linear' if data is None else 'lsq'} scenario {j}: {err:.2e}")
                assert abs(J) > 0 and err <= bar, (j, err)
    finally:
        s.close()


# 3 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,km", [("depth6_N40", (2, 1)), ("Y_N4", (3, 2))])
def test_batch_independence(name, km):
    """A scenario's bits are the same alone (B = 1), at another position in a batch of 3, and
    under NXHIP_BATCH_CHUNK=2 (chunks of 2 and 1: one scenario sits in the partial last chunk)."""
    s = Setup(name, km)
    try:
        solver = Solver(s.asm, batch_continuous=True)
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
def forest_runs(s, solver):
    """U and D, the launches of the node forest's up / down pass, from solve_many's documented
    count (include/nxhip.h, nx_cp_batch_solve: F + chunks x S with F = 1 + U and S = 6 + U + D
    for the reference block order) at one and at two chunks."""
    one = solver.solve_many(s.items, s.f)
    with env(NXHIP_BATCH_CHUNK=2):
        two = solver.solve_many(s.items, s.f)
    assert one.path == two.path == "batched"
    assert one.info["refined"] == 0 and two.info["refined"] == 0
    assert one.info["chunk"] == 3 and two.info["chunk"] == 2
    ud = two.info["launches"] - one.info["launches"] - 6  # U + D
    U = one.info["launches"] - 7 - ud
    assert U >= 1 and ud - U >= 1
    return U, ud - U


def steady_launches(U, D, linear, chunks=1):
    """include/nxhip.h, nx_cp_batch_gradient: F = 1 + U per call, P = 4 + U + D per pass."""
    F, P = 1 + U, 4 + U + D
    if linear:
        return F + 1 + P + chunks * (1 + P + 1 + 1)
    return F + chunks * (1 + P + 1 + P + 1)


@pytest.mark.parametrize("name", ["depth6_N40", "Y_N4"])
def test_launch_counts_and_one_linear_adjoint(name):
    """One pass, not a loop: a call that finds everything current launches the documented
    steady count, whatever B is inside a chunk; the factor stage runs once per call and the
    linear kind solves ONE adjoint column per call. rtol = 1e-9 keeps the refinement pass out
    of the count (tests/test_gpu_cp_batch.py's test_one_pass_not_a_loop)."""
    s = Setup(name, (2, 1))
    try:
        solver = Solver(s.asm, batch_continuous=True, petsc_options={"ksp_rtol": 1e-9})
        kw = dict(rows=s.rows, weights=s.w)
        first = solver.gradient(s.items, s.f, **kw)  # (it assembles the matrix)
        U, D = forest_runs(s, solver)
        second = solver.gradient(s.items, s.f, **kw)
        print(f"{name}: U {U}, D {D}, first {first.info}, second {second.info}")
        assert second.info["refined"] == 0 and second.info["chunk"] == 3
        assert second.info["launches"] == steady_launches(U, D, True)
        # (+ 1 only where the assembly was deferred and the call flushed it)
        assert first.info["launches"] - steady_launches(U, D, True) in (0, 1)
        assert_same_bits(first, second, slice(None), slice(None))
        for B in (1, 3):
            lin = solver.gradient(s.items[:B], s.f[:B], **kw)
            lsq = solver.gradient(s.items[:B], s.f[:B], data=s.data[:B], **kw)
            print(f"{name} B={B}: linear {lin.info}, lsq {lsq.info}")
            assert lin.info["refined"] == 0 and lsq.info["refined"] == 0
            assert lin.info["launches"] == steady_launches(U, D, True)
            assert lsq.info["launches"] == steady_launches(U, D, False)
            assert lin.info["chunk"] == B and lsq.info["chunk"] == B
            assert lin.info["fallback"] == 0 and lsq.info["fallback"] == 0
            # the one adjoint column's figures, repeated for every scenario
            assert (lin.residual_norms[:, 1] == lin.residual_norms[0, 1]).all()
        with env(NXHIP_BATCH_CHUNK=2):
            lin = solver.gradient(s.items, s.f, **kw)
            lsq = solver.gradient(s.items, s.f, data=s.data, **kw)
        assert lin.info["refined"] == 0 and lsq.info["refined"] == 0
        assert lin.info["chunk"] == 2
        assert lin.info["launches"] == steady_launches(U, D, True, 2)
        assert lsq.info["launches"] == steady_launches(U, D, False, 2)
    finally:
        s.close()


# 5 ---------------------------------------------------------------------------------------
def test_handle_untouched_and_new_R():
    """The handle's rhs and solution are bit-identical after a gradient call and
    solver.solve() returns the bits it returned before. solve_many, gradient, solve_many: equal
    bits (the workspace grows by the gradient's part in between). After compute_forms with a
    new R the next gradient meets the CPU adjoint at the new R: the factor stage runs per call."""
    s = Setup("depth6_N40", (2, 1))
    try:
        solver = Solver(s.asm, batch_continuous=True)
        solver.assemble()
        x0 = np.concatenate([fn.x.array for fn in solver.solve()])
        h = s.asm.handle
        before = (h.rhs(), h.solution())
        many0 = solver.solve_many(s.items, s.f)
        assert many0.path == "batched"
        kw = dict(rows=s.rows, weights=s.w)
        g1 = None
        for data in (None, s.data):
            g1 = solver.gradient(s.items, s.f, data=data, **kw)
            np.testing.assert_array_equal(h.rhs(), before[0])
            np.testing.assert_array_equal(h.solution(), before[1])
        many1 = solver.solve_many(s.items, s.f)
        np.testing.assert_array_equal(many1.x, many0.x)
        np.testing.assert_array_equal(many1.residual_norms, many0.residual_norms)
        assert_same_bits(solver.gradient(s.items, s.f, data=s.data, **kw), g1, slice(None),
                         slice(None))
        x1 = np.concatenate([fn.x.array for fn in solver.solve()])
        np.testing.assert_array_equal(x1, x0)
        R2 = 2.0 * s.R[::-1].copy()
        s.asm.compute_forms(p_bc_ex=s.pbc, R=R2)
        g2 = solver.gradient(s.items, s.f, data=s.data, **kw)
        g3 = solver.gradient(s.items, s.f, data=s.data, **kw)
        assert_same_bits(g2, g3, slice(None), slice(None))
        assert g2.info["launches"] - g3.info["launches"] in (0, 1)  # (a flushed assembly)
        assert rel(g2.dR, g1.dR) > 1e-2
        worst = worst_error(s, g2, s.data, R=R2, tag="new R")
        assert worst <= PARITY_BAR, worst
    finally:
        s.close()


# 6 ---------------------------------------------------------------------------------------
def test_refinement_and_fallback():
    """tests/test_gpu_cp_batch.py::test_refinement_and_fallback's recipe: rtol = 1e-17 is below
    what the refinement pass reaches, so the non-zero columns of both passes take it and then
    the single-column route (MINRES capped at ksp_max_it = 20); nothing raises. The
    derivatives stay at the parity bar. The zero scenario (p_bc = 0, f = 0) does neither: exact
    zero dR, residual 0, converged. All-zero weights (linear): every derivative exactly zero."""
    s = Setup("double_Y_N5", (2, 1))
    try:
        base = Solver(s.asm, batch_continuous=True)
        base.assemble()
        x0 = np.concatenate([fn.x.array for fn in base.solve()])
        h = s.asm.handle
        rhs0, xd0 = h.rhs(), h.solution()
        tight = Solver(s.asm, batch_continuous=True,
                       petsc_options={"ksp_rtol": 1e-17, "ksp_max_it": 20,
                                      "ksp_error_if_not_converged": False})
        items = [s.items[0], np.zeros(s.mesh.num_nodes)]
        nodal = np.stack([s.nodal[0], np.zeros(s.mesh.num_nodes)])
        f = np.stack([s.f[0], np.zeros(s.mesh.num_edges)])
        kw = dict(rows=s.rows, weights=s.w)
        lin = tight.gradient(items, f, **kw)
        lsq = tight.gradient(items, f, data=s.data[:2], **kw)
        for tag, g, data in (("linear", lin, None), ("lsq", lsq, s.data[:2])):
            print(tag, g.info, g.iterations, g.residual_norms, g.converged)
            assert g.iterations.shape == g.residual_norms.shape == g.converged.shape == (2, 2)
            assert g.info["refined"] >= 2 and g.info["fallback"] >= 1
            worst = worst_error(s, g, data, tag=tag + " rtol 1e-17", nodal=nodal, f=f, cols=[0])
            assert worst <= PARITY_BAR, worst
            assert not g.dR[1].any() and g.residual_norms[1, 0] == 0.0 and g.converged[1, 0]
            assert g.iterations[1, 0] == 1
            assert g.dR[0].any()
        # (the fallback columns ran the single solve on the handle's own arrays, put back)
        np.testing.assert_array_equal(h.rhs(), rhs0)
        np.testing.assert_array_equal(h.solution(), xd0)
        np.testing.assert_array_equal(np.concatenate([fn.x.array for fn in base.solve()]), x0)
        assert lin.value[1] == 0.0
        J0 = objective(np.zeros(s.F.n_dofs), s.rows, s.w, s.data[1])
        assert lsq.value[1] == pytest.approx(J0, rel=1e-14)
        assert lsq.df[1].any() and lsq.dp_bc[1].any()
        g = tight.gradient(items, f, rows=s.rows, weights=np.zeros(s.rows.size))
        assert g.converged[:, 1].all() and not g.residual_norms[:, 1].any()
        assert not g.value.any() and not g.dR.any() and not g.df.any() and not g.dp_bc.any()
    finally:
        s.close()


# 7 ---------------------------------------------------------------------------------------
def test_where_it_must_not_engage(monkeypatch):
    monkeypatch.delenv("NXHIP_CP_BATCH", raising=False)
    s = Setup("Y_N4", (2, 1))
    try:
        for kw in ({}, {"batch_degrees": True}):  # option off; the other option only
            with pytest.raises(NotImplementedError, match="degrees") as err:
                Solver(s.asm, **kw).gradient(s.items, s.f, rows=s.rows)
            assert "batch_continuous" in str(err.value)
        solver = Solver(s.asm, batch_continuous=True)
        with pytest.raises(NotImplementedError, match="ensemble"):
            solver.gradient(s.items, s.f, rows=s.rows, R=np.ones((3, s.mesh.num_edges)))
        with pytest.raises(NotImplementedError, match="degrees"):
            solver.hessian_vector(s.items, s.f, rows=s.rows, v_R=np.ones(s.mesh.num_edges))
    finally:
        s.close()
    s = P1Setup("edge_info_N10", flux_degree=2, pressure_degree=1, cycle_direct=True)
    try:
        with pytest.raises(NotImplementedError, match="nx_cp_batch_supported"):
            Solver(s.asm, batch_continuous=True).gradient(s.items, s.f, rows=np.array([0, 1]))
        assert not s.asm.handle.cp_batch_supported()
    finally:
        s.close()


def _c_call(h, bc, value, gR, n_cols=1, kind=0, rows=(0, 1), w=(1.0, 1.0), d=None, n_obs=None,
            maxit=100, no_rows=False, no_w=False):
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rows = np.asarray(rows, dtype=np.int32)
    w = np.asarray(w, dtype=np.float64)
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
    return _lib.lib().nx_cp_batch_gradient(
        h.ptr, n_cols, p(bc, pd), None, None, 1e-12, maxit, kind,
        rows.size if n_obs is None else n_obs, None if no_rows else p(rows, pi),
        None if no_w else p(w, pd), p(d, pd), p(value, pd), p(gR, pd), None, None, None, None,
        None)


def test_c_abi_errors():
    """nx_cp_batch_gradient's NX_ERR_ARG cases (tests/test_gpu_fe_gradient.py's list) and
    NX_ERR_STATE on a P1/DG0 handle and on a (2, 0) handle, through the ctypes binding."""
    s = Setup("Y_N4", (2, 1))
    try:
        solver = Solver(s.asm, batch_continuous=True)
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
    for deg, opt in (((1, 0), {}), ((2, 0), {"batch_degrees": True})):
        s = P1Setup("Y_N4", flux_degree=deg[0], pressure_degree=deg[1])
        try:
            Solver(s.asm, **opt).gradient(s.items, s.f, rows=np.array([0, 1]))
            h = s.asm.handle
            edge_bc, _, _ = s.asm.scenario_coefficients(s.items[:1], None)
            rc = _c_call(h, np.ascontiguousarray(edge_bc), np.zeros(1), np.zeros(h.n_edges))
            assert rc == _lib.NX_ERR_STATE, deg
        finally:
            s.close()
