"""``Solver.gradient`` / ``nx_batch_gradient``: adjoint gradients of an observed-row objective
with respect to every edge's R, every boundary node's pressure and every edge's source, in two
batched direct solves on the device.

Set-up per graph: per-edge R = 0.5 + (e mod 3) / 2; B = 3 scenarios -- the case's own p_bc, p_x
and a fixed-seed random nodal array -- each with the per-edge source f = 0.1 + 0.02 (e mod 5);
about 12 observed rows drawn from the flux, the pressure AND the multiplier rows (a wrong sign
on a block is an O(1) error), weights in [0.5, 1.5); both kinds of objective (linear, and least
squares against random data).

Yardstick: the CPU adjoint of tests/gradient_ref.py (SuperLU on the oracle's A and A^T, itself
held to central finite differences in tests/test_gradient_ref.py). ``value``, ``dR``, ``df``
and ``dp_bc`` of every scenario are compared as relative 2-norms.

The parity bar: each figure is a product of two solves held to 1e-10 each, so the bar is set
from a measurement -- 10x the largest error over all the cases below on an MI355X (margin for
machine-to-machine rounding of the sweeps' order), and never above 1e-8 (any formula or sign
error is O(1)). Measured worst figure per case (both kinds, all scenarios and quantities):
demo_tree_N1 6.6e-16, Y_N4 1.1e-14, tree5_N15 7.7e-14, tree5_N16 4.1e-14, tree5_3d_N31 2.3e-13,
tree6_2d_N70 8.6e-13, long_N300 2.5e-13, edge_info_N10 3.9e-13, lattice6x6_N3 2.3e-14,
lattice19x20_N2 5.5e-13; the largest is PARITY_MEASURED = 8.608e-13, the bar 8.7e-12."""

from __future__ import annotations

import ctypes as C
import os
from contextlib import contextmanager

import numpy as np
import pytest

from cases import CASES, CYCLIC, p_x, p_y
from gradient_ref import AdjointRef
from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh, Solver, _lib
from networks_fenicsx_amd import network_generation as ng
from networks_fenicsx_amd.assembly import evaluate_nodal
from networks_fenicsx_amd.post_processing import terminal_conductance
from oracle import nx_oracle as O
from tree_shapes import FE_N_CAP, SHAPES, coefficients, p_xy

pytestmark = pytest.mark.gpu

PARITY_MEASURED = 8.608e-13  # the largest error over test_parity_with_cpu_adjoint's cases
PARITY_BAR = 8.7e-12  # 10 x PARITY_MEASURED (rounded up); may never exceed 1e-8
assert 10 * PARITY_MEASURED <= PARITY_BAR <= 1e-8
SOLVE_BAR = 1e-10  # the project's bar on a solve_many column against the oracle

PARITY_CASES = ["demo_tree_N1", "Y_N4", "tree5_N15", "tree5_N16", "tree5_3d_N31", "tree6_2d_N70",
                "long_N300", "edge_info_N10", "lattice6x6_N3", "lattice19x20_N2"]


@contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _graph(name):
    if name in CASES:
        return CASES[name]
    if name in CYCLIC:
        make, N = CYCLIC[name]
        return make, N, None, p_y
    if name == "long_N300":
        return (lambda: ng.make_tree(3, 1, 1)), 300, None, p_y
    if name in SHAPES:  # tests/tree_shapes.py (the degree-k set-ups of test_gpu_fe_shapes.py)
        return SHAPES[name][0], min(SHAPES[name][1], FE_N_CAP), None, p_xy
    raise KeyError(name)


class Setup:
    def __init__(self, name, **asm_kw):
        make, N, strategy, self.pbc = _graph(name)
        self.name = name
        self.mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
        self.asm = HydraulicNetworkAssembler(self.mesh, **asm_kw)
        E, nn = self.mesh.num_edges, self.mesh.num_nodes
        if name in SHAPES:  # the shape's own coefficients (none: R = 1, f = 0)
            coef = coefficients(name, E)
            self.R = np.asarray(coef.get("R", np.ones(E)), dtype=np.float64)
            self.asm.compute_forms(p_bc_ex=self.pbc, R=self.R, **({"f": coef["f"]} if coef else {}))
        else:
            self.R = 0.5 + (np.arange(E) % 3) / 2.0
            self.asm.compute_forms(p_bc_ex=self.pbc, R=self.R)
        src, dst = self.mesh.edges
        self.P = P = O.build_problem(self.mesh.node_coordinates, src, dst, N,
                                     self.mesh.edge_colors)
        rng = np.random.default_rng(11)
        self.items = [self.pbc, p_x, rng.standard_normal(nn)]
        self.nodal = np.stack([evaluate_nodal(it, self.mesh.node_coordinates)
                               for it in self.items])
        self.f = np.tile(0.1 + 0.02 * (np.arange(E) % 5), (3, 1))
        # observed rows (reference block order): flux, pressure and multiplier rows
        blocks = [(0, P.p_offset, 5), (P.p_offset, P.lm_offset, 4), (P.lm_offset, P.n_dofs, 3)]
        self.rows = np.concatenate([lo + rng.choice(hi - lo, size=min(k, hi - lo), replace=False)
                                    for lo, hi, k in blocks])
        assert (self.rows >= P.lm_offset).any() and (self.rows < P.p_offset).any()
        self.w = 0.5 + rng.random(self.rows.size)
        self.data = rng.standard_normal((3, self.rows.size))

    def close(self):
        self.asm.close()


_REFS = {}


def cpu_adjoint(s, R=None):
    """The CPU adjoint's operators for the graph (computed once per graph and R)."""
    key = (s.name, None if R is None else float(np.sum(R)))
    if key not in _REFS:
        _REFS[key] = AdjointRef(s.P, s.R if R is None else R)
    return _REFS[key]


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b))


def parity_errors(s, g, data, R=None):
    """The relative errors of every scenario's value, dR, df, dp_bc against the CPU adjoint."""
    ref = cpu_adjoint(s, R)
    out = []
    for j in range(len(g)):
        r = ref.gradient(s.nodal[j], s.f[j], s.rows, s.w, None if data is None else data[j])
        errs = {"value": abs(g.value[j] - r["value"]) / abs(r["value"]),
                "dR": rel(g.dR[j], r["dR"]), "df": rel(g.df[j], r["df"]),
                "dp_bc": rel(g.dp_bc[j], r["dp_bc"])}
        out.append(errs)
    return out


def assert_same_bits(a, b, j_a, j_b):
    for name in ("value", "dR", "df", "dp_bc"):
        np.testing.assert_array_equal(getattr(a, name)[j_a], getattr(b, name)[j_b], err_msg=name)


def steady_launches(cycles, linear, chunks=1):
    """include/nxhip.h, nx_batch_gradient: S = 5 / 7 launches per batched solve pass."""
    S = 7 if cycles else 5
    if linear:
        return (1 + S) + chunks * (1 + S + 1 + 1)
    return chunks * (1 + S + 1 + S + 1)


# 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PARITY_CASES)
def test_parity_with_cpu_adjoint(name):
    """Every lane shape of k_b_edge_form (one cell per edge; 4 and 2 edges per wave and their
    boundary N = 15 / 16 / 31; two 64-cell chunks; five chunks), forests and graphs with cycles
    (2, 25 and 342 cycle chains; on the last some columns take the refinement pass)."""
    s = Setup(name)
    try:
        solver = Solver(s.asm)
        worst = 0.0
        for kind, data in (("linear", None), ("lsq", s.data)):
            g = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=data)
            assert g.converged.all() and g.info["fallback"] == 0
            assert g.value.shape == (3,) and g.dR.shape == (3, s.mesh.num_edges)
            assert g.df.shape == g.dR.shape and g.dp_bc.shape == (3, s.mesh.num_nodes)
            for j, errs in enumerate(parity_errors(s, g, data)):
                print(f"{name} {kind} scenario {j}: "
                      + ", ".join(f"{k} {v:.2e}" for k, v in errs.items())
                      + f" (refined {g.info['refined']})")
                worst = max(worst, *errs.values())
        print(f"{name}: worst {worst:.3e}")
        assert worst <= PARITY_BAR, worst
    finally:
        s.close()


def test_refined_adjoint_columns():
    """lattice19x20_N2 (342 cycle chains) with ksp_rtol = 1e-13, below what one pass of the
    direct solve reaches there: forward AND adjoint columns take the refinement pass (a list of
    those columns only), ``refined`` counts both, and the refined gradients hold the same bar."""
    s = Setup("lattice19x20_N2")
    try:
        solver = Solver(s.asm, petsc_options={"ksp_rtol": 1e-13,
                                              "ksp_error_if_not_converged": False})
        for data in (None, s.data):
            g = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=data)
            two = g.iterations == 2
            print(f"iterations {g.iterations.tolist()}, relres {g.residual_norms.tolist()}, "
                  f"info {g.info}")
            n_adj = int(two[:, 1].sum()) if data is not None else int(two[0, 1])
            assert two[:, 1].any() and two[:, 0].any()
            if g.info["fallback"] == 0:
                assert g.info["refined"] == int(two[:, 0].sum()) + n_adj
            worst = max(max(e.values()) for e in parity_errors(s, g, data))
            print(f"worst {worst:.3e}")
            assert worst <= PARITY_BAR, worst
    finally:
        s.close()


# 2 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tree5_N16", "edge_info_N10"])
def test_own_data_gives_exact_zero(name):
    """data = the forward solution's own observed values (from solve_many): J = 0, c = 0, a
    zero adjoint reported converged, and every gradient exactly 0."""
    s = Setup(name)
    try:
        solver = Solver(s.asm)
        x = solver.solve_many(s.items, s.f).x
        g = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=x[:, s.rows].copy())
        assert not g.value.any() and not g.dR.any() and not g.df.any() and not g.dp_bc.any()
        assert g.converged.all() and not g.residual_norms[:, 1].any()
    finally:
        s.close()


# 3 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tree5_N16", "edge_info_N10"])
def test_launch_counts_and_one_linear_adjoint(name):
    """A call that finds everything current launches the documented steady count when nothing
    is refined, whatever B is inside a chunk; the linear kind solves ONE adjoint column per
    call (its count has one solve pass per call plus one per chunk, not two per chunk)."""
    s = Setup(name)
    cyc = name in CYCLIC
    try:
        solver = Solver(s.asm)
        solver.gradient(s.items, s.f, rows=s.rows, weights=s.w)  # (makes everything current)
        for B in (1, 3):
            lin = solver.gradient(s.items[:B], s.f[:B], rows=s.rows, weights=s.w)
            lsq = solver.gradient(s.items[:B], s.f[:B], rows=s.rows, weights=s.w,
                                  data=s.data[:B])
            print(f"{name} B={B}: linear {lin.info}, lsq {lsq.info}")
            assert lin.info["refined"] == 0 and lsq.info["refined"] == 0
            assert lin.info["launches"] == steady_launches(cyc, True) == (18 if cyc else 14)
            assert lsq.info["launches"] == steady_launches(cyc, False) == (17 if cyc else 13)
            assert lin.info["chunk"] == B
            # the one adjoint column's figures, repeated for every scenario
            assert (lin.residual_norms[:, 1] == lin.residual_norms[0, 1]).all()
        with env(NXHIP_BATCH_CHUNK=2):
            lin = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w)
            lsq = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=s.data)
        assert lin.info["chunk"] == 2 and lin.info["launches"] == steady_launches(cyc, True, 2)
        assert lsq.info["launches"] == steady_launches(cyc, False, 2)
    finally:
        s.close()


# 4 ---------------------------------------------------------------------------------------
def test_linear_end_flux_is_terminal_conductance():
    """J = the end flux at terminal s (one observed row, weight 1): dJ/dp_bc is row s of the
    conductance matrix up to its documented sign (+q_N at an edge's target, -q_0 at a source),
    whatever the scenario (x is linear in p_bc)."""
    s = Setup("tree5_N16")
    try:
        solver = Solver(s.asm)
        nodes, Cm = terminal_conductance(solver)
        asm, mesh = s.asm, s.mesh
        per = mesh.N + 1
        src, dst = mesh.edges
        q0 = np.full(src.size, -1, dtype=np.int64)
        off = 0
        for V in asm.flux_spaces:
            edges = np.asarray(V.edges, dtype=np.int64)
            q0[edges] = off + per * np.arange(edges.size)
            off += per * edges.size
        for i in (0, 1, nodes.size - 1):
            t = nodes[i]
            e_t = np.flatnonzero(dst == t)
            pos, sign = ((q0[e_t[0]] + per - 1, 1.0) if e_t.size
                         else (q0[np.flatnonzero(src == t)[0]], -1.0))
            g = solver.gradient(s.items[:2], s.f[:2], rows=np.array([pos]))
            for j in range(2):
                err = rel(sign * g.dp_bc[j, nodes], Cm[i])
                print(f"terminal {int(t)} scenario {j}: {err:.2e}")
                # (C comes from solve_many's columns, each within SOLVE_BAR of the oracle)
                assert err <= SOLVE_BAR + PARITY_BAR
                off_boundary = np.setdiff1d(np.arange(mesh.num_nodes), nodes)
                assert not g.dp_bc[j, off_boundary].any()
    finally:
        s.close()


# 5 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tree5_N15", "tree6_2d_N70", "lattice6x6_N3"])
def test_batch_independence(name):
    """A scenario's bits are the same alone (B = 1), at another position in B = 5, and under
    NXHIP_BATCH_CHUNK=2 (chunks 2, 2, 1: it sits in the partial last chunk)."""
    s = Setup(name)
    try:
        solver = Solver(s.asm)
        order = [0, 1, 0, 1, 2]
        items5, f5, data5 = [s.items[i] for i in order], s.f[order], s.data[order]
        for data1, d5 in ((None, None), (s.data[2:3], data5)):
            kw = dict(rows=s.rows, weights=s.w)
            alone = solver.gradient(s.items[2:3], s.f[2:3], data=data1, **kw)
            five = solver.gradient(items5, f5, data=d5, **kw)
            with env(NXHIP_BATCH_CHUNK=2):
                chunked = solver.gradient(items5, f5, data=d5, **kw)
            assert chunked.info["chunk"] == 2 and five.info["chunk"] == 5
            assert_same_bits(alone, five, 0, 4)
            assert_same_bits(alone, chunked, 0, 4)
            assert_same_bits(five, chunked, 0, 2)
            assert alone.dR.any() and alone.df.any() and alone.dp_bc.any()
    finally:
        s.close()


# 6 ---------------------------------------------------------------------------------------
def test_handle_state_untouched():
    """solver.solve() returns identical bits before and after a gradient call (the handle's
    rhs, x, published state are left as they were)."""
    s = Setup("tree5_3d_N31")
    try:
        solver = Solver(s.asm)
        solver.assemble()
        x0 = np.concatenate([fn.x.array for fn in solver.solve()])
        v0 = solver.solution_vector().copy()
        solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=s.data)
        np.testing.assert_array_equal(solver.solution_vector(), v0)
        x1 = np.concatenate([fn.x.array for fn in solver.solve()])
        np.testing.assert_array_equal(x1, x0)
    finally:
        s.close()


# 7 ---------------------------------------------------------------------------------------
def test_new_R_rebuilds_the_cycle_correction_once():
    """compute_forms with another R: the next gradient assembles the matrix and rebuilds the
    cycle correction (at least 1 + 4 m + 3 launches more, m = 2 n_cyc), matches the CPU adjoint
    for the new R and differs from the old one; the call after it builds nothing."""
    s = Setup("edge_info_N10")
    try:
        solver = Solver(s.asm)
        kw = dict(rows=s.rows, weights=s.w, data=s.data)
        g1 = solver.gradient(s.items, s.f, **kw)
        R2 = 2.0 * s.R[::-1].copy()
        s.asm.compute_forms(p_bc_ex=s.pbc, R=R2)
        g2 = solver.gradient(s.items, s.f, **kw)
        g3 = solver.gradient(s.items, s.f, **kw)
        m = np.asarray(s.asm.tree_preconditioner.cyc_rows).size
        steady = steady_launches(True, False)
        print(f"launches: {g1.info['launches']}, {g2.info['launches']}, {g3.info['launches']}")
        assert g2.info["refined"] == 0 and g3.info["refined"] == 0
        assert g2.info["launches"] >= steady + 1 + 4 * m + 3
        assert g3.info["launches"] == steady
        assert_same_bits(g2, g3, slice(None), slice(None))
        assert rel(g2.dR, g1.dR) > 1e-2
        worst = max(max(e.values()) for e in parity_errors(s, g2, s.data, R=R2))
        assert worst <= PARITY_BAR, worst
    finally:
        s.close()


# 8 ---------------------------------------------------------------------------------------
def test_errors():
    s = Setup("Y_N4")
    try:
        solver = Solver(s.asm)
        n = s.asm.handle.n_rows
        with pytest.raises(ValueError, match="distinct"):
            solver.gradient(s.items, s.f, rows=np.array([1, 2, 1]))
        with pytest.raises(ValueError, match="rows must lie"):
            solver.gradient(s.items, s.f, rows=np.array([0, n]))
        with pytest.raises(ValueError, match="rows must lie"):
            solver.gradient(s.items, s.f, rows=np.array([-1, 0]))
        with pytest.raises(ValueError, match="data must be"):
            solver.gradient(s.items, s.f, rows=s.rows, data=np.zeros((2, s.rows.size)))
        for opts, word in (({"ksp_type": "minres"}, "MINRES"), ({"pc_type": "none"}, "pc_type"),
                           ({"pc_mass": "lumped"}, "lumped")):
            with pytest.raises(NotImplementedError, match=word):
                Solver(s.asm, petsc_options=opts).gradient(s.items, s.f, rows=s.rows)
    finally:
        s.close()
    s = Setup("Y_N4", flux_degree=2, pressure_degree=0)
    try:
        with pytest.raises(NotImplementedError, match="degrees"):
            Solver(s.asm).gradient(s.items, s.f, rows=np.array([0, 1]))
    finally:
        s.close()


def test_c_abi_argument_errors():
    """nx_batch_gradient's NX_ERR_ARG cases, through the ctypes binding."""
    s = Setup("Y_N4")
    try:
        solver = Solver(s.asm)
        solver.gradient(s.items, s.f, rows=s.rows)  # (the handle configured and assembled)
        h = s.asm.handle
        E, n = h.n_edges, h.n_rows
        edge_bc, _, _ = s.asm.scenario_coefficients(s.items[:1], None)
        bc = np.ascontiguousarray(edge_bc)
        value, gR = np.zeros(1), np.zeros(E)
        pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)

        def call(n_cols=1, bc=bc, kind=0, rows=(0, 1), w=(1.0, 1.0), d=None, value=value,
                 gR=gR, n_obs=None):
            rows = np.asarray(rows, dtype=np.int32)
            w = np.asarray(w, dtype=np.float64)
            p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
            return _lib.lib().nx_batch_gradient(
                h.ptr, n_cols, p(bc, pd), None, None, 1e-12, kind,
                rows.size if n_obs is None else n_obs, p(rows, pi), p(w, pd), p(d, pd),
                p(value, pd), p(gR, pd), None, None, None, None, None)

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
        assert call(kind=1, d=np.zeros(2)) == _lib.NX_OK
    finally:
        s.close()
