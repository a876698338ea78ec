"""``Solver.solve_ensemble`` / ``nx_ensemble_solve`` and ``Solver.gradient(R=...)`` /
``nx_ensemble_gradient``: many resistance fields in one batched pass, a matrix per column.

Set-up per graph: the resident R = 0.5 + (e mod 3) / 2 (``compute_forms``); B = 11 scenarios
(two residual tiles, 8 + 3) whose boundary / source data cycle through ``test_gpu_batch.py``'s
seven (the case's own p_bc, p_x, a fixed-seed random nodal array, a unit pressure at one
terminal, an all-zero column, the first two again with the per-edge source), so scenario 4 is the
zero column and 5, 6 carry the source. Their R rows: 0 the resident R, 1 the constant 1, 2 the
constant 3.7, 3-9 ``10 ** uniform(-1, 1)`` per edge, 10 ``10 ** uniform(-2, 2)`` (fixed seed).

Yardstick: per scenario the oracle's sparse LU of the reference matrix for that scenario's R
and, where f = 0, the analytic resistor network for that R. Rows 0-9 are held to the project's
bar, 1e-10 relative 2-norm (on these graphs the oracle's LU agrees with the analytic answer to
<= 3.5e-15 at +-1 decade, so the reference leaves four orders of margin).

Row 10 (+-2 decades; the oracle's own worst there is 1.9e-13, on linear_alt_N3): measured on an
MI355X against the oracle's LU -- demo_tree_N1 1.7e-16, Y_N4 3.9e-15, linear_alt_N3 2.6e-14,
tree5_N15 5.3e-14, tree5_N16 1.2e-14, depth6_N40 4.4e-14, tree6_2d_N70 4.2e-14, long_N300
6.7e-15 (after the refinement pass) -- three orders below the bar, so row 10 is held to the same
1e-10 and must converge. (Rows 0-9 in the same run: worst 4.0e-13, on tree6_2d_N70.)

The gradients at many R are held against ``tests/gradient_ref.AdjointRef(P, R_j)``, one per R;
the bar is 10x the largest error measured over the cases on an MI355X, never above 1e-8. Measured
worst figure per graph (both kinds, all scenarios and quantities): Y_N4 1.1e-14, tree5_N15
7.8e-14, tree6_2d_N70 8.608e-13 (dR of the resident-R scenario, least squares: the figure
test_gpu_gradient.py records for that graph); GRAD_MEASURED = 8.608e-13, the bar 8.7e-12."""

from __future__ import annotations

import ctypes as C
import os
from contextlib import contextmanager

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from cases import CASES, CYCLIC, p_x, p_y
from gradient_ref import AdjointRef
from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh, Solver, _lib
from networks_fenicsx_amd import network_generation as ng
from networks_fenicsx_amd.assembly import evaluate_nodal
from oracle import nx_oracle as O
from oracle import nx_oracle_fe as OF

pytestmark = pytest.mark.gpu

SOL_TOL = 1e-10  # the project's bar (tests/test_gpu_direct.py)
ROW10_BAR = 1e-10  # row 10 (+-2 decades): measured worst 5.3e-14 (the module docstring)
B = 11
N_SCEN = 7  # test_gpu_batch.py's scenarios, cycled
ZERO = 4

GRAD_MEASURED = 8.608e-13  # the largest error over test_gradient_at_many_R's cases
GRAD_BAR = 8.7e-12  # 10 x GRAD_MEASURED (rounded up); may never exceed 1e-8
assert 10 * GRAD_MEASURED <= GRAD_BAR <= 1e-8


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
    raise KeyError(name)


def resident_R(E):
    return 0.5 + (np.arange(E) % 3) / 2.0


def ensemble_R(E):
    rng = np.random.default_rng(2024)
    R = np.empty((B, E))
    R[0] = resident_R(E)
    R[1] = 1.0
    R[2] = 3.7
    R[3:10] = 10.0 ** rng.uniform(-1.0, 1.0, size=(7, E))
    R[10] = 10.0 ** rng.uniform(-2.0, 2.0, size=E)
    return R


class Setup:
    def __init__(self, name, **asm_kw):
        make, N, strategy, self.pbc = _graph(name)
        self.name, self.kw = name, asm_kw
        self.mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
        self.asm = HydraulicNetworkAssembler(self.mesh, **asm_kw)
        E, nn = self.mesh.num_edges, self.mesh.num_nodes
        self.R0 = resident_R(E)
        self.asm.compute_forms(p_bc_ex=self.pbc, R=self.R0)
        src, dst = self.mesh.edges
        self.P = O.build_problem(self.mesh.node_coordinates, src, dst, N, self.mesh.edge_colors)
        rnd = np.random.default_rng(7).standard_normal(nn)
        unit = np.zeros(nn)
        unit[np.asarray(self.mesh.boundary_in_nodes)[0]] = 1.0
        seven = [self.pbc, p_x, rnd, unit, np.zeros(nn), self.pbc, p_x]
        self.items = [seven[j % N_SCEN] for j in range(B)]
        self.nodal = np.stack([evaluate_nodal(it, self.mesh.node_coordinates)
                               for it in self.items])
        self.f = np.zeros((B, E))
        self.f[5] = self.f[6] = 0.1 + 0.02 * (np.arange(E) % 5)
        self.R = ensemble_R(E)

    def close(self):
        self.asm.close()


_REF = {}


def oracle(s, j, R):
    """(x, A, b) of scenario j at the per-edge R: the oracle's LU, computed once per
    (graph, scenario, R) and shared by the tests."""
    key = (s.name, tuple(sorted(s.kw.items())), j, R.tobytes())
    if key not in _REF:
        if s.kw:
            F = OF.build_problem_fe(s.mesh.node_coordinates, *s.mesh.edges, s.mesh.N,
                                    s.kw.get("flux_degree", 1), s.kw.get("pressure_degree", 0),
                                    s.mesh.edge_colors)
            A, b = OF.assemble_reference_fe(F, s.nodal[j], f=s.f[j], R=R)
        else:
            A, b = O.assemble_reference(s.P, s.nodal[j], f=s.f[j], R=R)
        x = spla.splu(A.tocsc()).solve(b)
        x.setflags(write=False)
        _REF[key] = (x, A, b)
    return _REF[key]


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def check_against_oracle(s, res, cols, R, tol=SOL_TOL, residual=True):
    """Per listed scenario (its own row of R): the oracle bar, the analytic bar (f = 0), the
    residual's bars with the oracle's matrix for that R; the zero column. Returns the errors."""
    errs = {}
    for i, j in enumerate(cols):
        if not s.nodal[j].any() and not s.f[j].any():
            assert not res.x[i].any() and res.residual_norms[i] == 0.0 and res.converged[i]
            continue
        x_ref, A, b = oracle(s, j, R[i])
        errs[j] = e = rel(res.x[i], x_ref)
        print(f"{s.name} scenario {j}: vs oracle {e:.3e}, relres {res.residual_norms[i]:.3e}, "
              f"iterations {res.iterations[i]}")
        bar = tol if np.isscalar(tol) else tol[i]
        assert e <= bar, (j, e)
        if not s.f[j].any() and not s.kw:
            xa = O.resistor_network_solution(s.P, s.nodal[j], R=R[i])
            assert rel(res.x[i], xa) <= bar, (j, rel(res.x[i], xa))
        assert res.converged[i], j
        if residual:
            assert res.residual_norms[i] <= 1e-12, (j, res.residual_norms[i])
            Ab, bb, perm, _ = O.to_build_layout(s.P, A, b)
            host = np.linalg.norm(bb - Ab @ res.x[i][perm]) / np.linalg.norm(bb)
            assert abs(res.residual_norms[i] - host) <= 0.05 * host + 5e-16, (j, host)
    return errs


class HandleState:
    """Check 4: the handle's values, rhs and solution, a solve() and a solve_many."""

    def __init__(self, s, solver, many=None):
        self.s, self.solver, self.many_solver = s, solver, many or solver
        solver.assemble()
        solver.solve()
        # (first: where solve_many takes its own sequential loop it leaves its last solution)
        self.many = self.many_solver.solve_many(s.items[:3], s.f[:3]).x.copy()
        # (a solve with nothing to assemble: what a later solve() of the same system repeats)
        self.sol = np.concatenate([f.x.array for f in solver.solve()])
        h = s.asm.handle
        self.val, self.rhs, self.x = h.csr()[2].copy(), h.rhs(), h.solution()

    def check(self):
        h = self.s.asm.handle
        np.testing.assert_array_equal(h.csr()[2], self.val)
        np.testing.assert_array_equal(h.rhs(), self.rhs)
        np.testing.assert_array_equal(h.solution(), self.x)
        sol = np.concatenate([f.x.array for f in self.solver.solve()])
        np.testing.assert_array_equal(sol, self.sol)
        np.testing.assert_array_equal(
            self.many_solver.solve_many(self.s.items[:3], self.s.f[:3]).x, self.many)


# 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["demo_tree_N1", "Y_N4", "linear_alt_N3", "tree5_N15",
                                  "tree5_N16", "depth6_N40", "tree6_2d_N70", "long_N300"])
def test_parity_with_the_oracle(name):
    """No interior vertex (N = 1), one job, flipped chains, the lane-shape boundary N = 15 / 16,
    8 jobs with 63 top slots, two 64-cell chunks, N = 300.

    Row 10 (R over +-2 decades), relative 2-norm against the oracle's LU, measured on an
    MI355X: 1.7e-16, 3.9e-15, 2.6e-14, 5.3e-14, 1.2e-14, 4.4e-14, 4.2e-14, 6.7e-15 in the order
    of the cases (the last after a refinement pass of 3 columns)."""
    s = Setup(name)
    try:
        solver = Solver(s.asm)
        solver.assemble()
        solver.solve()  # (the call below finds the values assembled)
        res = solver.solve_ensemble(s.R, s.items, s.f)
        assert res.path == "batched" and res.info["fallback"] == 0
        assert res.info["chunk"] == B
        assert res.info["launches"] == 7 + (6 if res.info["refined"] else 0), res.info
        assert res.x.shape == (B, s.asm.handle.n_rows)
        errs = check_against_oracle(s, res, range(B), s.R, tol=[SOL_TOL] * 10 + [ROW10_BAR])
        e10 = errs.pop(10)
        print(f"{name}: rows 0-9 worst {max(errs.values()):.3e}, row 10 {e10:.3e}, "
              f"info {res.info}")
    finally:
        s.close()


# 2 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Y_N4", "tree5_N15", "depth6_N40", "long_N300"])
def test_resident_R_gives_solve_many_bits(name):
    """Every row of R the resident R: the set-up kernel's lumped mass and the residual kernel's
    regenerated entries have the assembly's bits, so x, iterations and the reported residual
    are solve_many's, bit for bit."""
    s = Setup(name)
    try:
        solver = Solver(s.asm)
        many = solver.solve_many(s.items, s.f)
        ens = solver.solve_ensemble(np.tile(s.R0, (B, 1)), s.items, s.f)
        assert many.path == ens.path == "batched"
        np.testing.assert_array_equal(ens.x, many.x)
        np.testing.assert_array_equal(ens.iterations, many.iterations)
        np.testing.assert_array_equal(ens.residual_norms, many.residual_norms)
        # p_bc = None: the last compute_forms' boundary data on every scenario
        none = solver.solve_ensemble(np.tile(s.R0, (2, 1)))
        np.testing.assert_array_equal(none.x[0], many.x[0])
        np.testing.assert_array_equal(none.x[1], many.x[0])
    finally:
        s.close()


# 3 ---------------------------------------------------------------------------------------
def test_a_columns_bits_depend_on_the_column_alone():
    s = Setup("depth6_N40")
    try:
        solver = Solver(s.asm)
        a = solver.solve_ensemble(s.R, s.items, s.f)
        with env(NXHIP_BATCH_CHUNK=4):  # chunks 4 + 4 + 3: a partial last chunk
            b = solver.solve_ensemble(s.R, s.items, s.f)
            assert b.info["chunk"] == 4
            assert b.info["launches"] == 3 * 7 + 6 * sum(
                bool((b.iterations[c:c + 4] == 2).any()) for c in (0, 4, 8))
        c = solver.solve_ensemble(s.R[::-1], s.items[::-1], s.f[::-1])
        np.testing.assert_array_equal(b.x, a.x)
        np.testing.assert_array_equal(b.residual_norms, a.residual_norms)
        np.testing.assert_array_equal(c.x[::-1], a.x)
        np.testing.assert_array_equal(c.residual_norms[::-1], a.residual_norms)
        with env(NXHIP_BATCH=1):
            for j in (0, 3, 4, 6, 10):
                d = solver.solve_ensemble(s.R[j:j + 1], [s.items[j]], s.f[j:j + 1])
                assert d.path == "batched"
                np.testing.assert_array_equal(d.x[0], a.x[j])
                assert d.residual_norms[0] == a.residual_norms[j]
    finally:
        s.close()


# 4 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Y_N4", "depth6_N40"])
def test_handle_untouched(name):
    s = Setup(name)
    try:
        solver = Solver(s.asm)
        state = HandleState(s, solver)
        res = solver.solve_ensemble(s.R, s.items, s.f)
        assert res.path == "batched"
        state.check()
        g = solver.gradient(s.items[:2], s.f[:2], rows=np.array([0, 3]), R=s.R[5:7])
        assert g.converged.all()
        state.check()
    finally:
        s.close()


# 5 ---------------------------------------------------------------------------------------
def test_no_wrong_matrix_fallback():
    """rtol below what one refinement pass reaches (1e-16), as test_gpu_batch.py's
    test_fallback_columns: the device reports the two non-zero columns unconverged and does NOT
    hand them to the single-column path (it solves the handle's matrix); solve_ensemble solves
    them again through its sequential path at their own R, and counts them."""
    s = Setup("depth6_N40")
    try:
        tight = Solver(s.asm, petsc_options={"ksp_rtol": 1e-16,
                                             "ksp_error_if_not_converged": False})
        state = HandleState(s, tight, many=Solver(s.asm))
        cols = [3, ZERO, 5]
        h = s.asm.handle
        bc, ef, fc = s.asm.scenario_coefficients([s.items[j] for j in cols], s.f[cols])
        eR = s.R[cols][:, s.asm._edge_ids]
        _, it, _, cv = h.ensemble_solve(eR, bc, ef, fc, 1e-16)
        assert it.tolist() == [2, 1, 2] and cv.tolist() == [False, True, False]
        assert h.batch_info()["refined"] == 2 and h.batch_info()["fallback"] == 0
        state.check()
        res = tight.solve_ensemble(s.R[cols], [s.items[j] for j in cols], s.f[cols])
        assert res.path == "batched"
        assert res.info["refined"] == 2 and res.info["fallback"] == 2
        assert not res.x[1].any() and res.converged[1] and res.iterations[1] == 1
        check_against_oracle(s, res, cols, s.R[cols], residual=False)
        state.check()
    finally:
        s.close()


# 6 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["forced", "cycles", "fe20"])
def test_sequential_path(kind):
    """NXHIP_BATCH=0, a graph with cycles and general degrees take the per-scenario loop: the
    oracle bar per scenario at its own R, and the coefficients of the last compute_forms (R
    included), the values, rhs and solution are put back."""
    name = {"forced": "tree5_N15", "cycles": "edge_info_N10", "fe20": "Y_N4"}[kind]
    s = Setup(name, **({"flux_degree": 2} if kind == "fe20" else {}))
    try:
        solver = Solver(s.asm)
        state = HandleState(s, solver)
        cols = [0, 2, 3, ZERO, 6, 10]
        with env(**({"NXHIP_BATCH": 0} if kind == "forced" else {})):
            res = solver.solve_ensemble(s.R[cols], [s.items[j] for j in cols], s.f[cols])
        assert res.path == "sequential" and res.x.shape[0] == len(cols)
        for i, j in enumerate(cols):
            if j == ZERO:
                continue
            x_ref, _, _ = oracle(s, j, s.R[j])
            e = rel(res.x[i], x_ref)
            print(f"{name} ({kind}) scenario {j}: vs oracle {e:.3e}")
            assert e <= SOL_TOL and res.converged[i]
        state.check()
    finally:
        s.close()


# 7 ---------------------------------------------------------------------------------------
class GradSetup(Setup):
    """B = 3 scenarios and the observations of test_gpu_gradient.py."""

    def __init__(self, name):
        super().__init__(name)
        E, nn, P = self.mesh.num_edges, self.mesh.num_nodes, self.P
        rng = np.random.default_rng(11)
        self.items = [self.pbc, p_x, rng.standard_normal(nn)]
        self.nodal = np.stack([evaluate_nodal(it, self.mesh.node_coordinates)
                               for it in self.items])
        self.f = np.tile(0.1 + 0.02 * (np.arange(E) % 5), (3, 1))
        blocks = [(0, P.p_offset, 5), (P.p_offset, P.lm_offset, 4), (P.lm_offset, P.n_dofs, 3)]
        self.rows = np.concatenate([lo + rng.choice(hi - lo, size=min(k, hi - lo), replace=False)
                                    for lo, hi, k in blocks])
        self.w = 0.5 + rng.random(self.rows.size)
        self.data = rng.standard_normal((3, self.rows.size))
        self.R = np.stack([self.R0, 10.0 ** rng.uniform(-1.0, 1.0, size=E), np.full(E, 2.0)])


@pytest.mark.parametrize("name", ["Y_N4", "tree5_N15", "tree6_2d_N70"])
def test_gradient_at_many_R(name):
    """value, dR, df, dp_bc of scenario j against the CPU adjoint at R_j, both kinds of
    objective. Measured worst relative error per graph on an MI355X: Y_N4 1.1e-14, tree5_N15
    7.8e-14, tree6_2d_N70 8.608e-13.

    With every row the resident R the outputs are gradient()'s without R, bit for bit (the
    linear kind's one adjoint column and the ensemble's per-column adjoints included), and
    derivatives=False gives the full call's value bits and no derivative."""
    s = GradSetup(name)
    try:
        solver = Solver(s.asm)
        solver.assemble()
        solver.solve()  # (the calls below find the values assembled)
        refs = [AdjointRef(s.P, s.R[j]) for j in range(3)]
        worst = 0.0
        for kind, data in (("linear", None), ("lsq", s.data)):
            g = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=data, R=s.R)
            assert g.converged.all() and g.converged.shape == (3, 2)
            assert g.info["fallback"] == 0
            assert g.info["launches"] == 13 + 6 * int(
                (g.iterations[:, 0] == 2).any()) + 6 * int((g.iterations[:, 1] == 2).any())
            for j in range(3):
                r = refs[j].gradient(s.nodal[j], s.f[j], s.rows, s.w,
                                     None if data is None else data[j])
                errs = {"value": abs(g.value[j] - r["value"]) / abs(r["value"]),
                        "dR": rel(g.dR[j], r["dR"]), "df": rel(g.df[j], r["df"]),
                        "dp_bc": rel(g.dp_bc[j], r["dp_bc"])}
                print(f"{name} {kind} scenario {j}: "
                      + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
                worst = max(worst, *errs.values())
            obj = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=data, R=s.R,
                                  derivatives=False)
            np.testing.assert_array_equal(obj.value, g.value)
            assert obj.dR is None and obj.df is None and obj.dp_bc is None
            assert obj.converged.all() and obj.info["launches"] == 7 + 6 * int(
                (obj.iterations == 2).any())
            base = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=data)
            same = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=data,
                                   R=np.tile(s.R0, (3, 1)))
            for what in ("value", "dR", "df", "dp_bc"):
                np.testing.assert_array_equal(getattr(same, what), getattr(base, what),
                                              err_msg=what)
        print(f"{name}: worst {worst:.3e}")
        assert worst <= GRAD_BAR, worst
    finally:
        s.close()


# 8 ---------------------------------------------------------------------------------------
def _ensemble_rc(h, n_cols, eR, bc, out):
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    return _lib.lib().nx_ensemble_solve(h.ptr, n_cols, p(eR), p(bc), None, None, 1e-12, 0, p(out),
                                        None, None, None)


def test_argument_and_state_errors():
    NX_ERR_ARG, NX_ERR_STATE = _lib.NX_ERR_ARG, _lib.NX_ERR_STATE
    s = Setup("Y_N4")
    try:
        h = s.asm.handle
        solver = Solver(s.asm)
        solver._configure()
        E = h.n_edges
        eR = np.ones((2, E))
        bc = np.zeros((2, E, 2))
        out = np.zeros((2, h.n_rows))
        assert h.ensemble_supported()
        assert _ensemble_rc(h, 2, eR, bc, out) == NX_ERR_STATE  # values not assembled
        solver.assemble()
        assert _ensemble_rc(h, 2, eR, bc, out) == _lib.NX_OK
        assert _ensemble_rc(h, 0, eR, bc, out) == NX_ERR_ARG
        assert _ensemble_rc(h, 2, None, bc, out) == NX_ERR_ARG
        assert _ensemble_rc(h, 2, eR, None, out) == NX_ERR_ARG
        assert _ensemble_rc(h, 2, eR, bc, None) == NX_ERR_ARG
        for bad in (0.0, -1.0, np.nan, np.inf):
            eB = eR.copy()
            eB[1, E - 1] = bad
            assert _ensemble_rc(h, 2, eB, bc, out) == NX_ERR_ARG, bad
            with pytest.raises(_lib.NxError):
                h.ensemble_gradient(eB, bc, rows=np.array([0]), weights=np.ones(1))
        with pytest.raises(ValueError):
            solver.solve_ensemble(np.array([1.0, -1.0]))
        with pytest.raises(ValueError):
            solver.solve_ensemble(np.ones((2, E + 1)))
        with pytest.raises(NotImplementedError):
            solver.gradient(s.items[:2], rows=np.array([0]), derivatives=False)
        s.asm._nranks = 2  # (what an assembler of a two-rank run carries)
        with pytest.raises(NotImplementedError):
            solver.solve_ensemble(np.array([1.0, 2.0]))
        s.asm._nranks = 1
    finally:
        s.close()
    s = Setup("edge_info_N10")
    try:
        h = s.asm.handle
        solver = Solver(s.asm)
        solver.assemble()
        solver.solve()
        E = h.n_edges
        assert h.batch_supported() and not h.ensemble_supported()
        assert _ensemble_rc(h, 2, np.ones((2, E)), np.zeros((2, E, 2)),
                            np.zeros((2, h.n_rows))) == NX_ERR_STATE
        with pytest.raises(NotImplementedError):
            solver.gradient(s.items[:2], rows=np.array([0]), R=np.array([1.0, 2.0]))
    finally:
        s.close()
