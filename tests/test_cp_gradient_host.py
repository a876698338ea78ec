"""Host side of the continuous-pressure adjoint gradient (``nx_cp_batch_gradient``), no device.

Part 1, the model: the device matrix of the (k, m) layouts is symmetric (the host evaluation of
the term tables), so the adjoint is ``cp_apply_model`` on ``k_b_obs``'s right-hand side; the
numpy restatement of the contraction kernel (``layout_fe.cp_edge_form_model``, from the tables
the device gets) is then held against the general-degree CPU adjoint of
tests/gradient_ref_fe.py: value, dR, df and dp_bc to 1e-10 relative -- two solves at the
oracle's bar, exact host arithmetic otherwise. demo_tree_N1 has one cell per edge (no interior
pressure row: both pressure rows of the cell are node rows), linear_alt_N3 alternating edge
orientation; hub5, broom33, cat70, hubhub5x5 and rand200_s1 (tests/tree_shapes.py, N <= 6) put
nodes past the record caps, edges pointing into their parent at junctions of degree 3 to 19 and
the seeded R = 10^U(-1, 1) under the same bar -- before tests/test_gpu_fe_shapes.py runs the
device there, so that a failure on the device is the kernel's, not the model's or the oracle's.

Part 2, the route: the C ABI's new entry (header and ctypes table) and ``Solver.gradient``'s
routing with the handle stubbed -- the new route engages only with ``batch_continuous`` (or
``NXHIP_CP_BATCH=1``) on degrees k > m >= 1, and everything it does not serve still raises
``NotImplementedError`` before any handle call."""

import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from cases import CASES
from gradient_ref_fe import AdjointRefFe
from networks_fenicsx_amd import NetworkMesh, Solver, _lib
from networks_fenicsx_amd.assembly import batch_coefficients, edge_boundary_rhs_adjoint
from networks_fenicsx_amd.layout_fe import (build_cp_tables, build_fe_layout, cp_apply_model,
                                            cp_factor_model, evaluate_terms)
from oracle import nx_oracle as O
from oracle import nx_oracle_fe as OF
from tree_shapes import (FE_N_CAP, SHAPES, coefficients, cp_record_facts, p_xy,
                         reversed_edges)

HEADER = Path(__file__).resolve().parent.parent / "include" / "nxhip.h"
PAIRS = [(2, 1), (3, 1), (3, 2), (4, 3)]
MODEL_CASES = [("Y_N4", km) for km in PAIRS] + [("demo_tree_N1", (2, 1)),
                                                 ("linear_alt_N3", (2, 1))]
# forests that are not binary (tests/tree_shapes.py), the degrees of tests/test_gpu_fe_shapes.py
SHAPE_MODEL_CASES = [(n, km) for n in ("hub5", "broom33", "cat70", "hubhub5x5", "rand200_s1")
                     for km in ((2, 1), (3, 2))]
BAR = 1e-10


class _Model:
    """One graph at (k, m): the layout with its tables, the oracle's problem, the map from the
    reference block order to device rows, and one scenario of tests/test_gpu_cp_gradient.py."""

    def __init__(self, case, k, m):
        if case in SHAPES:  # tests/tree_shapes.py: p_xy, the shape's own R (none: R = 1)
            make, N, _ = SHAPES[case]
            N, strategy, pbc = min(N, FE_N_CAP), None, p_xy
        else:
            make, N, strategy, pbc = CASES[case]
        self.mesh = mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
        src, dst = mesh.edges
        pos = np.asarray(mesh.node_coordinates, dtype=np.float64)
        self.lay = lay = build_fe_layout(pos, src, dst, mesh.degrees, N, k, m)
        self.tab = build_cp_tables(lay, src, dst)
        assert self.tab is not None
        self.F = F = OF.build_problem_fe(pos, src, dst, N, k, m, mesh.edge_colors)
        assert F.n_dofs == lay.n_rows
        E = self.E = mesh.num_edges
        if case in SHAPES:
            self.R = np.asarray(coefficients(case, E).get("R", np.ones(E)), dtype=np.float64)
        else:
            self.R = 0.5 + (np.arange(E) % 3) / 2.0
        self.f = 0.1 + 0.02 * (np.arange(E) % 5)
        self.pb = np.asarray(pbc(F.base.pos3.T.copy()), dtype=np.float64)
        _, self.h = O.cell_geometry(F.base)
        # reference block order -> device rows: flux by colour, pressure (nodes, then the
        # edges' interior nodes), multipliers
        dev = np.empty(F.n_dofs, dtype=np.int64)
        nf = k * N + 1
        for e in range(E):
            dev[F.flux_offset[e]:F.flux_offset[e] + nf] = lay.flux_rows[e]
        dev[F.p_offset:F.lm_offset] = lay.p_rows
        dev[F.lm_offset:] = lay.lm_rows
        assert np.array_equal(np.sort(dev), np.arange(F.n_dofs))
        self.dev = dev
        self.edge_ids = np.arange(E)
        bc, ef, _ = batch_coefficients(mesh, self.edge_ids, self.pb[None, :], self.f[None, :])
        self.val, self.rhs = evaluate_terms(lay, self.R, ef[0], bc[0], self.h)
        self.A = sp.csr_matrix((self.val, lay.col, lay.rowptr), shape=(lay.n_rows, lay.n_rows))


@pytest.mark.parametrize("km", PAIRS)
def test_device_matrix_is_symmetric(km):
    s = _Model("Y_N4", *km)
    assert abs(s.A - s.A.T).max() == 0.0
    assert abs(s.A).max() > 0


@pytest.mark.parametrize("case,km", MODEL_CASES + SHAPE_MODEL_CASES)
@pytest.mark.parametrize("kind", ["linear", "lsq"])
def test_model_matches_cpu_adjoint(case, km, kind):
    from networks_fenicsx_amd.layout_fe import cp_edge_form_model

    s = _Model(case, *km)
    lay, tab, F = s.lay, s.tab, s.F
    if case == "demo_tree_N1":
        assert lay.N == 1 and km[1] * lay.N - 1 == 0  # no interior pressure row
    if case in SHAPES:  # what the shape is there for: nodes past the record caps (the lists),
        # edges pointing into their parent at junctions, the seeded two-decade R
        rec = cp_record_facts(tab)
        rev = reversed_edges(*s.mesh.edges, s.mesh.degrees)
        assert rec["over"] >= 1 or case == "cat70", rec
        assert (rev >= 3).sum() >= 20 or case in ("hub5", "broom33"), rev
        assert (s.R.max() / s.R.min() > 30.0) == (case in ("hubhub5x5", "rand200_s1"))
    rng = np.random.default_rng(11)
    rows = rng.choice(F.n_dofs, size=min(12, F.n_dofs), replace=False)
    assert (rows < F.p_offset).any() and (rows >= F.p_offset).any()
    w = 0.5 + rng.random(rows.size)
    data = None if kind == "linear" else rng.standard_normal(rows.size)
    ref = AdjointRefFe(F, s.R).gradient(s.pb, s.f, rows, w, data)

    fm = cp_factor_model(lay, tab, s.R, s.h)
    x = cp_apply_model(lay, tab, fm, s.rhs[None, :], s.R, s.h)[0]
    x = x + cp_apply_model(lay, tab, fm, (s.rhs - s.A @ x)[None, :], s.R, s.h)[0]
    assert np.linalg.norm(x[s.dev] - ref["x"]) <= BAR * np.linalg.norm(ref["x"])
    # k_b_obs: the objective and the adjoint's right-hand side on the device rows
    xo = x[s.dev[rows]]
    c = np.zeros(lay.n_rows)
    if data is None:
        value = float(np.sum(w * xo))
        c[s.dev[rows]] = w
    else:
        value = 0.5 * float(np.sum(w * (xo - data) ** 2))
        c[s.dev[rows]] = w * (xo - data)
    mu = cp_apply_model(lay, tab, fm, c[None, :], s.R, s.h)[0]
    mu = mu + cp_apply_model(lay, tab, fm, (c - s.A @ mu)[None, :], s.R, s.h)[0]
    gR, gf, gbc = cp_edge_form_model(lay, tab, x, mu, s.h)
    index, sign = edge_boundary_rhs_adjoint(s.mesh, s.edge_ids)
    dp = np.take(gbc.reshape(-1), index) * sign

    def rel(a, b):
        assert np.linalg.norm(b) > 0
        return float(np.linalg.norm(a - b) / np.linalg.norm(b))

    errs = {"value": abs(value - ref["value"]) / abs(ref["value"]), "dR": rel(gR, ref["dR"]),
            "df": rel(gf, ref["df"]), "dp_bc": rel(dp, ref["dp_bc"])}
    print(f"{case} {km} {kind}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAR, errs


def test_tables_carry_mass_and_source_behind_Fh():
    from networks_fenicsx_amd.element import element_tensors

    for k, m in PAIRS:
        s = _Model("Y_N4", k, m)
        nI = s.tab.nI
        off = 16 + 8 * nI + nI * nI
        Mref, _, wref = element_tensors(k, m)
        assert s.tab.cst.size == off + (k + 1) ** 2 + m + 1
        np.testing.assert_array_equal(s.tab.cst[off:off + (k + 1) ** 2], Mref.ravel())
        np.testing.assert_array_equal(s.tab.cst[off + (k + 1) ** 2:], -wref)  # (negated rows)


# ---- part 2: the route ------------------------------------------------------------------
E, NODES, ROWS = 3, 4, 20


class _StubHandle:
    n_rows = ROWS

    def __init__(self, cp_ok=True):
        self.calls = []
        self.touched = []
        self._cp_ok = cp_ok

    def pc_exact(self):
        return True

    def set_ensemble_cycles(self, enable):
        pass

    def batch_supported(self):
        self.touched.append("batch_supported")
        return False

    def fe_batch_supported(self):
        self.touched.append("fe_batch_supported")
        return False

    def cp_batch_supported(self):
        self.touched.append("cp_batch_supported")
        return self._cp_ok

    def batch_info(self):
        return {"launches": 0, "refined": 0, "fallback": 0, "chunk": 1}

    def cp_batch_gradient(self, edge_bc, edge_f, f_const, rtol, maxit, *, rows, weights, data):
        B = edge_bc.shape[0]
        self.calls.append(dict(rows=np.asarray(rows), rtol=rtol, maxit=maxit, data=data))
        gR = np.tile(np.arange(E, dtype=float), (B, 1))
        gbc = np.arange(B * E * 2, dtype=float).reshape(B, E, 2)
        one = np.ones((B, 2))
        return np.zeros(B), gR, gbc, gR + 10.0, one.astype(np.int32), 0 * one, one.astype(bool)

    def batch_gradient(self, *a, **kw):
        raise AssertionError("another entry point on a continuous-pressure system")

    fe_batch_gradient = ensemble_gradient = batch_hvp = batch_gradient


class _StubAssembler:
    """What ``Solver.gradient`` reads of the assembler, for degrees ``deg``."""

    preconditioned = True
    fe_direct_available = True
    lhs_current = True
    _coefficients = object()

    def __init__(self, deg, nranks=1, cp_ok=True):
        self.degrees = deg
        self._nranks = nranks
        self.handle = _StubHandle(cp_ok)

    def set_direct(self, on):
        pass

    def set_preconditioner(self, on):
        pass

    def scenario_coefficients(self, p_bc, f):
        B = len(p_bc)
        return np.zeros((B, E, 2)), None, np.zeros(B)

    def ensemble_coefficients(self, R, p_bc, f):
        B = len(R)
        return np.ones((B, E)), np.zeros((B, E, 2)), None, np.zeros(B)

    def hvp_directions(self, B, v_R, v_p_bc, v_f):
        return np.ones((B, E)), None, None

    def block_order_rows(self):
        return np.arange(ROWS)[::-1].copy()  # (a permutation the route must apply)

    def gradient_maps(self):
        # edge slots reversed; two boundary nodes reading gbc entries 0 and 5, one negated
        return np.arange(E)[::-1].copy(), np.array([0, 5, 0, 0]), np.array([-1.0, 1.0, 0.0, 0.0])


KW = dict(rows=np.array([1, 7]), weights=np.array([1.0, 2.0]))


def test_symbol_is_declared_and_exported():
    text = HEADER.read_text()
    assert "nx_cp_batch_gradient" in _lib.EXPORTED_SYMBOLS
    assert _lib._SIGS["nx_cp_batch_gradient"] == _lib._SIGS["nx_fe_batch_gradient"]
    a = re.search(r"^int nx_cp_batch_gradient\(([^;]*)\);", text, re.M | re.S).group(1)
    b = re.search(r"^int nx_fe_batch_gradient\(([^;]*)\);", text, re.M | re.S).group(1)
    assert " ".join(a.split()) == " ".join(b.split())


@pytest.mark.parametrize("deg", PAIRS)
def test_route_engages_with_batch_continuous(deg):
    asm = _StubAssembler(deg)
    solver = Solver(asm, batch_continuous=True,
                    petsc_options={"ksp_rtol": 1e-11, "ksp_max_it": 77})
    g = solver.gradient([None, None], **KW)
    (call,) = asm.handle.calls
    np.testing.assert_array_equal(call["rows"], asm.block_order_rows()[KW["rows"]])
    assert call["rtol"] == 1e-11 and call["maxit"] == 77 and call["data"] is None
    # the host gathers: edge slots -> graph.edges() order, flux end rows -> boundary nodes
    np.testing.assert_array_equal(g.dR, np.tile([2.0, 1.0, 0.0], (2, 1)))
    np.testing.assert_array_equal(g.df, g.dR + 10.0)
    np.testing.assert_array_equal(g.dp_bc, [[-0.0, 5.0, 0.0, 0.0], [-6.0, 11.0, 0.0, 0.0]])
    assert g.iterations.shape == (2, 2) and g.converged.all()
    solver.gradient([None], data=np.array([0.5, 0.25]), **KW)
    assert asm.handle.calls[-1]["data"].shape == (1, 2)
    assert "batch_supported" not in asm.handle.touched
    assert "fe_batch_supported" not in asm.handle.touched


def test_env_switch_engages_the_route(monkeypatch):
    monkeypatch.setenv("NXHIP_CP_BATCH", "1")
    asm = _StubAssembler((2, 1))
    Solver(asm).gradient([None], **KW)
    assert len(asm.handle.calls) == 1


def test_without_the_option_it_still_raises(monkeypatch):
    monkeypatch.delenv("NXHIP_CP_BATCH", raising=False)
    monkeypatch.delenv("NXHIP_FE_BATCH", raising=False)
    for solver in (Solver(_StubAssembler((2, 1))),
                   Solver(_StubAssembler((3, 2)), batch_continuous=False),
                   Solver(_StubAssembler((2, 1)), batch_degrees=True)):  # (the other option)
        with pytest.raises(NotImplementedError, match="degrees") as err:
            solver.gradient([None], **KW)
        assert "batch_continuous" in str(err.value)
        assert not solver.assembler.handle.calls and not solver.assembler.handle.touched


def test_what_the_route_does_not_serve():
    def solver(deg=(2, 1), opts=None, **kw):
        return Solver(_StubAssembler(deg, **kw), batch_continuous=True, petsc_options=opts)

    def refused(s):
        assert not s.assembler.handle.calls and not s.assembler.handle.touched

    s = solver()
    with pytest.raises(NotImplementedError, match="ensemble"):
        s.gradient([None], R=np.ones((1, E)), **KW)
    refused(s)
    s = solver()
    with pytest.raises(NotImplementedError, match="degrees"):
        s.hessian_vector([None], v_R=np.ones(E), **KW)
    refused(s)
    s = solver((2, 0))  # (k, 0) is batch_degrees', not this option's
    with pytest.raises(NotImplementedError, match="degrees"):
        s.gradient([None], **KW)
    refused(s)
    s = solver(nranks=2)
    with pytest.raises(NotImplementedError, match="one rank"):
        s.gradient([None], **KW)
    refused(s)
    for opts, word in (({"ksp_type": "minres"}, "MINRES"), ({"pc_type": "none"}, "pc_type"),
                       ({"pc_mass": "lumped"}, "lumped")):
        s = solver(opts=opts)
        with pytest.raises(NotImplementedError, match=word):
            s.gradient([None], **KW)
        refused(s)
    # a handle whose batched node-condensed solve does not apply (a graph with cycles)
    s = solver(cp_ok=False)
    with pytest.raises(NotImplementedError, match="nx_cp_batch_supported"):
        s.gradient([None], **KW)
    assert not s.assembler.handle.calls
    s = solver()
    with pytest.raises(NotImplementedError, match="derivatives=False"):
        s.gradient([None], derivatives=False, **KW)
    refused(s)
