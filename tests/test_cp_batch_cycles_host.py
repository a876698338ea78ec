"""Host side of the batched continuous-pressure solve on graphs with cycles
(``nx_set_cp_batch_cycles`` / ``Solver(..., batch_continuous_cycles=True)``), no device.

Part 1, the model: ``layout_fe.cp_cyc_factor_model`` (the grounded factor stage, U^T Z, the
capacitance matrix and its inverse by a pivoted elimination) and ``cp_cyc_apply_model`` (the
corrected right-hand-side sweeps with the grounded solve's one refinement), in the kernels'
order, against SuperLU on ``oracle.nx_oracle_fe.assemble_reference_fe``. The columns are the 7
scenarios of tests/test_gpu_batch.py on the matrix of its per-edge R. Bars: every non-zero
column <= 1e-10 against the LU, and a true residual <= 1e-12 after one pass plus at most one
outer refinement -- the batch has one refinement pass where the single solve has two, and this
is the condition under which tests/test_gpu_cp_batch_cycles.py forbids fallback columns.
The figures of every case are printed; DESIGN.md section 3m tabulates them.

Part 2: the gradient through the model and ``cp_edge_form_model`` against the general-degree
CPU adjoint (tests/gradient_ref_fe.py), chords included, to 1e-10 -- two solves at the
oracle's bar, exact host arithmetic otherwise (tests/test_cp_gradient_host.py's bar).

Part 3: the C ABI's two new entries and the ``Solver`` keyword with its environment switch."""

import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from cases import CASES, CYCLIC, p_x, p_y
from gradient_ref_fe import AdjointRefFe
from networks_fenicsx_amd import NetworkMesh, Solver, _lib
from networks_fenicsx_amd.assembly import (batch_coefficients, edge_boundary_rhs_adjoint,
                                           evaluate_nodal)
from networks_fenicsx_amd.layout_fe import (build_cp_tables, build_fe_layout, cp_apply_model,
                                            cp_cyc_apply_model, cp_cyc_factor_model,
                                            cp_edge_form_model, cp_factor_model, evaluate_terms)
from oracle import nx_oracle as O
from oracle import nx_oracle_fe as OF

HEADER = Path(__file__).resolve().parent.parent / "include" / "nxhip.h"
PAIRS = [(2, 1), (3, 1), (3, 2), (4, 3)]
SMALL = ["edge_info_N10", "lattice4x5_N6", "lattice6x6_N3"]
MODEL_CASES = [(n, km) for n in SMALL for km in PAIRS] + [("lattice19x20_N2", (2, 1))]
N_SCEN, ZERO = 7, 4
SOL_TOL, RES_TOL = 1e-10, 1e-12


def _scenarios(mesh, pbc_case):
    """tests/test_gpu_batch.py's ``scenarios`` (that module needs a device to import its
    neighbours' fixtures; the 7 columns are restated here): nodal values (7, nodes), f (7, E)."""
    nn = mesh.num_nodes
    rnd = np.random.default_rng(7).standard_normal(nn)
    unit = np.zeros(nn)
    unit[np.asarray(mesh.boundary_in_nodes)[0]] = 1.0
    items = [pbc_case, p_x, rnd, unit, np.zeros(nn), pbc_case, p_x]
    nodal = np.stack([evaluate_nodal(it, mesh.node_coordinates) for it in items])
    f = np.zeros((N_SCEN, mesh.num_edges))
    f[5] = f[6] = 0.1 + 0.02 * (np.arange(mesh.num_edges) % 5)
    return nodal, f


class _Model:
    """One graph at (k, m): the layout and its tables with chords, the oracle's problem, the
    map from the reference block order to device rows, the 7 scenario columns in the device
    layout and the device matrix from the term tables."""

    def __init__(self, case, k, m):
        if case in CYCLIC:
            make, N = CYCLIC[case]
            strategy, pbc = None, p_y
        else:
            make, N, strategy, pbc = CASES[case]
        self.mesh = mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
        src, dst = mesh.edges
        pos = np.asarray(mesh.node_coordinates, dtype=np.float64)
        self.lay = lay = build_fe_layout(pos, src, dst, mesh.degrees, N, k, m)
        self.tab = build_cp_tables(lay, src, dst, cycles=True)
        assert self.tab is not None
        self.F = F = OF.build_problem_fe(pos, src, dst, N, k, m, mesh.edge_colors)
        assert F.n_dofs == lay.n_rows
        E = self.E = mesh.num_edges
        self.R = 0.5 + (np.arange(E) % 3) / 2.0
        _, self.h = O.cell_geometry(F.base)
        dev = np.empty(F.n_dofs, dtype=np.int64)
        nf = k * N + 1
        for e in range(E):
            dev[F.flux_offset[e]:F.flux_offset[e] + nf] = lay.flux_rows[e]
        dev[F.p_offset:F.lm_offset] = lay.p_rows
        dev[F.lm_offset:] = lay.lm_rows
        assert np.array_equal(np.sort(dev), np.arange(F.n_dofs))
        self.dev = dev
        self.edge_ids = np.arange(E)
        self.nodal, self.f = _scenarios(mesh, pbc)
        bc, ef, _ = batch_coefficients(mesh, self.edge_ids, self.nodal, self.f)
        cols = [evaluate_terms(lay, self.R, ef[j], bc[j], self.h) for j in range(N_SCEN)]
        self.val = cols[0][0]
        self.B = np.stack([c[1] for c in cols])
        self.A = sp.csr_matrix((self.val, lay.col, lay.rowptr), shape=(lay.n_rows, lay.n_rows))

    def oracle(self):
        A, bs = None, []
        for j in range(N_SCEN):
            A, b = OF.assemble_reference_fe(self.F, self.nodal[j], f=self.f[j], R=self.R)
            bs.append(b)
        lu = spla.splu(A.tocsc())
        return np.stack([lu.solve(b) for b in bs])


_models = {}


def model(case, km):
    """Built once per (case, degrees) and read only: (the model, its factors, the 7 columns'
    one-pass solutions)."""
    key = (case, km)
    if key not in _models:
        s = _Model(case, *km)
        fm = cp_cyc_factor_model(s.lay, s.tab, s.R, s.h)
        X = cp_cyc_apply_model(s.lay, s.tab, fm, s.B, s.R, s.h)
        _models[key] = (s, fm, X)
    return _models[key]


# ---- part 1 -----------------------------------------------------------------------------
@pytest.mark.parametrize("case,km", MODEL_CASES)
def test_model_matches_lu(case, km):
    s, fm, X = model(case, km)
    assert fm["ok"] and fm["ns"] == np.asarray(s.tab.cslot).size // 2 > 0
    # the inverse is one: cap inv = I to rounding
    eye = fm["cap"] @ fm["inv"]
    assert np.abs(eye - np.eye(fm["ns"])).max() <= 1e-9
    x_ref = s.oracle()
    worst_e = worst_1 = worst_2 = 0.0
    for j in range(N_SCEN):
        if j == ZERO:
            assert not s.B[j].any() and not X[j].any()  # b = 0: exact zeros
            continue
        nb = np.linalg.norm(s.B[j])
        r1 = np.linalg.norm(s.B[j] - s.A @ X[j]) / nb
        x = X[j]
        if r1 > RES_TOL:  # the batch's one outer refinement pass
            r = s.B[j] - s.A @ x
            x = x + cp_cyc_apply_model(s.lay, s.tab, fm, r[None, :], s.R, s.h)[0]
        r2 = np.linalg.norm(s.B[j] - s.A @ x) / nb
        e = np.linalg.norm(x[s.dev] - x_ref[j]) / np.linalg.norm(x_ref[j])
        worst_e, worst_1, worst_2 = max(worst_e, e), max(worst_1, r1), max(worst_2, r2)
        assert e <= SOL_TOL, (j, e)
        assert r2 <= RES_TOL, (j, r1, r2)
    print(f"{case} {km}: ns {fm['ns']}, vs LU {worst_e:.2e}, residual one pass {worst_1:.2e}, "
          f"after at most one refinement {worst_2:.2e}")


@pytest.mark.parametrize("case,km", [("edge_info_N10", (2, 1)), ("lattice4x5_N6", (3, 2))])
def test_column_bits_do_not_depend_on_the_batch(case, km):
    s, fm, X = model(case, km)
    for j in (0, 2, ZERO):
        one = cp_cyc_apply_model(s.lay, s.tab, fm, s.B[j:j + 1], s.R, s.h)[0]
        np.testing.assert_array_equal(one, X[j])
    perm = np.array([3, 0, 6, 4, 2, 1, 5])
    np.testing.assert_array_equal(cp_cyc_apply_model(s.lay, s.tab, fm, s.B[perm], s.R, s.h),
                                  X[perm])
    nine = np.concatenate([s.B, s.B[[0, 2]]])
    X9 = cp_cyc_apply_model(s.lay, s.tab, fm, nine, s.R, s.h)
    np.testing.assert_array_equal(X9[:N_SCEN], X)
    np.testing.assert_array_equal(X9[N_SCEN:], X[[0, 2]])


@pytest.mark.parametrize("km", [(2, 1), (3, 2)])
def test_a_forest_gives_the_forest_models_bits(km):
    s = _Model("Y_N4", *km)
    assert np.asarray(s.tab.chord).size == 0
    fm = cp_cyc_factor_model(s.lay, s.tab, s.R, s.h)
    f0 = cp_factor_model(s.lay, build_cp_tables(s.lay, *s.mesh.edges), s.R, s.h)
    assert fm["ns"] == 0
    for key in ("fac", "Se", "Pinv"):
        np.testing.assert_array_equal(fm[key], f0[key])
    np.testing.assert_array_equal(cp_cyc_apply_model(s.lay, s.tab, fm, s.B, s.R, s.h),
                                  cp_apply_model(s.lay, s.tab, f0, s.B, s.R, s.h))


# ---- part 2 -----------------------------------------------------------------------------
@pytest.mark.parametrize("case,km", [("edge_info_N10", (2, 1)), ("edge_info_N10", (4, 3)),
                                     ("lattice4x5_N6", (2, 1)), ("lattice4x5_N6", (3, 2))])
@pytest.mark.parametrize("kind", ["linear", "lsq"])
def test_gradient_through_the_model_matches_cpu_adjoint(case, km, kind):
    s, fm, X = model(case, km)
    lay, tab, F = s.lay, s.tab, s.F
    k, N = km[0], lay.N
    j = 5  # the case's own p_bc with the per-edge source
    chord = int(np.asarray(tab.chord)[0])
    eb = np.asarray(tab.eb).reshape(-1, 4)
    # observed: a chord's interior flux node, the node pressure at a chord end, and seeded rows
    inv_dev = np.empty_like(s.dev)
    inv_dev[s.dev] = np.arange(s.dev.size)
    must = [F.flux_offset[chord] + 1,
            int(inv_dev[np.asarray(tab.nrow).reshape(-1, 2)[eb[chord, 0], 0]])]
    assert F.flux_offset[chord] + 1 < F.flux_offset[chord] + k * N  # an interior flux node
    assert F.p_offset <= must[1] < F.lm_offset
    rng = np.random.default_rng(11)
    rest = rng.choice(np.setdiff1d(np.arange(F.n_dofs), must), size=10, replace=False)
    rows = np.concatenate([must, rest])
    w = 0.5 + rng.random(rows.size)
    data = None if kind == "linear" else rng.standard_normal(rows.size)
    ref = AdjointRefFe(F, s.R).gradient(s.nodal[j], s.f[j], rows, w, data)

    def solve(b):
        x = cp_cyc_apply_model(lay, tab, fm, b[None, :], s.R, s.h)[0]
        return x + cp_cyc_apply_model(lay, tab, fm, (b - s.A @ x)[None, :], s.R, s.h)[0]

    x = solve(s.B[j])
    assert np.linalg.norm(x[s.dev] - ref["x"]) <= 1e-10 * np.linalg.norm(ref["x"])
    xo = x[s.dev[rows]]
    c = np.zeros(lay.n_rows)
    if data is None:
        value = float(np.sum(w * xo))
        c[s.dev[rows]] = w
    else:
        value = 0.5 * float(np.sum(w * (xo - data) ** 2))
        c[s.dev[rows]] = w * (xo - data)
    mu = solve(c)
    gR, gf, gbc = cp_edge_form_model(lay, tab, x, mu, s.h)
    index, sign = edge_boundary_rhs_adjoint(s.mesh, s.edge_ids)
    dp = np.take(gbc.reshape(-1), index) * sign

    def rel(a, b):
        assert np.linalg.norm(b) > 0
        return float(np.linalg.norm(a - b) / np.linalg.norm(b))

    errs = {"value": abs(value - ref["value"]) / abs(ref["value"]), "dR": rel(gR, ref["dR"]),
            "df": rel(gf, ref["df"]), "dp_bc": rel(dp, ref["dp_bc"])}
    print(f"{case} {km} {kind}: " + ", ".join(f"{k_} {v:.2e}" for k_, v in errs.items()))
    assert abs(ref["dR"][chord]) > 0  # the chord contributes through its own rows
    assert max(errs.values()) <= 1e-10, errs


# ---- part 3 -----------------------------------------------------------------------------
class _StubAssembler:
    handle = None


def test_new_symbols_are_declared_and_exported():
    text = HEADER.read_text()
    for name in ("nx_set_cp_batch_cycles", "nx_get_cp_batch_cycles"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert re.search(rf"^int {name}\(nx_network_t\* h,", text, re.M), name
    assert _lib._SIGS["nx_set_cp_batch_cycles"] == _lib._SIGS["nx_set_ensemble_cycles"]
    assert _lib._SIGS["nx_get_cp_batch_cycles"] == _lib._SIGS["nx_get_ensemble_cycles"]
    decl = re.search(r"^int nx_get_cp_batch_cycles\(([^;]*)\);", text, re.M | re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["h", "enabled", "applied",
                                                                    "builds"]


def test_keyword_and_env_switch(monkeypatch):
    p = inspect.signature(Solver.__init__).parameters["batch_continuous_cycles"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    for value, on in ((None, False), ("1", True), ("0", False), ("", False), ("true", False)):
        if value is None:
            monkeypatch.delenv("NXHIP_CP_BATCH_CYCLES", raising=False)
        else:
            monkeypatch.setenv("NXHIP_CP_BATCH_CYCLES", value)
        assert Solver(_StubAssembler())._cp_batch_cycles is on
        assert Solver(_StubAssembler(), batch_continuous_cycles=True)._cp_batch_cycles is True
        # an explicit False overrides the environment
        assert Solver(_StubAssembler(), batch_continuous_cycles=False)._cp_batch_cycles is False
        # neither of the other options switches it on, nor it them
        assert Solver(_StubAssembler(), batch_continuous=True)._cp_batch_cycles is on
        assert Solver(_StubAssembler(), batch_continuous_cycles=True)._cp_batch is False


def test_configure_follows_the_handles_own_state():
    """``_configure`` sets the switch where this solver wants it and takes it back where the
    handle itself reports it on -- two solvers on one assembler each get their own, and a call
    made on the handle directly is seen."""
    class H:
        def __init__(self):
            self.on = False
            self.told = []

        def pc_exact(self):
            return True

        def set_ensemble_cycles(self, enable):
            pass

        def set_cp_batch_cycles(self, enable):
            self.told.append(enable)
            self.on = enable

        def cp_batch_cycles_info(self):
            return {"enabled": self.on, "applied": False, "builds": 0}

    class A:
        preconditioned = True
        fe_direct_available = True

        def __init__(self):
            self.handle = H()

        def set_direct(self, on):
            pass

    asm = A()
    on = Solver(asm, batch_continuous=True, batch_continuous_cycles=True)
    off = Solver(asm, batch_continuous=True)
    off._configure()
    Solver(asm, batch_continuous_cycles=True)._configure()  # (alone it changes nothing)
    assert asm.handle.told == []
    on._configure()
    assert asm.handle.told == [True] and asm.handle.on
    off._configure()
    off._configure()
    assert asm.handle.told == [True, False]
    asm.handle.on = True  # (set on the handle directly)
    off._configure()
    assert asm.handle.told == [True, False, False] and not asm.handle.on
