"""Host side of the (k, 0) adjoint gradient: the C ABI's new entry (header and ctypes table) and
``Solver.gradient``'s routing with the handle stubbed (no device) -- the new route engages only
with ``batch_degrees`` on degrees (k, 0), k >= 2, and everything it does not serve still raises
``NotImplementedError``. Before it, the contraction's model: a numpy restatement of
``k_fe_b_edge_form`` through the row maps the device gets, held to the general-degree CPU adjoint
on a binary tree and on the forests of tests/tree_shapes.py (``test_model_matches_cpu_adjoint``)."""

import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from cases import CASES
from gradient_ref_fe import AdjointRefFe
from networks_fenicsx_amd import NetworkMesh, Solver, _lib
from networks_fenicsx_amd.assembly import batch_coefficients, edge_boundary_rhs_adjoint
from networks_fenicsx_amd.element import element_tensors
from networks_fenicsx_amd.layout import build_local_problem
from networks_fenicsx_amd.layout_fe import build_fe_aux_maps, build_fe_layout, evaluate_terms
from oracle import nx_oracle as O
from oracle import nx_oracle_fe as OF
from tree_shapes import FE_N_CAP, SHAPES, coefficients, p_xy, reversed_edges

HEADER = Path(__file__).resolve().parent.parent / "include" / "nxhip.h"
E, NODES, ROWS = 3, 4, 20


class _StubHandle:
    n_rows = ROWS

    def __init__(self, fe_ok=True):
        self.calls = []
        self._fe_ok = fe_ok

    def pc_exact(self):
        return True

    def set_ensemble_cycles(self, enable):
        pass

    def batch_supported(self):
        return False

    def fe_batch_supported(self):
        return self._fe_ok

    def batch_info(self):
        return {"launches": 0, "refined": 0, "fallback": 0, "chunk": 1}

    def fe_batch_gradient(self, edge_bc, edge_f, f_const, rtol, maxit, *, rows, weights, data):
        B = edge_bc.shape[0]
        self.calls.append(dict(rows=np.asarray(rows), rtol=rtol, maxit=maxit, data=data))
        gR = np.tile(np.arange(E, dtype=float), (B, 1))
        gbc = np.arange(B * E * 2, dtype=float).reshape(B, E, 2)
        one = np.ones((B, 2))
        return np.zeros(B), gR, gbc, gR + 10.0, one.astype(np.int32), 0 * one, one.astype(bool)

    def batch_gradient(self, *a, **kw):
        raise AssertionError("the P1/DG0 entry point on a (k, 0) system")

    ensemble_gradient = batch_hvp = batch_gradient


class _StubAssembler:
    """What ``Solver.gradient`` reads of the assembler, for degrees ``deg``."""

    preconditioned = True
    fe_direct_available = True
    lhs_current = True
    _coefficients = object()

    def __init__(self, deg, nranks=1, fe_ok=True):
        self.degrees = deg
        self._nranks = nranks
        self.handle = _StubHandle(fe_ok)

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


# ---- the contraction's model ---------------------------------------------------------------
MODEL_BAR = 1e-10  # tests/test_cp_gradient_host.py's: two solves at the oracle's bar
MODEL_CASES = [("Y_N4", 2), ("Y_N4", 3)] + [(n, k) for n in ("hub5", "broom33", "cat70",
                                                             "hubhub5x5", "rand200_s1")
                                            for k in (2, 3)]


def fe_edge_form_model(lay, maps, x, mu, cell_h):
    """numpy restatement of ``k_fe_b_edge_form`` (``nx_fe_batch_gradient``'s contraction) from
    the row maps the device gets (``layout_fe.build_fe_aux_maps``: ``v_fe`` the vertex flux
    rows, ``i_fe`` the interior flux rows, ``p_fe`` the pressure rows): ``x`` the forward and
    ``mu`` the adjoint column in device rows; per edge over its cells c

    * ``gR[e] = -sum_c h_c mu_c^T M x_c`` -- the cell's left vertex, k - 1 interior nodes and
      right vertex, ``M`` the reference mass (``element_tensors(k, 0)``);
    * ``gf[e] = -sum_c h_c mu[p_c]`` (DG0: the source enters a cell's pressure row as -f h);
    * ``gbc[e] = mu`` at the edge's first and last vertex row."""
    E, N, k = lay.E, lay.N, lay.k
    km = k - 1
    M = np.asarray(element_tensors(k, 0)[0], dtype=np.float64).reshape(k + 1, k + 1)
    vfe = np.asarray(maps.v_fe, dtype=np.int64).reshape(E, N + 1)
    ife = np.asarray(maps.i_fe, dtype=np.int64).reshape(E, N, km)
    pfe = np.asarray(maps.p_fe, dtype=np.int64).reshape(E, N)
    h = np.asarray(cell_h, dtype=np.float64).reshape(E, N)
    gR, gf, gbc = np.zeros(E), np.zeros(E), np.zeros((E, 2))
    for e in range(E):
        for c in range(N):
            rows = np.concatenate([vfe[e, c:c + 1], ife[e, c], vfe[e, c + 1:c + 2]])
            gR[e] -= h[e, c] * float(mu[rows] @ (M @ x[rows]))
            gf[e] -= h[e, c] * float(mu[pfe[e, c]])
        gbc[e] = mu[vfe[e, 0]], mu[vfe[e, N]]
    return gR, gf, gbc


@pytest.mark.parametrize("case,k", MODEL_CASES)
@pytest.mark.parametrize("kind", ["linear", "lsq"])
def test_model_matches_cpu_adjoint(case, k, kind):
    """The (k, 0) counterpart of tests/test_cp_gradient_host.py's model test: the device matrix
    of the (k, 0) layout is symmetric, so the adjoint is a second solve with it on ``k_b_obs``'s
    right-hand side (here SuperLU on the host evaluation of the term tables: the condensed
    sweeps are tests/test_gpu_fe_batch.py's subject); the numpy restatement of the contraction
    through ``nx_fe_set_direct``'s row maps is held against the general-degree CPU adjoint --
    value, dR, df and dp_bc to 1e-10 relative. Y_N4 and the forests of tests/tree_shapes.py
    (N <= 6; the shape's own R, else R = 1) on which tests/test_gpu_fe_shapes.py runs the
    device: junctions of up to 34 multiplier rows, edges pointing into their parent, the
    seeded two-decade R -- a failure there on the device is then the kernel's."""
    if case in SHAPES:
        make, N, _ = SHAPES[case]
        N, strategy, pbc = min(N, FE_N_CAP), None, p_xy
    else:
        make, N, strategy, pbc = CASES[case]
    mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
    src, dst = mesh.edges
    pos = np.asarray(mesh.node_coordinates, dtype=np.float64)
    lay = build_fe_layout(pos, src, dst, mesh.degrees, N, k, 0)
    lp = build_local_problem(pos, src, dst, mesh.degrees, N, 0, 1)
    maps = build_fe_aux_maps(lay, lp)
    F = OF.build_problem_fe(pos, src, dst, N, k, 0, mesh.edge_colors)
    assert F.n_dofs == lay.n_rows
    E = mesh.num_edges
    if case in SHAPES:
        R = np.asarray(coefficients(case, E).get("R", np.ones(E)), dtype=np.float64)
        rev = reversed_edges(src, dst, mesh.degrees)
        assert (rev >= 3).sum() >= 20 or case in ("hub5", "broom33"), rev
        assert (R.max() / R.min() > 30.0) == (case in ("hubhub5x5", "rand200_s1"))
        if case == "broom33":
            assert int(np.max(mesh.degrees)) == 34  # 34 multiplier rows at one junction
    else:
        R = 0.5 + (np.arange(E) % 3) / 2.0
    f = 0.1 + 0.02 * (np.arange(E) % 5)
    pb = np.asarray(pbc(F.base.pos3.T.copy()), dtype=np.float64)
    _, h = O.cell_geometry(F.base)
    dev = np.empty(F.n_dofs, dtype=np.int64)  # reference block order -> device rows
    nf = k * N + 1
    for e in range(E):
        dev[F.flux_offset[e]:F.flux_offset[e] + nf] = lay.flux_rows[e]
    dev[F.p_offset:F.lm_offset] = lay.p_rows
    dev[F.lm_offset:] = lay.lm_rows
    assert np.array_equal(np.sort(dev), np.arange(F.n_dofs))
    edge_ids = np.arange(E)
    bc, ef, _ = batch_coefficients(mesh, edge_ids, pb[None, :], f[None, :])
    val, rhs = evaluate_terms(lay, R, ef[0], bc[0], h)
    A = sp.csr_matrix((val, lay.col, lay.rowptr), shape=(lay.n_rows, lay.n_rows))
    assert abs(A - A.T).max() == 0.0 and abs(A).max() > 0

    rng = np.random.default_rng(11)
    rows = rng.choice(F.n_dofs, size=min(12, F.n_dofs), replace=False)
    assert (rows < F.p_offset).any() and (rows >= F.p_offset).any()
    w = 0.5 + rng.random(rows.size)
    data = None if kind == "linear" else rng.standard_normal(rows.size)
    ref = AdjointRefFe(F, R).gradient(pb, f, rows, w, data)

    lu = spla.splu(A.tocsc())
    x = lu.solve(rhs)
    assert np.linalg.norm(x[dev] - ref["x"]) <= MODEL_BAR * np.linalg.norm(ref["x"])
    xo = x[dev[rows]]
    c = np.zeros(lay.n_rows)
    if data is None:
        value = float(np.sum(w * xo))
        c[dev[rows]] = w
    else:
        value = 0.5 * float(np.sum(w * (xo - data) ** 2))
        c[dev[rows]] = w * (xo - data)
    mu = lu.solve(c)
    gR, gf, gbc = fe_edge_form_model(lay, maps, x, mu, h)
    index, sign = edge_boundary_rhs_adjoint(mesh, edge_ids)
    dp = np.take(gbc.reshape(-1), index) * sign

    def rel(a, b):
        assert np.linalg.norm(b) > 0
        return float(np.linalg.norm(a - b) / np.linalg.norm(b))

    errs = {"value": abs(value - ref["value"]) / abs(ref["value"]), "dR": rel(gR, ref["dR"]),
            "df": rel(gf, ref["df"]), "dp_bc": rel(dp, ref["dp_bc"])}
    print(f"{case} k={k} {kind}: " + ", ".join(f"{q} {v:.2e}" for q, v in errs.items()))
    assert max(errs.values()) <= MODEL_BAR, errs


# ---- the route -------------------------------------------------------------------------------
def test_symbol_is_declared_and_exported():
    text = HEADER.read_text()
    assert "nx_fe_batch_gradient" in _lib.EXPORTED_SYMBOLS
    # nx_batch_gradient's argument list with maxit after rtol
    sig, ref = _lib._SIGS["nx_fe_batch_gradient"][1], _lib._SIGS["nx_batch_gradient"][1]
    assert len(sig) == len(ref) + 1 and sig[:6] == ref[:6] and sig[7:] == ref[6:]
    decl = re.search(r"^int nx_fe_batch_gradient\(([^;]*)\);", text, re.M | re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == [
        "h", "n_cols", "edge_bc", "edge_f", "f_const", "rtol", "maxit", "kind", "n_obs",
        "obs_rows", "obs_w", "obs_d", "value", "grad_R", "grad_bc", "grad_f", "iters", "relres",
        "converged"]


@pytest.mark.parametrize("k", [2, 3])
def test_route_engages_with_batch_degrees(k):
    asm = _StubAssembler((k, 0))
    solver = Solver(asm, batch_degrees=True, petsc_options={"ksp_rtol": 1e-11, "ksp_max_it": 77})
    g = solver.gradient([None, None], **KW)
    (call,) = asm.handle.calls
    np.testing.assert_array_equal(call["rows"], asm.block_order_rows()[KW["rows"]])
    assert call["rtol"] == 1e-11 and call["maxit"] == 77 and call["data"] is None
    # the host gathers: edge slots -> graph.edges() order, flux end rows -> boundary nodes
    np.testing.assert_array_equal(g.dR, np.tile([2.0, 1.0, 0.0], (2, 1)))
    np.testing.assert_array_equal(g.df, g.dR + 10.0)
    np.testing.assert_array_equal(g.dp_bc, [[-0.0, 5.0, 0.0, 0.0], [-6.0, 11.0, 0.0, 0.0]])
    assert g.iterations.shape == (2, 2) and g.converged.all()
    g = solver.gradient([None], data=np.array([0.5, 0.25]), **KW)
    assert asm.handle.calls[-1]["data"].shape == (1, 2)


def test_env_switch_engages_the_route(monkeypatch):
    monkeypatch.setenv("NXHIP_FE_BATCH", "1")
    asm = _StubAssembler((2, 0))
    Solver(asm).gradient([None], **KW)
    assert len(asm.handle.calls) == 1


def test_without_batch_degrees_it_still_raises(monkeypatch):
    monkeypatch.delenv("NXHIP_FE_BATCH", raising=False)
    for solver in (Solver(_StubAssembler((2, 0))),
                   Solver(_StubAssembler((2, 0)), batch_degrees=False)):
        with pytest.raises(NotImplementedError, match="degrees") as err:
            solver.gradient([None], **KW)
        assert "batch_degrees" in str(err.value)
        assert not solver.assembler.handle.calls


def test_what_the_route_does_not_serve():
    def solver(deg=(2, 0), opts=None, **kw):
        return Solver(_StubAssembler(deg, **kw), batch_degrees=True, petsc_options=opts)

    with pytest.raises(NotImplementedError, match="ensemble"):
        solver().gradient([None], R=np.ones((1, E)), **KW)
    with pytest.raises(NotImplementedError, match="degrees"):
        solver().hessian_vector([None], v_R=np.ones(E), **KW)
    for deg in ((2, 1), (3, 2)):  # continuous pressure
        with pytest.raises(NotImplementedError, match="degrees"):
            solver(deg).gradient([None], **KW)
    with pytest.raises(NotImplementedError, match="one rank"):
        solver(nranks=2).gradient([None], **KW)
    for opts, word in (({"ksp_type": "minres"}, "MINRES"), ({"pc_type": "none"}, "pc_type"),
                       ({"pc_mass": "lumped"}, "lumped")):
        with pytest.raises(NotImplementedError, match=word):
            solver(opts=opts).gradient([None], **KW)
    # a (k, 0) handle whose batched condensed solve does not apply (no auxiliary handle)
    with pytest.raises(NotImplementedError, match="nx_fe_batch_supported"):
        solver(fe_ok=False).gradient([None], **KW)
    s = solver()
    with pytest.raises(NotImplementedError, match="derivatives=False"):
        s.gradient([None], derivatives=False, **KW)
    assert not s.assembler.handle.calls
