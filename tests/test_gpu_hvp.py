"""``Solver.hessian_vector`` / ``nx_batch_hvp`` / ``nx_ensemble_hvp``: exact Hessian-vector
products of the observed-row objective in four batched direct solves on the device.

Set-up per graph: that of tests/test_gpu_gradient.py (per-edge R = 0.5 + (e mod 3) / 2, B = 3
scenarios with the per-edge source, about 12 observed rows from the flux, pressure and
multiplier blocks, both kinds of objective) plus two fixed-seed random directions with nonzero
``v_R``, ``v_p_bc`` (on the boundary nodes) and ``v_f`` for every scenario.

Yardstick: the CPU product of tests/hessian_ref.py (SuperLU on the oracle's matrices, itself
held to central differences of the CPU adjoint, to the symmetry of H and to the homogeneity
identities in tests/test_hessian_ref.py). ``HdR``, ``Hdf``, ``Hdp_bc`` (and in full mode
``value``, ``dR``, ``df``, ``dp_bc``) of every scenario are compared as relative 2-norms.

The parity bar: every figure is a product of up to four solves held to 1e-10 each, so the bar is
set from a measurement -- 10x the largest error over all the cases of
test_parity_with_cpu_reference and test_ensemble_distinct_R on an MI355X, never above 1e-8 (a
sign or formula error is O(1)). Measured worst figure per case (full mode in both kinds and
Gauss-Newton, all scenarios and quantities): see PARITY_MEASURED_BY_CASE below."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from cases import CYCLIC
from hessian_ref import HessianRef
from networks_fenicsx_amd import Solver, _lib
from networks_fenicsx_amd.solver import HessianVectorResult
from test_gpu_gradient import Setup, env, rel

pytestmark = pytest.mark.gpu

PARITY_MEASURED_BY_CASE = {  # worst figure of the case on an MI355X
    "demo_tree_N1": 4.6e-15, "Y_N4": 1.3e-14, "tree5_N15": 1.0e-13, "tree5_N16": 7.4e-14,
    "tree5_3d_N31": 2.3e-13, "tree6_2d_N70": 8.6e-13, "long_N300": 3.3e-13,
    "edge_info_N10": 3.9e-13, "lattice6x6_N3": 3.2e-14,
    "tree5_N15 ensemble": 5.5e-13, "tree6_2d_N70 ensemble": 4.891e-12}
PARITY_MEASURED = 4.891e-12  # the largest of them (Gauss-Newton HdR at R_j = 10^U(-1, 1))
PARITY_BAR = 4.9e-11  # 10 x PARITY_MEASURED (rounded up); may never exceed 1e-8
assert PARITY_MEASURED == max(PARITY_MEASURED_BY_CASE.values())
assert 10 * PARITY_MEASURED <= PARITY_BAR <= 1e-8
GRADIENT_BAR = 8.7e-12  # tests/test_gpu_gradient.py's bar on dR

PARITY_CASES = ["demo_tree_N1", "Y_N4", "tree5_N15", "tree5_N16", "tree5_3d_N31", "tree6_2d_N70",
                "long_N300", "edge_info_N10", "lattice6x6_N3"]
H_NAMES = ("HdR", "Hdf", "Hdp_bc")
G_NAMES = ("value", "dR", "df", "dp_bc")


class HvpSetup(Setup):
    """The gradient tests' set-up with two directions per scenario."""

    def __init__(self, name, **asm_kw):
        super().__init__(name, **asm_kw)
        E, nn = self.mesh.num_edges, self.mesh.num_nodes
        rng = np.random.default_rng(23)
        bnd = np.concatenate([self.P.leaf_in, self.P.root_out])
        self.dirs = []
        for _ in range(2):
            v_p = np.zeros((3, nn))
            v_p[:, bnd] = rng.standard_normal((3, bnd.size))
            self.dirs.append(dict(v_R=rng.standard_normal((3, E)), v_p_bc=v_p,
                                  v_f=rng.standard_normal((3, E))))
        self.kw = dict(rows=self.rows, weights=self.w)


_REFS = {}


def cpu_ref(s, R=None):
    """The CPU reference's operators for the graph (computed once per graph and R)."""
    key = (s.name, None if R is None else float(np.sum(R)))
    if key not in _REFS:
        _REFS[key] = HessianRef(s.P, s.R if R is None else R)
    return _REFS[key]


def parity_errors(s, hv, data, d, gauss_newton, R=None):
    """The relative errors of every scenario's blocks against the CPU reference; every
    reference block must be nonzero."""
    out = []
    for j in range(len(hv)):
        ref = cpu_ref(s, None if R is None else R[j])
        r = ref.hvp(s.nodal[j], s.f[j], s.rows, s.w, None if data is None else data[j],
                    v_R=d["v_R"][j], v_p=d["v_p_bc"][j], v_f=d["v_f"][j],
                    gauss_newton=gauss_newton)
        errs = {}
        for name in H_NAMES:
            assert np.linalg.norm(r[name]) > 0.0, name
            errs[name] = rel(getattr(hv, name)[j], r[name])
        if not gauss_newton:
            assert r["value"] != 0.0
            errs["value"] = abs(hv.value[j] - r["value"]) / abs(r["value"])
            for name in G_NAMES[1:]:
                assert np.linalg.norm(r[name]) > 0.0, name
                errs[name] = rel(getattr(hv, name)[j], r[name])
        out.append(errs)
    return out


def assert_same_bits(a, b, j_a, j_b, names=G_NAMES + H_NAMES):
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        if x is None:
            assert y is None, name
            continue
        np.testing.assert_array_equal(x[j_a], y[j_b], err_msg=name)


def steady_launches(cycles, mode, chunks=1):
    """include/nxhip.h, nx_batch_hvp: S = 5 / 7 launches per batched solve pass."""
    S = 7 if cycles else 5
    if mode == "gn":
        return chunks * (3 * S + 6)
    if mode == "linear":
        return (1 + S) + chunks * (3 * S + 7)
    return chunks * (4 * S + 7)  # least squares; both kinds of an ensemble


MODES = (("linear", False, False), ("lsq", True, False), ("gn", True, True))


# 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PARITY_CASES)
def test_parity_with_cpu_reference(name):
    """Every lane shape of k_b_mass_apply* and k_b_edge_form2* (one cell per edge; 4 and 2
    edges per wave and their boundary N = 15 / 16 / 31; two 64-cell chunks; five chunks and an
    edge count that is no multiple of the edges per wave), forests and graphs with cycles."""
    s = HvpSetup(name)
    try:
        solver = Solver(s.asm)
        worst = 0.0
        for mode, lsq, gn in MODES:
            data = s.data if lsq else None
            hv = solver.hessian_vector(s.items, s.f, data=data, gauss_newton=gn, **s.kw,
                                       **s.dirs[0])
            assert isinstance(hv, HessianVectorResult) and len(hv) == 3
            assert hv.converged.all() and hv.info["fallback"] == 0
            assert hv.converged.shape == hv.iterations.shape == (3, 3 if gn else 4)
            assert hv.HdR.shape == hv.Hdf.shape == (3, s.mesh.num_edges)
            assert hv.Hdp_bc.shape == (3, s.mesh.num_nodes) and hv.value.shape == (3,)
            if gn:
                assert hv.dR is None and hv.df is None and hv.dp_bc is None
            for j, errs in enumerate(parity_errors(s, hv, data, s.dirs[0], gn)):
                print(f"{name} {mode} scenario {j}: "
                      + ", ".join(f"{k} {v:.2e}" for k, v in errs.items())
                      + f" (refined {hv.info['refined']})")
                worst = max(worst, *errs.values())
        print(f"{name}: worst {worst:.3e}")
        assert worst <= PARITY_BAR, worst
    finally:
        s.close()


# 2 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Y_N4", "tree5_N16", "tree6_2d_N70", "edge_info_N10"])
def test_gradient_part_has_gradients_bits(name):
    """Full mode: value, dR, df, dp_bc are Solver.gradient's on the same scenarios, bit for bit
    (k_b_edge_form2 against k_b_edge_form, in every lane shape)."""
    s = HvpSetup(name)
    try:
        solver = Solver(s.asm)
        for data in (None, s.data):
            g = solver.gradient(s.items, s.f, data=data, **s.kw)
            hv = solver.hessian_vector(s.items, s.f, data=data, **s.kw, **s.dirs[0])
            assert_same_bits(g, hv, slice(None), slice(None), names=G_NAMES)
            assert g.dR.any() and g.df.any() and g.dp_bc.any()
            np.testing.assert_array_equal(g.residual_norms, hv.residual_norms[:, :2])
    finally:
        s.close()


# 3 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tree5_N15", "tree6_2d_N70", "edge_info_N10"])
def test_homogeneity_in_R(name):
    """f = 0, the linear objective, v = (R, 0, 0): the fluxes are homogeneous of degree -1 in
    R and the pressures of degree 0, so flux rows observed alone give HdR = -2 dR and pressure
    rows alone HdR = -dR -- no CPU reference involved. The product's and the gradient's errors
    add."""
    s = HvpSetup(name)
    try:
        solver = Solver(s.asm)
        f0 = np.zeros_like(s.f)
        P = s.P
        flux = s.rows[s.rows < P.p_offset]
        pres = s.rows[(s.rows >= P.p_offset) & (s.rows < P.lm_offset)]
        assert flux.size and pres.size
        for rows, factor in ((flux, 2.0), (pres, 1.0)):
            hv = solver.hessian_vector(s.items, f0, rows=rows, v_R=s.R)
            for j in range(3):
                assert np.linalg.norm(hv.dR[j]) > 0.0
                err = (np.linalg.norm(hv.HdR[j] + factor * hv.dR[j])
                       / np.linalg.norm(factor * hv.dR[j]))
                print(f"{name} factor {factor} scenario {j}: {err:.2e}")
                assert err <= PARITY_BAR + GRADIENT_BAR, err
    finally:
        s.close()


# 4 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tree5_N16", "tree6_2d_N70", "lattice6x6_N3"])
def test_symmetry(name):
    """u^T H v = v^T H u per scenario over the concatenated blocks (R, p_bc, f), for both kinds
    and the Gauss-Newton product, which is also positive semidefinite."""
    s = HvpSetup(name)
    try:
        solver = Solver(s.asm)
        du, dv = s.dirs

        def flat(d):
            return np.concatenate([d["v_R"], d["v_p_bc"], d["v_f"]], axis=1)

        def flat_h(hv):
            return np.concatenate([hv.HdR, hv.Hdp_bc, hv.Hdf], axis=1)

        u, v = flat(du), flat(dv)
        for mode, lsq, gn in MODES:
            data = s.data if lsq else None
            Hu = flat_h(solver.hessian_vector(s.items, s.f, data=data, gauss_newton=gn, **s.kw,
                                              **du))
            Hv = flat_h(solver.hessian_vector(s.items, s.f, data=data, gauss_newton=gn, **s.kw,
                                              **dv))
            for j in range(3):
                a, b = float(u[j] @ Hv[j]), float(v[j] @ Hu[j])
                scale = (np.linalg.norm(u[j]) * np.linalg.norm(Hv[j])
                         + np.linalg.norm(v[j]) * np.linalg.norm(Hu[j]))
                print(f"{name} {mode} scenario {j}: {abs(a - b) / scale:.2e}")
                assert abs(a - b) <= PARITY_BAR * scale
                if gn:
                    assert float(u[j] @ Hu[j]) > 0.0 and float(v[j] @ Hv[j]) > 0.0
    finally:
        s.close()


# 5 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tree5_N16", "edge_info_N10"])
def test_exact_zeros(name):
    """A zero direction given as arrays of zeros: zero right-hand sides, the tangent and the
    second-order adjoint exactly zero and reported converged, every block of H v exactly 0.
    The linear objective with v_R None: cd = 0 and Ad = 0, so Hdf and Hdp_bc are exactly 0
    while HdR (the tangent's part) is not."""
    s = HvpSetup(name)
    try:
        solver = Solver(s.asm)
        E, nn = s.mesh.num_edges, s.mesh.num_nodes
        zero = dict(v_R=np.zeros((3, E)), v_p_bc=np.zeros((3, nn)), v_f=np.zeros((3, E)))
        for data in (None, s.data):
            hv = solver.hessian_vector(s.items, s.f, data=data, **s.kw, **zero)
            assert not hv.HdR.any() and not hv.Hdf.any() and not hv.Hdp_bc.any()
            assert hv.converged.all() and not hv.residual_norms[:, 2:].any()
            assert hv.dR.any()
        d = s.dirs[0]
        hv = solver.hessian_vector(s.items, s.f, v_p_bc=d["v_p_bc"], v_f=d["v_f"], **s.kw)
        assert not hv.Hdf.any() and not hv.Hdp_bc.any() and hv.HdR.any()
        assert hv.converged.all() and not hv.residual_norms[:, 3].any()
    finally:
        s.close()


# 6 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tree5_N15", "tree6_2d_N70", "lattice6x6_N3"])
def test_column_independence(name):
    """A scenario's bits are the same alone (B = 1), at another position of B = 3, and in the
    partial last chunk under NXHIP_BATCH_CHUNK=2 (chunks 2, 1)."""
    s = HvpSetup(name)
    try:
        solver = Solver(s.asm)
        d = s.dirs[0]
        order = [2, 0, 1]

        def call(idx, data, gn):
            return solver.hessian_vector(
                [s.items[i] for i in idx], s.f[idx], data=None if data is None else data[idx],
                gauss_newton=gn, **s.kw, **{k: v[idx] for k, v in d.items()})

        for mode, lsq, gn in MODES:
            data = s.data if lsq else None
            alone = call([2], data, gn)
            moved = call(order, data, gn)
            with env(NXHIP_BATCH_CHUNK=2):
                chunked = call([0, 1, 2], data, gn)
            assert chunked.info["chunk"] == 2 and moved.info["chunk"] == 3
            assert_same_bits(alone, moved, 0, 0)
            assert_same_bits(alone, chunked, 0, 2)
            assert_same_bits(moved, chunked, 1, 0)
            assert alone.HdR.any() and alone.Hdf.any() and alone.Hdp_bc.any()
    finally:
        s.close()


# 7 ---------------------------------------------------------------------------------------
def test_ensemble_resident_R_has_the_batch_calls_bits():
    """R= with every row the resident R: nx_ensemble_hvp's columns are nx_batch_hvp's."""
    s = HvpSetup("tree5_3d_N31")
    try:
        solver = Solver(s.asm)
        R3 = np.tile(s.R, (3, 1))
        for mode, lsq, gn in MODES:
            data = s.data if lsq else None
            a = solver.hessian_vector(s.items, s.f, data=data, gauss_newton=gn, **s.kw,
                                      **s.dirs[0])
            b = solver.hessian_vector(s.items, s.f, data=data, gauss_newton=gn, R=R3, **s.kw,
                                      **s.dirs[0])
            assert_same_bits(a, b, slice(None), slice(None))
            assert b.info["launches"] == steady_launches(False, "gn" if gn else "lsq")
    finally:
        s.close()


@pytest.mark.parametrize("name", ["tree5_N15", "tree6_2d_N70"])
def test_ensemble_distinct_R(name):
    """Distinct rows R_j = 10^U(-1, 1) on a forest: every scenario against the CPU reference
    at its own R_j."""
    s = HvpSetup(name)
    try:
        solver = Solver(s.asm)
        R = 10.0 ** np.random.default_rng(5).uniform(-1.0, 1.0, (3, s.mesh.num_edges))
        worst = 0.0
        for mode, lsq, gn in MODES:
            data = s.data if lsq else None
            hv = solver.hessian_vector(s.items, s.f, data=data, gauss_newton=gn, R=R, **s.kw,
                                       **s.dirs[0])
            assert hv.converged.all()
            for j, errs in enumerate(parity_errors(s, hv, data, s.dirs[0], gn, R=R)):
                print(f"{name} {mode} scenario {j}: "
                      + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
                worst = max(worst, *errs.values())
        print(f"{name} ensemble: worst {worst:.3e}")
        assert worst <= PARITY_BAR, worst
    finally:
        s.close()


def test_ensemble_on_cycles_is_not_implemented():
    s = HvpSetup("edge_info_N10")
    try:
        with pytest.raises(NotImplementedError, match="ensemble"):
            Solver(s.asm).hessian_vector(s.items, s.f, R=np.tile(s.R, (3, 1)), **s.kw,
                                         **s.dirs[0])
    finally:
        s.close()


# 8 ---------------------------------------------------------------------------------------
def test_handle_state_untouched():
    """solve(), gradient() and solve_many() return identical bits before and after
    hessian_vector calls: the handle's rhs, x and published state are left as they were, and
    the workspace's new part lies behind everything the earlier calls use."""
    s = HvpSetup("tree5_3d_N31")
    try:
        solver = Solver(s.asm)
        solver.assemble()
        x0 = np.concatenate([fn.x.array for fn in solver.solve()])
        v0 = solver.solution_vector().copy()
        g0 = solver.gradient(s.items, s.f, data=s.data, **s.kw)
        m0 = solver.solve_many(s.items, s.f).x.copy()
        for gn in (False, True):
            solver.hessian_vector(s.items, s.f, data=s.data, gauss_newton=gn, **s.kw,
                                  **s.dirs[0])
        np.testing.assert_array_equal(solver.solution_vector(), v0)
        g1 = solver.gradient(s.items, s.f, data=s.data, **s.kw)
        for name in G_NAMES:
            np.testing.assert_array_equal(getattr(g1, name), getattr(g0, name), err_msg=name)
        np.testing.assert_array_equal(solver.solve_many(s.items, s.f).x, m0)
        x1 = np.concatenate([fn.x.array for fn in solver.solve()])
        np.testing.assert_array_equal(x1, x0)
    finally:
        s.close()


# 9 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tree5_N16", "edge_info_N10"])
def test_launch_counts(name):
    """A call that finds everything current launches the header's steady count when nothing is
    refined, whatever B is inside a chunk and whichever direction parts are given."""
    s = HvpSetup(name)
    cyc = name in CYCLIC
    try:
        solver = Solver(s.asm)
        solver.hessian_vector(s.items, s.f, **s.kw, **s.dirs[0])  # (makes everything current)
        for mode, lsq, gn in MODES:
            data = s.data if lsq else None
            for B in (1, 3):
                d = {k: v[:B] for k, v in s.dirs[0].items()}
                hv = solver.hessian_vector(s.items[:B], s.f[:B], gauss_newton=gn,
                                           data=None if data is None else data[:B], **s.kw, **d)
                print(f"{name} {mode} B={B}: {hv.info}")
                assert hv.info["refined"] == 0 and hv.info["chunk"] == B
                assert hv.info["launches"] == steady_launches(cyc, mode)
            only_f = solver.hessian_vector(s.items, s.f, data=data, gauss_newton=gn,
                                           v_f=s.dirs[0]["v_f"], **s.kw)
            assert only_f.info["launches"] == steady_launches(cyc, mode)
            with env(NXHIP_BATCH_CHUNK=2):
                hv = solver.hessian_vector(s.items, s.f, data=data, gauss_newton=gn, **s.kw,
                                           **s.dirs[0])
            assert hv.info["chunk"] == 2
            assert hv.info["launches"] == steady_launches(cyc, mode, 2)
        assert steady_launches(False, "lsq") == 27 and steady_launches(True, "lsq") == 35
        assert steady_launches(False, "gn") == 21 and steady_launches(True, "linear") == 36
    finally:
        s.close()


# 10 --------------------------------------------------------------------------------------
def test_errors():
    s = HvpSetup("Y_N4")
    try:
        solver = Solver(s.asm)
        d = s.dirs[0]
        E = s.mesh.num_edges
        with pytest.raises(ValueError, match="gauss_newton"):
            solver.hessian_vector(s.items, s.f, gauss_newton=True, **s.kw, **d)
        with pytest.raises(ValueError, match="direction"):
            solver.hessian_vector(s.items, s.f, **s.kw)
        with pytest.raises(ValueError, match="v_R"):
            solver.hessian_vector(s.items, s.f, v_R=np.ones((2, E)), **s.kw)
        with pytest.raises(ValueError, match="v_p_bc"):
            solver.hessian_vector(s.items, s.f, v_p_bc=np.ones(s.mesh.num_nodes + 1), **s.kw)
        with pytest.raises(ValueError, match="v_f"):
            solver.hessian_vector(s.items, s.f, v_f=np.ones((3, E + 1)), **s.kw)
        with pytest.raises(ValueError, match="distinct"):
            solver.hessian_vector(s.items, s.f, rows=np.array([1, 2, 1]), **d)
        with pytest.raises(ValueError, match="data must be"):
            solver.hessian_vector(s.items, s.f, data=np.zeros((2, s.rows.size)), **s.kw, **d)
        for opts, word in (({"ksp_type": "minres"}, "MINRES"), ({"pc_type": "none"}, "pc_type"),
                           ({"pc_mass": "lumped"}, "lumped")):
            with pytest.raises(NotImplementedError, match=word):
                Solver(s.asm, petsc_options=opts).hessian_vector(s.items, s.f, **s.kw, **d)
    finally:
        s.close()
    s = HvpSetup("Y_N4", flux_degree=2, pressure_degree=0)
    try:
        with pytest.raises(NotImplementedError, match="degrees"):
            Solver(s.asm).hessian_vector(s.items, s.f, rows=np.array([0, 1]), **s.dirs[0])
    finally:
        s.close()


def test_c_abi_argument_errors():
    """nx_batch_hvp's NX_ERR_ARG cases, through the ctypes binding."""
    s = HvpSetup("Y_N4")
    try:
        solver = Solver(s.asm)
        solver.gradient(s.items, s.f, rows=s.rows)  # (the handle configured and assembled)
        h = s.asm.handle
        E = h.n_edges
        edge_bc, _, _ = s.asm.scenario_coefficients(s.items[:1], None)
        bc = np.ascontiguousarray(edge_bc)
        value, hR, vR = np.zeros(1), np.zeros(E), np.ones(E)
        pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)

        def call(kind=0, d=None, dir_R=vR, dir_f=None, gn=0, hR=hR, value=value):
            rows = np.asarray((0, 1), dtype=np.int32)
            w = np.ones(2)
            p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
            return _lib.lib().nx_batch_hvp(
                h.ptr, 1, p(bc, pd), None, None, 1e-12, kind, 2, p(rows, pi), p(w, pd), p(d, pd),
                p(dir_R, pd), None, p(dir_f, pd), gn, p(value, pd), None, None, None, p(hR, pd),
                None, None, None, None, None)

        assert call() == _lib.NX_OK  # (every optional output and the status arrays NULL)
        assert hR.any()
        assert call(dir_R=None, dir_f=vR) == _lib.NX_OK
        assert call(dir_R=None) == _lib.NX_ERR_ARG  # no direction at all
        assert call(gn=1) == _lib.NX_ERR_ARG  # Gauss-Newton with the linear objective
        assert call(gn=2, kind=1, d=np.zeros(2)) == _lib.NX_ERR_ARG
        assert call(kind=1, d=None) == _lib.NX_ERR_ARG
        assert call(kind=2) == _lib.NX_ERR_ARG
        assert call(hR=None) == _lib.NX_ERR_ARG
        assert call(value=None) == _lib.NX_ERR_ARG
        assert call(kind=1, d=np.zeros(2), gn=1) == _lib.NX_OK
        # nx_ensemble_hvp without edge_R
        assert _lib.lib().nx_ensemble_hvp(
            h.ptr, 1, None, bc.ctypes.data_as(pd), None, None, 1e-12, 0, 2, None, None, None,
            None, None, None, 0, None, None, None, None, None, None, None, None, None,
            None) == _lib.NX_ERR_ARG
    finally:
        s.close()
