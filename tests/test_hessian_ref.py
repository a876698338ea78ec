"""The CPU Hessian-vector product (tests/hessian_ref.py) before it is trusted as the yardstick of
tests/test_gpu_hvp.py: central differences of ``AdjointRef.gradient`` along the direction, the
symmetry of H, the positive semidefinite Gauss-Newton product and the two homogeneity identities.

Central differences: ``(g(theta + eps v) - g(theta - eps v)) / (2 eps)`` at ``eps = 1e-5`` with
``theta = (R, p_bc, f)`` and a fixed-seed random ``v`` in all three parts, per block as
``max |Hv - fd| / max |fd|``. Measured worst figure over the cases below (both kinds, all three
blocks): MEASURED = 4.02e-10 (Y_N4 linear Hdf); per case Y_N4 4.0e-10, tree5_N15 1.8e-10,
edge_info_N10 2.9e-10. The bar is ten times that (rounded up) and may never exceed 1e-7."""

import numpy as np
import pytest

from cases import CASES, CYCLIC, p_y
from hessian_ref import HessianRef
from networks_fenicsx_amd import NetworkMesh
from oracle import nx_oracle as O

MEASURED = 4.02e-10
BAR = 4.1e-9
assert 10 * MEASURED <= BAR <= 1e-7
EPS = 1e-5
GRAPHS = ["Y_N4", "tree5_N15", "edge_info_N10"]

_CACHE = {}


def _setup(case):
    if case not in _CACHE:
        if case in CASES:
            make, N, strategy, pbc = CASES[case]
        else:
            (make, N), strategy, pbc = CYCLIC[case], None, p_y
        m = NetworkMesh(make(), N=N, color_strategy=strategy)
        src, dst = m.edges
        P = O.build_problem(m.node_coordinates, src, dst, N, m.edge_colors)
        E = m.num_edges
        R = 0.5 + (np.arange(E) % 3) / 2.0
        f = 0.1 + 0.02 * (np.arange(E) % 5)
        pb = np.asarray(pbc(P.pos3.T.copy()), dtype=np.float64)
        rng = np.random.default_rng(5)
        blocks = [(0, P.p_offset, 5), (P.p_offset, P.lm_offset, 4), (P.lm_offset, P.n_dofs, 3)]
        rows = np.concatenate([lo + rng.choice(hi - lo, size=min(k, hi - lo), replace=False)
                               for lo, hi, k in blocks])
        w = 0.5 + rng.random(rows.size)
        data = rng.standard_normal(rows.size)
        dirs = []
        for _ in range(2):
            v_p = np.zeros(pb.size)
            bnd = np.concatenate([P.leaf_in, P.root_out])
            v_p[bnd] = rng.standard_normal(bnd.size)
            dirs.append((rng.standard_normal(E), v_p, rng.standard_normal(E)))
        _CACHE[case] = (P, R, f, pb, rows, w, data, dirs, HessianRef(P, R))
    return _CACHE[case]


def _flat(h):
    return np.concatenate([h["HdR"], h["Hdp_bc"], h["Hdf"]])


@pytest.mark.parametrize("case", GRAPHS)
@pytest.mark.parametrize("kind", ["linear", "lsq"])
def test_hvp_matches_central_differences(case, kind):
    P, R, f, pb, rows, w, data, dirs, ref = _setup(case)
    d = None if kind == "linear" else data
    v_R, v_p, v_f = dirs[0]
    h = ref.hvp(pb, f, rows, w, d, v_R=v_R, v_p=v_p, v_f=v_f)
    gp = HessianRef(P, R + EPS * v_R).gradient(pb + EPS * v_p, f + EPS * v_f, rows, w, d)
    gm = HessianRef(P, R - EPS * v_R).gradient(pb - EPS * v_p, f - EPS * v_f, rows, w, d)
    for name, g in (("HdR", "dR"), ("Hdf", "df"), ("Hdp_bc", "dp_bc")):
        fd = (gp[g] - gm[g]) / (2 * EPS)
        assert np.abs(fd).max() > 0.0
        err = np.abs(h[name] - fd).max() / np.abs(fd).max()
        print(f"{case} {kind} {name}: {err:.2e} of max|fd|")
        assert err <= BAR, (name, err)


@pytest.mark.parametrize("case", GRAPHS)
@pytest.mark.parametrize("kind", ["linear", "lsq"])
def test_hessian_is_symmetric(case, kind):
    P, R, f, pb, rows, w, data, dirs, ref = _setup(case)
    d = None if kind == "linear" else data
    (uR, up, uf), (vR, vp, vf) = dirs
    Hu = _flat(ref.hvp(pb, f, rows, w, d, v_R=uR, v_p=up, v_f=uf))
    Hv = _flat(ref.hvp(pb, f, rows, w, d, v_R=vR, v_p=vp, v_f=vf))
    u, v = np.concatenate([uR, up, uf]), np.concatenate([vR, vp, vf])
    a, b = float(u @ Hv), float(v @ Hu)
    scale = np.linalg.norm(u) * np.linalg.norm(Hv) + np.linalg.norm(v) * np.linalg.norm(Hu)
    print(f"{case} {kind}: u.Hv {a:.15e}, v.Hu {b:.15e}, rel {abs(a - b) / scale:.1e}")
    assert abs(a - b) <= 1e-12 * scale


@pytest.mark.parametrize("case", GRAPHS)
def test_gauss_newton_is_positive_semidefinite(case):
    P, R, f, pb, rows, w, data, dirs, ref = _setup(case)
    for vR, vp, vf in dirs:
        h = ref.hvp(pb, f, rows, w, data, v_R=vR, v_p=vp, v_f=vf, gauss_newton=True)
        assert h["dR"] is None
        q = float(np.concatenate([vR, vp, vf]) @ _flat(h))
        # v^T J^T W J v written out: the same number from the tangent alone
        direct = float(np.sum(w * h["xdot"][rows] ** 2))
        print(f"{case}: v.H_GN v = {q:.6e}, sum w xdot^2 = {direct:.6e}")
        assert q >= 0.0
        assert q == pytest.approx(direct, rel=1e-10)
    with pytest.raises(ValueError):
        ref.hvp(pb, f, rows, w, None, v_R=dirs[0][0], gauss_newton=True)


@pytest.mark.parametrize("case", GRAPHS)
def test_homogeneity_in_R(case):
    """f = 0: the fluxes are homogeneous of degree -1 in R, the pressures and multipliers of
    degree 0, so for the linear objective and v = (R, 0, 0): flux rows observed alone give
    HR = -2 gR, pressure rows alone HR = -gR."""
    P, R, f, pb, rows, w, data, dirs, ref = _setup(case)
    zero_f = np.zeros_like(f)
    flux = rows[rows < P.p_offset]
    pres = rows[(rows >= P.p_offset) & (rows < P.lm_offset)]
    for sel, factor in ((flux, 2.0), (pres, 1.0)):
        ws = np.ones(sel.size)
        h = ref.hvp(pb, zero_f, sel, ws, None, v_R=R)
        assert np.linalg.norm(h["dR"]) > 0.0
        err = np.linalg.norm(h["HdR"] + factor * h["dR"]) / np.linalg.norm(factor * h["dR"])
        print(f"{case} factor {factor}: {err:.2e}")
        assert err <= 1e-12
