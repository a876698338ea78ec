"""The general-degree CPU adjoint (tests/gradient_ref_fe.py) against central finite differences
of the oracle's own forward solve, before it is trusted as the yardstick of
tests/test_gpu_fe_gradient.py.

Differences in every ``R_e`` (step ``1e-5 R_e``), every boundary node's ``p_bc`` and every
``f_e`` (step ``1e-3``: x is linear in both, so J is at most quadratic and the central
difference has no truncation error). Bar: 1e-7 of ``max |g|`` per gradient, the bar of
tests/test_gradient_ref.py (observed over these eight cases: 2.8e-10 for dR, 8.2e-12 for df,
5.5e-13 for dp_bc).

The same recipe on forests that are not binary (``tree_shapes.FD_SHAPES``: hub(5) at N = 3,
broom(5), caterpillar(7) and hubhub(2, 2) with the seeded R = 10^U(-1, 1) at N = 2), on which
the adjoint is the yardstick of tests/test_gpu_fe_shapes.py."""

import numpy as np
import pytest

from cases import CASES, CYCLIC, p_y
from gradient_ref_fe import AdjointRefFe, forward_fe, objective
from networks_fenicsx_amd import NetworkMesh
from oracle import nx_oracle_fe as OF
from tree_shapes import (FD_SHAPES, K_CP_REC_CH, K_CP_REC_INC, fd_shape, p_xy, reversed_edges)

BAR = 1e-7


def _setup(case, k):
    if case in CASES:
        make, N, strategy, pbc = CASES[case]
    else:
        (make, N), strategy, pbc = CYCLIC[case], None, p_y
    m = NetworkMesh(make(), N=N, color_strategy=strategy)
    src, dst = m.edges
    P = OF.build_problem_fe(m.node_coordinates, src, dst, N, k, 0, m.edge_colors)
    E = m.num_edges
    R = 0.5 + (np.arange(E) % 3) / 2.0
    f = 0.1 + 0.02 * (np.arange(E) % 5)
    pb = np.asarray(pbc(P.base.pos3.T.copy()), dtype=np.float64)
    return P, R, f, pb


def fd_check(P, R, f, pb, kind, tag):
    """The recipe of this module's docstring on one problem: the adjoint's value and its three
    gradients against central differences of ``forward_fe``, each to BAR of ``max |g|``; every
    boundary node is differentiated (``leaf_in``: an edge's target, ``root_out``: its source)."""
    rng = np.random.default_rng(3)
    rows = rng.choice(P.n_dofs, size=12, replace=False)
    w = 0.5 + rng.random(12)
    data = None if kind == "linear" else rng.standard_normal(12)
    g = AdjointRefFe(P, R).gradient(pb, f, rows, w, data)

    def J(pb_, f_, R_):
        return objective(forward_fe(P, pb_, f_, R_), rows, w, data)

    assert g["value"] == pytest.approx(J(pb, f, R), rel=1e-13, abs=1e-15)
    E = P.base.src.size
    fd_R = np.zeros(E)
    fd_f = np.zeros(E)
    for e in range(E):
        d = np.zeros(E)
        d[e] = 1e-5 * R[e]
        fd_R[e] = (J(pb, f, R + d) - J(pb, f, R - d)) / (2 * d[e])
        d[e] = 1e-3
        fd_f[e] = (J(pb, f + d, R) - J(pb, f - d, R)) / 2e-3
    fd_p = np.zeros(pb.size)
    for v in np.concatenate([P.base.leaf_in, P.base.root_out]):
        d = np.zeros(pb.size)
        d[v] = 1e-3
        fd_p[v] = (J(pb + d, f, R) - J(pb - d, f, R)) / 2e-3
    errs = {}
    for name, fd in (("dR", fd_R), ("df", fd_f), ("dp_bc", fd_p)):
        assert np.abs(fd).max() > 0, name
        errs[name] = err = np.abs(g[name] - fd).max() / np.abs(fd).max()
        print(f"{tag} {kind} {name}: {err:.2e} of max|g|")
        assert err <= BAR, (name, err)
    return g, fd_p, errs


def shape_setup(name, k, m):
    """An ``FD_SHAPES`` forest at degrees (k, m): its R and f (``tree_shapes.fd_shape``) and
    p_bc = ``p_xy``. Asserted: a hub or broom node past both record caps of the continuous-
    pressure node forest where the shape is there for one, and -- where the shape has edges
    pointing into their parent -- a boundary node that is the SOURCE of such an edge besides
    node 0 (its p_bc enters the right-hand side with the other sign), which ``fd_check``
    differentiates with the others."""
    G, N, R, f = fd_shape(name)
    mesh = NetworkMesh(G, N=N)
    src, dst = mesh.edges
    assert mesh.num_edges <= 16
    P = OF.build_problem_fe(mesh.node_coordinates, src, dst, N, k, m, mesh.edge_colors)
    pb = np.asarray(p_xy(P.base.pos3.T.copy()), dtype=np.float64)
    rev = reversed_edges(src, dst, mesh.degrees)
    deg = int(np.max(mesh.degrees))
    if name.startswith(("hub5", "broom5")):  # 6 incident edges, 5 children: past both caps
        assert deg == 6 and deg > K_CP_REC_INC and deg - 1 > K_CP_REC_CH
    if name.startswith(("cat7", "hubhub")):
        assert rev.size >= 2 and (rev >= 3).all(), rev  # reversed edges, all at junctions
        inward = np.setdiff1d(P.base.root_out, [0])  # boundary nodes on the "in" side
        assert inward.size == rev.size, (inward, rev)
        assert np.isin(inward, src).all() and not np.isin(inward, dst).any()
    if name.startswith("hubhub"):
        assert R.max() / R.min() > 10.0  # the seeded two-decade R
    return P, R, f, pb


@pytest.mark.parametrize("case", ["Y_N4", "edge_info_N10"])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("kind", ["linear", "lsq"])
def test_adjoint_matches_finite_differences(case, k, kind):
    P, R, f, pb = _setup(case, k)
    fd_check(P, R, f, pb, kind, f"{case} k={k}")


@pytest.mark.parametrize("name", list(FD_SHAPES))
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("kind", ["linear", "lsq"])
def test_adjoint_matches_finite_differences_on_shapes(name, k, kind):
    """Forests that are not binary (``tree_shapes.FD_SHAPES``), before the adjoint is the
    yardstick of tests/test_gpu_fe_shapes.py on them: a hub and a broom past the record caps,
    side edges pointing into a spine, a hub of hubs with the seeded two-decade R."""
    P, R, f, pb = shape_setup(name, k, 0)
    g, fd_p, _ = fd_check(P, R, f, pb, kind, f"{name} k={k}")
    inward = np.setdiff1d(P.base.root_out, [0])
    if inward.size:  # the derivative at the "in" side of a reversed edge is not trivially 0
        assert np.abs(fd_p[inward]).min() > 0 and np.abs(g["dp_bc"][inward]).min() > 0
