"""The general-degree CPU adjoint (tests/gradient_ref_fe.py) at continuous pressure (m >= 1)
against central finite differences of the oracle's own forward solve, before it is trusted as
the yardstick of tests/test_cp_gradient_host.py and tests/test_gpu_cp_gradient.py.

The recipe and the bar are tests/test_gradient_ref_fe.py's: differences in every ``R_e`` (step
``1e-5 R_e``), every boundary node's ``p_bc`` and every ``f_e`` (step ``1e-3``: x is linear in
both, so J is at most quadratic and the central difference has no truncation error); 1e-7 of
``max |g|`` per gradient (observed over these eight cases: <= 1.2e-9 for dR, <= 1e-11 for df
and dp_bc)."""

import numpy as np
import pytest

from cases import CASES
from gradient_ref_fe import AdjointRefFe, forward_fe, objective
from networks_fenicsx_amd import NetworkMesh
from oracle import nx_oracle_fe as OF

BAR = 1e-7


def _setup(case, k, m):
    make, N, strategy, pbc = CASES[case]
    mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
    src, dst = mesh.edges
    P = OF.build_problem_fe(mesh.node_coordinates, src, dst, N, k, m, mesh.edge_colors)
    E = mesh.num_edges
    R = 0.5 + (np.arange(E) % 3) / 2.0
    f = 0.1 + 0.02 * (np.arange(E) % 5)
    pb = np.asarray(pbc(P.base.pos3.T.copy()), dtype=np.float64)
    return P, R, f, pb


@pytest.mark.parametrize("case,k,m", [("Y_N4", 2, 1), ("Y_N4", 3, 2), ("Y_N4", 4, 3),
                                      ("double_Y_N5", 3, 1)])
@pytest.mark.parametrize("kind", ["linear", "lsq"])
def test_adjoint_matches_finite_differences(case, k, m, kind):
    P, R, f, pb = _setup(case, k, m)
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
    for name, fd in (("dR", fd_R), ("df", fd_f), ("dp_bc", fd_p)):
        assert np.abs(fd).max() > 0, name
        err = np.abs(g[name] - fd).max() / np.abs(fd).max()
        print(f"{case} ({k},{m}) {kind} {name}: {err:.2e} of max|g|")
        assert err <= BAR, (name, err)
