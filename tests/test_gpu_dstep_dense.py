"""The dense top of the fused direct step (``k_dir_step<W, 2, true>``; DESIGN.md section 3c,
round 7): no workgroup solves the top part. Every workgroup posts its top inputs pre-weighted,
waits for the arrival counter, and forms the top values it needs as rows of ``G`` (the inverse
of the top part's Schur matrix, built once per decomposition and per R) times the summed
inputs. ``NXHIP_DIR_DENSE=0`` keeps the top solver (``k_dir_step_ts``).

Small trees with a FORCED top part: with the default 256 jobs these graphs are one job and
have no top part. The decompositions are built here with small ``target_jobs`` (8 and 16 as a
rule; 2 for the one-slot top part; 128 where no cut reaches that many jobs, so the whole tree
is the top part over chain-only jobs and a job reads more top values than it has waves).

The dense step is the ``<8, 2>`` instantiation's (N <= 16; the 16- and 64-lane and the 3- and
4-cell variants keep the top solver). ``depth6_N40`` and
``arterial5_N40`` run at their own N = 40 on ``<16, 4>`` -- there the bar is that the step
stays on the top solver and still meets every other assertion -- and again at N = 16, where
the dense top must run (arterial: with ``R = 1 / radius**4``, conductances over orders of
magnitude).

Bars: CSR values and rhs bit-equal to the oracle; x within 1e-10 of the oracle's direct solve;
reported residual within 5 % + 5e-16 of the true one; dense against the top solver on the
same handle within 1e-14 relative 2-norm (the bar between the project's direct paths: G a
and the elimination are both backward-stable solves of the same well-conditioned top system);
repeats bit for bit."""

from __future__ import annotations

import numpy as np
import pytest

from cases import CASES
from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh
from networks_fenicsx_amd import network_generation as ng
from networks_fenicsx_amd.precond import build_tree_preconditioner
from oracle import nx_oracle as O

pytestmark = pytest.mark.gpu

SOL_TOL = 1e-10


def _p_y(x):
    return x[1]


# name -> (graph factory, N, colour strategy, p_bc, per-edge R from the radius)
def _case(name, N=None, radius_R=False):
    make, n0, strategy, pbc = CASES[name]
    return make, (n0 if N is None else N), strategy, pbc, radius_R


SHAPES = {
    "depth6_N40": _case("depth6_N40"),
    "arterial5_N40": _case("arterial5_N40", radius_R=True),
    "linear_alt_N3": _case("linear_alt_N3"),
    "tree5_N16": _case("tree5_N16"),
    "tree8_N4": (lambda: ng.make_tree(8, 8, 8), 4, "smallest_last", _p_y, False),
    "depth6_N16": _case("depth6_N40", N=16),
    "arterial5_N16": _case("arterial5_N40", N=16, radius_R=True),
}
# (shape, target_jobs)
CONFIGS = [("depth6_N40", 8), ("depth6_N40", 16), ("arterial5_N40", 8), ("arterial5_N40", 16),
           ("linear_alt_N3", 8), ("tree5_N16", 8), ("tree5_N16", 16), ("tree8_N4", 8),
           ("tree8_N4", 16), ("tree8_N4", 128), ("depth6_N16", 2), ("depth6_N16", 8),
           ("arterial5_N16", 8), ("arterial5_N16", 16)]
_IDS = [f"{s}-j{j}" for s, j in CONFIGS]


def _setup(shape, jobs, R=None, pbc=None):
    make, N, strategy, pbc0, radius_R = SHAPES[shape]
    pbc = pbc or pbc0
    mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
    asm = HydraulicNetworkAssembler(mesh)
    src, dst = mesh.edges
    asm._pc = build_tree_preconditioner(asm._local, src, dst, mesh.degrees, target_jobs=jobs)
    asm.set_preconditioner(True)
    if R is None and radius_R:
        R = 1.0 / mesh.edge_radius ** 4
    forms = {} if R is None else {"R": R}
    asm.compute_forms(p_bc_ex=pbc, **forms)
    asm.set_direct(True)
    P = O.build_problem(mesh.node_coordinates, src, dst, N, mesh.edge_colors)
    A, b = O.assemble_reference(P, pbc, **forms)
    return mesh, asm, P, A, b


def _top(pc):
    ts0, ts1 = int(pc.top_lvl_off[0]), int(pc.top_lvl_off[-1])
    need = np.diff(pc.job_need_off) if pc.job_need_off.size > 1 else np.zeros(0, int)
    own = np.diff(pc.job_tslot_off) if pc.job_tslot_off.size > 1 else np.zeros(0, int)
    reads_root = [bool((pc.job_need[pc.job_need_off[j]:pc.job_need_off[j + 1]] == ts0).any())
                  for j in range(need.size)]
    return ts1 - ts0, need, own, reads_root


def _step(asm):
    asm.assemble()
    it, rr, conv = asm.handle.solve(1e-12, 100, 4)
    assert asm.handle.direct_path() == "fused" and conv and it == 1, (it, rr)
    return rr, asm.handle.solution()


def test_dense_shapes_cover_the_paths():
    """What the decompositions above cover between them, from their host arrays: a top part on
    every one; a top part of one slot and one that is no multiple of 64; a job that owns no
    top slot; a job whose needs include the top root; a job needing more top values than its
    workgroup has waves (16)."""
    nts, covers = [], {"no_own": False, "root": False, "many": False}
    for shape, jobs in CONFIGS:
        make, N, strategy, _, _ = SHAPES[shape]
        if N > 16:
            continue  # (the top solver's cases)
        mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
        asm = HydraulicNetworkAssembler(mesh)
        src, dst = mesh.edges
        pc = build_tree_preconditioner(asm._local, src, dst, mesh.degrees, target_jobs=jobs)
        asm.close()
        nt, need, own, reads_root = _top(pc)
        assert nt > 0 and need.size == pc.n_jobs, (shape, jobs)
        nts.append(nt)
        covers["no_own"] |= bool((own == 0).any())
        covers["root"] |= any(reads_root)
        covers["many"] |= bool((need > 16).any())
    assert 1 in nts and any(nt % 64 for nt in nts)
    assert all(covers.values()), covers


@pytest.mark.parametrize("shape,jobs", CONFIGS, ids=_IDS)
def test_dense_matches_solver_path_and_oracle(shape, jobs, monkeypatch):
    mesh, asm, P, A, b = _setup(shape, jobs)
    h = asm.handle
    nt = _top(asm._pc)[0]
    assert nt > 0
    want_dense = mesh.N <= 16
    rr, x1 = _step(asm)
    assert h.direct_dense()["ran"] == want_dense
    assert h.direct_dense()["builds"] == (1 if want_dense else 0)
    Ab, bb, perm, _ = O.to_build_layout(P, A, b)
    rp, col, val = h.csr()
    np.testing.assert_array_equal(rp, Ab.indptr)
    np.testing.assert_array_equal(val, Ab.data)
    np.testing.assert_array_equal(h.rhs(), bb)
    x_ref = O.solve_reference(A, b)[perm]
    err = np.linalg.norm(x1 - x_ref) / np.linalg.norm(x_ref)
    true1 = h.true_residual()
    monkeypatch.setenv("NXHIP_DIR_DENSE", "0")
    rr0, x0 = _step(asm)
    assert not h.direct_dense()["ran"]
    diff = np.linalg.norm(x1 - x0) / np.linalg.norm(x0)
    print(f"{shape} jobs={jobs} nt={nt}: |x-x_ref|/|x_ref|={err:.3e} rr={rr:.3e} "
          f"true={true1:.3e} |x_dense-x_solver|/|x|={diff:.3e}")
    assert err <= SOL_TOL
    assert abs(rr - true1) <= 0.05 * true1 + 5e-16, (rr, true1)
    assert diff <= 1e-14
    asm.close()


@pytest.mark.parametrize("shape,jobs", [("tree5_N16", 8), ("tree8_N4", 128), ("depth6_N16", 2)],
                         ids=["tree5_N16-j8", "tree8_N4-j128", "depth6_N16-j2"])
def test_dense_repeats_and_minres_between(shape, jobs):
    """20 steps in a row give bit-identical x from the first one (G is valid before it), and a
    MINRES solve in between -- which rebuilds G in its own start application, from the same
    inputs by the same arithmetic -- leaves the next dense step's x bit-identical too."""
    mesh, asm, P, A, b = _setup(shape, jobs)
    h = asm.handle
    rr, x1 = _step(asm)
    assert h.direct_dense() == {"ran": True, "builds": 1}
    for _ in range(19):
        rr2, x2 = _step(asm)
        assert rr2 == rr
        np.testing.assert_array_equal(x2, x1)
    asm.set_direct(False)
    asm.assemble()
    it, _, conv = h.solve(1e-12, 100, 4)
    assert conv and it <= 4
    asm.set_direct(True)
    rr3, x3 = _step(asm)
    assert h.direct_dense() == {"ran": True, "builds": 1}
    assert rr3 == rr
    np.testing.assert_array_equal(x3, x1)
    asm.close()


@pytest.mark.parametrize("shape,jobs", [("tree5_N16", 8), ("arterial5_N16", 16)],
                         ids=["tree5_N16-j8", "arterial5_N16-j16"])
def test_dense_invalidation(shape, jobs):
    """G follows R's contents, not the other coefficients: new boundary values with the same
    R do not rebuild it; a new per-edge R rebuilds it once, and the step's x is bit-identical
    to a fresh handle's given that R from the start (no stale G)."""
    mesh, asm, P, A, b = _setup(shape, jobs)
    h = asm.handle
    _, _, _, _, radius_R = SHAPES[shape]
    R0 = 1.0 / mesh.edge_radius ** 4 if radius_R else None
    forms0 = {} if R0 is None else {"R": R0}
    _step(asm)
    builds = h.direct_dense()["builds"]
    assert builds == 1

    def pbc2(x):
        return 2.0 * x[1] - 0.5 * x[0] + 1.0

    asm.compute_forms(p_bc_ex=pbc2, **forms0)
    _, x = _step(asm)
    assert h.direct_dense() == {"ran": True, "builds": builds}
    A2, b2 = O.assemble_reference(P, pbc2, **forms0)
    perm = O.to_build_layout(P, A2, b2)[2]
    x_ref = O.solve_reference(A2, b2)[perm]
    assert np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref) <= SOL_TOL

    R = 0.5 + 0.25 * (np.arange(mesh.num_edges) % 7) ** 2
    asm.compute_forms(p_bc_ex=pbc2, R=R)
    _, x = _step(asm)
    assert h.direct_dense() == {"ran": True, "builds": builds + 1}
    A3, b3 = O.assemble_reference(P, pbc2, R=R)
    x_ref = O.solve_reference(A3, b3)[O.to_build_layout(P, A3, b3)[2]]
    assert np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref) <= SOL_TOL
    asm.close()
    _, asm2, _, _, _ = _setup(shape, jobs, R=R, pbc=pbc2)
    _, x_fresh = _step(asm2)
    assert asm2.handle.direct_dense() == {"ran": True, "builds": 1}
    np.testing.assert_array_equal(x, x_fresh)
    asm2.close()
