"""The exchange step on ranks that do not look alike (tests/unlike_ranks.py; the host side:
tests/test_unlike_ranks.py, which asserts every configuration's facts and runs the numpy model
on the mixed decompositions).

Every other multi-rank test runs ranks of the default decomposition on balanced trees cut into
equal chunks, nearly all with R = 1, f = 0. Here every rank of a ``RankGroup`` gets its own
``target_jobs``, with a seeded per-edge R, f != 0 and p_bc = x[1] + 0.3 x[0], so that these
cases of the one-launch step run beside each other: a rank whose job needs several chain passes
next to one whose jobs fit one pass (U1, U2, U6), a rank of one job and no job slots between
ranks of 42 and 43 jobs (U3), exactly one pass next to one chain under it (U4), several passes
everywhere (U5).

What the group's one launch (``k_dir_xg``) must take: the superposition instantiation only if
EVERY rank asks for it (``launch_xr_wc``). ``dir_step_body<.., SUP = true>`` ignores
``DirStep::sup`` (``keep = SUP || ..``, ``sup = SUP``) and carries no several-pass code, while
``dir_args`` clears ``sup`` per rank (a job of more than kPcThreads / W = 128 chains, or no room
for the park). Chosen from rank 0 alone, as it was, U1 would run the one-pass kernel on rank 1's
255-chain job: chains 128.. never swept, their x and posts not written, the fused residual formed
from stale posts. That is read from the code; it was not run.

Every solution is judged per block (``tree_shapes.block_errors``) at the project's 1e-10
against the oracle's sparse LU."""

from __future__ import annotations

import contextlib
import functools

import numpy as np
import pytest

import distributed_model as DM
from networks_fenicsx_amd import HydraulicNetworkAssembler
from networks_fenicsx_amd.group import RankGroup
from tree_shapes import block_errors, decomposition_facts, p_xy
from unlike_ranks import (CONFIGS, GROUP_SUP, RANK_SUP, STRATEGY, coefficients, mesh_of, oracle,
                          set_decompositions)

pytestmark = pytest.mark.gpu

SOL_TOL = 1e-10  # per block
ONE_RANK_TOL = 1e-12  # tests/test_gpu_tree_shapes.py::test_group_direct_on_hubs
PATH_TOL = 1e-14  # between two direct paths (tests/test_gpu_group.py, tests/test_gpu_dstep.py)

# |x_path - x_group| / |x_group| where a configuration misses 1e-14, measured on an MI355X;
# key: (configuration, path) with path "separate" (every rank's own launch, instantiations
# mixed), "graph" (NXHIP_DIR_XR=0) or "sup0" (NXHIP_DIR_SUP=0). Each path meets the oracle per
# block wherever it is listed here (asserted in the same test), so neither is wrong; the 1e-14
# was argued for R = 1 on binary trees. Bar: 10 x measured, at most 1e-12.
# U6 (N = 19, <8, 3>: three cells per lane), graph path against the group's launch: 3.78e-14,
# fluxes against the oracle 4.06e-12 / 3.89e-12 -- the lane shape of C4, whose rehearsal has
# its own bar against the graph path for the same reason (tests/test_gpu_c4.py: 5e-14 with
# R = 1, measured 1.9e-14). Every other configuration and path: <= 5.1e-16.
PATH_MEASURED: dict[tuple[str, str], float] = {("U6", "graph"): 3.78e-14}
PATH_BAR = {k: 10 * v for k, v in PATH_MEASURED.items()}
assert all(v <= 1e-12 for v in PATH_BAR.values())


@functools.lru_cache(maxsize=None)
def _one_rank(graph: str, N: int) -> np.ndarray:
    """The one-rank direct solve of (graph, N) with the same coefficients, once."""
    _, mesh = mesh_of(graph, N)
    asm = HydraulicNetworkAssembler(mesh)
    try:
        asm.compute_forms(p_bc_ex=p_xy, **coefficients(graph))
        asm.set_direct(True)
        asm.assemble()
        it, rr, conv = asm.handle.solve(1e-12, 100, 4)
        assert conv and asm.handle.solver() == (1, 1), (it, rr)
        x = asm.handle.solution().copy()
    finally:
        asm.close()
    x.setflags(write=False)
    return x


@contextlib.contextmanager
def _group(cid):
    graph, N, jobs, chains = CONFIGS[cid]
    G, mesh = mesh_of(graph, N)
    grp = RankGroup(G, N, len(jobs), color_strategy=STRATEGY)
    try:
        set_decompositions(grp, jobs)
        got = tuple(decomposition_facts(a.tree_preconditioner)["chains"] for a in grp.assemblers)
        assert got == chains, got
        grp.compute_forms(p_bc_ex=p_xy, **coefficients(graph))
        grp.set_direct(True)
        yield grp, mesh
    finally:
        grp.close()


def _gathered(grp, mesh, n):
    x = np.zeros(n)
    for a, xl in zip(grp.assemblers, grp.solutions()):
        x[DM.global_rows(a.local_problem, mesh.num_edges, mesh.bifurcation_index)] = xl
    return x


def _paths(grp):
    return [a.handle.direct_path() for a in grp.assemblers]


def _sups(grp):
    return [a.handle.direct_sup() for a in grp.assemblers]


def _step(grp, separate=False):
    """One step: the group's solve (``(passes, rr, converged)``), or every rank's own launch
    (``xr_separate``: it fails unless every rank published the same residual bits -- xr_conclude
    -- and falls back to the graph path, seen in ``direct_path()``, unless that converged)."""
    grp.assemble()
    if separate:
        return 1, grp._group.xr_separate(1e-12), True
    return grp.solve(1e-12, 50000, 4)


def _check(tag, grp, mesh, ref, want, separate=False, x_ref=None, residual=True):
    """One step against the bars of part (a): every rank on path ``want``, converged in 1 or 2
    passes with rr <= 1e-12, the reported residual the true one of the gathered x, every block
    within 1e-10 of ``x_ref`` (the oracle's LU). Returns (x, rr)."""
    it, rr, conv = _step(grp, separate)
    paths, sups = _paths(grp), _sups(grp)
    x = _gathered(grp, mesh, ref["Ab"].shape[0])
    err = block_errors(x, ref["x"] if x_ref is None else x_ref, ref["E"], ref["N"])
    true = np.linalg.norm(ref["bb"] - ref["Ab"] @ x) / np.linalg.norm(ref["bb"])
    print(f"{tag}: paths {paths} sup {sups} passes {it} rr {rr:.2e}"
          + (f" true {true:.2e}" if residual else "")
          + " blocks q/p/lm " + " ".join(f"{e:.2e}" for e in err))
    assert paths == [want] * grp.nranks, paths
    assert conv and grp.solver_used == "direct" and it in (1, 2) and rr <= 1e-12, (it, rr, conv)
    if residual:
        assert abs(rr - true) <= 0.05 * true + 5e-16, (rr, true)
    assert max(err) <= SOL_TOL, err
    return x, rr


def _path_diff(cid, path, x, x_a):
    d = float(np.linalg.norm(x - x_a) / np.linalg.norm(x_a))
    bar = PATH_BAR.get((cid, path), PATH_TOL)
    print(f"{cid}: |x_{path} - x_group| / |x_group| = {d:.2e} (bar {bar:.1e})")
    return d, bar


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_group_one_launch(cid):
    """(a) The group's one launch (``k_dir_xg``) on every configuration: every rank on the
    exchange path, 1 or 2 passes with rr <= 1e-12, the reported residual within 5 % + 5e-16 of
    the true one of the gathered x, every block within 1e-10 of the oracle's LU, the gathered x
    within 1e-12 of the one-rank solve, five more steps the same bits and the same rr, and
    ``direct_sup()`` the same on every rank: True on U4 (128 and 127 chains: one pass on both
    ranks), False on U1, U2, U3, U5, U6 (a rank with several passes, or <8, 3>). U1 also with
    f = 0 against the analytic resistor network per block.

    Measured on an MI355X (one pass everywhere): rr 2.9e-14 (T9, N = 15), 4.2e-15 (U3),
    3.7e-14 (U4), 2.3e-13 (U6), each equal to the true residual to three digits; worst block
    (the fluxes) against the LU 4.8e-13 (U1, U2, U5), 6.6e-14 (U3), 4.4e-13 (U4), 3.9e-12 (U6),
    pressures and multipliers <= 6.2e-14; U1 with f = 0 against the analytic answer 1.9e-12;
    against the one-rank solve <= 7.4e-16.

    U1 before the fix (the instantiation chosen from rank 0 alone) would have run the one-pass
    superposition kernel on rank 1's two-pass job; see the module's docstring. Not run."""
    graph, N, jobs, _ = CONFIGS[cid]
    ref = oracle(graph, N)
    x_one = _one_rank(graph, N)
    with _group(cid) as (grp, mesh):
        x, rr = _check(f"{cid} group", grp, mesh, ref, "exchange")
        assert _sups(grp) == [GROUP_SUP[cid]] * grp.nranks, _sups(grp)
        d1 = np.linalg.norm(x - x_one) / np.linalg.norm(x_one)
        print(f"{cid}: vs one rank {d1:.2e}")
        assert d1 <= ONE_RANK_TOL, d1
        for _ in range(5):
            it2, rr2, _ = _step(grp)
            assert rr2 == rr and _paths(grp) == ["exchange"] * grp.nranks
            np.testing.assert_array_equal(_gathered(grp, mesh, x.size), x)
        if cid == "U1":
            coef = ref["coef"]
            grp.compute_forms(p_bc_ex=p_xy, R=coef["R"], f=0.0)
            _check(f"{cid} group f=0", grp, mesh, ref, "exchange", x_ref=ref["xa"],
                   residual=False)
            assert _sups(grp) == [False, False]


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_per_rank_launches(cid):
    """(b) Every rank's ``k_dir_xr`` as its own launch on its own stream
    (``Group.xr_separate``, the shape of the multi-GPU path): each rank chooses its
    instantiation from its own ``DirStep`` -- on U1 ``direct_sup()`` is [True, False], on U2
    [False, True], on U3 [True, False, True]: a superposition kernel and a plain kernel exchange
    (``xr_coarse`` and ``dir_publish_xr`` do not depend on SUP). The same published residual on
    every rank (``xr_conclude`` fails otherwise), the oracle per block at 1e-10, the same bits
    over five steps. Where the instantiations are those of the group's launch (U4: superposition
    in both; U5, U6: plain in both) x and rr are bit-equal to (a) -- the claim of
    tests/test_gpu_group.py::test_separate_launches_exchange; where they differ (U1, U2, U3) the
    two agree to the path bar. The group's launch after them gives (a)'s bits again.

    Measured on an MI355X: mixed instantiations against the group's plain launch 1.9e-16 (U1),
    2.0e-16 (U2), 2.2e-16 (U3); block errors those of (a) (U3's fluxes 6.7e-14)."""
    graph, N, jobs, _ = CONFIGS[cid]
    ref = oracle(graph, N)
    with _group(cid) as (grp, mesh):
        x_a, rr_a = _check(f"{cid} group", grp, mesh, ref, "exchange")
        x_b, rr_b = _check(f"{cid} separate", grp, mesh, ref, "exchange", separate=True)
        assert _sups(grp) == list(RANK_SUP[cid]), _sups(grp)
        for _ in range(4):
            _, rr2, _ = _step(grp, separate=True)
            assert rr2 == rr_b and _paths(grp) == ["exchange"] * grp.nranks
            assert _sups(grp) == list(RANK_SUP[cid])
            np.testing.assert_array_equal(_gathered(grp, mesh, x_b.size), x_b)
        if all(s == GROUP_SUP[cid] for s in RANK_SUP[cid]):
            np.testing.assert_array_equal(x_b, x_a)
            assert rr_b == rr_a, (rr_b, rr_a)
        else:
            d, bar = _path_diff(cid, "separate", x_b, x_a)
            assert d <= bar, d
        _, rr3, _ = _step(grp)
        assert rr3 == rr_a and _sups(grp) == [GROUP_SUP[cid]] * grp.nranks
        np.testing.assert_array_equal(_gathered(grp, mesh, x_a.size), x_a)


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_graph_path_and_plain_phase2(cid, monkeypatch):
    """(c) The graph path (``NXHIP_DIR_XR=0``: separate launches with the all-reduces, path
    ``"launches"``) on the same mixed decompositions, and on U4 the exchange step with
    ``NXHIP_DIR_SUP=0`` (the plain phase 2 on jobs of exactly one pass): each meets the oracle
    per block and agrees with (a) to the path bar.

    Measured on an MI355X: the graph path against (a) 0 (U1, U3: the same bits), 1.6e-17 (U2,
    U5), 5.0e-16 (U4, whose (a) is superposition), 3.78e-14 (U6: PATH_MEASURED, both paths'
    fluxes 4e-12 from the oracle); U4 with ``NXHIP_DIR_SUP=0`` 5.0e-16."""
    graph, N, jobs, _ = CONFIGS[cid]
    ref = oracle(graph, N)
    with _group(cid) as (grp, mesh):
        x_a, rr_a = _check(f"{cid} group", grp, mesh, ref, "exchange")
        diffs = []
        if cid == "U4":
            monkeypatch.setenv("NXHIP_DIR_SUP", "0")
            x_s, _ = _check(f"{cid} sup0", grp, mesh, ref, "exchange")
            assert _sups(grp) == [False] * grp.nranks
            monkeypatch.delenv("NXHIP_DIR_SUP")
            diffs.append(_path_diff(cid, "sup0", x_s, x_a))
        monkeypatch.setenv("NXHIP_DIR_XR", "0")
        x_g, rr_g = _check(f"{cid} graph", grp, mesh, ref, "launches")
        diffs.append(_path_diff(cid, "graph", x_g, x_a))
        for d, bar in diffs:
            assert d <= bar, (d, bar)
