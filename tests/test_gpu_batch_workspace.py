"""The batched workspace growing across call kinds on one handle.

One ``Solver`` takes, in sequence, ``solve_many``, ``gradient`` (least squares),
``hessian_vector``, ``solve_ensemble``, ``gradient(R=...)``, ``solve_many`` again and
``solve_many`` with one scenario: the handle's workspace gains the gradient's, the
Hessian-vector product's and the ensemble's parts one after the other (and on a graph with
cycles the per-scenario cycle correction's, which widens it to 64 columns), and what the earlier
calls use must keep its place. Every result is compared, bit for bit -- arrays, iteration counts
and converged flags -- with the same call on a freshly built ``Solver`` of a fresh assembler,
whose workspace is allocated for that call alone. Between the calls the handle's own last
``solve()`` stands: ``solution_vector()`` and ``true_residual()`` do not change.

Set-up: test_gpu_hvp.py's (B = 3 scenarios with the per-edge source, 12 observed rows, fixed-seed
directions) on ``Y_N4`` (a forest) and ``edge_info_N10`` (cycles, ``ensemble_cycles=True``); the
ensemble's R rows are the resident R and two rows ``10 ** uniform(-1, 1)`` (fixed seed). Once
with the default chunk and once with ``NXHIP_BATCH_CHUNK=2`` (chunks 2 + 1: a partial last chunk).
A ``(2, 0)`` handle with ``batch_degrees=True`` on ``Y_N4`` takes ``solve_many`` with B = 3, 1, 3
(test_gpu_fe_batch.py's scenarios)."""

from __future__ import annotations

import numpy as np
import pytest

import test_gpu_fe_batch as fe
from networks_fenicsx_amd import Solver
from test_gpu_ensemble import env
from test_gpu_hvp import HvpSetup

pytestmark = pytest.mark.gpu

FIELDS = ("x", "value", "dR", "df", "dp_bc", "HdR", "Hdf", "Hdp_bc", "iterations",
          "residual_norms", "converged")


def assert_same_result(a, b, what):
    assert type(a) is type(b), what
    seen = 0
    for name in FIELDS:
        if not hasattr(a, name):
            continue
        x, y = getattr(a, name), getattr(b, name)
        assert x is not None and y is not None, (what, name)
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {name}")
        seen += 1
    assert seen >= 4, what
    assert getattr(a, "path", "batched") == getattr(b, "path", "batched") == "batched", what
    assert a.info["fallback"] == b.info["fallback"] == 0, what
    assert a.info["chunk"] == b.info["chunk"], what
    assert a.converged.all(), what


def ensemble_R(s):
    E = s.mesh.num_edges
    rng = np.random.default_rng(31)
    return np.stack([s.R, 10.0 ** rng.uniform(-1.0, 1.0, E), 10.0 ** rng.uniform(-1.0, 1.0, E)])


def calls(s):
    """(label, call on a solver) in the order of the sequence."""
    R = ensemble_R(s)
    return [
        ("solve_many", lambda sv: sv.solve_many(s.items, s.f)),
        ("gradient", lambda sv: sv.gradient(s.items, s.f, data=s.data, **s.kw)),
        ("hessian_vector",
         lambda sv: sv.hessian_vector(s.items, s.f, data=s.data, **s.kw, **s.dirs[0])),
        ("solve_ensemble", lambda sv: sv.solve_ensemble(R, s.items, s.f)),
        ("gradient(R)", lambda sv: sv.gradient(s.items, s.f, data=s.data, R=R, **s.kw)),
        ("solve_many again", lambda sv: sv.solve_many(s.items, s.f)),
        ("solve_many B = 1", lambda sv: sv.solve_many(s.items[:1], s.f[:1])),
    ]


def started(s, **solver_kw):
    """A solver whose handle has assembled and solved its own system."""
    solver = Solver(s.asm, **solver_kw)
    solver.assemble()
    solver.solve()
    return solver


@pytest.mark.parametrize("chunk", [None, 2])
@pytest.mark.parametrize("name, cycles", [("Y_N4", False), ("edge_info_N10", True)])
def test_results_do_not_depend_on_the_calls_before(name, cycles, chunk):
    kw = {"ensemble_cycles": True} if cycles else {}
    with env(**({} if chunk is None else {"NXHIP_BATCH_CHUNK": chunk})):
        s = HvpSetup(name)
        try:
            solver = started(s, **kw)
            x0, r0 = solver.solution_vector(), solver.true_residual()
            got = []
            for label, call in calls(s):
                got.append(call(solver))
                np.testing.assert_array_equal(solver.solution_vector(), x0, err_msg=label)
                assert solver.true_residual() == r0, label
            for res in got[:6]:
                assert res.info["chunk"] == (3 if chunk is None else 2)
            assert got[6].info["chunk"] == 1
        finally:
            s.close()
        for (label, call), res in zip(calls(s), got):
            t = HvpSetup(name)
            try:
                assert_same_result(res, call(started(t, **kw)), f"{name}, {label}")
            finally:
                t.close()


def test_fe_batch_workspace_shrinks_and_grows():
    """(2, 0) on Y_N4: B = 3, then 1, then 3 on one solver, each against a fresh one."""
    s = fe.Setup("Y_N4", 2)
    try:
        solver = started(s, batch_degrees=True)
        x0, r0 = solver.solution_vector(), solver.true_residual()
        got = []
        for B in (3, 1, 3):
            got.append(solver.solve_many(s.items[:B], s.f[:B]))
            np.testing.assert_array_equal(solver.solution_vector(), x0)
            assert solver.true_residual() == r0
            assert got[-1].info["chunk"] == B
    finally:
        s.close()
    for B, res in zip((3, 1, 3), got):
        t = fe.Setup("Y_N4", 2)
        try:
            fresh = started(t, batch_degrees=True).solve_many(t.items[:B], t.f[:B])
            assert_same_result(res, fresh, f"(2, 0) Y_N4, B = {B}")
        finally:
            t.close()
