"""The CSR values kept across steps while R is unchanged.

The values depend on the geometry, N and R alone, so once a launch has written all of them for
the resident R (``val_version == r_version`` in the library), the dense fused step runs its
values-free instantiation ``k_dir_step_kv<8, 2>`` (rhs, x, posts and the published state as
before; no CSR segment, no multiplier-row values) and the separate assembly launch runs with
``lhs = 0``. ``NXHIP_KEEP_VALUES=0`` (read per solve) forces the stores;
``handle.values_kept()`` reports ``kept`` (the last assembly or step left the values alone) and
``writes`` (launches of this handle that wrote them).

Shapes: the forced-top-part decompositions of ``test_gpu_dstep_dense.py`` that run the dense
``<8, 2>`` step (``tree5_N16`` j8, ``tree8_N4`` j128, ``depth6_N16`` j2, ``arterial5_N16`` j16
with per-edge R = 1 / radius**4); ``depth6_N40`` j8 (``<16, 4>``, the top solver), ``tree5_N16``
j8 with the dense top switched off and a default-decomposition one-job tree (``Y_N4``) cover
the instantiations that keep storing.

Bars, as in that file: CSR values and rhs bit-equal to the oracle; x within 1e-10 of the
oracle's direct solve; reported residual within 5 % + 5e-16 of the true one; a values-free
step's x within 1e-14 relative 2-norm of the storing step's on the same handle (the bar
between the project's direct paths; printed: whether it is bit-equal)."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh
from networks_fenicsx_amd._lib import NxError
from networks_fenicsx_amd.precond import build_tree_preconditioner
from oracle import nx_oracle as O
from cases import CASES
from test_gpu_dstep_dense import SHAPES as _DENSE_SHAPES

pytestmark = pytest.mark.gpu

SOL_TOL = 1e-10
# (graph factory, N, colour strategy, p_bc, per-edge R from the radius)
SHAPES = dict(_DENSE_SHAPES, Y_N4=CASES["Y_N4"] + (False,))
DENSE = [("tree5_N16", 8), ("tree8_N4", 128), ("depth6_N16", 2), ("arterial5_N16", 16)]
_IDS = [f"{s}-j{j}" for s, j in DENSE]


def _pbc2(x):
    return 2.0 * x[1] - 0.5 * x[0] + 1.0


def _mesh(shape):
    make, N, strategy, _, _ = SHAPES[shape]
    return NetworkMesh(make(), N=N, color_strategy=strategy)


def _R(mesh, shape, r_key):
    """Per graph edge: ``base`` (1 / radius**4 where the shape has radii, else ones -- the
    default constant's contents, as an array) or ``new``."""
    if r_key == "new":
        return 0.5 + 0.25 * (np.arange(mesh.num_edges) % 7) ** 2
    if SHAPES[shape][4]:
        return 1.0 / mesh.edge_radius ** 4
    return np.ones(mesh.num_edges)


def _pbc(shape, pbc_key):
    return _pbc2 if pbc_key == "2" else SHAPES[shape][3]


@functools.lru_cache(maxsize=None)
def _oracle(shape, pbc_key="0", r_key="base"):
    """The oracle's system in the build layout and its direct solve: computed once per (shape,
    boundary data, R), shared by the tests and read-only."""
    mesh = _mesh(shape)
    src, dst = mesh.edges
    P = O.build_problem(mesh.node_coordinates, src, dst, mesh.N, mesh.edge_colors)
    A, b = O.assemble_reference(P, _pbc(shape, pbc_key), R=_R(mesh, shape, r_key))
    Ab, bb, perm, _ = O.to_build_layout(P, A, b)
    out = {"rp": np.asarray(Ab.indptr), "val": np.asarray(Ab.data), "rhs": np.asarray(bb),
           "x": O.solve_reference(A, b)[perm]}
    for v in out.values():
        v.setflags(write=False)
    return out


def _handle(shape, jobs, pbc_key="0", r_key="base", base_as_array=False):
    """A handle with the forced decomposition (jobs None: the default one), the direct solve
    asked for. The base R goes up as the shape's own form (the default constant, or the radius
    array) unless ``base_as_array``."""
    mesh = _mesh(shape)
    asm = HydraulicNetworkAssembler(mesh)
    if jobs is not None:
        src, dst = mesh.edges
        asm._pc = build_tree_preconditioner(asm._local, src, dst, mesh.degrees, target_jobs=jobs)
        asm.set_preconditioner(True)
    forms = {}
    if r_key == "new" or SHAPES[shape][4] or base_as_array:
        forms["R"] = _R(mesh, shape, r_key)
    asm.compute_forms(p_bc_ex=_pbc(shape, pbc_key), **forms)
    asm.set_direct(True)
    return mesh, asm


def _step(asm, lhs=True, path="fused"):
    asm.assemble(assemble_lhs=lhs)
    h = asm.handle
    it, rr, conv = h.solve(1e-12, 100, 4)
    assert h.direct_path() == path and conv and it == 1, (h.direct_path(), it, rr)
    return rr, h.solution()


def _bars(h, ora, rr, x, what=""):
    rp, col, val = h.csr()
    np.testing.assert_array_equal(rp, ora["rp"])
    np.testing.assert_array_equal(val, ora["val"])
    np.testing.assert_array_equal(h.rhs(), ora["rhs"])
    err = np.linalg.norm(x - ora["x"]) / np.linalg.norm(ora["x"])
    true = h.true_residual()
    print(f"{what}: |x-x_ref|/|x_ref|={err:.3e} rr={rr:.3e} true={true:.3e} {h.values_kept()}")
    assert err <= SOL_TOL
    assert abs(rr - true) <= 0.05 * true + 5e-16, (rr, true)


@pytest.mark.parametrize("shape,jobs", DENSE, ids=_IDS)
def test_keeps_values_after_the_first_step(shape, jobs, monkeypatch):
    """Step 1 writes the values, steps 2-5 keep them (bit-identical x and residual among
    themselves); the storing step on the same handle gives the same x to 1e-14."""
    mesh, asm = _handle(shape, jobs)
    h, ora = asm.handle, _oracle(shape)
    assert h.values_kept() == {"kept": False, "writes": 0}
    rr1, x1 = _step(asm)
    assert h.values_kept() == {"kept": False, "writes": 1} and h.direct_dense()["ran"]
    _bars(h, ora, rr1, x1, f"{shape} step 1")
    kept = []
    for k in range(2, 6):
        rr, x = _step(asm)
        assert h.values_kept() == {"kept": True, "writes": 1}, k
        assert h.direct_dense()["ran"]
        _bars(h, ora, rr, x, f"{shape} step {k}")
        kept.append((rr, x))
    for rr, x in kept[1:]:
        assert rr == kept[0][0]
        np.testing.assert_array_equal(x, kept[0][1])
    monkeypatch.setenv("NXHIP_KEEP_VALUES", "0")
    rr0, x0 = _step(asm)
    assert h.values_kept() == {"kept": False, "writes": 2}
    diff = np.linalg.norm(kept[0][1] - x0) / np.linalg.norm(x0)
    print(f"{shape} j{jobs}: |x_kept-x_storing|/|x|={diff:.3e} "
          f"bit-equal={bool(np.array_equal(kept[0][1], x0))}")
    assert diff <= 1e-14
    _bars(h, ora, rr0, x0, f"{shape} storing")
    asm.close()


@pytest.mark.parametrize("shape,jobs", DENSE, ids=_IDS)
def test_new_rhs_same_R_is_kept(shape, jobs):
    """New boundary values with the same R -- R re-sent as an array, then through the keep-R
    form of nx_set_coefficients -- keep the values: the rhs is the new oracle's bit for bit."""
    mesh, asm = _handle(shape, jobs)
    h = asm.handle
    bc0 = np.array(asm._coefficients["edge_bc"], copy=True)
    _step(asm)
    _step(asm)
    builds = h.direct_dense()["builds"]
    assert h.values_kept() == {"kept": True, "writes": 1} and builds == 1
    asm.compute_forms(p_bc_ex=_pbc2, R=_R(mesh, shape, "base"))
    rr, x = _step(asm)
    assert h.values_kept() == {"kept": True, "writes": 1}
    _bars(h, _oracle(shape, "2"), rr, x, f"{shape} new p_bc, R re-sent")
    assert h.direct_dense() == {"ran": True, "builds": builds}
    h.set_coefficients(None, float("nan"), 0.0, bc0)  # (the resident R stays)
    rr, x = _step(asm)
    assert h.values_kept() == {"kept": True, "writes": 1}
    _bars(h, _oracle(shape), rr, x, f"{shape} first p_bc, keep-R form")
    assert h.direct_dense() == {"ran": True, "builds": builds}
    asm.close()


@pytest.mark.parametrize("shape,jobs", DENSE, ids=_IDS)
def test_new_R_is_written_once(shape, jobs):
    """A new R is written by the next step and kept by the one after it; R set back to its old
    contents counts as new; the kept step's x is a fresh handle's second step's, bit for bit
    (no stale values)."""
    mesh, asm = _handle(shape, jobs)
    h = asm.handle
    pbc = _pbc(shape, "0")
    _step(asm)
    _step(asm)
    assert h.values_kept() == {"kept": True, "writes": 1}
    asm.compute_forms(p_bc_ex=pbc, R=_R(mesh, shape, "new"))
    ora = _oracle(shape, "0", "new")
    rr, x = _step(asm)
    assert h.values_kept() == {"kept": False, "writes": 2}
    _bars(h, ora, rr, x, f"{shape} new R")
    rr, x_kept = _step(asm)
    assert h.values_kept() == {"kept": True, "writes": 2}
    _bars(h, ora, rr, x_kept, f"{shape} new R, kept")
    asm.compute_forms(p_bc_ex=pbc, R=_R(mesh, shape, "base"))
    rr, x = _step(asm)
    assert h.values_kept() == {"kept": False, "writes": 3}
    _bars(h, _oracle(shape), rr, x, f"{shape} R set back")
    asm.close()
    _, asm2 = _handle(shape, jobs, r_key="new")
    _step(asm2)
    _, x_fresh = _step(asm2)
    assert asm2.handle.values_kept() == {"kept": True, "writes": 1}
    np.testing.assert_array_equal(x_kept, x_fresh)
    asm2.close()


@pytest.mark.parametrize("shape,jobs", DENSE, ids=_IDS)
def test_rhs_only_assembly_runs_the_fused_step(shape, jobs):
    """assemble(lhs=False, rhs=True) after a current matrix: one launch, values kept. On a
    handle that never assembled the matrix the solve refuses, as it always did."""
    mesh, asm = _handle(shape, jobs)
    h = asm.handle
    _step(asm)
    asm.compute_forms(p_bc_ex=_pbc2, R=_R(mesh, shape, "base"))
    rr, x = _step(asm, lhs=False)
    assert h.values_kept() == {"kept": True, "writes": 1} and h.direct_dense()["ran"]
    _bars(h, _oracle(shape, "2"), rr, x, f"{shape} rhs only")
    asm.close()
    _, asm2 = _handle(shape, jobs)
    asm2.assemble(assemble_lhs=False)
    with pytest.raises(NxError, match="assemble lhs and rhs before solve"):
        asm2.handle.solve(1e-12, 100, 4)
    assert asm2.handle.values_kept() == {"kept": False, "writes": 0}
    asm2.close()


@pytest.mark.parametrize("shape,jobs", DENSE, ids=_IDS)
def test_minres_in_between_keeps_the_values(shape, jobs):
    mesh, asm = _handle(shape, jobs)
    h, ora = asm.handle, _oracle(shape)
    _step(asm)
    rr1, x1 = _step(asm)
    assert h.values_kept() == {"kept": True, "writes": 1}
    asm.set_direct(False)
    asm.assemble()
    it, _, conv = h.solve(1e-12, 100, 4)
    assert conv and it <= 4, it
    assert h.values_kept() == {"kept": True, "writes": 1}
    np.testing.assert_array_equal(h.csr()[2], ora["val"])
    np.testing.assert_array_equal(h.rhs(), ora["rhs"])
    asm.set_direct(True)
    rr, x = _step(asm)
    assert h.values_kept() == {"kept": True, "writes": 1}
    assert rr == rr1
    np.testing.assert_array_equal(x, x1)
    _bars(h, ora, rr, x, f"{shape} after MINRES")
    asm.close()


@pytest.mark.parametrize("shape,jobs", DENSE, ids=_IDS)
def test_storing_step_that_gives_up(shape, jobs):
    """A storing step (new R) whose waiting workgroups give up at once (the bounded-poll test
    hook, as test_dstep_give_up_falls_back_to_launches): the solve falls back to the separate
    launches, whose assembly writes every value; no kept step is claimed."""
    mesh, asm = _handle(shape, jobs)
    h = asm.handle
    _step(asm)
    asm.compute_forms(p_bc_ex=_pbc(shape, "0"), R=_R(mesh, shape, "new"))
    ora = _oracle(shape, "0", "new")
    h.set_wait_polls(0)
    rr, x = _step(asm, path="launches")
    assert h.values_kept() == {"kept": False, "writes": 2}
    _bars(h, ora, rr, x, f"{shape} gave up")
    h.set_wait_polls(1 << 20)
    for k in range(3):  # (the fallback is sticky: the separate launches from now on)
        rr, x = _step(asm, path="launches")
        _bars(h, ora, rr, x, f"{shape} after the give-up {k}")
    assert h.values_kept()["writes"] == 2
    asm.close()


@pytest.mark.parametrize("shape,jobs,dense_env",
                         [("depth6_N40", 8, None), ("tree5_N16", 8, "0"), ("Y_N4", None, None)],
                         ids=["depth6_N40-j8-top-solver", "tree5_N16-j8-dense-off", "Y_N4-one-job"])
def test_other_instantiations_keep_storing(shape, jobs, dense_env, monkeypatch):
    """Only the dense <8, 2> step has a values-free instantiation. The <16, 4> step on the top
    solver, the <8, 2> step with the dense top switched off (k_dir_step_ts) and a
    default-decomposition one-job tree are fused and meet every bar; a step that does not run
    the dense top stores the values every time (kept False, writes + 1), one that does keeps
    them from its second step on."""
    if dense_env is not None:
        monkeypatch.setenv("NXHIP_DIR_DENSE", dense_env)
    mesh, asm = _handle(shape, jobs)
    h, ora = asm.handle, _oracle(shape)
    if jobs is None:
        assert asm.tree_preconditioner.n_jobs == 1
    writes = 0
    for k in range(1, 4):
        rr, x = _step(asm)
        dense = h.direct_dense()["ran"]
        assert jobs is None or not dense  # (the forced decompositions: never the dense top)
        kept = dense and k > 1
        writes += 0 if kept else 1
        assert h.values_kept() == {"kept": kept, "writes": writes}, (k, dense)
        _bars(h, ora, rr, x, f"{shape} step {k} dense={dense}")
    asm.close()


@pytest.mark.parametrize("shape,jobs", DENSE, ids=_IDS)
def test_separate_launches_keep_the_values(shape, jobs, monkeypatch):
    """NXHIP_DIR_FUSED=0: the second step's assembly launch leaves the values alone; one
    assembly launch per step, as before."""
    monkeypatch.setenv("NXHIP_DIR_FUSED", "0")
    mesh, asm = _handle(shape, jobs)
    h, ora = asm.handle, _oracle(shape)
    h.set_profiling(True)
    h.reset_profile()
    for k in range(1, 4):
        rr, x = _step(asm, path="launches")
        assert h.values_kept() == {"kept": k > 1, "writes": 1}
        assert h.profile()["asm_count"] == k
        _bars(h, ora, rr, x, f"{shape} launches {k}")
    h.set_profiling(False)
    rr, x = _step(asm, path="launches")  # (and without the profiling path's own flush)
    assert h.values_kept() == {"kept": True, "writes": 1}
    _bars(h, ora, rr, x, f"{shape} launches, no profiling")
    asm.close()


@pytest.mark.parametrize("shape,jobs", DENSE, ids=_IDS)
def test_keep_values_switched_off(shape, jobs, monkeypatch):
    """NXHIP_KEEP_VALUES=0: every step writes the values (INTEGRATION.md's switch table)."""
    monkeypatch.setenv("NXHIP_KEEP_VALUES", "0")
    mesh, asm = _handle(shape, jobs)
    h, ora = asm.handle, _oracle(shape)
    for k in range(1, 4):
        rr, x = _step(asm)
        assert h.values_kept() == {"kept": False, "writes": k} and h.direct_dense()["ran"]
        _bars(h, ora, rr, x, f"{shape} step {k}")
    monkeypatch.setenv("NXHIP_DIR_FUSED", "0")
    rr, x = _step(asm, path="launches")
    assert h.values_kept() == {"kept": False, "writes": 4}
    _bars(h, ora, rr, x, f"{shape} launches")
    asm.close()
