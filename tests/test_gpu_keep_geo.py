"""The chains' R-only factors kept across values-free steps.

Every cell's length h and mass R h / 6 and every chain's T, 1 / T, mo and 1 / mo depend on the
geometry, N, the decomposition and R alone. The values-free dense step reads them from a
per-handle table (``k_dir_step_kg<8, 2>``) that ``k_chain_geo`` fills with the step's own
device functions; ``NXHIP_KEEP_GEO=0`` (read per solve) keeps the recomputing step
``k_dir_step_kv<8, 2>``. ``handle.geo_kept()`` reports ``ran`` (the last step read the table) and
``builds`` (how many times the handle built it).

Shapes (the smallest at which the lane layout can go wrong; <8, 2>: 8 lanes of 2 cells):
``tree5_N16`` j8 (every slot valid), ``tree5_N15`` j8 (the last lane holds one cell plus q_N),
``tree8_N4`` j128 (lanes 2-7 empty), ``arterial5_N16`` j16 (per-edge R = 1 / radius**4, uneven
lengths) and ``swapped5_N15`` j8 (the depth-5 tree with every other edge's end points swapped:
flipped chains, asserted from the decomposition's host arrays). Every shape has jobs with fewer
chains than the 128 lane groups, so inactive groups are covered too (asserted likewise).

Bars: a step on the table and the recomputing step on the same handle give x, rhs and the
reported residual equal as bytes; CSR values and rhs bit-equal to the oracle; x within 1e-10
of the oracle's direct solve (``test_gpu_dstep_dense.py``'s bar)."""

from __future__ import annotations

import functools

import networkx as nx
import numpy as np
import pytest

from cases import CASES
from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh
from networks_fenicsx_amd import network_generation as ng
from networks_fenicsx_amd.precond import build_tree_preconditioner
from oracle import nx_oracle as O
from test_gpu_dstep_dense import SHAPES as _DENSE_SHAPES

pytestmark = pytest.mark.gpu

SOL_TOL = 1e-10
LANE_GROUPS = 128  # 1024 threads / W = 8


def _swapped_tree():
    """``make_tree(5, 5, 5)`` with every other edge's end points swapped."""
    G = ng.make_tree(5, 5, 5)
    H = nx.DiGraph()
    H.add_nodes_from(G.nodes(data=True))
    for i, (u, v) in enumerate(G.edges()):
        H.add_edge(*((v, u) if i % 2 else (u, v)))
    return H


# name -> (graph factory, N, colour strategy, p_bc, per-edge R from the radius)
SHAPES = dict(_DENSE_SHAPES)
SHAPES["tree5_N15"] = CASES["tree5_N15"] + (False,)
SHAPES["swapped5_N15"] = (_swapped_tree, 15, "smallest_last", CASES["tree5_N15"][3], False)
# (shape, target_jobs, another target_jobs whose decomposition also runs the dense step)
CONFIGS = [("tree5_N16", 8, 16), ("tree5_N15", 8, 16), ("tree8_N4", 128, 16),
           ("arterial5_N16", 16, 8), ("swapped5_N15", 8, 16)]
_IDS = [f"{s}-j{j}" for s, j, _ in CONFIGS]
_SJ = [(s, j) for s, j, _ in CONFIGS]


def _pbc2(x):
    return 2.0 * x[1] - 0.5 * x[0] + 1.0


def _mesh(shape):
    make, N, strategy, _, _ = SHAPES[shape]
    return NetworkMesh(make(), N=N, color_strategy=strategy)


def _R(mesh, shape, r_key):
    if r_key == "new":
        return 0.5 + 0.25 * (np.arange(mesh.num_edges) % 7) ** 2
    if r_key == "new2":
        return 1.5 + 0.125 * (np.arange(mesh.num_edges) % 5)
    if SHAPES[shape][4]:
        return 1.0 / mesh.edge_radius ** 4
    return np.ones(mesh.num_edges)


def _f(mesh, f_key):
    """The source: none, a nonzero constant, or one value per graph edge."""
    if f_key == "const":
        return 0.75
    if f_key == "edge":
        return 0.25 + 0.5 * (np.arange(mesh.num_edges) % 3) - 0.125 * (np.arange(mesh.num_edges) % 5)
    return None


def _pbc(shape, pbc_key):
    return _pbc2 if pbc_key == "2" else SHAPES[shape][3]


@functools.lru_cache(maxsize=None)
def _oracle(shape, pbc_key="0", r_key="base", f_key="0"):
    """The oracle's system in the build layout and its direct solve: computed once per (shape,
    boundary data, R, source), shared by the tests and read-only."""
    mesh = _mesh(shape)
    src, dst = mesh.edges
    P = O.build_problem(mesh.node_coordinates, src, dst, mesh.N, mesh.edge_colors)
    f = _f(mesh, f_key)
    A, b = O.assemble_reference(P, _pbc(shape, pbc_key), f=0.0 if f is None else f,
                                R=_R(mesh, shape, r_key))
    Ab, bb, perm, _ = O.to_build_layout(P, A, b)
    out = {"rp": np.asarray(Ab.indptr), "val": np.asarray(Ab.data), "rhs": np.asarray(bb),
           "x": O.solve_reference(A, b)[perm]}
    for v in out.values():
        v.setflags(write=False)
    return out


def _decompose(asm, mesh, jobs):
    src, dst = mesh.edges
    asm._pc = build_tree_preconditioner(asm._local, src, dst, mesh.degrees, target_jobs=jobs)
    asm.set_preconditioner(True)


def _handle(shape, jobs, pbc_key="0", r_key="base", f_key="0"):
    """A handle with the forced decomposition, R as an array, the direct solve asked for."""
    mesh = _mesh(shape)
    asm = HydraulicNetworkAssembler(mesh)
    _decompose(asm, mesh, jobs)
    asm.compute_forms(p_bc_ex=_pbc(shape, pbc_key), f=_f(mesh, f_key), R=_R(mesh, shape, r_key))
    asm.set_direct(True)
    return mesh, asm


def _step(asm, path="fused"):
    asm.assemble()
    h = asm.handle
    it, rr, conv = h.solve(1e-12, 100, 4)
    assert h.direct_path() == path and conv and it == 1, (h.direct_path(), it, rr)
    return rr, h.solution(), h.rhs()


def _same(a, b):
    """(rr, x, rhs) equal as bytes."""
    assert np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes(), (a[0], b[0])
    assert a[1].tobytes() == b[1].tobytes()
    assert a[2].tobytes() == b[2].tobytes()


def _bars(h, ora, res, what=""):
    rr, x, rhs = res
    rp, col, val = h.csr()
    np.testing.assert_array_equal(rp, ora["rp"])
    np.testing.assert_array_equal(val, ora["val"])
    np.testing.assert_array_equal(rhs, ora["rhs"])
    err = np.linalg.norm(x - ora["x"]) / np.linalg.norm(ora["x"])
    print(f"{what}: |x-x_ref|/|x_ref|={err:.3e} rr={rr:.3e} {h.geo_kept()} {h.values_kept()}")
    assert err <= SOL_TOL


def _kept(h, ran, builds):
    assert h.geo_kept() == {"ran": ran, "builds": builds}, h.geo_kept()
    if ran:
        assert h.values_kept()["kept"] and h.direct_dense()["ran"]


def test_shapes_cover_the_lane_layout():
    """From the decompositions' host arrays: flipped chains where the test says so, jobs with
    fewer chains than lane groups everywhere, one chain pass per job."""
    for shape, jobs, jobs2 in CONFIGS:
        mesh = _mesh(shape)
        asm = HydraulicNetworkAssembler(mesh)
        for j in (jobs, jobs2):
            _decompose(asm, mesh, j)
            pc = asm.tree_preconditioner
            per_job = np.diff(np.asarray(pc.job_chain_off))
            flips = int(np.asarray(pc.chain_flip).sum())
            print(f"{shape} j{j}: {pc.n_jobs} jobs, chains per job {per_job.min()}..{per_job.max()}, "
                  f"{flips} of {len(pc.chain_flip)} chains flipped")
            assert per_job.min() < LANE_GROUPS and per_job.max() <= LANE_GROUPS
            if shape == "swapped5_N15":
                assert 0 < flips < len(pc.chain_flip)
        asm.close()


@pytest.mark.parametrize("shape,jobs", _SJ, ids=_IDS)
def test_kept_against_recomputed(shape, jobs, monkeypatch):
    """Steps on the table, then NXHIP_KEEP_GEO=0 on the same handle: the same bytes."""
    mesh, asm = _handle(shape, jobs)
    h, ora = asm.handle, _oracle(shape)
    _kept(h, False, 0)
    first = _step(asm)  # (stores the values: no values-free step yet, no table)
    _kept(h, False, 0)
    _bars(h, ora, first, f"{shape} step 1")
    on = [_step(asm) for _ in range(3)]
    _kept(h, True, 1)
    for r in on:
        _bars(h, ora, r, f"{shape} kept")
        _same(r, on[0])
    monkeypatch.setenv("NXHIP_KEEP_GEO", "0")
    off = _step(asm)
    _kept(h, False, 1)
    assert h.values_kept()["kept"]  # (k_dir_step_kv)
    _bars(h, ora, off, f"{shape} recomputed")
    _same(off, on[0])
    monkeypatch.delenv("NXHIP_KEEP_GEO")
    again = _step(asm)
    _kept(h, True, 1)
    _same(again, on[0])
    asm.close()


@pytest.mark.parametrize("f_key", ["const", "edge"])
@pytest.mark.parametrize("shape,jobs", _SJ, ids=_IDS)
def test_sources_read_the_kept_lengths(shape, jobs, f_key, monkeypatch):
    """A nonzero constant f, and a per-edge source through nx_set_source: the cell rows of the
    rhs, -(f h), are the only ones that read the kept h -- bit-equal to the oracle's."""
    mesh, asm = _handle(shape, jobs, f_key=f_key)
    h, ora = asm.handle, _oracle(shape, f_key=f_key)
    _step(asm)
    on = _step(asm)
    _kept(h, True, 1)
    _bars(h, ora, on, f"{shape} f={f_key}")
    # the source changed on the kept table (R re-sent with the same contents, then nx_set_source)
    f2 = _f(mesh, "edge" if f_key == "const" else "const")
    asm.compute_forms(p_bc_ex=_pbc(shape, "0"), f=f2, R=_R(mesh, shape, "base"))
    on2 = _step(asm)
    _kept(h, True, 1)
    _bars(h, _oracle(shape, f_key="edge" if f_key == "const" else "const"), on2,
          f"{shape} f swapped")
    monkeypatch.setenv("NXHIP_KEEP_GEO", "0")
    off2 = _step(asm)
    _kept(h, False, 1)
    _same(off2, on2)
    asm.close()


@pytest.mark.parametrize("shape,jobs", _SJ, ids=_IDS)
def test_table_lifetime(shape, jobs):
    """New boundary values leave the table alone; a new R is stored by the next step (no table
    read) and the step after rebuilds it once; R changed on every step never builds."""
    mesh, asm = _handle(shape, jobs)
    h = asm.handle
    bc0 = np.array(asm._coefficients["edge_bc"], copy=True)
    _step(asm)
    _step(asm)
    _kept(h, True, 1)
    asm.compute_forms(p_bc_ex=_pbc2, R=_R(mesh, shape, "base"))  # (R re-sent: same contents)
    r = _step(asm)
    _kept(h, True, 1)
    _bars(h, _oracle(shape, "2"), r, f"{shape} new p_bc, R re-sent")
    h.set_coefficients(None, float("nan"), 0.0, bc0)  # (the resident R stays)
    r = _step(asm)
    _kept(h, True, 1)
    _bars(h, _oracle(shape), r, f"{shape} first p_bc, keep-R form")
    pbc = _pbc(shape, "0")
    asm.compute_forms(p_bc_ex=pbc, R=_R(mesh, shape, "new"))
    ora = _oracle(shape, "0", "new")
    r = _step(asm)
    _kept(h, False, 1)
    assert not h.values_kept()["kept"]
    _bars(h, ora, r, f"{shape} new R, storing")
    kept = _step(asm)
    _kept(h, True, 2)
    _bars(h, ora, kept, f"{shape} new R, kept")
    _same(_step(asm), kept)
    _kept(h, True, 2)
    for k in range(4):  # R changed on every step: no values-free step, no build
        asm.compute_forms(p_bc_ex=pbc, R=_R(mesh, shape, "new2" if k % 2 == 0 else "new"))
        r = _step(asm)
        _kept(h, False, 2)
        _bars(h, _oracle(shape, "0", "new2" if k % 2 == 0 else "new"), r, f"{shape} R every step")
    asm.close()
    _, asm2 = _handle(shape, jobs, r_key="new")
    _step(asm2)
    fresh = _step(asm2)
    _kept(asm2.handle, True, 1)
    _same(fresh, kept)
    asm2.close()


@pytest.mark.parametrize("shape,jobs,jobs2", CONFIGS, ids=_IDS)
def test_interleaving(shape, jobs, jobs2, monkeypatch):
    """A MINRES solve and the separate launches in between leave results and builds alone; a
    new decomposition invalidates the table and the next kept step equals a fresh handle's."""
    mesh, asm = _handle(shape, jobs)
    h, ora = asm.handle, _oracle(shape)
    _step(asm)
    on = _step(asm)
    _kept(h, True, 1)
    asm.set_direct(False)
    asm.assemble()
    it, _, conv = h.solve(1e-12, 100, 4)
    assert conv and it <= 4, it
    _kept(h, False, 1)
    asm.set_direct(True)
    _same(_step(asm), on)
    _kept(h, True, 1)
    monkeypatch.setenv("NXHIP_DIR_FUSED", "0")
    sep = _step(asm, path="launches")
    _kept(h, False, 1)
    _bars(h, ora, sep, f"{shape} launches")
    monkeypatch.delenv("NXHIP_DIR_FUSED")
    _same(_step(asm), on)
    _kept(h, True, 1)
    _decompose(asm, mesh, jobs2)
    asm._direct_state = None
    asm.set_direct(True)
    _step(asm)
    redone = _step(asm)
    _kept(h, True, 2)
    _bars(h, ora, redone, f"{shape} j{jobs2} on the same handle")
    asm.close()
    _, asm2 = _handle(shape, jobs2)
    _step(asm2)
    fresh = _step(asm2)
    _kept(asm2.handle, True, 1)
    _same(fresh, redone)
    asm2.close()


@pytest.mark.parametrize("shape,jobs", _SJ, ids=_IDS)
def test_kept_step_that_gives_up(shape, jobs):
    """A step on the table whose waiting workgroups give up at once (the bounded-poll test
    hook, as test_gpu_keep_values.py): the solve falls back to the separate launches."""
    mesh, asm = _handle(shape, jobs)
    h, ora = asm.handle, _oracle(shape)
    _step(asm)
    _step(asm)
    _kept(h, True, 1)
    h.set_wait_polls(0)
    r = _step(asm, path="launches")
    _kept(h, False, 1)
    _bars(h, ora, r, f"{shape} gave up")
    h.set_wait_polls(1 << 20)
    r = _step(asm, path="launches")  # (the fallback is sticky)
    _kept(h, False, 1)
    _bars(h, ora, r, f"{shape} after the give-up")
    asm.close()
