"""Hubs, brooms and long spines on the host (tests/tree_shapes.py): every shape's decomposition
holds the structure it is in the suite for, and the host side -- the numpy model of the
preconditioner, the CPU port of the direct tree solve, the two references, the continuous-
pressure model -- is right on it, so that tests/test_gpu_tree_shapes.py judges the device alone.

Which branch of csrc/nxhip.hip each shape is there for (the facts asserted below):

* hub4: a slot with exactly ``kWaveKids`` junction children -- all four packed child words of
  ``slot_wave`` / ``top_wave`` are read; hub5: ``kWaveKids + 1`` -- the tables are dropped and
  ``__syncthreads_or(nkids > kWaveKids)`` sends ``pc_up_body`` / ``dir_up_fused`` / ``dir_up_v2``
  to the per-level workgroup loop, ``top_body`` (``rnk > kWaveKids``) to its LDS loops.
* broom5: a slot with no junction child and more than ``kPre`` down-chain entries (phase A
  reads the fifth and sixth from global memory, ``pq`` false); broom33: 34 entries.
* cat70 at one job: more than ``kCapLvl`` levels and more than 64 slots in a job (``sLvl``
  against ``lvl_slot_off`` past the staged levels); cat300: more than ``kMaxTopLvl`` top
  levels at the default decomposition (``lds = false`` in ``nx_set_preconditioner``).
* hub9 at the default: a top slot with more than four children that are top slots themselves
  (the top part's register sweeps and ``top_wave`` dropped); hub70: 70 of them, 71 top slots.
* hubhub5x5 at 4 jobs: a more-than-four-kid slot inside a job that also has a top part.
* the random trees: hubs of 13-18 children with 19-22 entries, in jobs and in the top part,
  flipped chains everywhere.
* continuous pressure (``test_cp_model_on_hubs``): the node records hold ``kCpRecInc`` = 4
  incident edges and ``kCpRecCh`` = 3 children -- hub3's hub fills its record exactly (the third
  child slot is read), cat70 stays under both caps, every other hub and broom is past both
  (``r[3] = -1`` / ``r[kc] = -1``: the lists; ``cp_lev_full = 0``: the pipelined runs erased)."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from networks_fenicsx_amd import NetworkMesh
from networks_fenicsx_amd.assembly import edge_boundary_rhs, evaluate_nodal
from networks_fenicsx_amd.layout import build_local_problem
from networks_fenicsx_amd.layout_fe import (build_cp_tables, build_fe_layout, cp_model,
                                            evaluate_terms)
from networks_fenicsx_amd.precond import apply_model, build_tree_preconditioner, lumped_mass
from oracle import nx_cpu
from oracle import nx_oracle as O
from tree_shapes import (CP_RECORDS, JOBS, K_CAP_LVL, K_CP_REC_CH, K_CP_REC_INC, K_MAX_TOP_LVL,
                         K_PRE, K_WAVE_KIDS, K_WAVE_SLOTS, SHAPES, block_errors,
                         block_errors_oracle, check_cp_records, coefficients, cp_record_facts,
                         decomposition_facts, p_xy)

NAMES = list(SHAPES)


@functools.lru_cache(maxsize=None)
def _problem(name):
    make, N, _ = SHAPES[name]
    m = NetworkMesh(make(), N=N)
    src, dst = m.edges
    lp = build_local_problem(m.node_coordinates, src, dst, m.degrees, N)
    P = O.build_problem(m.node_coordinates, src, dst, N, m.edge_colors)
    return m, lp, P


@functools.lru_cache(maxsize=None)
def _facts(name, jobs):
    m, lp, _ = _problem(name)
    src, dst = m.edges
    pc = build_tree_preconditioner(lp, src, dst, m.degrees, target_jobs=jobs)
    assert pc.tree_exact
    return decomposition_facts(pc)


def test_generators_are_forests_with_distinct_nodes():
    for name in NAMES:
        m, lp, P = _problem(name)
        src, dst = m.edges
        assert src.size == m.num_nodes - 1, name  # connected (tree_shapes._place), so a tree
        pos = np.asarray(m.node_coordinates)
        assert np.unique(pos, axis=0).shape[0] == pos.shape[0], name
        assert np.linalg.norm(pos[dst] - pos[src], axis=1).min() > 0.1, name
        bnd = np.flatnonzero(m.degrees == 1)
        assert np.unique(np.round(p_xy(pos[bnd].T), 9)).size == bnd.size, name  # distinct p_bc


def test_shapes_hold_the_facts_they_are_there_for():
    f = _facts
    # kWaveKids: at the cap (all packed child words), one past it, far past it
    assert f("hub3", 1)["job_kids"] == K_WAVE_KIDS - 1 and f("hub3", 1)["job_entries"] == 4
    assert f("hub3", 4)["top_slots"] == 4 and f("hub3", 4)["top_top_kids"] == 3
    assert f("hub4", 1)["job_kids"] == K_WAVE_KIDS and f("hub4", 1)["job_entries"] == 5
    assert f("hub4", 4)["n_jobs"] == 4 and f("hub4", 4)["top_slots"] == 1
    assert f("hub4", 4)["top_kids"] == K_WAVE_KIDS
    assert f("hub4", 256)["top_slots"] == 5 and f("hub4", 256)["top_top_kids"] == K_WAVE_KIDS
    assert f("hub5", 1)["job_kids"] == K_WAVE_KIDS + 1 and f("hub5", 1)["job_entries"] == 6
    assert f("hub5", 1)["job_entries"] > K_PRE
    assert f("hub5", 4)["n_jobs"] == 5 and f("hub5", 4)["top_kids"] == 5
    assert f("hub5", 256)["top_slots"] == 6
    assert f("hub5", 256)["top_top_kids"] == K_WAVE_KIDS + 1
    assert f("hub9", 1)["job_kids"] == 9 and f("hub9", 1)["job_entries"] == 10
    assert f("hub9", 4)["n_jobs"] == 9 and f("hub9", 4)["top_kids"] == 9
    d = f("hub9", 256)
    assert (d["n_jobs"], d["top_slots"], d["need"]) == (2, 10, 10)
    assert d["top_top_kids"] == 9
    assert d["top_top_kids"] > K_WAVE_KIDS
    assert f("hub70", 1)["job_slots"] == 71
    assert f("hub70", 1)["job_slots"] > K_WAVE_SLOTS
    assert f("hub70", 1)["job_kids"] == 70
    assert f("hub70", 4)["n_jobs"] == 70
    d = f("hub70", 256)
    assert (d["n_jobs"], d["top_slots"], d["top_levels"], d["need"]) == (9, 71, 2, 23)
    assert d["top_top_kids"] == 70
    # kPre: entries past the prefetched four on a slot without a junction child
    d = f("broom5", 1)
    assert d["job_slots"] == 1 and d["job_kids"] == 0
    assert d["job_entries"] == 6
    assert d["job_entries"] > K_PRE
    assert f("broom5", 4)["top_slots"] == 1 and f("broom5", 4)["top_entries"] == 6
    assert f("broom33", 1)["job_entries"] == 34 and f("broom33", 1)["job_slots"] == 1
    assert f("broom33", 4)["n_jobs"] == 3 and f("broom33", 256)["n_jobs"] == 3
    # kCapLvl and the 64 slots of the one-wave sweeps; kMaxTopLvl
    d = f("cat70", 1)
    assert d["n_jobs"] == 1
    assert d["job_levels"] == 69
    assert d["job_levels"] > K_CAP_LVL
    assert d["job_slots"] == 69
    assert d["job_slots"] > K_WAVE_SLOTS
    d = f("cat70", 4)
    assert (d["top_slots"], d["top_levels"], d["need"]) == (69, 69, 37)
    assert f("cat70", 256)["n_jobs"] == 9 and f("cat70", 256)["top_levels"] == 69
    d = f("cat300", 1)
    assert d["top_levels"] == 60 and d["job_slots"] == 239
    assert d["job_levels"] == 239
    assert d["job_levels"] > K_CAP_LVL
    assert f("cat300", 4)["top_levels"] == 299
    assert f("cat300", 4)["top_levels"] > K_MAX_TOP_LVL
    d = f("cat300", 256)
    assert d["n_jobs"] == 38
    assert d["top_levels"] == 299
    assert d["top_levels"] > K_MAX_TOP_LVL
    # a hub inside a job under a top part
    d = f("hubhub5x5", 1)
    assert (d["job_slots"], d["job_levels"], d["job_kids"]) == (31, 3, 5)
    d = f("hubhub5x5", 4)
    assert d["n_jobs"] == 5 and d["top_slots"] == 1
    assert d["job_top_kids"] == 5
    assert d["job_top_kids"] > K_WAVE_KIDS
    d = f("hubhub5x5", 256)
    assert (d["n_jobs"], d["top_slots"], d["top_levels"]) == (6, 31, 3)
    assert d["top_top_kids"] == 5
    # random trees: hubs with many children and many entries, in jobs and in the top part
    for name in ("rand200_s1", "rand200_s2"):
        d = f(name, 1)
        assert d["job_slots"] == 78
        assert 13 <= d["job_kids"] <= 15
        assert 19 <= d["job_entries"] <= 22
        d = f(name, 4)
        assert 13 <= d["n_jobs"] <= 15
        assert d["job_top_kids"] > K_WAVE_KIDS
        assert d["top_kids"] >= 13
        d = f(name, 256)
        assert d["top_slots"] == 78
        assert 6 <= d["top_levels"] <= 9
        assert d["top_top_kids"] >= 13
    for j in (1, 4):
        d = f("rand600_s3", j)
        assert (d["n_jobs"], d["job_kids"], d["job_entries"]) == (18, 14, 21)
        assert (d["top_kids"], d["top_entries"]) == (18, 22)
    d = f("rand600_s3", 256)
    assert (d["n_jobs"], d["top_slots"], d["top_levels"]) == (38, 236, 7)


def test_block_errors_measure_each_block():
    """A flux error of 1e-6 relative to the fluxes, invisible in the 2-norm over the whole vector
    at 1e-8, shows in the flux block; a vanishing block is measured against |x|."""
    E, N = 3, 2
    per = 2 * N + 1
    x = np.zeros(E * per + 1)
    loc = np.arange(E * per) % per
    x[:E * per][loc % 2 == 1] = 100.0
    x[:E * per][loc % 2 == 0] = 1.0
    x[-1] = 0.0
    y = x.copy()
    y[0] += 3e-6
    eq, ep, el = block_errors(y, x, E, N)
    assert eq == pytest.approx(1e-6, rel=1e-3) and ep == 0.0 and el == 0.0
    assert np.linalg.norm(y - x) / np.linalg.norm(x) < 2e-8
    y = x.copy()
    y[-1] = 1e-3
    assert block_errors(y, x, E, N)[2] == pytest.approx(1e-3 / np.linalg.norm(x))
    q, p, l = block_errors_oracle(np.r_[1.0, 2.0, 3.0 + 3e-6, 5.0], np.r_[1.0, 2.0, 3.0, 5.0], 2, 3)
    assert q == 0.0 and p == pytest.approx(1e-6) and l == 0.0


@pytest.mark.parametrize("jobs", JOBS)
@pytest.mark.parametrize("name", NAMES)
def test_exact_model_three_iterations(name, jobs):
    """``apply_model(exact=True)`` on the decomposition: preconditioned MINRES reaches the sparse
    direct solution in <= 4 iterations (P^{-1} A has three eigenvalues)."""
    m, lp, P = _problem(name)
    src, dst = m.edges
    A, b = O.assemble_reference(P, p_xy)
    Ab, bb, _, _ = O.to_build_layout(P, A, b)
    pc = build_tree_preconditioner(lp, src, dst, m.degrees, target_jobs=jobs)
    dq = lumped_mass(Ab, lp)
    n = Ab.shape[0]
    rhs = np.random.default_rng(5).standard_normal(n)
    x_direct = spla.spsolve(Ab.tocsc(), rhs)
    its = [0]

    def count(_x):
        its[0] += 1

    M = spla.LinearOperator((n, n), matvec=lambda r: apply_model(pc, lp, dq, r, exact=True))
    x, info = spla.minres(Ab, rhs, M=M, rtol=1e-12, maxiter=50, callback=count)
    assert info == 0 and its[0] <= 4, its[0]
    assert np.linalg.norm(x - x_direct) <= 1e-10 * np.linalg.norm(x_direct)


@pytest.mark.parametrize("name", NAMES)
def test_cpu_direct_per_block(name):
    """The host port of the device's direct tree solve (the same formulas): 1 or 2 passes, true
    residual <= 1e-12, the oracle's solution to 1e-10 in every block (3.3e-13 at worst, the
    fluxes of cat70)."""
    m, lp, P = _problem(name)
    src, dst = m.edges
    pc = build_tree_preconditioner(lp, src, dst, m.degrees)
    bc = edge_boundary_rhs(m, lp.edges, evaluate_nodal(p_xy, m.node_coordinates))
    st = nx_cpu.CpuStep(lp, pc, bc)
    A, b = O.assemble_reference(P, p_xy)
    Ab, bb, perm, _ = O.to_build_layout(P, A, b)
    np.testing.assert_array_equal(st.val, Ab.data)
    np.testing.assert_array_equal(st.rhs, bb)
    passes, rr = st.solve_direct(1e-12)
    assert passes in (1, 2) and rr <= 1e-12, (passes, rr)
    err = block_errors(st.x, O.solve_reference(A, b)[perm], m.num_edges, m.N)
    print(name, "cpu port per block", err)
    assert max(err) <= 1e-10, err


@pytest.mark.parametrize("name", NAMES)
def test_references_agree_per_block(name):
    """SuperLU and the resistor-network answer (f = 0) agree to 1e-12 in every block, with
    R = 1 and, on the shapes that get one on the device, with the seeded per-edge R: the
    reference is two digits tighter than the 1e-10 it judges."""
    m, lp, P = _problem(name)
    Rs = [1.0] + ([coefficients(name, m.num_edges)["R"]] if SHAPES[name][2] else [])
    for R in Rs:
        A, b = O.assemble_reference(P, p_xy, R=R)
        x = O.solve_reference(A, b)
        xa = O.resistor_network_solution(P, p_xy, R=R)
        err = block_errors_oracle(x, xa, P.p_offset, P.lm_offset)
        print(name, "R" if np.ndim(R) else "1", err)
        assert max(err) <= 1e-12, err


@pytest.mark.parametrize("km", [(2, 1), (3, 2)])
@pytest.mark.parametrize("name", ["hub3", "hub4", "hub5", "hub9", "broom5", "broom33", "cat70",
                                  "rand200_s1"])
def test_cp_model_on_hubs(name, km):
    """Continuous pressure condensed onto the graph nodes (``layout_fe.cp_model``) against the
    sparse LU of the full system to 1e-10, with the facts of the node records asserted from
    ``build_cp_tables`` (``tree_shapes.check_cp_records``): hub3's hub has exactly
    ``kCpRecInc`` = 4 incident edges and ``kCpRecCh`` = 3 children (the record exactly full),
    cat70 stays under both caps, every other hub and broom has a node past both (hub4's hub
    by one each: 5 and 4), and so has the random tree."""
    k, mdeg = km
    make, N, _ = SHAPES[name]
    N = min(N, 6)
    mesh = NetworkMesh(make(), N=N)
    src, dst = mesh.edges
    pos = np.asarray(mesh.node_coordinates, dtype=np.float64)
    lay = build_fe_layout(pos, src, dst, mesh.degrees, N, k, mdeg)
    E = mesh.num_edges
    R = 1.0 + 0.25 * (np.arange(E) % 3)
    bc = np.random.default_rng(3).standard_normal((E, 2))
    h = np.repeat((np.linalg.norm(pos[dst] - pos[src], axis=1) / N)[:, None], N, axis=1)
    val, rhs = evaluate_terms(lay, R, 0.3, bc, h)
    A = sp.csr_matrix((val, lay.col, lay.rowptr), shape=(lay.n_rows, lay.n_rows))
    tab = build_cp_tables(lay, src, dst)
    assert tab is not None
    if name in CP_RECORDS:
        check_cp_records(name, tab)
    else:  # the random tree: hubs past both caps
        f = cp_record_facts(tab)
        assert f["inc"] > K_CP_REC_INC and f["ch"] > K_CP_REC_CH, f
    x_ref = spla.spsolve(A.tocsc(), rhs)
    x = cp_model(lay, tab, val, rhs, R, h)
    assert np.linalg.norm(x - x_ref) <= 1e-10 * np.linalg.norm(x_ref)
