"""Continuous pressure (k > m >= 1) on graphs with cycles: the node-condensed solve's
low-rank correction (CPU model, layout_fe.cp_model with ``build_cp_tables(cycles=True)``).

The non-tree edges of the BFS forest are chords. The grounded node system S_g drops every
chord's two off-diagonal 2 x 2 border blocks (its diagonal blocks stay in its end nodes), so
the forest's level elimination inverts it unchanged; S = S_g + U C U^T over the distinct real
border slots at chord ends, and x = S_g^-1 (g - U w), w = (I + C U^T Z)^-1 C U^T x_g.
Checked against scipy's sparse LU of the full system to 1e-10 (the project's bar)."""

from __future__ import annotations

from dataclasses import fields

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from cases import CASES, CYCLIC
from networks_fenicsx_amd import NetworkMesh
from networks_fenicsx_amd.layout_fe import (build_cp_rank_tables, build_cp_tables,
                                            build_fe_layout, build_fe_partition, cp_model,
                                            evaluate_terms)
from networks_fenicsx_amd.layout import partition_edges

CHORDS = {"edge_info_N10": 2, "lattice4x5_N6": 12, "lattice6x6_N3": 25, "lattice19x20_N2": 342}


def _system(G, N, k, m, strategy=None):
    mesh = NetworkMesh(G, N=N, color_strategy=strategy)
    src, dst = mesh.edges
    pos = np.asarray(mesh.node_coordinates, dtype=np.float64)
    lay = build_fe_layout(pos, src, dst, mesh.degrees, N, k, m)
    E = mesh.num_edges
    R = 1.0 + 0.25 * (np.arange(E) % 3)
    bc = np.random.default_rng(3).standard_normal((E, 2))
    L = np.linalg.norm(pos[dst] - pos[src], axis=1)
    h = np.repeat((L / N)[:, None], N, axis=1)
    val, rhs = evaluate_terms(lay, R, 0.3, bc, h)
    A = sp.csr_matrix((val, lay.col, lay.rowptr), shape=(lay.n_rows, lay.n_rows))
    return mesh, lay, A, val, rhs, R, h


@pytest.fixture(scope="module")
def cyclic_tables():
    """(mesh, layout, tables) of every CYCLIC graph at (2, 1), N = 2: built once, read only."""
    out = {}
    for name, (make, _) in CYCLIC.items():
        mesh = NetworkMesh(make(), N=2)
        src, dst = mesh.edges
        lay = build_fe_layout(np.asarray(mesh.node_coordinates, dtype=np.float64), src, dst,
                              mesh.degrees, 2, 2, 1)
        out[name] = (mesh, lay, build_cp_tables(lay, src, dst, cycles=True))
    return out


@pytest.mark.parametrize("case", ["Y_N4", "tree5_N15", "linear_alt_N3"])
def test_forest_tables_unchanged(case):
    make, N, strategy, _ = CASES[case]
    mesh = NetworkMesh(make(), N=min(N, 4), color_strategy=strategy)
    src, dst = mesh.edges
    lay = build_fe_layout(np.asarray(mesh.node_coordinates, dtype=np.float64), src, dst,
                          mesh.degrees, min(N, 4), 2, 1)
    t0 = build_cp_tables(lay, src, dst)
    t1 = build_cp_tables(lay, src, dst, cycles=True)
    assert t0 is not None and t1 is not None
    assert np.asarray(t1.chord).size == 0 and np.asarray(t1.cslot).size == 0
    assert np.asarray(t0.chord).size == 0 and np.asarray(t0.cslot).size == 0
    for f in fields(t0):
        a, b = getattr(t0, f.name), getattr(t1, f.name)
        if isinstance(a, np.ndarray):
            assert a.dtype == b.dtype, f.name
            np.testing.assert_array_equal(a, b, err_msg=f.name)
        else:
            assert a == b, f.name


@pytest.mark.parametrize("case", list(CYCLIC))
def test_chords_leave_a_spanning_forest(case, cyclic_tables):
    mesh, lay, tab = cyclic_tables[case]
    assert tab is not None
    chord = np.asarray(tab.chord)
    assert chord.size == CHORDS[case]
    assert np.all(np.diff(chord) > 0)  # once each, ascending
    n = tab.n_nodes
    par = np.asarray(tab.parent).reshape(n, 3)
    eb = np.asarray(tab.eb).reshape(-1, 4)
    # every tree edge is some node's parent edge, no chord is; E - chords = n - components
    tree = par[par[:, 1] >= 0, 1]
    assert np.intersect1d(tree, chord).size == 0
    assert np.unique(tree).size == tree.size == lay.E - chord.size
    # the parent edge joins the node to its parent
    for nd in np.flatnonzero(par[:, 0] >= 0):
        p, e, end = par[nd]
        assert eb[e, end] == nd and eb[e, 1 - end] == p
    # parent reaches a root from every node (no loop among the parents)
    cur = np.arange(n)
    for _ in range(n):
        up = par[cur, 0]
        cur = np.where(up >= 0, up, cur)
    assert np.all(par[cur, 0] < 0)
    # the levels hold every node once; inc keeps every edge, chords included
    assert np.array_equal(np.sort(np.asarray(tab.order)), np.arange(n))
    inc = np.asarray(tab.inc).reshape(-1, 2)
    assert np.array_equal(np.bincount(inc[:, 0], minlength=lay.E), np.full(lay.E, 2))


@pytest.mark.parametrize("case", list(CYCLIC))
def test_cslot_sorted_distinct_real(case, cyclic_tables):
    _, _, tab = cyclic_tables[case]
    cs = np.asarray(tab.cslot).reshape(-1, 2)
    key = 2 * cs[:, 0].astype(np.int64) + cs[:, 1]
    assert np.all(np.diff(key) > 0)
    eb = np.asarray(tab.eb).reshape(-1, 4)
    nrow = np.asarray(tab.nrow).reshape(-1, 2)
    ends = np.unique(eb[np.asarray(tab.chord)][:, :2])
    want = [(a, 0) for a in ends] + [(a, 1) for a in ends if nrow[a, 1] >= 0]
    assert sorted(map(tuple, cs.tolist())) == sorted(want)


def test_self_loop_and_parallel_edges():
    pos = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0.5, 0]])

    def tables(src, dst):
        src, dst = np.asarray(src), np.asarray(dst)
        deg = np.bincount(np.concatenate([src, dst]), minlength=3)
        lay = build_fe_layout(pos, src, dst, deg, 2, 2, 1)
        return build_cp_tables(lay, src, dst, cycles=True)

    tab = tables([0, 1, 1], [1, 2, 2])  # two edges between nodes 1 and 2: the second a chord
    assert tab is not None
    np.testing.assert_array_equal(tab.chord, [2])
    np.testing.assert_array_equal(np.asarray(tab.cslot).reshape(-1, 2),
                                  [[1, 0], [1, 1], [2, 0], [2, 1]])
    src, dst = np.array([0, 1, 1]), np.array([1, 2, 2])
    lay = build_fe_layout(pos, src, dst, np.array([1, 3, 2]), 2, 2, 1)
    assert build_cp_tables(lay, src, np.array([1, 2, 1]), cycles=True) is None  # a self-loop


def _check_model(case, N, k, m):
    mesh, lay, A, val, rhs, R, h = _system(CYCLIC[case][0](), N, k, m)
    src, dst = mesh.edges
    tab = build_cp_tables(lay, src, dst, cycles=True)
    assert tab is not None and np.asarray(tab.chord).size == CHORDS[case]
    x_ref = spla.spsolve(A.tocsc(), rhs)
    info = {}
    x = cp_model(lay, tab, val, rhs, R, h, info=info)
    err = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
    res = np.linalg.norm(rhs - A @ x) / np.linalg.norm(rhs)
    print(f"{case} ({k},{m}) N={N}: err {err:.2e} res {res:.2e} "
          f"cond(cap) {np.linalg.cond(info['cap']):.2e}")
    # the grounded sweep's pivots: negative definite (the multiplier's dummy slot: +1)
    nrow = np.asarray(tab.nrow).reshape(-1, 2)
    ev = np.linalg.eigvalsh(0.5 * (info["Pinv"] + info["Pinv"].transpose(0, 2, 1)))
    neg = (ev < 0).sum(axis=1)
    assert np.array_equal(neg, np.where(nrow[:, 1] >= 0, 2, 1))
    assert err <= 1e-10
    assert res <= 1e-11  # one pass, no refinement


@pytest.mark.parametrize("case,N", [("edge_info_N10", 10), ("lattice4x5_N6", 6),
                                    ("lattice6x6_N3", 3)])
@pytest.mark.parametrize("km", [(2, 1), (3, 1), (3, 2), (4, 3)])
def test_corrected_solve_equals_lu(case, N, km):
    """Error <= 1e-10 and a one-pass true residual <= 1e-11, test_fe_cp.py's bars (measured:
    error <= 3.2e-13, residual <= 2.7e-13). Without the grounded solve's one refinement
    sweep the residual on edge_info at N = 10 (edges 0.1 and 0.3 long in ten cells) is
    1.58e-11 for (3, 1) and 1.93e-11 for (4, 3): the 2 x 2 pivots' explicit inverses."""
    _check_model(case, N, *km)


def test_corrected_solve_equals_lu_342_chords():
    _check_model("lattice19x20_N2", 2, 2, 1)


def test_no_chords_is_the_forest_model():
    """Without chords cp_model is the forest's: the same bits with either table."""
    make, N, strategy, _ = CASES["Y_N4"]
    mesh, lay, A, val, rhs, R, h = _system(make(), N, 3, 2, strategy)
    src, dst = mesh.edges
    x0 = cp_model(lay, build_cp_tables(lay, src, dst), val, rhs, R, h)
    x1 = cp_model(lay, build_cp_tables(lay, src, dst, cycles=True), val, rhs, R, h)
    np.testing.assert_array_equal(x0, x1)


@pytest.mark.parametrize("nranks", [2, 3])
def test_rank_tables_keep_chords(nranks):
    mesh = NetworkMesh(CYCLIC["edge_info_N10"][0](), N=4)
    src, dst = mesh.edges
    pos = np.asarray(mesh.node_coordinates, dtype=np.float64)
    full = build_fe_layout(pos, src, dst, mesh.degrees, 4, 2, 1)
    tab = build_cp_tables(full, src, dst, cycles=True)
    owner = partition_edges(src, dst, pos.shape[0], nranks)
    for rank in range(nranks):
        part = build_fe_partition(full, src, dst, owner, rank, nranks)
        tr, gid, nrowx = build_cp_rank_tables(tab, part)
        np.testing.assert_array_equal(tr.chord, tab.chord)
        np.testing.assert_array_equal(tr.cslot, tab.cslot)
        assert np.asarray(tr.chord).size == 2
        # the slots' multiplier entries are the nodes whose summed rhs has a multiplier row
        nb = np.asarray(tr.nrow).reshape(-1, 2)
        cs = np.asarray(tr.cslot).reshape(-1, 2)
        assert np.all(nb[cs[:, 0], cs[:, 1]] == 2 * cs[:, 0] + cs[:, 1])
