"""``batch_coefficients`` (no device): the rhs coefficients of B scenarios as
``nx_batch_solve`` takes them equal the per-scenario normalisation of ``compute_forms``
(``evaluate_nodal`` + ``edge_boundary_rhs``), for every accepted form of ``p_bc`` and ``f``."""

from __future__ import annotations

import numpy as np
import pytest

from cases import CASES, p_x, p_y
from networks_fenicsx_amd import NetworkMesh
from networks_fenicsx_amd.assembly import batch_coefficients, edge_boundary_rhs, evaluate_nodal


class _Eval:
    """The PressureFunction protocol: an object with ``eval(x)``."""

    def eval(self, x):
        return 2.0 * x[0] - x[1]


@pytest.fixture(scope="module")
def mesh():
    make, N, strategy, _ = CASES["tree5_N15"]
    return NetworkMesh(make(), N=N, color_strategy=strategy)


def _edge_ids(mesh):
    # a permuted subset-free order: the helper must follow the local edge order it is given
    return np.random.default_rng(3).permutation(mesh.num_edges)


def _one(mesh, ids, item):
    return edge_boundary_rhs(mesh, ids, evaluate_nodal(item, mesh.node_coordinates))


def test_pbc_forms_match_per_scenario_normalisation(mesh):
    ids = _edge_ids(mesh)
    nodal = np.random.default_rng(0).standard_normal(mesh.num_nodes)
    items = [p_y, p_x, _Eval(), nodal, 3.5, lambda x: np.zeros(x.shape[1])]
    bc, ef, fc = batch_coefficients(mesh, ids, items)
    assert bc.shape == (len(items), mesh.num_edges, 2) and bc.dtype == np.float64
    assert ef is None and fc is None
    for j, item in enumerate(items):
        np.testing.assert_array_equal(bc[j], _one(mesh, ids, item))
    # only terminals carry a value, with the reference's signs
    src, dst = mesh.edges
    inner = ~np.isin(src[ids], mesh.boundary_out_nodes)
    assert np.all(bc[:, inner, 0] == 0.0)
    assert np.all(bc[3, ~inner, 0] == -nodal[src[ids][~inner]])


def test_pbc_array_of_nodal_values(mesh):
    ids = np.arange(mesh.num_edges)
    arr = np.random.default_rng(1).standard_normal((4, mesh.num_nodes))
    bc, _, _ = batch_coefficients(mesh, ids, arr)
    for j in range(4):
        np.testing.assert_array_equal(bc[j], edge_boundary_rhs(mesh, ids, arr[j]))
    # a tuple of rows is the same batch
    np.testing.assert_array_equal(batch_coefficients(mesh, ids, tuple(arr))[0], bc)


def test_f_none_scalars_and_per_edge(mesh):
    ids = _edge_ids(mesh)
    items = [p_y, p_x, 1.0]
    assert batch_coefficients(mesh, ids, items, None)[1:] == (None, None)
    bc, ef, fc = batch_coefficients(mesh, ids, items, [0.0, 0.25, -1.0])
    assert ef is None
    np.testing.assert_array_equal(fc, [0.0, 0.25, -1.0])
    assert fc.dtype == np.float64 and fc.flags.c_contiguous
    per_edge = 0.1 + 0.02 * (np.arange(3 * mesh.num_edges).reshape(3, -1) % 5)
    bc2, ef, fc = batch_coefficients(mesh, ids, items, per_edge)
    assert fc is None and ef.shape == (3, mesh.num_edges) and ef.flags.c_contiguous
    # graph.edges() order in, local edge order out -- as compute_forms' f[edge_ids]
    for j in range(3):
        np.testing.assert_array_equal(ef[j], per_edge[j][ids])
    np.testing.assert_array_equal(bc2, bc)


def test_wrong_shapes_raise(mesh):
    ids = np.arange(mesh.num_edges)
    with pytest.raises(ValueError):
        batch_coefficients(mesh, ids, np.zeros((2, mesh.num_nodes + 1)))
    with pytest.raises(ValueError):
        batch_coefficients(mesh, ids, np.zeros(mesh.num_nodes))  # one scenario: not a batch
    with pytest.raises(ValueError):
        batch_coefficients(mesh, ids, [np.zeros(mesh.num_nodes - 1)])
    with pytest.raises(ValueError):
        batch_coefficients(mesh, ids, [])
    with pytest.raises(ValueError):
        batch_coefficients(mesh, ids, p_y)  # a single callable is not a sequence
    with pytest.raises(ValueError):
        batch_coefficients(mesh, ids, [p_y, p_x], [1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        batch_coefficients(mesh, ids, [p_y, p_x], np.zeros((2, mesh.num_edges - 1)))
    with pytest.raises(ValueError):
        batch_coefficients(mesh, ids, [p_y, p_x], np.zeros((3, mesh.num_edges)))
