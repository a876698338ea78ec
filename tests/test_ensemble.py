"""The host side of ``Solver.solve_ensemble``: the normalisation of B resistance fields and
their boundary / source data into what ``nx_ensemble_solve`` takes (no device)."""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest

from cases import p_y
from networks_fenicsx_amd import NetworkMesh
from networks_fenicsx_amd import network_generation as ng
from networks_fenicsx_amd.assembly import (HydraulicNetworkAssembler, batch_coefficients,
                                           edge_boundary_rhs, ensemble_resistances,
                                           evaluate_nodal)


@pytest.fixture(scope="module")
def mesh():
    return NetworkMesh(ng.make_tree(3, 2, 2), N=2)


def test_per_edge_rows_go_to_the_local_edge_order(mesh):
    E = mesh.num_edges
    R = 1.0 + np.arange(3 * E, dtype=np.float64).reshape(3, E)
    ids = np.random.default_rng(0).permutation(E)  # a local order that is not graph.edges()'s
    out = ensemble_resistances(mesh, ids, R)
    assert out.shape == (3, E) and out.flags.c_contiguous and out.dtype == np.float64
    np.testing.assert_array_equal(out, R[:, ids])
    sub = ids[: E // 2]  # a rank's share of the edges
    np.testing.assert_array_equal(ensemble_resistances(mesh, sub, R), R[:, sub])
    np.testing.assert_array_equal(ensemble_resistances(mesh, ids, R.tolist()), R[:, ids])


def test_constants_are_one_per_scenario(mesh):
    E = mesh.num_edges
    ids = np.arange(E)
    out = ensemble_resistances(mesh, ids, np.array([1.0, 3.7]))
    assert out.shape == (2, E)
    np.testing.assert_array_equal(out[0], np.full(E, 1.0))
    np.testing.assert_array_equal(out[1], np.full(E, 3.7))
    np.testing.assert_array_equal(ensemble_resistances(mesh, ids, [2.0, 0.5]),
                                  np.stack([np.full(E, 2.0), np.full(E, 0.5)]))
    # a 1-D R of num_edges values is num_edges scenarios of constants, never one per-edge row
    assert ensemble_resistances(mesh, ids, 1.0 + np.arange(E)).shape == (E, E)


@pytest.mark.parametrize("bad", [
    lambda E: np.ones((2, E + 1)),      # not one value per graph edge
    lambda E: np.ones((2, E, 1)),       # too many dimensions
    lambda E: np.float64(1.0),          # a scalar is not a batch
    lambda E: np.ones((0, E)),          # no scenario
    lambda E: np.zeros(0),
    lambda E: np.array([1.0, 0.0]),     # not positive
    lambda E: np.array([1.0, -2.0]),
    lambda E: np.array([1.0, np.nan]),  # not finite
    lambda E: np.array([np.inf, 1.0]),
    lambda E: np.where(np.arange(2 * E).reshape(2, E) == E + 1, 0.0, 1.0),
])
def test_value_errors(mesh, bad):
    with pytest.raises(ValueError):
        ensemble_resistances(mesh, np.arange(mesh.num_edges), bad(mesh.num_edges))


def _stub(mesh, ids):
    """What ``ensemble_coefficients`` reads of an assembler after ``compute_forms(p_y)``."""
    pbc = evaluate_nodal(p_y, mesh.node_coordinates)
    return SimpleNamespace(_network_mesh=mesh, _edge_ids=ids, _coefficients={"p_bc": pbc}), pbc


def test_p_bc_none_repeats_the_last_compute_forms(mesh):
    E = mesh.num_edges
    ids = np.arange(E)[::-1].copy()
    stub, pbc = _stub(mesh, ids)
    R = np.array([1.0, 2.0, 0.25])
    eR, bc, ef, fc = HydraulicNetworkAssembler.ensemble_coefficients(stub, R)
    assert eR.shape == (3, E) and bc.shape == (3, E, 2) and ef is None and fc is None
    one = edge_boundary_rhs(mesh, ids, pbc)
    assert one.any()
    for j in range(3):
        np.testing.assert_array_equal(bc[j], one)


def test_p_bc_and_f_as_solve_many_takes_them(mesh):
    E, nn = mesh.num_edges, mesh.num_nodes
    ids = np.arange(E)
    stub, _ = _stub(mesh, ids)
    items = [p_y, np.linspace(0.0, 1.0, nn)]
    f = np.arange(2 * E, dtype=np.float64).reshape(2, E)
    eR, bc, ef, fc = HydraulicNetworkAssembler.ensemble_coefficients(stub, [1.5, 2.5], items, f)
    bc0, ef0, fc0 = batch_coefficients(mesh, ids, items, f)
    np.testing.assert_array_equal(bc, bc0)
    np.testing.assert_array_equal(ef, ef0)
    assert fc is None and fc0 is None
    with pytest.raises(ValueError):  # three resistance fields, two boundary scenarios
        HydraulicNetworkAssembler.ensemble_coefficients(stub, [1.0, 2.0, 3.0], items)
    with pytest.raises(ValueError):
        HydraulicNetworkAssembler.ensemble_coefficients(stub, [1.0, 2.0], items, np.ones(3))
