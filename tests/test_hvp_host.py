"""Host side of ``Solver.hessian_vector``: the direction normalisation
(``assembly.hvp_directions``, no device) and the C ABI's new symbols."""

import numpy as np
import pytest

from networks_fenicsx_amd import NetworkMesh, _lib
from networks_fenicsx_amd import network_generation as ng
from networks_fenicsx_amd.assembly import edge_boundary_rhs, hvp_directions


@pytest.fixture(scope="module")
def mesh():
    return NetworkMesh(ng.make_tree(3, 2, 2), N=2)


@pytest.fixture(scope="module")
def edge_ids(mesh):
    # a local edge order that is not graph.edges() order
    return np.random.default_rng(0).permutation(mesh.num_edges)


def test_new_symbols_are_exported():
    assert "nx_batch_hvp" in _lib.EXPORTED_SYMBOLS
    assert "nx_ensemble_hvp" in _lib.EXPORTED_SYMBOLS


def test_shapes_and_local_edge_order(mesh, edge_ids):
    E, nn, B = mesh.num_edges, mesh.num_nodes, 3
    assert E != B and nn != B
    rng = np.random.default_rng(1)
    v_R, v_p, v_f = (rng.standard_normal((B, E)), rng.standard_normal((B, nn)),
                     rng.standard_normal((B, E)))
    dR, dbc, df = hvp_directions(mesh, edge_ids, B, v_R, v_p, v_f)
    assert dR.shape == (B, E) and dbc.shape == (B, E, 2) and df.shape == (B, E)
    assert dR.flags.c_contiguous and dbc.flags.c_contiguous and df.flags.c_contiguous
    np.testing.assert_array_equal(dR, v_R[:, edge_ids])
    np.testing.assert_array_equal(df, v_f[:, edge_ids])
    for j in range(B):
        np.testing.assert_array_equal(dbc[j], edge_boundary_rhs(mesh, edge_ids, v_p[j]))
    assert dbc.any()
    # only the boundary nodes' entries reach the direction
    inner = np.setdiff1d(np.arange(nn), np.concatenate([mesh.boundary_in_nodes,
                                                        mesh.boundary_out_nodes]))
    v_q = v_p.copy()
    v_q[:, inner] += 1.0
    np.testing.assert_array_equal(hvp_directions(mesh, edge_ids, B, v_p_bc=v_q)[1], dbc)


def test_one_dimensional_inputs_are_broadcast(mesh, edge_ids):
    E, nn, B = mesh.num_edges, mesh.num_nodes, 3
    rng = np.random.default_rng(2)
    v_R, v_p, v_f = rng.standard_normal(E), rng.standard_normal(nn), rng.standard_normal(E)
    dR, dbc, df = hvp_directions(mesh, edge_ids, B, v_R, v_p, v_f)
    for j in range(B):
        np.testing.assert_array_equal(dR[j], v_R[edge_ids])
        np.testing.assert_array_equal(df[j], v_f[edge_ids])
        np.testing.assert_array_equal(dbc[j], edge_boundary_rhs(mesh, edge_ids, v_p))
    # (B,) constants of v_f: one per scenario on every edge
    c = np.array([1.5, -2.0, 0.25])
    df = hvp_directions(mesh, edge_ids, B, v_f=c)[2]
    np.testing.assert_array_equal(df, np.repeat(c[:, None], E, axis=1))
    # lists are taken like arrays
    np.testing.assert_array_equal(hvp_directions(mesh, edge_ids, B, v_R=list(v_R))[0], dR)


def test_missing_part_is_zero_not_the_resident_source(mesh, edge_ids):
    E, B = mesh.num_edges, 2
    dR, dbc, df = hvp_directions(mesh, edge_ids, B, v_R=np.ones(E))
    assert dR is not None and dbc is None and df is None
    dR, dbc, df = hvp_directions(mesh, edge_ids, B, v_p_bc=np.ones(mesh.num_nodes))
    assert dR is None and dbc is not None and df is None
    dR, dbc, df = hvp_directions(mesh, edge_ids, B, v_f=np.ones(E))
    assert dR is None and dbc is None and df is not None


def test_negative_and_zero_v_R_are_accepted(mesh, edge_ids):
    E = mesh.num_edges
    v = -np.arange(E, dtype=np.float64)  # (zero and negative entries)
    np.testing.assert_array_equal(hvp_directions(mesh, edge_ids, 1, v_R=v)[0][0], v[edge_ids])


def test_value_errors(mesh, edge_ids):
    E, nn, B = mesh.num_edges, mesh.num_nodes, 3
    with pytest.raises(ValueError, match="direction"):
        hvp_directions(mesh, edge_ids, B)
    with pytest.raises(ValueError, match="v_R"):
        hvp_directions(mesh, edge_ids, B, v_R=np.ones((B + 1, E)))
    with pytest.raises(ValueError, match="v_R"):
        hvp_directions(mesh, edge_ids, B, v_R=np.ones(E + 1))
    with pytest.raises(ValueError, match="v_R"):
        hvp_directions(mesh, edge_ids, B, v_R=np.ones(B))  # (constants: v_f only)
    with pytest.raises(ValueError, match="v_p_bc"):
        hvp_directions(mesh, edge_ids, B, v_p_bc=np.ones((B, nn + 1)))
    with pytest.raises(ValueError, match="v_f"):
        hvp_directions(mesh, edge_ids, B, v_f=np.ones((B, E, 1)))
    with pytest.raises(ValueError, match="v_f"):
        hvp_directions(mesh, edge_ids, B, v_f=np.ones(B + 1))
    with pytest.raises(ValueError, match="finite"):
        hvp_directions(mesh, edge_ids, B, v_R=np.full(E, np.nan))
    with pytest.raises(ValueError, match="finite"):
        hvp_directions(mesh, edge_ids, B, v_f=np.array([0.0, np.inf, 1.0]))
    with pytest.raises(ValueError, match="scenario"):
        hvp_directions(mesh, edge_ids, 0, v_R=np.ones(E))
