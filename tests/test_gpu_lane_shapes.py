"""Which ``<W, CPL>`` lane shape an edge of N cells selects (``nx_get_lane_shapes``), at every
N where the selection changes. The solve tests cannot see the selection -- a too-wide shape
still gives right answers -- so the table of csrc/nxhip.hip (``sweep_lane_of`` /
``step_lane_of``) is written out here. No solve: the shapes are chosen
when the preconditioner is uploaded."""

from __future__ import annotations

import pytest

import unlike_ranks
from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh, _lib
from networks_fenicsx_amd import network_generation as ng

pytestmark = pytest.mark.gpu

# (largest N of the range, sweeps, one-launch / exchange step); (0, 0): no one-launch instantiation
TABLE = [
    (16, (8, 2), (8, 2)),
    (24, (16, 2), (8, 3)),
    (32, (16, 2), (8, 4)),
    (64, (16, 4), (16, 4)),
    (128, (64, 2), (64, 2)),
    (256, (64, 4), (64, 4)),
    (512, (64, 8), (0, 0)),
    (1024, (64, 16), (0, 0)),
]


def expected(N: int):
    return next((sweep, step) for top, sweep, step in TABLE if N <= top)


@pytest.mark.parametrize("N", [1, 16, 17, 24, 25, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024])
def test_lane_shapes(N):
    mesh = NetworkMesh(ng.make_tree(3, 1, 1), N=N)
    asm = HydraulicNetworkAssembler(mesh)
    asm.compute_forms(p_bc_ex=lambda x: x[1])
    assert asm.set_preconditioner(True)
    sweep, step = asm.handle.lane_shapes()
    assert (sweep, step) == expected(N)
    if N <= 64:
        assert unlike_ranks.lane_shape(N) == step


def test_lane_shapes_need_a_preconditioner():
    asm = HydraulicNetworkAssembler(NetworkMesh(ng.make_tree(3, 1, 1), N=15))
    asm.compute_forms(p_bc_ex=lambda x: x[1])
    asm.set_preconditioner(False)
    with pytest.raises(_lib.NxError, match=f"error {_lib.NX_ERR_STATE}:"):
        asm.handle.lane_shapes()
