"""The end-to-end cases of ``test_gpu_seg_shuffle_e2e.py`` and the recorder of their golden
file (not a test module).

One small tree, ``make_tree(5, 5, 5)`` (31 edges) split into 8 jobs, per lane shape that a small
N reaches through the lane-shape table (``sweep_lane_of`` / ``step_lane_of`` in csrc/nxhip.hip):

====  ==================  =====================================
 N    fused step          separate sweeps, MINRES, batch
====  ==================  =====================================
 15   ``<8, 2>`` (dense)  ``<8, 2>``
 19   ``<8, 3>``          ``<16, 2>``
 31   ``<8, 4>``          ``<16, 2>``
 40   ``<16, 4>``         ``<16, 4>``
====  ==================  =====================================

(No 4-lane shape exists: the table has none, and ``<4, 4>`` is not instantiated.) Every case
runs the fused step twice (the first stores the CSR values; at N = 15 the second is the values-free
``k_dir_step_kv``), the separate launches (``NXHIP_DIR_FUSED=0``), one MINRES solve and one
batch solve of two columns, and returns solution, rhs, CSR values and the reported residual
of each.

    python tests/seg_shuffle_cases.py OUT.npz

records them with whatever build of the package is first on ``sys.path``;
``tests/golden/seg_shuffle_parent.npz`` holds the arrays of the commit before the segment
helpers went from ``__shfl*`` to DPP row moves, recorded on an MI355X.
"""

from __future__ import annotations

import os
import sys

import numpy as np

NS = (15, 19, 31, 40)
JOBS = 8


def _pbc(x):
    return 2.0 * x[1] - 0.5 * x[0] + 1.0


def run_case(N: int) -> dict:
    """name -> array (a reported residual: a 0-d array) of one case's paths."""
    from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh
    from networks_fenicsx_amd import network_generation as ng
    from networks_fenicsx_amd.precond import build_tree_preconditioner

    mesh = NetworkMesh(ng.make_tree(5, 5, 5), N=N, color_strategy="smallest_last")
    asm = HydraulicNetworkAssembler(mesh)
    src, dst = mesh.edges
    asm._pc = build_tree_preconditioner(asm._local, src, dst, mesh.degrees, target_jobs=JOBS)
    asm.set_preconditioner(True)
    R = 0.5 + 0.25 * (np.arange(mesh.num_edges) % 7) ** 2
    asm.compute_forms(p_bc_ex=_pbc, R=R, f=0.75)
    asm.set_direct(True)
    h = asm.handle
    out = {}

    def keep(tag, rr):
        out[f"{tag}_solution"] = h.solution()
        out[f"{tag}_rhs"] = h.rhs()
        out[f"{tag}_csr_values"] = h.csr()[2]
        out[f"{tag}_relres"] = np.float64(rr)

    saved = os.environ.pop("NXHIP_DIR_FUSED", None)
    try:
        for tag in ("fused1", "fused2"):
            asm.assemble()
            it, rr, conv = h.solve(1e-12, 100, 4)
            assert h.direct_path() == "fused" and conv and it == 1, (tag, h.direct_path(), it, rr)
            keep(tag, rr)
        out["fused2_kept"] = np.int32(h.values_kept()["kept"])
        os.environ["NXHIP_DIR_FUSED"] = "0"
        asm.assemble()
        it, rr, conv = h.solve(1e-12, 100, 4)
        assert h.direct_path() == "launches" and conv and it == 1, (h.direct_path(), it, rr)
        keep("launches", rr)
    finally:
        os.environ.pop("NXHIP_DIR_FUSED", None)
        if saved is not None:
            os.environ["NXHIP_DIR_FUSED"] = saved
    asm.set_direct(False)  # MINRES on the assembled system
    it, rr, conv = h.solve(1e-12, 200, 4)
    assert conv and h.solver() == (0, 0), (it, rr)
    keep("minres", rr)
    out["minres_iterations"] = np.int32(it)
    asm.set_direct(True)
    bc0 = np.array(asm._coefficients["edge_bc"], dtype=np.float64).reshape(-1, 2)
    bc = np.stack([bc0, 2.0 * bc0 - 0.5])
    assert h.batch_supported()
    x, its, rrs, cv = h.batch_solve(bc, None, None, rtol=1e-12, blocks=False)
    assert cv.all(), (its, rrs)
    out["batch_solution"] = np.array(x, copy=True)
    out["batch_rhs"] = h.batch_rhs(bc)
    out["batch_relres"] = np.array(rrs, copy=True)
    asm.close()
    return out


def run_all() -> dict:
    return {f"N{N}_{k}": v for N in NS for k, v in run_case(N).items()}


if __name__ == "__main__":
    np.savez_compressed(sys.argv[1], **run_all())
    print(f"recorded {sys.argv[1]}")
