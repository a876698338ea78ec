#!/usr/bin/env python3
"""Milliseconds per scenario of ``Solver.solve_many`` for flux degree k >= 2 with DG0 pressure:
the batched pass (``nx_fe_batch_solve``, ``NXHIP_FE_BATCH=1``) against the sequential loop
(``NXHIP_FE_BATCH=0``: rhs coefficients, rhs assembly, the condensed direct solve and gather per
scenario -- the default) in the same process, at B = 1, 8, 64 on one MI355X (development /
DESIGN numbers).

Usage: python scripts/fe_batch_timing.py [degrees [graphs [Bs [pairs]]]]
  degrees comma list of flux degrees, default 2,3
  graphs  comma list of tree9 (make_tree(9,9,9), N = 15), c3 (make_tree(15,15,15), N = 15),
          lattice (lattice19x20, N = 2); default all three
  Bs      comma list, default 1,8,64
  pairs   alternating (batched, sequential) timed pairs after 2 warm-up pairs, default 5
Prints min and median per path, per scenario, and the batched pass's launches."""

from __future__ import annotations

import os
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

from cases import lattice_graph  # noqa: E402
from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh, Solver  # noqa: E402
from networks_fenicsx_amd import network_generation as ng  # noqa: E402

GRAPHS = {
    "tree9": (lambda: ng.make_tree(9, 9, 9), 15, "smallest_last"),
    "c3": (lambda: ng.make_tree(15, 15, 15), 15, "smallest_last"),
    "lattice": (lambda: lattice_graph(19, 20), 2, None),
}


def _run(asm, opts, pbc, f, batched: bool):
    # (the switch is read when the solver is made: one solver per path, outside the timing)
    os.environ["NXHIP_FE_BATCH"] = "1" if batched else "0"
    os.environ["NXHIP_BATCH"] = "1"  # (also where the single-scenario rule says loop)
    solver = Solver(asm, petsc_options=opts)
    t0 = time.perf_counter()
    res = solver.solve_many(pbc, f)
    dt = 1e3 * (time.perf_counter() - t0)
    os.environ.pop("NXHIP_FE_BATCH", None)
    os.environ.pop("NXHIP_BATCH", None)
    assert res.path == ("batched" if batched else "sequential"), res.path
    assert res.converged.all()
    return dt, res


def main() -> int:
    ks = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [2, 3]
    names = sys.argv[2].split(",") if len(sys.argv) > 2 else list(GRAPHS)
    Bs = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 8, 64]
    pairs = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    opts = {"ksp_type": "preonly", "pc_type": "lu"}
    for k in ks:
        for name in names:
            make, N, strategy = GRAPHS[name]
            mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
            asm = HydraulicNetworkAssembler(mesh, flux_degree=k, pressure_degree=0)
            asm.compute_forms(p_bc_ex=lambda x: x[1],
                              R=0.5 + (np.arange(mesh.num_edges) % 3) / 2.0)
            solver = Solver(asm, petsc_options=opts)
            solver.assemble()
            solver.solve()
            rng = np.random.default_rng(0)
            for B in Bs:
                pbc = rng.standard_normal((B, mesh.num_nodes))
                f = 0.1 * rng.standard_normal(B)
                for _ in range(2):  # warm-up pairs (workspace, pinned output, first launches)
                    _run(asm, opts, pbc, f, True)
                    _run(asm, opts, pbc, f, False)
                tb, ts, info, err = [], [], None, 0.0
                for _ in range(pairs):
                    dt, rb = _run(asm, opts, pbc, f, True)
                    tb.append(dt)
                    info = rb.info
                    dt, rs = _run(asm, opts, pbc, f, False)
                    ts.append(dt)
                    err = max(err, float(np.abs(rb.x - rs.x).max() / np.abs(rs.x).max()))
                print(f"k={k} {name} rows={asm.handle.n_rows} B={B}: batched min "
                      f"{min(tb) / B:.4f} median {float(np.median(tb)) / B:.4f} ms/scenario | "
                      f"sequential min {min(ts) / B:.4f} median {float(np.median(ts)) / B:.4f} "
                      f"ms/scenario | speed-up (medians) "
                      f"{float(np.median(ts)) / float(np.median(tb)):.2f}x | info {info} | "
                      f"max |x_b - x_s| / max |x_s| {err:.1e}", flush=True)
            asm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
