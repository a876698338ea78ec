#!/usr/bin/env python3
"""Milliseconds per scenario of ``Solver.solve_many`` for continuous pressure (k > m >= 1) on a
forest: the batched pass (``nx_cp_batch_solve``, ``NXHIP_CP_BATCH=1``) against the sequential
loop (``NXHIP_CP_BATCH=0``: rhs coefficients, rhs assembly, the node-condensed direct solve and
gather per scenario -- the default) in the same process, at B = 1, 8, 64 on one MI355X
(development / DESIGN numbers).

Usage: python scripts/cp_batch_timing.py [degrees [graphs [Bs [pairs]]]]
  degrees comma list of k:m pairs, default 2:1,3:2
  graphs  comma list of tree9 (make_tree(9,9,9), N = 15), c3 (make_tree(15,15,15), N = 15);
          default both
  Bs      comma list, default 1,8,64
  pairs   alternating (batched, sequential) timed pairs after 2 warm-up pairs, default 5
Prints min and median per path, per scenario, the batched pass's launches and refined /
fallback columns, and the largest batched-against-loop difference."""

from __future__ import annotations

import os
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh, Solver  # noqa: E402
from networks_fenicsx_amd import network_generation as ng  # noqa: E402

GRAPHS = {
    "tree9": (lambda: ng.make_tree(9, 9, 9), 15, "smallest_last"),
    "c3": (lambda: ng.make_tree(15, 15, 15), 15, "smallest_last"),
}


def _run(asm, opts, pbc, f, batched: bool):
    # (the switch is read when the solver is made: one solver per path, outside the timing)
    os.environ["NXHIP_CP_BATCH"] = "1" if batched else "0"
    os.environ["NXHIP_BATCH"] = "1"  # (also where the single-scenario rule says loop)
    solver = Solver(asm, petsc_options=opts)
    t0 = time.perf_counter()
    res = solver.solve_many(pbc, f)
    dt = 1e3 * (time.perf_counter() - t0)
    os.environ.pop("NXHIP_CP_BATCH", None)
    os.environ.pop("NXHIP_BATCH", None)
    assert res.path == ("batched" if batched else "sequential"), res.path
    assert res.converged.all()
    return dt, res


def main() -> int:
    kms = [tuple(int(a) for a in v.split(":"))
           for v in (sys.argv[1] if len(sys.argv) > 1 else "2:1,3:2").split(",")]
    names = sys.argv[2].split(",") if len(sys.argv) > 2 else list(GRAPHS)
    Bs = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 8, 64]
    pairs = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    opts = {"ksp_type": "preonly", "pc_type": "lu"}
    for k, m in kms:
        for name in names:
            make, N, strategy = GRAPHS[name]
            mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
            asm = HydraulicNetworkAssembler(mesh, flux_degree=k, pressure_degree=m)
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
                print(f"(k, m)=({k}, {m}) {name} rows={asm.handle.n_rows} B={B}: batched min "
                      f"{min(tb) / B:.4f} median {float(np.median(tb)) / B:.4f} ms/scenario | "
                      f"sequential min {min(ts) / B:.4f} median {float(np.median(ts)) / B:.4f} "
                      f"ms/scenario | speed-up (medians) "
                      f"{float(np.median(ts)) / float(np.median(tb)):.2f}x | info {info} | "
                      f"max |x_b - x_s| / max |x_s| {err:.1e}", flush=True)
            asm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
