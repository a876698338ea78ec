#!/usr/bin/env python3
"""Milliseconds per scenario of ``Solver.solve_many``: the batched pass (``nx_batch_solve``)
against the sequential loop in the same process (``NXHIP_BATCH=0``: rhs coefficients, rhs
assembly, solve and gather per scenario -- what a caller had before the batched call), at
B = 1, 8, 64 on one MI355X (development / DESIGN numbers).

Usage: python scripts/batch_timing.py [graphs [Bs [pairs]]]
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


def _run(solver, pbc, f, batched: bool):
    os.environ["NXHIP_BATCH"] = "1" if batched else "0"  # (1: also where the rule says loop)
    t0 = time.perf_counter()
    res = solver.solve_many(pbc, f)
    dt = 1e3 * (time.perf_counter() - t0)
    os.environ.pop("NXHIP_BATCH", None)
    assert res.path == ("batched" if batched else "sequential"), res.path
    assert res.converged.all()
    return dt, res


def main() -> int:
    names = sys.argv[1].split(",") if len(sys.argv) > 1 else list(GRAPHS)
    Bs = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 8, 64]
    pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    for name in names:
        make, N, strategy = GRAPHS[name]
        mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
        asm = HydraulicNetworkAssembler(mesh)
        asm.compute_forms(p_bc_ex=lambda x: x[1], R=0.5 + (np.arange(mesh.num_edges) % 3) / 2.0)
        solver = Solver(asm, petsc_options={"ksp_type": "preonly", "pc_type": "lu"})
        solver.assemble()
        solver.solve()
        rng = np.random.default_rng(0)
        for B in Bs:
            pbc = rng.standard_normal((B, mesh.num_nodes))
            f = 0.1 * rng.standard_normal(B)
            for _ in range(2):  # warm-up pairs (workspace, pinned output, first launches)
                _run(solver, pbc, f, True)
                _run(solver, pbc, f, False)
            tb, ts, info, err = [], [], None, 0.0
            for _ in range(pairs):
                dt, rb = _run(solver, pbc, f, True)
                tb.append(dt)
                info = rb.info
                dt, rs = _run(solver, pbc, f, False)
                ts.append(dt)
                err = max(err, float(np.abs(rb.x - rs.x).max() / np.abs(rs.x).max()))
            print(f"{name} rows={asm.handle.n_rows} B={B}: batched min {min(tb) / B:.4f} "
                  f"median {float(np.median(tb)) / B:.4f} ms/scenario | sequential min "
                  f"{min(ts) / B:.4f} median {float(np.median(ts)) / B:.4f} ms/scenario | "
                  f"speed-up (medians) {float(np.median(ts)) / float(np.median(tb)):.2f}x | "
                  f"info {info} | max |x_b - x_s| / max |x_s| {err:.1e}", flush=True)
        asm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
