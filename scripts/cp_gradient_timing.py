#!/usr/bin/env python3
"""Milliseconds per scenario of ``Solver(batch_continuous=True).gradient`` for continuous
pressure, k > m >= 1 (``nx_cp_batch_gradient``: objective and all derivatives of a scenario)
against what a user had before it: ``Solver(batch_continuous=True).solve_many`` on the same
scenarios (``nx_cp_batch_solve``: one forward pass with its solution copy), in the same process,
at B = 1, 8, 64 on one MI355X (development / DESIGN numbers).

Central differences over ``solve_many`` would need 2 (2 E + boundary nodes) such scenarios per
gradient; that factor is printed, not timed.

Usage: python scripts/cp_gradient_timing.py [pairs [graphs [Bs [rounds]]]]
  pairs   comma list of k:m, default 2:1,3:2
  graphs  comma list of tree9 (make_tree(9,9,9), N = 15), c3 (make_tree(15,15,15), N = 15: the
          depth-14 tree); default both
  Bs      comma list, default 1,8,64
  rounds  alternating (least squares, linear, solve_many) timed rounds after 2 warm-up rounds,
          default 5
Prints min and median per call, per scenario, the gradient's cost in solve_many scenarios and
its launches."""

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
N_OBS = 12


def _timed(fn):
    t0 = time.perf_counter()
    res = fn()
    return 1e3 * (time.perf_counter() - t0), res


def main() -> int:
    pairs = [tuple(int(d) for d in v.split(":"))
             for v in (sys.argv[1] if len(sys.argv) > 1 else "2:1,3:2").split(",")]
    names = sys.argv[2].split(",") if len(sys.argv) > 2 else list(GRAPHS)
    Bs = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 8, 64]
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    opts = {"ksp_type": "preonly", "pc_type": "lu"}
    os.environ["NXHIP_BATCH"] = "1"  # (solve_many: also where the single-scenario rule says loop)
    for k, m in pairs:
        for name in names:
            make, N, strategy = GRAPHS[name]
            mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
            asm = HydraulicNetworkAssembler(mesh, flux_degree=k, pressure_degree=m)
            asm.compute_forms(p_bc_ex=lambda x: x[1],
                              R=0.5 + (np.arange(mesh.num_edges) % 3) / 2.0)
            solver = Solver(asm, petsc_options=opts, batch_continuous=True)
            solver.assemble()
            solver.solve()
            rng = np.random.default_rng(0)
            rows = rng.choice(asm.handle.n_rows, size=N_OBS, replace=False)
            w = 0.5 + rng.random(N_OBS)
            n_bnd = int((np.asarray(mesh.degrees) == 1).sum())
            fd = 2 * (2 * mesh.num_edges + n_bnd)
            for B in Bs:
                pbc = rng.standard_normal((B, mesh.num_nodes))
                f = 0.1 * rng.standard_normal(B)
                data = rng.standard_normal((B, N_OBS))
                calls = {
                    "lsq": lambda: solver.gradient(pbc, f, rows=rows, weights=w, data=data),
                    "linear": lambda: solver.gradient(pbc, f, rows=rows, weights=w),
                    "solve_many": lambda: solver.solve_many(pbc, f),
                }
                for _ in range(2):  # warm-up rounds (workspace, pinned outputs, first launches)
                    for fn in calls.values():
                        fn()
                t = {key: [] for key in calls}
                info = {}
                for _ in range(rounds):
                    for key, fn in calls.items():
                        dt, res = _timed(fn)
                        t[key].append(dt)
                        info[key] = res.info
                        assert res.converged.all()
                        assert key != "solve_many" or res.path == "batched"
                med = {key: float(np.median(v)) for key, v in t.items()}
                print(f"({k},{m}) {name} rows={asm.handle.n_rows} E={mesh.num_edges} B={B}: "
                      + " | ".join(f"{key} min {min(v) / B:.4f} median {med[key] / B:.4f} "
                                   f"ms/scenario" for key, v in t.items())
                      + f" | a gradient costs {med['lsq'] / med['solve_many']:.2f}x (lsq) "
                      f"{med['linear'] / med['solve_many']:.2f}x (linear) a solve_many scenario"
                      f" | central differences: {fd} scenarios per gradient"
                      f" | launches lsq {info['lsq']['launches']} linear "
                      f"{info['linear']['launches']} solve_many {info['solve_many']['launches']}"
                      f" chunk {info['lsq']['chunk']} refined {info['lsq']['refined']}",
                      flush=True)
            asm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
