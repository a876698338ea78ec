#!/usr/bin/env python3
"""Milliseconds per scenario of ``Solver.gradient`` (``nx_batch_gradient``: two batched direct
solves, ``4 E + 1`` doubles per scenario to the host) against ``Solver.solve_many``'s batched
pass on the same scenarios (``nx_batch_solve``: the forward solve alone with its copy of the
solution to the host -- what a caller doing the adjoint algebra on the host starts from), at
B = 1, 8, 64 on one MI355X (development / DESIGN numbers).

Usage: python scripts/gradient_timing.py [graphs [Bs [pairs]]]
  graphs  comma list of tree9 (make_tree(9,9,9), N = 15), c3 (make_tree(15,15,15), N = 15),
          lattice (lattice19x20, N = 2); default all three
  Bs      comma list, default 1,8,64
  pairs   alternating (linear gradient, least-squares gradient, solve_many) timed rounds
          after 2 warm-up rounds, default 5
Prints min and median per call kind, per scenario, and the calls' launches. For the kernel
times of k_b_obs / k_b_edge_form run it under ``rocprofv3 --kernel-trace --stats`` (a run of its
own, not a timed one)."""

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
N_OBS = 12


def _timed(fn):
    t0 = time.perf_counter()
    res = fn()
    return 1e3 * (time.perf_counter() - t0), res


def main() -> int:
    names = sys.argv[1].split(",") if len(sys.argv) > 1 else list(GRAPHS)
    Bs = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 8, 64]
    pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    os.environ["NXHIP_BATCH"] = "1"  # solve_many's batched pass also at B = 1 on a large system
    for name in names:
        make, N, strategy = GRAPHS[name]
        mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
        asm = HydraulicNetworkAssembler(mesh)
        asm.compute_forms(p_bc_ex=lambda x: x[1], R=0.5 + (np.arange(mesh.num_edges) % 3) / 2.0)
        solver = Solver(asm, petsc_options={"ksp_type": "preonly", "pc_type": "lu"})
        solver.assemble()
        solver.solve()
        rng = np.random.default_rng(0)
        rows = rng.choice(asm.handle.n_rows, size=N_OBS, replace=False)
        w = 0.5 + rng.random(N_OBS)
        for B in Bs:
            pbc = rng.standard_normal((B, mesh.num_nodes))
            f = 0.1 * rng.standard_normal(B)
            data = rng.standard_normal((B, N_OBS))
            calls = {
                "linear": lambda: solver.gradient(pbc, f, rows=rows, weights=w),
                "lsq": lambda: solver.gradient(pbc, f, rows=rows, weights=w, data=data),
                "solve_many": lambda: solver.solve_many(pbc, f),
            }
            for _ in range(2):  # warm-up rounds (workspace, pinned output, first launches)
                for fn in calls.values():
                    fn()
            t = {k: [] for k in calls}
            info = {}
            for _ in range(pairs):
                for k, fn in calls.items():
                    dt, res = _timed(fn)
                    assert res.converged.all()
                    t[k].append(dt)
                    info[k] = res.info
            line = " | ".join(f"{k} min {min(v) / B:.4f} median {float(np.median(v)) / B:.4f}"
                              for k, v in t.items())
            ratio = {k: float(np.median(t[k])) / float(np.median(t["solve_many"]))
                     for k in ("linear", "lsq")}
            print(f"{name} rows={asm.handle.n_rows} E={mesh.num_edges} B={B} (ms/scenario): "
                  f"{line} | gradient / solve_many (medians): linear {ratio['linear']:.2f}x, lsq "
                  f"{ratio['lsq']:.2f}x | info {info}", flush=True)
        asm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
