#!/usr/bin/env python3
"""Milliseconds per scenario of ``Solver.solve_ensemble`` (``nx_ensemble_solve``: a resistance
field per scenario, a matrix per column) against the sequential loop in the same process
(``NXHIP_BATCH=0``: the scenario's coefficients with its R, assembly, solve and gather -- what a
caller had before; both write into the same page-locked buffer), and of
``Solver.gradient(R=...)`` with and without derivatives, at B = 1, 8, 64 on one MI355X
(development / DESIGN numbers).

Usage: python scripts/ensemble_timing.py [graphs [Bs [rounds]]]
  graphs  comma list of tree9 (make_tree(9,9,9), N = 15), c3 (make_tree(15,15,15), N = 15);
          default both
  Bs      comma list, default 1,8,64
  rounds  alternating timed rounds (batched, sequential, gradient, objective) after 2 warm-up
          rounds, default 5
Prints min and median per call, per scenario, and the batched pass's launches."""

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


def _timed(fn):
    t0 = time.perf_counter()
    res = fn()
    return 1e3 * (time.perf_counter() - t0), res


def _solve(solver, R, pbc, batched: bool):
    os.environ["NXHIP_BATCH"] = "1" if batched else "0"
    dt, res = _timed(lambda: solver.solve_ensemble(R, pbc))
    os.environ.pop("NXHIP_BATCH", None)
    assert res.path == ("batched" if batched else "sequential"), res.path
    assert res.converged.all()
    return dt, res


def main() -> int:
    names = sys.argv[1].split(",") if len(sys.argv) > 1 else list(GRAPHS)
    Bs = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 8, 64]
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    for name in names:
        make, N, strategy = GRAPHS[name]
        mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
        asm = HydraulicNetworkAssembler(mesh)
        E = mesh.num_edges
        asm.compute_forms(p_bc_ex=lambda x: x[1], R=0.5 + (np.arange(E) % 3) / 2.0)
        solver = Solver(asm, petsc_options={"ksp_type": "preonly", "pc_type": "lu"})
        solver.assemble()
        solver.solve()
        n = asm.handle.n_rows
        rng = np.random.default_rng(0)
        rows = rng.choice(n, size=12, replace=False)
        for B in Bs:
            R = 10.0 ** rng.uniform(-1.0, 1.0, size=(B, E))
            pbc = rng.standard_normal((B, mesh.num_nodes))
            data = rng.standard_normal((B, rows.size))
            calls = {
                "batched": lambda: _solve(solver, R, pbc, True),
                "sequential": lambda: _solve(solver, R, pbc, False),
                "gradient": lambda: _timed(lambda: solver.gradient(pbc, rows=rows, data=data,
                                                                   R=R)),
                "objective": lambda: _timed(lambda: solver.gradient(
                    pbc, rows=rows, data=data, R=R, derivatives=False)),
            }
            for _ in range(2):  # warm-up rounds (workspace, pinned output, first launches)
                for fn in calls.values():
                    fn()
            t = {k: [] for k in calls}
            info, err = {}, 0.0
            for _ in range(rounds):
                out = {}
                for k, fn in calls.items():
                    dt, out[k] = fn()
                    t[k].append(dt)
                    info[k] = out[k].info
                xb, xs = out["batched"].x, out["sequential"].x
                err = max(err, float(np.abs(xb - xs).max() / np.abs(xs).max()))
                del out, xb, xs  # (the page-locked buffers go back to their pool)
            fig = " | ".join(f"{k} min {min(v) / B:.4f} median {float(np.median(v)) / B:.4f}"
                             for k, v in t.items())
            print(f"{name} rows={n} B={B} (ms/scenario): {fig} | speed-up batched vs sequential "
                  f"(medians) {float(np.median(t['sequential'])) / float(np.median(t['batched'])):.2f}x"
                  f" | launches batched {info['batched']['launches']} gradient "
                  f"{info['gradient']['launches']} objective {info['objective']['launches']} "
                  f"chunk {info['batched']['chunk']} refined {info['batched']['refined']} | "
                  f"max |x_b - x_s| / max |x_s| {err:.1e}", flush=True)
        asm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
