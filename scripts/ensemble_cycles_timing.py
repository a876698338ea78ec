#!/usr/bin/env python3
"""Milliseconds per scenario of ``Solver.solve_ensemble`` and ``Solver.gradient(R=...)`` on graphs
with cycles with ``ensemble_cycles=True`` (a cycle correction per scenario: ``2 n_cyc`` batched
unit solves and one factorisation each) against the sequential loop in the same process -- the
path the same call takes with the flag off: the scenario's coefficients with its R, assembly, the
handle's cycle correction rebuilt, solve, gather -- at B = 1, 8, 64 on one MI355X (development /
DESIGN numbers; sibling of scripts/ensemble_timing.py, which covers forests).

Usage: python scripts/ensemble_cycles_timing.py [graphs [Bs [rounds]]]
  graphs  comma list of lat19x20 (lattice 19 x 20, N = 2: 342 cycle chains, 3,995 rows),
          lat16x17 (lattice 16 x 17, N = 15: 240 cycle chains, 16 k rows), lat23x24 (lattice
          23 x 24, N = 2: 506 cycle chains, near the cap of 512); default all
  Bs      comma list, default 1,8,64
  rounds  alternating timed rounds (batched, sequential, gradient, objective) after 2 warm-up
          rounds, default 5
Prints min and median per call, per scenario, and the batched pass's launches. For the kernel
times of k_e_cyc_factor run it under ``rocprofv3 --kernel-trace --stats`` (a run of its own, not
a timed one)."""

from __future__ import annotations

import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

from cases import lattice_graph  # noqa: E402
from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh, Solver  # noqa: E402

GRAPHS = {
    "lat19x20": (lambda: lattice_graph(19, 20), 2),
    "lat16x17": (lambda: lattice_graph(16, 17), 15),
    "lat23x24": (lambda: lattice_graph(23, 24), 2),
}


def _timed(fn):
    t0 = time.perf_counter()
    res = fn()
    return 1e3 * (time.perf_counter() - t0), res


def _solve(solver, R, pbc, path):
    dt, res = _timed(lambda: solver.solve_ensemble(R, pbc))
    assert res.path == path, res.path
    assert res.converged.all()
    return dt, res


def main() -> int:
    names = sys.argv[1].split(",") if len(sys.argv) > 1 else list(GRAPHS)
    Bs = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 8, 64]
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    for name in names:
        make, N = GRAPHS[name]
        mesh = NetworkMesh(make(), N=N)
        asm = HydraulicNetworkAssembler(mesh)
        E = mesh.num_edges
        n_cyc = E - mesh.num_nodes + 1
        asm.compute_forms(p_bc_ex=lambda x: x[1], R=0.5 + (np.arange(E) % 3) / 2.0)
        opts = {"ksp_type": "preonly", "pc_type": "lu"}
        on = Solver(asm, petsc_options=opts, ensemble_cycles=True)
        off = Solver(asm, petsc_options=opts, ensemble_cycles=False)
        on.assemble()
        on.solve()
        n = asm.handle.n_rows
        if not asm.handle.ensemble_supported():  # (the direct solve's caps, or n_cyc above 512)
            print(f"{name} rows={n} n_cyc={n_cyc}: the batched ensemble does not apply", flush=True)
            asm.close()
            continue
        rng = np.random.default_rng(0)
        rows = rng.choice(n, size=12, replace=False)
        for B in Bs:
            R = 10.0 ** rng.uniform(-1.0, 1.0, size=(B, E))
            pbc = rng.standard_normal((B, mesh.num_nodes))
            data = rng.standard_normal((B, rows.size))
            calls = {
                "batched": lambda: _solve(on, R, pbc, "batched"),
                "sequential": lambda: _solve(off, R, pbc, "sequential"),
                "gradient": lambda: _timed(lambda: on.gradient(pbc, rows=rows, data=data, R=R)),
                "objective": lambda: _timed(lambda: on.gradient(
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
            print(f"{name} rows={n} n_cyc={n_cyc} B={B} (ms/scenario): {fig} | speed-up batched "
                  f"vs sequential (medians) "
                  f"{float(np.median(t['sequential'])) / float(np.median(t['batched'])):.2f}x"
                  f" | launches batched {info['batched']['launches']} gradient "
                  f"{info['gradient']['launches']} objective {info['objective']['launches']} "
                  f"chunk {info['batched']['chunk']} refined {info['batched']['refined']} "
                  f"storage {asm.handle.ensemble_cycles_info()['storage']} | "
                  f"max |x_b - x_s| / max |x_s| {err:.1e}", flush=True)
        asm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
