#!/usr/bin/env python3
"""Milliseconds of the direct solve on a graph with cycles, one rank,
P1 / DG0, on one MI355X: the first solve after a new matrix, which builds the Woodbury
correction (one tree solve per column of Z, the capacitance matrix and its inversion) and then
solves, and a steady solve, which applies it.

Usage: python scripts/cyc_timing.py [graph [rounds [steady]]]
  graph   lattice (lattice19x20, N = 2: 342 cycle chains, 684 columns; default) or small
          (lattice4x5, N = 6)
  rounds  timed builds after one warm-up round, each with another per-edge R; default 5
  steady  timed steady solves per round, default 20
Prints min and median of both. To compare two builds run it once per build in turn
(``NXHIP_LIB=/path/to/libnxhip.so`` picks the library), several pairs."""

from __future__ import annotations

import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

from cases import lattice_graph  # noqa: E402
from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh  # noqa: E402

GRAPHS = {"lattice": (lambda: lattice_graph(19, 20), 2), "small": (lambda: lattice_graph(4, 5), 6)}


def main() -> int:
    name = sys.argv[1] if len(sys.argv) > 1 else "lattice"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    steady = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    make, N = GRAPHS[name]
    mesh = NetworkMesh(make(), N=N)
    asm = HydraulicNetworkAssembler(mesh)

    def p_y(x):
        return x[1]

    h = asm.handle
    first, later = [], []
    for r in range(rounds + 1):  # (round 0: warm-up -- workspace, first launches)
        asm.compute_forms(p_bc_ex=p_y, R=1.0 + 0.25 * ((np.arange(mesh.num_edges) + r) % 3))
        asm.set_direct(True)
        asm.assemble()
        t0 = time.perf_counter()
        it, rr, conv = h.solve(1e-12, 100, 4)
        dt = 1e3 * (time.perf_counter() - t0)
        assert conv and h.solver() == (1, 1), (it, rr)
        ts = []
        for _ in range(steady):
            asm.assemble()
            t0 = time.perf_counter()
            h.solve(1e-12, 100, 4)
            ts.append(1e3 * (time.perf_counter() - t0))
        if r:
            first.append(dt)
            later += ts
    m = 2 * np.asarray(asm.tree_preconditioner.cyc_rows).shape[0]
    print(f"{name} rows={h.n_rows} m={m} (ms): first solve (build + solve) min {min(first):.3f} "
          f"median {float(np.median(first)):.3f} max {max(first):.3f} | steady solve min "
          f"{min(later):.4f} median {float(np.median(later)):.4f}", flush=True)
    asm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
