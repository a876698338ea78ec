#!/usr/bin/env python3
"""Milliseconds per scenario of ``solve_many`` and ``gradient`` (both objective kinds) for
continuous pressure (2, 1), N = 15, on lattices -- graphs with cycles, the assembler built with
``cycle_direct=True`` -- with ``batch_continuous_cycles`` on (``nx_set_cp_batch_cycles``: the
chord correction per column) and off (what ran before the switch existed:
the per-scenario loop for ``solve_many``; ``gradient`` raises ``NotImplementedError`` there, so
its off column is empty), through the Python call, in one process on one MI355X.

Usage: python scripts/cp_batch_cycles_timing.py [graphs [Bs [pairs]]]
  graphs  comma list of nx x ny lattices, default 19x20,32x32
  Bs      comma list, default 1,8,64
  pairs   alternating (on, off) timed pairs after one warm-up pair, default 5
The one-off build of the batch's capacitance inverse is timed apart: the first batched call
after ``compute_forms`` with a new R, against the R-unchanged call after it. Prints min and
median per call and per scenario, the speed-up of the medians and the launches."""

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

N_OBS = 12


def _timed(fn):
    t0 = time.perf_counter()
    res = fn()
    return 1e3 * (time.perf_counter() - t0), res


def main() -> int:
    graphs = (sys.argv[1] if len(sys.argv) > 1 else "19x20,32x32").split(",")
    Bs = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 8, 64]
    pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    opts = {"ksp_type": "preonly", "pc_type": "lu"}
    os.environ["NXHIP_BATCH"] = "1"  # (also where the single-scenario rule says loop)
    for g in graphs:
        nx_, ny = (int(v) for v in g.split("x"))
        mesh = NetworkMesh(lattice_graph(nx_, ny), N=15)
        asm = HydraulicNetworkAssembler(mesh, flux_degree=2, pressure_degree=1,
                                        cycle_direct=True)
        E = mesh.num_edges
        R = 0.5 + (np.arange(E) % 3) / 2.0
        asm.compute_forms(p_bc_ex=lambda x: x[1], R=R)
        on = Solver(asm, petsc_options=opts, batch_continuous=True,
                    batch_continuous_cycles=True)
        off = Solver(asm, petsc_options=opts, batch_continuous=True,
                     batch_continuous_cycles=False)
        on.assemble()
        on.solve()
        h = asm.handle
        rng = np.random.default_rng(0)
        rows = rng.choice(h.n_rows, size=N_OBS, replace=False)
        w = 0.5 + rng.random(N_OBS)
        name = f"lattice{nx_}x{ny} N=15 (2,1) rows={h.n_rows} E={E}"
        # the one-off build: the first batched call after a new R against the call after it
        pb1 = rng.standard_normal((1, mesh.num_nodes))
        on.solve_many(pb1, np.zeros(1))
        build = []
        for i in range(3):
            asm.compute_forms(p_bc_ex=lambda x: x[1], R=R * (1.0 + 0.01 * (i + 1)))
            off.solve_many(pb1, np.zeros(1))  # (the assembly and the single solve's own build)
            b0 = h.cp_batch_cycles_info()["builds"]
            t_first, r1 = _timed(lambda: on.solve_many(pb1, np.zeros(1)))
            t_next, r2 = _timed(lambda: on.solve_many(pb1, np.zeros(1)))
            assert h.cp_batch_cycles_info()["builds"] == b0 + 1
            assert r1.path == r2.path == "batched"
            build.append((t_first, t_next, r1.info["launches"], r2.info["launches"]))
        print(f"{name}: the build (B = 1, first call after a new R | the call after it, ms; "
              "launches): " + "; ".join(f"{a:.2f} | {b:.2f} ({la} | {lb})"
                                        for a, b, la, lb in build), flush=True)
        asm.compute_forms(p_bc_ex=lambda x: x[1], R=R)
        for B in Bs:
            pbc = rng.standard_normal((B, mesh.num_nodes))
            f = 0.1 * rng.standard_normal(B)
            data = rng.standard_normal((B, N_OBS))
            calls = {
                "solve_many": lambda s: s.solve_many(pbc, f),
                "linear": lambda s: s.gradient(pbc, f, rows=rows, weights=w),
                "lsq": lambda s: s.gradient(pbc, f, rows=rows, weights=w, data=data),
            }
            for key, fn in calls.items():
                t = {"on": [], "off": []}
                info = {}
                for i in range(pairs + 1):  # (the first pair warms up)
                    for tag, s in (("on", on), ("off", off)):
                        if tag == "off" and key != "solve_many":
                            continue  # (NotImplementedError: nothing to time)
                        dt, res = _timed(lambda: fn(s))
                        assert res.converged.all()
                        if key == "solve_many":
                            assert res.path == ("batched" if tag == "on" else "sequential")
                        info[tag] = res.info
                        if i > 0:
                            t[tag].append(dt)
                line = f"{name} B={B} {key}:"
                for tag in ("on", "off"):
                    if t[tag]:
                        line += (f" {tag} min {min(t[tag]) / B:.4f} median "
                                 f"{np.median(t[tag]) / B:.4f} ms/scenario |")
                if t["off"]:
                    line += f" off / on {np.median(t['off']) / np.median(t['on']):.2f}x |"
                line += (f" launches {info['on']['launches']} chunk {info['on']['chunk']} "
                         f"refined {info['on']['refined']} fallback {info['on']['fallback']}")
                print(line, flush=True)
        print(f"{name}: slots builds {h.cp_batch_cycles_info()}", flush=True)
        asm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
