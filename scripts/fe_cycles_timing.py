#!/usr/bin/env python3
"""Continuous pressure on graphs with cycles: the node-condensed direct solve with the
chords' correction (cycle_direct=True) against plain MINRES (the switch off: what the same
graph ran before the switch existed), on square-ish lattices (development / DESIGN numbers).

Usage: python scripts/fe_cycles_timing.py [N ["nx,ny;nx,ny.."] ["k,m;k,m.."] [direct]]
("direct": the direct solves only, for profiling passes). Per graph and pair: the first
assemble + solve (it builds the capacitance matrix), the steady assemble + solve with R
unchanged (min / median of 10, after it), one with a new R (rebuilds), then MINRES."""

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


def _timed(h):
    t0 = time.perf_counter()
    h.assemble(True, True)
    it, rr, conv = h.solve(1e-12, 400000, 32)
    h.sync()
    return 1e3 * (time.perf_counter() - t0), it, rr, conv


def main() -> int:
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    graphs = [(19, 20), (45, 45)]
    if len(sys.argv) > 2:
        graphs = [tuple(int(v) for v in g.split(",")) for g in sys.argv[2].split(";")]
    pairs = [(2, 1)]
    if len(sys.argv) > 3:
        pairs = [tuple(int(v) for v in p.split(",")) for p in sys.argv[3].split(";")]
    direct_only = len(sys.argv) > 4 and sys.argv[4] == "direct"
    pbc = lambda x: x[1]  # noqa: E731
    for nx_, ny in graphs:
        mesh = NetworkMesh(lattice_graph(nx_, ny), N=N)
        E = mesh.num_edges
        R = 1.0 + 0.5 * (np.arange(E) % 3)
        for km in pairs:
            asm = HydraulicNetworkAssembler(mesh, flux_degree=km[0], pressure_degree=km[1],
                                            cycle_direct=True)
            tab = asm._fe_cp
            name = f"lattice{nx_}x{ny} N={N} k={km[0]} m={km[1]}"
            if tab is None:
                print(f"{name}: no direct solve (past the cap)", flush=True)
                asm.close()
                continue
            h = asm.handle
            asm.compute_forms(p_bc_ex=pbc, f=0.3, R=R)
            asm.set_direct(True)
            first, it, rr, conv = _timed(h)
            ts = [_timed(h)[0] for _ in range(10)]
            b0 = h.cp_cycles()["builds"]
            asm.compute_forms(p_bc_ex=lambda x: x[0], f=0.1, R=R)  # new values, R unchanged
            same_r = _timed(h)[0]
            b1 = h.cp_cycles()["builds"]
            asm.compute_forms(p_bc_ex=pbc, f=0.3, R=R[::-1].copy())
            new_r = _timed(h)[0]
            print(f"{name} rows={h.n_rows} chords={np.asarray(tab.chord).size} "
                  f"slots={np.asarray(tab.cslot).size // 2} direct used={h.solver()[1]} "
                  f"path={h.direct_path()} passes={it} relres={rr:.2e} conv={conv}: first "
                  f"{first:.3f} ms (builds the capacitance matrix), steady min {min(ts):.3f} "
                  f"median {float(np.median(ts)):.3f} ms, new bc/f same R {same_r:.3f} ms "
                  f"(builds {b0} -> {b1}), new R {new_r:.3f} ms "
                  f"(builds -> {h.cp_cycles()['builds']})", flush=True)
            asm.close()
            if direct_only:
                continue
            asm = HydraulicNetworkAssembler(mesh, flux_degree=km[0], pressure_degree=km[1],
                                            cycle_direct=False)
            h = asm.handle
            asm.compute_forms(p_bc_ex=pbc, f=0.3, R=R)
            _timed(h)  # warm
            tm = [_timed(h) for _ in range(2)]
            print(f"{name} plain MINRES (switch off) it={tm[-1][1]} relres={tm[-1][2]:.2e} "
                  f"conv={tm[-1][3]}: {min(t[0] for t in tm):.2f} ms", flush=True)
            asm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
