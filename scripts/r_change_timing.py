#!/usr/bin/env python3
"""Step time when the coefficients are uploaded every step (GPU box): compute_forms + assemble
+ solve on the bench workload (C3 by default) with the SAME per-edge R re-sent each step (the
CSR values in device memory stay current: the dense step's values-free instantiation) and with
a NEW R each step (every step stores the values and rebuilds G). Medians per repeat, so that
the spread between repeats of the same-R figure is the yardstick for the new-R one (DESIGN.md
section 3c, round 8).

    python scripts/r_change_timing.py [levels N steps repeats]
"""

from __future__ import annotations

import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (HIP runtime first)

from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh  # noqa: E402
from networks_fenicsx_amd import network_generation as ng  # noqa: E402


def _p_y(x):
    return x[1]


def main() -> int:
    pos = [int(a) for a in sys.argv[1:]]
    levels, N, steps, repeats = (pos + [15, 15, 50, 5][len(pos):])[:4]
    mesh = NetworkMesh(ng.make_tree(levels, levels, levels), N=N, color_strategy="smallest_last")
    asm = HydraulicNetworkAssembler(mesh)
    h = asm.handle
    E = mesh.num_edges
    R0 = 1.0 + 0.125 * (np.arange(E) % 5)
    Rs = [R0 * (1.0 + 0.001 * (k + 1)) for k in range(8)]  # (rotated: each differs from the last)
    asm.compute_forms(p_bc_ex=_p_y, R=R0)
    asm.set_direct(True)

    def step(R):
        asm.compute_forms(p_bc_ex=_p_y, R=R)
        asm.assemble()
        it, rr, conv = h.solve(1e-12, 100, 4)
        assert conv and h.direct_path() == "fused", (it, rr, h.direct_path())

    out = {"same_R": [], "new_R": []}
    k = 0
    for r in range(repeats):
        for name in ("same_R", "new_R"):
            ts = []
            for i in range(steps + 5):
                R = R0 if name == "same_R" else Rs[k % len(Rs)]
                k += 1
                h.sync()
                t0 = time.perf_counter()
                step(R)
                h.sync()
                if i >= 5:
                    ts.append(1e3 * (time.perf_counter() - t0))
            out[name].append(float(np.median(ts)))
            kept = getattr(h, "values_kept", lambda: None)()
            print(f"repeat {r} {name}: median {out[name][-1]:.4f} ms/step "
                  f"(compute_forms + assemble + solve), {kept}", flush=True)
    for name, v in out.items():
        print(f"{name:7s} medians: min {min(v):.4f} med {float(np.median(v)):.4f} "
              f"max {max(v):.4f} ms/step (spread {max(v) - min(v):.4f})", flush=True)
    asm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
