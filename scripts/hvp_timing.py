#!/usr/bin/env python3
"""Milliseconds per scenario of ``Solver.hessian_vector`` (``nx_batch_hvp``: four batched direct
solves, ``8 E + 1`` doubles per scenario to the host) against what a user had before it, on the
same scenarios and the same direction, least-squares objective, at B = 1, 8, 64 on one MI355X
(development / DESIGN numbers):

* on a forest the central difference of two ``gradient(R = R +- eps v)`` calls
  (``nx_ensemble_gradient``), which gives the ``v_R`` column of ``H v`` to about half the digits;
* on a graph with cycles (no ensembles there) two rounds of ``compute_forms(R +- eps v)`` +
  ``gradient`` on the B scenarios: each round assembles and rebuilds the cycle correction.

Also timed: one ``gradient`` call, the Gauss-Newton product, and ``Handle.batch_hvp`` alone (the
C call through its ctypes binding with the coefficient arrays prepared: no host normalisation,
no output gathers).

Usage: python scripts/hvp_timing.py [graphs [Bs [pairs [calls]]]]
  graphs  comma list of tree9 (make_tree(9,9,9), N = 15), c3 (make_tree(15,15,15), N = 15),
          lattice (lattice19x20, N = 2); default all three
  Bs      comma list, default 1,8,64
  pairs   alternating timed rounds over the calls after 2 warm-up rounds, default 5
  calls   comma list out of hvp, hvp_gn, hvp_c, gradient, yardstick; default all (a profiler run
          takes one kind at a time)
Prints min and median per call kind, per scenario, and the calls' launches. For kernel times
run it under ``rocprofv3 --kernel-trace --stats`` (a run of its own, not a timed one)."""

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
from networks_fenicsx_amd import network_generation as ng  # noqa: E402

GRAPHS = {
    "tree9": (lambda: ng.make_tree(9, 9, 9), 15, "smallest_last", True),
    "c3": (lambda: ng.make_tree(15, 15, 15), 15, "smallest_last", True),
    "lattice": (lambda: lattice_graph(19, 20), 2, None, False),
}
N_OBS = 12
EPS = 1e-5
ALL_CALLS = ("hvp", "hvp_gn", "hvp_c", "gradient", "yardstick")


def _timed(fn):
    t0 = time.perf_counter()
    res = fn()
    return 1e3 * (time.perf_counter() - t0), res


def main() -> int:
    names = sys.argv[1].split(",") if len(sys.argv) > 1 else list(GRAPHS)
    Bs = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 8, 64]
    pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    kinds = sys.argv[4].split(",") if len(sys.argv) > 4 else list(ALL_CALLS)
    for name in names:
        make, N, strategy, forest = GRAPHS[name]
        mesh = NetworkMesh(make(), N=N, color_strategy=strategy)
        asm = HydraulicNetworkAssembler(mesh)
        E = mesh.num_edges
        R0 = 0.5 + (np.arange(E) % 3) / 2.0

        def p_y(x):
            return x[1]

        asm.compute_forms(p_bc_ex=p_y, R=R0)
        solver = Solver(asm, petsc_options={"ksp_type": "preonly", "pc_type": "lu"})
        solver.assemble()
        solver.solve()
        h = asm.handle
        rng = np.random.default_rng(0)
        rows = rng.choice(h.n_rows, size=N_OBS, replace=False)
        w = 0.5 + rng.random(N_OBS)
        kw = dict(rows=rows, weights=w)
        for B in Bs:
            pbc = rng.standard_normal((B, mesh.num_nodes))
            f = 0.1 * rng.standard_normal(B)
            data = rng.standard_normal((B, N_OBS))
            v_R = rng.standard_normal((B, E))
            v_f = rng.standard_normal((B, E))
            v_p = rng.standard_normal((B, mesh.num_nodes))
            d = dict(v_R=v_R, v_p_bc=v_p, v_f=v_f)
            # the C call's inputs, prepared once
            edge_bc, edge_f, f_const = asm.scenario_coefficients(pbc, f)
            dir_R, dir_bc, dir_f = asm.hvp_directions(B, **d)
            dev_rows = asm.block_order_rows()[rows]

            def central_difference():
                if forest:  # two ensemble gradients at R +- eps v
                    gp = solver.gradient(pbc, f, data=data, R=R0 + EPS * v_R, **kw)
                    gm = solver.gradient(pbc, f, data=data, R=R0 - EPS * v_R, **kw)
                    return gp, (gp.dR - gm.dR) / (2 * EPS)
                # cycles: the direction of scenario 0 for all (one R per compute_forms)
                out = []
                for sgn in (1.0, -1.0):
                    asm.compute_forms(p_bc_ex=p_y, R=R0 + sgn * EPS * v_R[0])
                    out.append(solver.gradient(pbc, f, data=data, **kw))
                return out[0], (out[0].dR - out[1].dR) / (2 * EPS)

            calls = {
                "hvp": lambda: solver.hessian_vector(pbc, f, data=data, **kw, **d),
                "hvp_gn": lambda: solver.hessian_vector(pbc, f, data=data, gauss_newton=True,
                                                        **kw, **d),
                "hvp_c": lambda: h.batch_hvp(edge_bc, edge_f, f_const, solver.rtol,
                                             rows=dev_rows, weights=w, data=data, dir_R=dir_R,
                                             dir_bc=dir_bc, dir_f=dir_f),
                "gradient": lambda: solver.gradient(pbc, f, data=data, **kw),
                "yardstick": central_difference,
            }
            calls = {k: calls[k] for k in ALL_CALLS if k in kinds}
            if not forest and "yardstick" in calls:
                # the yardstick leaves another R resident: every round starts from R0 again
                def reset():
                    asm.compute_forms(p_bc_ex=p_y, R=R0)
                    solver.gradient(pbc, f, data=data, **kw)
            else:
                def reset():
                    return None
            for _ in range(2):  # warm-up rounds (workspace, pinned output, first launches)
                for fn in calls.values():
                    fn()
                reset()
            t = {k: [] for k in calls}
            info = {}
            for _ in range(pairs):
                for k, fn in calls.items():
                    dt, res = _timed(fn)
                    t[k].append(dt)
                    if k == "yardstick":
                        reset()
                    elif k != "hvp_c":
                        assert res.converged.all()
                        info[k] = res.info["launches"]
            line = " | ".join(f"{k} min {min(v) / B:.4f} median {float(np.median(v)) / B:.4f}"
                              for k, v in t.items())
            med = {k: float(np.median(v)) for k, v in t.items()}
            ratios = []
            if "hvp" in med and "gradient" in med:
                ratios.append(f"hvp / gradient {med['hvp'] / med['gradient']:.2f}x")
            if "hvp" in med and "yardstick" in med:
                ratios.append(f"yardstick / hvp {med['yardstick'] / med['hvp']:.2f}x")
            print(f"{name} rows={h.n_rows} E={E} B={B} (ms/scenario): {line} | "
                  f"{', '.join(ratios)} (medians) | launches {info}", flush=True)
        asm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
