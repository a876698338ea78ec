"""The cases of ``test_gpu_cyc_unify.py`` and the recorder of their golden file (not a test
module).

The Woodbury correction of the cycle chains has one build, one apply
and one kernel set; these cases run every caller of it at the smallest shapes at which each
path can still go wrong:

=========  ==========================================  ==========================================
 case       graph                                       what it runs
=========  ==========================================  ==========================================
 p1_*       ``edge_info_N10``, ``lattice4x5_N6``        first solve, a forced refinement pass
                                                        (rtol = rr / 2), new per-edge R (rebuild):
                                                        the CSR couplings, ``prev`` / ``save``
 p1_wide    ``lattice_graph(12, 13)``, N = 2            132 cycles, m = 264: two workgroups of
                                                        the ``w`` kernel (``blockIdx.x > 0``)
 fe_k2      ``edge_info_N10``, (k, m) = (2, 0)          the couplings by P1 position, the
                                                        auxiliary handle on a borrowed stream
 group_*    ``lattice4x5_N6`` P = 2,                    the team gather, the all-reduced shares,
            ``edge_info_N10`` P = 3                     U^T x read directly (no rows)
 batch      ``lattice4x5_N6``, three columns            the batched launches, first call (builds)
                                                        and second (steady), with their counts
=========  ==========================================  ==========================================

    python tests/cyc_unify_cases.py OUT.npz

records them with whatever build of the package is first on ``sys.path``;
``tests/golden/cyc_unify_parent.npz`` holds the arrays of the commit before the copies were
merged, recorded on an MI355X.
"""

from __future__ import annotations

import sys

import numpy as np

from cases import CYCLIC, lattice_graph, p_x, p_y

CASES = ("p1_edge_info_N10", "p1_lattice4x5_N6", "p1_wide", "fe_k2", "group_lattice4x5_N6_P2",
         "group_edge_info_N10_P3", "batch")
WIDE = (12, 13, 2)  # lattice_graph(12, 13), N = 2: 132 cycle chains, m = 264 > 256


def _graph(name):
    if name == "wide":
        return lattice_graph(*WIDE[:2]), WIDE[2]
    make, N = CYCLIC[name]
    return make(), N


def _p1(name: str, rebuild: bool) -> dict:
    from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh

    G, N = _graph(name)
    mesh = NetworkMesh(G, N=N)
    asm = HydraulicNetworkAssembler(mesh)
    if name == "wide":
        assert np.asarray(asm.tree_preconditioner.cyc_rows).shape == (132, 2)
    asm.compute_forms(p_bc_ex=p_y)
    asm.set_direct(True)
    h = asm.handle
    out = {}

    def solve(tag, rtol):
        asm.assemble()
        it, rr, conv = h.solve(rtol, 100, 4)
        assert h.solver() == (1, 1), (tag, h.solver())
        out[f"{tag}_x"] = h.solution()
        out[f"{tag}_relres"] = np.float64(rr)
        out[f"{tag}_iterations"] = np.int32(it)
        return rr

    rr = solve("first", 1e-12)
    assert rr > 0.0
    solve("refined", rr / 2)  # (a forced refinement pass, as test_direct_solve_with_cycles)
    assert out["refined_iterations"] == 2
    if rebuild:
        R = 1.0 + 0.5 * (np.arange(mesh.num_edges) % 3)
        asm.compute_forms(p_bc_ex=p_y, R=R)
        solve("new_R", 1e-12)
    asm.close()
    return out


def _fe_k2() -> dict:
    from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh, Solver

    G, N = _graph("edge_info_N10")
    mesh = NetworkMesh(G, N=N)
    asm = HydraulicNetworkAssembler(mesh, flux_degree=2, pressure_degree=0)
    R = 1.0 + 0.5 * (np.arange(mesh.num_edges) % 3)
    asm.compute_forms(p_bc_ex=p_y, f=0.2, R=R)
    solver = Solver(asm)
    solver.assemble()
    solver.solve()
    assert solver.ksp.solver_used == "direct" and asm.handle.direct_path() == "condensed"
    out = {"x": asm.handle.solution(),
           "relres": np.float64(solver.ksp.residual_estimate),
           "iterations": np.int32(solver.ksp.iterations)}
    asm.close()
    return out


def _group(name: str, P: int) -> dict:
    from networks_fenicsx_amd.group import RankGroup

    G, N = _graph(name)
    grp = RankGroup(G, N, P)
    out = {}
    try:
        grp.compute_forms(p_bc_ex=p_y)
        grp.set_direct(True)

        def solve(tag, rtol):
            grp.assemble()
            it, rr, conv = grp.solve(rtol, 50000, 4)
            assert grp.solver_used == "direct", (tag, grp.solver_used)
            for r, x in enumerate(grp.solutions()):
                out[f"{tag}_x_rank{r}"] = np.array(x, copy=True)
            out[f"{tag}_relres"] = np.float64(rr)
            out[f"{tag}_iterations"] = np.int32(it)
            return rr

        rr = solve("first", 1e-12)
        assert rr > 0.0
        solve("refined", rr / 2)
    finally:
        grp.close()
    return out


def _batch() -> dict:
    from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh, Solver

    G, N = _graph("lattice4x5_N6")
    mesh = NetworkMesh(G, N=N)
    asm = HydraulicNetworkAssembler(mesh)
    E = mesh.num_edges
    asm.compute_forms(p_bc_ex=p_y, R=0.5 + (np.arange(E) % 3) / 2.0)
    rnd = np.random.default_rng(7).standard_normal(mesh.num_nodes)
    items = [p_y, p_x, rnd]
    f = np.zeros((3, E))
    f[1] = 0.1 + 0.02 * (np.arange(E) % 5)
    solver = Solver(asm)
    out = {}
    for tag in ("first", "second"):
        res = solver.solve_many(items, f)
        assert res.path == "batched" and res.info["fallback"] == 0
        out[f"{tag}_X"] = np.array(res.x, copy=True)
        out[f"{tag}_relres"] = np.array(res.residual_norms, copy=True)
        out[f"{tag}_launches"] = np.int32(res.info["launches"])
    asm.close()
    return out


def run_case(case: str) -> dict:
    """name -> array (a reported residual or a count: a 0-d array) of one case."""
    if case == "p1_wide":
        return _p1("wide", rebuild=False)
    if case.startswith("p1_"):
        return _p1(case[3:], rebuild=True)
    if case == "fe_k2":
        return _fe_k2()
    if case.startswith("group_"):
        name, P = case[6:].rsplit("_P", 1)
        return _group(name, int(P))
    assert case == "batch", case
    return _batch()


def run_all() -> dict:
    return {f"{c}/{k}": v for c in CASES for k, v in run_case(c).items()}


if __name__ == "__main__":
    np.savez_compressed(sys.argv[1], **run_all())
    print(f"recorded {sys.argv[1]}")
