"""Ranks that do not look alike: every rank of a group with its own decomposition
(``target_jobs`` per rank), so that the one-launch step cases of the exchange step run beside
each other -- a rank whose job needs several chain passes next to ranks whose jobs fit one, a
rank of one job without job slots between ranks of 40 jobs, a rank that takes the
superposition instantiation next to one that cannot (tests/test_unlike_ranks.py asserts the
facts on the host, tests/test_gpu_unlike_ranks.py runs the device).

Graphs: ``make_tree(9, 9, 9)`` (511 edges) and ``make_tree(8, 8, 8)`` (255 edges), coloured
``smallest_last``. Coefficients: a seeded per-edge R = 10^U(-1, 1), f = 0.1 + 0.02 (e mod 5),
p_bc = x[1] + 0.3 x[0] -- the multi-rank tests have had R = 1, f = 0 almost everywhere."""

from __future__ import annotations

import functools

import numpy as np

from networks_fenicsx_amd import NetworkMesh
from networks_fenicsx_amd import network_generation as ng
from networks_fenicsx_amd.layout import build_local_problem
from networks_fenicsx_amd.precond import build_tree_preconditioner
from oracle import nx_oracle as O
from tree_shapes import p_xy

STRATEGY = "smallest_last"
GRAPHS = {"T9": lambda: ng.make_tree(9, 9, 9), "T8": lambda: ng.make_tree(8, 8, 8)}
EDGES = {"T9": 511, "T8": 255}

# csrc/nxhip.hip: kPcThreads; kCapC, kCapS (chains and slots of a job in LDS), kMaxNeed (top
# values a job needs); kCapT (top slots)
K_PC_THREADS, CAP_C, CAP_S, K_MAX_NEED, CAP_T = 1024, 512, 256, 128, 1152

# id -> (graph, N, target_jobs per rank, most chains of a job per rank)
#   U1  rank 0 asks for superposition, rank 1 needs two chain passes
#   U2  the same pair the other way round (the plain kernel was always launched: control)
#   U3  the middle rank is one job with no job slots, 90 top slots and 90 needed top values,
#       between ranks of 42 and 43 jobs
#   U4  exactly one pass (G = 128 chains) on rank 0, one chain under it on rank 1:
#       superposition on both
#   U5  every rank has several passes
#   U6  <8, 3>, no superposition instantiation; mixed passes in one launch
CONFIGS = {
    "U1": ("T9", 15, (256, 1), (4, 255)),
    "U2": ("T9", 15, (1, 256), (256, 4)),
    "U3": ("T9", 4, (256, 1, 256), (5, 170, 4)),
    "U4": ("T8", 15, (1, 1), (128, 127)),
    "U5": ("T9", 15, (1, 1), (256, 255)),
    "U6": ("T9", 19, (256, 1), (4, 255)),
}
# whether the group's one launch takes the superposition instantiation (every rank or none),
# and what every rank's own launch takes
GROUP_SUP = {"U1": False, "U2": False, "U3": False, "U4": True, "U5": False, "U6": False}
RANK_SUP = {"U1": (True, False), "U2": (False, True), "U3": (True, False, True),
            "U4": (True, True), "U5": (False, False), "U6": (False, False)}


def lane_shape(N: int) -> tuple[int, int]:
    """(W, CPL) of the one-launch / exchange step at N <= 64 cells per edge (csrc/nxhip.hip,
    step_lane_of; tests/test_gpu_lane_shapes.py compares it with ``Handle.lane_shapes``)."""
    return (8, 2) if N <= 16 else (8, 3) if N <= 24 else (8, 4) if N <= 32 else (16, 4)


def pass_chains(N: int) -> int:
    """G: the chains of one pass of a 1024-thread workgroup."""
    return K_PC_THREADS // lane_shape(N)[0]


def coefficients(graph: str) -> dict:
    E = EDGES[graph]
    R = 10.0 ** np.random.default_rng(E + 17).uniform(-1.0, 1.0, E)
    return {"R": R, "f": 0.1 + 0.02 * (np.arange(E) % 5)}


@functools.lru_cache(maxsize=None)
def mesh_of(graph: str, N: int):
    G = GRAPHS[graph]()
    return G, NetworkMesh(G, N=N, color_strategy=STRATEGY)


@functools.lru_cache(maxsize=None)
def oracle(graph: str, N: int) -> dict:
    """The references of (graph, N), computed once and read-only: the oracle's system in build
    layout with the general coefficients, its LU solution in build layout, and the analytic
    answer of the same R with f = 0."""
    _, mesh = mesh_of(graph, N)
    assert mesh.num_edges == EDGES[graph]
    src, dst = mesh.edges
    P = O.build_problem(mesh.node_coordinates, src, dst, N, mesh.edge_colors)
    coef = coefficients(graph)
    A, b = O.assemble_reference(P, p_xy, **coef)
    Ab, bb, perm, _ = O.to_build_layout(P, A, b)
    out = {"Ab": Ab, "bb": bb, "perm": perm, "coef": coef, "E": mesh.num_edges, "N": N,
           "x": O.solve_reference(A, b)[perm],
           "xa": O.resistor_network_solution(P, p_xy, R=coef["R"])[perm]}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def host_ranks(cid: str):
    """Every rank's local problem and decomposition of a configuration, on the host."""
    graph, N, jobs, _ = CONFIGS[cid]
    _, m = mesh_of(graph, N)
    src, dst = m.edges
    P = len(jobs)
    lps = [build_local_problem(m.node_coordinates, src, dst, m.degrees, N, r, P)
           for r in range(P)]
    pcs = [build_tree_preconditioner(lp, src, dst, m.degrees, target_jobs=j)
           for lp, j in zip(lps, jobs)]
    return lps, pcs


def set_decompositions(grp, target_jobs) -> None:
    """Give rank r of a ``RankGroup`` the decomposition of ``target_jobs[r]`` (with several
    ranks the coarse forest comes from ``lp.edge_owner``), upload them and let the ranks agree
    on their kernels and cycle shares again."""
    assert len(target_jobs) == grp.nranks
    grp._close_group()
    for a, mesh, j in zip(grp.assemblers, grp.meshes, target_jobs):
        src, dst = mesh.edges
        a._pc = build_tree_preconditioner(a._local, src, dst, mesh.degrees, target_jobs=j)
    grp.set_preconditioner(True)
