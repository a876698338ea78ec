"""Forests that are not binary: hubs (many junction children below one junction), brooms (many
leaf edges at one junction), caterpillars (a long spine with side edges), hubs of hubs and
random recursive trees with hubs -- the shapes at which the tree solve leaves its binary-tree
paths (tests/test_tree_shapes.py, tests/test_gpu_tree_shapes.py).

Besides the generators: ``decomposition_facts`` (what a decomposition holds, from its host
arrays) and the per-block error measure ``block_errors`` (flux / pressure / multiplier blocks
separately: on these graphs the pressures carry the 2-norm of x, and one norm over the whole
vector lets a flux error four digits above the bar pass)."""

from __future__ import annotations

from collections import deque

import networkx as nx
import numpy as np

# csrc/nxhip.hip: kWaveKids (junction children per slot of the one-wave / register sweeps),
# kPre (down-chain entries of a slot prefetched in phase A), kCapLvl (job levels staged in
# LDS; the one-wave sweeps also need <= 64 slots), kMaxTopLvl (top levels of the LDS kernels)
K_WAVE_KIDS, K_PRE, K_CAP_LVL, K_WAVE_SLOTS, K_MAX_TOP_LVL = 4, 4, 64, 64, 255
# csrc/nxhip.hip: kCpRecInc, kCpRecCh -- the incident edges and the children that a node record
# of the continuous-pressure direct solve holds; a node past either walks the lists
# (``r[3] = -1`` / ``r[kc] = -1``), its level gets ``cp_lev_full = 0``
K_CP_REC_INC, K_CP_REC_CH = 4, 3


def p_xy(x):
    return x[1] + 0.3 * x[0]


def _place(n_nodes: int, edges) -> nx.DiGraph:
    """Positions from the breadth-first depth (from node 0, edges taken undirected): the k-th
    node (by id) of depth d at (0.37 k + 0.11 d, d + 0.05 k, 0.013 v) -- no two nodes coincide,
    no edge has zero length, and ``p_xy`` differs between any two boundary nodes."""
    adj = [[] for _ in range(n_nodes)]
    for a, b in edges:
        adj[a].append(b)
        adj[b].append(a)
    depth = [-1] * n_nodes
    depth[0] = 0
    q = deque([0])
    while q:
        u = q.popleft()
        for w in adj[u]:
            if depth[w] < 0:
                depth[w] = depth[u] + 1
                q.append(w)
    assert min(depth) >= 0, "connected"
    G = nx.DiGraph()
    seen: dict[int, int] = {}
    for v in range(n_nodes):
        d = depth[v]
        k = seen.get(d, 0)
        seen[d] = k + 1
        G.add_node(v, pos=np.array([0.37 * k + 0.11 * d, float(d) + 0.05 * k, 0.013 * v]))
    for a, b in edges:
        G.add_edge(a, b)
    return G


def hub(k: int, grand: int = 2, inward: bool = False) -> nx.DiGraph:
    """Inlet edge 0 -> 1, k edges 1 -> m_i, ``grand`` leaf edges from every m_i: junction 1
    has k junction children (m_i and its leaves are numbered together). ``inward``: the last
    leaf edge of every m_i points into it -- the edge partition (chunks of the directed
    depth-first order) then hands those edges to the last rank, so most m_i have edges of two
    ranks (tests/test_gpu_tree_shapes.py, several ranks)."""
    edges = [(0, 1)]
    nxt = 2
    for _ in range(k):
        m = nxt
        nxt += 1
        edges.append((1, m))
        for g in range(grand):
            edges.append((nxt, m) if inward and g == grand - 1 else (m, nxt))
            nxt += 1
    return _place(nxt, edges)


def broom(k: int) -> nx.DiGraph:
    """Edge 0 -> 1 and k leaf edges from node 1: one junction, no junction child, k + 1
    chains at it."""
    return _place(k + 2, [(0, 1)] + [(1, 2 + i) for i in range(k)])


def caterpillar(L: int) -> nx.DiGraph:
    """A spine of L edges 0 -> 1 -> ... -> L with one side edge at every interior spine node;
    every third side edge points INTO the spine (its chain is flipped)."""
    edges = [(i, i + 1) for i in range(L)]
    for i in range(1, L):
        s = L + i
        edges.append((s, i) if i % 3 == 0 else (i, s))
    return _place(2 * L, edges)


def hubhub(k1: int, k2: int) -> nx.DiGraph:
    """A hub of k1 hubs of k2 junctions; each of those has one outgoing and one incoming leaf
    edge."""
    edges = [(0, 1)]
    nxt = 2
    mids = []
    for _ in range(k1):
        edges.append((1, nxt))
        mids.append(nxt)
        nxt += 1
    js = []
    for m in mids:
        for _ in range(k2):
            edges.append((m, nxt))
            js.append(nxt)
            nxt += 1
    for j in js:
        edges.append((j, nxt))
        edges.append((nxt + 1, j))
        nxt += 2
    return _place(nxt, edges)


def random_tree(n: int, seed: int) -> nx.DiGraph:
    """Node v attaches to a uniformly random earlier node with probability 0.6, else to one of
    the first v // 8 nodes (hubs); the edge is reversed with probability 0.3."""
    rng = np.random.default_rng(seed)
    edges = []
    for v in range(1, n):
        if rng.random() < 0.6:
            u = int(rng.integers(0, v))
        else:
            u = int(rng.integers(0, max(1, v // 8)))
        edges.append((v, u) if rng.random() < 0.3 else (u, v))
    return _place(n, edges)


# name -> (graph factory, N, per-edge random R and f (the general coefficients))
SHAPES = {
    "hub3": (lambda: hub(3), 4, False),
    "hub4": (lambda: hub(4), 5, False),
    "hub5": (lambda: hub(5), 3, False),
    "hub9": (lambda: hub(9), 8, True),
    "hub70": (lambda: hub(70, grand=1), 2, False),
    "broom5": (lambda: broom(5), 6, False),
    "broom33": (lambda: broom(33), 3, False),
    "cat70": (lambda: caterpillar(70), 3, False),
    "cat300": (lambda: caterpillar(300), 2, False),
    "hubhub5x5": (lambda: hubhub(5, 5), 4, True),
    "rand200_s1": (lambda: random_tree(200, 1), 5, True),
    "rand200_s2": (lambda: random_tree(200, 2), 17, True),
    "rand600_s3": (lambda: random_tree(600, 3), 2, True),
}
JOBS = (1, 4, 256)  # target_jobs; 256 is build_tree_preconditioner's default


def seeded_coefficients(seed: int, E: int) -> dict:
    """A seeded per-edge R = 10^U(-1, 1) (two decades) with f = 0.1 + 0.02 (e mod 5)."""
    R = 10.0 ** np.random.default_rng(seed).uniform(-1.0, 1.0, E)
    return {"R": R, "f": 0.1 + 0.02 * (np.arange(E) % 5)}


def coefficients(name: str, E: int) -> dict:
    """The forms' coefficients of a shape: nothing (R = 1, f = 0), or a seeded per-edge
    R = 10^U(-1, 1) with f = 0.1 + 0.02 (e mod 5)."""
    if not SHAPES[name][2]:
        return {}
    return seeded_coefficients(sorted(SHAPES).index(name) + 11, E)


# The degree-k gradients (tests/test_gradient_ref_fe.py, tests/test_gradient_ref_cp.py: the CPU
# adjoint against finite differences; at most 16 edges): name -> (graph factory, N, seeded R).
# hub(5)'s hub is past both record caps of the continuous-pressure node forest, broom(5)'s
# junction too; caterpillar(7) has side edges pointing INTO the spine at i = 3, 6 and
# hubhub(2, 2) four incoming leaf edges, so both have boundary nodes that are an edge's source.
FD_SHAPES = {
    "hub5_N3": (lambda: hub(5), 3, False),
    "broom5_N2": (lambda: broom(5), 2, False),
    "cat7_N2": (lambda: caterpillar(7), 2, False),
    "hubhub2x2_N2": (lambda: hubhub(2, 2), 2, True),
}
# the forests the degree-k batched paths are held on (tests/test_gpu_fe_shapes.py, and the host
# models before them: tests/test_fe_gradient_host.py, tests/test_cp_gradient_host.py)
FE_GRADIENT_SHAPES = ["hub3", "hub5", "hub70", "broom33", "cat70", "hubhub5x5", "rand200_s1"]
FE_N_CAP = 6  # cells per edge at general degrees (tests/test_gpu_tree_shapes.py, _fe_open)


def fd_shape(name: str):
    """``(graph, N, R (E,), f (E,))`` of an ``FD_SHAPES`` entry: the gradient tests' R = 0.5 +
    (e mod 3) / 2, or the seeded two-decade R; f = 0.1 + 0.02 (e mod 5)."""
    make, N, seeded = FD_SHAPES[name]
    G = make()
    E = G.number_of_edges()
    f = 0.1 + 0.02 * (np.arange(E) % 5)
    R = seeded_coefficients(29, E)["R"] if seeded else 0.5 + (np.arange(E) % 3) / 2.0
    return G, N, R, f


def reversed_edges(src, dst, degrees) -> np.ndarray:
    """The degree of the node each REVERSED edge points into, one entry per reversed edge: an
    edge is reversed where its target is its source's parent in the breadth-first forest from
    node 0 (the forest of ``layout_fe.build_cp_tables``), so the edge's local direction runs
    against the forest's. Entries >= 3: reversed edges at junctions."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    n = int(max(src.max(), dst.max())) + 1
    adj = [[] for _ in range(n)]
    for a, b in zip(src, dst):
        adj[a].append(int(b))
        adj[b].append(int(a))
    depth = np.full(n, -1, dtype=np.int64)
    depth[0] = 0
    q = deque([0])
    while q:
        u = q.popleft()
        for w in adj[u]:
            if depth[w] < 0:
                depth[w] = depth[u] + 1
                q.append(w)
    assert depth.min() >= 0, "connected"
    rev = depth[dst] < depth[src]
    return np.asarray(degrees, dtype=np.int64)[dst[rev]]


def decomposition_facts(pc) -> dict:
    """What a decomposition holds, from its host arrays, split into job slots and top slots:
    most junction children and most down-chain entries of a slot, most slots / levels /
    needed top values of a job, the top part's slots and levels; ``job_top_kids``: most
    children of a job slot in a decomposition that also has a top part (else 0)."""
    ts0, ts1 = int(pc.top_lvl_off[0]), int(pc.top_lvl_off[-1])
    ent = np.diff(pc.slot_dc_off).astype(np.int64)
    kid = np.zeros(pc.n_slots, dtype=np.int64)
    own = np.repeat(np.arange(pc.n_slots), ent)
    np.add.at(kid, own[np.asarray(pc.dc_lo) >= 0], 1)
    # a top slot's children that are top slots themselves (the top sweeps' children)
    tkid = np.zeros(pc.n_slots, dtype=np.int64)
    np.add.at(tkid, own[np.asarray(pc.dc_lo) >= ts0], 1)
    js, jl = [0], [0]
    for j in range(pc.n_jobs):
        lv0, lv1 = int(pc.job_lvl_off[j]), int(pc.job_lvl_off[j + 1])
        jl.append(lv1 - lv0)
        js.append(int(pc.lvl_slot_off[lv1] - pc.lvl_slot_off[lv0]) if lv1 > lv0 else 0)
    need = np.diff(pc.job_need_off) if pc.job_need_off.size > 1 else np.zeros(1, int)
    mx = lambda a: int(a.max()) if a.size else 0  # noqa: E731
    return {
        "job_kids": mx(kid[:ts0]), "top_kids": mx(kid[ts0:ts1]), "top_top_kids": mx(tkid[ts0:ts1]),
        "job_entries": mx(ent[:ts0]), "top_entries": mx(ent[ts0:ts1]),
        "job_slots": max(js), "job_levels": max(jl),
        "top_slots": ts1 - ts0, "top_levels": int(pc.top_lvl_off.size - 1) if ts1 > ts0 else 0,
        "need": mx(need), "n_jobs": int(pc.n_jobs),
        "chains": mx(np.diff(pc.job_chain_off)) if pc.n_jobs else 0,
        "job_top_kids": mx(kid[:ts0]) if ts1 > ts0 else 0,
    }


def cp_record_facts(tab) -> dict:
    """What the node records of the continuous-pressure direct solve have to hold, from the
    tables of ``layout_fe.build_cp_tables`` (the breadth-first forest from node 0): the most
    incident edges and the most children of a node, the nodes whose record is exactly full
    (``kCpRecInc`` incident edges and ``kCpRecCh`` children: every slot of the record is
    read) and the nodes past either cap (the lists)."""
    inc = np.diff(np.asarray(tab.inc_off, dtype=np.int64))
    ch = np.diff(np.asarray(tab.child_off, dtype=np.int64))
    return {"inc": int(inc.max()), "ch": int(ch.max()),
            "full": int(np.count_nonzero((inc == K_CP_REC_INC) & (ch == K_CP_REC_CH))),
            "over": int(np.count_nonzero((inc > K_CP_REC_INC) | (ch > K_CP_REC_CH)))}


# shape -> (most incident edges, most children) of a node of its breadth-first forest: hub3's
# hub fills its record exactly, cat70 stays under both caps, every other hub and broom is past
# both (hub4 by one each)
CP_RECORDS = {"hub3": (4, 3), "hub4": (5, 4), "hub5": (6, 5), "hub9": (10, 9),
              "broom5": (6, 5), "broom33": (34, 33), "cat70": (3, 2),
              # (hub70: 71 incident edges at one node; hubhub5x5: the hub of hubs and its five
              # hubs; rand200_s1: 13 nodes past the caps, the largest with 19 edges)
              "hub70": (71, 70), "hubhub5x5": (6, 5), "rand200_s1": (19, 19)}


def check_cp_records(name: str, tab) -> dict:
    """Assert the facts of ``CP_RECORDS`` on a shape's tables, and on which side of the caps
    they put it; returns ``cp_record_facts``."""
    f = cp_record_facts(tab)
    assert (f["inc"], f["ch"]) == CP_RECORDS[name], (name, f)
    if name == "hub3":  # at the caps: one record exactly full, none past it
        assert (f["inc"], f["ch"]) == (K_CP_REC_INC, K_CP_REC_CH), f
        assert f["full"] == 1 and f["over"] == 0, f
    elif name == "cat70":  # under both caps
        assert f["inc"] < K_CP_REC_INC and f["ch"] < K_CP_REC_CH, f
        assert f["full"] == 0 and f["over"] == 0, f
    else:  # past both caps: the lists, the level's pipelined runs erased
        assert f["inc"] > K_CP_REC_INC and f["ch"] > K_CP_REC_CH and f["over"] >= 1, f
    return f


def _blocks(d: np.ndarray, ref: np.ndarray, parts) -> tuple[float, ...]:
    tot = np.linalg.norm(ref)
    out = []
    for idx in parts:
        nr = np.linalg.norm(ref[idx])
        out.append(float(np.linalg.norm(d[idx]) / (nr if nr >= 1e-8 * tot else tot)))
    return tuple(out)


def block_errors(x, x_ref, E: int, N: int) -> tuple[float, float, float]:
    """Build layout (per edge ``[q_0, p_0, q_1, .., p_{N-1}, q_N]``, then the multipliers):
    ``|x - x_ref| / |x_ref|`` over the flux rows, the pressure rows and the multipliers
    separately. A block whose reference norm is below 1e-8 |x_ref| (no junction, or
    multipliers that vanish by symmetry) is measured against |x_ref| instead."""
    x, x_ref = np.asarray(x), np.asarray(x_ref)
    per = 2 * N + 1
    loc = np.arange(E * per) % per
    q = np.flatnonzero(loc % 2 == 0)
    p = np.flatnonzero(loc % 2 == 1)
    lm = np.arange(E * per, x_ref.size)
    return _blocks(x - x_ref, x_ref, (q, p, lm))


def block_errors_oracle(x, x_ref, p_offset: int, lm_offset: int) -> tuple[float, float, float]:
    """The same in the oracle's block order ``[fluxes | pressures | multipliers]``
    (``P.p_offset``, ``P.lm_offset``)."""
    x, x_ref = np.asarray(x), np.asarray(x_ref)
    n = x_ref.size
    return _blocks(x - x_ref, x_ref, (np.arange(p_offset), np.arange(p_offset, lm_offset),
                                      np.arange(lm_offset, n)))
