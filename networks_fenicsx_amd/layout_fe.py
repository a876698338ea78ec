"""DoF layout and gather-assembly tables for general element degrees.

``HydraulicNetworkAssembler(mesh, flux_degree=k, pressure_degree=m)`` (reference
``assembly.py:121-146``) with ``(k, m) != (1, 0)``. The P1/DG0 default keeps its own layout
and kernels (``layout.py``, ``k_assemble*``); this module serves every other stable pair.

Device layout (``n_rows`` owned rows, no ghosts):

* every graph edge ``e`` (``graph.edges()`` order) owns ``kN+1`` flux rows (the Lagrange
  nodes along the edge, source -> target) followed by its edge-interior pressure rows:
  ``N`` cell values for DG0, else the ``mN-1`` interior nodes of continuous P_m;
* continuous pressure only: one row per graph node that has an edge (ascending id) --
  the pressure value shared by every edge meeting there (``assembly.py:135-145``: the
  pressure space lives on the whole network mesh);
* one multiplier row per bifurcation (ascending node id).

Pressure rows and their rhs are negated, as in the P1 path, so the matrix is symmetric.

Several ranks (DG0 pressure, ``build_fe_rank_layout``): a rank holds the edges, owned
multipliers and ghost columns of its P1/DG0 rank layout (``layout.build_local_problem``) --
its local edges' rows, then its owned multipliers, then the ghost columns in the P1 layout's
order (the multipliers of cut bifurcations owned elsewhere and the remote flux ends its
multiplier rows read). The halo plan is the P1 rank layout's, renumbered.

Assembly tables: every nonzero and every rhs entry is a short sum of terms
``table_val[ent] x factor`` (factor ``R_e h_c``, ``f h_c``, ``edge_bc`` or 1; see
``include/nxhip.h`` ``nx_create_fe``). The terms are generated cell by cell from the
reference element tensors (:mod:`element`) and grouped per output in generation order,
so the device sums them in a fixed order (``k_assemble_fe``).
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from .element import element_tensors, stable_pair

__all__ = ["FeLayout", "build_fe_layout", "build_fe_rank_layout", "build_fe_partition",
           "fe_global_rows", "fe_row_owner", "build_cp_rank_tables", "KIND_CONST", "KIND_MASS", "KIND_SOURCE", "KIND_BC"]

KIND_CONST, KIND_MASS, KIND_SOURCE, KIND_BC = 0, 1, 2, 3


@dataclass
class FeLayout:
    N: int
    k: int
    m: int
    E: int
    n_rows: int
    rowptr: np.ndarray  # int32 (n_rows+1,)
    col: np.ndarray  # int32 (nnz,)
    table_kind: np.ndarray  # int32
    table_val: np.ndarray  # f64
    a_ptr: np.ndarray  # int32 (nnz+1,)
    a_idx: np.ndarray  # int32
    a_ent: np.ndarray  # int32
    b_ptr: np.ndarray  # int32 (n_rows+1,)
    b_idx: np.ndarray  # int32
    b_ent: np.ndarray  # int32
    flux_rows: np.ndarray  # (E, kN+1) device rows of each edge's flux nodes
    p_rows: np.ndarray  # device row of every pressure DoF, in the function's order
    p_nodes: np.ndarray  # graph nodes carrying a pressure DoF (m >= 1)
    lm_nodes: np.ndarray  # bifurcations, ascending
    lm_rows: np.ndarray
    edge_x: np.ndarray  # (E, 6) source xyz, target xyz
    # several ranks (build_fe_rank_layout): the ghost columns after the owned rows, the
    # global edge id of every local edge, and the halo plan (nx_set_halo's arrays)
    n_ghost: int = 0
    edges: np.ndarray | None = None
    n_edges_global: int = 0
    peers: np.ndarray | None = None
    send_off: np.ndarray | None = None
    send_idx: np.ndarray | None = None
    recv_off: np.ndarray | None = None
    n_own_edges: int = -1  # build_fe_partition: edges [0, n_own_edges) own rows, the rest
    global_rows: np.ndarray | None = None  # are ghost edges (coefficients only)
    ghost_rows: np.ndarray | None = None

    @property
    def nnz(self) -> int:
        return int(self.col.size)


def _tables(k: int, m: int):
    """The term table (kinds, values) and its entry indices for the pair (k, m)."""
    Mref, Dref, wref = element_tensors(k, m)
    nq, npl = k + 1, wref.size
    ent = {"mass": np.arange(nq * nq).reshape(nq, nq),
           "b": nq * nq + np.arange(npl * nq).reshape(npl, nq)}
    ent["plus"] = nq * nq + npl * nq
    ent["minus"] = ent["plus"] + 1
    ent["src"] = ent["minus"] + 1 + np.arange(npl)
    ent["bc"] = int(ent["src"][-1]) + 1
    table_kind = np.concatenate([np.full(nq * nq, KIND_MASS), np.full(npl * nq, KIND_CONST),
                                 [KIND_CONST, KIND_CONST], np.full(npl, KIND_SOURCE),
                                 [KIND_BC]]).astype(np.int32)
    # negated pressure rows: divergence -Dref (row p, col q); gradient -Dref^T (row q, col p)
    table_val = np.concatenate([Mref.ravel(), -Dref.ravel(), [1.0, -1.0], -wref, [1.0]])
    return table_kind, table_val, ent, nq, npl


def _cell_terms(qrow, prow, cell, ent, nq, npl, E, N):
    """Every cell's mass and divergence / gradient terms, in generation order."""
    rows, cols, idx, ents = [], [], [], []
    for i in range(nq):
        for j in range(nq):
            rows.append(qrow[:, :, i]); cols.append(qrow[:, :, j])  # noqa: E702
            idx.append(cell); ents.append(np.full((E, N), ent["mass"][i, j]))  # noqa: E702
    for a in range(npl):
        for j in range(nq):
            rows.append(prow[:, :, a]); cols.append(qrow[:, :, j])  # noqa: E702
            idx.append(cell); ents.append(np.full((E, N), ent["b"][a, j]))  # noqa: E702
            rows.append(qrow[:, :, j]); cols.append(prow[:, :, a])  # noqa: E702
            idx.append(cell); ents.append(np.full((E, N), ent["b"][a, j]))  # noqa: E702
    return rows, cols, idx, ents


def _csr_and_rhs(rows, cols, idx, ents, br, bi, be, n_rows):
    """Terms grouped per (row, column) in generation order -> CSR pattern and term lists;
    rhs terms grouped per row."""
    R = np.concatenate([np.ravel(x) for x in rows])
    C = np.concatenate([np.ravel(x) for x in cols])
    Ix = np.concatenate([np.ravel(x) for x in idx])
    T = np.concatenate([np.ravel(x) for x in ents])
    order = np.lexsort((np.arange(R.size), C, R))  # by row, column, then generation order
    R, C, Ix, T = R[order], C[order], Ix[order], T[order]
    new = np.ones(R.size, dtype=bool)
    new[1:] = (R[1:] != R[:-1]) | (C[1:] != C[:-1])
    starts = np.flatnonzero(new)
    a_ptr = np.append(starts, R.size)
    col = C[starts]
    rowptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(R[starts], minlength=n_rows), out=rowptr[1:])
    BR = np.concatenate([np.ravel(x) for x in br])
    BI = np.concatenate([np.ravel(x) for x in bi])
    BE = np.concatenate([np.ravel(x) for x in be])
    border = np.argsort(BR, kind="stable")
    b_ptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(BR, minlength=n_rows), out=b_ptr[1:])
    if max(a_ptr[-1], rowptr[-1], n_rows) >= np.iinfo(np.int32).max:
        raise ValueError("problem too large for 32-bit CSR indices")
    return rowptr, col, a_ptr, Ix, T, b_ptr, BI[border], BE[border]


def build_fe_layout(pos: np.ndarray, src: np.ndarray, dst: np.ndarray, degree: np.ndarray,
                    N: int, k: int, m: int) -> FeLayout:
    """Layout and term tables for flux degree ``k`` and pressure degree ``m``."""
    if not stable_pair(k, m):
        raise ValueError(
            f"flux_degree={k}, pressure_degree={m}: continuous pressure needs a flux degree "
            "above the pressure degree, otherwise the system is singular")
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    E = src.size
    n_nodes = pos.shape[0]
    nf = k * N + 1
    npe = N if m == 0 else m * N - 1
    per = nf + npe
    base = np.arange(E, dtype=np.int64) * per
    flux_rows = base[:, None] + np.arange(nf)[None, :]
    p_nodes = np.flatnonzero(degree > 0) if m >= 1 else np.zeros(0, dtype=np.int64)
    node_row = np.full(n_nodes, -1, dtype=np.int64)
    node_row[p_nodes] = E * per + np.arange(p_nodes.size)
    lm_nodes = np.flatnonzero(degree > 1)
    lm_row = np.full(n_nodes, -1, dtype=np.int64)
    lm_row[lm_nodes] = E * per + p_nodes.size + np.arange(lm_nodes.size)
    n_rows = E * per + p_nodes.size + lm_nodes.size

    c = np.arange(N)
    qrow = base[:, None, None] + (c[:, None] * k + np.arange(k + 1)[None, :])[None]  # (E,N,k+1)
    if m == 0:
        prow = (base[:, None] + nf + c[None, :])[:, :, None]  # (E,N,1)
    else:
        ppos = c[:, None] * m + np.arange(m + 1)[None, :]  # (N, m+1) positions 0..mN
        prow = np.broadcast_to(base[:, None, None] + nf + ppos[None] - 1, (E, N, m + 1)).copy()
        prow = np.where(ppos[None] == 0, node_row[src][:, None, None], prow)
        prow = np.where(ppos[None] == m * N, node_row[dst][:, None, None], prow)

    table_kind, table_val, ent, nq, npl = _tables(k, m)
    cell = np.arange(E, dtype=np.int64)[:, None] * N + c[None, :]  # (E, N)
    rows, cols, idx, ents = _cell_terms(qrow, prow, cell, ent, nq, npl, E, N)
    # junctions (assembly.py:268-277): +1 at in-edge ends, -1 at out-edge starts, both blocks
    e_in = np.flatnonzero(lm_row[dst] >= 0)
    e_out = np.flatnonzero(lm_row[src] >= 0)
    for e_set, lam, qr, en in ((e_in, lm_row[dst[e_in]], flux_rows[e_in, -1], ent["plus"]),
                               (e_out, lm_row[src[e_out]], flux_rows[e_out, 0], ent["minus"])):
        z = np.zeros(e_set.size, dtype=np.int64)
        rows += [lam, qr]; cols += [qr, lam]  # noqa: E702
        idx += [z, z]; ents += [np.full(e_set.size, en), np.full(e_set.size, en)]  # noqa: E702
    # rhs: source on pressure rows, boundary data at both flux ends of every edge
    e_ids = np.arange(E, dtype=np.int64)
    br = [prow[:, :, a] for a in range(npl)] + [flux_rows[:, 0], flux_rows[:, -1]]
    bi = [cell for _ in range(npl)] + [2 * e_ids, 2 * e_ids + 1]
    be = [np.full((E, N), ent["src"][a]) for a in range(npl)] + [np.full(E, ent["bc"])] * 2
    rowptr, col, a_ptr, Ix, T, b_ptr, BI, BE = _csr_and_rhs(rows, cols, idx, ents, br, bi, be,
                                                            n_rows)

    if m == 0:
        p_rows = (base[:, None] + nf + c[None, :]).ravel()
    else:
        p_rows = np.concatenate([node_row[p_nodes],
                                 (base[:, None] + nf + np.arange(m * N - 1)[None, :]).ravel()])
    pos3 = np.zeros((n_nodes, 3))
    pos3[:, : pos.shape[1]] = pos
    edge_x = np.concatenate([pos3[src], pos3[dst]], axis=1)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    return FeLayout(N, k, m, E, int(n_rows), i32(rowptr), i32(col), table_kind,
                    np.ascontiguousarray(table_val), i32(a_ptr), i32(Ix), i32(T), i32(b_ptr),
                    i32(BI), i32(BE), flux_rows, p_rows, p_nodes, lm_nodes,
                    lm_row[lm_nodes], edge_x, n_edges_global=E)


def build_fe_rank_layout(pos: np.ndarray, src: np.ndarray, dst: np.ndarray, N: int, k: int,
                         lp) -> FeLayout:
    """One rank's (k, 0) layout over the edges, owned multipliers and ghost columns of its
    P1/DG0 rank layout ``lp`` (``layout.build_local_problem``, several ranks). Its rows are
    the one-rank layout's rows of those edges and multipliers (``fe_global_rows``): the same
    terms, the remote flux ends of an owned multiplier row as ghost columns."""
    m = 0
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    edges = np.asarray(lp.edges, dtype=np.int64)
    E = edges.size
    nf, npe = k * N + 1, N
    per = nf + npe
    per1 = 2 * N + 1
    n_lm = int(np.asarray(lp.lm_nodes).size)
    n_own = E * per + n_lm
    n_own1 = int(lp.n_own)
    n_edge1 = E * per1
    base = np.arange(E, dtype=np.int64) * per
    flux_rows = base[:, None] + np.arange(nf)[None, :]

    def col_of(c1):  # P1 rank column -> this layout's column
        c1 = np.asarray(c1, dtype=np.int64)
        s, j = np.divmod(np.minimum(c1, n_edge1 - 1) if E else c1 * 0, per1)
        edge_col = s * per + np.where(j == 0, 0, nf - 1)
        return np.where(c1 >= n_own1, n_own + (c1 - n_own1),
                        np.where(c1 >= n_edge1, E * per + (c1 - n_edge1), edge_col))

    c = np.arange(N)
    qrow = base[:, None, None] + (c[:, None] * k + np.arange(k + 1)[None, :])[None]
    prow = (base[:, None] + nf + c[None, :])[:, :, None]
    table_kind, table_val, ent, nq, npl = _tables(k, m)
    cell = np.arange(E, dtype=np.int64)[:, None] * N + c[None, :]
    rows, cols, idx, ents = _cell_terms(qrow, prow, cell, ent, nq, npl, E, N)
    # flux end rows -> their multiplier (owned row or ghost column): lp.edge_lm
    elm = np.asarray(lp.edge_lm, dtype=np.int64).reshape(E, 2)
    for end, en in ((0, ent["minus"]), (1, ent["plus"])):
        on = np.flatnonzero(elm[:, end] >= 0)
        rows.append(flux_rows[on, 0 if end == 0 else -1])
        cols.append(col_of(elm[on, end]))
        idx.append(np.zeros(on.size, dtype=np.int64))
        ents.append(np.full(on.size, en))
    # owned multiplier rows -> every incident flux end (local or ghost): lp's rows
    lrp = np.asarray(lp.lm_rowptr, dtype=np.int64)
    lcol = np.asarray(lp.lm_col, dtype=np.int64)
    lval = np.asarray(lp.lm_val, dtype=np.float64)
    lrow = np.repeat(np.arange(n_lm), np.diff(lrp))
    rows.append(E * per + lrow)
    cols.append(col_of(lcol))
    idx.append(np.zeros(lcol.size, dtype=np.int64))
    ents.append(np.where(lval > 0, ent["plus"], ent["minus"]))
    e_ids = np.arange(E, dtype=np.int64)
    br = [prow[:, :, 0], flux_rows[:, 0], flux_rows[:, -1]]
    bi = [cell, 2 * e_ids, 2 * e_ids + 1]
    be = [np.full((E, N), ent["src"][0]), np.full(E, ent["bc"]), np.full(E, ent["bc"])]
    rowptr, col, a_ptr, Ix, T, b_ptr, BI, BE = _csr_and_rhs(rows, cols, idx, ents, br, bi, be,
                                                            n_own)
    n_nodes = pos.shape[0]
    pos3 = np.zeros((n_nodes, 3))
    pos3[:, : pos.shape[1]] = pos
    edge_x = np.concatenate([pos3[src[edges]], pos3[dst[edges]]], axis=1)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    lay = FeLayout(N, k, m, E, int(n_own), i32(rowptr), i32(col), table_kind,
                   np.ascontiguousarray(table_val), i32(a_ptr), i32(Ix), i32(T), i32(b_ptr),
                   i32(BI), i32(BE), flux_rows, (base[:, None] + nf + c[None, :]).ravel(),
                   np.zeros(0, dtype=np.int64), np.asarray(lp.lm_nodes, dtype=np.int64),
                   E * per + np.arange(n_lm, dtype=np.int64), edge_x)
    lay.n_ghost = int(lp.n_ghost)
    lay.edges = edges
    lay.n_edges_global = int(src.size)
    lay.peers = i32(lp.peers)
    lay.send_off = i32(lp.send_off)
    lay.send_idx = i32(col_of(np.asarray(lp.send_idx, dtype=np.int64)))
    lay.recv_off = i32(lp.recv_off)
    return lay


def fe_row_owner(lay: FeLayout, src: np.ndarray, dst: np.ndarray, edge_owner: np.ndarray,
                 n_nodes: int) -> np.ndarray:
    """Owning rank of every row of a one-rank layout: an edge's rows go with the edge, a
    node's shared pressure row and a bifurcation's multiplier row with the node's first
    in-edge, else its first out-edge (``layout.build_local_problem``'s rule)."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    E = src.size
    per = lay.k * lay.N + 1 + (lay.N if lay.m == 0 else lay.m * lay.N - 1)
    first_in = np.full(n_nodes, E, dtype=np.int64)
    np.minimum.at(first_in, dst, np.arange(E))
    first_out = np.full(n_nodes, E, dtype=np.int64)
    np.minimum.at(first_out, src, np.arange(E))
    anchor = np.where(first_in < E, first_in, first_out)
    own = np.empty(lay.n_rows, dtype=np.int32)
    own[: E * per] = np.repeat(np.asarray(edge_owner, dtype=np.int32), per)
    pn = np.asarray(lay.p_nodes, dtype=np.int64)
    own[E * per: E * per + pn.size] = edge_owner[anchor[pn]]
    own[np.asarray(lay.lm_rows, dtype=np.int64)] = edge_owner[anchor[np.asarray(lay.lm_nodes)]]
    return own


def build_fe_partition(full: FeLayout, src: np.ndarray, dst: np.ndarray,
                       edge_owner: np.ndarray, rank: int, nranks: int) -> FeLayout:
    """One rank's part of a one-rank layout ``full`` by row ownership (``fe_row_owner``),
    for any pair -- continuous pressure's shared node rows included. The rank's rows are
    its owned rows in the one-rank order (its edges' rows, its node pressure rows, its
    multipliers); every other column it reads is a ghost, ordered by owner, then by the
    owner's local index, so the owner's send list and the ghost slots line up. Its edges
    are its own (ascending) then the ghost edges whose cells its rows' terms read (a shared
    node row sums the element terms of every edge at the node): coefficients and cell
    lengths cover both, rows only the owned."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    E, N = src.size, full.N
    per = full.k * N + 1 + (N if full.m == 0 else full.m * N - 1)
    owner_e = np.asarray(edge_owner, dtype=np.int32)
    n_nodes = int(max(src.max(), dst.max())) + 1 if E else 0
    n_nodes = max(n_nodes, int(np.max(full.p_nodes, initial=-1)) + 1,
                  int(np.max(full.lm_nodes, initial=-1)) + 1)
    row_own = fe_row_owner(full, src, dst, owner_e, n_nodes)
    rows_of = [np.flatnonzero(row_own == q) for q in range(nranks)]
    loc = np.empty(full.n_rows, dtype=np.int64)  # local index on the owning rank
    for q in range(nranks):
        loc[rows_of[q]] = np.arange(rows_of[q].size)
    mine = rows_of[rank]
    n_own = mine.size
    rp = np.asarray(full.rowptr, dtype=np.int64)
    starts, ends = rp[mine], rp[mine + 1]
    cnt = ends - starts
    ent_idx = (np.repeat(starts - np.cumsum(np.concatenate([[0], cnt[:-1]])), cnt)
               + np.arange(int(cnt.sum())))  # the owned rows' entries, in order
    gcol = np.asarray(full.col, dtype=np.int64)[ent_idx]

    def ghosts_of(q):
        rq = rows_of[q]
        s_, e_ = rp[rq], rp[rq + 1]
        c_ = e_ - s_
        ix = np.repeat(s_ - np.cumsum(np.concatenate([[0], c_[:-1]])), c_) + np.arange(int(c_.sum()))
        cq = np.unique(np.asarray(full.col, dtype=np.int64)[ix])
        cq = cq[row_own[cq] != q]
        return cq[np.lexsort((loc[cq], row_own[cq]))]

    gh = ghosts_of(rank)
    col_local = np.empty(full.n_rows, dtype=np.int64)
    col_local[mine] = np.arange(n_own)
    col_local[gh] = n_own + np.arange(gh.size)
    col = col_local[gcol]
    o = np.lexsort((col, np.repeat(np.arange(n_own), cnt)))  # rows keep sorted local columns
    ent_idx, col = ent_idx[o], col[o]
    # terms of the owned entries and rhs rows; the cells / edges they read
    kind = np.asarray(full.table_kind)
    ap = np.asarray(full.a_ptr, dtype=np.int64)
    t0, t1 = ap[ent_idx], ap[ent_idx + 1]
    tcnt = t1 - t0
    tix = np.repeat(t0 - np.cumsum(np.concatenate([[0], tcnt[:-1]])), tcnt) + np.arange(int(tcnt.sum()))
    a_idx = np.asarray(full.a_idx, dtype=np.int64)[tix]
    a_ent = np.asarray(full.a_ent, dtype=np.int64)[tix]
    bp = np.asarray(full.b_ptr, dtype=np.int64)
    b0, b1 = bp[mine], bp[mine + 1]
    bcnt = b1 - b0
    bix = np.repeat(b0 - np.cumsum(np.concatenate([[0], bcnt[:-1]])), bcnt) + np.arange(int(bcnt.sum()))
    b_idx = np.asarray(full.b_idx, dtype=np.int64)[bix]
    b_ent = np.asarray(full.b_ent, dtype=np.int64)[bix]
    # a term's idx is a cell for the mass / source kinds and for the divergence entries (the
    # constants before the junctions' +-1, kept as their cell: _cell_terms), else 0 / 2e+end
    ent_junction = (full.k + 1) ** 2 + (1 if full.m == 0 else full.m + 1) * (full.k + 1)
    a_cell = np.isin(kind[a_ent], [KIND_MASS, KIND_SOURCE]) | (
        (kind[a_ent] == KIND_CONST) & (a_ent < ent_junction))
    b_cell = np.isin(kind[b_ent], [KIND_MASS, KIND_SOURCE])
    b_bc = kind[b_ent] == KIND_BC
    own_e = np.flatnonzero(owner_e == rank)
    read_e = np.unique(np.concatenate([a_idx[a_cell] // N, b_idx[b_cell] // N, b_idx[b_bc] // 2]))
    ghost_e = np.setdiff1d(read_e, own_e)
    edges = np.concatenate([own_e, ghost_e])
    e_loc = np.full(E, -1, dtype=np.int64)
    e_loc[edges] = np.arange(edges.size)
    a_idx[a_cell] = e_loc[a_idx[a_cell] // N] * N + a_idx[a_cell] % N
    b_new = b_idx.copy()
    b_new[b_cell] = e_loc[b_idx[b_cell] // N] * N + b_idx[b_cell] % N
    b_new[b_bc] = 2 * e_loc[b_idx[b_bc] // 2] + b_idx[b_bc] % 2
    b_idx = b_new
    rowptr = np.concatenate([[0], np.cumsum(cnt)])
    a_ptr = np.concatenate([[0], np.cumsum(tcnt)])
    b_ptr = np.concatenate([[0], np.cumsum(bcnt)])
    # the function rows: owned edges' flux rows, pressure in the function's order, multipliers
    flux_rows = col_local[np.asarray(full.flux_rows)[own_e]]
    p_sel = np.asarray(full.p_rows, dtype=np.int64)
    p_rows = col_local[p_sel[row_own[p_sel] == rank]]
    pn = np.asarray(full.p_nodes, dtype=np.int64)
    pn_rows = E * per + np.arange(pn.size)
    lmr = np.asarray(full.lm_rows, dtype=np.int64)
    lm_mine = row_own[lmr] == rank
    # halo plan: what each peer reads of mine, in its ghost order
    peers, send_off, send_idx, recv_off = [], [0], [], [0]
    g_owner = row_own[gh]
    for q in range(nranks):
        if q == rank:
            continue
        theirs = ghosts_of(q)
        snd = loc[theirs[row_own[theirs] == rank]]
        rcv = int(np.count_nonzero(g_owner == q))
        if snd.size == 0 and rcv == 0:
            continue
        peers.append(q)
        send_idx.extend(snd.tolist())
        send_off.append(len(send_idx))
        recv_off.append(recv_off[-1] + rcv)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    lay = FeLayout(N, full.k, full.m, int(edges.size), int(n_own), i32(rowptr), i32(col),
                   full.table_kind, full.table_val, i32(a_ptr), i32(a_idx), i32(a_ent),
                   i32(b_ptr), i32(b_idx), i32(b_ent), flux_rows, p_rows,
                   pn[row_own[pn_rows] == rank], np.asarray(full.lm_nodes)[lm_mine],
                   col_local[lmr[lm_mine]], np.asarray(full.edge_x)[edges])
    lay.n_ghost = int(gh.size)
    lay.edges = edges
    lay.n_edges_global = E
    lay.n_own_edges = int(own_e.size)
    lay.global_rows = mine
    lay.ghost_rows = gh
    lay.peers = i32(peers)
    lay.send_off = i32(send_off)
    lay.send_idx = i32(send_idx)
    lay.recv_off = i32(recv_off)
    return lay


def fe_global_rows(lay: FeLayout, degree: np.ndarray) -> np.ndarray:
    """The one-rank layout row (``build_fe_layout`` of the whole graph) of every owned row of
    a rank layout: edge rows by global edge, multipliers by bifurcation rank (DG0)."""
    if getattr(lay, "global_rows", None) is not None:  # build_fe_partition keeps them
        return np.asarray(lay.global_rows, dtype=np.int64)
    per = lay.k * lay.N + 1 + lay.N
    edges = np.arange(lay.E) if lay.edges is None else np.asarray(lay.edges, dtype=np.int64)
    bif = np.flatnonzero(np.asarray(degree) > 1)
    lam = lay.n_edges_global * per + np.searchsorted(bif, np.asarray(lay.lm_nodes, np.int64))
    return np.concatenate([(edges[:, None] * per + np.arange(per)[None, :]).ravel(), lam])


def evaluate_terms(lay: FeLayout, R_edge: np.ndarray, f, edge_bc: np.ndarray,
                   cell_h: np.ndarray):
    """Host evaluation of the term tables (what ``k_assemble_fe`` computes), for tests and
    debugging: returns ``(val, rhs)``. ``cell_h`` is ``(E, N)``; ``f`` a constant or one value
    per edge."""
    h = np.asarray(cell_h, dtype=np.float64).ravel()
    Rc = np.repeat(np.asarray(R_edge, dtype=np.float64), lay.N)
    fc = np.repeat(np.broadcast_to(np.asarray(f, dtype=np.float64), (lay.E,)), lay.N)
    bc = np.asarray(edge_bc, dtype=np.float64).ravel()

    def term(i, e):
        kind, v = lay.table_kind[e], lay.table_val[e]
        if kind == KIND_MASS:
            return (Rc[i] * h[i]) * v
        if kind == KIND_SOURCE:
            return (fc[i] * h[i]) * v
        if kind == KIND_BC:
            return bc[i] * v
        return v

    kind = lay.table_kind[lay.a_ent]
    v = lay.table_val[lay.a_ent]
    tv = np.where(kind == KIND_MASS, (Rc[np.where(kind == KIND_MASS, lay.a_idx, 0)]
                                      * h[np.where(kind == KIND_MASS, lay.a_idx, 0)]) * v, v)
    val = np.add.reduceat(tv, lay.a_ptr[:-1]) if tv.size else np.zeros(0)
    rhs = np.zeros(lay.n_rows)
    for r in range(lay.n_rows):
        s = 0.0
        for t in range(lay.b_ptr[r], lay.b_ptr[r + 1]):
            s += term(lay.b_idx[t], lay.b_ent[t])
        rhs[r] = s
    return val, rhs


@dataclass
class FeAuxMaps:
    """Rows of the P1/DG0-structured system that the flux-degree-k / DG0 system condenses to
    (``nx_fe_set_direct``): per FE cell-vertex flux, pressure cell and multiplier, the row of
    the auxiliary P1 handle built from ``layout.build_local_problem`` of the same graph."""

    v_fe: np.ndarray  # (E (N+1),) FE rows of the vertex fluxes, edge-major (graph order)
    v_aux: np.ndarray  # their rows in the auxiliary system
    i_fe: np.ndarray  # (E N (k-1),) FE rows of the interior fluxes, cell-major
    p_fe: np.ndarray  # (E N,) FE pressure rows, edge-major
    p_aux: np.ndarray
    l_fe: np.ndarray  # (B,) FE multiplier rows, ascending node
    l_aux: np.ndarray


def fe_aux_slots(lay: FeLayout, lp) -> np.ndarray:
    """The auxiliary P1 handle's slot of every edge of the layout (its local order)."""
    ge = np.arange(lay.E) if lay.edges is None else np.asarray(lay.edges, dtype=np.int64)
    full = np.full(max(lay.n_edges_global, lay.E), -1, dtype=np.int64)
    full[np.asarray(lp.edges, dtype=np.int64)] = np.arange(np.asarray(lp.edges).size)
    slot = full[ge]
    if (slot < 0).any() or np.asarray(lp.edges).size != lay.E:
        raise ValueError("the auxiliary problem must hold the layout's edges")
    return slot


def build_fe_aux_maps(lay: FeLayout, lp) -> FeAuxMaps:
    """Row maps between a (k, 0) layout and the P1 local problem ``lp`` of the same edges
    (one rank: the whole graph; several: the rank's P1 layout that ``build_fe_rank_layout``
    followed) -- its edge slots ``lp.edges`` in its own order, multipliers by ascending node."""
    if lay.m != 0:
        raise ValueError("the condensed direct solve is DG0's (pressure_degree 0)")
    E, N, k = lay.E, lay.N, lay.k
    slot = fe_aux_slots(lay, lp)
    per1 = 2 * N + 1
    g = np.arange(N + 1)
    v_fe = lay.flux_rows[:, k * g].ravel()
    v_aux = (slot[:, None] * per1 + 2 * g[None, :]).ravel()
    c = np.arange(N)
    i_fe = (lay.flux_rows[:, (k * c)[:, None] + np.arange(1, k)[None, :]]).ravel()
    p_fe = lay.p_rows.astype(np.int64)
    p_aux = (slot[:, None] * per1 + 2 * c[None, :] + 1).ravel()
    lm1 = np.asarray(lp.lm_nodes, dtype=np.int64)
    pos = np.searchsorted(lm1, lay.lm_nodes)
    if not np.array_equal(lm1[np.minimum(pos, lm1.size - 1)], lay.lm_nodes):
        raise ValueError("multiplier nodes differ")
    l_aux = lp.n_edge_dofs + pos
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    return FeAuxMaps(i32(v_fe), i32(v_aux), i32(i_fe), i32(p_fe), i32(p_aux),
                     i32(lay.lm_rows), i32(l_aux))


@dataclass
class CpTables:
    """The continuous-pressure direct solve's tables (``nx_fe_set_cp``, include/nxhip.h):
    reference blocks, border nodes (every graph node with an edge), per edge its end nodes
    and multiplier couplings, and the node forest in level order."""

    k: int
    m: int
    nI: int
    cst: np.ndarray  # Kh | Ch | Eh | Fh | reference flux mass (k+1)^2 | source weights (m+1)
    tI: np.ndarray
    n_nodes: int
    nrow: np.ndarray  # (n, 2) pressure row, multiplier row or -1
    eb: np.ndarray  # (E, 4) source node, target node, q_0 - lam_src, q_N - lam_dst couplings
    lev_off: np.ndarray
    order: np.ndarray
    inc_off: np.ndarray
    inc: np.ndarray  # (n_inc, 2) edge, end (0 source, 1 target)
    parent: np.ndarray  # (n, 3) parent node, edge, this node's end of it (-1 at a root)
    child_off: np.ndarray
    child: np.ndarray
    nown: np.ndarray  # the edge that writes each node's rows
    # graphs with cycles (``build_cp_tables(..., cycles=True)``): the non-tree edges of the BFS
    # forest, ascending, and the distinct real border slots at their ends, sorted -- (node,
    # slot) pairs, slot 0 the pressure, 1 the multiplier (where the node has one)
    chord: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    cslot: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))  # (n_slots, 2)


def build_cp_tables(lay: FeLayout, src: np.ndarray, dst: np.ndarray,
                    cycles: bool = False) -> CpTables | None:
    """Tables of the node-condensed direct solve for continuous pressure (``lay.m >= 1``), or
    ``None`` when the graph is not a forest (a cycle: MINRES). ``cycles=True``: a non-tree
    edge of the BFS becomes a chord (``chord``, ``cslot``: the grounded solve's low-rank
    correction, ``nx_fe_cp_set_cycles``) instead; ``parent`` / ``child`` / the levels describe
    the spanning forest, ``inc`` keeps every edge. A self-loop still gives ``None``."""
    from collections import deque

    from .element import condensed_cell_blocks

    if lay.m < 1:
        raise ValueError("the node-condensed solve is continuous pressure's (m >= 1)")
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    E = lay.E
    nodes = np.asarray(lay.p_nodes, dtype=np.int64)
    n = nodes.size
    idx = np.full(int(max(src.max(), dst.max())) + 1 if E else 0, -1, dtype=np.int64)
    idx[nodes] = np.arange(n)
    u, v = idx[src], idx[dst]
    per = lay.k * lay.N + 1 + lay.m * lay.N - 1
    lam = np.full(idx.size, -1, dtype=np.int64)
    lam[np.asarray(lay.lm_nodes, dtype=np.int64)] = np.asarray(lay.lm_rows, dtype=np.int64)
    nrow = np.stack([E * per + np.arange(n), lam[nodes]], axis=1)
    eb = np.stack([u, v, np.where(lam[src] >= 0, -1, 0), np.where(lam[dst] >= 0, 1, 0)], axis=1)
    # incidence (edge, end), by node then edge
    ne = np.concatenate([u, v])
    ee = np.concatenate([np.arange(E), np.arange(E)])
    en = np.concatenate([np.zeros(E, np.int64), np.ones(E, np.int64)])
    o = np.lexsort((ee, ne))
    inc = np.stack([ee[o], en[o]], axis=1)
    inc_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ne, minlength=n), out=inc_off[1:])
    # BFS forest from the lowest node of every component
    parent = np.full((n, 3), -1, dtype=np.int64)
    level = np.full(n, -1, dtype=np.int64)
    if cycles and bool((u == v).any()):
        return None  # a self-loop
    is_chord = np.zeros(E, dtype=bool)
    for r in range(n):
        if level[r] >= 0:
            continue
        level[r] = 0
        dq = deque([r])
        while dq:
            a = dq.popleft()
            for j in range(inc_off[a], inc_off[a + 1]):
                e, end = inc[j]
                b = v[e] if end == 0 else u[e]
                if b == a or (parent[a, 1] == e):
                    continue
                if level[b] >= 0:
                    if not cycles:
                        return None  # a cycle
                    is_chord[e] = True  # (met from both its ends: recorded once)
                    continue
                level[b] = level[a] + 1
                parent[b] = (a, e, 1 - end)
                dq.append(b)
    order = np.lexsort((np.arange(n), level))
    nlev = int(level.max()) + 1 if n else 1
    lev_off = np.zeros(nlev + 1, dtype=np.int64)
    np.cumsum(np.bincount(level, minlength=nlev), out=lev_off[1:])
    has = parent[:, 0] >= 0
    ch_par = parent[has, 0]
    ch = np.flatnonzero(has)
    oc = np.lexsort((ch, ch_par))
    child = ch[oc]
    child_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ch_par, minlength=n), out=child_off[1:])
    nown = inc[inc_off[:-1], 0]
    Kh, Ch, Eh, Fh, tI = condensed_cell_blocks(lay.k, lay.m)
    # (behind them the reference mass and a cell's source weights, from the term tables the rhs
    # kernel evaluates: nx_cp_batch_gradient's contraction)
    _, tval, ent, _, _ = _tables(lay.k, lay.m)
    cst = np.concatenate([Kh.ravel(), Ch.ravel(), Eh.ravel(), Fh.ravel(),
                          tval[ent["mass"]].ravel(), tval[ent["src"]]])
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ravel()  # noqa: E731
    tab = CpTables(lay.k, lay.m, int(tI.size), cst, i32(tI), int(n), i32(nrow), i32(eb),
                   i32(lev_off), i32(order), i32(inc_off), i32(inc), i32(parent),
                   i32(child_off), i32(child), i32(nown))
    chord = np.flatnonzero(is_chord)
    if chord.size:
        ends = np.unique(np.concatenate([u[chord], v[chord]]))
        real = ends[nrow[ends, 1] >= 0]
        cs = np.concatenate([np.stack([ends, np.zeros_like(ends)], axis=1),
                             np.stack([real, np.ones_like(real)], axis=1)])
        tab.chord = i32(chord)
        tab.cslot = i32(cs[np.lexsort((cs[:, 1], cs[:, 0]))])
    return tab


def build_cp_rank_tables(tab: CpTables, part: FeLayout):
    """One rank's share of the node-condensed solve (``nx_fe_cp_ranks`` + ``nx_fe_set_cp``)
    from the one-rank tables ``tab`` and the rank's partition ``part``
    (``build_fe_partition``): ``(tab_rank, gid, nrowx)``. The rank's edges run the edge
    kernels (``eb`` of its own edges; ``gid`` their global ids); the node tables keep global
    nodes and edges, every rank solving the whole node forest over the summed blocks; ``nrow``
    names the summed node rhs (2n, 2n + 1 or -1); ``nrowx`` the local rows of the node rows
    this rank owns, and ``nown`` the local edge that writes them (-1 elsewhere). ``chord`` /
    ``cslot`` (a graph with cycles) pass through: the node tables are global on every rank."""
    from dataclasses import replace

    own_e = np.asarray(part.edges, dtype=np.int64)[: part.n_own_edges]
    n = tab.n_nodes
    nrow_g = np.asarray(tab.nrow, dtype=np.int64).reshape(n, 2)
    grows = np.asarray(part.global_rows, dtype=np.int64)

    def local(rows):
        i = np.searchsorted(grows, rows)
        i = np.minimum(i, max(grows.size - 1, 0))
        hit = (rows >= 0) & (grows.size > 0) & (grows[i] == rows)
        return np.where(hit, i, -1)

    nrowx = np.stack([local(nrow_g[:, 0]), local(nrow_g[:, 1])], axis=1)
    nrow_nb = np.stack([2 * np.arange(n), np.where(nrow_g[:, 1] >= 0, 2 * np.arange(n) + 1, -1)],
                       axis=1)
    # the node rows' writer: the node's anchor edge when this rank owns the rows (the anchor
    # is then one of its own edges)
    e_loc = np.full(part.n_edges_global, -1, dtype=np.int64)
    e_loc[own_e] = np.arange(own_e.size)
    src_e = np.asarray(tab.eb, dtype=np.int64).reshape(-1, 4)
    # one-rank writer (nown) is any incident edge; take the owned one: the first incident
    # edge of the node that is local
    inc = np.asarray(tab.inc, dtype=np.int64).reshape(-1, 2)
    off = np.asarray(tab.inc_off, dtype=np.int64)
    nown = np.full(n, -1, dtype=np.int64)
    for nd in np.flatnonzero(nrowx[:, 0] >= 0):
        loc_edges = e_loc[inc[off[nd]:off[nd + 1], 0]]
        loc_edges = loc_edges[loc_edges >= 0]
        nown[nd] = loc_edges[0]
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ravel()  # noqa: E731
    tab_r = replace(tab, nrow=i32(nrow_nb), eb=i32(src_e[own_e]), nown=i32(nown))
    return tab_r, i32(own_e), i32(nrowx)


def cp_model(lay: FeLayout, tab: CpTables, val: np.ndarray, b: np.ndarray, R: np.ndarray,
             cell_h: np.ndarray, info: dict | None = None) -> np.ndarray:
    """numpy restatement of the device's node-condensed solve (k_cp_edge, k_cp_nodes,
    k_cp_back) for tests: ``x`` of the (k, m) system with values ``val`` and rhs ``b``. With
    chords (``tab.chord``) the grounded sweep is corrected as ``fe_cp_solve`` does. ``info``
    (a dict) receives the nodes' pivot inverses ``Pinv`` and the capacitance matrix ``cap``."""
    import scipy.sparse as sp

    A = sp.csr_matrix((val, lay.col, lay.rowptr), shape=(lay.n_rows, lay.n_rows))
    N, k, m, nI, E = lay.N, lay.k, lay.m, tab.nI, lay.E
    nf = k * N + 1
    per = nf + m * N - 1
    Kh = tab.cst[:16].reshape(4, 4)
    Ch = tab.cst[16:16 + 4 * nI].reshape(4, nI)
    Eh = tab.cst[16 + 4 * nI:16 + 8 * nI].reshape(nI, 4)
    Fh = tab.cst[16 + 8 * nI:16 + 8 * nI + nI * nI].reshape(nI, nI)
    tI = tab.tI.astype(np.int64)
    tV = np.array([1, -1, 1, -1])
    eb = tab.eb.reshape(-1, 4)
    nrow = tab.nrow.reshape(-1, 2)
    h = np.asarray(cell_h).reshape(E, N)
    x = np.zeros(lay.n_rows)
    Se, ge, facs = np.zeros((E, 4, 4)), np.zeros((E, 4)), []
    for e in range(E):
        base = e * per
        prow = lambda j: base + nf + j - 1  # noqa: E731
        irow = lambda c, i: base + c * k + 1 + i if tI[i] > 0 else prow(c * m + 1 + i - (k - 1))  # noqa: E731
        P = np.array([[0.0, 0.0], [0.0, 1.0]])
        W = np.zeros((2, 4))
        W[0, 1] = eb[e, 2]
        rho = np.array([b[base], 0.0])
        Sb, gb, fe = np.zeros((4, 4)), np.zeros(4), []
        for c in range(N):
            s = R[e] * h[e, c]
            K = Kh * s ** ((tV[:, None] + tV[None, :]) // 2)
            bI = np.array([b[irow(c, i)] for i in range(nI)])
            rV = -(Ch * s ** ((tV[:, None] - tI[None, :]) // 2)) @ bI if nI else np.zeros(4)
            Wn = np.zeros((2, 4))
            if c == 0:
                P[0, 0] += K[0, 0]; W[0, 0] += K[0, 1]; Sb[0, 0] += K[1, 1]  # noqa: E702
                rho[0] += rV[0]; gb[0] += rV[1]  # noqa: E702
                C = np.array([[K[0, 2], K[0, 3]], [0.0, 0.0]])
                Wn[0, 0], Wn[1, 0] = K[2, 1], K[3, 1]
            else:
                P += K[:2, :2]; rho += rV[:2]  # noqa: E702
                C = K[:2, 2:].copy()
            if c + 1 < N:
                Pn = K[2:, 2:].copy()
                rn = rV[2:] + np.array([b[base + k * (c + 1)], b[prow(m * (c + 1))]])
            else:
                Sb[2, 2] += K[3, 3]; gb[2] += rV[3]  # noqa: E702
                if c == 0:
                    Sb[0, 2] += K[1, 3]; Sb[2, 0] += K[3, 1]  # noqa: E702
                Wn[0, 2] += K[2, 3]; Wn[0, 3] = eb[e, 3]; Wn[1, 0] = 0.0  # noqa: E702
                W[:, 2] += C[:, 1]; C[:, 1] = 0.0  # noqa: E702
                Pn = np.array([[K[2, 2], 0.0], [0.0, 1.0]])
                rn = np.array([rV[2] + b[base + nf - 1], 0.0])
            Pi = np.linalg.inv(P)
            Pn -= C.T @ Pi @ C; Wn -= C.T @ Pi @ W; rn -= C.T @ Pi @ rho  # noqa: E702
            Sb -= W.T @ Pi @ W; gb -= W.T @ Pi @ rho  # noqa: E702
            fe.append((Pi, C, W, rho))
            P, W, rho = Pn, Wn, rn
        Pi = np.linalg.inv(P)
        Sb -= W.T @ Pi @ W; gb -= W.T @ Pi @ rho  # noqa: E702
        fe.append((Pi, np.zeros((2, 2)), W, rho))
        Se[e], ge[e] = Sb, gb
        facs.append(fe)
    n = tab.n_nodes
    inc = tab.inc.reshape(-1, 2)
    par = tab.parent.reshape(-1, 3)
    Pinv, hv, xn = np.zeros((n, 2, 2)), np.zeros((n, 2)), np.zeros((n, 2))
    blk = lambda e, ra, cb: Se[e][2 * ra:2 * ra + 2, 2 * cb:2 * cb + 2]  # noqa: E731
    lev = tab.lev_off
    for L in range(lev.size - 2, -1, -1):
        for i in range(lev[L], lev[L + 1]):
            nd = tab.order[i]
            D = np.zeros((2, 2))
            g = np.array([b[nrow[nd, 0]], b[nrow[nd, 1]] if nrow[nd, 1] >= 0 else 0.0])
            for j in range(tab.inc_off[nd], tab.inc_off[nd + 1]):
                e, end = inc[j]
                D += blk(e, end, end)
                g += ge[e][2 * end:2 * end + 2]
            if nrow[nd, 1] < 0:
                D[1, 1] = 1.0
            for j in range(tab.child_off[nd], tab.child_off[nd + 1]):
                c = tab.child[j]
                B = blk(par[c, 1], par[c, 2], 1 - par[c, 2])
                D -= B.T @ Pinv[c] @ B
                g -= B.T @ Pinv[c] @ hv[c]
            Pinv[nd], hv[nd] = np.linalg.inv(D), g
    for L in range(lev.size - 1):
        for i in range(lev[L], lev[L + 1]):
            nd = tab.order[i]
            r = hv[nd].copy()
            if par[nd, 0] >= 0:
                r -= blk(par[nd, 1], par[nd, 2], 1 - par[nd, 2]) @ xn[par[nd, 0]]
            xn[nd] = Pinv[nd] @ r
    if info is not None:
        info["Pinv"] = Pinv.copy()
    if np.asarray(tab.chord).size:
        # a graph with cycles: the sweeps above solved the grounded system S_g (every chord's
        # off-diagonal blocks dropped); S = S_g + U C U^T, x = S_g^-1 (g - U w) with
        # w = (I + C U^T Z)^-1 C U^T x_g, Z = S_g^-1 U (rhs-only sweeps with the stored pivots)
        def sweep(gn):
            hh, xx = np.zeros_like(gn), np.zeros_like(gn)  # (n, 2, columns)
            for L in range(lev.size - 2, -1, -1):
                for i in range(lev[L], lev[L + 1]):
                    nd = tab.order[i]
                    g = gn[nd].copy()
                    for j in range(tab.child_off[nd], tab.child_off[nd + 1]):
                        c = tab.child[j]
                        g -= blk(par[c, 1], par[c, 2], 1 - par[c, 2]).T @ Pinv[c] @ hh[c]
                    hh[nd] = g
            for L in range(lev.size - 1):
                for i in range(lev[L], lev[L + 1]):
                    nd = tab.order[i]
                    r = hh[nd].copy()
                    if par[nd, 0] >= 0:
                        r -= blk(par[nd, 1], par[nd, 2], 1 - par[nd, 2]) @ xx[par[nd, 0]]
                    xx[nd] = Pinv[nd] @ r
            return xx

        cs = np.asarray(tab.cslot).reshape(-1, 2)
        ns = cs.shape[0]
        pos = {(int(a), int(s)): i for i, (a, s) in enumerate(cs)}
        Cm = np.zeros((ns, ns))
        for e in np.asarray(tab.chord):
            for end in (0, 1):
                a, o = eb[e, end], eb[e, 1 - end]
                B = blk(e, end, 1 - end)
                for s in (0, 1):
                    for t in (0, 1):
                        if (a, s) in pos and (o, t) in pos:
                            Cm[pos[a, s], pos[o, t]] += B[s, t]
        unit = np.zeros((n, 2, ns))
        unit[cs[:, 0], cs[:, 1], np.arange(ns)] = 1.0
        UtZ = sweep(unit)[cs[:, 0], cs[:, 1], :]
        cap = np.eye(ns) + Cm @ UtZ
        w = np.linalg.solve(cap, Cm @ xn[cs[:, 0], cs[:, 1]])
        gn = np.zeros((n, 2))
        for nd in range(n):
            gn[nd] = (b[nrow[nd, 0]], b[nrow[nd, 1]] if nrow[nd, 1] >= 0 else 0.0)
            for j in range(tab.inc_off[nd], tab.inc_off[nd + 1]):
                e, end = inc[j]
                gn[nd] += ge[e][2 * end:2 * end + 2]
        gn[cs[:, 0], cs[:, 1]] -= w
        xn = sweep(gn[:, :, None])[:, :, 0]
        # one refinement of the grounded solve (k_cp_cyc_res, the sweep, k_cp_cyc_add): the
        # 2 x 2 pivots' explicit inverses cost the one-sweep residual up to two digits
        for _ in range(1):
            rho = gn.copy()
            for nd in range(n):
                D = np.zeros((2, 2))
                for j in range(tab.inc_off[nd], tab.inc_off[nd + 1]):
                    e, end = inc[j]
                    D += blk(e, end, end)
                if nrow[nd, 1] < 0:
                    D[1, 1] = 1.0
                rho[nd] -= D @ xn[nd]
                if par[nd, 0] >= 0:
                    rho[nd] -= blk(par[nd, 1], par[nd, 2], 1 - par[nd, 2]) @ xn[par[nd, 0]]
                for j in range(tab.child_off[nd], tab.child_off[nd + 1]):
                    c = tab.child[j]
                    rho[nd] -= blk(par[c, 1], par[c, 2], 1 - par[c, 2]).T @ xn[c]
            xn = xn + sweep(rho[:, :, None])[:, :, 0]
        if info is not None:
            info["cap"] = cap
    for nd in range(n):
        x[nrow[nd, 0]] = xn[nd, 0]
        if nrow[nd, 1] >= 0:
            x[nrow[nd, 1]] = xn[nd, 1]
    for e in range(E):
        base = e * per
        prow = lambda j: base + nf + j - 1  # noqa: E731
        xb = np.concatenate([xn[eb[e, 0]], xn[eb[e, 1]]])
        yn = np.zeros(2)
        for i in range(N, -1, -1):
            Pi, C, W, rho = facs[e][i]
            y = Pi @ (rho - C @ yn - W @ xb)
            x[base + k * i] = y[0]
            if 0 < i < N:
                x[prow(m * i)] = y[1]
            if i < N:
                s = R[e] * h[e, i]
                xv = np.array([y[0], xb[0] if i == 0 else y[1], yn[0], xb[2] if i + 1 == N else yn[1]])
                bI = np.array([b[base + i * k + 1 + j] if tI[j] > 0
                               else b[prow(i * m + 1 + j - (k - 1))] for j in range(nI)])
                xI = (Fh * s ** (-(tI[:, None] + tI[None, :]) // 2)) @ bI \
                    - (Eh * s ** ((-tI[:, None] + tV[None, :]) // 2)) @ xv if nI else []
                for j in range(nI):
                    r = base + i * k + 1 + j if tI[j] > 0 else prow(i * m + 1 + j - (k - 1))
                    x[r] = xI[j]
            yn = y
    del A
    return x


def cp_factor_model(lay: FeLayout, tab: CpTables, R: np.ndarray, cell_h: np.ndarray) -> dict:
    """numpy restatement of ``nx_cp_batch_solve``'s factor stage (k_cp_b_factor, then the node
    forest's up-sweep on a zero right-hand side), in the kernels' order of operations: what
    the node-condensed solve derives from the matrix alone. No right-hand side enters.
    Returns ``fac`` (E, N + 1, 16): per vertex Pi | C | W, ``Se`` (E, 16) and ``Pinv``
    (n_nodes, 4), for :func:`cp_apply_model`."""
    N, E = lay.N, lay.E
    Kh = np.asarray(tab.cst[:16], dtype=np.float64)
    tV = (1, -1, 1, -1)
    eb = tab.eb.reshape(-1, 4)
    nrow = tab.nrow.reshape(-1, 2)
    h = np.asarray(cell_h, dtype=np.float64).reshape(E, N)

    def pw(s, ex):
        return s if ex > 0 else (1.0 / s if ex < 0 else 1.0)

    def inv2(P):
        idet = 1.0 / (P[0] * P[3] - P[1] * P[2])
        return [P[3] * idet, -P[1] * idet, -P[2] * idet, P[0] * idet]

    fac = np.zeros((E, N + 1, 16))
    Se = np.zeros((E, 16))
    for e in range(E):
        P = [0.0, 0.0, 0.0, 1.0]
        W = [0.0] * 8
        W[1] = float(eb[e, 2])
        Sb = [0.0] * 16
        for c in range(N):
            s = float(R[e]) * float(h[e, c])
            K = [float(Kh[4 * r + q]) * pw(s, (tV[r] + tV[q]) // 2)
                 for r in range(4) for q in range(4)]
            Wn = [0.0] * 8
            if c == 0:
                P[0] += K[0]
                W[0] += K[1]
                Sb[0] += K[5]
                C = [K[2], K[3], 0.0, 0.0]
                Wn[0], Wn[4] = K[9], K[13]
            else:
                P[0] += K[0]
                P[1] += K[1]
                P[2] += K[4]
                P[3] += K[5]
                C = [K[2], K[3], K[6], K[7]]
            if c + 1 < N:
                Pn = [K[10], K[11], K[14], K[15]]
            else:
                Sb[10] += K[15]
                if c == 0:
                    Sb[2] += K[7]
                    Sb[8] += K[13]
                Wn[2] += K[11]
                Wn[3] = float(eb[e, 3])
                Wn[4] = 0.0
                W[2] += C[1]
                W[6] += C[3]
                C[1] = C[3] = 0.0
                Pn = [K[10], 0.0, 0.0, 1.0]
            Pi = inv2(P)
            X = [Pi[2 * r] * C[q] + Pi[2 * r + 1] * C[2 + q] for r in range(2) for q in range(2)]
            Y = [Pi[2 * r] * W[q] + Pi[2 * r + 1] * W[4 + q] for r in range(2) for q in range(4)]
            for r in range(2):
                for q in range(2):
                    Pn[2 * r + q] -= C[r] * X[q] + C[2 + r] * X[2 + q]
                for q in range(4):
                    Wn[4 * r + q] -= C[r] * Y[q] + C[2 + r] * Y[4 + q]
            for r in range(4):
                for q in range(4):
                    Sb[4 * r + q] -= W[r] * Y[q] + W[4 + r] * Y[4 + q]
            fac[e, c] = Pi + C + W
            P, W = Pn, Wn
        Pi = inv2(P)
        Y = [Pi[2 * r] * W[q] + Pi[2 * r + 1] * W[4 + q] for r in range(2) for q in range(4)]
        for r in range(4):
            for q in range(4):
                Sb[4 * r + q] -= W[r] * Y[q] + W[4 + r] * Y[4 + q]
        fac[e, N] = Pi + [0.0] * 4 + W
        Se[e] = Sb
    n = tab.n_nodes
    inc = tab.inc.reshape(-1, 2)
    par = tab.parent.reshape(-1, 3)
    Pinv = np.zeros((n, 4))
    lev = tab.lev_off
    for L in range(lev.size - 2, -1, -1):
        for i in range(lev[L], lev[L + 1]):
            nd = tab.order[i]
            D = [0.0] * 4
            for j in range(tab.inc_off[nd], tab.inc_off[nd + 1]):
                e, end = inc[j]
                Bk = _cp_blk(Se, e, end, end)
                for q in range(4):
                    D[q] += Bk[q]
            if nrow[nd, 1] < 0:
                D[3] = 1.0
            for j in range(tab.child_off[nd], tab.child_off[nd + 1]):
                c = tab.child[j]
                Bk = _cp_blk(Se, par[c, 1], par[c, 2], 1 - par[c, 2])
                Pc = Pinv[c]
                X = [Pc[2 * r] * Bk[q] + Pc[2 * r + 1] * Bk[2 + q]
                     for r in range(2) for q in range(2)]
                for r in range(2):
                    for q in range(2):
                        D[2 * r + q] -= Bk[r] * X[q] + Bk[2 + r] * X[2 + q]
            Pinv[nd] = inv2(D)
    return {"fac": fac, "Se": Se, "Pinv": Pinv}


def _cp_blk(Se, e, ra, cb):
    """cp_block: rows of end ``ra``, columns of end ``cb`` of edge ``e``'s border block."""
    S = Se[e]
    return [float(S[4 * (2 * ra) + 2 * cb]), float(S[4 * (2 * ra) + 2 * cb + 1]),
            float(S[4 * (2 * ra + 1) + 2 * cb]), float(S[4 * (2 * ra + 1) + 2 * cb + 1])]


def cp_apply_model(lay: FeLayout, tab: CpTables, fm: dict, Bm: np.ndarray, R: np.ndarray,
                   cell_h: np.ndarray) -> np.ndarray:
    """numpy restatement of ``nx_cp_batch_solve``'s right-hand-side sweeps (k_cp_b_fwd,
    k_cp_b_nodes, k_cp_b_back) on the factors ``fm`` of :func:`cp_factor_model`: ``Bm``
    ``(n_cols, n_rows)`` right-hand sides, returns the ``(n_cols, n_rows)`` solutions. Every
    operation is elementwise over the columns, in the kernels' order, so a column's bits do
    not depend on the columns beside it."""
    Bm = np.ascontiguousarray(Bm, dtype=np.float64)
    z, ge = _cp_fwd_model(lay, tab, fm, Bm, R, cell_h)
    xn = _cp_sweep_model(tab, fm, _cp_node_rhs_model(tab, Bm, ge))
    return _cp_back_model(lay, tab, fm, Bm, R, cell_h, z, xn)


def _cp_fwd_model(lay, tab, fm, Bm, R, cell_h):
    """k_cp_b_fwd: per column z = Pi rho per vertex ``(E, N + 1, 2, nc)`` and ge per edge
    ``(E, 4, nc)``."""
    nc = Bm.shape[0]
    N, k, m, nI, E = lay.N, lay.k, lay.m, tab.nI, lay.E
    nf = k * N + 1
    per = nf + m * N - 1
    Ch = np.asarray(tab.cst[16:16 + 4 * nI], dtype=np.float64).reshape(4, nI)
    tI = [int(t) for t in tab.tI]
    h = np.asarray(cell_h, dtype=np.float64).reshape(E, N)
    fac = fm["fac"]
    zero = np.zeros(nc)

    def lrow(c, i):  # cell c's interior node i (local row)
        return c * k + 1 + i if tI[i] > 0 else nf + (c * m + 1 + (i - (k - 1))) - 1

    z = np.zeros((E, N + 1, 2, nc))
    ge = np.zeros((E, 4, nc))
    for e in range(E):
        bl = Bm[:, e * per:(e + 1) * per]
        rho = [bl[:, 0].copy(), zero.copy()]
        gb = [zero.copy() for _ in range(4)]
        for c in range(N + 1):
            f = [float(v) for v in fac[e, c]]
            Pi, C, W = f[:4], f[4:8], f[8:]
            if c < N:
                s = float(R[e]) * float(h[e, c])
                si = 1.0 / s
                rV = [zero.copy() for _ in range(4)]
                for i in range(nI):
                    pq, pp = (1.0, si) if tI[i] > 0 else (s, 1.0)
                    cf = [float(Ch[0, i]) * pq, float(Ch[1, i]) * pp, float(Ch[2, i]) * pq,
                          float(Ch[3, i]) * pp]
                    bi = bl[:, lrow(c, i)]
                    for r in range(4):
                        rV[r] = rV[r] - cf[r] * bi
                rho[0] = rho[0] + rV[0]
                if c == 0:
                    gb[0] = gb[0] + rV[1]
                else:
                    rho[1] = rho[1] + rV[1]
                if c + 1 < N:
                    rn = [rV[2] + bl[:, k * (c + 1)], rV[3] + bl[:, nf + m * (c + 1) - 1]]
                else:
                    gb[2] = gb[2] + rV[3]
                    rn = [rV[2] + bl[:, nf - 1], zero.copy()]
            z0 = Pi[0] * rho[0] + Pi[1] * rho[1]
            z1 = Pi[2] * rho[0] + Pi[3] * rho[1]
            if c < N:
                for r in range(2):
                    rn[r] = rn[r] - (C[r] * z0 + C[2 + r] * z1)
            for r in range(4):
                gb[r] = gb[r] - (W[r] * z0 + W[4 + r] * z1)
            z[e, c, 0], z[e, c, 1] = z0, z1
            if c < N:
                rho = rn
        for r in range(4):
            ge[e, r] = gb[r]
    return z, ge


def _cp_node_rhs_model(tab, Bm, ge):
    """The node right-hand side ``(n, 2, nc)``: a node's rows of B plus its edges' ge in list
    order (cp_b_node_up's first sums; k_cp_b_cyc_rhs before it subtracts w)."""
    nc = Bm.shape[0]
    n = tab.n_nodes
    inc = tab.inc.reshape(-1, 2)
    nrow = tab.nrow.reshape(-1, 2)
    g = np.zeros((n, 2, nc))
    for nd in range(n):
        g0 = Bm[:, nrow[nd, 0]].copy()
        g1 = Bm[:, nrow[nd, 1]].copy() if nrow[nd, 1] >= 0 else np.zeros(nc)
        for j in range(tab.inc_off[nd], tab.inc_off[nd + 1]):
            e, end = inc[j]
            g0 = g0 + ge[e, 2 * end]
            g1 = g1 + ge[e, 2 * end + 1]
        g[nd, 0], g[nd, 1] = g0, g1
    return g


def _cp_sweep_model(tab, fm, g):
    """k_cp_b_nodes / k_cp_b_level on the node right-hand sides ``g`` ``(n, 2, nc)``: up (minus
    the children's terms, the node's own term for its parent), then down; returns the node
    values ``(n, 2, nc)``."""
    Se, Pinv = fm["Se"], fm["Pinv"]
    n = tab.n_nodes
    nc = g.shape[2]
    par = tab.parent.reshape(-1, 3)
    hv, ct, xn = np.zeros((n, 2, nc)), np.zeros((n, 2, nc)), np.zeros((n, 2, nc))
    lev = tab.lev_off
    for L in range(lev.size - 2, -1, -1):
        for i in range(lev[L], lev[L + 1]):
            nd = tab.order[i]
            g0, g1 = g[nd, 0].copy(), g[nd, 1].copy()
            for j in range(tab.child_off[nd], tab.child_off[nd + 1]):
                c = tab.child[j]
                g0 = g0 - ct[c, 0]
                g1 = g1 - ct[c, 1]
            hv[nd, 0], hv[nd, 1] = g0, g1
            if par[nd, 0] >= 0:
                Bk = _cp_blk(Se, par[nd, 1], par[nd, 2], 1 - par[nd, 2])
                Pc = [float(v) for v in Pinv[nd]]
                z0 = Pc[0] * g0 + Pc[1] * g1
                z1 = Pc[2] * g0 + Pc[3] * g1
                ct[nd, 0] = Bk[0] * z0 + Bk[2] * z1
                ct[nd, 1] = Bk[1] * z0 + Bk[3] * z1
    for L in range(lev.size - 1):
        for i in range(lev[L], lev[L + 1]):
            nd = tab.order[i]
            r0, r1 = hv[nd, 0].copy(), hv[nd, 1].copy()
            if par[nd, 0] >= 0:
                Bk = _cp_blk(Se, par[nd, 1], par[nd, 2], 1 - par[nd, 2])
                xp = xn[par[nd, 0]]
                r0 = r0 - (Bk[0] * xp[0] + Bk[1] * xp[1])
                r1 = r1 - (Bk[2] * xp[0] + Bk[3] * xp[1])
            Pn = [float(v) for v in Pinv[nd]]
            xn[nd, 0] = Pn[0] * r0 + Pn[1] * r1
            xn[nd, 1] = Pn[2] * r0 + Pn[3] * r1
    return xn


def _cp_back_model(lay, tab, fm, Bm, R, cell_h, z, xn):
    """k_cp_b_back: the columns' solutions ``(nc, n_rows)`` from z and the node values."""
    nc = Bm.shape[0]
    N, k, m, nI, E = lay.N, lay.k, lay.m, tab.nI, lay.E
    nf = k * N + 1
    per = nf + m * N - 1
    Eh = np.asarray(tab.cst[16 + 4 * nI:16 + 8 * nI], dtype=np.float64).reshape(nI, 4)
    Fh = np.asarray(tab.cst[16 + 8 * nI:16 + 8 * nI + nI * nI],
                    dtype=np.float64).reshape(nI, nI)
    tI = [int(t) for t in tab.tI]
    eb = tab.eb.reshape(-1, 4)
    nrow = tab.nrow.reshape(-1, 2)
    h = np.asarray(cell_h, dtype=np.float64).reshape(E, N)
    fac = fm["fac"]
    n = tab.n_nodes
    zero = np.zeros(nc)

    def lrow(c, i):  # cell c's interior node i (local row)
        return c * k + 1 + i if tI[i] > 0 else nf + (c * m + 1 + (i - (k - 1))) - 1

    X = np.zeros_like(Bm)
    for nd in range(n):
        X[:, nrow[nd, 0]] = xn[nd, 0]
        if nrow[nd, 1] >= 0:
            X[:, nrow[nd, 1]] = xn[nd, 1]
    for e in range(E):
        base = e * per
        bl = Bm[:, base:base + per]
        xb = [xn[eb[e, 0], 0], xn[eb[e, 0], 1], xn[eb[e, 1], 0], xn[eb[e, 1], 1]]
        yn = [zero.copy(), zero.copy()]
        for i in range(N, -1, -1):
            f = [float(v) for v in fac[e, i]]
            Pi, C, W = f[:4], f[4:8], f[8:]
            Xc = [Pi[2 * r] * C[q] + Pi[2 * r + 1] * C[2 + q] for r in range(2) for q in range(2)]
            Y = [Pi[2 * r] * W[q] + Pi[2 * r + 1] * W[4 + q] for r in range(2) for q in range(4)]
            y0, y1 = z[e, i, 0].copy(), z[e, i, 1].copy()
            for q in range(4):
                y0 = y0 - Y[q] * xb[q]
                y1 = y1 - Y[4 + q] * xb[q]
            y0 = y0 - (Xc[0] * yn[0] + Xc[1] * yn[1])
            y1 = y1 - (Xc[2] * yn[0] + Xc[3] * yn[1])
            X[:, base + k * i] = y0
            if 0 < i < N:
                X[:, base + nf + m * i - 1] = y1
            if i < N:
                s = float(R[e]) * float(h[e, i])
                si = 1.0 / s
                xv = [y0, xb[0] if i == 0 else y1, yn[0], xb[2] if i + 1 == N else yn[1]]
                for j in range(nI):
                    val = zero.copy()
                    for l in range(nI):  # noqa: E741
                        ex = -(tI[j] + tI[l]) // 2
                        cf = float(Fh[j, l]) * (s if ex > 0 else si if ex < 0 else 1.0)
                        val = val + cf * bl[:, lrow(i, l)]
                    pq, pp = (1.0, si) if tI[j] > 0 else (s, 1.0)
                    ce = [float(Eh[j, 0]) * pq, float(Eh[j, 1]) * pp, float(Eh[j, 2]) * pq,
                          float(Eh[j, 3]) * pp]
                    for q in range(4):
                        val = val - ce[q] * xv[q]
                    X[:, base + lrow(i, j)] = val
            yn = [y0, y1]
    return X


CP_CYC_PARTS = 8  # kCpcParts of csrc/nxhip.hip: the strided parts of a row's sum in k_cp_b_cyc_w


def _cp_cyc_tables(tab: CpTables):
    """The slot tables ``nx_fe_cp_set_cycles`` derives (cpc_attach): ``slot`` (ns,) = 2 node +
    (0 pressure, 1 multiplier), ``slot_of`` (2 n,) and per slot its node's chord ends in
    ascending chord order -- ``(chord edge, the node's end, the other end's pressure slot, its
    multiplier slot or -1)``."""
    cs = np.asarray(tab.cslot).reshape(-1, 2)
    slot = [2 * int(a) + int(s) for a, s in cs]
    slot_of = -np.ones(2 * tab.n_nodes, dtype=np.int64)
    slot_of[slot] = np.arange(len(slot))
    eb = tab.eb.reshape(-1, 4)
    at = [[] for _ in range(tab.n_nodes)]
    for e in np.asarray(tab.chord):
        e = int(e)
        at[int(eb[e, 0])].append((e, 0))
        at[int(eb[e, 1])].append((e, 1))
    ent = []
    for sl in slot:
        row = []
        for e, end in at[sl >> 1]:
            o = int(eb[e, 1 - end])
            row.append((e, end, int(slot_of[2 * o]), int(slot_of[2 * o + 1])))
        ent.append(row)
    return slot, slot_of, ent


def _cp_cyc_coef(Se, e, end, s):
    """cp_cyc_coef: the coupling of row ``s`` of chord ``e``'s end ``end`` to the other end's
    pressure and multiplier."""
    S = Se[e]
    q = 4 * (2 * end + s) + 2 * (1 - end)
    return float(S[q]), float(S[q + 1])


def cp_cyc_factor_model(lay: FeLayout, tab: CpTables, R: np.ndarray, cell_h: np.ndarray) -> dict:
    """:func:`cp_factor_model` on a graph with cycles, with what ``nx_cp_batch_solve`` builds
    once per contents of ``R`` on top of it (cp_batch_cyc_build). The chords are absent from
    the forest's parent and child lists and their diagonal blocks are in the incidence lists,
    so the factor stage factors the grounded system ``S_g`` as it stands. Then, in the kernels'
    order: ``UtZ`` (ns, ns) by unit right-hand sides through the stored pivots (k_cp_zcols: the
    sweeps of :func:`cp_apply_model`'s node part), ``cap = I + C U^T Z`` (k_cp_cap: a row
    slot's chord ends in list order) and ``inv``, its inverse by Gauss-Jordan elimination with
    partial pivoting (k_gj_*: the first row of the largest magnitude; the device may contract
    the elimination's multiply-subtract, so ``inv`` agrees to rounding). ``ok`` is False where
    a pivot is zero. Without chords it returns :func:`cp_factor_model`'s dict with ``ns = 0``."""
    fm = cp_factor_model(lay, tab, R, cell_h)
    fm["ns"] = 0
    if not np.asarray(tab.chord).size:
        return fm
    slot, slot_of, ent = _cp_cyc_tables(tab)
    ns = len(slot)
    Se = fm["Se"]
    unit = np.zeros((tab.n_nodes, 2, ns))
    for j, sl in enumerate(slot):
        unit[sl >> 1, sl & 1, j] = 1.0
    Z = _cp_sweep_model(tab, fm, unit)
    UtZ = np.stack([Z[sl >> 1, sl & 1] for sl in slot])  # (slot i, column j)
    cap = np.eye(ns)
    for r, sl in enumerate(slot):
        v = cap[r].copy()
        for e, end, op, om in ent[r]:
            cp, cm = _cp_cyc_coef(Se, e, end, sl & 1)
            v = v + cp * UtZ[op]
            if om >= 0:
                v = v + cm * UtZ[om]
        cap[r] = v
    aug = np.hstack([cap, np.eye(ns)])
    ok = True
    for col in range(ns):
        p = col + int(np.argmax(np.abs(aug[col:, col])))
        if not abs(aug[p, col]) > 0.0:
            ok = False
            break
        if p != col:
            aug[[col, p]] = aug[[p, col]]
        aug[col] = aug[col] * (1.0 / aug[col, col])
        f = aug[:, col].copy()
        f[col] = 0.0
        aug -= f[:, None] * aug[col][None, :]
    fm.update(ns=ns, slot=slot, slot_of=slot_of, ent=ent, UtZ=UtZ, cap=cap,
              inv=aug[:, ns:].copy(), ok=ok)
    return fm


def cp_cyc_apply_model(lay: FeLayout, tab: CpTables, fm: dict, Bm: np.ndarray, R: np.ndarray,
                       cell_h: np.ndarray) -> np.ndarray:
    """:func:`cp_apply_model` on the factors of :func:`cp_cyc_factor_model`: per column
    ``fe_cp_solve``'s corrected solve ``x = S_g^-1 (g - U w)``, ``w = inv (C U^T x_g)``, and
    one refinement of the grounded solve, in the kernels' order --

    * the forward sweep and the node sweep as on a forest: ``x_g``;
    * k_cp_b_cyc_w: ``y = C U^T x_g`` over the slot entry tables, ``w = inv y`` with a row's
      sum in ``CP_CYC_PARTS`` strided parts joined in part order;
    * k_cp_b_cyc_rhs: the node right-hand side (b rows plus ge in list order) minus ``U w``;
    * the node sweep on it; k_cp_b_cyc_res: its node residual against ``S_g``; the node sweep
      on the residual; k_cp_b_cyc_add; k_cp_b_back.

    Elementwise over the columns. Without chords (``fm["ns"] == 0``) it is
    :func:`cp_apply_model`, bit for bit."""
    if not fm.get("ns"):
        return cp_apply_model(lay, tab, fm, Bm, R, cell_h)
    Bm = np.ascontiguousarray(Bm, dtype=np.float64)
    nc = Bm.shape[0]
    Se, inv, slot, ent = fm["Se"], fm["inv"], fm["slot"], fm["ent"]
    ns = fm["ns"]
    n = tab.n_nodes
    inc = tab.inc.reshape(-1, 2)
    par = tab.parent.reshape(-1, 3)
    nrow = tab.nrow.reshape(-1, 2)
    z, ge = _cp_fwd_model(lay, tab, fm, Bm, R, cell_h)
    g = _cp_node_rhs_model(tab, Bm, ge)
    xg = _cp_sweep_model(tab, fm, g)
    y = np.zeros((ns, nc))
    for r, sl in enumerate(slot):
        v = np.zeros(nc)
        for e, end, op, om in ent[r]:
            cp, cm = _cp_cyc_coef(Se, e, end, sl & 1)
            on = slot[op] >> 1
            v = v + cp * xg[on, 0]
            if om >= 0:
                v = v + cm * xg[on, 1]
        y[r] = v
    w = None
    for q in range(CP_CYC_PARTS):
        s = np.zeros((ns, nc))
        for j in range(q, ns, CP_CYC_PARTS):
            s = s + inv[:, j][:, None] * y[j][None, :]
        w = s if w is None else w + s
    g2 = g.copy()
    for j, sl in enumerate(slot):
        g2[sl >> 1, sl & 1] = g2[sl >> 1, sl & 1] - w[j]
    xn = _cp_sweep_model(tab, fm, g2)
    rho = np.zeros_like(g2)
    for nd in range(n):
        D = [0.0] * 4
        for j in range(tab.inc_off[nd], tab.inc_off[nd + 1]):
            e, end = inc[j]
            Bk = _cp_blk(Se, e, end, end)
            for q in range(4):
                D[q] += Bk[q]
        x0, x1 = xn[nd, 0], xn[nd, 1]
        g0 = g2[nd, 0] - (D[0] * x0 + D[1] * x1)
        g1 = g2[nd, 1] - (D[2] * x0 + D[3] * x1)
        if par[nd, 0] >= 0:
            Bk = _cp_blk(Se, par[nd, 1], par[nd, 2], 1 - par[nd, 2])
            xp = xn[par[nd, 0]]
            g0 = g0 - (Bk[0] * xp[0] + Bk[1] * xp[1])
            g1 = g1 - (Bk[2] * xp[0] + Bk[3] * xp[1])
        for j in range(tab.child_off[nd], tab.child_off[nd + 1]):
            c = tab.child[j]
            Bk = _cp_blk(Se, par[c, 1], par[c, 2], 1 - par[c, 2])
            g0 = g0 - (Bk[0] * xn[c, 0] + Bk[2] * xn[c, 1])
            g1 = g1 - (Bk[1] * xn[c, 0] + Bk[3] * xn[c, 1])
        rho[nd, 0] = g0
        rho[nd, 1] = g1 if nrow[nd, 1] >= 0 else 0.0
    xn = xn + _cp_sweep_model(tab, fm, rho)
    return _cp_back_model(lay, tab, fm, Bm, R, cell_h, z, xn)


def cp_edge_form_model(lay: FeLayout, tab: CpTables, x: np.ndarray, mu: np.ndarray,
                       cell_h: np.ndarray):
    """numpy restatement of ``k_cp_b_edge_form`` (``nx_cp_batch_gradient``'s contraction) from
    the tables the device gets: ``x`` the forward and ``mu`` the adjoint column (device rows);
    returns ``(gR (E,), gf (E,), gbc (E, 2))`` with, per edge over its cells c,

    * ``gR[e] = -sum_c h_c mu_c^T M x_c`` -- the cell's k + 1 flux nodes, local rows
      ``k c .. k c + k``; ``M`` the reference mass behind ``Fh`` in ``tab.cst``;
    * ``gf[e] = sum_c h_c sum_i s_i mu[p_ci]`` -- the cell's m + 1 pressure rows (the first of
      cell 0 and the last of cell N - 1 are the end nodes' rows ``nrow[u, 0]`` / ``nrow[v, 0]``),
      ``s`` the source weights behind ``M``;
    * ``gbc[e] = mu`` at the edge's first and last flux row.

    Sums in the kernel's order per cell (j inside i, from 0.0); the cells are added in order
    where the kernel adds them by a butterfly, so the two agree to rounding, not in bits."""
    N, k, m, nI, E = lay.N, lay.k, lay.m, tab.nI, lay.E
    nq = k + 1
    nf = k * N + 1
    per = nf + m * N - 1
    off = 16 + 8 * nI + nI * nI
    M = np.asarray(tab.cst[off:off + nq * nq], dtype=np.float64).reshape(nq, nq)
    s = np.asarray(tab.cst[off + nq * nq:off + nq * nq + m + 1], dtype=np.float64)
    eb = tab.eb.reshape(-1, 4)
    nrow = tab.nrow.reshape(-1, 2)
    h = np.asarray(cell_h, dtype=np.float64).reshape(E, N)
    x = np.asarray(x, dtype=np.float64)
    mu = np.asarray(mu, dtype=np.float64)
    gR, gf, gbc = np.zeros(E), np.zeros(E), np.zeros((E, 2))
    for e in range(E):
        base = e * per
        aR = af = 0.0
        for c in range(N):
            t = 0.0
            for i in range(nq):
                sm = 0.0
                for j in range(nq):
                    sm += float(M[i, j]) * float(x[base + k * c + j])
                t += float(mu[base + k * c + i]) * sm
            aR += float(h[e, c]) * t
            g = 0.0
            for i in range(m + 1):
                pos = m * c + i
                row = (nrow[eb[e, 0], 0] if pos == 0 else nrow[eb[e, 1], 0] if pos == m * N
                       else base + nf + pos - 1)
                g += float(s[i]) * float(mu[row])
            af += float(h[e, c]) * g
        gR[e], gf[e] = -aR, af
        gbc[e] = mu[base], mu[base + k * N]
    return gR, gf, gbc
