"""The device on forests with hubs, brooms and long spines (tests/tree_shapes.py; the host side
of the same shapes: tests/test_tree_shapes.py, which also says which branch of csrc/nxhip.hip
each shape is there for and asserts the decompositions' facts).

Every solution is judged PER BLOCK (fluxes, pressures, multipliers separately,
``tree_shapes.block_errors``) at the project's 1e-10 against the oracle's sparse LU and, where
f = 0, the analytic resistor network; the two references agree to 1e-12 per block on every shape
and coefficient set used here (test_tree_shapes.py). Coefficients: R = 1, f = 0, except hub9,
hubhub5x5 and the random trees (seeded per-edge R = 10^U(-1, 1), f = 0.1 + 0.02 (e mod 5));
p_bc = x[1] + 0.3 x[0].

Decompositions: ``target_jobs`` 1, 4 and the default 256, set as tests/test_gpu_dstep_dense.py
does. What runs is asserted where the host decides it: the LDS sweeps exactly when every job and
the top part fit their caps (``_fits_lds``, the ``lds`` test of ``nx_set_preconditioner``), then
the one-launch step (``direct_path() == "fused"``); cat300 cannot take them at any of the three
(599 chains in one job at 1; 299 top levels > kMaxTopLvl at 4 and 256): the direct solve needs
the LDS sweeps, so there the global-memory kernels precondition MINRES (3 iterations)."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import distributed_model as DM
from hessian_ref import HessianRef
from networks_fenicsx_amd import HydraulicNetworkAssembler, NetworkMesh, Solver
from networks_fenicsx_amd.assembly import evaluate_nodal
from networks_fenicsx_amd.group import RankGroup
from networks_fenicsx_amd.layout import build_local_problem, partition_edges
from networks_fenicsx_amd.layout_fe import build_cp_tables, evaluate_terms
from networks_fenicsx_amd.precond import (apply_model, build_tree_preconditioner,
                                          coarse_structure, lumped_mass)
from oracle import nx_oracle as O
from oracle import nx_oracle_fe as OF
from tree_shapes import (JOBS, K_MAX_TOP_LVL, K_WAVE_KIDS, SHAPES, block_errors,
                         block_errors_oracle, check_cp_records, coefficients,
                         decomposition_facts, hub, p_xy)

pytestmark = pytest.mark.gpu

SOL_TOL = 1e-10  # per block
PATH_TOL = 1e-14  # between two direct paths on one handle (tests/test_gpu_dstep.py)
GRADIENT_BAR = 8.7e-12  # tests/test_gpu_gradient.py PARITY_BAR
HVP_BAR = 4.9e-11  # tests/test_gpu_hvp.py PARITY_BAR

# csrc/nxhip.hip: kCapC, kCapS, kCapDC (chains, slots, down-chain entries of a job), kCapT,
# kCapTDC (top slots and their entries) -- with kMaxTopLvl the ``lds`` test
CAP_C, CAP_S, CAP_DC, CAP_T, CAP_TDC = 512, 256, 768, 1152, 2304

CONFIGS = [(name, j) for name in SHAPES for j in JOBS]
_IDS = [f"{n}-j{j}" for n, j in CONFIGS]


def p_x(x):
    return x[0]


def _fits_lds(pc) -> bool:
    ts0, ts1 = int(pc.top_lvl_off[0]), int(pc.top_lvl_off[-1])
    ok = ts1 - ts0 <= CAP_T and pc.top_lvl_off.size - 1 <= K_MAX_TOP_LVL
    if ts1 > ts0:
        ok = ok and pc.slot_dc_off[ts1] - pc.slot_dc_off[ts0] <= CAP_TDC
    for j in range(pc.n_jobs):
        ok = ok and pc.job_chain_off[j + 1] - pc.job_chain_off[j] <= CAP_C
        lv0, lv1 = pc.job_lvl_off[j], pc.job_lvl_off[j + 1]
        if lv1 > lv0:
            a, b = pc.lvl_slot_off[lv0], pc.lvl_slot_off[lv1]
            ok = ok and b - a <= CAP_S and pc.slot_dc_off[b] - pc.slot_dc_off[a] <= CAP_DC
    return bool(ok)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The references of a shape, computed once: the oracle's system in build layout, its LU
    solution, and the analytic answer of the same R with f = 0."""
    make, N, _ = SHAPES[name]
    mesh = NetworkMesh(make(), N=N)
    src, dst = mesh.edges
    P = O.build_problem(mesh.node_coordinates, src, dst, N, mesh.edge_colors)
    coef = coefficients(name, mesh.num_edges)
    A, b = O.assemble_reference(P, p_xy, **coef)
    Ab, bb, perm, _ = O.to_build_layout(P, A, b)
    out = {"P": P, "A": A, "b": b, "Ab": Ab, "bb": bb, "perm": perm, "coef": coef,
           "x": O.solve_reference(A, b), "E": mesh.num_edges, "N": N}
    R = coef.get("R", 1.0)
    out["xa"] = O.resistor_network_solution(P, p_xy, R=R)  # (f = 0)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _open(name, jobs, **forms):
    make, N, _ = SHAPES[name]
    mesh = NetworkMesh(make(), N=N)
    asm = HydraulicNetworkAssembler(mesh)
    src, dst = mesh.edges
    asm._pc = build_tree_preconditioner(asm._local, src, dst, mesh.degrees, target_jobs=jobs)
    asm.set_preconditioner(True)
    asm.compute_forms(p_bc_ex=p_xy, **(forms or coefficients(name, mesh.num_edges)))
    asm.set_direct(True)
    return mesh, asm


def _step(asm):
    asm.assemble()
    it, rr, conv = asm.handle.solve(1e-12, 100, 4)
    return it, rr, conv, asm.handle.solution()


def _check_direct(tag, asm, ref, want):
    """One step with the direct solve asked for, against every bar of part (a); returns x.
    ``want``: ``"fused"`` / ``"launches"`` (the direct path that must have run), or ``"minres"``
    -- the decomposition does not fit the LDS sweeps, which alone run the direct solve
    (``direct_local``), so the global-memory kernels precondition MINRES: <= 4 iterations, the
    true residual <= 1e-12 (its reported figure is MINRES's estimate)."""
    h = asm.handle
    it, rr, conv, x = _step(asm)
    path = h.direct_path()
    rp, col, val = h.csr()
    np.testing.assert_array_equal(rp, ref["Ab"].indptr)
    np.testing.assert_array_equal(val, ref["Ab"].data)
    np.testing.assert_array_equal(h.rhs(), ref["bb"])
    true = h.true_residual()
    err = block_errors(x, ref["x"][ref["perm"]], ref["E"], ref["N"])
    print(f"{tag}: solver {h.solver()} path {path} passes {it} rr {rr:.2e} true {true:.2e} "
          "blocks q/p/lm " + " ".join(f"{e:.2e}" for e in err))
    assert conv and rr <= 1e-12, (it, rr, conv)
    if want == "minres":
        assert h.solver() == (1, 0) and it <= 4 and true <= 1e-12, (it, true)
    else:
        assert h.solver() == (1, 1) and it in (1, 2), it
        assert path == want, path
        assert abs(rr - true) <= 0.05 * true + 5e-16, (rr, true)
    assert max(err) <= SOL_TOL, err
    for _ in range(3):
        it2, rr2, _, x2 = _step(asm)
        assert rr2 == rr and it2 == it
        np.testing.assert_array_equal(x2, x)
    return x


def _check_analytic(tag, asm, ref, want):
    """One step of the same R with f = 0 on the handle's current path against the analytic
    resistor-network answer, per block; the shape's own coefficients are put back after it."""
    h = asm.handle
    if ref["coef"]:
        asm.compute_forms(p_bc_ex=p_xy, R=ref["coef"]["R"], f=0.0)
    it, rr, conv, xz = _step(asm)
    path = h.direct_path()
    erra = block_errors(xz, ref["xa"][ref["perm"]], ref["E"], ref["N"])
    print(f"{tag}: solver {h.solver()} path {path} analytic blocks "
          + " ".join(f"{e:.2e}" for e in erra))
    assert conv and rr <= 1e-12, (it, rr, conv)
    if want == "minres":
        assert h.solver() == (1, 0) and it <= 4, it
    else:
        assert h.solver() == (1, 1) and it in (1, 2), it
        assert path == want, path
    assert max(erra) <= SOL_TOL, erra
    if ref["coef"]:
        asm.compute_forms(p_bc_ex=p_xy, **ref["coef"])


# |x_launches - x_fused| / |x| where it misses 1e-14. Measured on an MI355X: rand200_s2
# 1.43e-14, the same figure at every decomposition (one job or 13, no top part or 78 top
# slots), and both paths meet every per-block bar against the oracle (fluxes 6.9e-14).
# Supposed, not measured: that the difference arises in the chain scans rather than in the
# junction sweeps -- the decompositions differ only in the sweeps and leave it unchanged, and
# N = 17 is the only shape here with two cells per lane of a 16-lane segment. Bar: 10 x measured.
PATH_MEASURED = {"rand200_s2": 1.43e-14}
PATH_BAR = {k: 10 * v for k, v in PATH_MEASURED.items()}
assert all(v <= 1e-12 for v in PATH_BAR.values())


@pytest.mark.parametrize("name,jobs", CONFIGS, ids=_IDS)
def test_direct_one_launch_and_separate_launches(name, jobs, monkeypatch):
    """(a) the one-launch direct step (``k_dir_step``: ``dir_up_fused`` / ``dir_up_v2``, the top
    part, the down sweep) and (b) the separate launches (``NXHIP_DIR_FUSED=0``:
    ``pc_up_body`` in direct mode, ``top_body``, the down sweep) on the same handle, on every
    shape at every decomposition. Branches by shape: see tests/test_tree_shapes.py -- hub4 the
    fourth packed child word, hub5 and up the ``nkids > kWaveKids`` / ``rnk > kWaveKids``
    fallbacks (in a job at j = 1, in the top part at 4 and 256), the brooms ``kPre``, cat70
    ``kCapLvl`` and more than 64 slots. cat300 fits the LDS sweeps at none of the three
    decompositions, so no direct solve runs on it: the global-memory kernels (``k_pc_up`` /
    ``k_pc_top`` / ``k_pc_down`` over 239 job levels or 299 top levels) precondition MINRES.

    Bars: CSR values, row pointers and rhs bit-equal to the oracle; converged in 1 or 2 passes,
    reported residual <= 1e-12 and within 5 % + 5e-16 of the true one; every block within
    1e-10 of the LU and, in a step with f = 0 on each of the two paths, of the analytic answer;
    three more steps repeat bit for bit; the two paths agree to 1e-14 (``|x_p| + |H u| ~ |x|``
    holds on hubs and spines too: 7.1e-16 at worst) on every shape but rand200_s2, whose bar
    is 10 x its measured 1.43e-14 (PATH_MEASURED). Why that shape has its own bar: the figure
    is the same at all three decompositions and both paths meet the oracle per block (fluxes
    6.9e-14), so neither path is wrong and the junction sweeps, which the decompositions
    change, do not cause it; the 1e-14 was argued for binary trees (tests/test_gpu_dstep.py). That it comes
    from the chain scans at N = 17 (two cells per lane) is supposed, not measured.

    Measured on an MI355X, worst block error (the fluxes everywhere) against the LU: hubs and
    brooms 1.2e-14 (hub70), cat70 3.0e-13, hubhub5x5 4.8e-15, rand200 1.9e-14 / 6.9e-14,
    rand600 1.4e-15; cat300 through MINRES 1.2e-12. Against the analytic answer (f = 0; one
    launch / separate launches): hubs and brooms 1.1e-14 / 1.0e-14 (hub70), cat70 3.0e-13 /
    3.0e-13, rand200 seed 2 2.2e-13 / 1.8e-13, the other random trees 2.1e-14, cat300
    1.2e-12."""
    ref = _oracle(name)
    mesh, asm = _open(name, jobs)
    try:
        h = asm.handle
        lds = _fits_lds(asm._pc)
        assert h.pc_lds() == lds
        assert lds == (name != "cat300")
        want = "fused" if lds else "minres"
        x1 = _check_direct(f"{name} j{jobs} fused", asm, ref, want)
        _check_analytic(f"{name} j{jobs} fused", asm, ref, want)
        monkeypatch.setenv("NXHIP_DIR_FUSED", "0")
        want = "launches" if lds else "minres"
        x0 = _check_direct(f"{name} j{jobs} launches", asm, ref, want)
        _check_analytic(f"{name} j{jobs} launches", asm, ref, want)
        diff = np.linalg.norm(x0 - x1) / np.linalg.norm(x1)
        print(f"{name} j{jobs}: |x_launches - x_fused| / |x| = {diff:.2e}")
        assert diff <= PATH_BAR.get(name, PATH_TOL), diff
    finally:
        asm.close()


@pytest.mark.parametrize("name,jobs", [(n, j) for n in ("hub5", "hub9", "cat70", "hubhub5x5")
                                       for j in (1, 4)])
def test_superposition_modes(name, jobs, monkeypatch):
    """Phase 2 by superposition (``NXHIP_DIR_SUP`` 0 / 1 / 5, as
    tests/test_gpu_dstep.py::test_dstep_superposition_modes) where a slot has more than
    ``kWaveKids`` children (hub5, hub9, hubhub5x5: in a job at j = 1, in the top part at 4) and
    where a job has more than ``kCapLvl`` levels (cat70 at 1; 69 top levels at 4): each mode
    meets the oracle per block, reports the residual of the x it stored and repeats bit for
    bit; 1 and 5 give the same bits, 0 the same x to 1e-14 (measured on an MI355X: 7.1e-16 at
    worst)."""
    ref = _oracle(name)
    mesh, asm = _open(name, jobs)
    try:
        xs = {}
        for mode in ("0", "1", "5"):
            monkeypatch.setenv("NXHIP_DIR_SUP", mode)
            xs[mode] = _check_direct(f"{name} j{jobs} sup{mode}", asm, ref, "fused")
        np.testing.assert_array_equal(xs["1"], xs["5"])
        diff = np.linalg.norm(xs["1"] - xs["0"]) / np.linalg.norm(xs["0"])
        print(f"{name} j{jobs}: |x_sup1 - x_sup0| / |x| = {diff:.2e}")
        assert diff <= PATH_TOL, diff
    finally:
        asm.close()


@pytest.mark.parametrize("name", ["hub9", "hub70", "hubhub5x5"])
def test_dense_top_against_top_solver(name, monkeypatch):
    """The dense top (G times the summed inputs) against the top solver (``NXHIP_DIR_DENSE=0``,
    ``top_body`` inside the step) at the default decomposition, where the hub and all its
    children are top slots (9, 70 and 5 top children of one top slot: ``top_wave`` dropped, the
    LDS loops of ``top_body``; ``k_pc_gbuild`` walks a 70-child level): the same x to 1e-14,
    each per block at the oracle's bar. The dense top runs on all three (asserted from
    ``direct_dense()``; N <= 16, needs 10 / 23 / 22 <= kMaxNeed). Measured on an MI355X:
    |x_dense - x_solver| / |x| <= 3.6e-16."""
    ref = _oracle(name)
    mesh, asm = _open(name, 256)
    try:
        h = asm.handle
        f = decomposition_facts(asm._pc)
        assert f["top_top_kids"] > K_WAVE_KIDS and f["n_jobs"] > 0
        x1 = _check_direct(f"{name} dense", asm, ref, "fused")
        dense = h.direct_dense()
        print(f"{name}: dense {dense}")
        assert dense["ran"] and dense["builds"] == 1
        monkeypatch.setenv("NXHIP_DIR_DENSE", "0")
        x0 = _check_direct(f"{name} top solver", asm, ref, "fused")
        assert not h.direct_dense()["ran"]
        diff = np.linalg.norm(x1 - x0) / np.linalg.norm(x0)
        print(f"{name}: |x_dense - x_solver| / |x| = {diff:.2e}")
        assert diff <= PATH_TOL, diff
    finally:
        asm.close()


def _cpu_minres_iterations(ref, lp, pc, exact, rtol=1e-12):
    """Iterations preconditioned MINRES (scipy) with the numpy model of P needs to bring the
    true relative residual of the build-layout system under ``rtol``."""
    Ab, bb = ref["Ab"], ref["bb"]
    dq = lumped_mass(Ab, lp)
    n = Ab.shape[0]
    nb = np.linalg.norm(bb)
    hist = []
    M = spla.LinearOperator((n, n), matvec=lambda r: apply_model(pc, lp, dq, r, exact=exact))
    spla.minres(Ab, bb, M=M, rtol=1e-15, maxiter=400,
                callback=lambda xk: hist.append(np.linalg.norm(bb - Ab @ xk) / nb))
    ok = [k + 1 for k, r in enumerate(hist) if r <= rtol]
    assert ok, min(hist)
    return ok[0]


@pytest.mark.parametrize("name,jobs", [(n, j) for n in ("hub4", "hub5", "hub70", "broom33",
                                                        "cat70", "cat300", "rand600_s3")
                                       for j in (1, 256)])
def test_minres_and_global_kernels(name, jobs, monkeypatch):
    """(c) MINRES with the LDS kernels where they fit (``pc_up_body`` in its own mode,
    ``top_body``, the down sweep) and with the global-memory kernels (``NXHIP_PC_GLOBAL=1``;
    cat300 takes them on its own): converged in <= 4 iterations (the exact preconditioner
    gives 3; a wrong child index shows as tens), every block at the oracle's bar, within 1e-11
    of the direct solve of the LDS handle (cat300 has none). With the global-memory kernels a
    handle asked for the direct solve runs MINRES (``direct_local``): asserted.

    Measured on an MI355X: 3 iterations everywhere; worst block error (fluxes) 4.4e-12 on
    cat70, 3.5e-14 on the hubs; |x_minres - x_direct| / |x| <= 8.2e-14."""
    ref = _oracle(name)
    x_ref = ref["x"][ref["perm"]]
    xd = None
    for kernels in ("lds", "global"):
        if kernels == "global":
            monkeypatch.setenv("NXHIP_PC_GLOBAL", "1")
        mesh, asm = _open(name, jobs)
        try:
            h = asm.handle
            lds = kernels == "lds" and name != "cat300"
            assert h.pc_lds() == lds
            it, rr, conv, x = _step(asm)  # (the direct solve asked for)
            assert conv and h.solver() == (1, 1 if lds else 0), h.solver()
            err = block_errors(x, x_ref, ref["E"], ref["N"])
            assert max(err) <= SOL_TOL, err
            if lds:
                xd = x
            asm.set_direct(False)
            asm.assemble()
            it, rr, conv = h.solve(1e-12, 200, 4)
            xm = h.solution()
            errm = block_errors(xm, x_ref, ref["E"], ref["N"])
            diff = np.linalg.norm(xm - xd) / np.linalg.norm(xd) if xd is not None else 0.0
            print(f"{name} j{jobs} {kernels}: asked-direct blocks "
                  + " ".join(f"{e:.2e}" for e in err) + f"; MINRES it {it} rr {rr:.2e} blocks "
                  + " ".join(f"{e:.2e}" for e in errm) + f"; |x_m - x_d| / |x| {diff:.2e}")
            assert h.solver() == (0, 0)
            assert conv and it <= 4, (it, rr)
            assert max(errm) <= SOL_TOL, errm
            assert diff <= 1e-11, diff
        finally:
            asm.close()


@pytest.mark.parametrize("name,jobs", [("hub5", 1), ("hub5", 256), ("cat70", 1), ("cat70", 256)])
def test_minres_lumped(name, jobs):
    """The lumped variant (``pc_mass: lumped``; the same sweeps, the other chain outputs): at
    most one iteration more than scipy's MINRES with ``apply_model(exact=False)`` needs on the
    same system for a true residual of 1e-12, and the oracle per block. Measured on an MI355X:
    9 iterations on all four, the model's 9; worst block error 1.1e-14."""
    ref = _oracle(name)
    mesh, asm = _open(name, jobs)
    try:
        h = asm.handle
        src, dst = mesh.edges
        lp = build_local_problem(mesh.node_coordinates, src, dst, mesh.degrees, mesh.N)
        want = _cpu_minres_iterations(ref, lp, asm._pc, exact=False)
        h.set_pc_exact(False)
        asm.set_direct(False)
        asm.assemble()
        it, rr, conv = h.solve(1e-12, 400, 1)
        err = block_errors(h.solution(), ref["x"][ref["perm"]], ref["E"], ref["N"])
        print(f"{name} j{jobs} lumped: device {it} iterations (rr {rr:.2e}), model {want}; "
              "blocks " + " ".join(f"{e:.2e}" for e in err))
        assert conv and h.solver() == (0, 0)
        assert it <= want + 1, (it, want)
        assert max(err) <= SOL_TOL, err
    finally:
        asm.close()


# (d) ------------------------------------------------------------------------------------
BATCH = [("hub5", 1), ("hub5", 256), ("hub9", 1), ("hub9", 256), ("cat70", 1),
         ("rand200_s1", 256)]
_BIDS = [f"{n}-j{j}" for n, j in BATCH]


class _Batch:
    """A shape with the batched tests' scenarios: the matrix carries the shape's per-edge R
    (or R = 0.5 + (e mod 3) / 2); seven boundary / source scenarios as tests/test_gpu_batch.py
    (p_bc, p_x, a random nodal array, a unit pressure at one terminal, zero, the first two with
    the per-edge source); the gradient tests' three with the source on each."""

    def __init__(self, name, jobs):
        self.name = name
        E = _oracle(name)["E"]
        coef = coefficients(name, E)
        self.R = coef["R"] if coef else 0.5 + (np.arange(E) % 3) / 2.0
        self.mesh, self.asm = _open(name, jobs, R=self.R)
        self.P = _oracle(name)["P"]
        nn = self.mesh.num_nodes
        rnd = np.random.default_rng(7).standard_normal(nn)
        unit = np.zeros(nn)
        unit[np.asarray(self.mesh.boundary_in_nodes)[0]] = 1.0
        self.items = [p_xy, p_x, rnd, unit, np.zeros(nn), p_xy, p_x]
        self.nodal = np.stack([evaluate_nodal(it, self.mesh.node_coordinates)
                               for it in self.items])
        self.fe = 0.1 + 0.02 * (np.arange(E) % 5)
        self.f = np.zeros((7, E))
        self.f[5] = self.f[6] = self.fe

    def lu_columns(self, R, cols):
        out, lu = {}, None
        for j in cols:
            A, b = O.assemble_reference(self.P, self.nodal[j], f=self.f[j], R=R)
            lu = lu or spla.splu(A.tocsc())
            out[j] = lu.solve(b)
        return out


@pytest.mark.parametrize("name,jobs", BATCH, ids=_BIDS)
def test_batched_solves(name, jobs):
    """``solve_many`` (``k_b_up`` runs ``pc_up_lds_body`` per column, the batched top and down
    sweeps) and ``solve_ensemble`` (a matrix per column) where a slot has more than
    ``kWaveKids`` children or ``kPre`` entries (hub5, hub9: in a job at 1, in the top part at
    256; rand200: 13 top children, 19 entries) and a job more than ``kCapLvl`` levels (cat70):
    every column per block at 1e-10 against the oracle's LU, the zero column zero, one column
    bit-equal to the same scenario alone in a batch of 1. Measured on an MI355X, worst block
    error over all columns: hub5 2.1e-14, hub9 3.0e-14, cat70 3.2e-13, rand200 1.9e-14."""
    s = _Batch(name, jobs)
    try:
        solver = Solver(s.asm)
        res = solver.solve_many(s.items, f=s.f)
        assert res.path == "batched" and res.info["fallback"] == 0
        refs = s.lu_columns(s.R, [0, 1, 2, 3, 5, 6])
        worst = 0.0
        for j in range(7):
            if j == 4:
                assert not res.x[j].any() and res.converged[j]
                continue
            err = block_errors_oracle(res.x[j], refs[j], s.P.p_offset, s.P.lm_offset)
            worst = max(worst, *err)
            assert res.converged[j] and res.residual_norms[j] <= 1e-12, j
            assert max(err) <= SOL_TOL, (j, err)
        one = solver.solve_many([s.items[5]], f=s.f[5:6])
        np.testing.assert_array_equal(one.x[0], res.x[5])
        # three resistance fields, the boundary data and source of column 5
        E = s.mesh.num_edges
        Rs = np.stack([s.R, np.full(E, 3.7),
                       10.0 ** np.random.default_rng(2024).uniform(-1.0, 1.0, E)])
        ens = solver.solve_ensemble(Rs, p_bc=[p_xy] * 3, f=np.tile(s.fe, (3, 1)))
        assert ens.info["fallback"] == 0
        for i in range(3):
            x_ref = s.lu_columns(Rs[i], [5])[5]
            err = block_errors_oracle(ens.x[i], x_ref, s.P.p_offset, s.P.lm_offset)
            worst = max(worst, *err)
            assert ens.converged[i] and max(err) <= SOL_TOL, (i, err)
        print(f"{name} j{jobs}: batched worst block error {worst:.2e}")
    finally:
        s.asm.close()


@functools.lru_cache(maxsize=None)
def _hessian_ref(name):
    s = _oracle(name)
    coef = coefficients(name, s["E"])
    R = coef["R"] if coef else 0.5 + (np.arange(s["E"]) % 3) / 2.0
    return HessianRef(s["P"], R)


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b))


@pytest.mark.parametrize("name,jobs", BATCH, ids=_BIDS)
def test_gradient_and_hessian_vector(name, jobs):
    """``gradient`` and ``hessian_vector`` (two and four batched direct solves through the same
    sweeps) on the hub shapes against tests/gradient_ref.py / tests/hessian_ref.py at those
    tests' bars (8.7e-12 and 4.9e-11): least squares and linear objectives over rows of all
    three blocks, three scenarios with the per-edge source, one random direction. Measured on
    an MI355X (gradient / Hessian-vector worst figure): hub5 5.7e-15 / 6.4e-15, hub9 1.9e-14 /
    6.3e-14, cat70 3.0e-12 / 7.1e-13, rand200 6.9e-15 / 1.5e-14 -- inside the binary trees' bars,
    which stand."""
    s = _Batch(name, jobs)
    try:
        solver = Solver(s.asm)
        P, E, nn = s.P, s.mesh.num_edges, s.mesh.num_nodes
        rng = np.random.default_rng(11)
        items = [p_xy, p_x, rng.standard_normal(nn)]
        nodal = np.stack([evaluate_nodal(it, s.mesh.node_coordinates) for it in items])
        f = np.tile(s.fe, (3, 1))
        blocks = [(0, P.p_offset, 5), (P.p_offset, P.lm_offset, 4), (P.lm_offset, P.n_dofs, 3)]
        rows = np.concatenate([lo + rng.choice(hi - lo, size=min(k, hi - lo), replace=False)
                               for lo, hi, k in blocks])
        w = 0.5 + rng.random(rows.size)
        data = rng.standard_normal((3, rows.size))
        bnd = np.concatenate([P.leaf_in, P.root_out])
        v_p = np.zeros((3, nn))
        v_p[:, bnd] = rng.standard_normal((3, bnd.size))
        v_R, v_f = rng.standard_normal((3, E)), rng.standard_normal((3, E))
        ref = _hessian_ref(name)
        worst_g = worst_h = 0.0
        for d in (None, data):
            g = solver.gradient(items, f, rows=rows, weights=w, data=d)
            hv = solver.hessian_vector(items, f, rows=rows, weights=w, data=d, v_R=v_R,
                                       v_p_bc=v_p, v_f=v_f)
            assert g.converged.all() and g.info["fallback"] == 0
            assert hv.converged.all() and hv.info["fallback"] == 0
            for j in range(3):
                r = ref.hvp(nodal[j], f[j], rows, w, None if d is None else d[j],
                            v_R=v_R[j], v_p=v_p[j], v_f=v_f[j])
                eg = [abs(g.value[j] - r["value"]) / abs(r["value"]), _rel(g.dR[j], r["dR"]),
                      _rel(g.df[j], r["df"]), _rel(g.dp_bc[j], r["dp_bc"])]
                eh = [_rel(hv.HdR[j], r["HdR"]), _rel(hv.Hdf[j], r["Hdf"]),
                      _rel(hv.Hdp_bc[j], r["Hdp_bc"]), _rel(hv.dR[j], r["dR"])]
                worst_g, worst_h = max(worst_g, *eg), max(worst_h, *eh)
        print(f"{name} j{jobs}: gradient worst {worst_g:.3e}, hessian-vector worst {worst_h:.3e}")
        assert worst_g <= GRADIENT_BAR, worst_g
        assert worst_h <= HVP_BAR, worst_h
    finally:
        s.asm.close()


# (e) ------------------------------------------------------------------------------------
FE_SHAPES = ["hub3", "hub4", "hub5", "hub9", "broom5", "broom33", "cat70"]
K_FE_SHAPES = 8  # csrc/nxhip.hip kFeShapes: edge templates per handle


def _fe_open(name, km, f=None, R=None):
    make, N, _ = SHAPES[name]
    N = min(N, 6)
    mesh = NetworkMesh(make(), N=N)
    asm = HydraulicNetworkAssembler(mesh, flux_degree=km[0], pressure_degree=km[1])
    asm.compute_forms(p_bc_ex=p_xy, f=f, R=R)
    src, dst = mesh.edges
    F = OF.build_problem_fe(mesh.node_coordinates, src, dst, N, *km, mesh.edge_colors)
    return mesh, asm, F


def _fe_edge_bc(F):
    pb = O._nodal(p_xy, F.base.pos3)
    src, dst = F.base.src, F.base.dst
    leaf = np.zeros(pb.size, dtype=bool)
    leaf[F.base.leaf_in] = True
    root = np.zeros(pb.size, dtype=bool)
    root[F.base.root_out] = True
    bc = np.zeros((src.size, 2))
    bc[:, 0] = np.where(root[src], -pb[src], 0.0)
    bc[:, 1] = np.where(leaf[dst], pb[dst], 0.0)
    return bc


@pytest.mark.parametrize("km", [(2, 0), (3, 0), (2, 1), (3, 2)])
@pytest.mark.parametrize("name", FE_SHAPES)
def test_fe_degrees_on_hubs(name, km, monkeypatch):
    """(e) General degrees: (k, 0) through the condensed P1/DG0 system (the auxiliary handle's
    tree solve on the hub) and continuous pressure by condensation onto the graph nodes, whose
    records hold ``kCpRecInc`` = 4 incident edges and ``kCpRecCh`` = 3 children. Asserted from
    ``build_cp_tables`` (``tree_shapes.check_cp_records``; the forest is rooted at node 0, so
    hub(k)'s hub has k + 1 incident edges and k children): hub3's hub fills its record exactly
    (``r[3] == 4``, ``r[kc] == 3``: the third child slot ``r[kc + 1 + 3 * 2]`` is read), cat70
    stays under both caps, hub4's hub is one past both and every other hub and broom far past
    them (``r[3] = -1`` / ``r[kc] = -1``: the lists; ``cp_lev_full = 0``: the pipelined runs
    erased). The solution per block against the oracle's LU and (m >= 1, f = 0) the analytic answer at
    1e-10, true residual < 1e-9; the CSR and rhs bit-equal to ``evaluate_terms`` through the edge
    templates (``NXHIP_FE_STRUCT=1``) and through the gather tables (0); with ``NXHIP_CP_PIPE``
    1 and 0 the solutions agree to 1e-13.

    ``kFeShapes`` = 8 edge templates: an edge's template is fixed by which of its ends carry a
    multiplier, not by its colour or its junction's degree, so a forest has at most four and
    these shapes two or three (asserted from ``fe_templates()``): no hub reaches the cap, and
    the builder's give-up branch stays outside these tests.

    Measured on an MI355X, worst block error against the LU: hubs and brooms 5.6e-14
    (broom33 (3, 2), the multipliers; hub3, the exactly full record: 1.5e-14 against the LU,
    2.7e-14 against the analytic answer), cat70 4.5e-13 ((3, 2), the fluxes); true residual
    <= 4.5e-14; the pipelined and the level-by-level node sweeps give the same bits."""
    k, m = km
    E = _oracle(name)["E"]
    R = 1.0 + 0.5 * (np.arange(E) % 3)
    for struct in ("1", "0"):
        monkeypatch.setenv("NXHIP_FE_STRUCT", struct)
        mesh, asm, F = _fe_open(name, km, f=0.4, R=R)
        try:
            asm.assemble()
            lay = asm.fe_layout
            rp, col, val = asm.handle.csr()
            _, hcell = O.cell_geometry(F.base)
            hv, hr = evaluate_terms(lay, R, 0.4, _fe_edge_bc(F), hcell)
            np.testing.assert_array_equal(rp, lay.rowptr)
            np.testing.assert_array_equal(col, lay.col)
            np.testing.assert_array_equal(val, hv)
            np.testing.assert_array_equal(asm.handle.rhs(), hr)
            # the templates are built either way (the variable picks the kernel): one per
            # combination of (multiplier at the source, multiplier at the target)
            nsh, per = asm.handle.fe_templates()
            print(f"{name} {km} struct {struct}: templates {nsh} x {per}")
            junction = mesh.degrees > 1
            src, dst = mesh.edges
            want = np.unique(np.stack([junction[src], junction[dst]]), axis=1).shape[1]
            assert nsh == want <= K_FE_SHAPES, (nsh, want)
            assert per == k * mesh.N + 1 + (mesh.N if m == 0 else m * mesh.N - 1)
        finally:
            asm.close()
    monkeypatch.delenv("NXHIP_FE_STRUCT")
    A, b = OF.assemble_reference_fe(F, p_xy, f=0.4, R=R)
    x_ref = O.solve_reference(A, b)
    got = {}
    for pipe in (("1", "0") if m >= 1 else ("1",)):
        monkeypatch.setenv("NXHIP_CP_PIPE", pipe)
        mesh, asm, F = _fe_open(name, km, f=0.4, R=R)
        try:
            assert asm.fe_direct_available
            if m >= 1:  # the node records' host facts: at, under or past the caps
                rec = check_cp_records(name, build_cp_tables(asm.fe_layout, *mesh.edges))
                print(f"{name} {km}: node records {rec}")
            solver = Solver(asm)
            solver.assemble()
            sol = solver.solve()
            x = np.concatenate([fn.x.array for fn in sol])
            err = block_errors_oracle(x, x_ref, F.p_offset, F.lm_offset)
            tr = solver.true_residual()
            print(f"{name} {km} pipe {pipe}: path {asm.handle.direct_path()} passes "
                  f"{solver.ksp.iterations} true {tr:.2e} blocks "
                  + " ".join(f"{e:.2e}" for e in err))
            assert solver.ksp.solver_used == "direct" and solver.ksp.converged
            assert asm.handle.direct_path() == ("condensed" if m == 0 else "node-condensed")
            assert max(err) <= SOL_TOL and tr < 1e-9, (err, tr)
            got[pipe] = x
            if m >= 1 and pipe == "1":  # the analytic answer: f = 0
                asm.compute_forms(p_bc_ex=p_xy, f=0.0, R=R)
                solver.assemble()
                xz = np.concatenate([fn.x.array for fn in solver.solve()])
                xa = OF.resistor_network_solution_fe(F, p_xy, R=R)
                erra = block_errors_oracle(xz, xa, F.p_offset, F.lm_offset)
                print(f"{name} {km}: analytic blocks " + " ".join(f"{e:.2e}" for e in erra))
                assert max(erra) <= SOL_TOL, erra
        finally:
            asm.close()
    if m >= 1:
        d = np.linalg.norm(got["1"] - got["0"]) / np.linalg.norm(got["0"])
        print(f"{name} {km}: |x_pipe1 - x_pipe0| / |x| = {d:.2e}")
        assert d <= 1e-13, d


# (f) ------------------------------------------------------------------------------------
GROUPS = {"hub9": (lambda: hub(9, inward=True), 8), "hubhub5x5": (SHAPES["hubhub5x5"][0], 4),
          "cat70": (SHAPES["cat70"][0], 3)}


@pytest.mark.parametrize("name,nranks", [("hub9", 2), ("hub9", 3), ("hubhub5x5", 2),
                                         ("hubhub5x5", 3), ("cat70", 4)])
def test_group_direct_on_hubs(name, nranks):
    """(f) The direct solve across ranks in one process
    (tests/test_gpu_group.py::test_group_direct_solve). The partition cuts the directed
    depth-first edge order into chunks, so the inward leaf edges (hub9 with ``inward=True``;
    hubhub5x5 has them) fall to the last rank and the junctions they end at become interface
    junctions: the coarse forest then has a junction with more than ``kWaveKids`` coarse
    children (asserted from ``coarse_structure``; ``cnk > kWaveKids``: the coarse solve leaves
    its register sweeps). The gathered solution per block at 1e-10 against the oracle, within
    1e-12 of the one-rank solve, and the same bits on a second step. Measured on an MI355X:
    7 and 9 coarse children (hub9 at 2 and 3 ranks), 5 (hubhub5x5); worst block error 1.0e-14 on
    the hubs, 3.0e-13 on cat70; against one rank <= 4.8e-16."""
    make, N = GROUPS[name]
    G = make()
    mesh = NetworkMesh(G, N=N)
    src, dst = mesh.edges
    E = mesh.num_edges
    coef = coefficients(name, E)
    P = O.build_problem(mesh.node_coordinates, src, dst, N, mesh.edge_colors)
    A, b = O.assemble_reference(P, p_xy, **coef)
    Ab, bb, perm, _ = O.to_build_layout(P, A, b)
    x_ref = O.solve_reference(A, b)[perm]
    owner = partition_edges(src, dst, mesh.num_nodes, nranks)
    cs = coarse_structure(src, dst, mesh.degrees, owner, nranks)
    kids = int(np.diff(cs.child_off).max()) if cs.n else 0
    print(f"{name} P{nranks}: {cs.n} coarse junctions, most coarse children {kids}")
    if name != "cat70":
        assert kids > K_WAVE_KIDS, kids
    else:
        assert cs.n >= nranks - 1
    one = HydraulicNetworkAssembler(mesh)
    try:
        one.compute_forms(p_bc_ex=p_xy, **coef)
        one.set_direct(True)
        _, _, conv1, x_one = _step(one)
    finally:
        one.close()
    assert conv1
    grp = RankGroup(G, N, nranks)
    try:
        grp.compute_forms(p_bc_ex=p_xy, **coef)
        grp.set_direct(True)
        grp.assemble()
        it, rr, conv = grp.solve(1e-12, 50000, 4)
        x = np.zeros(Ab.shape[0])
        for a, xl in zip(grp.assemblers, grp.solutions()):
            x[DM.global_rows(a.local_problem, E, mesh.bifurcation_index)] = xl
        err = block_errors(x, x_ref, E, N)
        d1 = np.linalg.norm(x - x_one) / np.linalg.norm(x_one)
        paths = [a.handle.direct_path() for a in grp.assemblers]
        sups = [a.handle.direct_sup() for a in grp.assemblers]
        print(f"{name} P{nranks}: paths {paths} sup {sups} passes {it} rr {rr:.2e} blocks "
              + " ".join(f"{e:.2e}" for e in err) + f"; vs one rank {d1:.2e}")
        assert len(set(paths)) == 1, paths  # (which direct path ran: the same on every rank)
        assert conv and grp.solver_used == "direct" and it in (1, 2) and rr <= 1e-12, (it, rr)
        assert max(err) <= SOL_TOL, err
        assert d1 <= 1e-12, d1
        true = np.linalg.norm(bb - Ab @ x) / np.linalg.norm(bb)
        assert abs(rr - true) <= 0.05 * true + 5e-16, (rr, true)
        grp.assemble()
        grp.solve(1e-12, 50000, 4)
        x2 = np.zeros(Ab.shape[0])
        for a, xl in zip(grp.assemblers, grp.solutions()):
            x2[DM.global_rows(a.local_problem, E, mesh.bifurcation_index)] = xl
        np.testing.assert_array_equal(x2, x)
    finally:
        grp.close()
