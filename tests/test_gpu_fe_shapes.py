"""The degree-k batched paths on forests that are not binary (tests/tree_shapes.py):
``Solver(asm, batch_degrees=True).solve_many`` / ``.gradient`` (``nx_fe_batch_solve``,
``nx_fe_batch_gradient``, ``k_fe_b_edge_form``) at degrees (2, 0) and (3, 0), and
``Solver(asm, batch_continuous=True).gradient`` (``nx_cp_batch_gradient``, ``k_cp_b_edge_form``)
at (2, 1) and (3, 2). The binary trees, the chain and the graphs with cycles of
tests/test_gpu_fe_batch.py, tests/test_gpu_fe_gradient.py and tests/test_gpu_cp_gradient.py leave
every node of the continuous-pressure node forest inside its record and every slot of the
auxiliary P1/DG0 decomposition inside the binary paths; here

====================  =========================================================================
hub3                  a node record exactly full (4 incident edges, 3 children)
hub5                  past both record caps (the lists); a slot with 5 > kWaveKids children, in
                      a job at ``target_jobs`` 1, in the top part at the default 256
hub70 (N = 2)         71 incident edges at one node; 71 slots, 70 of them on one level
broom33               34 multiplier rows at one junction, no junction child, 34 > kPre entries
cat70                 69 > kCapLvl levels (job levels at ``target_jobs`` 1, top levels at 256);
                      23 side edges pointing INTO the spine
hubhub5x5             the seeded R and f; 25 leaf edges pointing into junctions below a hub of
                      hubs
rand200_s1            the seeded R and f; 68 of 199 edges point into their parent, 56 of them
                      at junctions of degree 3 to 19; 13 nodes past the record caps
====================  =========================================================================

each fact asserted from the host tables in the test that relies on it (``shape_facts``: the node
records from ``layout_fe.build_cp_tables``, the auxiliary decomposition ``asm._fe_aux_pc``, the
edges pointing into their parent from the mesh), so that a change of the generators or the caps
cannot empty a case. N is the shape's, capped at 6.

Set-up: tests/test_gpu_fe_gradient.py's and tests/test_gpu_cp_gradient.py's ``Setup`` with the
shapes' branch of tests/test_gpu_gradient.py -- ``p_xy``, no colour strategy, the shape's own
coefficients (``tree_shapes.coefficients``: the seeded R = 10^U(-1, 1) and f = 0.1 + 0.02 (e mod
5) on hubhub5x5 and rand200_s1, else R = 1); the observed rows drawn from every kind of row as
there. The auxiliary decomposition is steered from Python: ``assembly.build_tree_preconditioner``
is patched to another ``target_jobs`` while the assembler is built (hub5 and cat70 at 1).

Yardsticks. Solves: the oracle's sparse LU, PER BLOCK (fluxes, pressures, multipliers:
``tree_shapes.block_errors_oracle``) at the project's 1e-10, the reported residual <= 1e-12.
Gradients: the CPU adjoint of tests/gradient_ref_fe.py, held to central finite differences on
hubs, brooms, side edges pointing into a spine and the seeded R in
tests/test_gradient_ref_fe.py / tests/test_gradient_ref_cp.py; the numpy restatements of the two
contractions are held to it on these very shapes in tests/test_fe_gradient_host.py /
tests/test_cp_gradient_host.py, so a failure here is the device's.

The gradient bars: max(the binary trees' PARITY_BAR, 10 x the worst figure measured on an MI355X
over the cases below), never above 1e-8; any formula, sign or row-map error is O(1). Measured
worst figure per case (both kinds, all scenarios and quantities):
(k, 0), k = 2 / 3 -- hub3 4.3e-15 / 7.8e-15, hub5 2.7e-15 / 5.6e-15, hub70 8.0e-15 / 1.9e-14,
broom33 7.2e-15 / 7.1e-15, cat70 4.7e-13 / 5.7e-13, hubhub5x5 3.9e-15 / 5.0e-14, rand200_s1
7.5e-15 / 1.9e-14: FE_SHAPES_MEASURED = 5.699e-13 (cat70, k = 3), so the bar is 5.7e-12 -- the
binary trees' 5.2e-12 is 9.1 x this figure, just short of the 10 x margin;
(k, m), (2, 1) / (3, 2) -- hub3 2.5e-14 / 3.7e-14, hub5 1.3e-14 / 2.7e-14, hub70 2.1e-14 /
1.4e-14, broom33 4.1e-15 / 7.9e-15, cat70 1.01e-12 / 9.1e-13, hubhub5x5 7.1e-14 / 7.8e-14,
rand200_s1 2.4e-13 / 6.5e-13: CP_SHAPES_MEASURED = 1.011e-12 (cat70, (2, 1)), so the bar stays the
binary trees' 1.1e-10. No case is near 1e-9 and no call took a refinement pass
(``info["refined"] == 0`` everywhere); the two-decade R costs nothing, the 70-edge spine two
digits, as on the P1 paths. ``solve_many``, worst block error over all columns (always the
fluxes): hubs and brooms <= 1.3e-14 (hub70 k = 3), cat70 2.9e-13 at either decomposition,
hubhub5x5 1.1e-14, rand200_s1 5.0e-14; first-pass residual <= 6.6e-14.

Records and lists (``NXHIP_CP_NOREC=1``: every node reads the lists). Read from csrc/nxhip.hip:
a record holds its node's incident edges and children in the lists' order (``nx_fe_set_cp``
copies ``inc`` / ``child`` entry by entry), ``cp_node_up`` / ``cp_b_node_up`` add the edges'
blocks and subtract the children's terms in that order on either path, and a child's term is
formed by the same expressions with contraction off whether the child stores it (``cp_up_term``,
records) or the parent forms it (``cp_up_child_v``, lists). The two runs therefore give the same
bits -- on hub3, where no node is past the caps (every node changes path), and on hub5 and
broom33, where the hub reads the lists either way: asserted as bit equality."""

from __future__ import annotations

import numpy as np
import pytest

import test_gpu_cp_gradient as CP
import test_gpu_fe_gradient as FE
from gradient_ref_fe import objective
from networks_fenicsx_amd import Solver
from networks_fenicsx_amd import assembly as assembly_module
from networks_fenicsx_amd.layout_fe import build_cp_tables
from test_gpu_batch import N_SCEN, scenarios
from test_gpu_gradient import assert_same_bits, env
from tree_shapes import (FE_GRADIENT_SHAPES, FE_N_CAP, K_CAP_LVL, K_CP_REC_CH, K_CP_REC_INC,
                         K_PRE, K_WAVE_KIDS, K_WAVE_SLOTS, SHAPES, block_errors_oracle,
                         check_cp_records, decomposition_facts, reversed_edges)

pytestmark = pytest.mark.gpu

SOL_TOL = 1e-10  # per block
ZERO = 4  # the all-zero column of test_gpu_batch.scenarios
# One pass of the batched direct solve, no refinement pass: a residual above ksp_rtol after the
# first pass starts one, and one refinement pass heals a forward sweep that drops a term at a
# single node exactly (the error operator is then nilpotent) -- at the default 1e-12 such a
# defect would pass every bar below. The first pass leaves <= 6.6e-14 on these shapes (measured
# on an MI355X; tests/test_gpu_cp_batch.py keeps the pass out of its launch counts the same way).
ONE_PASS = {"ksp_rtol": 1e-9}
FE_SHAPES_MEASURED = 5.699e-13  # the largest error over test_fe_gradient_on_shapes' cases
CP_SHAPES_MEASURED = 1.011e-12  # the largest error over test_cp_gradient_on_shapes' cases
FE_BAR = max(FE.PARITY_BAR, 10 * FE_SHAPES_MEASURED)
CP_BAR = max(CP.PARITY_BAR, 10 * CP_SHAPES_MEASURED)
assert 10 * FE_SHAPES_MEASURED <= FE_BAR <= 1e-8
assert 10 * CP_SHAPES_MEASURED <= CP_BAR <= 1e-8

assert FE_GRADIENT_SHAPES == ["hub3", "hub5", "hub70", "broom33", "cat70", "hubhub5x5",
                              "rand200_s1"]
SEEDED = ("hubhub5x5", "rand200_s1")
JOBS_ONE = ("hub5", "cat70")  # also at target_jobs = 1: the hub and the spine inside one job
# edges pointing into their parent: (all, those at junctions, the largest such junction)
REVERSED = {"cat70": (23, 23, 3), "hubhub5x5": (25, 25, 3), "rand200_s1": (68, 56, 19)}


def shape_facts(s, name, pc=None, jobs=256, cp=False):
    """Assert what ``name`` is in this module for (the table of the docstring) on the set-up
    ``s``: N, the coefficients, the edges pointing into their parent; with ``pc`` the auxiliary
    P1/DG0 decomposition built at ``target_jobs = jobs``; with ``cp`` the node records."""
    mesh = s.mesh
    assert mesh.N == min(SHAPES[name][1], FE_N_CAP) <= 6 and mesh.num_edges <= 210
    if name in SEEDED:  # two decades of R
        assert s.R.max() / s.R.min() > 30.0
    else:
        assert (s.R == 1.0).all()
    rev = reversed_edges(*mesh.edges, mesh.degrees)
    at = rev[rev >= 3]
    assert (rev.size, at.size, int(at.max()) if at.size else 0) == REVERSED.get(name, (0, 0, 0))
    if pc is not None:
        f = decomposition_facts(pc)
        one = jobs == 1  # the whole forest one job, no top part; else the junctions on top
        assert (f["top_slots"] == 0) == one and (f["job_slots"] == 0) != one, f
        kids = f["job_kids"] if one else f["top_top_kids"]
        entries = f["job_entries"] if one else f["top_entries"]
        slots = f["job_slots"] if one else f["top_slots"]
        levels = f["job_levels"] if one else f["top_levels"]
        if name == "hub3":  # inside the binary paths, its entries exactly kPre
            assert kids == 3 < K_WAVE_KIDS + 1 and entries == K_PRE
        elif name == "hub5":
            assert kids == 5 > K_WAVE_KIDS and entries == 6 > K_PRE
        elif name == "hub70":
            assert kids == 70 > K_WAVE_KIDS and slots == 71 > K_WAVE_SLOTS and levels == 2
        elif name == "broom33":
            assert kids == 0 and slots == 1 and entries == 34 > K_PRE
            assert int(np.max(mesh.degrees)) == 34  # the junction's multiplier rows
        elif name == "cat70":
            assert levels == 69 > K_CAP_LVL and slots == 69 > K_WAVE_SLOTS
        elif name == "hubhub5x5":
            assert kids == 5 > K_WAVE_KIDS and slots == 31 and levels == 3
        else:
            assert name == "rand200_s1" and kids >= 13 and entries >= 19 and slots == 78
    if cp:
        rec = check_cp_records(name, build_cp_tables(s.asm.fe_layout, *mesh.edges))
        if name == "hub70":
            assert rec["inc"] == 71 > K_CP_REC_INC and rec["ch"] == 70 > K_CP_REC_CH
        if name in SEEDED:
            assert rec["over"] == {"hubhub5x5": 6, "rand200_s1": 13}[name]


class FeSetup(FE.Setup):
    """tests/test_gpu_fe_gradient.py's set-up on a shape; ``jobs``: the ``target_jobs`` of the
    auxiliary P1/DG0 handle's decomposition (the assembler's own call asks for 256)."""

    def __init__(self, name, k, jobs=256):
        assert name in SHAPES
        build = assembly_module.build_tree_preconditioner
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(assembly_module, "build_tree_preconditioner",
                       lambda *a, **kw: build(*a, **{**kw, "target_jobs": jobs}))
            super().__init__(name, k)
        assert self.asm.fe_direct_available
        shape_facts(self, name, pc=self.asm._fe_aux_pc, jobs=jobs)


class CpSetup(CP.Setup):
    """tests/test_gpu_cp_gradient.py's set-up on a shape."""

    def __init__(self, name, km):
        assert name in SHAPES
        super().__init__(name, km)
        assert self.asm.fe_direct_available
        shape_facts(self, name, cp=True)


# a ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("name", FE_GRADIENT_SHAPES)
def test_fe_batch_columns_on_shapes(name, k):
    """``solve_many`` at (k, 0): the seven scenarios of tests/test_gpu_fe_batch.py; every column
    batched, none fallen back; flux, pressure and multiplier blocks separately within 1e-10 of
    the oracle's LU; the reported residual <= 1e-12; the zero column exactly zero; column 5
    bit-equal to the same scenario in a batch of one; the same blocks in ONE pass (``ONE_PASS``:
    no refinement pass that could heal a sweep). hub5 and cat70 also with the auxiliary
    decomposition at ``target_jobs`` 1 (the default is 256)."""
    for jobs in ((256, 1) if name in JOBS_ONE else (256,)):
        s = FeSetup(name, k, jobs)
        try:
            items, nodal, f = scenarios(s.mesh, s.pbc)
            solver = Solver(s.asm, batch_degrees=True)
            res = solver.solve_many(items, f)
            print(f"{name} k={k} j{jobs}: {res.info}")
            once = Solver(s.asm, batch_degrees=True, petsc_options=ONE_PASS).solve_many(items, f)
            assert once.info["refined"] == 0, once.info
            ref = FE.cpu_adjoint(s)
            worst = 0.0
            for r in (res, once):
                assert r.path == "batched" and r.info["chunk"] == N_SCEN
                assert r.info["fallback"] == 0
                for j in range(N_SCEN):
                    if j == ZERO:
                        assert not r.x[j].any() and r.residual_norms[j] == 0.0
                        assert r.converged[j]
                        continue
                    x_ref = ref.solve(nodal[j], f[j])
                    assert np.linalg.norm(x_ref) > 0
                    err = block_errors_oracle(r.x[j], x_ref, s.F.p_offset, s.F.lm_offset)
                    print(f"{name} k={k} j{jobs} column {j}: blocks q/p/lm "
                          + " ".join(f"{e:.2e}" for e in err)
                          + f", relres {r.residual_norms[j]:.2e}, passes {r.iterations[j]}")
                    worst = max(worst, *err)
                    assert max(err) <= SOL_TOL, (j, err)
                    assert r.converged[j]
                    if r is res:
                        assert r.residual_norms[j] <= 1e-12, j
            print(f"SOLVE {name} k={k} j{jobs}: worst block error {worst:.3e}")
            with env(NXHIP_BATCH=1):
                one = solver.solve_many([items[5]], f[5:6])
            assert one.path == "batched" and one.info["chunk"] == 1
            np.testing.assert_array_equal(one.x[0], res.x[5])
            assert one.residual_norms[0] == res.residual_norms[5]
        finally:
            s.close()


# b, c ------------------------------------------------------------------------------------
def _gradients(s, opt, mod, tag):
    """Both kinds on the set-up's three scenarios, at the default tolerance and in ONE pass
    (``ONE_PASS``: a refinement pass would heal a sweep that drops a term): converged, none
    fallen back, the shapes; the worst error of value, dR, df, dp_bc over all of them
    (``parity_errors``: no quantity skipped, no reference norm zero); returns it with the two
    results of the default tolerance."""
    worst, out = 0.0, []
    for once in (False, True):
        solver = Solver(s.asm, petsc_options=ONE_PASS if once else None, **opt)
        for kind, data in (("linear", None), ("lsq", s.data)):
            g = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=data)
            assert g.converged.all() and g.info["fallback"] == 0
            assert not once or g.info["refined"] == 0, g.info
            assert g.value.shape == (3,) and g.dR.shape == (3, s.mesh.num_edges)
            assert g.df.shape == g.dR.shape and g.dp_bc.shape == (3, s.mesh.num_nodes)
            worst = max(worst, mod.worst_error(s, g, data, tag=kind + " one pass" * once))
            if not once:
                out.append(g)
    print(f"SHAPES {tag}: worst {worst:.3e}")
    return worst, out


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("name", FE_GRADIENT_SHAPES)
def test_fe_gradient_on_shapes(name, k):
    """``gradient`` at (k, 0) against the CPU adjoint: value, dR, df and dp_bc of three
    scenarios, both kinds of objective, as relative 2-norms under FE_BAR."""
    s = FeSetup(name, k)
    try:
        worst, _ = _gradients(s, {"batch_degrees": True}, FE, f"{name} k={k}")
        assert worst <= FE_BAR, worst
    finally:
        s.close()


@pytest.mark.parametrize("km", [(2, 1), (3, 2)])
@pytest.mark.parametrize("name", FE_GRADIENT_SHAPES)
def test_cp_gradient_on_shapes(name, km, monkeypatch):
    """``gradient`` at (k, m) against the CPU adjoint, the same assertions under CP_BAR. hub3,
    hub5 and broom33 also without node records (``NXHIP_CP_NOREC=1``, read when the tables are
    attached): the same bits as the default run (the module's docstring says why)."""
    monkeypatch.delenv("NXHIP_CP_NOREC", raising=False)
    s = CpSetup(name, km)
    try:
        worst, got = _gradients(s, {"batch_continuous": True}, CP, f"{name} {km}")
        assert worst <= CP_BAR, worst
    finally:
        s.close()
    if name not in ("hub3", "hub5", "broom33"):
        return
    monkeypatch.setenv("NXHIP_CP_NOREC", "1")
    s = CpSetup(name, km)
    try:
        worst, lists = _gradients(s, {"batch_continuous": True}, CP, f"{name} {km} lists")
        assert worst <= CP_BAR, worst
        for a, b in zip(lists, got):
            assert_same_bits(a, b, slice(None), slice(None))
    finally:
        s.close()


# d ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,km", [("cat70", (2, 0)), ("cat70", (3, 2)),
                                     ("rand200_s1", (3, 0)), ("rand200_s1", (2, 1))])
def test_gradient_value_is_solve_many_objective_on_shapes(name, km):
    """``value`` against the objective evaluated on the host from ``solve_many``'s columns of
    the same solver, 1e-12 relative (the same forward columns; one sum in another order), both
    kinds; ``dp_bc`` exactly zero at every node that is not a boundary node."""
    if km[1] == 0:
        s, opt = FeSetup(name, km[0]), {"batch_degrees": True}
    else:
        s, opt = CpSetup(name, km), {"batch_continuous": True}
    try:
        solver = Solver(s.asm, **opt)
        res = solver.solve_many(s.items, s.f)
        assert res.path == "batched" and res.info["fallback"] == 0
        inner = np.asarray(s.mesh.degrees) > 1
        assert inner.any() and not inner.all()
        for data in (None, s.data):
            g = solver.gradient(s.items, s.f, rows=s.rows, weights=s.w, data=data)
            assert g.converged.all() and g.info["fallback"] == 0
            for j in range(3):
                J = objective(res.x[j], s.rows, s.w, None if data is None else data[j])
                err = abs(g.value[j] - J) / abs(J)
                print(f"{name} {km} {'linear' if data is None else 'lsq'} scenario {j}: {err:.2e}")
                assert abs(J) > 0 and err <= 1e-12, (j, err)
            assert not g.dp_bc[:, inner].any()
            assert g.dp_bc[:, ~inner].any(axis=1).all()
    finally:
        s.close()


# e ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,km", [("hub5", (3, 2)), ("cat70", (2, 0))])
def test_batch_independence_on_shapes(name, km):
    """Scenario 2 alone (``NXHIP_BATCH=1``), in its batch of 3 and in the reversed batch: the
    same bits, both kinds."""
    if km[1] == 0:
        s, opt = FeSetup(name, km[0]), {"batch_degrees": True}
    else:
        s, opt = CpSetup(name, km), {"batch_continuous": True}
    try:
        solver = Solver(s.asm, **opt)
        kw = dict(rows=s.rows, weights=s.w)
        for lsq in (False, True):
            three = solver.gradient(s.items, s.f, data=s.data if lsq else None, **kw)
            back = solver.gradient(s.items[::-1], s.f[::-1].copy(),
                                   data=s.data[::-1].copy() if lsq else None, **kw)
            with env(NXHIP_BATCH=1):
                alone = solver.gradient(s.items[2:3], s.f[2:3],
                                        data=s.data[2:3] if lsq else None, **kw)
            assert alone.info["chunk"] == 1 and three.info["chunk"] == 3
            assert back.info["chunk"] == 3
            assert_same_bits(alone, three, 0, 2)
            assert_same_bits(alone, back, 0, 0)
            assert_same_bits(back, three, slice(None), slice(None, None, -1))
            assert alone.dR.any() and alone.df.any() and alone.dp_bc.any()
    finally:
        s.close()
