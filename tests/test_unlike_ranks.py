"""Unlike ranks on the host (tests/unlike_ranks.py): every configuration's per-rank
decompositions hold the facts they are in the suite for, and the numpy model of the multi-rank
direct solve is right on the MIXED decompositions, so that tests/test_gpu_unlike_ranks.py judges
the device alone.

What the facts decide in csrc/nxhip.hip: a rank with a job of more than G = kPcThreads / W
chains (128 at W = 8) has ``dstep_multi`` and cannot take the superposition instantiation
(``dir_args`` clears ``DirStep::sup``); the group's one launch takes it only if every rank can
(``launch_xr_wc``), a rank's own launch decides for itself."""

from __future__ import annotations

import numpy as np
import pytest

import distributed_model as DM
from networks_fenicsx_amd.layout import build_local_problem
from networks_fenicsx_amd.precond import (build_tree_preconditioner, lumped_mass,
                                          pc_finish_model, pc_up_model)
from tree_shapes import block_errors, decomposition_facts
from unlike_ranks import (CAP_C, CAP_S, CAP_T, CONFIGS, GROUP_SUP, K_MAX_NEED, RANK_SUP,
                          host_ranks, lane_shape, mesh_of, oracle, pass_chains)


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_configurations_hold_their_facts(cid):
    graph, N, jobs, chains = CONFIGS[cid]
    lps, pcs = host_ranks(cid)
    facts = [decomposition_facts(pc) for pc in pcs]
    print(cid, [{k: f[k] for k in ("n_jobs", "chains", "job_slots", "top_slots", "need")}
                for f in facts])
    assert all(pc.tree_exact for pc in pcs)
    assert tuple(f["chains"] for f in facts) == chains
    # every cap of the LDS sweeps and of the exchange step; one workgroup per job, all ranks'
    # in one launch (xr_on: the jobs' sum <= the CU count, 256 on an MI355X): 86 on U3, at
    # most 65 on the others
    for f in facts:
        assert f["chains"] <= CAP_C and f["job_slots"] <= CAP_S and f["need"] <= K_MAX_NEED
        assert 1 <= f["top_slots"] <= CAP_T
    assert sum(f["n_jobs"] for f in facts) <= (86 if cid == "U3" else 65)
    G = pass_chains(N)
    assert G == 128
    multi = tuple(c > G for c in chains)
    W, CPL = lane_shape(N)
    # the superposition instantiation exists for CPL <= 2; a rank takes it without a
    # several-pass job (the park fits: about a thousand top slots would be needed to lose it)
    assert RANK_SUP[cid] == tuple(CPL <= 2 and not m for m in multi)
    assert GROUP_SUP[cid] == all(RANK_SUP[cid])
    if cid == "U1":
        assert multi == (False, True)
    elif cid == "U2":
        assert multi == (True, False)
    elif cid == "U3":
        assert multi == (False, True, False)
        mid = facts[1]
        assert (mid["n_jobs"], mid["job_slots"], mid["top_slots"], mid["need"]) == (1, 0, 90, 90)
        assert (facts[0]["n_jobs"], facts[2]["n_jobs"]) == (42, 43)
    elif cid == "U4":  # exactly one pass, and one chain under it
        assert chains == (G, G - 1) and multi == (False, False)
    elif cid == "U5":
        assert multi == (True, True)
    elif cid == "U6":
        assert (W, CPL) == (8, 3) and multi == (False, True)


@pytest.mark.parametrize("cid", ["U1", "U3", "U4"])
def test_model_on_mixed_decompositions(cid):
    """The numpy model of the multi-rank direct solve (every rank's ``pc_up_model``, the summed
    coarse partials, ``pc_finish_model``; three applications, as ``direct_multi`` of
    tests/test_precond.py) with every rank on its OWN decomposition, against the oracle's LU per
    block at 1e-10: the ranks' decompositions need not match for the coarse step to pair. U4's
    graph at N = 4 (its decompositions are N-independent; 128 / 127 chains asserted). Measured:
    fluxes 3.5e-13 (U3), 2.4e-13 (U4's graph at N = 4), 8.3e-12 (U1 at N = 15); pressures and
    multipliers <= 7e-15 -- the reference model alone stays inside the bar."""
    graph, N, jobs, chains = CONFIGS[cid]
    if cid == "U4":
        N = 4
        _, m = mesh_of(graph, N)
        src, dst = m.edges
        lps = [build_local_problem(m.node_coordinates, src, dst, m.degrees, N, r, len(jobs))
               for r in range(len(jobs))]
        pcs = [build_tree_preconditioner(lp, src, dst, m.degrees, target_jobs=j)
               for lp, j in zip(lps, jobs)]
        assert tuple(decomposition_facts(pc)["chains"] for pc in pcs) == chains
    else:
        _, m = mesh_of(graph, N)
        src, dst = m.edges
        lps, pcs = host_ranks(cid)
    ref = oracle(graph, N)
    Ab, bb = ref["Ab"], ref["bb"]
    E, bif = m.num_edges, m.bifurcation_index
    lp1 = build_local_problem(m.node_coordinates, src, dst, m.degrees, N)
    dq_global = lumped_mass(Ab, lp1)
    rows = [DM.global_rows(lp, E, bif) for lp in lps]

    def apply_all(r):  # P^{-1} over the ranks: sweeps, the partials summed, coarse forest
        sts = [pc_up_model(pc, lp, dq_global[lp.edges], r[rw])
               for lp, pc, rw in zip(lps, pcs, rows)]
        tot = sum(st["partial"] for st in sts)
        z = np.zeros_like(r)
        for lp, pc, rw, st in zip(lps, pcs, rows, sts):
            z[rw] = pc_finish_model(pc, lp, dq_global[lp.edges], st, tot)
        return z

    per = 2 * N + 1
    rid = np.arange(Ab.shape[0])
    flux = (rid < E * per) & (rid % per % 2 == 0)
    y = apply_all(np.where(flux, bb, 0.0))
    w = np.where(flux, 0.0, Ab @ np.where(flux, y, 0.0) - bb)
    xs = apply_all(w)
    t = np.where(flux, bb - Ab @ np.where(flux, 0.0, xs), 0.0)
    x = np.where(flux, apply_all(t), xs)
    err = block_errors(x, ref["x"], E, N)
    print(cid, "model on mixed decompositions, blocks q/p/lm", " ".join(f"{e:.2e}" for e in err))
    assert max(err) <= 1e-10, err
