"""Device MINRES solver for the hydraulic network system.

Mirrors ``Solver`` of the reference (``src/networks_fenicsx/solver.py:16-143``):
same constructor signature, ``assemble``, ``solve``, ``A``, ``b``, ``ksp`` and
``assembler`` accessors. The reference factorises the system with MUMPS
(``preonly`` + ``lu``, ``solver.py:58-65``). Here both KSP types run on the GPU
(``nx_solve`` in ``csrc/nxhip.hip``):

* ``ksp_type="preonly"`` (the reference default): a direct solve -- the block LU of the
  saddle-point system whose Schur complement the tree preconditioner inverts exactly
  (``nx_set_solver``), checked by the true residual. Used where it is exact: a tree, on one
  rank or on several (every rank's decomposition must run the LDS sweeps with the coarse
  step; the ranks decide together); otherwise, or with a residual above ``ksp_rtol`` after
  one refinement step, MINRES runs;
* ``ksp_type="minres"`` (or any other iterative type): preconditioned MINRES -- CSR SpMV,
  fused vector updates and deterministic reductions in HIP graphs.

PETSc options understood (with or without the options prefix):

``ksp_rtol``                      relative residual tolerance (default 1e-12, chosen so the
                                  solution matches a direct solve to <= 1e-10 rel. norm)
``ksp_max_it``                    iteration cap (default 50000)
``ksp_error_if_not_converged``    raise :class:`NxNotConverged` (default True)
``ksp_monitor``                   print iterations / residual after each solve
``ksp_check_every``               iterations per host convergence check (default 4 with the
                                  preconditioner -- the exact one converges in 3, + 1 launch for
                                  the last update -- and 32 for plain MINRES)

``pc_type``                       ``"none"`` runs plain MINRES; anything else (the reference's
                                  default ``"lu"`` included) uses the tree Schur-complement
                                  preconditioner (``precond.py``)
``pc_mass``                       ``"consistent"`` (default: exact Schur complement, 3 MINRES
                                  iterations) or ``"lumped"``

``ksp_type``                      ``"preonly"`` (default): the direct tree solve where exact,
                                  else MINRES; anything else: MINRES.
``pc_factor_mat_solver_type`` is accepted and recorded. ``ksp.solver_used`` tells which
solve ran last (``"direct"`` or ``"minres"``).
"""

from __future__ import annotations

import os
import sys
import typing

import numpy as np

from . import _lib
from .assembly import DeviceMatrix, DeviceVector, HydraulicNetworkAssembler
from .timing import timed

__all__ = ["Solver", "KSPInfo", "BatchResult", "GradientResult", "HessianVectorResult"]

_DEFAULTS = {
    "ksp_type": "preonly",
    "pc_type": "lu",
    "pc_factor_mat_solver_type": "mumps",
    "ksp_monitor": None,
    "ksp_error_if_not_converged": True,
}


class KSPInfo:
    """What ``solver.ksp`` exposes: options and the last solve's statistics."""

    def __init__(self, prefix: str, options: dict):
        self.prefix = prefix
        self.options = options
        self.iterations = 0
        self.residual_estimate = float("nan")
        self.converged = False
        self.solver_used = ""

    def getOptionsPrefix(self) -> str:  # noqa: N802
        return self.prefix

    def getIterationNumber(self) -> int:  # noqa: N802
        return self.iterations

    def getResidualNorm(self) -> float:  # noqa: N802
        return self.residual_estimate

    def getConvergedReason(self) -> int:  # noqa: N802
        return 2 if self.converged else -3  # KSP_CONVERGED_RTOL / KSP_DIVERGED_ITS

    def destroy(self) -> None:
        return None


# solve_many: a single scenario on more rows than this takes the sequential path
BATCH_SINGLE_MAX_ROWS = 1 << 18


class BatchResult:
    """What :meth:`Solver.solve_many` and :meth:`Solver.solve_ensemble` return.

    ``x``: ``(B, n)``, every row in the reference's block order -- the concatenated functions
    ``[flux_color_0 .., pressure, global_flux]`` that ``solve()`` returns;
    ``iterations``, ``residual_norms``, ``converged``: ``(B,)`` each; ``path``: ``"batched"``
    (``nx_batch_solve``) or ``"sequential"`` (the per-scenario loop); ``info``: the dict of
    ``nx_get_batch_info`` (launches, refined, fallback, chunk; for ``solve_ensemble``
    ``fallback`` counts the scenarios solved again by its sequential path)."""

    def __init__(self, assembler, x, iterations, residual_norms, converged, path, info):
        self._assembler = assembler
        self.x = x
        self.iterations = np.asarray(iterations)
        self.residual_norms = np.asarray(residual_norms)
        self.converged = np.asarray(converged, dtype=bool)
        self.path = path
        self.info = dict(info)

    def __len__(self) -> int:
        return self.x.shape[0]

    def functions(self, j: int) -> list:
        """The function list of scenario ``j`` (new functions, filled by
        ``scatter_solution``)."""
        from .fem import Function

        asm = self._assembler
        names = [f"flux_color_{i}" for i in range(len(asm.flux_spaces))]
        names += ["pressure", "global_flux"]
        fns = [Function(V, name=nm) for V, nm in zip(asm.function_spaces, names)]
        xdev = np.empty(self.x.shape[1], dtype=np.float64)  # block order -> device layout
        xdev[np.concatenate([asm._block_rows(i) for i in range(len(fns))])] = self.x[j]
        return asm.scatter_solution(xdev, fns)


class GradientResult:
    """What :meth:`Solver.gradient` returns: per scenario the objective and its derivatives.

    ``value``: ``(B,)``; ``dR``, ``df``: ``(B, num_edges)`` in ``graph.edges()`` order -- with
    respect to every edge's resistance and source; ``dp_bc``: ``(B, num_nodes)`` -- with respect
    to the nodal boundary pressure, zero off the boundary nodes; ``iterations``,
    ``residual_norms``, ``converged``: ``(B, 2)`` each, the forward and the adjoint solve;
    ``info``: the dict of ``nx_get_batch_info`` (launches, refined, fallback, chunk). With
    ``derivatives=False`` the derivatives are None and the three ``(B, 1)``: the forward solve."""

    def __init__(self, value, dR, df, dp_bc, iterations, residual_norms, converged, info):
        self.value = value
        self.dR = dR
        self.df = df
        self.dp_bc = dp_bc
        self.iterations = np.asarray(iterations)
        self.residual_norms = np.asarray(residual_norms)
        self.converged = np.asarray(converged, dtype=bool)
        self.info = dict(info)

    def __len__(self) -> int:
        return self.value.shape[0]


class HessianVectorResult:
    """What :meth:`Solver.hessian_vector` returns: per scenario the objective, its gradient
    and the product of its Hessian with the scenario's direction.

    ``value``, ``dR``, ``df``, ``dp_bc``: as :class:`GradientResult` (the three derivatives are
    None in Gauss-Newton mode); ``HdR``, ``Hdf``: ``(B, num_edges)`` in ``graph.edges()`` order
    and ``Hdp_bc``: ``(B, num_nodes)``, zero off the boundary nodes -- the blocks of ``H v``
    belonging to ``R``, ``f`` and the nodal boundary pressure; ``iterations``,
    ``residual_norms``, ``converged``: ``(B, 4)`` each -- the forward, adjoint, tangent and
    second-order adjoint solve -- or ``(B, 3)`` in Gauss-Newton mode (no adjoint); ``info``: the
    dict of ``nx_get_batch_info``."""

    def __init__(self, value, dR, df, dp_bc, HdR, Hdf, Hdp_bc, iterations, residual_norms,
                 converged, info):
        self.value = value
        self.dR = dR
        self.df = df
        self.dp_bc = dp_bc
        self.HdR = HdR
        self.Hdf = Hdf
        self.Hdp_bc = Hdp_bc
        self.iterations = np.asarray(iterations)
        self.residual_norms = np.asarray(residual_norms)
        self.converged = np.asarray(converged, dtype=bool)
        self.info = dict(info)

    def __len__(self) -> int:
        return self.value.shape[0]


def _truthy(v) -> bool:
    if v is None:
        return True  # PETSc flag options given as None mean "set"
    if isinstance(v, str):
        return v.strip().lower() not in ("0", "false", "no", "off")
    return bool(v)


class Solver:
    """GPU solver interface for the network problem.

    Args:
        assembler: the hydraulic network assembler
        petsc_options_prefix: options prefix (kept for API compatibility)
        petsc_options: dictionary of PETSc-style options (see module docstring)
        kind: matrix kind (None, "mpi" or "nest"); recorded, storage is device CSR
        ensemble_cycles: let :meth:`solve_ensemble`, :meth:`gradient` and
            :meth:`hessian_vector` with ``R=`` take the batched path on a graph with cycles
            (``nx_set_ensemble_cycles``: a cycle correction per scenario, up to 512 cycle
            chains). ``None`` reads ``NXHIP_ENS_CYCLES`` (``"1"`` on; off when unset). Off, these
            calls behave as before on such a graph: the per-scenario loop, or
            ``NotImplementedError``. The batched results agree with the one-matrix path to
            rounding, not bit for bit (the correction solves again instead of storing
            ``A_g^{-1} U``). Measured against the per-scenario loop: 1.5 to
            37 x faster at 240 to 506 cycle chains and B = 1 to 64, except B = 1 at 506 cycle
            chains, where the one-workgroup factorisation makes it 0.80 x the loop.
        batch_degrees: let :meth:`solve_many` (and ``terminal_conductance``) take the batched
            path for flux degree k >= 2 with DG0 pressure (``nx_fe_batch_solve``: the per-cell
            condensation, the auxiliary tree sweeps and the expansion with a column dimension).
            ``None`` reads ``NXHIP_FE_BATCH`` (``"1"`` on; off when unset). Off, these degrees
            take the per-scenario loop, whose columns are bit-equal to single solves; the
            batched columns agree with them to rounding. The option
            also lets :meth:`gradient` serve these degrees (``nx_fe_batch_gradient``, DESIGN.md
            section 3k); off, it raises ``NotImplementedError`` there.
        batch_continuous: let :meth:`solve_many` (and ``terminal_conductance``) take the
            batched path for continuous pressure (k > m >= 1) on a forest
            (``nx_cp_batch_solve``: the node-condensed direct solve factored once per call,
            its right-hand-side sweeps with a column dimension). ``None`` reads
            ``NXHIP_CP_BATCH`` (``"1"`` on; off when unset). Off -- and on a graph with cycles
            (``cycle_direct``), with several ranks or with ``ksp_type="minres"`` -- these
            degrees take the per-scenario loop, whose columns are bit-equal to single solves;
            the batched columns agree with them to rounding (with the
            measurements). The option also lets :meth:`gradient` serve these degrees on a
            forest (``nx_cp_batch_gradient``); off, it raises
            ``NotImplementedError`` there.
        batch_continuous_cycles: with ``batch_continuous`` and an assembler built with
            ``cycle_direct=True``, let :meth:`solve_many`, ``terminal_conductance`` and
            :meth:`gradient` take the batched path on a graph with cycles
            (``nx_set_cp_batch_cycles``: the single solve's chord correction per column, on
            the batch's own factors and its own capacitance inverse, built once per contents
            of ``R``; up to 4096 border slots at chord ends). ``None`` reads
            ``NXHIP_CP_BATCH_CYCLES`` (``"1"`` on; off when unset); an explicit ``False``
            overrides the environment. Alone -- without ``batch_continuous``, or on an
            assembler without ``cycle_direct`` -- it changes nothing; off, such a graph takes
            the per-scenario loop and :meth:`gradient` raises ``NotImplementedError``, as
            before. :meth:`hessian_vector`, ``R=`` ensembles, several ranks and
            ``ksp_type="minres"`` are not served on these degrees either way (DESIGN.md
            section 3m, with the measurements).
    """

    def __init__(
        self,
        assembler: HydraulicNetworkAssembler,
        petsc_options_prefix: str = "NetworkSolver_",
        petsc_options: dict | None = None,
        kind: str | typing.Sequence[typing.Sequence[str]] | None = None,
        *,
        ensemble_cycles: bool | None = None,
        batch_degrees: bool | None = None,
        batch_continuous: bool | None = None,
        batch_continuous_cycles: bool | None = None,
    ):
        self._assembler = assembler
        if batch_degrees is None:
            batch_degrees = os.environ.get("NXHIP_FE_BATCH", "") == "1"
        self._fe_batch = bool(batch_degrees)
        if batch_continuous is None:
            batch_continuous = os.environ.get("NXHIP_CP_BATCH", "") == "1"
        self._cp_batch = bool(batch_continuous)
        if batch_continuous_cycles is None:
            batch_continuous_cycles = os.environ.get("NXHIP_CP_BATCH_CYCLES", "") == "1"
        self._cp_batch_cycles = bool(batch_continuous_cycles)
        if ensemble_cycles is None:
            ensemble_cycles = os.environ.get("NXHIP_ENS_CYCLES", "") == "1"
        self._ens_cycles = bool(ensemble_cycles)
        opts = dict(_DEFAULTS if petsc_options is None else petsc_options)
        clean = {}
        for k, v in opts.items():
            key = k[len(petsc_options_prefix):] if k.startswith(petsc_options_prefix) else k
            clean[key.lstrip("-")] = v
        self._rtol = float(clean.get("ksp_rtol", 1e-12))
        self._maxit = int(clean.get("ksp_max_it", 50000))
        ce = clean.get("ksp_check_every")
        self._check_every = None if ce is None else int(ce)
        self._raise = _truthy(clean.get("ksp_error_if_not_converged", True))
        self._monitor = "ksp_monitor" in clean and _truthy(clean["ksp_monitor"])
        self._ksp = KSPInfo(petsc_options_prefix, clean)
        self._pc = str(clean.get("pc_type", "lu")).lower() != "none"
        self._pc_exact = str(clean.get("pc_mass", "consistent")).lower() != "lumped"
        self._direct = str(clean.get("ksp_type", "preonly")).lower() == "preonly"
        self._kind = kind
        self._A = DeviceMatrix(assembler.handle, kind)
        self._b = DeviceVector(assembler.handle)
        self._closed = False

    @property
    def assembler(self) -> HydraulicNetworkAssembler:
        return self._assembler

    @property
    def A(self) -> DeviceMatrix:  # noqa: N802
        return self._A

    @property
    def b(self) -> DeviceVector:
        return self._b

    @property
    def ksp(self) -> KSPInfo:
        return self._ksp

    @property
    def rtol(self) -> float:
        return self._rtol

    def assemble(self, lhs: bool = True, rhs: bool = True) -> None:
        """Assemble the system matrix and/or rhs (values are overwritten, not added)."""
        self.assembler.assemble(self._A, self._b, assemble_lhs=lhs, assemble_rhs=rhs)

    @timed("nxfx:Solver:solve")
    def solve(self, functions: list | None = None) -> list:
        """Solve on the device and return ``[flux_color_0.., pressure, global_flux]``
        (``solver.py:107-135``). One gather kernel snapshots the solution on the device in
        the functions' order; new functions read it -- one DMA into a pinned buffer for all
        of them -- when the first ``x.array`` is used, so later solves never change them
        (``HydraulicNetworkAssembler.solution_functions``). Given ``functions`` are filled
        at once."""
        if self._closed:
            raise RuntimeError("the solver has been destroyed")
        h = self.assembler.handle
        self._configure()
        ce = self._check_every or (4 if self.assembler.preconditioned else 32)
        it, relres, conv = h.solve(self._rtol, self._maxit, ce)
        self._ksp.iterations, self._ksp.residual_estimate, self._ksp.converged = it, relres, conv
        used = "direct" if h.solver()[1] == 1 else "minres"
        self._ksp.solver_used = used
        if self._monitor:
            what = ("direct tree solve, true residual" if used == "direct"
                    else f"MINRES: {it} iterations, residual estimate")
            print(f"  {what} {relres:.3e} ({'converged' if conv else 'NOT converged'})",
                  file=sys.stdout)
        if not conv and self._raise:
            raise _lib.NxNotConverged(
                f"MINRES did not converge: {it} iterations, relative residual {relres:.3e} "
                f"> rtol {self._rtol:.1e}")
        return self.assembler.solution_functions(functions)

    def _configure(self) -> None:
        """The handle in the state this solver's options ask for (as :meth:`solve` does)."""
        if self.assembler.preconditioned != self._pc:
            self.assembler.set_preconditioner(self._pc)
        h = self.assembler.handle
        if self.assembler.preconditioned and h.pc_exact() != self._pc_exact:
            h.set_pc_exact(self._pc_exact)
        self.assembler.set_direct(self._direct and (self.assembler.preconditioned
                                                    or self.assembler.fe_direct_available))
        # (handle state, set on every call: two solvers on one assembler each get their own)
        h.set_ensemble_cycles(self._ens_cycles)
        # (the same for the batched continuous-pressure calls' cycle switch, which has no effect
        # without batch_continuous: set where this solver wants it, and taken back where the
        # handle itself says another solver left it on. The getattr: handle objects without
        # the query -- the stubs that the host tests drive this method with -- have never had
        # the switch on; a real handle pays one C call here)
        if self._cp_batch and self._cp_batch_cycles:
            h.set_cp_batch_cycles(True)
        elif getattr(h, "cp_batch_cycles_info", None) and h.cp_batch_cycles_info()["enabled"]:
            h.set_cp_batch_cycles(False)

    @timed("nxfx:Solver:solve_many")
    def solve_many(self, p_bc, f=None) -> "BatchResult":
        """Solve B boundary / source scenarios against the matrix of the last
        ``compute_forms`` (its ``R``): ``p_bc`` a sequence of B items, each in any form
        ``compute_forms`` accepts, or an array ``(B, num_nodes)``; ``f`` None (the last
        ``compute_forms``' source), B scalars or ``(B, num_edges)`` values in ``graph.edges()``
        order.

        Where the handle supports it (``nx_batch_supported``: P1/DG0, one rank, the direct
        solve) the scenarios go through ``nx_batch_solve`` in one batched pass
        (``path == "batched"``); with ``batch_degrees`` so do flux degrees k >= 2 with DG0
        pressure where ``nx_fe_batch_supported`` holds (``nx_fe_batch_solve``: the condensed
        direct solve with a column dimension), and with ``batch_continuous`` continuous
        pressure on a forest where ``nx_cp_batch_supported`` holds (``nx_cp_batch_solve``: the
        node-condensed solve factored once per call) -- and, with ``batch_continuous_cycles``
        on top, on a graph with cycles whose assembler has ``cycle_direct`` (the chord
        correction per column). Otherwise -- general degrees,
        ``ksp_type="minres"``,
        ``pc_type="none"``, the lumped mass, the global-memory sweeps, or ``NXHIP_BATCH=0`` --
        the per-scenario loop runs (``"sequential"``): the rhs coefficients alone are set (R
        is never uploaded again), then rhs assembly, solve, gather; afterwards the coefficients
        and the rhs of the last ``compute_forms`` are put back. The reference has no
        counterpart (one KSP solve per call, ``solver.py:107-135``)."""
        if self._closed:
            raise RuntimeError("the solver has been destroyed")
        asm = self.assembler
        if getattr(asm, "_coefficients", None) is None:
            raise RuntimeError("compute_forms() must be called before solve_many()")
        if getattr(asm, "_nranks", 1) > 1:
            raise NotImplementedError("solve_many runs on one rank; with several ranks loop "
                                      "over compute_forms / assemble / solve")
        edge_bc, edge_f, f_const = asm.scenario_coefficients(p_bc, f)
        B = edge_bc.shape[0]
        h = asm.handle
        self._configure()
        if not asm.lhs_current:  # the matrix of the last compute_forms (its R), values only
            asm.assemble(assemble_lhs=True, assemble_rhs=False)
        # the documented rule ("Batched scenarios"): one scenario on a large system
        # has nothing to batch and measured no gain over the single solve (1.03 M rows:
        # 0.98x; 16 k rows: 1.44x), so it takes the loop; NXHIP_BATCH=1 overrides the rule,
        # NXHIP_BATCH=0 forces the loop
        want = os.environ.get("NXHIP_BATCH", "")
        worth = want == "1" or not (B == 1 and h.n_rows > BATCH_SINGLE_MAX_ROWS)
        batched = want != "0" and worth and h.batch_supported()
        # (k, 0), k >= 2, with batch_degrees: the condensed direct solve's batched pass
        fe_batched = (not batched and self._fe_batch and want != "0" and worth and self._direct
                      and len(asm.degrees) == 2 and asm.degrees[0] >= 2 and asm.degrees[1] == 0
                      and h.fe_batch_supported())
        # (k, m), m >= 1, with batch_continuous: the node-condensed solve's batched pass
        cp_batched = (not batched and not fe_batched and self._cp_batch and want != "0" and worth
                      and self._direct and len(asm.degrees) == 2 and asm.degrees[1] >= 1
                      and h.cp_batch_supported())
        if batched:
            x, it, rr, conv = h.batch_solve(edge_bc, edge_f, f_const, self._rtol, blocks=True)
            info = h.batch_info()
        elif fe_batched:
            batched = True
            x, it, rr, conv = h.fe_batch_solve(edge_bc, edge_f, f_const, self._rtol,
                                               self._maxit, blocks=True)
            info = h.batch_info()
        elif cp_batched:
            batched = True
            x, it, rr, conv = h.cp_batch_solve(edge_bc, edge_f, f_const, self._rtol,
                                               self._maxit, blocks=True)
            info = h.batch_info()
        else:
            x = h.batch_output(B)  # page-locked and reused, as the batched path's
            it = np.zeros(B, dtype=np.int32)
            rr = np.zeros(B, dtype=np.float64)
            conv = np.zeros(B, dtype=bool)
            ce = self._check_every or (4 if asm.preconditioned else 32)
            try:
                for j in range(B):
                    asm.set_rhs_coefficients(edge_bc[j],
                                             None if f_const is None else float(f_const[j]),
                                             None if edge_f is None else edge_f[j])
                    h.assemble(False, True)
                    it[j], rr[j], conv[j] = h.solve(self._rtol, self._maxit, ce)
                    h.solution_blocks(x[j])
            finally:
                asm.restore_rhs_coefficients()
                h.assemble(False, True)
            info = {"launches": 0, "refined": 0, "fallback": 0, "chunk": 1}
        res = BatchResult(asm, x, it, rr, conv, "batched" if batched else "sequential", info)
        if self._raise and not conv.all():
            bad = np.flatnonzero(~conv)
            raise _lib.NxNotConverged(
                f"solve_many: columns {bad.tolist()} did not converge (relative residuals "
                f"{rr[bad].tolist()} > rtol {self._rtol:.1e})")
        return res

    def _ensemble_batched(self) -> bool:
        """Whether the options and the handle put an ensemble on the batched path (the handle
        configured as :meth:`solve` does it first)."""
        asm = self.assembler
        return (tuple(asm.degrees) == (1, 0) and self._direct and self._pc and self._pc_exact
                and asm.handle.ensemble_supported())

    @timed("nxfx:Solver:solve_ensemble")
    def solve_ensemble(self, R, p_bc=None, f=None) -> "BatchResult":
        """Solve B scenarios that differ in the resistance field: scenario j solves the system
        of ``R[j]``. ``R``: ``(B, num_edges)`` in ``graph.edges()`` order, or ``(B,)`` constants;
        ``p_bc``: None (the boundary data of the last ``compute_forms`` on every scenario) or B
        items as :meth:`solve_many` takes them; ``f``: as for :meth:`solve_many`.

        Where ``nx_ensemble_supported`` holds (P1/DG0, one rank, the direct solve; a forest, or
        with ``ensemble_cycles=True`` a graph with up to 512 cycle chains: a cycle correction
        per scenario, ``2 n_cyc`` batched unit solves and one factorisation each)
        the scenarios go through ``nx_ensemble_solve`` in one batched pass
        (``path == "batched"``): a matrix per column, none of them assembled. The matrix of the
        last ``compute_forms`` is assembled first if it is not current (the residual reads its
        R-independent entries). A scenario the batched pass reports unconverged is solved again
        by the sequential path and counted in ``info["fallback"]``.

        Otherwise -- a graph with cycles without ``ensemble_cycles``, general degrees, ``ksp_type="minres"``,
        ``pc_type="none"``, the lumped mass, or ``NXHIP_BATCH=0`` -- the per-scenario loop runs
        (``"sequential"``): the scenario's coefficients are uploaded, R included, then assembly,
        solve, gather. Afterwards the coefficients of the last ``compute_forms`` are put back,
        the system is assembled again and the handle's solution, rhs and last-solve figures
        are restored (``nx_stash_solution``), so a later ``solve()`` returns the bits it returned before. The reference has no
        counterpart (it would loop ``compute_forms`` / ``assemble`` / ``solve``)."""
        if self._closed:
            raise RuntimeError("the solver has been destroyed")
        asm = self.assembler
        if getattr(asm, "_coefficients", None) is None:
            raise RuntimeError("compute_forms() must be called before solve_ensemble()")
        if getattr(asm, "_nranks", 1) > 1:
            raise NotImplementedError("solve_ensemble runs on one rank; with several ranks loop "
                                      "over compute_forms / assemble / solve")
        edge_R, edge_bc, edge_f, f_const = asm.ensemble_coefficients(R, p_bc, f)
        B = edge_R.shape[0]
        h = asm.handle
        self._configure()
        batched = os.environ.get("NXHIP_BATCH", "") != "0" and self._ensemble_batched()
        info = {"launches": 0, "refined": 0, "fallback": 0, "chunk": 1}
        if batched:
            if not asm.lhs_current:  # (the residual reads the +-1 entries of the values)
                asm.assemble(assemble_lhs=True, assemble_rhs=False)
            x, it, rr, conv = h.ensemble_solve(edge_R, edge_bc, edge_f, f_const, self._rtol,
                                               blocks=True)
            info = h.batch_info()
            todo = np.flatnonzero(~conv)
            info["fallback"] = int(todo.size)
        else:
            x = h.batch_output(B)  # page-locked and reused, as the batched path's
            it = np.zeros(B, dtype=np.int32)
            rr = np.zeros(B, dtype=np.float64)
            conv = np.zeros(B, dtype=bool)
            todo = np.arange(B)
        if todo.size:
            self._ensemble_loop(todo, edge_R, edge_bc, edge_f, f_const, x, it, rr, conv)
        res = BatchResult(asm, x, it, rr, conv, "batched" if batched else "sequential", info)
        if self._raise and not conv.all():
            bad = np.flatnonzero(~conv)
            raise _lib.NxNotConverged(
                f"solve_ensemble: columns {bad.tolist()} did not converge (relative residuals "
                f"{rr[bad].tolist()} > rtol {self._rtol:.1e})")
        return res

    def _ensemble_loop(self, todo, edge_R, edge_bc, edge_f, f_const, x, it, rr, conv) -> None:
        """The sequential path of :meth:`solve_ensemble` on the scenarios ``todo``."""
        asm = self.assembler
        h = asm.handle
        ce = self._check_every or (4 if asm.preconditioned else 32)
        h.stash_solution(False)
        try:
            for j in todo:
                asm.set_scenario_coefficients(edge_R[j], edge_bc[j],
                                              None if f_const is None else float(f_const[j]),
                                              None if edge_f is None else edge_f[j])
                h.assemble(True, True)
                it[j], rr[j], conv[j] = h.solve(self._rtol, self._maxit, ce)
                h.solution_blocks(x[j])
        finally:
            asm.restore_coefficients()
            asm.assemble(assemble_lhs=True, assemble_rhs=True)
            h.stash_solution(True)  # (flushes that assembly, then x, rhs, the last solve's figures)

    @timed("nxfx:Solver:gradient")
    def gradient(self, p_bc, f=None, *, rows, weights=None, data=None, R=None,
                 derivatives: bool = True) -> "GradientResult":
        """Adjoint gradients of an observed-row objective for B scenarios against the matrix
        of the last ``compute_forms`` (``nx_batch_gradient``: two batched direct solves, no
        solution leaves the device).

        ``p_bc`` / ``f``: as for :meth:`solve_many`. ``rows``: distinct indices into the
        reference block order (the columns of ``BatchResult.x``); ``weights``: one per row
        (default ones). ``data`` None: the linear objective ``J_j = sum_i w_i x_j[r_i]``;
        otherwise ``(B, n_obs)`` (or ``(n_obs,)``, the same for every scenario): the least
        squares objective ``J_j = 1/2 sum_i w_i (x_j[r_i] - d_ji)^2``. Returns a
        :class:`GradientResult`: the objective and its derivatives with respect to every
        edge's ``R`` and source and every boundary node's pressure.

        It runs where ``solve_many`` takes its batched path; elsewhere -- several ranks,
        general degrees, ``ksp_type="minres"``, ``pc_type="none"``, the lumped mass -- it
        raises ``NotImplementedError`` (there is no host fallback). The reference has no
        counterpart.

        With ``batch_degrees`` it also serves flux degree k >= 2 with DG0 pressure where
        ``nx_fe_batch_supported`` holds (``nx_fe_batch_gradient``: both solves through the
        batched condensed solve, the contraction with the degree-k element mass); ``rows`` then
        index the (k, 0) system's block order, interior flux nodes included. Not served on
        these degrees: ``R=`` (ensembles), :meth:`hessian_vector` and several ranks --
        ``NotImplementedError``, as without the option.

        With ``batch_continuous`` it serves continuous pressure (k > m >= 1) on a forest, where
        ``nx_cp_batch_supported`` holds (``nx_cp_batch_gradient``: one factor stage of the
        node-condensed solve per call, both solves on its factors, the contraction over the
        (k, m) rows); ``rows`` then index the (k, m) system's block order. ``batch_degrees``
        alone does not switch it on. Not served on these degrees: ``R=``,
        :meth:`hessian_vector`, several ranks, and graphs with cycles unless
        ``batch_continuous_cycles`` is on as well (with ``cycle_direct`` on the assembler: both
        solves then go through the corrected batched solve, chords included in ``dR`` / ``df``).

        ``R`` (``(B, num_edges)`` or ``(B,)`` constants, as :meth:`solve_ensemble`): scenario j
        is evaluated at ``R[j]`` instead of the last ``compute_forms``' R
        (``nx_ensemble_gradient``; a forest, or a graph with cycles under
        ``ensemble_cycles=True``, elsewhere ``NotImplementedError``), and
        ``p_bc`` may be None (the last ``compute_forms``' boundary data).
        ``derivatives=False`` (with ``R``): the objective values alone -- the forward solves,
        no adjoint; ``dR``, ``df`` and ``dp_bc`` are None and ``iterations``,
        ``residual_norms``, ``converged`` are ``(B, 1)``."""
        if self._closed:
            raise RuntimeError("the solver has been destroyed")
        asm = self.assembler
        if getattr(asm, "_coefficients", None) is None:
            raise RuntimeError("compute_forms() must be called before gradient()")
        if R is None and not derivatives:
            raise NotImplementedError("derivatives=False needs R (the ensemble call)")
        fe = self._adjoint_supported("gradient", ensemble=R is not None)
        if R is None:
            edge_R = None
            edge_bc, edge_f, f_const = asm.scenario_coefficients(p_bc, f)
        else:
            edge_R, edge_bc, edge_f, f_const = asm.ensemble_coefficients(R, p_bc, f)
        B = edge_bc.shape[0]
        h = asm.handle
        rows, w, data = self._observations(rows, weights, data, B)
        dev_rows = self._adjoint_ready("gradient", rows, edge_R is not None, fe)
        if fe:
            call = h.cp_batch_gradient if fe == "cp" else h.fe_batch_gradient
            value, gR, gbc, gf, it, rr, conv = call(
                edge_bc, edge_f, f_const, self._rtol, self._maxit, rows=dev_rows, weights=w,
                data=data)
        elif edge_R is not None:
            value, gR, gbc, gf, it, rr, conv = h.ensemble_gradient(
                edge_R, edge_bc, edge_f, f_const, self._rtol, rows=dev_rows, weights=w,
                data=data, derivatives=derivatives)
        else:
            value, gR, gbc, gf, it, rr, conv = h.batch_gradient(
                edge_bc, edge_f, f_const, self._rtol, rows=dev_rows, weights=w, data=data)
        if gR is None:  # the objective alone
            res = GradientResult(value.copy(), None, None, None, it, rr, conv, h.batch_info())
            if self._raise and not conv.all():
                bad = np.flatnonzero(~conv.all(axis=1))
                raise _lib.NxNotConverged(
                    f"gradient: columns {bad.tolist()} did not converge (relative residuals "
                    f"{rr[bad].tolist()} > rtol {self._rtol:.1e})")
            return res
        # edge slots -> graph.edges() order, flux end rows -> boundary nodes (gathers: every
        # output is copied out of the handle's page-locked buffer, which the next call of this
        # batch size then reuses)
        slot, node_idx, node_sign = asm.gradient_maps()
        dR = np.take(gR, slot, axis=1)
        df = np.take(gf, slot, axis=1)
        dp_bc = np.take(gbc.reshape(B, -1), node_idx, axis=1) * node_sign
        res = GradientResult(value.copy(), dR, df, dp_bc, it, rr, conv, h.batch_info())
        if self._raise and not conv.all():
            bad = np.flatnonzero(~conv.all(axis=1))
            raise _lib.NxNotConverged(
                f"gradient: columns {bad.tolist()} did not converge (relative residuals "
                f"{rr[bad].tolist()} > rtol {self._rtol:.1e})")
        return res

    def _adjoint_supported(self, what: str, ensemble: bool = False) -> str:
        """The options under which :meth:`gradient` and :meth:`hessian_vector` run. Returns the
        general-degree route of the call, or "" (P1/DG0): "fe" -- :meth:`gradient` on degrees
        (k, 0), k >= 2, under ``batch_degrees`` (``nx_fe_batch_gradient``); "cp" -- on
        continuous pressure, k > m >= 1, under ``batch_continuous``
        (``nx_cp_batch_gradient``)."""
        asm = self.assembler
        if getattr(asm, "_nranks", 1) > 1:
            raise NotImplementedError(f"{what} runs on one rank")
        deg = tuple(asm.degrees)
        k0 = len(deg) == 2 and deg[0] >= 2 and deg[1] == 0
        km = len(deg) == 2 and deg[0] > deg[1] >= 1
        fe = ""
        if what == "gradient":
            fe = "fe" if k0 and self._fe_batch else "cp" if km and self._cp_batch else ""
        if deg != (1, 0) and not fe:
            hint = ""
            if k0 and what == "gradient":
                hint = ("; Solver(..., batch_degrees=True) (or NXHIP_FE_BATCH=1) serves gradient "
                        "on flux degree k >= 2 with DG0 pressure")
            if km and what == "gradient":
                hint = ("; Solver(..., batch_continuous=True) (or NXHIP_CP_BATCH=1) serves "
                        "gradient on continuous pressure (k > m >= 1) on a forest")
            raise NotImplementedError(
                f"{what} needs the P1/DG0 discretisation, not degrees {deg}{hint}")
        if fe and ensemble:
            raise NotImplementedError(
                f"{what}(R=...): the ensemble route serves P1/DG0 only, not degrees {deg}")
        if not self._direct:
            raise NotImplementedError(f"{what} needs the direct solve (ksp_type='preonly'), "
                                      "not MINRES")
        if not self._pc:
            raise NotImplementedError(f"{what} needs the tree decomposition (pc_type != 'none')")
        if not self._pc_exact:
            raise NotImplementedError(f"{what} needs the consistent mass (pc_mass='lumped' "
                                      "is not exact)")
        return fe

    def _observations(self, rows, weights, data, B: int):
        """The observed rows, weights and data of B scenarios, checked and normalised."""
        n = self.assembler.handle.n_rows
        rows = np.asarray(rows)
        if rows.ndim != 1 or rows.size < 1 or not np.issubdtype(rows.dtype, np.integer):
            raise ValueError("rows must be a 1-D array of at least one integer index")
        if rows.min() < 0 or rows.max() >= n:
            raise ValueError(f"rows must lie in [0, {n})")
        if np.unique(rows).size != rows.size:
            raise ValueError("rows must be distinct")
        w = np.ones(rows.size) if weights is None else np.asarray(weights, dtype=np.float64)
        if w.shape != (rows.size,):
            raise ValueError("weights must have one value per observed row")
        if data is not None:
            data = np.asarray(data, dtype=np.float64)
            if data.shape == (rows.size,):
                data = np.broadcast_to(data, (B, rows.size))
            if data.shape != (B, rows.size):
                raise ValueError(f"data must be ({B}, {rows.size}) or ({rows.size},)")
        return rows, w, data

    def _adjoint_ready(self, what: str, rows, ensemble: bool, fe: str = "") -> np.ndarray:
        """The handle configured, its matrix current and the batched path checked (``fe``: the
        general-degree route of :meth:`_adjoint_supported`); returns the observed rows as
        device rows."""
        asm = self.assembler
        h = asm.handle
        self._configure()
        if not asm.lhs_current:  # the matrix of the last compute_forms (its R), values only
            asm.assemble(assemble_lhs=True, assemble_rhs=False)
        if fe == "cp":
            if not h.cp_batch_supported():
                raise NotImplementedError(f"{what}: the batched node-condensed solve does not "
                                          "apply to this handle (nx_cp_batch_supported)")
            return asm.block_order_rows()[rows]
        if fe:
            if not h.fe_batch_supported():
                raise NotImplementedError(f"{what}: the batched condensed solve does not apply "
                                          "to this handle (nx_fe_batch_supported)")
            return asm.block_order_rows()[rows]
        if not h.batch_supported():
            raise NotImplementedError(f"{what}: the batched direct solve does not apply to this "
                                      "handle (nx_batch_supported)")
        if ensemble and not h.ensemble_supported():
            raise NotImplementedError(f"{what}(R=...): the batched ensemble does not apply "
                                      "to this handle (nx_ensemble_supported)")
        return asm.block_order_rows()[rows]

    @timed("nxfx:Solver:hessian_vector")
    def hessian_vector(self, p_bc, f=None, *, rows, weights=None, data=None, v_R=None,
                       v_p_bc=None, v_f=None, R=None,
                       gauss_newton: bool = False) -> "HessianVectorResult":
        """Exact Hessian-vector products of :meth:`gradient`'s objective for B scenarios
        (``nx_batch_hvp``: four batched direct solves -- forward, adjoint, tangent and
        second-order adjoint -- and one contraction; no solution leaves the device).

        ``p_bc`` / ``f`` / ``rows`` / ``weights`` / ``data`` / ``R``: as for :meth:`gradient`.
        The direction of scenario j is ``(v_R[j], v_p_bc[j], v_f[j])``: ``v_R`` ``(B,
        num_edges)`` or ``(num_edges,)`` in ``graph.edges()`` order (any sign), ``v_p_bc`` nodal
        ``(B, num_nodes)`` or ``(num_nodes,)``, ``v_f`` ``(B, num_edges)``, ``(num_edges,)`` or
        ``(B,)`` constants; a part left None is zero
        (:func:`~networks_fenicsx_amd.assembly.hvp_directions`), all three None a
        ``ValueError``. Returns a :class:`HessianVectorResult`: ``H v`` in the three blocks
        ``HdR``, ``Hdf``, ``Hdp_bc`` and, from the same pass, the objective and the gradient
        with :meth:`gradient`'s bits.

        ``gauss_newton=True`` (least squares only: ``data`` None raises ``ValueError``): the
        product with the positive semidefinite ``J^T W J`` of the observed values' Jacobian --
        three solves, no adjoint, no gradient (``dR``, ``df``, ``dp_bc`` None).

        It runs where :meth:`gradient` runs and raises ``NotImplementedError`` elsewhere; with
        ``R`` on a forest, or on a graph with cycles under ``ensemble_cycles=True``
        (``nx_ensemble_hvp``). The reference has no counterpart."""
        if self._closed:
            raise RuntimeError("the solver has been destroyed")
        asm = self.assembler
        if getattr(asm, "_coefficients", None) is None:
            raise RuntimeError("compute_forms() must be called before hessian_vector()")
        if gauss_newton and data is None:
            raise ValueError("gauss_newton=True needs the least-squares objective (data)")
        if v_R is None and v_p_bc is None and v_f is None:
            raise ValueError("a direction is needed: v_R, v_p_bc or v_f")
        self._adjoint_supported("hessian_vector")
        if R is None:
            edge_R = None
            edge_bc, edge_f, f_const = asm.scenario_coefficients(p_bc, f)
        else:
            edge_R, edge_bc, edge_f, f_const = asm.ensemble_coefficients(R, p_bc, f)
        B = edge_bc.shape[0]
        h = asm.handle
        dir_R, dir_bc, dir_f = asm.hvp_directions(B, v_R, v_p_bc, v_f)
        rows, w, data = self._observations(rows, weights, data, B)
        dev_rows = self._adjoint_ready("hessian_vector", rows, edge_R is not None)
        value, gR, gbc, gf, hR, hbc, hf, it, rr, conv = h.batch_hvp(
            edge_bc, edge_f, f_const, self._rtol, rows=dev_rows, weights=w, data=data,
            dir_R=dir_R, dir_bc=dir_bc, dir_f=dir_f, edge_R=edge_R, gauss_newton=gauss_newton)
        # the gathers of gradient(): edge slots -> graph.edges() order, flux end rows -> nodes
        # (every output is copied out of the handle's page-locked buffer)
        slot, node_idx, node_sign = asm.gradient_maps()

        def edges(a):
            return None if a is None else np.take(a, slot, axis=1)

        def nodes(a):
            return None if a is None else np.take(a.reshape(B, -1), node_idx, axis=1) * node_sign

        res = HessianVectorResult(value.copy(), edges(gR), edges(gf), nodes(gbc), edges(hR),
                                  edges(hf), nodes(hbc), it, rr, conv, h.batch_info())
        if self._raise and not conv.all():
            bad = np.flatnonzero(~conv.all(axis=1))
            raise _lib.NxNotConverged(
                f"hessian_vector: columns {bad.tolist()} did not converge (relative residuals "
                f"{rr[bad].tolist()} > rtol {self._rtol:.1e})")
        return res

    def solution_vector(self) -> np.ndarray:
        """Device-layout solution (owned DoFs of this rank)."""
        return self.assembler.handle.solution()

    def true_residual(self) -> float:
        return self.assembler.handle.true_residual()

    def destroy(self) -> None:
        """Release what the solver owns (the reference destroys its KSP, b and x,
        ``solver.py:137-143``). The device matrix, rhs and Krylov vectors belong to the
        assembler's handle (shared by every solver of that assembler) and go with
        ``assembler.close()``; functions returned by :meth:`solve` stay valid."""
        self._closed = True
        self._ksp.destroy()
        self._A = None
        self._b = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass
