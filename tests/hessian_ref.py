"""CPU Hessian-vector product of the observed-row objective, from the oracle alone (test helper).

Built on :class:`gradient_ref.AdjointRef` (the reference's non-symmetric ``A x = b``, SuperLU on
``A`` and ``A^T``, ``dA/dR_e`` and ``db/dp_bc``, ``db/df`` as differences of assemblies). A
direction ``v = (v_R (E,), v_p (nodes,), v_f (E,))``, any part None meaning zero:

* ``Adot = sum_e v_R[e] dA/dR_e``, ``bdot = db_p^T v_p + db_f^T v_f``;
* tangent ``A xdot = bdot - Adot x``;
* second-order adjoint ``A^T lamdot = cdot - Adot^T lam`` with ``cdot = w xdot[rows]`` on the
  observed rows (least squares) or 0 (linear);
* ``HR[e] = -(lamdot^T dA_e x + lam^T dA_e xdot)``, ``Hf = db_f lamdot``, ``Hp = db_p lamdot``.

Gauss-Newton (least squares only): ``A^T lamdot = W xdot`` and ``HR[e] = -lamdot^T dA_e x`` --
``J_x^T W J_x v`` with ``J_x`` the Jacobian of the observed values, positive semidefinite.
Nothing of the device code is used."""

from __future__ import annotations

import numpy as np

from gradient_ref import AdjointRef


class HessianRef(AdjointRef):
    """:class:`AdjointRef` with :meth:`hvp`; the factorisations are shared with ``gradient``."""

    def hvp(self, pbc, f, rows, weights, data=None, v_R=None, v_p=None, v_f=None,
            gauss_newton=False):
        """``dict(value, dR, df, dp_bc, HdR (E,), Hdf (E,), Hdp_bc (nodes,), xdot, lamdot)`` of
        one scenario; ``dR``, ``df``, ``dp_bc`` are None in Gauss-Newton mode."""
        if gauss_newton and data is None:
            raise ValueError("Gauss-Newton needs the least-squares objective")
        if v_R is None and v_p is None and v_f is None:
            raise ValueError("at least one direction")
        rows = np.asarray(rows, dtype=np.int64)
        w = np.asarray(weights, dtype=np.float64)
        g = self.gradient(pbc, f, rows, w, data)
        x, lam = g["x"], g["lam"]
        n = self.P.n_dofs
        Ax = np.zeros(n)  # Adot x
        ATl = np.zeros(n)  # Adot^T lam
        if v_R is not None:
            for e, dA in enumerate(self.dA):
                Ax += v_R[e] * (dA @ x)
                ATl += v_R[e] * (dA.T @ lam)
        bdot = np.zeros(n)
        if v_p is not None:
            bdot += np.asarray(v_p, dtype=np.float64) @ self.db_p
        if v_f is not None:
            bdot += np.asarray(v_f, dtype=np.float64) @ self.db_f
        xdot = self.lu.solve(bdot - Ax)
        cdot = np.zeros(n)
        if data is not None:
            cdot[rows] = w * xdot[rows]
        lamdot = self.luT.solve(cdot if gauss_newton else cdot - ATl)
        HR = np.empty(len(self.dA))
        for e, dA in enumerate(self.dA):
            t = lamdot @ (dA @ x)
            if not gauss_newton:
                t += lam @ (dA @ xdot)
            HR[e] = -t
        out = {"value": g["value"], "dR": g["dR"], "df": g["df"], "dp_bc": g["dp_bc"],
               "HdR": HR, "Hdf": self.db_f @ lamdot, "Hdp_bc": self.db_p @ lamdot,
               "xdot": xdot, "lamdot": lamdot}
        if gauss_newton:
            out["dR"] = out["df"] = out["dp_bc"] = None
        return out
