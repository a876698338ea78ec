"""CPU adjoint gradient of an observed-row objective at general degrees, from the oracle alone
(test helper): the recipe of tests/gradient_ref.py on
``oracle.nx_oracle_fe.assemble_reference_fe`` (flux degree k, pressure degree m).

The reference's (non-symmetric) system ``A x = b``; objective over observed rows ``r_i``
(reference block order) with weights ``w_i``, least squares (``data`` given) or linear.
``A^T lambda = c`` (SuperLU on ``A^T``), then ``dJ/dR_e = -lambda^T (dA/dR_e) x`` with
``dA/dR_e = A(R = e_e) - A(R = 0)`` (A is affine in R), and ``dJ/dp_bc``, ``dJ/df`` from
``lambda^T db`` with ``db`` the difference of two right-hand sides (b is linear in ``p_bc`` and
``f``). Nothing of the device code is used."""

from __future__ import annotations

import numpy as np
import scipy.sparse.linalg as spla

from gradient_ref import objective
from oracle import nx_oracle_fe as OF

__all__ = ["AdjointRefFe", "forward_fe", "objective"]


def forward_fe(P, pbc, f, R):
    """``x`` of one scenario (nodal ``pbc``, per-edge or constant ``f`` and ``R``)."""
    A, b = OF.assemble_reference_fe(P, pbc, f=f, R=R)
    return spla.splu(A.tocsc()).solve(b)


class AdjointRefFe:
    """One graph, one pair of degrees and one ``R``: the factorisations and the derivative
    operators, computed once and shared by every scenario and objective of a test module."""

    def __init__(self, P, R):
        self.P = P
        base = P.base
        E = base.src.size
        nn = base.pos3.shape[0]
        self.R = np.broadcast_to(np.asarray(R, dtype=np.float64), (E,)).copy()
        zero_p = np.zeros(nn)
        self.A, _ = OF.assemble_reference_fe(P, zero_p, f=0.0, R=self.R)
        self.lu = spla.splu(self.A.tocsc())
        self.luT = spla.splu(self.A.T.tocsc())
        A0, b0 = OF.assemble_reference_fe(P, zero_p, f=0.0, R=np.zeros(E))
        unit = np.eye(E)
        self.dA = []  # dA/dR_e
        self.db_f = np.zeros((E, P.n_dofs))  # db/df_e
        for e in range(E):
            Ae, _ = OF.assemble_reference_fe(P, zero_p, f=0.0, R=unit[e])
            self.dA.append((Ae - A0).tocsr())
            _, be = OF.assemble_reference_fe(P, zero_p, f=unit[e], R=self.R)
            self.db_f[e] = be - b0
        self.boundary = np.concatenate([base.leaf_in, base.root_out])
        self.db_p = np.zeros((nn, P.n_dofs))  # db/dp_bc[node], zero off the boundary nodes
        for v in self.boundary:
            pv = np.zeros(nn)
            pv[v] = 1.0
            _, bv = OF.assemble_reference_fe(P, pv, f=0.0, R=self.R)
            self.db_p[v] = bv - b0

    def solve(self, pbc, f):
        _, b = OF.assemble_reference_fe(self.P, pbc, f=f, R=self.R)
        return self.lu.solve(b)

    def gradient(self, pbc, f, rows, weights, data=None):
        """``dict(value, dR (E,), df (E,), dp_bc (nodes,), x, lam)`` of one scenario."""
        rows = np.asarray(rows, dtype=np.int64)
        w = np.asarray(weights, dtype=np.float64)
        x = self.solve(pbc, f)
        c = np.zeros(self.P.n_dofs)
        c[rows] = w if data is None else w * (x[rows] - np.asarray(data, dtype=np.float64))
        lam = self.luT.solve(c)
        dR = np.array([-(lam @ (dA @ x)) for dA in self.dA])
        return {"value": objective(x, rows, w, data), "dR": dR, "df": self.db_f @ lam,
                "dp_bc": self.db_p @ lam, "x": x, "lam": lam}
