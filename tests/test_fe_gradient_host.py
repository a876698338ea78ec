"""Host side of the (k, 0) adjoint gradient: the C ABI's new entry (header and ctypes table) and
``Solver.gradient``'s routing with the handle stubbed (no device) -- the new route engages only
with ``batch_degrees`` on degrees (k, 0), k >= 2, and everything it does not serve still raises
``NotImplementedError``."""

import re
from pathlib import Path

import numpy as np
import pytest

from networks_fenicsx_amd import Solver, _lib

HEADER = Path(__file__).resolve().parent.parent / "include" / "nxhip.h"
E, NODES, ROWS = 3, 4, 20


class _StubHandle:
    n_rows = ROWS

    def __init__(self, fe_ok=True):
        self.calls = []
        self._fe_ok = fe_ok

    def pc_exact(self):
        return True

    def set_ensemble_cycles(self, enable):
        pass

    def batch_supported(self):
        return False

    def fe_batch_supported(self):
        return self._fe_ok

    def batch_info(self):
        return {"launches": 0, "refined": 0, "fallback": 0, "chunk": 1}

    def fe_batch_gradient(self, edge_bc, edge_f, f_const, rtol, maxit, *, rows, weights, data):
        B = edge_bc.shape[0]
        self.calls.append(dict(rows=np.asarray(rows), rtol=rtol, maxit=maxit, data=data))
        gR = np.tile(np.arange(E, dtype=float), (B, 1))
        gbc = np.arange(B * E * 2, dtype=float).reshape(B, E, 2)
        one = np.ones((B, 2))
        return np.zeros(B), gR, gbc, gR + 10.0, one.astype(np.int32), 0 * one, one.astype(bool)

    def batch_gradient(self, *a, **kw):
        raise AssertionError("the P1/DG0 entry point on a (k, 0) system")

    ensemble_gradient = batch_hvp = batch_gradient


class _StubAssembler:
    """What ``Solver.gradient`` reads of the assembler, for degrees ``deg``."""

    preconditioned = True
    fe_direct_available = True
    lhs_current = True
    _coefficients = object()

    def __init__(self, deg, nranks=1, fe_ok=True):
        self.degrees = deg
        self._nranks = nranks
        self.handle = _StubHandle(fe_ok)

    def set_direct(self, on):
        pass

    def set_preconditioner(self, on):
        pass

    def scenario_coefficients(self, p_bc, f):
        B = len(p_bc)
        return np.zeros((B, E, 2)), None, np.zeros(B)

    def ensemble_coefficients(self, R, p_bc, f):
        B = len(R)
        return np.ones((B, E)), np.zeros((B, E, 2)), None, np.zeros(B)

    def hvp_directions(self, B, v_R, v_p_bc, v_f):
        return np.ones((B, E)), None, None

    def block_order_rows(self):
        return np.arange(ROWS)[::-1].copy()  # (a permutation the route must apply)

    def gradient_maps(self):
        # edge slots reversed; two boundary nodes reading gbc entries 0 and 5, one negated
        return np.arange(E)[::-1].copy(), np.array([0, 5, 0, 0]), np.array([-1.0, 1.0, 0.0, 0.0])


KW = dict(rows=np.array([1, 7]), weights=np.array([1.0, 2.0]))


def test_symbol_is_declared_and_exported():
    text = HEADER.read_text()
    assert "nx_fe_batch_gradient" in _lib.EXPORTED_SYMBOLS
    # nx_batch_gradient's argument list with maxit after rtol
    sig, ref = _lib._SIGS["nx_fe_batch_gradient"][1], _lib._SIGS["nx_batch_gradient"][1]
    assert len(sig) == len(ref) + 1 and sig[:6] == ref[:6] and sig[7:] == ref[6:]
    decl = re.search(r"^int nx_fe_batch_gradient\(([^;]*)\);", text, re.M | re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == [
        "h", "n_cols", "edge_bc", "edge_f", "f_const", "rtol", "maxit", "kind", "n_obs",
        "obs_rows", "obs_w", "obs_d", "value", "grad_R", "grad_bc", "grad_f", "iters", "relres",
        "converged"]


@pytest.mark.parametrize("k", [2, 3])
def test_route_engages_with_batch_degrees(k):
    asm = _StubAssembler((k, 0))
    solver = Solver(asm, batch_degrees=True, petsc_options={"ksp_rtol": 1e-11, "ksp_max_it": 77})
    g = solver.gradient([None, None], **KW)
    (call,) = asm.handle.calls
    np.testing.assert_array_equal(call["rows"], asm.block_order_rows()[KW["rows"]])
    assert call["rtol"] == 1e-11 and call["maxit"] == 77 and call["data"] is None
    # the host gathers: edge slots -> graph.edges() order, flux end rows -> boundary nodes
    np.testing.assert_array_equal(g.dR, np.tile([2.0, 1.0, 0.0], (2, 1)))
    np.testing.assert_array_equal(g.df, g.dR + 10.0)
    np.testing.assert_array_equal(g.dp_bc, [[-0.0, 5.0, 0.0, 0.0], [-6.0, 11.0, 0.0, 0.0]])
    assert g.iterations.shape == (2, 2) and g.converged.all()
    g = solver.gradient([None], data=np.array([0.5, 0.25]), **KW)
    assert asm.handle.calls[-1]["data"].shape == (1, 2)


def test_env_switch_engages_the_route(monkeypatch):
    monkeypatch.setenv("NXHIP_FE_BATCH", "1")
    asm = _StubAssembler((2, 0))
    Solver(asm).gradient([None], **KW)
    assert len(asm.handle.calls) == 1


def test_without_batch_degrees_it_still_raises(monkeypatch):
    monkeypatch.delenv("NXHIP_FE_BATCH", raising=False)
    for solver in (Solver(_StubAssembler((2, 0))),
                   Solver(_StubAssembler((2, 0)), batch_degrees=False)):
        with pytest.raises(NotImplementedError, match="degrees") as err:
            solver.gradient([None], **KW)
        assert "batch_degrees" in str(err.value)
        assert not solver.assembler.handle.calls


def test_what_the_route_does_not_serve():
    def solver(deg=(2, 0), opts=None, **kw):
        return Solver(_StubAssembler(deg, **kw), batch_degrees=True, petsc_options=opts)

    with pytest.raises(NotImplementedError, match="ensemble"):
        solver().gradient([None], R=np.ones((1, E)), **KW)
    with pytest.raises(NotImplementedError, match="degrees"):
        solver().hessian_vector([None], v_R=np.ones(E), **KW)
    for deg in ((2, 1), (3, 2)):  # continuous pressure
        with pytest.raises(NotImplementedError, match="degrees"):
            solver(deg).gradient([None], **KW)
    with pytest.raises(NotImplementedError, match="one rank"):
        solver(nranks=2).gradient([None], **KW)
    for opts, word in (({"ksp_type": "minres"}, "MINRES"), ({"pc_type": "none"}, "pc_type"),
                       ({"pc_mass": "lumped"}, "lumped")):
        with pytest.raises(NotImplementedError, match=word):
            solver(opts=opts).gradient([None], **KW)
    # a (k, 0) handle whose batched condensed solve does not apply (no auxiliary handle)
    with pytest.raises(NotImplementedError, match="nx_fe_batch_supported"):
        solver(fe_ok=False).gradient([None], **KW)
    s = solver()
    with pytest.raises(NotImplementedError, match="derivatives=False"):
        s.gradient([None], derivatives=False, **KW)
    assert not s.assembler.handle.calls
