"""Host side of the batched continuous-pressure solve (``nx_cp_batch_solve``): the C ABI's new
entries (header and ctypes table), ``Solver``'s ``batch_continuous`` option with its
``NXHIP_CP_BATCH`` switch, and the numpy restatement of the split -- the factor stage without a
right-hand side (``layout_fe.cp_factor_model``), the right-hand-side sweeps on stacked columns
(``layout_fe.cp_apply_model``) -- against scipy's LU at tests/test_fe_cp.py's bars (no device).

The batched pass has one refinement pass where the single solve has two, so the model is also
held to the default rtol (1e-12) after one solve and one refinement on every graph."""

import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from cases import CASES
from networks_fenicsx_amd import Solver, _lib
from networks_fenicsx_amd.layout_fe import build_cp_tables, cp_apply_model, cp_factor_model
from test_fe_cp import _system
from tree_shapes import SHAPES

NEW = ("nx_cp_batch_supported", "nx_cp_batch_solve", "nx_cp_batch_rhs")
HEADER = Path(__file__).resolve().parent.parent / "include" / "nxhip.h"
PAIRS = [(2, 1), (3, 1), (3, 2), (4, 3)]
GRAPHS = ["Y_N4", "double_Y_N5", "tree5_N15", "arterial5_N40", "linear_alt_N3", "demo_tree_N1",
          "hub5", "hub70"]


class _StubAssembler:
    """What ``Solver.__init__`` reads: the handle (kept, never called)."""

    handle = None


def test_new_symbols_are_declared_and_exported():
    text = HEADER.read_text()
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS
        assert re.search(rf"^int {name}\(nx_network_t\* h,", text, re.M), name
    sig = _lib._SIGS
    assert sig["nx_cp_batch_solve"] == sig["nx_fe_batch_solve"]
    assert sig["nx_cp_batch_rhs"] == sig["nx_fe_batch_rhs"]
    assert sig["nx_cp_batch_supported"] == sig["nx_fe_batch_supported"]
    decl = re.search(r"^int nx_cp_batch_solve\(([^;]*)\);", text, re.M | re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == [
        "h", "n_cols", "edge_bc", "edge_f", "f_const", "rtol", "maxit", "order", "out", "iters",
        "relres", "converged"]
    for name in ("nx_cp_batch_rhs", "nx_cp_batch_supported"):
        fe = name.replace("nx_cp_", "nx_fe_")
        a = re.search(rf"^int {name}\(([^;]*)\);", text, re.M | re.S).group(1)
        b = re.search(rf"^int {fe}\(([^;]*)\);", text, re.M | re.S).group(1)
        assert " ".join(a.split()) == " ".join(b.split())


def test_keyword():
    p = inspect.signature(Solver.__init__).parameters["batch_continuous"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


@pytest.mark.parametrize("value,on", [(None, False), ("1", True), ("0", False), ("", False),
                                      ("true", False)])
def test_env_switch_is_read_when_the_keyword_is_none(monkeypatch, value, on):
    if value is None:
        monkeypatch.delenv("NXHIP_CP_BATCH", raising=False)
    else:
        monkeypatch.setenv("NXHIP_CP_BATCH", value)
    assert Solver(_StubAssembler())._cp_batch is on
    # given, the keyword decides and the environment is not consulted
    assert Solver(_StubAssembler(), batch_continuous=True)._cp_batch is True
    assert Solver(_StubAssembler(), batch_continuous=False)._cp_batch is False
    # the other batch option does not switch this one on
    assert Solver(_StubAssembler(), batch_degrees=True)._cp_batch is on


def test_stored_per_solver(monkeypatch):
    monkeypatch.setenv("NXHIP_CP_BATCH", "1")
    a = Solver(_StubAssembler())
    monkeypatch.setenv("NXHIP_CP_BATCH", "0")
    b = Solver(_StubAssembler())
    assert a._cp_batch is True and b._cp_batch is False


def _graph(name):
    if name in CASES:
        make, N, strategy, _ = CASES[name]
        return make, min(N, 12), strategy
    make, N, _ = SHAPES[name]
    return make, N, None


def _columns(rhs, n=5):
    """The system's own rhs, three seeded random columns of its size, an all-zero column."""
    rng = np.random.default_rng(11)
    cols = [rhs] + [rng.standard_normal(rhs.size) * np.abs(rhs).max() for _ in range(n - 2)]
    return np.stack(cols + [np.zeros_like(rhs)])


@pytest.mark.parametrize("case", GRAPHS)
@pytest.mark.parametrize("km", PAIRS)
def test_split_model_equals_lu(case, km):
    make, N, strategy = _graph(case)
    k, m = km
    mesh, lay, A, val, rhs, R, h = _system(make(), N, k, m, strategy)
    tab = build_cp_tables(lay, *mesh.edges)
    assert tab is not None
    fm = cp_factor_model(lay, tab, R, h)  # (no right-hand side)
    Bm = _columns(rhs, 3)
    X = cp_apply_model(lay, tab, fm, Bm, R, h)
    lu = spla.splu(A.tocsc())
    worst = 0.0
    for j in range(2):
        x_ref = lu.solve(Bm[j])
        assert np.linalg.norm(X[j] - x_ref) <= 1e-10 * np.linalg.norm(x_ref)
        # the true residual of the model's x (one pass, no refinement)
        assert np.linalg.norm(Bm[j] - A @ X[j]) <= 1e-11 * np.linalg.norm(Bm[j])
        # one refinement pass, the batch's only one: inside the default rtol
        r = Bm[j] - A @ X[j]
        x2 = X[j] + cp_apply_model(lay, tab, fm, r[None, :], R, h)[0]
        worst = max(worst, np.linalg.norm(Bm[j] - A @ x2) / np.linalg.norm(Bm[j]))
    print(f"{case} {km}: residual after one refinement {worst:.2e}")
    assert worst <= 1e-12
    assert not X[2].any()  # b = 0: exact zeros


@pytest.mark.parametrize("case,km", [("Y_N4", (2, 1)), ("double_Y_N5", (3, 2)),
                                     ("demo_tree_N1", (4, 3)), ("hub5", (3, 1))])
def test_stacked_columns_equal_single_columns_bit_for_bit(case, km):
    make, N, strategy = _graph(case)
    mesh, lay, A, val, rhs, R, h = _system(make(), N, *km, strategy)
    tab = build_cp_tables(lay, *mesh.edges)
    fm = cp_factor_model(lay, tab, R, h)
    Bm = _columns(rhs)
    X = cp_apply_model(lay, tab, fm, Bm, R, h)
    for j in range(Bm.shape[0]):
        np.testing.assert_array_equal(cp_apply_model(lay, tab, fm, Bm[j:j + 1], R, h)[0], X[j])
    perm = np.array([3, 0, 4, 2, 1])
    np.testing.assert_array_equal(cp_apply_model(lay, tab, fm, Bm[perm], R, h), X[perm])
