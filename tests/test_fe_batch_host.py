"""Host side of the batched (k, 0) solve: the C ABI's new entries (header and ctypes table)
and ``Solver``'s ``batch_degrees`` option with its ``NXHIP_FE_BATCH`` switch (no device)."""

import inspect
import re
from pathlib import Path

import pytest

from networks_fenicsx_amd import Solver, _lib

NEW = ("nx_fe_batch_supported", "nx_fe_batch_solve", "nx_fe_batch_rhs")
HEADER = Path(__file__).resolve().parent.parent / "include" / "nxhip.h"


class _StubAssembler:
    """What ``Solver.__init__`` reads: the handle (kept, never called)."""

    handle = None


def test_new_symbols_are_declared_and_exported():
    text = HEADER.read_text()
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS
        assert re.search(rf"^int {name}\(nx_network_t\* h,", text, re.M), name
    # the argument lists: nx_batch_solve's with maxit after rtol; nx_batch_rhs's
    sig = _lib._SIGS
    solve, ref = sig["nx_fe_batch_solve"][1], sig["nx_batch_solve"][1]
    assert len(solve) == len(ref) + 1 and solve[:6] == ref[:6] and solve[7:] == ref[6:]
    assert sig["nx_fe_batch_rhs"] == sig["nx_batch_rhs"]
    assert sig["nx_fe_batch_supported"] == sig["nx_batch_supported"]
    decl = re.search(r"^int nx_fe_batch_solve\(([^;]*)\);", text, re.M | re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == [
        "h", "n_cols", "edge_bc", "edge_f", "f_const", "rtol", "maxit", "order", "out", "iters",
        "relres", "converged"]


def test_keyword():
    p = inspect.signature(Solver.__init__).parameters["batch_degrees"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


@pytest.mark.parametrize("value,on", [(None, False), ("1", True), ("0", False), ("", False),
                                      ("true", False)])
def test_env_switch_is_read_when_the_keyword_is_none(monkeypatch, value, on):
    if value is None:
        monkeypatch.delenv("NXHIP_FE_BATCH", raising=False)
    else:
        monkeypatch.setenv("NXHIP_FE_BATCH", value)
    assert Solver(_StubAssembler())._fe_batch is on
    # given, the keyword decides and the environment is not consulted
    assert Solver(_StubAssembler(), batch_degrees=True)._fe_batch is True
    assert Solver(_StubAssembler(), batch_degrees=False)._fe_batch is False


def test_stored_per_solver(monkeypatch):
    monkeypatch.setenv("NXHIP_FE_BATCH", "1")
    a = Solver(_StubAssembler())
    monkeypatch.setenv("NXHIP_FE_BATCH", "0")
    b = Solver(_StubAssembler())
    assert a._fe_batch is True and b._fe_batch is False
