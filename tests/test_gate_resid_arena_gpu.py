"""GPU tests (-m gpu): the memory contract of the C ABI for the three entries of the residual (+ ReLU) epilogue of SELayer / ECALayer /
CBAM.  The rows are tests/gate_resid_arena_rows.py; the three runs per row (plain, poisoned arena, junk workspaces) are those of
tests/test_abi_memory_gpu.py, whose function and arena fixture are used as they are."""
import pytest

import gate_resid_arena_rows
from test_abi_memory_gpu import arena  # noqa: F401  (fixture)
from test_abi_memory_gpu import test_entry_keeps_the_memory_contract as _contract

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rid", gate_resid_arena_rows.IDS)
def test_gate_resid_entry_keeps_the_memory_contract(rid, arena, monkeypatch):  # noqa: F811
    _contract(rid, arena, monkeypatch)
