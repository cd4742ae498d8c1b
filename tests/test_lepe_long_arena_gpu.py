"""GPU tests (-m gpu): the memory contract of the C ABI for the three LePE entries at stripe windows above 224 tokens (the long-window
kernel of csrc/attn.hip).  The rows are tests/lepe_long_arena_rows.py; the three runs per row (plain, poisoned arena, junk workspaces)
are those of tests/test_abi_memory_gpu.py, whose function and arena fixture are used as they are."""
import pytest

import lepe_long_arena_rows
from test_abi_memory_gpu import arena  # noqa: F401  (fixture)
from test_abi_memory_gpu import test_entry_keeps_the_memory_contract as _contract

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rid", lepe_long_arena_rows.IDS)
def test_lepe_long_entry_keeps_the_memory_contract(rid, arena, monkeypatch):  # noqa: F811
    _contract.__wrapped__(rid, arena, monkeypatch) if hasattr(_contract, "__wrapped__") else _contract(rid, arena, monkeypatch)
