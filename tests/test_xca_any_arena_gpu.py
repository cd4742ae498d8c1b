"""GPU tests (-m gpu): the memory contract of the C ABI for mi355_xca_fwd, mi355_xca16_fwd and mi355_class_attn_fwd on the
run-time-width kernels (head widths 5 and 72: heads that start and end inside a 16-byte unit, a partial last row block).  The rows
are tests/xca_any_arena_rows.py; the three runs per row (plain, poisoned arena, junk workspaces) are those of
tests/test_abi_memory_gpu.py, whose function and arena fixture are used as they are."""
import pytest

import xca_any_arena_rows
from test_abi_memory_gpu import arena  # noqa: F401  (fixture)
from test_abi_memory_gpu import test_entry_keeps_the_memory_contract as _contract

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rid", xca_any_arena_rows.IDS)
def test_any_width_entry_keeps_the_memory_contract(rid, arena, monkeypatch):  # noqa: F811
    _contract.__wrapped__(rid, arena, monkeypatch) if hasattr(_contract, "__wrapped__") else _contract(rid, arena, monkeypatch)
