"""GPU tests (-m gpu): the memory contract of the C ABI for mi355_linear16_res_scale_fwd, mi355_linear16_stats_r16_fwd and
mi355_mlp_fused_o16_fwd.  The rows are tests/xcit_io16_arena_rows.py; the three runs per row (plain, poisoned arena, junk workspaces)
are those of tests/test_abi_memory_gpu.py, whose function and arena fixture are used as they are."""
import pytest

import xcit_io16_arena_rows
from test_abi_memory_gpu import arena  # noqa: F401  (fixture)
from test_abi_memory_gpu import test_entry_keeps_the_memory_contract as _contract

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rid", xcit_io16_arena_rows.IDS)
def test_xcit16_entry_keeps_the_memory_contract(rid, arena, monkeypatch):  # noqa: F811
    _contract.__wrapped__(rid, arena, monkeypatch) if hasattr(_contract, "__wrapped__") else _contract(rid, arena, monkeypatch)
