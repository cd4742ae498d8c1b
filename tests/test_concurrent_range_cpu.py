"""CPU tests: the strict re-run of range_fallback_forward (functional._forced_strict) on several threads at once.

A re-run is strict for the thread that runs it, and for nobody else: overlapping re-runs on two threads -- in either exit order, with
one module of each thread and one module shared by both -- leave the process default and every module's `precision` as they found
them, and a third thread that never re-runs keeps computing in fp16 throughout.  No GPU: the test reads the precision every op would
resolve (functional._prec) and the package default.
"""
import threading

import pytest
import torch

from mi355attn import functional as F

TIMEOUT = 10.0


class _Pinned(torch.nn.Module):
    """A module built with an explicit 16-bit `precision=` (what the re-run has to override)."""

    def __init__(self):
        super().__init__()
        self.precision = F.PREC_FP16


def _effective(m):
    return F._prec(m.precision)


@pytest.mark.parametrize("order", ["A-B-A-B", "A-B-B-A"], ids=["a_exits_first", "b_exits_first"])
def test_overlapping_strict_reruns_keep_default_and_modules(order):
    start = F.default_precision()
    assert start == F.PREC_FP16
    mods = {"A": _Pinned(), "B": _Pinned()}
    shared = _Pinned()
    for m in mods.values():
        m.shared = shared                                      # a sub-module of both threads' modules
    exits = ["A", "B"] if order == "A-B-A-B" else ["B", "A"]
    # steps: 0 A enters, 1 B enters, 2 first exit, 3 second exit; every thread hits the barrier after each step
    bar = threading.Barrier(3, timeout=TIMEOUT)
    errors, seen = [], {"A": [], "B": [], "C": []}

    def runner(name):
        try:
            ctx = F._forced_strict(mods[name])
            for step in range(4):
                if step == 0 and name == "A" or step == 1 and name == "B":
                    ctx.__enter__()
                if step >= 2 and exits[step - 2] == name:
                    ctx.__exit__(None, None, None)
                inside = (name == "A" and 0 <= step < 2 + exits.index("A")) or (name == "B" and 1 <= step < 2 + exits.index("B"))
                seen[name].append((step, inside, F.default_precision(), _effective(mods[name]), _effective(shared)))
                bar.wait()
        except Exception as e:                                 # noqa: BLE001 -- reported by the main thread
            errors.append((name, repr(e)))
            bar.abort()

    def bystander():
        try:
            other = _Pinned()
            for step in range(4):
                seen["C"].append((step, False, F.default_precision(), _effective(other), _effective(shared)))
                bar.wait()
        except Exception as e:                                 # noqa: BLE001
            errors.append(("C", repr(e)))
            bar.abort()

    threads = [threading.Thread(target=runner, args=("A",)), threading.Thread(target=runner, args=("B",)),
               threading.Thread(target=bystander)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(TIMEOUT)
        assert not t.is_alive(), "a thread did not finish"
    assert not errors, errors
    assert F.default_precision() == start, f"{order}: the process default is stuck at {F.default_precision()}"
    for m in (mods["A"], mods["B"], shared):
        assert m.precision == F.PREC_FP16, f"{order}: a module's precision attribute was left at {m.precision}"
    for name, rows in seen.items():
        assert len(rows) == 4, (name, rows)
        for step, inside, default, own, sh in rows:
            want = F.PREC_STRICT if inside else F.PREC_FP16
            assert default == (F.PREC_STRICT if inside else start), f"{order}: thread {name} step {step}: default {default}"
            assert own == want, f"{order}: thread {name} step {step}: own module runs in {own}, expected {want}"
            assert sh == want, f"{order}: thread {name} step {step}: shared module runs in {sh}, expected {want}"


def test_forced_strict_overrides_explicit_precision_and_nests():
    """Inside the context every resolution is strict -- the default, None, and an explicit 16-bit setting -- and a nested context
    exits without ending the outer one."""
    start = F.default_precision()
    with F._forced_strict(None):
        assert F._prec(None) == F._prec(F.PREC_FP16) == F._prec(F.PREC_BF16) == F.PREC_STRICT
        with F._forced_strict(None):
            assert F.default_precision() == F.PREC_STRICT
        assert F.default_precision() == F.PREC_STRICT
    assert F.default_precision() == start
    assert F._prec(F.PREC_BF16) == F.PREC_BF16 and F._prec(None) == start


def test_forced_strict_is_restored_when_the_rerun_raises():
    start = F.default_precision()
    with pytest.raises(RuntimeError):
        with F._forced_strict(None):
            raise RuntimeError("forward failed")
    assert F.default_precision() == start and F._prec(F.PREC_FP16) == F.PREC_FP16
