"""CPU tests of the option surface: csrc/options.h is the one list (key, default, range), mi355attn.options() the one scoped setter.

The library loads without a GPU (the current device is then ordinal 0).  Expected keys, defaults and ranges are parsed out of the
header, never read back from the library.
"""
import os
import re
import subprocess
import sys

import pytest

from conftest import PKG

_INT = r"\s*(-?\d+)L?(?:\s*<<\s*(\d+))?\s*"
_ROW = re.compile(r'^MI355_OPT\(\s*([A-Z0-9_]+)\s*,\s*"([a-z0-9_]+)"\s*,' + _INT + "," + _INT + "," + _INT + r"\)", flags=re.M)


def _header_rows():
    """[(identifier, key, default, low, high)] in list order."""
    src = open(os.path.join(PKG, "csrc", "options.h")).read()
    rows = []
    for m in _ROW.finditer(src):
        g = m.groups()
        vals = [int(g[i]) << int(g[i + 1] or 0) for i in (2, 4, 6)]
        rows.append((g[0], g[1], *vals))
    assert len(rows) == len(re.findall(r"^MI355_OPT\(", src, flags=re.M)), "a list line the test's pattern does not read"
    return rows


def test_list_header_is_well_formed():
    rows = _header_rows()
    assert len(rows) >= 30
    assert len({r[0] for r in rows}) == len(rows) and len({r[1] for r in rows}) == len(rows), "duplicate identifier or key"
    for ident, key, d, lo, hi in rows:
        assert ident == key.upper(), f"O_{ident} is not named after its key '{key}'"
        assert lo <= d <= hi, f"{key}: default {d} outside {lo} .. {hi}"


def test_defaults_in_a_fresh_process_are_the_headers(built_lib):
    """A process that has set nothing reads the header's defaults (raw ctypes: the binding itself sets a default at load time)."""
    rows = _header_rows()
    code = ("import sys, ctypes, torch\n"
            "lib = ctypes.CDLL(sys.argv[1])\n"
            "lib.mi355_get_option.restype = ctypes.c_long\n"
            "lib.mi355_get_option.argtypes = [ctypes.c_char_p]\n"
            "print(' '.join(str(lib.mi355_get_option(k.encode())) for k in sys.argv[2:]))\n")
    r = subprocess.run([sys.executable, "-c", code, built_lib] + [k for _, k, *_ in rows], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(v) for v in r.stdout.split()]
    assert got == [d for _, _, d, _, _ in rows], dict(zip((k for _, k, *_ in rows), got))


def test_every_key_round_trips_over_its_range(built_lib):
    import mi355attn
    for _, key, d, lo, hi in _header_rows():
        for v in (lo, hi, d):
            with mi355attn.options(**{key: v}):
                assert mi355attn.get_option(key) == v, key
        for v in (lo - 1, hi + 1):
            if key == "spin_limit" and v == 0:
                continue
            before = mi355attn.get_option(key)
            with pytest.raises(mi355attn.Mi355Error, match=key):
                with mi355attn.options(**{key: v}):
                    pass
            assert mi355attn.get_option(key) == before, key
    with mi355attn.options(spin_limit=0):                                 # the one value accepted outside a range (forces the time-out path)
        assert mi355attn.get_option("spin_limit") == 0
    with pytest.raises(mi355attn.Mi355Error, match="spin_limit"):
        with mi355attn.options(spin_limit=1023):
            pass


def test_options_scopes_and_restores(built_lib):
    import mi355attn
    nt, rev = mi355attn.get_option("nt"), mi355attn.get_option("reverse")
    with mi355attn.options():                                             # no keys: nothing happens
        assert (mi355attn.get_option("nt"), mi355attn.get_option("reverse")) == (nt, rev)
    with mi355attn.options(nt=1, reverse=1):
        assert (mi355attn.get_option("nt"), mi355attn.get_option("reverse")) == (1, 1)
    assert (mi355attn.get_option("nt"), mi355attn.get_option("reverse")) == (nt, rev)
    with pytest.raises(ZeroDivisionError):
        with mi355attn.options(nt=2, reverse=1):
            assert mi355attn.get_option("nt") == 2
            1 / 0
    assert (mi355attn.get_option("nt"), mi355attn.get_option("reverse")) == (nt, rev)


def test_nested_options_restore_in_order(built_lib):
    import mi355attn
    nt = mi355attn.get_option("nt")
    with mi355attn.options(nt=0):
        with mi355attn.options(nt=1, chunk_images=5):
            with mi355attn.options(nt=2):
                assert mi355attn.get_option("nt") == 2
            assert (mi355attn.get_option("nt"), mi355attn.get_option("chunk_images")) == (1, 5)
        assert mi355attn.get_option("nt") == 0
    assert mi355attn.get_option("nt") == nt


def test_a_refused_key_leaves_the_others_as_they_were(built_lib):
    import mi355attn
    keys = ("nt", "chunk_images", "reverse")
    before = [mi355attn.get_option(k) for k in keys]
    ran = []
    with pytest.raises(mi355attn.Mi355Error, match="no_such_key"):
        with mi355attn.options(nt=1, chunk_images=9, no_such_key=1, reverse=1):
            ran.append(1)
    assert not ran, "the body ran although a key was refused"
    assert [mi355attn.get_option(k) for k in keys] == before
    with pytest.raises(mi355attn.Mi355Error, match="nt"):                  # a value out of range, after a valid key
        with mi355attn.options(chunk_images=9, nt=4):
            ran.append(1)
    assert not ran and [mi355attn.get_option(k) for k in keys] == before
