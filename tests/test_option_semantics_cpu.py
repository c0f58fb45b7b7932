"""The switch and counter surface, value by value, against tests/golden/option_semantics.json: what r3g_set_option returned and
r3g_get_option read back for every (name, probe) in the library BEFORE the option table (csrc/options.h) existed, recorded by
tools/record_option_semantics.py.  Host state only: no GPU."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import switch_table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "option_semantics.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    from r3g import ffi
    return ffi.lib(), ffi


def enumerate_names(fn):
    names = []
    while fn(len(names)) is not None:
        names.append(fn(len(names)).decode())
        assert len(names) < 1000
    return names


def test_the_golden_file_covers_the_switch_table(golden):
    assert sorted(golden["options"]) == sorted(T.ROWS)
    assert len(golden["counters"]) == 54
    for name, probes in golden["options"].items():
        assert [int(p) for p in probes] == golden["probes"], name


@pytest.mark.parametrize("name", sorted(T.ROWS))       # = the file's names (test_the_golden_file_covers_the_switch_table)
def test_every_probe_is_taken_as_before(lib, golden, name):
    L, ffi = lib
    default = T.ROWS[name]["default"]
    v = ctypes.c_int(0)
    try:
        for probe, (rc, back) in golden["options"][name].items():
            assert L.r3g_set_option(name.encode(), default) == 0
            got_rc = L.r3g_set_option(name.encode(), int(probe))
            assert L.r3g_get_option(name.encode(), ctypes.byref(v)) == 0
            assert (got_rc, v.value) == (rc, back), (name, probe)
    finally:
        assert L.r3g_set_option(name.encode(), default) == 0
    assert T.get_option(L, ffi, name) == default


def test_the_enumerators_list_exactly_the_recorded_names(lib, golden):
    L, ffi = lib
    options = enumerate_names(L.r3g_option_name)
    counters = enumerate_names(L.r3g_counter_name)
    assert len(set(options)) == len(options) and sorted(options) == sorted(golden["options"])
    assert len(set(counters)) == len(counters) and sorted(counters) == sorted(golden["counters"])
    assert L.r3g_option_name(-1) is None and L.r3g_option_name(len(options)) is None
    assert L.r3g_counter_name(-1) is None and L.r3g_counter_name(len(counters)) is None


def test_every_counter_reads_as_recorded_in_a_fresh_process(golden):
    """return code and value of r3g_get_counter in a child process that has done nothing else (this one may have moved some)"""
    code = ("import ctypes, json, sys\n"
            "sys.path[:0] = %r\n"
            "from r3g import ffi\n"
            "L, v, out = ffi.lib(), ctypes.c_int64(-1), {}\n"
            "for n in %r:\n"
            "    rc = L.r3g_get_counter(n.encode(), ctypes.byref(v))\n"
            "    out[n] = [rc, v.value]\n"
            "print(json.dumps(out))\n"
            % ([os.path.join(ROOT, "3d-re-gen_amd"), ROOT], sorted(golden["counters"])))
    env = {k: v for k, v in os.environ.items() if k != "R3G_OPTIONS"}
    out = subprocess.run([sys.executable, "-c", code], env=env, check=True, capture_output=True, text=True).stdout
    assert json.loads(out.strip().splitlines()[-1]) == golden["counters"]
