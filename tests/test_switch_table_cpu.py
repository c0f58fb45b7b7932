"""The switch surface as host state (no GPU): tests/switch_table.py against r3g_set_option's source, against a fresh process's
defaults, and every value through r3g_set_option / r3g_get_option and back."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

import switch_table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def option_names_in_source():
    """the names r3g_set_option accepts, as the library enumerates them (r3g_option_name), like tests/test_abi.py does"""
    from r3g import ffi
    L, names = ffi.lib(), []
    while L.r3g_option_name(len(names)) is not None:
        names.append(L.r3g_option_name(len(names)).decode())
    assert len(names) == len(set(names)) and len(names) >= 50
    return names


@pytest.fixture(scope="module")
def lib():
    from r3g import ffi
    return ffi.lib(), ffi


def test_the_table_has_one_row_per_option():
    names = option_names_in_source()
    assert sorted(names) == sorted(T.ROWS), (sorted(set(names) - set(T.ROWS)), sorted(set(T.ROWS) - set(names)))
    for n, r in T.ROWS.items():
        assert r["default"] not in r["alternates"] and len(r["alternates"]) >= 1, n
        assert set(r["stages"]) <= set(T.STAGES), n
        assert all(p in ("bits", "tol") for p in ([r["promise"]] if isinstance(r["promise"], str) else r["promise"].values())), n
        assert r.get("excluded") or r["stages"], n                 # a row that runs nowhere says why
        for stage_alts in r.get("stages_by_alt", {}).values():
            assert set(stage_alts) <= set(r["stages"]), n
        for w in r.get("with_", {}):
            assert w in T.ROWS and w != n, n


def test_a_fresh_process_reports_the_defaults():
    """r3g_get_option in a child process that has set nothing (the environment's R3G_OPTIONS hook included)"""
    code = ("import ctypes, json, sys\n"
            "sys.path[:0] = %r\n"
            "from r3g import ffi\n"
            "import switch_table as T\n"
            "L = ffi.lib()\n"
            "print(json.dumps({n: T.get_option(L, ffi, n) for n in T.ROWS}))\n"
            % [os.path.join(ROOT, "3d-re-gen_amd"), os.path.join(ROOT, "tests"), ROOT])
    env = {k: v for k, v in os.environ.items() if k != "R3G_OPTIONS"}
    out = subprocess.run([sys.executable, "-c", code], env=env, check=True, capture_output=True, text=True).stdout
    got = json.loads(out.strip().splitlines()[-1])
    wrong = {n: (got[n], r["default"]) for n, r in T.ROWS.items() if got[n] != r["default"]}
    assert not wrong, "option: (fresh process, table default) %s" % wrong


def test_unknown_names_and_null_arguments_are_refused(lib):
    L, ffi = lib
    v = ctypes.c_int(77)
    assert L.r3g_get_option(b"no_such_option", ctypes.byref(v)) == -1 and v.value == 77       # R3G_ERR_INVALID
    assert L.r3g_get_option(b"geo_kv_nothing", ctypes.byref(v)) == -1
    assert L.r3g_get_option(None, ctypes.byref(v)) == -1 and L.r3g_get_option(b"lds_dma", None) == -1


@pytest.mark.parametrize("name", sorted(T.ROWS))
def test_set_get_restore(lib, name):
    L, ffi = lib
    row = T.ROWS[name]
    old = T.get_option(L, ffi, name)
    try:
        for alt in row["alternates"]:
            T.set_option(L, ffi, name, alt)
            assert T.get_option(L, ffi, name) == alt, (name, alt)
            for bad in row.get("refused", ()):                       # refused or ignored: what was set stays in force
                L.r3g_set_option(name.encode(), bad)
                assert T.get_option(L, ffi, name) == alt, (name, alt, bad)
            T.set_option(L, ffi, name, old)
            assert T.get_option(L, ffi, name) == old, name
            with T.switched(L, ffi, **{name: alt}):
                assert T.get_option(L, ffi, name) == alt
            assert T.get_option(L, ffi, name) == old
    finally:
        T.set_option(L, ffi, name, old)


def test_switched_restores_when_the_body_raises(lib):
    L, ffi = lib
    before = {n: T.get_option(L, ffi, n) for n in ("gemm_num_cu", "gemm_phased", "flow_last_step")}
    with pytest.raises(RuntimeError):
        with T.switched(L, ffi, gemm_num_cu=8, gemm_phased=0, flow_last_step=3):
            assert T.get_option(L, ffi, "gemm_num_cu") == 8 and T.get_option(L, ffi, "flow_last_step") == 3
            raise RuntimeError("body")
    assert {n: T.get_option(L, ffi, n) for n in before} == before


def test_staging_reads_back_as_lds_dma(lib):
    """r3g_set_staging and "lds_dma" are one switch; it reads 1 only while both kernel families stage through LDS-DMA"""
    L, ffi = lib
    try:
        ffi.check(L.r3g_set_staging(0))
        assert T.get_option(L, ffi, "lds_dma") == 0
        ffi.check(L.r3g_set_staging(1))
        assert T.get_option(L, ffi, "lds_dma") == 1
    finally:
        ffi.check(L.r3g_set_staging(1))


def test_kernel_choice_counters_exist_and_start_readable(lib):
    """every counter the table names is one r3g_get_counter knows and include/r3g.h lists"""
    L, ffi = lib
    hdr = open(os.path.join(ROOT, "include", "r3g.h")).read()
    doc = hdr[hdr.index("/* Process-wide event counters"):hdr.index("int r3g_get_counter(")]
    names = sorted({c[0] for r in T.ROWS.values() for c in r.get("counter", ())})
    assert len(names) >= 20
    for n in names:
        assert T.get_counter(L, ffi, n) >= 0
        assert '"%s"' % n in doc, "counter without documentation in include/r3g.h: " + n
    listed = []
    while L.r3g_counter_name(len(listed)) is not None:
        listed.append(L.r3g_counter_name(len(listed)).decode())
    assert set(names) <= set(listed)
    for n in listed:                                            # every counter the library enumerates, not only the table's
        assert '"%s"' % n in doc, "counter without documentation in include/r3g.h: " + n
    v = ctypes.c_int64(0)
    assert L.r3g_get_counter(b"no_such_counter", ctypes.byref(v)) == -1
