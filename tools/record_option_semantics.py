#!/usr/bin/env python3
"""Record what r3g_set_option / r3g_get_option / r3g_get_counter do, value by value, into tests/golden/option_semantics.json.

    python tools/record_option_semantics.py [--library path/to/libr3g.so] [--out file]

The file is the behaviour of the library it was recorded FROM (the commit before the option table, csrc/options.h, existed), and
tests/test_option_semantics_cpu.py replays it against the library of the tree: it is not regenerated when the table changes.
No GPU is needed: the switches are host state and no counter has moved in a fresh process.

For every name of tests/switch_table.py's ROWS and every probe value, in ONE child process that starts with the defaults (the
environment's R3G_OPTIONS hook removed): set the table's default, set the probe, record r3g_set_option's return code and what
r3g_get_option reports, restore the default.  For every counter: r3g_get_counter's return code and value.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-re-gen_amd"), os.path.join(ROOT, "tests")]

PROBES = [-2, -1, 0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 13, 16, 32, 100, 256, 1024, 8192, 65536, 1 << 30]
# the public counter names of include/r3g.h ("Process-wide event counters")
COUNTERS = [
    "dit_f16_fallbacks", "dit_groups", "dit_evals", "geo_q_cache_builds", "geo_kv_groups", "geo_narrow_passes", "geo_lnf_passes",
    "geo_lnd_passes", "device_bytes_live",
    "meshdist_tests", "meshinside_tests", "meshfit_steps", "meshtopo_builds", "meshtopo_rounds", "meshfill_plans", "meshfill_rounds",
    "cloud_tests", "orient_rounds", "dbscan_launches", "dbscan_tests", "recon_solves", "recon_cycles",
    "gemm_w4_128", "gemm_w8_128", "gemm_w16_256", "gemm_two_stage_256", "gemm_256x128", "gemm_phased", "gemm_phased_persistent",
    "gemm_mixed", "gemm_splitk2", "gemm_splitk128", "gemm_deep_ring", "gemm_conv_implicit", "gemm_register_staged", "gemm_fp8",
    "attn_gen1", "attn_pipelined", "attn_gen2", "attn_gen3", "attn_gen4", "attn_gen5", "attn_gen6", "attn_gen9", "attn_register_staged",
    "ln_rows1", "ln_rows4", "ln_fixed_count", "ln_mode_inst", "mc_rows4", "mc_rows8", "mc_rows16", "mc_rows32", "mc_deferred_rows"]


def record():
    """runs in the child: {"options": {name: {probe: [return code, read-back]}}, "counters": {name: [return code, value]}}"""
    import switch_table as T
    from r3g import ffi
    L = ffi.lib()

    def get(name):
        v = ctypes.c_int(0)
        assert L.r3g_get_option(name.encode(), ctypes.byref(v)) == 0, name
        return int(v.value)

    options = {}
    for name, row in T.ROWS.items():
        assert get(name) == row["default"], name
        options[name] = {}
        for probe in PROBES:
            assert L.r3g_set_option(name.encode(), row["default"]) == 0, name
            rc = L.r3g_set_option(name.encode(), probe)
            options[name][str(probe)] = [int(rc), get(name)]
            assert L.r3g_set_option(name.encode(), row["default"]) == 0 and get(name) == row["default"], name
    counters = {}
    for name in COUNTERS:
        v = ctypes.c_int64(-1)
        rc = L.r3g_get_counter(name.encode(), ctypes.byref(v))
        counters[name] = [int(rc), int(v.value)]
    return {"options": options, "counters": counters}


def dump(rec):
    """one line per name, names sorted: a diff of the file reads as a diff of the behaviour"""
    out = ['{"probes": %s,' % json.dumps(PROBES), ' "options": {']
    names = sorted(rec["options"])
    for i, n in enumerate(names):
        out.append('  %s: %s%s' % (json.dumps(n), json.dumps(rec["options"][n]), "," if i + 1 < len(names) else ""))
    out.append(' },')
    out.append(' "counters": %s}' % json.dumps(rec["counters"], sort_keys=True))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--library", help="the libr3g.so to record (default: the tree's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "option_semantics.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(record()))
        return
    env = {k: v for k, v in os.environ.items() if k != "R3G_OPTIONS"}
    if a.library:
        env["R3G_LIBRARY"] = os.path.abspath(a.library)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True, capture_output=True, text=True).stdout
    rec = json.loads(out.strip().splitlines()[-1])
    assert len(rec["counters"]) == len(set(COUNTERS)) == 54
    with open(a.out, "w") as f:
        f.write(dump(rec))
    print("recorded %d options x %d probes, %d counters -> %s" % (len(rec["options"]), len(PROBES), len(rec["counters"]), a.out))


if __name__ == "__main__":
    main()
