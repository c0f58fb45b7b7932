#!/usr/bin/env python3
"""Build libr3g.so (HIP kernels + C ABI) for gfx950, in-tree, with hipcc.

    python 3d-re-gen_amd/build.py [--force]

Each translation unit is compiled to build/<name>.o and linked into 3d-re-gen_amd/libr3g.so.
mc_kernels.hip is compiled with -ffp-contract=off (its fp64 ambiguity tests and interpolation must
reproduce the sequential reference bit-for-bit), dmc_kernels.hip likewise (its positions are fixed to the bit; surf_compact_kernels.hip, the scan and workspace the two share, holds integers only and needs no flag), meshdist_kernels.hip (its distances equal the host twin's) meshinside_kernels.hip (its crossing counts equal the host twin's), meshfit_kernels.hip (its float64 sums equal the host twin's), meshtopo_kernels.hip (its quantised volumes equal the host twin's), meshfill_kernels.hip (its centroids equal the host twin's), recon_kernels.hip (its lattices equal the host twin's), orient_kernels.hip (its edge weights equal the host twin's), dbscan_kernels.hip (its float64 neighbour predicate equals the host twin's), plane_kernels.hip (its float64 inlier test and sums equal the host twin's), softras_kernels.hip (its float32 fragments, sigmoids and gradient sums equal the host twin's), facecloud_kernels.hip (its point-triangle distances, weights and gradient sums equal the host twin's), cloud_kernels.hip (its squared distances equal the host twin's; grid_csr_kernels.hip, the workspace layout that meshdist, meshinside and cloud share, and scan_kernels.hip, the exclusive scan that they, the cleaners and meshfill share, hold integers only and need no flag) and r3g_api.cpp (it holds the registration's host solver, csrc/meshfit_core.h, which the twin shares, and the plane fit's eigen solver, csrc/plane_core.h, likewise); the MFMA kernels keep hipcc's default contraction.
hipcc cross-compiles without a GPU, so this also runs in the CPU-only build container.

Staleness is decided by CONTENT, not by mtimes: build/manifest.json records, per object, the SHA-256 of its source,
of every header it can include and of the compile flags, and for the library the hashes of all objects' inputs.
A snapshot that carries a prebuilt .so from different sources is therefore rebuilt, and `source_digest()` lets the
tests assert that the library they loaded was built from the sources next to it (tests/test_abi.py).
"""
import hashlib
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INC = os.path.join(os.path.dirname(HERE), "include")
OBJ = os.path.join(HERE, "build")
OUT = os.path.join(HERE, "libr3g.so")
MANIFEST = os.path.join(OBJ, "manifest.json")
STAMP = os.path.join(HERE, "libr3g.digest")     # travels with the .so (the GPU box gets both)
ARCH = "gfx950"
COMMON = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-Wno-missing-braces", "-I" + INC, "-I" + CSRC]
PER_FILE = {"mc_kernels.hip": ["-ffp-contract=off"], "dmc_kernels.hip": ["-ffp-contract=off"], "tex_kernels.hip": ["-ffp-contract=off"],
            "meshdist_kernels.hip": ["-ffp-contract=off"], "meshinside_kernels.hip": ["-ffp-contract=off"],
            "meshfit_kernels.hip": ["-ffp-contract=off"], "meshtopo_kernels.hip": ["-ffp-contract=off"],
            "meshfill_kernels.hip": ["-ffp-contract=off"], "cloud_kernels.hip": ["-ffp-contract=off"], "facecloud_kernels.hip": ["-ffp-contract=off"], "dbscan_kernels.hip": ["-ffp-contract=off"], "plane_kernels.hip": ["-ffp-contract=off"], "softras_kernels.hip": ["-ffp-contract=off"], "recon_kernels.hip": ["-ffp-contract=off"], "orient_kernels.hip": ["-ffp-contract=off"], "r3g_api.cpp": ["-ffp-contract=off"]}


def sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp")))


def _sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        h.update(f.read())
    return h.hexdigest()


def _headers_digest():
    h = hashlib.sha256()
    for d in (CSRC, INC):
        for f in sorted(os.listdir(d)):
            if f.endswith(".h"):
                h.update(f.encode())
                h.update(_sha(os.path.join(d, f)).encode())
    return h.hexdigest()


def _unit_key(src, hdr):
    flags = " ".join(COMMON[:5] + PER_FILE.get(src, []))      # without the absolute -I paths
    return hashlib.sha256((_sha(os.path.join(CSRC, src)) + hdr + flags).encode()).hexdigest()


def source_digest():
    """digest of everything libr3g.so is built from (sources, headers, flags)"""
    hdr = _headers_digest()
    return hashlib.sha256("".join(_unit_key(s, hdr) for s in sources()).encode()).hexdigest()


def built_digest():
    try:
        with open(STAMP) as f:
            return f.read().strip()
    except OSError:
        return None


def _load_manifest():
    try:
        with open(MANIFEST) as f:
            return json.load(f)
    except (OSError, ValueError):
        return {}


def _compile(src, key, old, force):
    obj = os.path.join(OBJ, os.path.splitext(src)[0] + ".o")
    if not force and os.path.exists(obj) and old.get(src) == key:
        return obj, False
    cmd = ["hipcc"] + COMMON + PER_FILE.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", obj]
    subprocess.check_call(cmd)
    return obj, True


def build(force=False, verbose=True):
    os.makedirs(OBJ, exist_ok=True)
    old = _load_manifest()
    hdr = _headers_digest()
    keys = {s: _unit_key(s, hdr) for s in sources()}
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        res = list(ex.map(lambda s: _compile(s, keys[s], old.get("units", {}), force), sources()))
    objs = [o for o, _ in res]
    digest = source_digest()
    if any(ch for _, ch in res) or not os.path.exists(OUT) or built_digest() != digest:
        subprocess.check_call(["hipcc", "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", OUT] + objs)
        with open(STAMP, "w") as f:
            f.write(digest + "\n")
        if verbose:
            print("linked", OUT)
    elif verbose:
        print("up to date:", OUT)
    with open(MANIFEST, "w") as f:
        json.dump({"units": keys, "library": digest}, f, indent=1)
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
