#!/usr/bin/env python3
"""Times the mesh topology build and fix_normals (include/r3g.h r3g_meshtopo_build / r3g_meshtopo_orient)
on the 257^3 sphere (golden D of tests/mc_volumes.py: 376 760 faces) and the 257^3 blob (the field of tools/bench_mc.py:
226 244 faces), both by the product's marching cubes, and prints the topology report of the blob after each surface generator
and cleaner of the stage.  One JSON line, and with --write a table in profiles/meshtopo.md:
  ms_build        median and min over --reps after a warm-up, HIP events on the stream (one call with its read-backs)
  ms_fix_normals  the same for r3g_meshtopo_orient with outward = 2 on a copy wound inward (every face is reversed: two builds
                  and the apply) and on its own output (nothing to do: one build and the apply)
  rounds          label rounds of one build (counter "meshtopo_rounds")
  ms_numpy        the numpy / scipy restatement (tests/meshtopo_ref.py) of the same build on the host, once, for scale
No time is asserted anywhere.

    python tools/bench_meshtopo.py [--reps 7] [--n 257] [--budget 40000] [--no-numpy] [--meshes sphere blob] [--no-stages] [--write [PATH]]

--write replaces only what stands between the two marker lines of the file; text written by hand outside them is kept.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-re-gen_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

COUNTS = ("usable", "skipped", "vref", "edges", "boundary", "clash", "nonmanifold", "bodies", "unorientable", "euler", "nonfinite")


def blob(n):
    """smooth closed surface (union of a few spheres), the field of tools/bench_mc.py"""
    ax = torch.linspace(-1, 1, n)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    f = torch.full((n, n, n), -1.0)
    for cx, cy, cz, r in ((0, 0, 0, .55), (.35, .2, .1, .35), (-.3, -.25, .2, .3), (.1, -.4, -.3, .28)):
        f = torch.maximum(f, r - torch.sqrt((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2))
    return f.contiguous()


def sphere(n):
    i = torch.arange(n, dtype=torch.int64) - n // 2
    r2 = (i ** 2)[:, None, None] + (i ** 2)[None, :, None] + (i ** 2)[None, None, :]
    return ((100 * 100 * (n // 2) ** 2) // (128 * 128) - r2).to(torch.float32).contiguous()       # n = 257: 10000 - rho^2


def timed(fn):
    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b.record()
    out = fn()
    e.record()
    e.synchronize()
    return b.elapsed_time(e), out


def med(ms):
    return {"median": statistics.median(ms), "min": min(ms)}


def measure(v, f, reps, numpy_too):
    from r3g import ffi, meshtopo
    meshtopo.build(v, f)                                          # warm-up: workspace, code objects
    inward = f.flip(1).contiguous() if meshtopo.report(0)["six_volume_q"] > 0 else f
    meshtopo.fix_normals(v, inward.clone())
    torch.cuda.synchronize()
    ms_b, ms_fix, ms_noop, rounds = [], [], [], 0
    for _ in range(max(1, reps)):
        r0 = ffi.counter("meshtopo_rounds")
        t, rep = timed(lambda: meshtopo.build(v, f))
        ms_b.append(t)
        rounds = ffi.counter("meshtopo_rounds") - r0
        work = inward.clone()
        t, (fixed, info) = timed(lambda: meshtopo.fix_normals(v, work))
        ms_fix.append(t)
        assert info["faces_reversed"] == f.shape[0]
        t, (_, info) = timed(lambda: meshtopo.fix_normals(v, fixed))
        ms_noop.append(t)
        assert info["faces_reversed"] == 0
    out = {"verts": int(v.shape[0]), "faces": int(f.shape[0]), "rounds": rounds, "ms_build": med(ms_b),
           "ms_fix_normals_all": med(ms_fix), "ms_fix_normals_none": med(ms_noop),
           "report": {k: rep[k] for k in COUNTS + ("volume", "area", "watertight", "winding_consistent")}}
    if numpy_too:
        import meshtopo_ref
        hv, hf = v.cpu().numpy(), f.cpu().numpy()
        t0 = time.perf_counter()
        r = meshtopo_ref.build(hv, hf)
        out["ms_numpy"] = 1e3 * (time.perf_counter() - t0)
        out["numpy_agrees"] = all(r["report"][k] == rep[k] for k in COUNTS)
    return out


def stage_reports(n, budget):
    """the blob's report after each generator / cleaner of the stage"""
    from r3g import dmc, mc, meshops, meshtopo
    vol = blob(n).cuda()
    v, f = mc.marching_cubes(vol, 0.0)
    steps = [("marching cubes", (v, f)), ("dual marching cubes", dmc.dual_marching_cubes(vol, 0.0))]
    fv, ff = meshops.remove_floaters(v, f, 0.02)
    steps.append(("remove_floaters(0.02)", (fv, ff)))
    steps.append(("reduce_faces(%d)" % budget, meshops.reduce_faces(fv, ff, budget)))
    steps.append(("cluster_faces(%d)" % budget, meshops.cluster_faces(fv, ff, budget)))
    out = []
    for name, (sv, sf) in steps:
        rep = meshtopo.build(sv.contiguous(), sf.contiguous())
        out.append({"step": name, **{k: rep[k] for k in COUNTS + ("volume", "area", "watertight", "winding_consistent")}})
    return out


BEGIN, END = "<!-- bench_meshtopo.py --write: begin (generated; edit outside the markers) -->", "<!-- bench_meshtopo.py --write: end -->"


def write_profile(path, out):
    """the generated tables go between the BEGIN / END markers of `path`; what is written by hand outside them stays"""
    rows = [BEGIN, "",
            "Tool: `python tools/bench_meshtopo.py --write` (HIP events on the stream; medians over %d repetitions after a warm-up;" % out["reps"],
            "meshes by the product's marching cubes at %d³).  `fix_normals, all` starts from the mesh wound inward (every face is" % out["n"],
            "reversed: two builds and the apply), `fix_normals, none` from its output (one build and the apply).  `numpy` is the",
            "restatement of tests/meshtopo_ref.py on the host, once.  Yardstick for scale: §4g builds its column table of the same",
            "class of mesh in 0.47 ms (profiles/meshinside.md).", "", "## Recorded run", "",
            "| mesh | faces | build ms (median / min) | rounds | fix_normals, all ms (median / min) | fix_normals, none ms (median / min) | numpy ms |",
            "|---|---|---|---|---|---|---|"]
    for name in out["meshes"]:
        r = out[name]
        rows.append("| %s | %d | %.3f / %.3f | %d | %.3f / %.3f | %.3f / %.3f | %s |" % (
            name, r["faces"], r["ms_build"]["median"], r["ms_build"]["min"], r["rounds"], r["ms_fix_normals_all"]["median"],
            r["ms_fix_normals_all"]["min"], r["ms_fix_normals_none"]["median"], r["ms_fix_normals_none"]["min"],
            "%.0f" % r["ms_numpy"] if "ms_numpy" in r else "-"))
    if out.get("stages"):
        rows += ["", "## The blob after each step of the stage", "",
                 "| step | faces | V_ref | E | χ | boundary | clash | non-manifold | bodies | unorientable | skipped | watertight | volume |",
                 "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for s in out["stages"]:
            rows.append("| %s | %d | %d | %d | %d | %d | %d | %d | %d | %d | %d | %s | %.6f |" % (
                s["step"], s["usable"], s["vref"], s["edges"], s["euler"], s["boundary"], s["clash"], s["nonmanifold"], s["bodies"],
                s["unorientable"], s["skipped"], s["watertight"], s["volume"]))
    rows += ["", END]
    block = "\n".join(rows)
    try:
        with open(path) as fh:
            old = fh.read()
    except OSError:
        old = "# Mesh topology (DESIGN.md §4i): timings and what the stage's meshes look like\n\n" + BEGIN + "\n" + END + "\n"
    if BEGIN not in old or END not in old:
        raise SystemExit("%s has no bench_meshtopo.py markers: refusing to overwrite it" % path)
    with open(path, "w") as fh:
        fh.write(old[:old.index(BEGIN)] + block + old[old.index(END) + len(END):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=257, help="side of the volumes")
    ap.add_argument("--budget", type=int, default=40000)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--meshes", nargs="+", default=["sphere", "blob"], choices=["sphere", "blob"])
    ap.add_argument("--no-stages", action="store_true", help="skip the blob's reports after each step of the stage")
    ap.add_argument("--write", nargs="?", const=os.path.join(ROOT, "profiles", "meshtopo.md"), default=None,
                    help="write the tables (default path: profiles/meshtopo.md)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meshtopo.py needs an MI355X (the product has no CPU path)")
    from r3g import ffi, mc
    out = {"bench": "meshtopo", "n": a.n, "reps": a.reps, "meshes": a.meshes}
    with ffi.device_lock(0):
        for name in a.meshes:
            vol, level = (sphere(a.n), 0.5) if name == "sphere" else (blob(a.n), 0.0)
            v, f = mc.marching_cubes(vol.cuda(), level)
            out[name] = measure(v.contiguous(), f.contiguous(), a.reps, not a.no_numpy)
        if not a.no_stages:
            out["stages"] = stage_reports(a.n, a.budget)
    print(json.dumps(out), flush=True)
    if a.write:
        write_profile(a.write, out)


if __name__ == "__main__":
    main()
