#!/usr/bin/env python3
"""Times the mesh fill (include/r3g.h r3g_meshfill_plan / r3g_meshfill_emit) and shows what it does to the
one open mesh the stage makes.  One JSON line, and with --write a table in profiles/meshfill.md:
  sphere          the 257^3 sphere (golden D of tests/mc_volumes.py: 376 760 faces) by the product's marching cubes: no boundary,
                  so the plan is r3g_meshtopo_build plus its own bookkeeping -- the overhead over the build alone
  sphere_holes    the same with a seeded 1 % of its faces removed
  ms_build        r3g_meshtopo_build alone on the same mesh, timed ALTERNATELY with the plan in the same process
  ms_plan/ms_emit median and min over --reps after a warm-up, HIP events on the stream (a plan with its read-backs; an emit)
  ms_numpy        the numpy / Python restatement (tests/meshfill_ref.py) of the same plan on the host, once, for scale
  blob            the 257^3 blob (the field of tools/bench_mc.py) after cluster_faces(--budget): the topology report before and
                  after fill_holes at max_loop 4 and 64.  Its non-manifold edges remain; nothing about the outcome is asserted.
No time is asserted anywhere.

    python tools/bench_meshfill.py [--reps 7] [--n 257] [--budget 40000] [--no-numpy] [--no-blob] [--write [PATH]]

--write replaces only what stands between the two marker lines of the file; text written by hand outside them is kept.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-re-gen_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench_meshtopo import COUNTS, blob, med, sphere, timed  # noqa: E402

FILL = ("boundary", "loops", "tangled", "filled", "oversize", "longest", "faces_added", "rounds")


def measure(v, f, reps, numpy_too, max_loop=64):
    from r3g import ffi, meshfill, meshtopo
    L, ctx = ffi.lib(), ffi.context(0)
    _, _, rep = meshfill._plan(v, f, None, max_loop, "fan")                  # warm-up: workspaces, code objects
    new_f = torch.empty((max(1, rep["faces_added"]), 3), dtype=torch.int32, device=f.device)

    def emit():
        ffi.check(L.r3g_meshfill_emit(ctx, ctypes.c_void_p(new_f.data_ptr()), ctypes.c_void_p(0), ffi.stream_ptr()))
    emit()
    meshtopo.build(v, f)
    torch.cuda.synchronize()
    ms_build, ms_plan, ms_emit = [], [], []
    for _ in range(max(1, reps)):
        ms_build.append(timed(lambda: meshtopo.build(v, f))[0])
        ms_plan.append(timed(lambda: meshfill._plan(v, f, None, max_loop, "fan"))[0])
        ms_emit.append(timed(emit)[0])
    out = {"verts": int(v.shape[0]), "faces": int(f.shape[0]), "max_loop": max_loop, "ms_build": med(ms_build), "ms_plan": med(ms_plan),
           "ms_emit": med(ms_emit), "report": {k: rep[k] for k in FILL}}
    if numpy_too:
        import meshfill_ref
        hv, hf = v.cpu().numpy(), f.cpu().numpy()
        t0 = time.perf_counter()
        r = meshfill_ref.plan(hv, hf, max_loop=max_loop)
        out["ms_numpy"] = 1e3 * (time.perf_counter() - t0)
        out["numpy_agrees"] = all(r["report"][k] == rep[k] for k in FILL) and bool(
            (torch.from_numpy(r["new_faces"]) == new_f[:rep["faces_added"]].cpu()).all())
    return out


def blob_reports(n, budget):
    """the clustered blob's topology before and after fill_holes at max_loop 4 and 64"""
    from r3g import mc, meshfill, meshops, meshtopo
    v, f = mc.marching_cubes(blob(n).cuda(), 0.0)
    fv, ff = meshops.remove_floaters(v, f, 0.02)
    cv, cf = (t.contiguous() for t in meshops.cluster_faces(fv, ff, budget))
    keys = COUNTS + ("watertight", "winding_consistent")
    rep = meshtopo.build(cv, cf)
    out = [{"step": "cluster_faces(%d)" % budget, **{k: rep[k] for k in keys}}]
    for max_loop in (4, 64):
        _, _, info = meshfill.fill_holes(cv, cf, max_loop=max_loop)
        out.append({"step": "fill_holes(max_loop=%d)" % max_loop, **{k: info["topology"][k] for k in keys}, "fill": {k: info[k] for k in FILL}})
    return out


BEGIN, END = "<!-- bench_meshfill.py --write: begin (generated; edit outside the markers) -->", "<!-- bench_meshfill.py --write: end -->"


def write_profile(path, out):
    rows = [BEGIN, "",
            "Tool: `python tools/bench_meshfill.py --write` (HIP events on the stream; medians over %d repetitions after a warm-up; the" % out["reps"],
            "sphere by the product's marching cubes at %d³).  `build` is `r3g_meshtopo_build` alone, timed alternately with the plan in" % out["n"],
            "the same process: the plan contains one such build.  `numpy` is the restatement of tests/meshfill_ref.py on the host, once.",
            "", "## Recorded run", "",
            "| mesh | faces | boundary | loops | filled | faces added | rounds | build ms (median / min) | plan ms (median / min) | emit ms (median / min) | numpy ms |",
            "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name in ("sphere", "sphere_holes"):
        r = out[name]
        p = r["report"]
        rows.append("| %s | %d | %d | %d | %d | %d | %d | %.3f / %.3f | %.3f / %.3f | %.3f / %.3f | %s |" % (
            name, r["faces"], p["boundary"], p["loops"], p["filled"], p["faces_added"], p["rounds"], r["ms_build"]["median"],
            r["ms_build"]["min"], r["ms_plan"]["median"], r["ms_plan"]["min"], r["ms_emit"]["median"], r["ms_emit"]["min"],
            "%.0f" % r["ms_numpy"] if "ms_numpy" in r else "-"))
    if out.get("blob"):
        rows += ["", "## The clustered blob before and after the fill", "",
                 "| step | faces | V_ref | E | χ | boundary | clash | non-manifold | bodies | watertight | loops | filled | tangled | faces added |",
                 "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for s in out["blob"]:
            fl = s.get("fill")
            rows.append("| %s | %d | %d | %d | %d | %d | %d | %d | %d | %s | %s |" % (
                s["step"], s["usable"], s["vref"], s["edges"], s["euler"], s["boundary"], s["clash"], s["nonmanifold"], s["bodies"],
                s["watertight"], " | ".join(str(fl[k]) for k in ("loops", "filled", "tangled", "faces_added")) if fl else "- | - | - | -"))
    rows += ["", END]
    block = "\n".join(rows)
    try:
        with open(path) as fh:
            old = fh.read()
    except OSError:
        old = "# Mesh fill (DESIGN.md §4j): timings and the clustered blob\n\n" + BEGIN + "\n" + END + "\n"
    if BEGIN not in old or END not in old:
        raise SystemExit("%s has no bench_meshfill.py markers: refusing to overwrite it" % path)
    with open(path, "w") as fh:
        fh.write(old[:old.index(BEGIN)] + block + old[old.index(END) + len(END):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=257, help="side of the volumes")
    ap.add_argument("--budget", type=int, default=40000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--no-blob", action="store_true", help="skip the clustered blob's reports")
    ap.add_argument("--write", nargs="?", const=os.path.join(ROOT, "profiles", "meshfill.md"), default=None,
                    help="write the tables (default path: profiles/meshfill.md)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meshfill.py needs an MI355X (the product has no CPU path)")
    from r3g import ffi, mc
    out = {"bench": "meshfill", "n": a.n, "reps": a.reps, "seed": a.seed}
    with ffi.device_lock(0):
        v, f = (t.contiguous() for t in mc.marching_cubes(sphere(a.n).cuda(), 0.5))
        out["sphere"] = measure(v, f, a.reps, not a.no_numpy)
        keep = torch.rand(f.shape[0], generator=torch.Generator().manual_seed(a.seed)) >= 0.01
        out["sphere_holes"] = measure(v, f[keep.to(f.device)].contiguous(), a.reps, not a.no_numpy)
        if not a.no_blob:
            out["blob"] = blob_reports(a.n, a.budget)
    print(json.dumps(out), flush=True)
    if a.write:
        write_profile(a.write, out)


if __name__ == "__main__":
    main()
