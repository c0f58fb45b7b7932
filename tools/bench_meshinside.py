#!/usr/bin/env python3
"""Times the point-in-mesh query (include/r3g.h r3g_meshinside_build / r3g_meshinside_query) on the
257^3 blob mesh (a union of four spheres by the product's marching cubes, the size of a typical object mesh) with the cell
centres of an n^3 lattice over its bounding box as query points, n = 128 and 256, against resolution 1 (every point tests
every usable face) on the same device.  One JSON line, and with --write a table in profiles/meshinside.md:
  ms_build / ms_query   median and min over --reps, HIP events on the stream (build: one call with its read-backs; query: all
                        lattice points, in chunks of 2^22)
  tests_per_point       point-face tests per query point (counter "meshinside_tests")
  resolution, pairs     the columns the automatic rule settled on
  brute                 the same for resolution 1 on --brute-points lattice points from the middle slab (all of them would take minutes)
No time is asserted anywhere.

    python tools/bench_meshinside.py [--reps 5] [--axis 2] [--brute-points 16384] [--write [PATH]]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-re-gen_amd"))
import torch  # noqa: E402

CHUNK = 1 << 22


def blob(n):
    """smooth closed surface (union of a few spheres), V ~ 2e5 at n = 257 (the field of tools/bench_mc.py)"""
    ax = torch.linspace(-1, 1, n)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    f = torch.full((n, n, n), -1.0)
    for cx, cy, cz, r in ((0, 0, 0, .55), (.35, .2, .1, .35), (-.3, -.25, .2, .3), (.1, -.4, -.3, .28)):
        f = torch.maximum(f, r - torch.sqrt((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2))
    return f.contiguous()


def timed(fn):
    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b.record()
    out = fn()
    e.record()
    e.synchronize()
    return b.elapsed_time(e), out


def lattice(v, n):
    from r3g import meshinside
    lo, hi = v.min(0).values.double().tolist(), v.max(0).values.double().tolist()
    ax = [meshinside.lattice_axis(lo[k], hi[k], n, v.device) for k in range(3)]
    return torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def measure(v, f, pts, axis, resolution, reps):
    from r3g import ffi, meshinside

    def query_all():
        inside = 0
        for s in range(0, pts.shape[0], CHUNK):
            inside += int((meshinside.query(pts[s:s + CHUNK]) & 1).sum())
        return inside
    meshinside.build(v, f, axis, resolution)                     # warm-up: workspaces, code objects
    meshinside.query(pts[:1024])
    torch.cuda.synchronize()
    ms_b, ms_q, tests, inside = [], [], 0, 0
    for _ in range(max(1, reps)):
        t, info = timed(lambda: meshinside.build(v, f, axis, resolution))
        ms_b.append(t)
        n0 = ffi.counter("meshinside_tests")
        t, inside = timed(query_all)
        ms_q.append(t)
        tests = ffi.counter("meshinside_tests") - n0
    n = int(pts.shape[0])
    return {"points": n, "inside": inside, "resolution": info["resolution"], "pairs": info["pairs"],
            "ms_build": {"median": statistics.median(ms_b), "min": min(ms_b)},
            "ms_query": {"median": statistics.median(ms_q), "min": min(ms_q)},
            "tests_per_point": tests / n, "ns_per_point": 1e6 * statistics.median(ms_q) / n}


def write_profile(path, out):
    rows = ["# Point-in-mesh query (DESIGN.md §4g): timings", "",
            "Tool: `python tools/bench_meshinside.py --write` (HIP events on the stream; medians over %d repetitions; the 257³ blob"
            % out["reps"], "mesh, %d vertices, %d faces, rays along axis %d; query points = the cell centres of an n³ lattice over the"
            % (out["verts"], out["faces"], out["axis"]), "mesh's bounding box; `R = 1` = every point against every usable face, on %d points from the middle of the lattice)."
            % out["brute_points"], "", "## Recorded run", "",
            "| lattice | columns R | pairs | build ms | query ms | ns / point | tests / point | R = 1: ns / point | R = 1: tests / point |",
            "|---|---|---|---|---|---|---|---|---|"]
    for n, r in sorted(out["lattices"].items()):
        g, b = r["grid"], r["brute"]
        rows.append("| %s³ | %d | %d | %.3f | %.3f | %.2f | %.1f | %.1f | %.0f |" % (
            n, g["resolution"], g["pairs"], g["ms_build"]["median"], g["ms_query"]["median"], g["ns_per_point"], g["tests_per_point"],
            b["ns_per_point"], b["tests_per_point"]))
    rows += ["", "The counts of the two runs agree on the points they share (`brute_agrees` in the JSON line): %s." % out["brute_agrees"], ""]
    with open(path, "w") as fh:
        fh.write("\n".join(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--axis", type=int, default=2)
    ap.add_argument("--n", type=int, default=257, help="side of the blob volume")
    ap.add_argument("--lattices", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--brute-points", type=int, default=16384)
    ap.add_argument("--write", nargs="?", const=os.path.join(ROOT, "profiles", "meshinside.md"), default=None,
                    help="write the table (default path: profiles/meshinside.md)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meshinside.py needs an MI355X (the product has no CPU path)")
    from r3g import ffi, mc, meshinside
    v, f = mc.marching_cubes(blob(a.n).cuda(), 0.0)
    out = {"bench": "meshinside", "volume": "blob %d^3" % a.n, "verts": int(v.shape[0]), "faces": int(f.shape[0]), "axis": a.axis,
           "reps": a.reps, "brute_points": a.brute_points, "lattices": {}, "brute_agrees": True}
    with ffi.device_lock(0):
        for n in a.lattices:
            pts = lattice(v, n)
            sub = pts[pts.shape[0] // 2:][:a.brute_points]          # from the middle slab: rays that do meet the mesh
            grid = measure(v, f, pts, a.axis, 0, a.reps)
            brute = measure(v, f, sub, a.axis, 1, 1)
            want = meshinside.query(sub)                             # resolution 1 is still built
            meshinside.build(v, f, a.axis, 0)
            out["brute_agrees"] = out["brute_agrees"] and bool(torch.equal(want, meshinside.query(sub)))
            out["lattices"][str(n)] = {"grid": grid, "brute": brute}
    print(json.dumps(out), flush=True)
    if a.write:
        write_profile(a.write, out)


if __name__ == "__main__":
    main()
