#!/usr/bin/env python3
"""Record the goldens of tests/test_dbscan_cpu.py and tests/test_dbscan_gpu.py from the reference's own point-cloud filters and
from scikit-learn (host only, run once by hand):

    python tools/make_dbscan_goldens.py REFERENCE_ROOT

REFERENCE_ROOT is a checkout of the reference project; its src/scene_reconstruction/source/utils_SR/pc_utils.py is loaded by
path and RUN, nothing of its text is copied.  That file imports trimesh and utils.global_utils, which filter_dbscan and
filter_points_by_quantile do not use: stub modules are put in sys.modules for both.

Writes tests/golden/dbscan_clouds.npz (the random clouds of tests/dbscan_ref.py RANDOM, as found) and
tests/golden/dbscan_expect.json: per cloud eps, min_samples, scikit-learn's labels_ and core_sample_indices_ (every cloud of
tests/dbscan_ref.py without a non-finite row; scikit-learn refuses those), and for the random clouds the row indices that the
reference's filter_dbscan (at the cloud's eps and min_samples) and filter_points_by_quantile (q = 0.02) keep (the latter
only where RANDOM asks for it).

A random cloud is regenerated with another seed until, in float64, no quantile bound lies within 1e-5 of a coordinate of that
axis, relative to the axis extent: then the kept set cannot depend on how float32 interpolates the bound.  Asserted below.
The filters return points, not rows, so the kept points are matched back to rows by exact coordinates; the random clouds
have no duplicate rows (asserted).
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dbscan_ref  # noqa: E402

Q = 0.02
MARGIN = 1e-5


def load_pc_utils(reference_root):
    tm, ut, gu = types.ModuleType("trimesh"), types.ModuleType("utils"), types.ModuleType("utils.global_utils")
    gu.B2P = None
    ut.global_utils = gu
    sys.modules["trimesh"], sys.modules["utils"], sys.modules["utils.global_utils"] = tm, ut, gu
    path = os.path.join(reference_root, "src", "scene_reconstruction", "source", "utils_SR", "pc_utils.py")
    spec = importlib.util.spec_from_file_location("reference_pc_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def quantile_clear(p):
    """no float64 quantile bound within MARGIN (relative to the extent) of a coordinate"""
    x = p.astype(np.float64)
    for a in range(3):
        ext = x[:, a].max() - x[:, a].min()
        for q in (Q, 1 - Q):
            if np.abs(x[:, a] - np.quantile(x[:, a], q)).min() <= MARGIN * ext:
                return False
    return True


def rows_of(kept, p):
    """the rows of p that `kept` (a subset of them, in order) holds"""
    index = {tuple(r): i for i, r in enumerate(p.tolist())}
    assert len(index) == len(p), "duplicate rows"
    rows = [index[tuple(r)] for r in kept.tolist()]
    assert rows == sorted(rows)
    return rows


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    from sklearn.cluster import DBSCAN
    ref = load_pc_utils(sys.argv[1])
    found, expect = {}, {}
    for name, (make, eps, min_samples, quantile) in dbscan_ref.RANDOM.items():
        seed = None
        for seed in range(100, 200):
            p = make(seed)
            if not quantile or quantile_clear(p):
                break
        assert not quantile or quantile_clear(p), name
        found[name] = p
        t = torch.from_numpy(p)
        kept_db = ref.filter_dbscan(t, eps=eps, min_samples=min_samples).numpy()
        kept_q = rows_of(ref.filter_points_by_quantile(t, q=Q).numpy(), p) if quantile else None
        expect[name] = {"seed": seed, "q": Q, "dbscan_keep": rows_of(kept_db, p), "quantile_keep": kept_q}
    clouds = {k: (found[k], v[1], v[2]) for k, v in dbscan_ref.RANDOM.items()}
    clouds.update(dbscan_ref.fixed_clouds())
    for name, (p, eps, min_samples) in clouds.items():
        e = expect.setdefault(name, {})
        e["eps"], e["min_samples"], e["n"] = eps, min_samples, len(p)
        if len(p) and np.isfinite(p).all():
            db = DBSCAN(eps=eps, min_samples=min_samples).fit(p)
            e["labels"], e["core"] = db.labels_.tolist(), db.core_sample_indices_.tolist()
    import sklearn
    os.makedirs(GOLDEN, exist_ok=True)
    np.savez_compressed(os.path.join(GOLDEN, "dbscan_clouds.npz"), **found)
    with open(os.path.join(GOLDEN, "dbscan_expect.json"), "w") as f:
        json.dump({"sklearn": sklearn.__version__, "clouds": expect}, f, separators=(",", ":"))
    print("wrote", len(found), "clouds and", len(expect), "expectations")


if __name__ == "__main__":
    main()
