#!/usr/bin/env python3
"""The point-cloud scores of the reference's evaluation for two PLY files, on the GPU (r3g.cloud.evaluate):
one JSON line with CD, FSCORE, IOU_BBOX, HAUSDORFF, PRECISION, RECALL (the latter two under upstream's naming, see
r3g.cloud.precision_recall) and the two point counts.

    python tools/eval_clouds.py PRED.ply GT.ply
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-re-gen_amd"))


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("eval_clouds.py needs an MI355X (the product has no CPU path)")
    from r3g import cloud
    pred, gt = (torch.from_numpy(cloud.load_ply(p).vertices).to("cuda", dtype=torch.float32) for p in sys.argv[1:])
    out = cloud.evaluate(pred, gt)
    out.update({"pred_points": int(pred.shape[0]), "gt_points": int(gt.shape[0])})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
