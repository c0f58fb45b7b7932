#!/usr/bin/env python3
"""tools/verify_checkpoint.py <snapshot dir> [--subfolder hunyuan3d-dit-v2-0] [--variant fp16] [--steps 4] [--full] [--keys-only]

One command for the day a real Hunyuan3D-2 snapshot is reachable: key diff of the SAME files against the
oracle's module tree (strict=True) and the product's weight table, per-block deltas and max |residual| per block (decides the fp16
stream by data), N-step latents on the fp16 AND the fp32 stream, VAE output, grid logits, the texture loaders -- every figure at
the tolerance the parity tests use.  The implementation is test infrastructure (it drives oracle/) and lives in
tests/checkpoint_verify.py; this file is its command line.  Exit code 0 = inside every tolerance; JSON report on stdout.
A guidance-distilled snapshot (guidance_embed: true) is not covered: one sentence on stderr and exit code 2."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import checkpoint_verify  # noqa: E402


def distilled_snapshot(argv):
    """the snapshot's config.yaml says guidance_embed: true (upstream's -fast / -turbo subfolders)"""
    import argparse
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("snapshot", nargs="?")
    ap.add_argument("--subfolder", default="hunyuan3d-dit-v2-0")
    a, _ = ap.parse_known_args(argv)
    if not a.snapshot:
        return False
    import yaml
    try:
        with open(os.path.join(os.path.expanduser(a.snapshot), a.subfolder, "config.yaml")) as f:
            doc = yaml.safe_load(f) or {}
        return bool(doc.get("model", {}).get("params", {}).get("guidance_embed", False))
    except (OSError, ValueError, AttributeError, yaml.YAMLError):
        return False          # unreadable: the verifier reports that itself


if __name__ == "__main__":
    if distilled_snapshot(sys.argv[1:]):
        # out of scope, said where a user meets it: the verifier drives the oracle's module tree, which has no guidance_in
        print("verify_checkpoint: this snapshot is guidance-distilled (config.yaml: guidance_embed: true); the checkpoint "
              "verifier covers the CFG models only -- its oracle has no guidance_in --, so nothing was verified.", file=sys.stderr)
        sys.exit(2)
    sys.exit(checkpoint_verify.main())
