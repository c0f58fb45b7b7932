"""csrc/scan_device.h: the one exclusive prefix sum behind the mesh cleaners' compactions, the CSR row starts of the grid build,
meshfill's tile offsets and the hierarchical decoder's popcount prefix.  Its users are pinned bit for bit by their own tests; this one
drives the templates directly.  tools/ubench/scan_check.hip compares the device-wide scan with a host loop modulo 2^32, out of place
and in place, with and without the total, at the thread, tile and sums-loop boundaries and past the 20 971 520 elements the grid
build's scan used to end at, for plain counts and for the popcount Load, and block_exclusive_scan<4> and <16> in one block."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shared_scan_matches_the_host_prefix_sum(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is not on this box")
    exe = str(tmp_path / "scan_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", exe,
                           os.path.join(ROOT, "tools", "ubench", "scan_check.hip")], stderr=subprocess.DEVNULL)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "scan: 0 of" in out.stdout and "mismatches" in out.stdout, out.stdout
