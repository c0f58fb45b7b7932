"""csrc/dev_buf.h on the host: tests/emu/dev_buf_selftest.cpp defines the HIP entry points the header calls on top of malloc / free
and walks DevBuf through growth, injected allocation failures, moves, a map of buffer pairs and the pinned flavour.  It is a
stand-alone program built with -fsanitize=address,undefined (runtimes linked statically), never loaded into Python; the
assertions are in the program, which exits non-zero on the first miss."""
import os
import subprocess

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "3d-re-gen_amd", "csrc")
_ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
_SANITIZE = ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"]


def test_selftest_program_under_sanitizers(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + _SANITIZE + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime for g++ on this machine")
    exe = str(tmp_path / "dev_buf_selftest")
    # (a compile error of the program itself is a failure, not a skip: the probe above has shown that the sanitizers link)
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + _ROCM_INCLUDE, "-I" + _CSRC] + _SANITIZE +
                          ["-fno-omit-frame-pointer", "-g", "-o", exe, os.path.join(_HERE, "emu", "dev_buf_selftest.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
