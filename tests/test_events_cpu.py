"""csrc/events.h on the host: tests/emu/events_selftest.cpp defines the HIP entry points the header calls on top of malloc / free and
walks PassTimer through a creation that fails at every position, the retry, recording and read-out with injected errors and moves,
Event and Stream through their flavours, and the model's all-or-none creation of its second stream and two events.  It is a
stand-alone program built with -fsanitize=address,undefined (runtimes linked statically), never loaded into Python; the assertions
are in the program, which exits non-zero on the first miss."""
import os
import subprocess

import pytest

import emu_build

_ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_selftest_program_under_sanitizers():
    if not emu_build.sanitizers_link():
        pytest.skip("no sanitizer runtime for g++ on this machine")
    # (a compile error of the program itself is a failure, not a skip: the probe above has shown that the sanitizers link)
    exe = emu_build.program("events", ["events_selftest.cpp"], defines=("__HIP_PLATFORM_AMD__",), extra=("-I" + _ROCM_INCLUDE,),
                            sanitize=True, arith=())
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
