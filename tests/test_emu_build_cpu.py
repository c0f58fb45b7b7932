"""tests/emu_build.py, the one builder of the host twins, on a throw-away twin in tmp_path: a program that prints a constant it takes
from a one-line header.  What it pins is the staleness rule (content, never mtimes; a fresh artefact starts no compiler) and the order
of artefact and stamp.  Rebuilt artefacts are observed by running them, never through an in-process dlopen (which would return the
image loaded first).  The real tests/emu/build/ is touched by the last case only, which does what build() does."""
import os
import subprocess
import sys

import pytest

import emu_build

SOURCE = '#include <cstdio>\n#include "toy.h"\nint main() { std::printf("%d\\n", TOY + EXTRA); return 0; }\n'
DEFINES = ("EXTRA=0",)


@pytest.fixture
def toy(tmp_path, monkeypatch):
    """emu_build pointed at tmp_path: emu/toy_emu.cpp includes csrc/toy.h; -> tmp_path"""
    for d in ("emu", "csrc"):
        (tmp_path / d).mkdir()
    (tmp_path / "emu" / "toy_emu.cpp").write_text(SOURCE)
    (tmp_path / "csrc" / "toy.h").write_text("#define TOY 41\n")
    monkeypatch.setattr(emu_build, "EMU", str(tmp_path / "emu"))
    monkeypatch.setattr(emu_build, "CSRC", str(tmp_path / "csrc"))
    monkeypatch.setattr(emu_build, "OUT", str(tmp_path / "emu" / "build"))
    monkeypatch.setattr(emu_build, "TWINS", {"toy": ["toy_emu.cpp"]})
    new_process()
    yield tmp_path
    new_process()


def new_process():
    """the headers are hashed once per process: forget them, as the next process would"""
    emu_build._headers_digest.cache_clear()


def build(defines=DEFINES):
    new_process()
    return emu_build.program("toy", defines=defines)


def value(exe):
    return int(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)


def build_without_compiler(monkeypatch, tmp_path):
    """the same call with no g++ within reach: it succeeds only if it starts none"""
    with monkeypatch.context() as m:
        m.setenv("PATH", str(tmp_path / "no_such_folder"))
        return build()


def stamp_of(exe):
    return exe + ".digest"


def inputs(root):
    return [str(root / "emu" / "toy_emu.cpp"), str(root / "csrc" / "toy.h")]


def test_first_call_compiles_and_the_second_starts_no_compiler(toy, monkeypatch):
    exe = build()
    assert os.path.dirname(exe) == emu_build.OUT and os.path.exists(stamp_of(exe)) and value(exe) == 41
    before = os.stat(exe).st_mtime_ns
    assert build_without_compiler(monkeypatch, toy) == exe and os.stat(exe).st_mtime_ns == before
    with monkeypatch.context() as m:                      # the same trick does stop a build that is due
        m.setenv("PATH", str(toy / "no_such_folder"))
        with pytest.raises(OSError):
            build(("EXTRA=1",))


def test_changed_content_rebuilds_even_with_older_mtimes(toy):
    exe = build()
    assert value(exe) == 41
    (toy / "csrc" / "toy.h").write_text("#define TOY 42\n")
    old = os.stat(exe).st_mtime - 1000
    for p in inputs(toy):
        os.utime(p, (old, old))
    assert all(os.path.getmtime(p) < os.path.getmtime(exe) for p in inputs(toy))     # the mtime rule would keep the 41
    assert value(build()) == 42


def test_touched_inputs_do_not_rebuild(toy, monkeypatch):
    exe = build()
    new = os.stat(exe).st_mtime + 1000
    for p in inputs(toy):
        os.utime(p, (new, new))
    assert build_without_compiler(monkeypatch, toy) == exe and value(exe) == 41


def test_a_new_header_rebuilds_to_the_same_result(toy, monkeypatch):
    exe = build()
    (toy / "emu" / "unused.h").write_text("#define UNUSED 1\n")
    with pytest.raises(OSError):                          # every header is in the key, included or not
        build_without_compiler(monkeypatch, toy)
    assert value(build()) == 41
    assert build_without_compiler(monkeypatch, toy) == exe


def _change_define(exe, toy):
    return ("EXTRA=1",)


def _remove_artefact(exe, toy):
    os.remove(exe)


def _remove_stamp(exe, toy):
    os.remove(stamp_of(exe))


def _foreign_stamp(exe, toy):
    with open(stamp_of(exe), "w") as f:
        f.write("not a digest\n")


@pytest.mark.parametrize("disturb", (_change_define, _remove_artefact, _remove_stamp, _foreign_stamp))
def test_each_of_these_rebuilds(toy, monkeypatch, disturb):
    exe = build()
    defines = disturb(exe, toy) or DEFINES
    with monkeypatch.context() as m:
        m.setenv("PATH", str(toy / "no_such_folder"))
        with pytest.raises(OSError):
            build(defines)
    assert not os.path.exists(stamp_of(exe))              # a build that was due and did not finish leaves no stamp behind
    assert value(build(defines)) == (42 if disturb is _change_define else 41)


def test_changed_flag_rebuilds(toy, monkeypatch):
    build()
    monkeypatch.setattr(emu_build, "COMMON", emu_build.COMMON + ["-DTOY_FLAG"])
    with pytest.raises(OSError):
        build_without_compiler(monkeypatch, toy)


def test_failed_compile_leaves_neither_stamp_nor_artefact(toy, monkeypatch):
    src = toy / "emu" / "toy_emu.cpp"
    src.write_text(SOURCE + "this is no C++\n")
    with pytest.raises(subprocess.CalledProcessError):
        build()
    assert os.listdir(emu_build.OUT) == []
    src.write_text(SOURCE)
    exe = build()
    assert value(exe) == 41 and sorted(os.listdir(emu_build.OUT)) == ["toy_selftest", "toy_selftest.digest"]
    # ... and one that fails over a good artefact takes its stamp away, so that it is never taken for fresh
    src.write_text(SOURCE + "this is no C++\n")
    with pytest.raises(subprocess.CalledProcessError):
        build()
    assert not os.path.exists(stamp_of(exe)) and not [f for f in os.listdir(emu_build.OUT) if "tmp" in f]


def test_shared_library_of_a_row(toy):
    """the library flavour, seen from a fresh child process"""
    (toy / "emu" / "toy_emu.cpp").write_text('#include "toy.h"\nextern "C" int toy() { return TOY; }\n')
    code = "import ctypes, sys; print(ctypes.CDLL(sys.argv[1]).toy())"
    for want in (41, 43):
        (toy / "csrc" / "toy.h").write_text("#define TOY %d\n" % want)
        new_process()
        so = emu_build.shared("toy")
        assert os.path.basename(so) == "libr3g_toy_emu.so"
        assert int(subprocess.run([sys.executable, "-c", code, so], capture_output=True, text=True, check=True).stdout) == want


def test_table_names_exactly_the_twins_present():
    present = {f for f in os.listdir(emu_build.EMU) if f.endswith("_emu.cpp")}
    assert {s for row in emu_build.TWINS.values() for s in row} == present
    assert all(row[0] == name + "_emu.cpp" for name, row in emu_build.TWINS.items())


def test_build_all_returns_one_library_per_row():
    libs = emu_build.build_all()
    assert len(libs) == len(emu_build.TWINS) == len(set(libs)) and all(os.path.isfile(p) for p in libs)
