"""The one builder of the host twins (tests/emu/*_emu.cpp: the csrc/*_core.h and *_cell.h text the kernels use, compiled with g++)
and of the stand-alone programs over them; test-only.

An artefact is stale by CONTENT, the rule of 3d-re-gen_amd/build.py: its key is the SHA-256 of its sources, of the name and content of
EVERY header in csrc/ and tests/emu/ (so no include chain is followed by hand) and of its flags.  The key sits in <artefact>.digest,
written after the artefact; a fresh artefact is used without starting a compiler, whatever the mtimes say.  Everything lands in
tests/emu/build/, which travels with the tree to the machine that runs the GPU tests."""
import functools
import hashlib
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
CSRC = os.path.join(os.path.dirname(os.path.dirname(EMU)), "3d-re-gen_amd", "csrc")
OUT = os.path.join(EMU, "build")

# twin -> its sources, relative to tests/emu/ (a new twin is one row)
TWINS = {
    "mc": ["mc_emu.cpp"],
    "dmc": ["dmc_emu.cpp"],
    "qem": ["qem_emu.cpp"],
    "meshdist": ["meshdist_emu.cpp"],
    "meshinside": ["meshinside_emu.cpp"],
    "meshfit": ["meshfit_emu.cpp"],
    "meshtopo": ["meshtopo_emu.cpp"],
    "meshfill": ["meshfill_emu.cpp", "meshtopo_emu.cpp"],
    "cloud": ["cloud_emu.cpp"],
    "orient": ["orient_emu.cpp"],
    "recon": ["recon_emu.cpp"],
    "dbscan": ["dbscan_emu.cpp"],
    "plane": ["plane_emu.cpp"],
    "softras": ["softras_emu.cpp"],
}

COMMON = ["-std=c++17", "-w"]
NO_CONTRACTION = "-ffp-contract=off"      # the twins are bit-exact references: this and the -O level decide their arithmetic
SANITIZE = ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"]


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


@functools.lru_cache(maxsize=None)
def _headers_digest(dirs):
    """name and content of every *.h of dirs; once per process and folder pair"""
    h = hashlib.sha256()
    for d in dirs:
        for f in sorted(os.listdir(d)):
            if f.endswith(".h"):
                h.update(f.encode())
                h.update(_sha(os.path.join(d, f)).encode())
    return h.hexdigest()


def _key(sources, flags):
    text = "".join(_sha(os.path.join(EMU, s)) for s in sources) + _headers_digest((CSRC, EMU))
    return hashlib.sha256((text + " ".join(f for f in flags if not f.startswith("-I"))).encode()).hexdigest()     # no absolute path


def _read(path):
    try:
        with open(path) as f:
            return f.read().strip()
    except OSError:
        return None


def _artefact(filename, sources, flags, quiet=False):
    out = os.path.join(OUT, filename)
    stamp, key = out + ".digest", _key(sources, flags)
    if os.path.exists(out) and _read(stamp) == key:
        return out
    os.makedirs(OUT, exist_ok=True)
    if os.path.exists(stamp):
        os.remove(stamp)              # from here to the last line the artefact counts as stale, wherever the build stops
    tmp = "%s.tmp%d" % (out, os.getpid())
    try:
        subprocess.check_call(["g++"] + flags + ["-I" + CSRC, "-o", tmp] + [os.path.join(EMU, s) for s in sources],
                              stderr=subprocess.DEVNULL if quiet else None)
        os.replace(tmp, out)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    with open(stamp, "w") as f:
        f.write(key + "\n")
    return out


def shared(name):
    """the twin `name` of TWINS as a shared library for ctypes -> path"""
    return _artefact("libr3g_%s_emu.so" % name, TWINS[name], ["-O2", NO_CONTRACTION] + COMMON + ["-fPIC", "-shared"])


def program(name, sources=None, defines=(), extra=(), sanitize=False, arith=("-O1", NO_CONTRACTION)):
    """the stand-alone program <name>_selftest over `sources` (default: the twin's own, whose main() a define switches on) -> path;
    sanitize: -fsanitize=address,undefined with the runtimes linked statically (host programs only, never loaded into Python)"""
    flags = list(arith) + COMMON + ["-g", "-fno-omit-frame-pointer"] + ["-D" + d for d in defines] + list(extra)
    return _artefact(name + "_selftest", TWINS[name] if sources is None else sources, flags + (SANITIZE if sanitize else []))


@functools.lru_cache(maxsize=None)
def sanitizers_link():
    """does an empty program link with SANITIZE?  (The only reason to skip a sanitizer build: with this shown, a compile or link
    error of the program under test is its own.)  The probe is an artefact like the others, so a fresh one starts no compiler."""
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(OUT, "sanitizer_probe.cpp")
    if not os.path.exists(src):
        with open(src, "w") as f:
            f.write("int main() { return 0; }\n")
    try:
        _artefact("sanitizer_probe", [src], SANITIZE, quiet=True)
    except (OSError, subprocess.CalledProcessError):
        return False
    return True


def build_all():
    """every shared library of TWINS -> paths"""
    _headers_digest((CSRC, EMU))          # once, before the threads ask for it
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return list(ex.map(shared, TWINS))


if __name__ == "__main__":
    print("\n".join(build_all()))
