"""What the tests of the C++ mirror (include/pfhe.hpp) share: the committed list of the C functions the header calls, the
compile that reads such a list off an object file, and building and running a small program against libpfhe_hip.so."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
SUPPORT = os.path.join(ROOT, "tests", "support")
SYMBOLS = os.path.join(SUPPORT, "cpp_mirror_symbols.txt")
INSTANTIATE = os.path.join(SUPPORT, "cpp_mirror_instantiate.cpp")
# every inline function is kept, so a non-template function counts whether or not anything calls it
COMPILE = ["g++", "-std=c++17", "-fkeep-inline-functions", "-I", INCLUDE, "-c"]


def mirror_symbols():
    """the pfhe_* functions the header called before its two widths were folded into templates, one per line: the undefined
    symbols of a unit that only includes it"""
    return set(open(SYMBOLS).read().split())


def need_gxx():
    if shutil.which("g++") is None or shutil.which("nm") is None:
        pytest.skip("g++ or nm not available")


def undefined_pfhe_symbols(source):
    """compile `source` (never linked, never run) and return the pfhe_* symbols its object file leaves undefined"""
    need_gxx()
    with tempfile.TemporaryDirectory() as d:
        obj = os.path.join(d, "unit.o")
        r = subprocess.run(COMPILE + [source, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        names = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout.split()
    return {n for n in names if n.startswith("pfhe_")}


def build_and_run(program):
    """link `program` (C++ source text) against the built library and run it; the finished process"""
    need_gxx()
    import primus_fhe_amd as p
    if not os.path.exists(p.library_path()):
        pytest.skip("libpfhe_hip.so not built")
    lib_dir = os.path.dirname(p.library_path())
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.cpp"), os.path.join(d, "t")
        with open(src, "w") as f:
            f.write(program)
        r = subprocess.run(["g++", "-std=c++17", "-I", INCLUDE, src, "-o", exe, "-L", lib_dir, "-lpfhe_hip",
                            f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return subprocess.run([exe], capture_output=True, text=True)
