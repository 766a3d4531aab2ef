"""What the ABI tests of the *_cpu modules share: where the C and C++ sources and the library are, the C99 record check built with
gcc, the adapter compiled on the reference's shapes (C++20, -Werror) and the exported-symbol check."""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "banggameengine_amd")


def build_and_run_c99(tmp_path, source, marker):
    """Builds tests/cpp/<source> as strict C99 against the library, runs it and expects the marker it prints at the end."""
    exe = str(tmp_path / source[:-len(".c")])
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(CPP, source),
                           f"-L{LIBDIR}", "-lbge_world", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert marker in r.stdout, r.stdout + r.stderr


def compile_reference_shapes(tmp_path, source):
    """Compiles tests/cpp/<source>: the adapter's members on types with the reference's shapes, C++20 as the reference builds."""
    subprocess.check_call(["g++", "-std=c++20", "-O0", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-c",
                           os.path.join(CPP, source), "-o", str(tmp_path / (source[:-len(".cpp")] + ".o"))])


def assert_exported(names):
    """Every name is declared in the binding's symbol table and resolves in the built library."""
    from banggameengine_amd import _capi
    lib = _capi.lib()
    for name in names:
        assert name in _capi.SYMBOLS, name
        assert getattr(lib, name) is not None, name
