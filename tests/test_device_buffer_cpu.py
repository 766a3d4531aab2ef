"""The library's owning buffer (csrc/bge_device_buffer.hpp, DESIGN.md "Who owns device memory"), without a GPU.

A stand-alone C++ program (tests/cpp/device_buffer.cpp), built with ASan + UBSan, runs the buffer template over a counting stand-in
allocator that can fail the k-th allocation: grow-only ensure, one free and one allocation per growth, a failed ensure leaves the
buffer empty and can be retried, release + destructor free once, moves / swaps / a growing vector of owners free every block exactly
once, and the live counters behind bge_device_memory end at zero."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "banggameengine_amd", "csrc")


def test_device_buffer_program(tmp_path):
    exe = str(tmp_path / "device_buffer")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "device_buffer.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device_buffer ok" in r.stdout


def test_the_header_compiles_alone(tmp_path):
    """Host-only: no HIP include path, so the template and the counters and nothing else."""
    tu = tmp_path / "alone.cpp"
    tu.write_text('#include "bge_device_buffer.hpp"\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", CSRC, str(tu)])
