"""The arithmetic of fused ticks (csrc/bge_fuse_math.hpp, DESIGN.md §4.1 "Lean fusion"), without a GPU.

A stand-alone C++ program (tests/cpp/fuse_math.cpp), built with ASan + UBSan and -ffp-contract=off, includes the header the kernel
includes, with a 64-float array for the wave and an any-lane loop for the ballot, and compares the reduced loop (fuse::fuse_ticks)
with the exact one for the returned flag and, where true, the bits of all six floats: groups of 1, 2, 3, 8, 64, 65 and 1024 ticks,
seeded random waves and constructed ones (a lane entering the band at every tick of a group, crossing it, jumping it; v.y on the
threshold; s = 0 and s < 0; -0.0; a sideways gravity absorbed and not absorbed; NaN and infinities in every input; denormals).
It counts how each wave was decided and fails unless every class holds 1 % of the seeded waves and every constructed wave lands in
the class it was built for."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "banggameengine_amd", "csrc")


def test_fuse_math_program(tmp_path):
    exe = str(tmp_path / "fuse_math")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "fuse_math.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fuse_math ok" in r.stdout
    m = re.search(r"seeded: (\d+) waves; lean (\d+), exact accepted (\d+), exact refused (\d+), not fixed (\d+)", r.stdout)
    assert m, r.stdout
    total, *classes = map(int, m.groups())
    assert all(100 * c >= total for c in classes), r.stdout


def test_the_kernel_runs_the_header():
    text = open(os.path.join(CSRC, "bge_kernels.hip")).read()
    assert '#include "bge_fuse_math.hpp"' in text
    # one function between the kernel and the reduced loop: the first attempt of a solo group goes through it
    assert text.count("fuse::fuse_ticks<WaveLanes>(") == 1 and text.count("fuse::fuse_ticks_exact<WaveLanes>(") == 1
    assert len(re.findall(r"[( ]fuse_ticks\(gf, p, remaining, vn, xn\)", text)) == 1
    # SOLO's retry inside its loop over the ticks keeps the exact loop (an occupancy step otherwise), through the header as well
    assert len(re.findall(r"[( ]fuse_ticks_exact\(gf, p, remaining, vn, xn\)", text)) == 1
    # the ordinary kernel's n_left block keeps round 9's loop written out: that kernel's ISA stays the parent's
    assert text.count("vn.y + (gf.y * gf.w) * p.dt") == 1
