"""What a tick call decides before it launches (csrc/bge_tick_plan.hpp), without a GPU.

A stand-alone C++ program (tests/cpp/tick_plan.cpp), built with ASan + UBSan, compares TickPlan::of and TickGroups with a copy of the
expressions tick_impl held inline before the header existed: all 128 flag values x 576 scenes x 384 environments for the plan, K in
1..9, 17, 1000 and T in 1, 2, 3, 8, 32 with and without solo groups (and across a wrap of the clock) for the groups.  It asserts the
implications directly (fusable, defer_row3, which launches carry a serial or stand for several ticks, every tick in exactly one
launch) and that TickKnobs::from_env reads the environment anew at every call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "banggameengine_amd", "csrc")


def test_tick_plan_program(tmp_path):
    exe = str(tmp_path / "tick_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "tick_plan.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tick_plan ok" in r.stdout


def test_the_header_compiles_alone(tmp_path):
    """Host-only: no HIP, nothing but bge_epochs.hpp and the C header."""
    tu = tmp_path / "alone.cpp"
    tu.write_text('#include "bge_tick_plan.hpp"\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", CSRC, str(tu)])
