"""The host bookkeeping of fused ticks (csrc/bge_epochs.hpp FuseClock, DESIGN.md §4.1 "Fused ticks"), without a GPU.

* A stand-alone C++ program (tests/cpp/fuse_clock.cpp) replays tick_impl's group loop on bge::FuseClock: the split of K ticks into
  groups of at most T for K in 1..9, 17, 1000 and T in 1, 2, 3, 4, 8, serials that only rise across groups and calls, and the wrap
  that asks for the zeroing of the words.
* bge_world.cpp keeps that state in the struct and nowhere else; what a launch carries comes from csrc/bge_tick_plan.hpp TickGroups,
  which tests/test_tick_plan_cpu.py runs."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "banggameengine_amd", "csrc")


def test_fuse_clock_program(tmp_path):
    exe = str(tmp_path / "fuse_clock")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "fuse_clock.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fuse_clock ok" in r.stdout


def _tick_impl(src):
    m = re.search(r"^int tick_impl\([^;{]*\)\s*\{(.*?)^\}", src, re.S | re.M)
    assert m
    return m.group(1)


def test_a_launch_carries_a_serial_only_where_the_tick_is_fusable():
    src = open(os.path.join(CSRC, "bge_world.cpp")).read()
    plan = open(os.path.join(CSRC, "bge_tick_plan.hpp")).read()
    assert "bge::FuseClock fuse;" in src
    tick = _tick_impl(src)
    # one place hands serials out (TickGroups::next), only tick_impl gives it the clock, and only tick_impl writes the two parameters
    assert plan.count(".begin_group(") == 1 and "begin_group(" not in src
    assert len(re.findall(r"\bfuse\b", src)) == 2 and tick.count("groups.next(t, w->fuse)") == 1
    assert len(re.findall(r"\b(fuse|clock)\.next\b", src + plan)) == 0
    assert len(re.findall(r"\.serial\s*=[^=]", src + plan)) == 1 and len(re.findall(r"\.n_left\s*=[^=]", src + plan)) == 1
    assert "p.serial = group.serial;" in tick and "p.n_left = group.n_left;" in tick
    # which launches carry a serial (fusable, not solo, a group of more than one) is run, not read: tests/cpp/tick_plan.cpp.
    # TickParams starts zeroed
    assert "bge::TickParams p{};" in tick
    # the zeroing the clock asks for is ordered on the world's stream, after the group began and before the launches
    memset = "if (group.clear_adv) HIP_TRY(hipMemsetAsync(w->adv.p, 0, w->adv.bytes, w->stream));"
    assert -1 < tick.find("groups.next(t, w->fuse)") < tick.find(memset) < tick.find("launch_tick(")
    # the words are zeroed with every layout
    assert "hipMemsetAsync(w->adv.p, 0, T * 16, w->stream)" in src


def test_only_the_flat_physics_tick_knows_the_words():
    """WorldView::adv is read and written by k_tick under kFuse (PHYS and the translation-row variants) and by nothing else."""
    users = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp")):
            text = open(os.path.join(CSRC, name)).read()
            hits = re.findall(r"\b\w+\.adv\[", text)
            if hits:
                users[name] = len(hits)
    assert users == {"bge_kernels.hip": 2}, users
    text = open(os.path.join(CSRC, "bge_kernels.hip")).read()
    assert "constexpr bool kFuse = PHYS && kRowsPath;" in text
    for m in re.finditer(r"\bw\.adv\[", text):
        before = text[:m.start()]
        guard = before.rfind("if (kFuse && p.serial != 0u")
        assert guard >= 0 and before.count("\n", guard) <= 22, "a use of adv without the guard in front of it"
