"""The host bookkeeping of fused ticks (csrc/bge_epochs.hpp FuseClock, DESIGN.md §4.1 "Fused ticks"), without a GPU.

* A stand-alone C++ program (tests/cpp/fuse_clock.cpp) replays tick_impl's group loop on bge::FuseClock: the split of K ticks into
  groups of at most T for K in 1..9, 17, 1000 and T in 1, 2, 3, 4, 8, serials that only rise across groups and calls, and the wrap
  that asks for the zeroing of the words.
* bge_world.cpp keeps that state in the struct and nowhere else, and a launch carries a serial only where the tick is fusable."""
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
    assert "bge::FuseClock fuse;" in src
    tick = _tick_impl(src)
    # one place hands serials out, and only tick_impl touches the clock or writes the two parameters
    assert src.count("fuse.begin_group(") == 1 and tick.count("fuse.begin_group(") == 1
    assert len(re.findall(r"\bfuse\.next\b", src)) == 0
    assert len(re.findall(r"\.serial\s*=[^=]", src)) == 1 and len(re.findall(r"\.n_left\s*=[^=]", src)) == 1
    # the fusable condition: the physics + transform tick on the translation-row path with the flag word, one pass, no frozen root,
    # no event pair per tick
    m = re.search(r"const bool fusable = ([^;]*);", tick)
    assert m
    cond = m.group(1)
    for term in ("phys", "rows_path", "flag_word", "w->flat.pass_tile_begin.size() - 1 == 1", "!w->any_frozen", "w->profiling != 2"):
        assert term in [t.strip() for t in cond.split("&&")], (term, cond)
    # serial is `fused ? ... : 0u`, and `fused` implies `fusable`; TickParams starts zeroed
    m = re.search(r"const bool fused = ([^;]*);", tick)
    assert m and m.group(1).split("&&")[0].strip() == "fusable"
    assert re.search(r"p\.serial = fused \? [^:;]* : 0u;", tick) and re.search(r"p\.n_left = fused \? [^:;]* : 1u;", tick)
    assert "bge::TickParams p{};" in tick
    # the clock moves only for a fusable tick, and the zeroing it asks for is ordered on the world's stream before the launches
    m = re.search(r"if \(([^{]*)\) \{\s*group_t0 = t;(.*?)\n        \}", tick, re.S)
    assert m and m.group(1).split("&&")[0].strip() == "fusable"
    body = m.group(2)
    assert "if (wrapped) HIP_TRY(hipMemsetAsync(w->adv.p, 0, w->adv.bytes, w->stream));" in body
    assert tick.find("fuse.begin_group(") < tick.find("launch_tick(")
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
