"""The host bookkeeping of the deferred translation row (csrc/bge_epochs.hpp Row3State), without a GPU.

* A stand-alone C++ program (tests/cpp/row3_state.cpp) drives bge::Row3State next to bge::PathEpochs: which tick may defer (one
  pass, no frozen root, not pinned, not switched off), when a store is due and with which epoch, and that pinning ends deferral.
* bge_world.cpp keeps that state in the struct and nowhere else, and stores the deferred rows BEFORE anything that would break the
  rule "row 3 is (pos, 1) while the wave's rows word equals the pending epoch": before either epoch bump, before the words are
  zeroed, before the calls that write pos or move matrices, and before every launch that writes pos outside a translation-row tick."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "banggameengine_amd", "csrc")


def test_row3_state_program(tmp_path):
    exe = str(tmp_path / "row3_state")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "row3_state.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "row3_state ok" in r.stdout


def _functions(src):
    """(name, body) of every function definition that starts in column 0 (the C-ABI entry points and the file-level helpers)."""
    heads = [m for m in re.finditer(r"^(?:static )?(?:int|void|uint64_t|const char\*) (\w+)\([^;{]*\)\s*(?:try\s*)?\{", src, re.M)]
    out = {}
    for k, m in enumerate(heads):
        end = heads[k + 1].start() if k + 1 < len(heads) else len(src)
        out[m.group(1)] = src[m.end():end]
    return out


def _before(body, first, then):
    a, b = body.find(first), body.find(then)
    return a >= 0 and b >= 0 and a < b


def test_the_store_comes_before_everything_that_would_break_the_rule():
    src = open(os.path.join(CSRC, "bge_world.cpp")).read()
    assert "bge::Row3State row3;" in src
    # one place sets it, one place takes it
    assert src.count("row3.deferred(") == 1 and src.count("row3.take_sync()") == 1
    assert len(re.findall(r"\brow3\.pending\s*(=[^=]|\+\+)", src)) == 0
    # the struct's own helpers: the store precedes the zeroing and the bump
    m = re.search(r"void words_clear\(\)\s*\{(.*?)\n    \}", src, re.S)
    assert m and _before(m.group(1), "ensure_row3_current()", "hipMemsetAsync(rs_word.p")
    m = re.search(r"void epochs_edit\(\)\s*\{(.*?)\n    \}", src, re.S)
    assert m and _before(m.group(1), "ensure_row3_current()", "epochs.host_edit()")
    fn = _functions(src)
    # a tick without the translation-row path: before its epoch bump (and so before all of its kernels)
    tick = fn["tick_impl"]
    assert _before(tick, "if (!plan.rows_path) HIP_TRY(w->ensure_row3_current());", "epochs.tick_without_rows()")
    assert _before(tick, "epochs.tick_without_rows()", "contact_substep(") and _before(tick, "epochs.tick_without_rows()", "launch_tick(")
    # (which tick defers — a translation-row tick that may — is run, not read: tests/cpp/tick_plan.cpp)
    assert _before(tick, "bge::TickPlan::of(flags, scene, bge::TickKnobs::from_env(), w->row3)", "if (plan.defer_row3) {") and _before(tick, "if (plan.defer_row3) {", "row3.deferred(w->epochs.rows)")
    # calls that write pos, or move stored matrices, before their epochs_edit()
    assert _before(fn["upload_trs"], "ensure_row3_current()", "upload_rows(")
    assert _before(fn["bge_world_set_topology"], "ensure_row3_current()", "launch_gather_rows(")
    assert _before(fn["bge_world_step_simulation"], "ensure_row3_current()", "launch_pose_only(")
    # the raw pointers pin
    arr = fn["bge_world_device_array"]
    assert _before(arr, "case BGE_ARRAY_WORLD:", "row3.pinned = true") and _before(arr, "case BGE_ARRAY_POSITION:", "row3.pinned = true")
    assert _before(arr, "row3.pinned = true", "ensure_row3_current()")
    assert src.count("row3.pinned = ") == 1
    # every reader of the world array outside the tick gets the view to compose with
    for call in re.findall(r"launch_pack_roots\([^;]*;", src):
        assert "w->row3_view()" in call
    assert "p.row3 = w->row3_view();" in fn["cull_params"]
    assert "launch_gather_world(" in fn["download_rows"] and "w->row3.pending != 0u" in fn["download_rows"]


def test_only_the_kernels_of_the_audit_write_positions():
    """DESIGN.md §4.1 lists who stores to WorldView::pos; a new writer has to be looked at (does it run with rows deferred?)."""
    writers = set()
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".hpp")):
            continue
        text = open(os.path.join(CSRC, name)).read()
        if re.search(r"st3\(\s*\w+\.pos\s*,|\.pos\[[^\]]*\]\s*=[^=]", text):
            writers.add(name)
    assert writers == {"bge_kernels.hip", "bge_contact_device.hpp", "bge_island.hip"}, sorted(writers)
