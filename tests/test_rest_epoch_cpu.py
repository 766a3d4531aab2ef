"""The two epochs behind the tick kernel's per-wave words (csrc/bge_epochs.hpp), without a GPU.

* A stand-alone C++ program (tests/cpp/path_epochs.cpp) drives bge::PathEpochs: a host edit moves BOTH epochs, a tick without one
  path moves that path's epoch alone, neither is ever 0, and a wrap is reported so that the words get zeroed.
* bge_world.cpp keeps its epochs in that struct and nowhere else, and every C-ABI entry point that invalidates the translation-row
  words does so through bge_world::epochs_edit(), which moves the rest epoch with it: the only rows-only bump is the one tick_impl
  makes for a tick that runs without the translation-row path."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "banggameengine_amd", "csrc")


def test_path_epochs_program(tmp_path):
    exe = str(tmp_path / "path_epochs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "path_epochs.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "path_epochs ok" in r.stdout


def _functions(src):
    """(name, body) of every function definition that starts in column 0 (the C-ABI entry points and the file-level helpers)."""
    heads = [m for m in re.finditer(r"^(?:static )?(?:int|void|uint64_t|const char\*) (\w+)\([^;{]*\)\s*(?:try\s*)?\{", src, re.M)]
    out = []
    for k, m in enumerate(heads):
        end = heads[k + 1].start() if k + 1 < len(heads) else len(src)
        out.append((m.group(1), src[m.end():end]))
    return out


def test_every_entry_point_that_bumps_the_rows_epoch_bumps_the_rest_epoch():
    src = open(os.path.join(CSRC, "bge_world.cpp")).read()
    # the epochs live in the struct: no second counter, no hand-made increment
    assert "bge::PathEpochs epochs;" in src
    assert not re.search(r"\brs_epoch\s*(=[^=]|\+\+)|\+\+\s*\w*rs_epoch|\brest_epoch\s*(=[^=]|\+\+)", src.replace("p.rs_epoch = w->epochs.rows", "").replace("p.rest_epoch = w->epochs.rest", ""))
    assert src.count("epochs.tick_without_rows()") == 1 and src.count("epochs.tick_without_rest()") == 1
    assert src.count("epochs.host_edit()") == 1  # inside bge_world::epochs_edit
    editors = set()
    for name, body in _functions(src):
        rows_only = "tick_without_rows()" in body
        if rows_only:
            assert name == "tick_impl", f"{name} moves the rows epoch without the rest epoch"
        if "epochs_edit()" in body:
            editors.add(name)
    # everything that can change what a sleeping body's wave vouched for
    want = {"bge_world_set_topology", "upload_trs", "bge_world_mark_dirty", "upload_bodies", "bge_world_set_velocities",
            "bge_world_step_simulation", "bge_world_set_ground_plane", "bge_world_set_static_contacts", "bge_world_set_dynamic_contacts",
            "bge_world_set_sleeping"}
    assert want <= editors, sorted(want - editors)
