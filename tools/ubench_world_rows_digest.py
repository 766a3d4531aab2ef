#!/usr/bin/env python3
"""Digest of tools/ubench_world_rows.sh: per kernel, store policy and size, the event time, the median traced dispatch time
and the bytes per slot from the PMC passes.

    python tools/ubench_world_rows_digest.py OUT_DIR

Bytes per slot: 2 x FETCH_SIZE (gfx950 tallies 128-B read requests at 64 B) and WRITE_SIZE as counted, both KiB -> B,
over the slots of the dispatch (k_full_rows runs four threads per slot)."""
import csv
import glob
import json
import os
import statistics
import sys
from collections import defaultdict


def key(name, grid):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
    base, _, arg = name.partition("<")
    slots = grid // 4 if base == "k_full_rows" else grid
    return base, arg.rstrip(">") == "true", slots  # (kernel (i) has no store policy: nt = False)


def grid_of(row):
    return int(row.get("Grid_Size") or row.get("Grid_Size_X") or 0)


def main():
    out = sys.argv[1]
    times = {}
    names = {"a_full_rows": "k_full_rows", "b_row3": "k_row3", "c_flat_full": "k_flat_full", "d_flat_row3": "k_flat_row3",
             "b2_rows23": "k_rows23", "e_flat_rows23": "k_flat_rows23", "f_flat_row3_vy": "k_flat_row3_vy",
             "g_flat_row3_vblk": "k_flat_row3_vblk", "h_flat_row3_wave": "k_flat_row3_wave",
             "i_flat_norow_wave": "k_flat_norow_wave"}
    seq = defaultdict(list)  # "(j), then T - 1 x (k)": per-launch (= per-tick) event times by (T, slots)
    for line in open(os.path.join(out, "times.jsonl")):
        d = json.loads(line)
        if d["kernel"].startswith("jk_fused_T"):
            seq[(int(d["kernel"][len("jk_fused_T"):]), d["slots"])].append(d["us"])
            continue
        times.setdefault((names[d["kernel"]], bool(d["nt"]), d["slots"]), []).append(d["us"])  # (d), (f) and (h) run more than once
    traced = defaultdict(list)
    for path in glob.glob(os.path.join(out, "stats", "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            traced[key(row["Kernel_Name"], grid_of(row))].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    pmc = defaultdict(lambda: defaultdict(list))
    for c in ("FETCH_SIZE", "WRITE_SIZE"):
        for path in glob.glob(os.path.join(out, f"pmc_{c}", "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if row["Counter_Name"] != c:
                    continue
                pmc[key(row.get("Kernel_Name") or row.get("Kernel"), grid_of(row))][c].append(float(row["Counter_Value"]))
    rows = []
    print(f"{'kernel':12s} {'nt':>2s} {'slots':>9s} {'event_us':>9s} {'trace_us':>9s} {'read_B':>7s} {'write_B':>7s}")
    for k in sorted(times, key=lambda k: (k[2], k[1], k[0])):
        base, nt, slots = k
        ev = statistics.median(times[k])
        tr = statistics.median(traced[k]) if traced[k] else float("nan")
        rd = 2 * statistics.median(pmc[k]["FETCH_SIZE"]) * 1024 / slots if pmc[k]["FETCH_SIZE"] else float("nan")
        wr = statistics.median(pmc[k]["WRITE_SIZE"]) * 1024 / slots if pmc[k]["WRITE_SIZE"] else float("nan")
        rows.append(dict(kernel=base, nt=nt, slots=slots, event_us=ev, event_us_all=times[k], trace_median_us=round(tr, 3),
                         read_B_per_slot=round(rd, 2), write_B_per_slot=round(wr, 2)))
        print(f"{base:12s} {int(nt):2d} {slots:9d} {ev:9.2f} {tr:9.2f} {rd:7.2f} {wr:7.2f}")
    # (j) and (k) are timed as sequences (below); traced and counted per dispatch like every other kernel
    for base in ("k_flat_fused", "k_flat_follow"):
        for slots in sorted({k[1] for k in seq}):
            k = (base, False, slots)
            if not traced[k] and not pmc[k]["FETCH_SIZE"]:
                continue
            tr = statistics.median(traced[k]) if traced[k] else float("nan")
            rd = 2 * statistics.median(pmc[k]["FETCH_SIZE"]) * 1024 / slots if pmc[k]["FETCH_SIZE"] else float("nan")
            wr = statistics.median(pmc[k]["WRITE_SIZE"]) * 1024 / slots if pmc[k]["WRITE_SIZE"] else float("nan")
            rows.append(dict(kernel=base, nt=False, slots=slots, trace_median_us=round(tr, 3), read_B_per_slot=round(rd, 2),
                             write_B_per_slot=round(wr, 2)))
            print(f"{base:12s} {0:2d} {slots:9d} {'':>9s} {tr:9.2f} {rd:7.2f} {wr:7.2f}")
    for (T, slots), us in sorted(seq.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        rows.append(dict(kernel=f"jk_fused_T{T}", nt=False, slots=slots, event_us=statistics.median(us), event_us_all=us))
        print(f"{'jk_fused_T' + str(T):12s} {0:2d} {slots:9d} {statistics.median(us):9.2f}   (per tick: (j), then {T - 1} x (k))")
    json.dump(rows, open(os.path.join(out, "digest.json"), "w"), indent=1)
    # the gate of (h): its slower run against the fastest of the last three (f) runs, the ones around it, at 1 M slots
    f = times.get(("k_flat_row3_vy", False, 1 << 20), [])[-3:]
    h = times.get(("k_flat_row3_wave", False, 1 << 20), [])
    if len(f) == 3 and h:
        gain, spread = min(f) - max(h), max(f) - min(f)
        print(f"gate (h): f {f} h {h}: min f - max h = {gain:.3f} us, 2 x (max f - min f) = {2 * spread:.3f} us: "
              f"{'PASS' if gain >= 2 * spread else 'FAIL'}")
    # the gate of (i): its slowest run against the fastest of the three (h) runs around it, at 1 M slots and 16 M slots
    for n in (1 << 20, 1 << 24):
        h = times.get(("k_flat_row3_wave", False, n), [])[-3:]
        i = times.get(("k_flat_norow_wave", False, n), [])
        if len(h) == 3 and i:
            gain, spread = min(h) - max(i), max(h) - min(h)
            print(f"gate (i) at {n}: h {h} i {i}: min h - max i = {gain:.3f} us, 2 x (max h - min h) = {2 * spread:.3f} us: "
                  f"{'PASS' if gain > 2 * spread else 'FAIL'}")
    # the gate of (j) + (k): the slowest T = 4 sequence, per tick, against the fastest of the four (i) runs around the sequences
    for n in (1 << 20, 1 << 24):
        i = times.get(("k_flat_norow_wave", False, n), [])[-4:]
        for T in (2, 4, 8):
            jk = seq.get((T, n), [])
            if len(i) == 4 and jk:
                gain, spread = min(i) - max(jk), max(i) - min(i)
                print(f"gate (j, k) T = {T} at {n}: i {i} jk {jk}: min i - max jk = {gain:.3f} us, 2 x (max i - min i) = {2 * spread:.3f} us: "
                      f"{'PASS' if gain > 2 * spread else 'FAIL'}{'  <- the gate' if T == 4 and n == 1 << 20 else ''}")


if __name__ == "__main__":
    main()
