#!/usr/bin/env python3
"""The emit pass of the C3 cluster search (k_rows_pack + k_cs_emit_rows: packed 64-byte rows) over fresh reservations of the
table: every round releases the library's cached device memory, builds plan, view and table again and prints the emit times of
eight searches - the spread the twelve column arrays of round 3 showed (0.50 .. 0.66 ms) should be gone.

--rebuild: the two regimes of the pass in ONE process.  Every round then runs its searches alternately with
plan.rebuild_dictionary() in front (what bench.py's timed step does: k_cl_fill has written the dictionary's arrays several hundred
MB of traffic before the emit pass) and without (the dictionary resident), and prints v_emit_rows_ms, v_count_ms and v_templates_ms
of either kind; the last line is one JSON object with the medians over all rounds (the first pair of a round is left out).
--only rebuilt|resident: one regime alone (for a counter run, where the two kinds of launch must not mix)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crispr-hawk_amd")]
from crisprhawk_hip import _lib, synth  # noqa: E402
from crisprhawk_hip.pam import PAM  # noqa: E402
from crisprhawk_hip.workload import expand_on_device  # noqa: E402

KEYS = ("v_emit_rows_ms", "v_count_ms", "v_templates_ms")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("rounds", nargs="?", type=int, default=4)
    ap.add_argument("--rebuild", action="store_true", help="alternate searches behind plan.rebuild_dictionary() with resident ones")
    ap.add_argument("--only", choices=("rebuilt", "resident"), help="with --rebuild: one regime alone")
    ap.add_argument("--pairs", type=int, default=8, help="with --rebuild: searches of either kind per round")
    a = ap.parse_args()
    reg = synth.config_c3()
    pam = PAM("NGG", False, True)
    pam.encode(0)
    mm, pt = synth.cfd_tables()
    acc = {"rebuilt": {k: [] for k in KEYS}, "resident": {k: [] for k in KEYS}}
    for rnd in range(a.rounds):
        ds, info, ms, kept = expand_on_device(reg, 3, keep_plan=True)
        v = ds.plan.view()
        search = lambda: v.search(pam.bits, pam.bitsrc, 3, 20, False, mm, pt, download=False).timing  # noqa: E731
        if not a.rebuild:
            t = [search() for _ in range(8)]
            print(rnd, "emit", " ".join(f"{x['v_emit_ms']:.3f}" for x in t), "| rows kernel", " ".join(f"{x['v_emit_rows_ms']:.3f}" for x in t[-3:]), flush=True)
        else:
            search()  # reservations made, template rows sized
            got = {"rebuilt": [], "resident": []}
            for _ in range(a.pairs):
                for kind in ("rebuilt", "resident"):
                    if a.only and kind != a.only:
                        continue
                    if kind == "rebuilt":
                        ds.plan.rebuild_dictionary()
                    got[kind].append(search())
            for kind, t in got.items():
                if not t:
                    continue
                print(rnd, f"{kind:8s}", " | ".join(k[2:-3] + " " + " ".join(f"{x[k]:.3f}" for x in t) for k in KEYS), flush=True)
                for k in KEYS:
                    acc[kind][k] += [x[k] for x in t[1:]]
        ds.plan.close()
        ds.close()
        _lib.lib().hawk_release_cached_memory(_lib.context())
    if a.rebuild:
        out = {kind: {k: {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4), "n": len(x)}
                      for k, x in d.items() if x} for kind, d in acc.items()}
        print(json.dumps({"emit_probe": out, "lib": os.path.basename(_lib.LIB_PATH)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
