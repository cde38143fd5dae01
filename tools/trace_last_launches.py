#!/usr/bin/env python3
"""Mean duration of the last N dispatches of a kernel in a rocprofv3 --kernel-trace CSV (and over all of them).
    python tools/trace_last_launches.py DIR [kernel substring] [N]"""
import csv
import glob
import os
import sys

d = sys.argv[1]
name = sys.argv[2] if len(sys.argv) > 2 else "gc_encode_persistent_kernel"
n = int(sys.argv[3]) if len(sys.argv) > 3 else 25
rows = []
for f in glob.glob(os.path.join(d, "**", "*kernel_trace*.csv"), recursive=True):
    with open(f, newline="") as fh:
        rows += [r for r in csv.DictReader(fh) if name in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows]
if not ms:
    raise SystemExit("no dispatch of %s under %s" % (name, d))
last = ms[-n:]
print("%s: last %d mean %.3f ms  (min %.3f max %.3f)   all %d mean %.3f ms" % (name, len(last), sum(last) / len(last), min(last), max(last), len(ms), sum(ms) / len(ms)))
