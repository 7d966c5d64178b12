#!/usr/bin/env python3
"""Average PMC value per dispatch by FULL kernel name (template arguments
kept: the pack16 instantiations differ from the whole-key ones only in their
last arguments), from rocprofv3 --pmc counter_collection CSVs.
    python tools/pmc_by_kernel.py DIR [REGEX]
FETCH_SIZE / WRITE_SIZE are in KiB; on gfx950 FETCH_SIZE reports half the bytes
of a streaming read, so the bytes column doubles it."""
import collections
import csv
import glob
import re
import sys

root = sys.argv[1]
pat = re.compile(sys.argv[2]) if len(sys.argv) > 2 else None
acc = collections.defaultdict(list)
for f in glob.glob(root + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        name = r.get("Kernel_Name", "?").replace("lsort::", "").replace("unsigned int", "u32")
        name = name.split("(")[0]
        if pat and not pat.search(name):
            continue
        acc[(name, r["Counter_Name"])].append(float(r["Counter_Value"]))
for (name, c), v in sorted(acc.items()):
    avg = sum(v) / len(v)
    mb = avg * 1024 * (2 if c == "FETCH_SIZE" else 1) / 1e6
    print("%-12s %12.1f KiB = %9.1f MB/launch (n=%4d)  %s" % (c, avg, mb, len(v), name[:140]))
