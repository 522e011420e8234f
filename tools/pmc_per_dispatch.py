"""rocprofv3 --pmc counters (csv output) of one kernel, averaged per launch geometry (the dispatches are
grouped by Grid_Size, so a tool that runs a kernel at several shapes gets one line block per shape).
usage: python tools/pmc_per_dispatch.py <counter_collection.csv> <kernel substring>"""
import collections
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
sub = sys.argv[2]
agg = collections.defaultdict(float)
disp = collections.defaultdict(set)
for r in rows:
    if sub in r["Kernel_Name"]:
        key = (r["Kernel_Name"][:60], r.get("Grid_Size", "?"), r.get("Workgroup_Size", "?"), r["Counter_Name"])
        agg[key] += float(r["Counter_Value"])
        disp[key].add(r["Dispatch_Id"])
last = None
for key in sorted(agg):
    if key[:3] != last:
        last = key[:3]
        print(f"-- {key[0]} grid {key[1]} wg {key[2]} ({len(disp[key])} dispatches)")
    print(f"   {key[3]:40s} {agg[key] / len(disp[key]):14.5g}")
