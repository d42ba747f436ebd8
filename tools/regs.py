#!/usr/bin/env python3
"""Per-instance register use and spills from `make asm`'s resource remarks:
python tools/regs.py [F ...]  (default: every render_tiles instance);
python tools/regs.py --kernel NAME  prints the kernels whose name contains NAME
(RES=<file> names another remark file, e.g. one written for rt_temporal.hip)."""
import re
import subprocess
import sys

t = open(__import__("os").environ.get("RES", "real-time-ray-tracing-engine_amd/build/asm/resource.txt")).read()
cur, rows = None, {}
for line in t.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = m.group(1)
        rows[cur] = {}
        continue
    m = re.search(r"remark: .*?(VGPRs|SGPRs|VGPRs Spill|SGPRs Spill|Occupancy \[waves/SIMD\]|ScratchSize \[bytes/lane\]): (\d+)", line)
    if m and cur:
        rows[cur][m.group(1)] = int(m.group(2))
if sys.argv[1:2] == ["--kernel"]:
    for k, v in rows.items():
        if sys.argv[2] in k:
            print("%s VGPR %3s SGPR %3s spillV %3s spillS %3s occ %s scratch %s" % (
                k, v.get("VGPRs"), v.get("SGPRs"), v.get("VGPRs Spill"), v.get("SGPRs Spill"),
                v.get("Occupancy [waves/SIMD]"), v.get("ScratchSize [bytes/lane]")))
    sys.exit(0)
want = set(int(a) for a in sys.argv[1:])
for k, v in rows.items():
    # ... and the material set (rt_path.h MatSet: 0 any, 1 diffuse)
    m = re.search(r"render_tilesILb(\d)ELj(\d+)ELi(\d+)ELb(\d)E(?:LN3rtp6MatSetE(\d+)E)?", k)
    if not m or (want and int(m.group(2)) not in want):
        continue
    print("STATS=%s F=%-2s PC=%-2s COST=%s MS=%s VGPR %3s SGPR %3s spillV %3s spillS %3s occ %s scratch %s" % (
        m.group(1), m.group(2), m.group(3), m.group(4), m.group(5) or "0", v.get("VGPRs"), v.get("SGPRs"), v.get("VGPRs Spill"),
        v.get("SGPRs Spill"), v.get("Occupancy [waves/SIMD]"), v.get("ScratchSize [bytes/lane]")))
