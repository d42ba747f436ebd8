"""Step 0: C2's shade passes by lanes served (the RT_PARK_HIST scratch build), and the price of parking."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "real-time-ray-tracing-engine_amd"))
from rtx.lib import load
from rtx.render import Renderer, camera_frame
from rtx.scene import load_scene

L = load()
S = load_scene(os.path.join(ROOT, "real-time-ray-tracing-engine_amd", "scenes", "three_spheres.json"))
f = camera_frame(S.camera_desc(image_width=1920, samples_per_pixel=64, max_depth=8))
with Renderer(S) as R:
    st = R.stats(f, seed=42)
    h = (C.c_uint64 * 32)()
    L.rtk_park_hist.argtypes = [C.c_void_p]
    assert L.rtk_park_hist(h) == 0
h = list(h)
print("STATS", json.dumps(st))
print("# shade passes of C2 (1920x1080, 64 strata, depth 8; STATS instance, schedule of the parent loop)")
print("# lanes served | passes, no refill possible | passes, refill possible | lanes of the latter")
for b in range(8):
    print("%2d-%2d %10d %10d %12d" % (8 * b + 1, 8 * b + 8, h[b], h[8 + b], h[24 + b]))
tot = sum(h[:16])
print("# passes %d (wave_shade_iters %d), lanes %d (shade_events %d)" % (tot, st["wave_shade_iters"], sum(h[16:]), st["shade_events"]))
c_shade = st["cyc_shade"] / max(1, st["wave_shade_iters"])
c_trace = st["cyc_trace"] / max(1, st["wave_trips"])
c_regen = st["cyc_regen"] / max(1, st["wave_trips"])
print("# cycles per pass: shade %.0f, trace %.0f, regen (per trip) %.0f; loop cycles %.4g" % (c_shade, c_trace, c_regen, st["cyc_loop"]))
print("# price of threshold K: passes with <= K lanes and a refill possible wait and merge into a later pass;")
print("#   saved = passes x shade pass; cost = their lanes / 64 x trace pass (the slots parked lanes sit out)")
for K, nb in ((16, 2), (24, 3), (32, 4), (48, 6)):
    n = sum(h[8:8 + nb])
    l = sum(h[24:24 + nb])
    saved, cost = n * c_shade, l / 64.0 * c_trace
    print("K=%2d: passes deferred %9d (%.1f %% of all), lanes %10d; saved %.3g, cost %.3g cycles; predicted loop time %+.1f %%" % (
        K, n, 100.0 * n / max(1, tot), l, saved, cost, -100.0 * (saved - cost) / st["cyc_loop"]))
