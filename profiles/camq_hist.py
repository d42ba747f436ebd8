"""Step 0: C2's refill passes by lanes refilled (the RT_CAMQ_HIST scratch build, profiles/camq_hist_variant.patch),
and the first-order price of generating camera rays with the whole wave at every refill."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "real-time-ray-tracing-engine_amd"))
from rtx.lib import load
from rtx.render import Renderer, camera_frame
from rtx.scene import load_scene

GEN_VALU = 123       # the parent's refill pass: decision 21 + camera_ray 101 (profiles/parked_after_asm_blocks.txt)
POP_VALU = 25        # a pop, as estimated before it was written (this build: decision 7 + pop 17 + origin 10 = 34)
SQ_INSTS_VALU = 2166e6  # the parent's C2 frame (profiles/parked_after_C2_pmc_table.txt)

L = load()
S = load_scene(os.path.join(ROOT, "real-time-ray-tracing-engine_amd", "scenes", "three_spheres.json"))
f = camera_frame(S.camera_desc(image_width=1920, samples_per_pixel=64, max_depth=8))
with Renderer(S) as R:
    st = R.stats(f, seed=42)
    h = (C.c_uint64 * 32)()
    L.rtk_camq_hist.argtypes = [C.c_void_p]
    assert L.rtk_camq_hist(h) == 0
h = list(h)
print("STATS", json.dumps(st))
print("# refill passes of C2 (1920x1080, 64 strata, depth 8; STATS instance: the schedule is the parent's)")
print("# lanes refilled | passes | lanes")
for b in range(8):
    print("%2d-%2d %10d %12d" % (8 * b + 1, 8 * b + 8, h[b], h[8 + b]))
passes, lanes = sum(h[:8]), sum(h[8:16])
print("# passes %d, lanes refilled %d (samples %d), mean lanes per pass %.1f" % (passes, lanes, st["samples"], lanes / max(1, passes)))
print("# trips %d, of them without a refill pass %d; batches generated %d (samples / 64 = %d)" % (
    st["wave_trips"], h[16], h[17], st["samples"] // 64))
price = (passes * GEN_VALU - st["samples"] / 64.0 * GEN_VALU - passes * POP_VALU) / SQ_INSTS_VALU
print("# first-order price: (passes x %d - samples / 64 x %d - passes x %d) / SQ_INSTS_VALU %.4g = %.1f %% of the frame's VALU wave instructions" % (
    GEN_VALU, GEN_VALU, POP_VALU, SQ_INSTS_VALU, 100.0 * price))
