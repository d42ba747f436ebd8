"""Step 0: C2's trace passes by lanes traced, camera rays (bounce 0) apart from bounce rays (the RT_TRACE_HIST
scratch build of the parent, profiles/batch_hist_variant.patch; RTX_LIB names it), and the model of tracing
camera-ray batches at generation restated from those figures."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "real-time-ray-tracing-engine_amd"))
from rtx.lib import load
from rtx.render import Renderer, camera_frame
from rtx.scene import load_scene

TEST_VALU = 48          # a sphere root test (profiles/flat_table_blocks.md)
ORIGIN_VALU = 9         # of its fp64 operations, those that form oc and c
N_ROOTS = 3
SQ_INSTS_VALU = 1862e6  # the parent's C2 frame (profiles/albedo_after_C2_pmc_table.txt)

L = load()
S = load_scene(os.path.join(ROOT, "real-time-ray-tracing-engine_amd", "scenes", "three_spheres.json"))
f = camera_frame(S.camera_desc(image_width=1920, samples_per_pixel=64, max_depth=8))
with Renderer(S) as R:
    st = R.stats(f, seed=42)
    h = (C.c_uint64 * 32)()
    L.rtk_trace_hist.argtypes = [C.c_void_p]
    assert L.rtk_trace_hist(h) == 0
h = list(h)
print("STATS", json.dumps({k: v for k, v in sorted(st.items()) if not k.startswith("cyc_")}))
print("# trace passes of C2 (1920x1080, 64 strata, depth 8; STATS instance: the schedule is the parent's)")
print("# lanes traced | passes | camera-ray lanes | bounce-ray lanes")
for b in range(8):
    print("%2d-%2d %10d %12d %12d" % (8 * b + 1, 8 * b + 8, h[b], h[8 + b], h[16 + b]))
passes, cam, bnc = sum(h[:8]), sum(h[8:16]), sum(h[16:24])
print("# passes %d (trips %d, without a trace pass %d), lanes traced %d = camera %d + bounce %d (segments %d, samples %d)" % (
    passes, st["wave_trips"], h[24], cam + bnc, cam, bnc, st["segments"], st["samples"]))
print("# lane use of the trace %.3f; camera rays are %.1f %% of the traced lanes" % (
    (cam + bnc) / (64.0 * max(1, passes)), 100.0 * cam / max(1, cam + bnc)))
batches, shades = st["samples"] // 64, st["wave_shade_iters"]
after = batches + shades  # one full pass per batch; bounce rays arise from a shade pass only
part1 = (passes - after) * N_ROOTS * TEST_VALU
part2 = batches * N_ROOTS * ORIGIN_VALU
print("# model, part 1: passes %d -> at most %d batches + %d shade passes = %d: -%.0f M VALU (%.1f %% of %.0f M)" % (
    passes, batches, shades, after, part1 / 1e6, 100.0 * part1 / SQ_INSTS_VALU, SQ_INSTS_VALU / 1e6))
print("# model, part 2: %d batches x %d roots x %d operations: -%.0f M VALU (%.1f %%)" % (
    batches, N_ROOTS, ORIGIN_VALU, part2 / 1e6, 100.0 * part2 / SQ_INSTS_VALU))
