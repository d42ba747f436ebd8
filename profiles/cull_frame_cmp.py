"""cull_frame_cmp.py P.npy B.npy: the C2 1080p frames of radiance sums (tools/frame_dump.py) of the parent's
library and of this build.  Pixels of the tiles the host twin of the reach test (tests/native/rt_tile_cull_check
masks) leaves with an empty mask must be bit-equal; all others within the order-of-adds bound 2 (n - 1) 2^-53."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "real-time-ray-tracing-engine_amd"))
from rtx.render import camera_frame
from rtx.scene import load_scene

a, b = np.load(sys.argv[1]), np.load(sys.argv[2])
assert a.shape == b.shape == (1080, 1920, 3)
path = os.path.join(ROOT, "real-time-ray-tracing-engine_amd", "scenes", "three_spheres.json")
doc = json.load(open(path))
f = camera_frame(load_scene(path).camera_desc(image_width=1920, samples_per_pixel=64, max_depth=8))
native = os.path.join(ROOT, "tests", "native")
subprocess.run(["make", "-s", "-C", native, "-f", "tile_cull.mk"], check=True)
args = [os.path.join(native, "build", "rt_tile_cull_check"), "masks", "1920", "1080"]
for v in (f.center, f.pixel00_loc, f.pixel_delta_u, f.pixel_delta_v):
    args += [float(x).hex() for x in v.tolist()]
args.append(str(len(doc["world"])))
for s in doc["world"]:
    args += [float(x).hex() for x in s["center"]] + [float(s["radius"]).hex()]
w = subprocess.run(args, capture_output=True, text=True, check=True).stdout.split()
m = np.array([int(x) for x in w[1:]]).reshape(135, 240)
sky = np.kron(m == 0, np.ones((8, 8), bool))
n = 64
bound = 2 * (n - 1) * 2.0 ** -53
rel = np.abs(a - b) / np.maximum(np.abs(a), 1e-300)
sky_bad = int((a[sky] != b[sky]).sum())
bad = int((rel > bound).sum())
print("frame_sums", sys.argv[1], sys.argv[2], "all-sky tiles %d of %d (popcounts %s): differing channels %d;" % (
    int((m == 0).sum()), m.size, np.bincount([bin(x).count("1") for x in m.ravel()]).tolist(), sky_bad),
    "elsewhere differing channels %d of %d, max relative difference %.3g (bound %.3g, n = 64), outside the bound: %d" % (
    int((a[~sky] != b[~sky]).sum()), int(a[~sky].size), rel.max(), bound, bad))
sys.exit(0 if bad == 0 and sky_bad == 0 else 1)
