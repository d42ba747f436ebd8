"""The one-stratum (progressive) frames of C2: bench.py's device loop (progressive_rates), 64 frames, three
times in one process.  RTX_LIB names the library; prints one line.  python profiles/camq_progressive.py TAG"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "real-time-ray-tracing-engine_amd"))
import torch
from rtx.progressive import for_renderer, frame_bytes
from rtx.render import Renderer, camera_frame
from rtx.scene import load_scene

FRAMES = 64
dev = torch.device("cuda", 0)
S = load_scene(os.path.join(ROOT, "real-time-ray-tracing-engine_amd", "scenes", "three_spheres.json"))
f = camera_frame(S.camera_desc(image_width=1920, samples_per_pixel=64, max_depth=8))
ms = []
with Renderer(S, device=0) as R:
    pr = for_renderer(R, f, seed=5)
    out = torch.empty(pr.acc.shape, dtype=torch.uint8, device=dev)
    for _ in range(2):  # warm
        pr.step(1)
        frame_bytes(pr, out)
    for _ in range(3):
        torch.cuda.synchronize(dev)
        pr.reset()
        t0 = time.perf_counter()
        for _ in range(FRAMES):
            pr.step(1)
            frame_bytes(pr, out)
        torch.cuda.synchronize(dev)
        ms.append(round((time.perf_counter() - t0) * 1e3 / FRAMES, 4))
print(sys.argv[1], "C2 progressive device_ms_per_frame", ms, flush=True)
