#!/usr/bin/env python3
"""Ray queries measured.

    python tools/trace_bench.py [--scenes three_spheres bouncing_seed42 cloud] [--width 1920]
                                [--reps 20] [--warm 5] [--rounds 3]

Per scene, the pixel-centre rays of a `width` x (width * 9 / 16) frame of the
scene's camera (rt_pixel_ray's expression, vectorised) through rt_trace_device
in three orders:
  tile    the guide kernel's: 8 x 8 tiles row-major, a tile's 64 pixels
          row-major within it (one wavefront per tile),
  rows    row-major over the frame,
  random  a seeded permutation,
each timed between HIP events: the mean of `reps` calls after `warm` calls,
`rounds` times over -- the rounds' spread is the run-to-run noise a difference
has to exceed.  Beside them, timed the same way in the same process and
alternating with the query rounds: one stratum of rt_render_guides_device of
the same frame (the yardstick: the same tree and unstaged nodes, plus a camera
ray and an albedo).  Then `pick`: one ray, host call to host result
(Renderer.pick), by the host clock, best of 20.
Scenes: the committed ones by name, and `cloud`: 100,000 random spheres.
One JSON line per result."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "real-time-ray-tracing-engine_amd")
sys.path.insert(0, PKG)


def say(**kw):
    print(json.dumps(kw), flush=True)


def cloud_doc(n, seed=1):
    """n small spheres in a 100-unit cube over a ground sphere."""
    import numpy as np
    rng = np.random.default_rng(seed)
    c = rng.uniform(-50, 50, size=(n, 3))
    r = rng.uniform(0.05, 0.4, size=n)
    world = [{"type": "sphere", "center": list(map(float, c[k])), "radius": float(r[k]), "material": "m%d" % (k % 3)}
             for k in range(n)]
    world.append({"type": "sphere", "center": [0, -1000, 0], "radius": 940, "material": "m0"})
    return {"camera": {"vfov": 50.0, "lookfrom": [0, 20, 110], "lookat": [0, 0, 0], "background": [0.7, 0.8, 1.0]},
            "materials": {"m0": {"type": "lambertian", "albedo": [0.5, 0.5, 0.5]},
                          "m1": {"type": "metal", "albedo": [0.8, 0.7, 0.6], "fuzz": 0.1},
                          "m2": {"type": "dielectric", "refraction_index": 1.5}},
            "world": world}


def frame_rays(f):
    """[H, W] RAY_DTYPE: rt_pixel_ray(f, i, j) for every pixel."""
    import numpy as np
    from rtx.render import RAY_DTYPE
    v = lambda x: np.array([x.x, x.y, x.z])  # noqa: E731
    H, W = f.image_height, f.image_width
    i = np.arange(W, dtype=np.float64)[None, :, None]
    j = np.arange(H, dtype=np.float64)[:, None, None]
    r = np.zeros((H, W), dtype=RAY_DTYPE)
    r["origin"] = v(f.center)
    r["direction"] = v(f.pixel00_loc) + i * v(f.pixel_delta_u) + j * v(f.pixel_delta_v) - v(f.center)
    r["t_max"] = np.inf
    return r


def orders(H, W, seed=1):
    """name -> the frame's pixel indices (row-major numbering) in that order."""
    import numpy as np
    idx = np.arange(H * W).reshape(H, W)
    th, tw = (H + 7) // 8, (W + 7) // 8
    pad = np.full((th * 8, tw * 8), -1)
    pad[:H, :W] = idx
    tile = pad.reshape(th, 8, tw, 8).transpose(0, 2, 1, 3).reshape(-1)
    return {"tile": tile[tile >= 0], "rows": idx.reshape(-1), "random": np.random.default_rng(seed).permutation(H * W)}


def event_ms(torch, stream, fn, reps, warm):
    for _ in range(warm):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record(stream)
    for _ in range(reps):
        fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="*", default=["three_spheres", "bouncing_seed42", "cloud"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--cloud", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("trace_bench.py measures on a GPU: none found")
    from rtx import abi
    from rtx.render import HIT_DTYPE, Renderer, camera_frame
    from rtx.scene import load_scene
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    for name in a.scenes:
        S = load_scene(cloud_doc(a.cloud) if name == "cloud" else os.path.join(PKG, "scenes", name + ".json"))
        f = camera_frame(S.camera_desc(image_width=a.width, aspect_ratio=16.0 / 9.0, samples_per_pixel=1))
        H, W = f.image_height, f.image_width
        rays = frame_rays(f).reshape(-1)
        n = H * W
        with Renderer(S) as R:
            info = R.info()
            hits = torch.empty(n * HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            guides = torch.zeros((H, W, abi.RT_GUIDE_CHANNELS), dtype=torch.float64, device=dev)
            dev_rays, ref = {}, None
            for order, idx in orders(H, W).items():
                dev_rays[order] = torch.from_numpy(np.ascontiguousarray(rays[idx]).view(np.uint8).reshape(-1)).to(dev)
                # the three orders answer alike, ray for ray
                R.trace_device(dev_rays[order].data_ptr(), hits.data_ptr(), n, st.cuda_stream)
                got = np.empty(n, dtype=HIT_DTYPE)
                got[idx] = hits.cpu().numpy().view(HIT_DTYPE)
                assert ref is None or got.tobytes() == ref.tobytes(), order
                ref = got

            def guide():
                R.render_guides_device(f, guides.data_ptr(), st.cuda_stream, seed=7, samples=(0, 1), accumulate=0)

            ms = {k: [] for k in ("guides", "tile", "rows", "random")}
            for _ in range(a.rounds):  # alternating: the spread and the comparison from one process
                ms["guides"].append(event_ms(torch, st, guide, a.reps, a.warm))
                for order in ("tile", "rows", "random"):
                    p = dev_rays[order].data_ptr()
                    ms[order].append(event_ms(
                        torch, st, lambda: R.trace_device(p, hits.data_ptr(), n, st.cuda_stream), a.reps, a.warm))
            mean = {k: sum(v) / len(v) for k, v in ms.items()}
            pick = []
            for _ in range(20):
                t0 = time.perf_counter()
                R.pick(f, W // 2, H // 2)
                pick.append((time.perf_counter() - t0) * 1e3)
            say(scene=name, width=W, height=H, rays=n, hits=int((ref["object"] >= 0).sum()),
                features=info["features"], bvh_arity=info["bvh_arity"], n_nodes=info["n_nodes"],
                reps=a.reps, warm=a.warm,
                guides_ms=[round(x, 4) for x in ms["guides"]], tile_ms=[round(x, 4) for x in ms["tile"]],
                rows_ms=[round(x, 4) for x in ms["rows"]], random_ms=[round(x, 4) for x in ms["random"]],
                tile_Mrays_per_s=round(n / mean["tile"] / 1e3, 1), rows_Mrays_per_s=round(n / mean["rows"] / 1e3, 1),
                random_Mrays_per_s=round(n / mean["random"] / 1e3, 1),
                tile_over_guides=round(mean["tile"] / mean["guides"], 3),
                rows_over_tile=round(mean["rows"] / mean["tile"], 3),
                random_over_tile=round(mean["random"] / mean["tile"], 3),
                pick_ms_best_of_20=round(min(pick), 4))


if __name__ == "__main__":
    main()
