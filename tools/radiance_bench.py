#!/usr/bin/env python3
"""Radiance queries measured beside the render.

    python tools/radiance_bench.py [--scenes three_spheres bouncing_seed42 cornell_fog] [--width 1920]
                                   [--strata 16] [--depth 8] [--reps 5] [--warm 2] [--rounds 3]

Per scene, a `width` x (width * 9 / 16) frame of the scene's camera with
`strata` strata (a square) and max_depth `depth`, RT_OUT_SUM, on one build in
one process:
  render         rt_render_device over the strata in one launch (the yardstick:
                 the same integrator with staged nodes, cost-ordered 8 x 8
                 tiles and regeneration across pixels),
  calls          rt_radiance_device on the render's own camera rays
                 (rt_camera_rays, row-major): one one-sample call per stratum,
                 accumulated -- its sums are asserted against the render's,
  calls_tile     the same with each stratum's rays in the render's 8 x 8 tile
                 order (a wavefront's 64 rays cover a tile, not a row segment),
  calls_random   the same in a seeded permutation,
  one            one call with the pixel-centre rays (rt_pixel_ray's
                 expression) and samples = strata, row-major: the in-lane
                 sample loop,
  one_random     the same rays in the permutation.
Each is timed between HIP events: the mean of `reps` repetitions after `warm`,
`rounds` times over, the variants alternating -- the rounds' spread (highest
over lowest mean) is the noise a ratio has to exceed.  One JSON line per scene."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "real-time-ray-tracing-engine_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from trace_bench import PKG, event_ms, frame_rays, orders, say  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="*", default=["three_spheres", "bouncing_seed42", "cornell_fog"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--strata", type=int, default=16)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("radiance_bench.py measures on a GPU: none found")
    from rtx import abi
    from rtx.render import Renderer, camera_frame, camera_rays
    from rtx.scene import load_scene
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    seed = 7
    for name in a.scenes:
        S = load_scene(os.path.join(PKG, "scenes", name + ".json"))
        f = camera_frame(S.camera_desc(image_width=a.width, aspect_ratio=16.0 / 9.0, samples_per_pixel=a.strata,
                                       max_depth=a.depth))
        H, W, K = f.image_height, f.image_width, f.sqrt_spp * f.sqrt_spp
        n = H * W
        order = orders(H, W)

        def on_device(rays):
            return torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1)).to(dev)

        cam = {o: [] for o in ("rows", "tile", "random")}
        for k in range(K):
            r = camera_rays(f, seed, k)
            for o in cam:
                cam[o].append(on_device(r[order[o]]))
        centre = frame_rays(f).reshape(-1)
        centres = {o: on_device(centre[order[o]]) for o in ("rows", "random")}
        kw = dict(seed=seed, max_depth=f.max_depth, background=f.background)
        with Renderer(S) as R:
            info = R.info()
            frame = torch.zeros((H, W, 3), dtype=torch.float64, device=dev)
            rgb = torch.zeros((n, 3), dtype=torch.float64, device=dev)

            def render():
                R.render_device(f, frame.data_ptr(), st.cuda_stream, seed=seed, samples=(0, K),
                                output=abi.RT_OUT_SUM, accumulate=0)

            def calls(o):
                def run():
                    for k in range(K):
                        R.radiance_device(cam[o][k].data_ptr(), rgb.data_ptr(), n, samples=1, first_sample=k,
                                          accumulate=1 if k else 0, stream_ptr=st.cuda_stream, **kw)
                return run

            def one(o):
                def run():
                    R.radiance_device(centres[o].data_ptr(), rgb.data_ptr(), n, samples=K, stream_ptr=st.cuda_stream,
                                      **kw)
                return run

            # the same light: stratum by stratum the bits are the render's (tests/test_radiance_gpu.py);
            # the sums differ only by the order of the render's LDS additions
            render()
            calls("rows")()
            torch.cuda.synchronize()
            want, got = frame.cpu().numpy().reshape(n, 3), rgb.cpu().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(want)), name
            scale = np.maximum(np.abs(np.nan_to_num(want)), 1.0)
            worst = float((np.abs(np.nan_to_num(got) - np.nan_to_num(want)) / scale).max())
            assert worst < 1e-9, (name, worst)  # reported beside the timings
            variants = {"render": render, "calls": calls("rows"), "calls_tile": calls("tile"),
                        "calls_random": calls("random"), "one": one("rows"), "one_random": one("random")}
            ms = {v: [] for v in variants}
            for _ in range(a.rounds):  # alternating: the spread and the comparison from one process
                for v, fn in variants.items():
                    ms[v].append(event_ms(torch, st, fn, a.reps, a.warm))
            mean = {v: sum(x) / len(x) for v, x in ms.items()}
            out = dict(scene=name, width=W, height=H, strata=K, max_depth=f.max_depth, rays=n,
                       features=info["features"], bvh_arity=info["bvh_arity"], n_nodes=info["n_nodes"],
                       reps=a.reps, warm=a.warm, sum_vs_render_rel=worst)
            for v in variants:
                out[v + "_ms"] = [round(x, 3) for x in ms[v]]
                out[v + "_spread"] = round(max(ms[v]) / min(ms[v]), 3)
                if v != "render":
                    out[v + "_over_render"] = round(mean[v] / mean["render"], 3)
            out["render_Msamples_per_s"] = round(n * K / mean["render"] / 1e3, 1)
            out["calls_Msamples_per_s"] = round(n * K / mean["calls"] / 1e3, 1)
            out["one_Msamples_per_s"] = round(n * K / mean["one"] / 1e3, 1)
            say(**out)


if __name__ == "__main__":
    main()
