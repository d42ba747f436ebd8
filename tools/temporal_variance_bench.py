#!/usr/bin/env python3
"""Temporal variance measured.

    python tools/temporal_variance_bench.py time    [--configs C2 C3 C4] [--reps 50]
    python tools/temporal_variance_bench.py quality [--width 1080] [--ref-spp 4096]

time:    per config (bench.py CONFIGS: its scene, width and depth): pose A with 8
         batches of 2 strata of an AdaptiveRenderer (threshold 0) and its
         displayed history, pose B (tools/temporal_bench.py poses) with 2
         batches of 2; HIP events around `reps` calls after a warm-up, in one
         run:
           temporal_ms           rt_temporal_device at pose B with A's history,
           temporal_variance_ms  rt_temporal_variance_device on the same inputs
                                 (and their ratio beside 308 / 272, the bytes'),
           guided_ms             rt_denoise_variance_device on the blend's frame,
           given_ms              rt_denoise_given_variance_device on the blend,
           estimate_ms           call 1 of image(): rt_denoise_variance_device,
                                 passes -1,
           image_ms              TemporalVarianceDisplay.image(), three calls,
           temporal_display_ms   TemporalDisplay.image(),
           guided_display_ms     VarianceGuidedDisplay.image(),
           copy_GBps             a device-to-device hipMemcpyAsync of the fp64
                                 frame, read + written bytes over its time,
           floor_ms              the new temporal kernel's compulsory bytes at
                                 that bandwidth: temporal_bench's 272 B per pixel
                                 + 8 B variance_now + 8 B variance_out + 4 B var
                                 + 4 x 4 B var taps = 308 B.
quality: cornell and cornell_fog: 64 strata at pose A in 8 batches of 8, image(),
         the move, then 1, 4, 16 and 64 strata at pose B; RMSE of
         clip(image, 0, 1) against a `ref-spp`-strata render at pose B with
         another seed, six columns: raw; restart + shipped filter; restart +
         variance-guided; blend alone; blend + shipped filter (TemporalDisplay);
         blend + variance-guided with the carried variance
         (TemporalVarianceDisplay).  The shipped RT_TEMPORAL_* and RT_DENOISE_*
         defaults, nothing tuned.
One JSON line per result."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "real-time-ray-tracing-engine_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from temporal_bench import BYTES_PER_PIXEL, event_ms, poses, say  # noqa: E402

VARIANCE_BYTES_PER_PIXEL = BYTES_PER_PIXEL + 8 + 8 + 4 + 4 * 4
BATCHES = {1: 1, 4: 2, 16: 8, 64: 8}  # strata at pose B -> batches
COLUMNS = ("raw", "restart_shipped", "restart_guided", "blend", "blend_shipped", "blend_carried")


def run_time(a):
    import torch
    from bench import CONFIGS
    from rtx import adaptive, progressive
    from rtx.denoise import VarianceGuidedDisplay
    from rtx.render import Renderer
    from rtx.scene import load_scene
    from rtx.temporal import TemporalDisplay, TemporalVarianceDisplay
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    hip = progressive._hip()
    for cfg in a.configs:
        name, width, _, depth = CONFIGS[cfg]
        S = load_scene(os.path.join(PKG, "scenes", name + ".json"))
        fA, fB = poses(S, image_width=a.width or width, samples_per_pixel=16, max_depth=depth)
        h, w = fA.image_height, fA.image_width
        with Renderer(S) as R:
            ar = adaptive.for_renderer(R, fA, seed=a.seed, threshold=0.0, batch_strata=2)
            # three displays over one renderer: they only read it
            tv, td, vd = TemporalVarianceDisplay(ar), TemporalDisplay(ar), VarianceGuidedDisplay(ar)
            for _ in range(8):
                ar.step()
            tv.image()
            td.image()
            for d in (tv, td, vd):
                d.reset(fB)
            for _ in range(2):
                ar.step()
            tv.image()
            td.image()
            vd.image()
            torch.cuda.synchronize()
            kept = float((tv.hist[1].view(torch.float32)[: h * w * 4].view(h, w, 4)[..., 3] > 4.5).double().mean())
            g, dd = tv.guides_done, tv.dd
            out = torch.empty_like(ar.acc)

            def plain():
                td.ops.temporal(fB, ar.acc, 1.0, ar.tile_strata, 0, td.guides, g, td.frame_prev, td.hist[0], None,
                                td.hist[1], td.blend)

            def carried():
                tv.ops.temporal_variance(fB, ar.acc, 1.0, ar.tile_strata, 0, tv.guides, g, tv.v_now, tv.frame_prev,
                                         tv.hist[0], None, tv.hist[1], tv.blend, tv.v_out)

            def guided():
                dd.ops.denoise_variance(fB, tv.blend, 1.0, None, tv.guides, g, None, None, 0, None, dd.workspace,
                                        dd.out, dd.var)

            def given():
                dd.ops.denoise_given_variance(fB, tv.blend, 1.0, None, tv.guides, g, tv.v_out, None, dd.workspace,
                                              dd.out, dd.var)

            def estimate():
                dd.ops.denoise_variance(fB, ar.acc, 1.0, ar.tile_strata, tv.guides, g, ar.s1, ar.s2, 2, tv._estimate,
                                        dd.workspace, dd.out, tv.v_now)

            def copy():
                rc = hip.hipMemcpyAsync(C.c_void_p(out.data_ptr()), C.c_void_p(ar.acc.data_ptr()),
                                        C.c_size_t(ar.acc.numel() * 8), 3, C.c_void_p(st.cuda_stream))
                assert rc == 0

            res = {}
            for rep in range(a.repeats):  # the whole set again: the run-to-run spread, in one process
                for key, fn in (("temporal", plain), ("temporal_variance", carried), ("guided", guided),
                                ("given", given), ("estimate", estimate), ("image", tv.image),
                                ("temporal_display", td.image), ("guided_display", vd.image), ("copy", copy)):
                    res.setdefault(key, []).append(event_ms(torch, st, fn, a.reps))
            best = {k: min(v) for k, v in res.items()}
            bw = 2 * ar.acc.numel() * 8 / (best["copy"] * 1e-3)
            floor_ms = VARIANCE_BYTES_PER_PIXEL * h * w / bw * 1e3
            ratios = [c / p for c, p in zip(res["temporal_variance"], res["temporal"])]
            say(run="time", config=cfg, scene=name, width=w, height=h, reps=a.reps, repeats=a.repeats,
                temporal_ms=round(best["temporal"], 4), temporal_variance_ms=round(best["temporal_variance"], 4),
                variance_over_plain=round(best["temporal_variance"] / best["temporal"], 3),
                variance_over_plain_runs=[round(r, 3) for r in ratios],
                bytes_ratio=round(VARIANCE_BYTES_PER_PIXEL / BYTES_PER_PIXEL, 3),
                guided_ms=round(best["guided"], 4), given_ms=round(best["given"], 4),
                given_over_guided=round(best["given"] / best["guided"], 3), estimate_ms=round(best["estimate"], 4),
                image_ms=round(best["image"], 4), temporal_display_ms=round(best["temporal_display"], 4),
                guided_display_ms=round(best["guided_display"], 4),
                image_over_temporal_display=round(best["image"] / best["temporal_display"], 3),
                image_over_guided_display=round(best["image"] / best["guided_display"], 3),
                all_ms={k: [round(x, 4) for x in v] for k, v in res.items()},
                copy_GBps=round(bw / 1e9, 1), bytes_per_pixel=VARIANCE_BYTES_PER_PIXEL, floor_ms=round(floor_ms, 4),
                temporal_variance_over_floor=round(best["temporal_variance"] / floor_ms, 2),
                pixels_with_history=round(kept, 4))


def run_quality(a):
    import torch
    from rtx import abi, adaptive
    from rtx.render import Renderer
    from rtx.scene import load_scene
    from rtx.temporal import TemporalDisplay, TemporalVarianceDisplay
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)

    def rmse(img, ref):
        return float(torch.sqrt(torch.mean((img.nan_to_num(0.0).clamp(0, 1) - ref.nan_to_num(0.0).clamp(0, 1)) ** 2)))

    for name in a.scenes:
        S = load_scene(os.path.join(PKG, "scenes", name + ".json"))
        cam = dict(image_width=a.width, max_depth=8)
        fA, _ = poses(S, samples_per_pixel=64, **cam)
        _, fr = poses(S, samples_per_pixel=a.ref_spp, **cam)
        with Renderer(S) as R:
            ref = torch.zeros((fr.image_height, fr.image_width, 3), dtype=torch.float64, device=dev)
            R.render_device(fr, ref.data_ptr(), st.cuda_stream, seed=a.seed + 1000, output=abi.RT_OUT_SCALED,
                            accumulate=0)
            for k in a.strata:
                _, fB = poses(S, samples_per_pixel=k, **cam)
                ar = adaptive.for_renderer(R, fA, seed=a.seed, threshold=0.0, batch_strata=8)
                tv, td = TemporalVarianceDisplay(ar), TemporalDisplay(ar)
                while not ar.done:
                    ar.step()
                tv.image()
                td.image()
                bs = k // BATCHES.get(k, min(k, 8))
                ar.batch_strata = bs
                tv.reset(fB)
                td.reset(fB)
                while not ar.done:
                    ar.step()
                new = tv.image().clone()
                blend = tv.blend.clone()
                both = td.image().clone()
                ops, g = tv.dd.ops, tv.guides_done
                shipped = ops.denoise(fB, ar.acc, 1.0, ar.tile_strata, tv.guides, g).clone()
                guided = ops.denoise_variance(fB, ar.acc, 1.0, ar.tile_strata, tv.guides, g, ar.s1, ar.s2, bs).clone()
                h, w = fB.image_height, fB.image_width
                kept = float((tv.hist[1].view(torch.float32)[: h * w * 4].view(h, w, 4)[..., 3] > k + 0.5)
                             .double().mean())
                e = dict(zip(COLUMNS, (rmse(i, ref) for i in (ar.image(), shipped, guided, blend, both, new))))
                say(run="quality", scene=name, width=w, height=h, ref_spp=a.ref_spp, strata_a=64, strata_b=k,
                    batch_strata_b=bs, rmse={c: round(v, 5) for c, v in e.items()},
                    carried_over_temporal_display=round(e["blend_carried"] / e["blend_shipped"], 3),
                    carried_over_restart_guided=round(e["blend_carried"] / e["restart_guided"], 3),
                    carried_over_blend=round(e["blend_carried"] / e["blend"], 3),
                    best=min(e, key=e.get), pixels_with_history=round(kept, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time", "quality"])
    ap.add_argument("--configs", nargs="*", default=["C2", "C3", "C4"])
    ap.add_argument("--scenes", nargs="*", default=["cornell", "cornell_fog"])
    ap.add_argument("--width", type=int, default=0, help="time: 0 = the config's; quality: default 1080")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3, help="time: how often the whole set is measured")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--strata", type=int, nargs="*", default=sorted(BATCHES))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("temporal_variance_bench.py measures on a GPU: none found")
    if a.mode == "time":
        run_time(a)
    else:
        a.width = a.width or 1080
        run_quality(a)


if __name__ == "__main__":
    main()
