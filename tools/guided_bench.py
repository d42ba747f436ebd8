#!/usr/bin/env python3
"""Guided sampling measured.

    python tools/guided_bench.py time    [--scene cornell] [--width 1920] [--reps 200]
    python tools/guided_bench.py kernels TRACE.csv --time-log profiles/guided_time.log
    python tools/guided_bench.py quality [--width 1080] [--ref-spp 4096] [--thresholds 0.1 0.2 0.3]

time:    a 16:9 frame of `scene` (1920x1080): pose A with 8 batches of 2 strata
         of an AdaptiveRenderer (threshold 0) under GuidedDisplay and its
         displayed history, pose B (tools/temporal_bench.py poses) with 2
         batches of 2 and the display's blend; HIP events around `reps` calls
         after a warm-up, the whole set `repeats` times in one run:
           select_ms   rt_guided_select_device over every tile of the frame: the
                       selection kernel and the compaction it shares with
                       rt_adaptive_select_device,
           moments_ms  rt_adaptive_select_device over the same list (the
                       renderer's own rule: 16 B per pixel and the same
                       compaction), beside it,
           copy_GBps   a device-to-device hipMemcpyAsync of the fp64 frame, read +
                       written bytes over its time (measured here, no data-sheet
                       figure),
           floor_ms    the selection kernel's compulsory bytes at that bandwidth:
                       per pixel 16 B of col + 8 B of variance read = 24 B, per
                       tile 4 B list + 4 B strata read and 4 B flag + 8 B error +
                       8 B count written = 28 B.
kernels: the selection kernel alone.  Two kernels of one call cannot be told
         apart by events around the call, so this reads the per-dispatch rows of
         a `rocprofv3 --kernel-trace --output-format csv -- python
         tools/guided_bench.py time` run of its own (tracing slows the host:
         the event figures come from the run without it), drops each kernel's
         first `skip` launches and reports the selection kernel's and the
         compaction's mean, median and minimum beside the floor of the time
         log's last `time` line.
quality: cornell and cornell_fog, `width` wide, depth 8: 64 strata at pose A in 8
         batches of 8 and its displayed history, as
         tools/temporal_variance_bench.py builds it; then at pose B batches of 2
         up to 64 nominal strata, a display frame after every batch, once under
         TemporalVarianceDisplay (the baseline) and once under GuidedDisplay per
         threshold (min_count and floor at their defaults; the wrapped
         renderer's own rule at threshold 0 in every run).  At 4, 16 and 64
         nominal strata: tile-strata traced, active tiles, RMSE of
         clip(image, 0, 1) against a `ref-spp`-strata render at pose B with
         another seed, and the wall time since the move (host clock, the device
         synchronised after every batch's step() and image(); the RMSE's own
         work excluded).
One JSON line per result."""
import argparse
import ctypes as C
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "real-time-ray-tracing-engine_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from temporal_bench import event_ms, poses, say  # noqa: E402

BYTES_PER_PIXEL = 16 + 8
BYTES_PER_TILE = 4 + 4 + 4 + 8 + 8
MARKS = (4, 16, 64)  # nominal strata at pose B
BS_B = 2


def run_time(a):
    import torch
    from rtx import adaptive, progressive
    from rtx.guided import GuidedDisplay
    from rtx.lib import check
    from rtx.render import Renderer
    from rtx.scene import load_scene
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    hip = progressive._hip()
    S = load_scene(os.path.join(PKG, "scenes", a.scene + ".json"))
    fA, fB = poses(S, image_width=a.width, aspect_ratio=16.0 / 9.0, samples_per_pixel=16, max_depth=8)
    h, w = fA.image_height, fA.image_width
    with Renderer(S) as R:
        ar = adaptive.for_renderer(R, fA, seed=a.seed, threshold=0.0, batch_strata=BS_B)
        gd = GuidedDisplay(ar, a.threshold, min_count=float("inf"))  # pose A: nothing retires
        for _ in range(8):
            gd.step()
        gd.image()
        gd.min_count = a.min_count
        gd.reset(fB)
        active = [ar.n_tiles]
        for _ in range(2):
            gd.step()
            active.append(ar.n_active)
        gd.image()
        torch.cuda.synchronize()
        tiles = ar.n_tiles
        every = torch.arange(tiles, dtype=torch.int32, device=dev)
        out = torch.empty_like(every)
        count = torch.zeros((1,), dtype=torch.int32, device=dev)
        err, num = torch.empty((tiles,), dtype=torch.float64, device=dev), torch.empty((tiles,), dtype=torch.float64,
                                                                                      device=dev)
        frame_copy = torch.empty_like(ar.acc)
        L = gd.guided.lib

        def p(t):
            return C.c_void_p(t.data_ptr())

        def select():
            check(L.rt_guided_select_device(C.byref(fB), p(gd.hist[1]), p(gd.v_out), p(ar.tile_strata), 0,
                                            a.threshold, gd.floor, a.min_count, p(every), tiles, p(out), p(count),
                                            p(err), p(num), C.c_void_p(st.cuda_stream)))

        def moments():
            check(L.rt_adaptive_select_device(p(ar.s1), p(ar.s2), p(ar.tile_strata), BS_B, C.byref(fB), a.threshold,
                                              1e-3, 2, p(every), tiles, p(out), p(count), p(err),
                                              C.c_void_p(st.cuda_stream)))

        def copy():
            rc = hip.hipMemcpyAsync(p(frame_copy), p(ar.acc), C.c_size_t(ar.acc.numel() * 8), 3,
                                    C.c_void_p(st.cuda_stream))
            assert rc == 0

        res = {}
        for _ in range(a.repeats):  # the whole set again: the run-to-run spread, in one process
            for key, fn in (("select", select), ("moments", moments), ("copy", copy)):
                res.setdefault(key, []).append(event_ms(torch, st, fn, a.reps))
        select()
        torch.cuda.synchronize()
        kept = int(count.item())
        best = {k: min(v) for k, v in res.items()}
        bw = 2 * ar.acc.numel() * 8 / (best["copy"] * 1e-3)
        floor_bytes = BYTES_PER_PIXEL * h * w + BYTES_PER_TILE * tiles
        floor_ms = floor_bytes / bw * 1e3
        say(run="time", scene=a.scene, width=w, height=h, tiles=tiles, reps=a.reps, repeats=a.repeats,
            threshold=a.threshold, min_count=a.min_count, active_after_each_batch=active, kept_of_all_tiles=kept,
            select_ms=round(best["select"], 5), moments_ms=round(best["moments"], 5),
            all_ms={k: [round(x, 5) for x in v] for k, v in res.items()}, copy_GBps=round(bw / 1e9, 1),
            bytes_per_pixel=BYTES_PER_PIXEL, bytes_per_tile=BYTES_PER_TILE, floor_bytes=floor_bytes,
            floor_ms=round(floor_ms, 5), select_over_floor=round(best["select"] / floor_ms, 2))


def run_kernels(a):
    last = None
    for line in open(a.time_log):
        line = line.strip()
        if line.startswith("{") and json.loads(line).get("run") == "time":
            last = json.loads(line)
    if last is None:
        sys.exit("no `time` line in %s" % a.time_log)
    by = {}
    rows = [r for r in csv.DictReader(open(a.trace)) if r.get("Kind", "KERNEL_DISPATCH") == "KERNEL_DISPATCH"]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        for key in ("guided_error_kernel", "adaptive_compact_kernel", "adaptive_error_kernel"):
            if key in r["Kernel_Name"]:
                by.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    out = dict(run="kernels", trace=os.path.basename(a.trace), skip=a.skip, width=last["width"],
               height=last["height"], tiles=last["tiles"], copy_GBps=last["copy_GBps"], floor_ms=last["floor_ms"])
    for key, ms in by.items():
        ms = ms[a.skip:] or ms
        out[key] = dict(launches=len(ms), mean_ms=round(statistics.fmean(ms), 5),
                        median_ms=round(statistics.median(ms), 5), min_ms=round(min(ms), 5))
    if "guided_error_kernel" in out:
        out["kernel_over_floor"] = round(out["guided_error_kernel"]["median_ms"] / last["floor_ms"], 2)
    say(**out)


def run_quality(a):
    import torch
    from rtx import abi, adaptive
    from rtx.guided import GuidedDisplay
    from rtx.render import Renderer
    from rtx.scene import load_scene
    from rtx.temporal import TemporalVarianceDisplay
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)

    def rmse(img, ref):
        return float(torch.sqrt(torch.mean((img.nan_to_num(0.0).clamp(0, 1) - ref.nan_to_num(0.0).clamp(0, 1)) ** 2)))

    for name in a.scenes:
        S = load_scene(os.path.join(PKG, "scenes", name + ".json"))
        cam = dict(image_width=a.width, max_depth=8)
        fA, fB = poses(S, samples_per_pixel=64, **cam)
        _, fr = poses(S, samples_per_pixel=a.ref_spp, **cam)
        with Renderer(S) as R:
            ref = torch.zeros((fr.image_height, fr.image_width, 3), dtype=torch.float64, device=dev)
            R.render_device(fr, ref.data_ptr(), st.cuda_stream, seed=a.seed + 1000, output=abi.RT_OUT_SCALED,
                            accumulate=0)
            torch.cuda.synchronize()
            for thr in [None] + list(a.thresholds):
                ar = adaptive.for_renderer(R, fA, seed=a.seed, threshold=0.0, batch_strata=8)
                d = TemporalVarianceDisplay(ar) if thr is None else GuidedDisplay(ar, thr, min_count=float("inf"))
                while not ar.done:  # pose A: 64 strata everywhere
                    d.step()
                d.image()
                if thr is not None:
                    d.min_count = a.min_count
                ar.batch_strata = BS_B
                d.reset(fB)
                torch.cuda.synchronize()
                wall, marks, active = 0.0, {}, []
                for k in range(MARKS[-1] // BS_B):
                    t0 = time.perf_counter()
                    d.step()
                    img = d.image()
                    torch.cuda.synchronize()
                    wall += time.perf_counter() - t0
                    active.append(ar.n_active)
                    nominal = (k + 1) * BS_B
                    if nominal in MARKS:
                        marks[nominal] = dict(tile_strata=int(ar.tile_strata.sum()), active_tiles=ar.n_active,
                                              rmse=round(rmse(img, ref), 5), wall_ms=round(wall * 1e3, 2))
                    if ar.done:
                        break
                say(run="quality", scene=name, width=fB.image_width, height=fB.image_height, tiles=ar.n_tiles,
                    ref_spp=a.ref_spp, display="baseline" if thr is None else "guided", threshold=thr,
                    min_count=None if thr is None else a.min_count, strata_a=64, batch_strata_b=BS_B,
                    at_nominal_strata=marks, active_after_each_batch=active)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time", "kernels", "quality"])
    ap.add_argument("trace", nargs="?", help="kernels: a rocprofv3 *_kernel_trace.csv")
    ap.add_argument("--time-log", default=os.path.join(ROOT, "profiles", "guided_time.log"))
    ap.add_argument("--skip", type=int, default=5, help="kernels: launches per kernel to drop (warm-up)")
    ap.add_argument("--scene", default="cornell")
    ap.add_argument("--scenes", nargs="*", default=["cornell", "cornell_fog"])
    ap.add_argument("--width", type=int, default=0, help="time: default 1920; quality: default 1080")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3, help="time: how often the whole set is measured")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--threshold", type=float, default=0.2, help="time: the selection's threshold")
    ap.add_argument("--thresholds", type=float, nargs="*", default=[0.1, 0.2, 0.3])
    ap.add_argument("--min-count", type=float, default=8.0)
    ap.add_argument("--ref-spp", type=int, default=4096)
    a = ap.parse_args()
    if a.mode == "kernels":
        if not a.trace:
            sys.exit("kernels: name the trace CSV")
        return run_kernels(a)
    import torch
    if not torch.cuda.is_available():
        sys.exit("guided_bench.py measures on a GPU: none found")
    if a.mode == "time":
        a.width = a.width or 1920
        run_time(a)
    else:
        a.width = a.width or 1080
        run_quality(a)


if __name__ == "__main__":
    main()
