#!/usr/bin/env python3
"""Moving spheres and the rebuild measured.

    python tools/refit_bench.py [--sizes 486 100000 1000000] [--reps 20] [--log profiles/rebuild_bench.log]

Per size -- 486: bouncing_seed42 (bench.py's C3 scene, host tree, binary);
otherwise that many random spheres in [-50, 50]^3 over a ground sphere
(tests/test_device_bvh.py's world; from 65536 the device SAH builder, from 4096
a 4-wide tree) -- one JSON line each for

  move      move_ms: one rt_scene_move_spheres_device of every sphere but the
            ground (centres, item boxes, full refit), the mean of `reps` calls
            between HIP events; recreate_ms: rt_scene_destroy + rt_scene_create
            of the same description, host clock, the best of 3 (the host
            compile, the upload and the BVH build a move replaces);
            rebuild_ms: one rt_scene_rebuild_bvh of a second scene of the same
            description, host clock, the best of 3 after the first (which
            allocates the rebuild state: first_rebuild_ms); cost_ms, for a
            4-wide scene: rt_scene_bvh_cost of the same world created binary,
            host clock -- the download of the binary tree and the host's sum
            that a 4-wide rebuild contains for its binary_cost;
  walk      after 1, 10 and 100 steps of a random walk (every step adds a vector
            uniform in [-step, step]^3 to every moved sphere; step is stated in
            the line): frame_ms of one-stratum 1080p frames (HIP events, the
            mean of `reps`) and rt_scene_bvh_cost of the refitted scene, beside
            the same of a scene freshly created at those positions, and the
            largest pixel difference between the two scenes' frames; and of
            a second scene that made the same moves and then one
            rt_scene_rebuild_bvh (rebuilt_frame_ms, rebuilt_bvh_cost, that
            rebuild's host ms, and its largest pixel difference from the fresh
            scene: 0 where the fresh scene is the device SAH builder's);
  every_k   §7j's break-even arithmetic at each of those step counts: the
            frame time the refitted tree loses against the rebuilt one, and
            the frames after which a rebuild, or destroy + create, is repaid.
            rt_scene_bvh_cost of a 4-wide scene is creation's figure (rt_api.h):
            there only frame_ms shows the refitted tree's quality.

With --instances N [N ...] the script runs the live-transform leg instead
(log: profiles/set_transforms_bench.log): a world of N
translate(rotate_y(box)) instances of one box on a grid (6 N world quads under
2 N transform records), one JSON line each for

  set_transforms  set_ms: one rt_scene_set_transforms_device of every translate
            (the records, every item's box, full refit), the mean of `reps`
            calls between HIP events; recreate_ms: rt_scene_destroy +
            rt_scene_create of the same description, host clock, the best of 3.

The lines go to stdout and to --log.  No test asserts any of these numbers."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "real-time-ray-tracing-engine_amd")
sys.path.insert(0, PKG)

import numpy as np  # noqa: E402

LOG = None


def say(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if LOG:
        LOG.write(line + "\n")
        LOG.flush()


def random_world(n, seed=1):
    """tests/test_device_bvh.py random_spheres, built without the JSON detour."""
    from rtx import abi
    from rtx.scene import SceneDescription
    rng = np.random.default_rng(seed)
    c, r = rng.uniform(-50, 50, size=(n, 3)), rng.uniform(0.05, 0.4, size=n)
    S = SceneDescription()
    S.camera = {"aspect_ratio": 1.0, "vfov": 50.0, "lookfrom": [0, 20, 110], "lookat": [0, 0, 0],
                "background": [0.7, 0.8, 1.0]}
    mats = [S.add_material(abi.RT_MAT_LAMBERTIAN, texture=S.add_texture(abi.RT_TEX_SOLID, color=(0.5, 0.5, 0.5))),
            S.add_material(abi.RT_MAT_METAL, albedo=(0.8, 0.7, 0.6), fuzz=0.1),
            S.add_material(abi.RT_MAT_DIELECTRIC, refraction_index=1.5)]
    ids = [S.add_object(abi.RT_OBJ_SPHERE, material=mats[k % 3], a=c[k], s=r[k]) for k in range(n)]
    ids.append(S.add_object(abi.RT_OBJ_SPHERE, material=mats[0], a=(0, -1000, 0), s=940))
    S.world = S.add_list(ids)
    return S


def instance_world(n, seed=2):
    """n instances translate(rotate_y(box)) of one 6 x 9 x 6 box on a square grid of pitch 12, over a floor quad."""
    from rtx import abi
    from rtx.scene import SceneDescription, make_box_quads
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    S = SceneDescription()
    half = 6.0 * side
    S.camera = {"aspect_ratio": 1.0, "vfov": 50.0, "lookfrom": [0, 0.9 * half, 2.2 * half], "lookat": [0, 0, 0],
                "background": [0.7, 0.8, 1.0]}
    mat = S.add_material(abi.RT_MAT_LAMBERTIAN, texture=S.add_texture(abi.RT_TEX_SOLID, color=(0.6, 0.6, 0.6)))
    box = S.add_list([S.add_object(abi.RT_OBJ_QUAD, material=mat, a=q, b=u, c=v)
                      for q, u, v in make_box_quads([0, 0, 0], [6, 9, 6])])
    angles = rng.uniform(-45, 45, size=n)
    ids, translates = [], []
    for k in range(n):
        rot = S.add_object(abi.RT_OBJ_ROTATE_Y, child=box, s=float(angles[k]))
        offset = (12.0 * (k % side) - half, 0.0, 12.0 * (k // side) - half)
        translates.append(S.add_object(abi.RT_OBJ_TRANSLATE, child=rot, a=offset))
    ids = translates + [S.add_object(abi.RT_OBJ_QUAD, material=mat, a=(-2 * half, 0, -2 * half), b=(4 * half, 0, 0),
                                     c=(0, 0, 4 * half))]
    S.world = S.add_list(ids)
    return S, np.array(translates, dtype=np.int32)


def set_transforms_leg(args):
    """One line per instance count: every translate set on the device against destroy + create."""
    import torch
    from rtx.lib import check
    from rtx.render import Renderer
    for n in args.instances:
        S, ids = instance_world(n)
        offsets = np.array([[S.objects[i].a.x, S.objects[i].a.y, S.objects[i].a.z] for i in ids])
        stream = torch.cuda.current_stream()
        t = time.perf_counter()
        R = Renderer(S)
        create_ms = [(time.perf_counter() - t) * 1e3]
        info = R.info()
        for _ in range(3):  # destroy + create through the ABI alone, as the sphere leg does
            h = C.c_void_p()
            t = time.perf_counter()
            check(R.lib.rt_scene_destroy(R.handle))
            check(R.lib.rt_scene_create(C.byref(R._desc), 0, C.byref(h)))
            create_ms.append((time.perf_counter() - t) * 1e3)
            R.handle = h
        d_ids = torch.from_numpy(ids).cuda()
        d_new = torch.from_numpy(offsets + np.array([0.25, 0.0, -0.25])).cuda()  # the work does not depend on the values
        edit = lambda: R.set_transforms_device(d_ids.data_ptr(), d_new.data_ptr(), len(ids), stream.cuda_stream)  # noqa: E731
        for _ in range(3):
            edit()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record(stream)
        for _ in range(args.reps):
            edit()
        t1.record(stream)
        t1.synchronize()
        say(kind="set_transforms", instances=n, world_items=info["n_leaf_refs"], transforms_set=len(ids),
            builder=info["bvh_builder"], arity=info["bvh_arity"], nodes=info["n_nodes"],
            set_ms=t0.elapsed_time(t1) / args.reps, recreate_ms=min(create_ms[1:]),
            first_create_with_python_ms=create_ms[0])
        R.close()


def world(n):
    from rtx.scene import load_scene
    if n == 486:
        return load_scene(os.path.join(PKG, "scenes", "bouncing_seed42.json")), 0.05
    return random_world(n), 0.5


def frame_ms(torch, R, frame, buf, reps):
    """Mean device ms of a one-stratum frame (a progressive step), and the frame of stratum 0."""
    from rtx import abi
    stream = torch.cuda.current_stream()
    strata = frame.sqrt_spp * frame.sqrt_spp

    def step(k, acc):
        R.render_device(frame, buf.data_ptr(), stream.cuda_stream, seed=5, samples=(k % strata, 1),
                        output=abi.RT_OUT_SUM, accumulate=acc)
    for k in range(3):
        step(k, 1)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record(stream)
    for k in range(reps):
        step(k, 1)
    t1.record(stream)
    t1.synchronize()
    step(0, 0)
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps, buf.cpu().numpy().copy()


def main():
    global LOG
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[486, 100000, 1000000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--instances", type=int, nargs="+", default=None,
                    help="run the live-transform leg on worlds of this many box instances (e.g. 400 100000)")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    if args.log is None:
        args.log = os.path.join(ROOT, "profiles", "set_transforms_bench.log" if args.instances else "rebuild_bench.log")
    import torch
    from rtx import abi
    from rtx.lib import check
    from rtx.render import Renderer, camera_frame, describe_move
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    LOG = open(args.log, "a")
    if args.instances:
        set_transforms_leg(args)
        LOG.close()
        return
    for n in args.sizes:
        S, step = world(n)
        cam = S.camera_desc(image_width=1920, aspect_ratio=16.0 / 9.0, samples_per_pixel=64, max_depth=8)
        frame = camera_frame(cam)
        spheres = [i for i, o in enumerate(S.objects) if o.kind == abi.RT_OBJ_SPHERE and o.s < 100]
        ids = np.array(spheres, dtype=np.int32)
        home = np.array([[S.objects[i].a.x, S.objects[i].a.y, S.objects[i].a.z] for i in spheres])
        d_ids = torch.from_numpy(ids).cuda()
        buf = torch.zeros((frame.image_height, frame.image_width, 3), dtype=torch.float64, device="cuda")
        stream = torch.cuda.current_stream()
        t = time.perf_counter()
        R = Renderer(S)
        create_ms = [(time.perf_counter() - t) * 1e3]
        info = R.info()
        tree = dict(spheres=len(spheres), builder=info["bvh_builder"], arity=info["bvh_arity"], nodes=info["n_nodes"])
        for _ in range(3):  # destroy + create through the ABI alone: the description's ctypes view is kept
            h = C.c_void_p()
            t = time.perf_counter()
            check(R.lib.rt_scene_destroy(R.handle))
            check(R.lib.rt_scene_create(C.byref(R._desc), 0, C.byref(h)))
            create_ms.append((time.perf_counter() - t) * 1e3)
            R.handle = h
        # one move of everything: to where it is (the refit does the same work wherever the centres go)
        d_home = torch.from_numpy(home).cuda()
        move = lambda d_c: R.move_spheres_device(d_ids.data_ptr(), d_c.data_ptr(), len(ids), stream.cuda_stream)  # noqa: E731
        for _ in range(3):
            move(d_home)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record(stream)
        for _ in range(args.reps):
            move(d_home)
        t1.record(stream)
        t1.synchronize()
        # the rebuild, on a scene of its own: R keeps creation's topology for the walk
        R2 = Renderer(S)
        rebuild_ms = []
        for _ in range(4):
            t = time.perf_counter()
            took = R2.rebuild_bvh()
            rebuild_ms.append((time.perf_counter() - t) * 1e3)
        cost_ms = None
        if info["bvh_arity"] == 4:
            arity, S.bvh_arity = S.bvh_arity, 2
            with Renderer(S) as R3:
                cost_ms = []
                for _ in range(3):
                    t = time.perf_counter()
                    R3.bvh_cost()
                    cost_ms.append((time.perf_counter() - t) * 1e3)
            S.bvh_arity, cost_ms = arity, min(cost_ms)
        recreate_ms = min(create_ms[1:])
        say(kind="move", n=n, **tree, move_ms=t0.elapsed_time(t1) / args.reps, recreate_ms=recreate_ms,
            first_create_with_python_ms=create_ms[0], rebuilt=took, rebuild_ms=min(rebuild_ms[1:]),
            first_rebuild_ms=rebuild_ms[0], cost_ms=cost_ms, rebuilt_nodes=R2.info()["n_nodes"])
        ms0, _ = frame_ms(torch, R, frame, buf, args.reps)
        say(kind="walk", n=n, steps=0, step=step, frame_ms=ms0, bvh_cost=R.bvh_cost())
        rng = np.random.default_rng(9)
        at, done = home.copy(), 0
        for upto in (1, 10, 100):
            while done < upto:
                at = at + rng.uniform(-step, step, size=at.shape)
                d_at = torch.from_numpy(at).cuda()
                move(d_at)
                R2.move_spheres_device(d_ids.data_ptr(), d_at.data_ptr(), len(ids), stream.cuda_stream)
                done += 1
            torch.cuda.synchronize()
            ms, img = frame_ms(torch, R, frame, buf, args.reps)
            cost = R.bvh_cost()
            describe_move(S, ids, at)
            with Renderer(S) as F:
                fms, fimg = frame_ms(torch, F, frame, buf, args.reps)
                fcost = F.bvh_cost()
            t = time.perf_counter()
            took = R2.rebuild_bvh()
            walk_rebuild_ms = (time.perf_counter() - t) * 1e3
            rms, rimg = frame_ms(torch, R2, frame, buf, args.reps)
            say(kind="walk", n=n, steps=upto, step=step, frame_ms=ms, fresh_frame_ms=fms, slowdown=ms / fms,
                bvh_cost=cost, fresh_bvh_cost=fcost, max_pixel_diff=float(np.nanmax(np.abs(img - fimg))),
                rebuilt=took, rebuild_ms=walk_rebuild_ms, rebuilt_frame_ms=rms, rebuilt_bvh_cost=R2.bvh_cost(),
                rebuilt_max_pixel_diff=float(np.nanmax(np.abs(rimg - fimg))))
            lost = ms - rms
            say(kind="every_k", n=n, k=upto, lost_ms_per_frame=lost, rebuild_ms=walk_rebuild_ms,
                recreate_ms=recreate_ms, frames_to_repay_rebuild=walk_rebuild_ms / lost if lost > 0 else None,
                frames_to_repay_recreate=recreate_ms / lost if lost > 0 else None)
        R2.close()
        R.close()
    LOG.close()


if __name__ == "__main__":
    main()
