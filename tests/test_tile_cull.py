"""The tile reach test (csrc/rt_cull.h tile_cone, root_unreachable): which roots
the camera rays of one 8x8 tile can reach, as the flat render loop asks once
per work unit.  "Unreachable" is a promise that the kernel's own root test
returns false for every ray of the tile; tests/native/rt_tile_cull_check holds
it to that with the kernel's camera_ray_jt + root_origin + sphere_root_origin,
over random pinhole cameras, tiles and spheres -- spheres tangent to a side of
the tile's pyramid from outside and inside within +-1e-6, +-1e-9 and +-1e-12
relative, spheres bisected to the function's own boundary, the camera on, just
inside and just outside a sphere, spheres behind the camera, huge ground
spheres, |oc| / r up to 1e6 and non-finite inputs -- at the jitter extremes of
three strata grids and 256 random jitters per pixel.  And it must not be
vacuous: at the benchmark's camera (three_spheres, 1920x1080) at least 36 % of
the tiles keep an empty mask (exact per-corner figure: 38.4 %) and the mean
popcount is at most 0.85 (exact: 0.72).  No GPU.
"""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
CHECK = os.path.join(NATIVE, "build", "rt_tile_cull_check")
SCENE = os.path.join(HERE, "..", "real-time-ray-tracing-engine_amd", "scenes", "three_spheres.json")
N_CASES = 2000


@pytest.fixture(scope="module")
def check():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "tile_cull.mk"], check=True)
    return CHECK


@pytest.mark.parametrize("seed", [1, 20261021])
def test_unreachable_is_never_wrong(check, seed):
    r = subprocess.run([check, "random", str(N_CASES), str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    w = r.stdout.split()
    assert w[0] == "OK"
    print(r.stdout)
    c = {k: tuple(int(x) for x in v.split("/")) for k, v in zip(w[5::2], w[6::2])}
    assert all(pairs == N_CASES for _, pairs in c.values())
    # the cases are there: the function's own boundary, the easy kinds, and rays behind each answer
    assert c["flip"][0] > N_CASES // 2 and c["behind"][0] > N_CASES // 2
    assert c["random"][0] > N_CASES // 4 and c["ground"][0] > N_CASES // 4 and c["camera_on"][0] > 0
    assert c["nonfinite"][0] == 0
    assert int(w[4]) > 10000 * N_CASES


def test_masks_at_the_benchmark_camera(check):
    with open(SCENE) as f:
        d = json.load(f)
    cam = d["camera"]
    args = [check, "hist", "1920", "1080", repr(float(cam["vfov"])), repr(float(cam["focus_dist"]))]
    for k in ("lookfrom", "lookat", "vup"):
        args += [repr(float(x)) for x in cam[k]]
    args.append(str(len(d["world"])))
    for s in d["world"]:
        assert s["type"] == "sphere"
        args += [repr(float(x)) for x in s["center"]] + [repr(float(s["radius"]))]
    r = subprocess.run(args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    w = r.stdout.split()
    assert w[0] == "HIST" and w[-2] == "tiles"
    hist, tiles = [int(x) for x in w[1:-2]], int(w[-1])
    print(hist, tiles)
    assert tiles == 240 * 135 == sum(hist)
    assert hist[0] >= 0.36 * tiles
    assert sum(k * n for k, n in enumerate(hist)) <= 0.85 * tiles
