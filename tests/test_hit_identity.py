"""Closest-hit identity frames: every ray of every path must find the item and
the face the brute-force closest hit finds.

Every world item carries its own diffuse_light whose emission is a small
integer code of the item index, (k & 63, (k >> 6) & 63, (k >> 12) + 1); the
background is 0, the light list empty, the output RT_OUT_SUM.  In the mirror
scenes every other item is a perfect mirror (metal, albedo 1, fuzz 0) and
max_depth is 4.  A pixel is then a sum of small integers -- exact in any
order -- so a frame equals the oracle's brute-force frame (use_bvh = 0: a loop
over all items, no boxes) BIT FOR BIT exactly when no walk drops, reorders away
or mis-ranges a hit: plane offsets, LDS staging, stacks, leaf ranges, tie rules,
static_spheres.  (Margin errors of the box tests are tests/slab_cases.py's
job: the node boxes' own padding hides them here.)  The scenes have no
coincident surfaces; the cap on differing pixels is zero.

CPU: the kernel source on the host (tests/native emulator) -- binary walk,
4-wide walk, flat worlds.  GPU: the same frames through the C ABI for every
walk the library can take (default staging, no and partial LDS node prefix,
the persistent instance with and without staged primitives, 4-wide, the
leafshare variant library, flat static / moving worlds, device-built trees).
"""
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from rtx import abi
from rtx.render import Renderer, camera_frame
from rtx.scene import load_scene
import oracle_lib as O

NATIVE = os.path.join(os.path.dirname(__file__), "native")
THREADS = max(1, min(16, os.cpu_count() or 1))
W, SPP, DEPTH = 256, 4, 4


def _material(k, mirrors):
    if mirrors and k % 2 == 1:
        return {"type": "metal", "albedo": [1.0, 1.0, 1.0], "fuzz": 0.0}
    return {"type": "diffuse_light", "emit": [float(k & 63), float((k >> 6) & 63), float((k >> 12) + 1)]}


def _world(rng, n_spheres, n_quads, center, half, r_lo, r_hi, mirrors):
    """n_spheres random spheres (a third of them moving) and n_quads random
    quads within +-half of center, and a 1000-radius ground sphere below."""
    c0 = np.asarray(center, dtype=np.float64)
    c = c0 + rng.uniform(-half, half, (n_spheres, 3))
    r = rng.uniform(r_lo, r_hi, n_spheres)
    move = rng.uniform(-1, 1, (n_spheres, 3)) * r_hi
    world = []
    for i in range(n_spheres):
        s = {"type": "sphere", "center": [float(x) for x in c[i]], "radius": float(r[i]),
             "material": _material(len(world), mirrors)}
        if i % 3 == 0:
            s["center2"] = [float(x) for x in c[i] + move[i]]
        world.append(s)
    for _ in range(n_quads):
        world.append({"type": "quad", "Q": [float(x) for x in c0 + rng.uniform(-half, half, 3)],
                      "u": [float(x) for x in rng.uniform(-0.2, 0.2, 3) * half],
                      "v": [float(x) for x in rng.uniform(-0.2, 0.2, 3) * half],
                      "material": _material(len(world), mirrors)})
    world.append({"type": "sphere", "center": [float(c0[0]), float(c0[1] - 1000.0 - 1.25 * half), float(c0[2])],
                  "radius": 1000.0, "material": _material(len(world), mirrors)})
    return world


def _doc(world, use_bvh=True):
    return {"world": world, "lights": [], "use_bvh": use_bvh,
            "camera": {"aspect_ratio": 1.0, "image_width": W, "samples_per_pixel": SPP, "max_depth": DEPTH,
                       "defocus_angle": 0, "focus_dist": 10, "background": [0, 0, 0], "vup": [0, 1, 0]}}


def _frames_cloud(center, half):
    """vfov that frames +-1.8 half around center from `dist` away."""
    c = np.asarray(center, dtype=np.float64)
    u = np.array([0.6, 0.5, 0.62]) / np.linalg.norm([0.6, 0.5, 0.62])

    def view(dist):
        return {"lookfrom": [float(x) for x in c + dist * u], "lookat": [float(x) for x in c],
                "vfov": 2 * math.degrees(math.atan(1.8 * half / dist))}
    return view


CLOUD_A, CLOUD_B = (1000.0, 700.0, -1300.0), (30000.0, -20000.0, 10000.0)
_general_far = _frames_cloud((0, 0, 0), 10.0)
_cloud_a, _cloud_b = _frames_cloud(CLOUD_A, 0.5), _frames_cloud(CLOUD_B, 0.5)

VIEWS = {
    "outside": {"lookfrom": [3, 8, 40], "lookat": [0, 0, 0], "vfov": 40},
    "inside": {"lookfrom": [0.3, 0.2, 0.1], "lookat": [5, 1, -3], "vfov": 90},
    "far": _general_far(1e5),
    "axis": {"lookfrom": [0, 0, 40], "lookat": [0, 0, 0], "vfov": 40},   # straight down -z
}
# name -> (scene key, camera overrides)
CASES = {}
for _v, _cam in VIEWS.items():
    CASES["lights-" + _v] = ("lights", _cam)
    CASES["mirrors-" + _v] = ("mirrors", _cam)
CASES["cloudA-far"] = ("cloudA", _cloud_a(1000.0))
CASES["cloudA-near"] = ("cloudA", _cloud_a(10.0))
CASES["cloudB-far"] = ("cloudB", _cloud_b(1000.0))
CASES["cloudB-near"] = ("cloudB", _cloud_b(10.0))
# small enough for the persistent instance to stage items and spheres after the whole tree
CASES["small-outside"] = ("small", {"lookfrom": [2, 4, 20], "lookat": [0, 0, 0], "vfov": 40})
CASES["small-inside"] = ("small", VIEWS["inside"])
FLAT = ("flat-static", "flat-moving")


@functools.lru_cache(maxsize=None)
def scene_doc(key):
    rng = np.random.default_rng({"lights": 1, "mirrors": 2, "cloudA": 3, "cloudB": 4, "flat-static": 5,
                                 "flat-moving": 6, "big": 7, "small": 8}[key])
    if key == "lights":       # 1000 items, all lights
        return _doc(_world(rng, 979, 20, (0, 0, 0), 10.0, 0.1, 0.6, False))
    if key == "mirrors":      # 601 items, every other one a mirror (the ground is a light)
        return _doc(_world(rng, 580, 20, (0, 0, 0), 10.0, 0.1, 0.6, True))
    if key == "small":        # 301 items
        return _doc(_world(rng, 280, 20, (0, 0, 0), 5.0, 0.1, 0.6, True))
    if key in ("cloudA", "cloudB"):  # tiny spheres far from the origin: fp32 box coordinates are coarse there
        return _doc(_world(rng, 800, 20, CLOUD_A if key == "cloudA" else CLOUD_B, 0.5, 0.004, 0.03, True))
    if key in FLAT:           # at most RT_FLAT_MAX = 8 items: one leaf, no walk
        w = _world(rng, 5, 2, (0, 0, 0), 3.0, 0.5, 1.5, True)
        if key == "flat-static":
            for it in w:
                it.pop("center2", None)
        return _doc(w)
    if key == "big":          # device-built trees
        return _doc(_world(rng, BIG_N, 20, (0, 0, 0), 30.0, 0.05, 0.4, True))
    raise KeyError(key)


BIG_N, BIG_W = 20000, 128


def case_scene(name):
    """(SceneDescription, camera desc) of a case."""
    if name in FLAT:
        key, cam = name, {"lookfrom": [2, 3, 12], "lookat": [0, 0, 0], "vfov": 35}
    elif name == "big":
        key, cam = "big", {"lookfrom": [10, 25, 110], "lookat": [0, 0, 0], "vfov": 40, "image_width": BIG_W}
    else:
        key, cam = CASES[name]
    S = load_scene(scene_doc(key))
    return S, S.camera_desc(**cam)


@functools.lru_cache(maxsize=None)
def brute_force(name, seed=11):
    """The oracle's frame with no BVH at all: every ray against every item.
    Computed once per case and shared; read-only."""
    S, cam = case_scene(name)
    ref = O.oracle_render(S, cam, O.MODE_COUNTER, seed, use_bvh=0, output=abi.RT_OUT_SUM, threads=THREADS)
    assert ref.any() and np.array_equal(ref, np.round(ref))  # integer codes, some item seen
    ref.setflags(write=False)
    return ref


def assert_identical(out, name, what):
    ref = brute_force(name)
    bad = np.argwhere((out != ref).any(axis=2))
    assert len(bad) == 0, "%s, %s: %d pixels differ from the brute-force frame, first (row, col) %s: %s vs %s" % (
        name, what, len(bad), tuple(bad[0]), out[tuple(bad[0])], ref[tuple(bad[0])])
    assert np.array_equal(out, ref)


# ---------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-C", NATIVE, "build/libemu.so"], check=True)
    L = C.CDLL(os.environ.get("RTX_EMU_LIB", os.path.join(NATIVE, "build", "libemu.so")))
    L.emu_render.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.Frame),
                             C.POINTER(abi.RenderParams), C.c_int, C.POINTER(C.c_double)]
    return L


def emu_frame(emu, name, features, seed=11):
    S, cam = case_scene(name)
    d = S.desc()
    f = camera_frame(cam)
    p = abi.RenderParams()
    p.seed, p.sample_count, p.output = seed, -1, abi.RT_OUT_SUM
    out = np.zeros((f.image_height, f.image_width, 3))
    assert emu.emu_render(C.byref(d), C.byref(f), C.byref(p), features,
                          out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return out


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("walk", ["binary", "bvh4"])
def test_kernel_source_finds_the_brute_force_hits(emu, name, walk):
    """Binary walk (slab2_planes over the staged DNodeL tree) and 4-wide walk
    (slab_planes<4>) of the kernel source on the host."""
    out = emu_frame(emu, name, abi.RT_FEAT_BVH4 if walk == "bvh4" else 0)
    assert_identical(out, name, "host " + walk)


@pytest.mark.parametrize("name", FLAT)
def test_kernel_source_flat_world_finds_the_brute_force_hits(emu, name):
    out = emu_frame(emu, name, 0)
    assert_identical(out, name, "host flat")


# ---------------------------------------------------------------- GPU
# walk variants of the product library: scene fields, rt_tuning fields, and
# what rt_scene_info must then report
VARIANTS = {
    "default": ({}, {}, {}),
    "no-lds-nodes": ({"bvh_arity": 2}, {"lds_nodes": -1, "no_persistent": 1}, {"lds_nodes": 0}),
    "lds-prefix": ({"bvh_arity": 2}, {"lds_nodes": 40, "no_persistent": 1}, {"lds_nodes": 40}),
    "binary-one-unit": ({"bvh_arity": 2}, {"no_persistent": 1}, {"bvh_arity": 2}),
    "persistent": ({"bvh_arity": 2}, {"grid_cap": 3}, {"bvh_arity": 2}),
    "persistent-no-prims": ({"bvh_arity": 2}, {"grid_cap": 3, "no_lds_prims": 1}, {"lds_prims_persistent": 0}),
    "persistent-prefix": ({"bvh_arity": 2}, {"grid_cap": 3, "lds_nodes_pc": 40}, {"lds_nodes_persistent": 40}),
    "bvh4": ({"bvh_arity": 4}, {}, {"bvh_arity": 4}),
    "bvh4-persistent": ({"bvh_arity": 4}, {"grid_cap": 3}, {"bvh_arity": 4}),
}


def gpu_frame(name, fields=None, tuning=None, want=None, seed=11):
    S, cam = case_scene(name)
    for k, v in (fields or {}).items():
        setattr(S, k, v)
    f = camera_frame(cam)
    with Renderer(S, tuning=tuning or None) as R:
        info = R.info()
        out = R.render(f, seed=seed, output=abi.RT_OUT_SUM)
    for k, v in (want or {}).items():
        assert info[k] == v, (k, info)
    return out, info


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_gpu_walks_find_the_brute_force_hits(name, variant):
    fields, tuning, want = VARIANTS[variant]
    out, info = gpu_frame(name, fields, tuning, want)
    assert info["features"] & abi.RT_FEAT_FLAT == 0
    if name.startswith("small") and variant == "persistent":  # whole tree, items and spheres staged
        assert info["lds_nodes_persistent"] == info["n_nodes"] and info["lds_prims_persistent"] == 1, info
    print(name, variant, {k: info[k] for k in ("n_nodes", "bvh_arity", "lds_nodes", "lds_nodes_persistent",
                                                "lds_prims_persistent", "persistent_block_waves")})
    assert_identical(out, name, "gfx950 " + variant)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FLAT)
def test_gpu_flat_worlds_find_the_brute_force_hits(name):
    """Flat worlds (one leaf, no walk): the static-sphere hit test and the
    moving one (DScene::static_spheres)."""
    out, info = gpu_frame(name)
    assert info["features"] & abi.RT_FEAT_FLAT
    assert_identical(out, name, "gfx950 flat")


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["RT_BVH_DEVICE_SAH", "RT_BVH_DEVICE"])
@pytest.mark.parametrize("arity", [2, 4])
def test_gpu_device_built_trees_find_the_brute_force_hits(builder, arity):
    b = getattr(abi, builder)
    out, info = gpu_frame("big", {"bvh_builder": b, "bvh_arity": arity}, None, {"bvh_builder": b, "bvh_arity": arity})
    assert_identical(out, "big", "gfx950 %s arity %d" % (builder, arity))


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["RT_BVH_DEVICE_SAH", "RT_BVH_DEVICE"])
def test_gpu_device_built_small_tree_finds_the_brute_force_hits(builder):
    """301 items, most of them visible (in "big" most never cover a pixel
    centre): a device-built tree that drops or mis-ranges one shows."""
    b = getattr(abi, builder)
    out, info = gpu_frame("small-outside", {"bvh_builder": b, "bvh_arity": 2}, None, {"bvh_builder": b, "bvh_arity": 2})
    assert info["features"] & abi.RT_FEAT_FLAT == 0
    assert_identical(out, "small-outside", "gfx950 %s" % builder)


@pytest.mark.gpu
def test_gpu_leafshare_variant_finds_the_brute_force_hits():
    """The compacted-leaf-test variant library (tests/test_leaf_share.py), in a
    process of its own: every case through the binary and the 4-wide walk."""
    from test_leaf_share import VARIANT
    env = dict(os.environ, RTX_LIB=VARIANT)
    p = subprocess.run([sys.executable, os.path.join(O.ROOT, "tools", "hit_identity_check.py")],
                       env=env, capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "librtx_hip_leafshare.so" in p.stdout
