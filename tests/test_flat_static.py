"""Flat worlds: the static and the moving form of the sphere walk.

A flat world (F_FLAT: at most 8 world items, no BVH walk) without a moving
sphere runs the static instantiations of trace's item loop and trace_tail's
item record (rt_path.h, sphere_center<false>): the center is c0, no
center.at(time) arithmetic.  One sphere with a `center2` switches the whole
world to the moving instantiations.  Both are separate machine code inside
each flat kernel instance, so each gets its own scenes here:

 * against the oracle's counter mode at tests/test_gpu_instances.py's bar
   (|diff| <= 1e-4 per channel, same NaN mask);
 * against each other: a moving sphere that no ray can reach (inside the
   ground sphere, listed last) switches the form without touching a pixel, so
   the two frames must be equal bit for bit (c0 + tm * 0 == c0).  The pair
   is bit-neutral by construction: the host emulator of the commit before the
   split, which selected the centre at run time, gives equal frames for it too.

The same pairs run through the kernel source compiled for the host
(tests/native emulator) without a GPU.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from rtx import abi
from rtx.render import Renderer, camera_frame
from rtx.scene import load_scene
import oracle_lib as O
from test_gpu_instances import feature_scene, FLAT, LIGHTS, SCENES

NATIVE = os.path.join(os.path.dirname(__file__), "native")
SEED = 31


def three_spheres(moving_visible=False, hidden_mover=False):
    with open(os.path.join(SCENES, "three_spheres.json")) as f:
        d = json.load(f)
    if moving_visible:  # the centre sphere drifts upwards during the exposure
        d["world"][1]["center2"] = [0, 0.25, -1.2]
    if hidden_mover:
        # at the ground sphere's centre, radius 1 inside radius 100: every ray
        # towards it hits the ground first, and the ground is tested first
        g = d["world"][0]
        d["world"].append({"type": "sphere", "center": list(g["center"]),
                           "center2": [g["center"][0] + 0.5, g["center"][1], g["center"][2]],
                           "radius": 1, "material": "left"})
    return d


def rich_flat(moving):
    d = feature_scene(FLAT | LIGHTS)
    sph = [o for o in d["world"] if o["type"] == "sphere"]
    assert len(sph) == 1
    if moving:
        c = sph[0]["center"]
        sph[0]["center2"] = [c[0] + 25, c[1] + 10, c[2]]
    return d


def is_static(d):
    return not any("center2" in o for o in d["world"])


def frame_of(S, width=64, spp=4):
    cam = S.camera_desc(image_width=width, samples_per_pixel=spp, max_depth=8)
    return cam, camera_frame(cam)


def gpu_frame(d, **kw):
    S = load_scene(d)
    cam, f = frame_of(S, **kw)
    with Renderer(S) as R:
        assert R.info()["features"] & FLAT
        return S, cam, R.render(f, seed=SEED)


def check_oracle(got, S, cam, atol):
    ref = O.oracle_render(S, cam, O.MODE_COUNTER, SEED)
    d = np.abs(np.nan_to_num(got) - np.nan_to_num(ref))
    print("max |diff| vs oracle: %g" % d.max())
    assert not (d > atol).any(), "%d channels off, max %g" % ((d > atol).sum(), d.max())
    assert np.array_equal(np.isnan(got), np.isnan(ref))


@pytest.mark.gpu
@pytest.mark.parametrize("moving", [False, True], ids=["static", "moving"])
def test_three_spheres_matches_oracle(moving):
    d = three_spheres(moving_visible=moving)
    assert is_static(d) == (not moving)
    S, cam, got = gpu_frame(d)  # 64 x 36
    check_oracle(got, S, cam, 1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("moving", [False, True], ids=["static", "moving"])
def test_rich_flat_scene_matches_oracle(moving):
    d = rich_flat(moving)
    assert is_static(d) == (not moving)
    S, cam, got = gpu_frame(d, width=40, spp=9)
    check_oracle(got, S, cam, 1e-4)


@pytest.mark.gpu
def test_static_form_gives_the_moving_form_its_bits():
    _, _, a = gpu_frame(three_spheres())
    _, _, b = gpu_frame(three_spheres(hidden_mover=True))
    assert np.isfinite(a).all()
    assert np.array_equal(a, b)


# ---- the same split in the kernel source compiled for the host (no GPU)
@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-C", NATIVE], check=True)
    L = C.CDLL(os.environ.get("RTX_EMU_LIB", os.path.join(NATIVE, "build", "libemu.so")))
    L.emu_render.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.Frame),
                             C.POINTER(abi.RenderParams), C.c_int, C.POINTER(C.c_double)]
    return L


def emu_frame(L, d, width=32, spp=4):
    S = load_scene(d)
    desc = S.desc()
    cam, f = frame_of(S, width, spp)
    p = abi.RenderParams()
    p.seed, p.sample_count, p.output = SEED, -1, abi.RT_OUT_SCALED
    out = np.zeros((f.image_height, f.image_width, 3))
    # feature bits 0: the emulator adds F_FLAT for a one-leaf world itself
    assert L.emu_render(C.byref(desc), C.byref(f), C.byref(p), 0,
                        out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return S, cam, out


def test_emulator_moving_flat_world_matches_oracle(emu):
    S, cam, out = emu_frame(emu, three_spheres(moving_visible=True))
    check_oracle(out, S, cam, 1e-10)  # tests/test_emulator.py's host bound


def test_emulator_static_form_gives_the_moving_form_its_bits(emu):
    _, _, a = emu_frame(emu, three_spheres())
    _, _, b = emu_frame(emu, three_spheres(hidden_mover=True))
    assert np.isfinite(a).all()
    assert np.array_equal(a, b)
