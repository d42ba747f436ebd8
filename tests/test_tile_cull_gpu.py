"""Tile culling in the plain flat world's render instances (rt_kernel.hip kCull,
rt_cull.h): a work unit of more than one batch tests at generation only the
roots its tile's camera rays can reach, and such a unit that reaches none adds
the background s_count times per pixel and runs no path loop.  Frames do not
change.  Held here, at the benchmark's camera scaled to 72x40 and 77x43 pixels
(a width that is no multiple of 8), depth 1 and 8, for the Lambertian-only and
the general instance (the latter through an unused metal material).

Which cases reach the new code: the mask is formed for units of more than one
batch only (one-batch units measured slower with it), so
the 4-strata frames in whole-tile units (whole_units) and the tile layout in 2
stratum chunks of 2 strata run kCull; the 1-stratum frames and the default
plan's one-stratum units run the parent's flow, and are kept as the check that
this flow, in the three instances whose text changed, still gives its frames.

 * against the oracle at the GPU bar (4 strata: kCull; 1 stratum: the old flow);
 * against the same world plus two unreachable spheres (tiny, behind the
   camera): 5 roots, more than the camera-origin table holds, so no mask is
   formed and every unit runs the full flow.  Pixels of the tiles the host twin
   (tests/native/rt_tile_cull_check masks) calls all-sky are bit-equal, all
   others lie within the order-of-adds bound of tests/test_batch_trace.py,
   2 (n - 1) 2^-53 relative for n non-negative terms (4 strata: kCull against
   the full flow; 1 stratum: both sides run the old flow, bit-equal);
 * against radiance along camera_rays for the one-stratum frame, bit for bit
   (the old flow);
 * a world nobody can see (all three spheres behind the camera): the whole
   frame is the sequential sum of bg, bit for bit, in frame layout (whole-tile
   units: kCull's all-sky shortcut; the default plan's one-stratum units: the
   old flow), in tile layout with 2 stratum chunks (kCull), with accumulate = 1,
   with RT_OUT_SCALED, and for a bg with a zero component;
 * edge worlds at 4 strata (kCull's branch is entered) and 1 stratum: a camera
   inside the ground sphere (nothing may be culled), a lens camera (the old
   flow) -- both against their 5-root twins within the bound -- and
   max_depth = 0, which gives zeros.
"""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from rtx import abi
from rtx.render import Renderer, camera_frame
from rtx.scene import load_scene
import oracle_lib as O
from test_batch_trace import frame_of_tiles, whole_units
from test_diffuse_instance import with_unused_metal
from test_parked_shading import BAR, SEED, sized
from test_radiance_gpu import strata_equal_the_render
from test_tile_cull import CHECK, NATIVE, SCENE

pytestmark = pytest.mark.gpu

FLAT, DIFFUSE = abi.RT_FEAT_FLAT, abi.RT_FEAT_DIFFUSE
SIZES = [(72, 40), (77, 43)]
INST = ["diffuse", "any"]
U = 2.0 ** -53


def world(extra=False, **cam):
    """three_spheres (the benchmark's world and camera); extra: plus two spheres
    no camera ray of the default camera can reach, which takes it to 5 roots."""
    with open(SCENE) as f:
        d = json.load(f)
    if extra:
        d["world"] += [{"type": "sphere", "center": [0.0, 0.0, 5.0], "radius": 0.01, "material": "left"},
                       {"type": "sphere", "center": [0.5, 0.3, 6.0], "radius": 0.01, "material": "center"}]
    d["camera"].update(cam)
    return d


def unseen(**cam):
    """The world with its three spheres made small and put behind the camera: nobody sees them."""
    d = world(**cam)
    for s, (c, r) in zip(d["world"], (([0.0, 0.0, 3.0], 0.5), ([1.0, 0.0, 4.0], 0.5), ([-1.0, 0.5, 5.0], 1.0))):
        s["center"], s["radius"] = c, r
    return d


def scene(doc, inst):
    S = load_scene(doc)
    return with_unused_metal(S) if inst == "any" else S


def want(inst):
    return FLAT | DIFFUSE if inst == "diffuse" else FLAT


def masks(doc, f):
    """The host twin's mask of every tile of frame f, [tiles_y, tiles_x]."""
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "tile_cull.mk"], check=True)
    args = [CHECK, "masks", str(f.image_width), str(f.image_height)]
    for v in (f.center, f.pixel00_loc, f.pixel_delta_u, f.pixel_delta_v):
        args += [float(x).hex() for x in v.tolist()]
    args.append(str(len(doc["world"])))
    for s in doc["world"]:
        args += [float(x).hex() for x in s["center"]] + [float(s["radius"]).hex()]
    r = subprocess.run(args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    w = r.stdout.split()
    assert w[0] == "MASKS"
    ty, tx = (f.image_height + 7) // 8, (f.image_width + 7) // 8
    return np.array([int(x) for x in w[1:]]).reshape(ty, tx)


def sky_pixels(doc, f):
    m = masks(doc, f) == 0
    return np.kron(m, np.ones((8, 8), bool))[:f.image_height, :f.image_width]


@functools.lru_cache(maxsize=None)
def frames(size, spp, depth, inst, cam=()):
    """RT_OUT_SUM frames of the world and of its 5-root twin, whole-tile units."""
    out = []
    for extra in (False, True):
        S = scene(world(extra, **dict(cam)), inst)
        _, f = sized(S, *size, spp, depth)
        with whole_units(S) as R:
            assert R.info()["features"] == want(inst)
            a = R.render(f, seed=SEED, output=abi.RT_OUT_SUM)
        a.setflags(write=False)
        out.append(a)
    return out


def within_add_order(a, b, n):
    return (np.abs(a - b) <= 2 * (n - 1) * U * np.maximum(a, b)).all()


@functools.lru_cache(maxsize=None)
def reference(size, spp, depth):
    S = load_scene(world())
    cam, _ = sized(S, *size, spp, depth)
    ref = O.oracle_render(S, cam, O.MODE_COUNTER, SEED, output=abi.RT_OUT_SUM)
    ref.setflags(write=False)
    return ref


CASES = [(s, spp, depth) for s in SIZES for spp in (1, 4) for depth in (1, 8)]


@pytest.mark.parametrize("inst", INST)
@pytest.mark.parametrize("size,spp,depth", CASES)
def test_frames_match_the_oracle(size, spp, depth, inst):
    got = frames(size, spp, depth, inst)[0]
    d = np.abs(got - reference(size, spp, depth)).max() / spp
    print("%s %s, %d strata, depth %d: max |gpu - oracle| = %g" % (inst, size, spp, depth, d))
    assert np.isfinite(got).all() and got.max() > 0
    assert d <= BAR


@pytest.mark.parametrize("inst", INST)
@pytest.mark.parametrize("size,spp,depth", CASES)
def test_frames_equal_the_five_root_twin(size, spp, depth, inst):
    got, twin = frames(size, spp, depth, inst)
    doc = world()
    _, f = sized(load_scene(doc), *size, spp, depth)
    sky = sky_pixels(doc, f)
    # teeth: at this camera 10 of 45 and 13 of 60 tiles are all-sky (fewer than the 38 % of 1920x1080's finer tiles)
    assert 0.15 * sky.size < sky.sum() < 0.6 * sky.size
    assert np.array_equal(got[sky], twin[sky])
    bg = np.asarray(doc["camera"]["background"])
    assert np.array_equal(got[sky], np.broadcast_to(sum_of(bg, spp), got[sky].shape))
    assert within_add_order(got, twin, spp)
    if spp == 1:
        assert np.array_equal(got, twin)


@pytest.mark.parametrize("inst", INST)
@pytest.mark.parametrize("size", SIZES)
def test_one_stratum_frames_have_radiances_bits(size, inst):
    S = scene(world(), inst)
    _, f = sized(S, *size, 1)
    with Renderer(S) as R:
        assert R.info()["features"] == want(inst)
        strata_equal_the_render(R, f, SEED)


# ---------------------------------------------------------------- a world nobody can see
def sum_of(bg, n):
    """bg added n times to 0, in sequence."""
    s = np.zeros(3)
    for _ in range(n):
        s = s + bg
    return s


@pytest.mark.parametrize("inst", INST)
@pytest.mark.parametrize("bg", [(0.7, 0.8, 1.0), (0.1, 0.0, 0.3)], ids=["sky", "zero_component"])
def test_an_unseen_world_is_the_sum_of_the_background(bg, inst):
    import torch
    w, h, spp = 77, 43, 4
    doc = unseen(background=list(bg))
    S = scene(doc, inst)
    _, f = sized(S, w, h, spp)
    assert not masks(doc, f).any()
    bg = np.asarray(bg)
    full = np.broadcast_to(sum_of(bg, spp), (h, w, 3))
    kw = dict(seed=SEED, output=abi.RT_OUT_SUM)
    for make in (whole_units, Renderer):  # units of 4 batches; the default plan's one-stratum units
        with make(S) as R:
            assert R.info()["features"] == want(inst)
            assert np.array_equal(R.render(f, **kw), full)
            # tile layout, 2 stratum chunks of 2 strata: slots outside the image stay 0
            tiles = R.render(f, layout=abi.RT_LAYOUT_TILES, chunks=2, **kw)
            assert tiles.shape == (10 * 6, 2, 64, 3)
            for c in range(2):
                assert np.array_equal(frame_of_tiles(tiles[:, c], w, h), np.broadcast_to(sum_of(bg, 2), (h, w, 3)))
                assert (tiles[:, c] != 0).any(axis=2).sum() == h * w
            # accumulate = 1
            acc = torch.full((h, w, 3), 0.375, dtype=torch.float64, device="cuda")
            R.render_device(f, acc.data_ptr(), 0, seed=SEED, output=abi.RT_OUT_SUM, accumulate=1)
            torch.cuda.synchronize()
            assert np.array_equal(acc.cpu().numpy(), 0.375 + full)
            # RT_OUT_SCALED: the epilogue's scale * sum
            assert np.array_equal(R.render(f, seed=SEED), f.pixel_samples_scale * full)


# ---------------------------------------------------------------- edge worlds
@pytest.mark.parametrize("inst", INST)
@pytest.mark.parametrize("spp", [1, 4])
def test_a_camera_inside_the_ground_sphere_culls_nothing(spp, inst):
    cam = (("lookfrom", (0.0, -20.0, 0.0)), ("lookat", (0.0, -20.0, -1.0)))
    doc = world(**{k: list(v) for k, v in cam})
    _, f = sized(load_scene(doc), 77, 43, spp)
    assert (masks(doc, f) & 1).all()  # the ground, root 0, in every tile's mask
    got, twin = frames((77, 43), spp, 8, inst, cam)
    assert np.isfinite(got).all()
    assert within_add_order(got, twin, spp)


@pytest.mark.parametrize("inst", INST)
@pytest.mark.parametrize("spp", [1, 4])
def test_a_lens_camera_keeps_the_old_flow(spp, inst):
    got, twin = frames((77, 43), spp, 8, inst, (("defocus_angle", 4.0), ("focus_dist", 1.0)))
    assert np.isfinite(got).all() and got.max() > 0
    assert within_add_order(got, twin, spp)


@pytest.mark.parametrize("inst", INST)
@pytest.mark.parametrize("hidden", [False, True])
def test_depth_zero_gives_zeros(hidden, inst):
    S = scene(unseen() if hidden else world(), inst)
    for spp in (1, 4):
        _, f = sized(S, 77, 43, spp, 0)
        for make in (whole_units, Renderer):
            with make(S) as R:
                got = R.render(f, seed=SEED, output=abi.RT_OUT_SUM)
            assert got.shape == (43, 77, 3) and not got.any()
