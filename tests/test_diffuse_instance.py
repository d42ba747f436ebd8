"""The Lambertian-only render instance of the plain flat world.

A scene whose materials table holds nothing but Lambertian materials with
solid-colour textures carries RT_FEAT_DIFFUSE in DScene::features (rt_scene.h
diffuse_only), and a world of RT_FEAT_FLAT alone then runs
render_tiles<false, F_FLAT, 0, false, M_DIFFUSE>: shade compiled as its
Lambertian code only (rt_path.h MatSet).  The property is one of the TABLE: a
material nothing references turns it off.  That gives every diffuse world a twin
that no pixel can tell apart from it but which runs the general instance -- the
same scene with one unused metal material appended.  Checked here:

 * the compiler's bit, host only: set for three_spheres and for an all-
   Lambertian world with quads; clear with an unused metal material, with a
   checker-textured Lambertian, and for cornell (a diffuse light);
 * on the GPU, bit for bit (RT_OUT_SUM frames): worlds of 1, 3 and 7 spheres
   against their twins, at 64x40 and 60x36 (whole and partial 8x8 tiles), two
   seeds, through the frame launch, the tile layout in 2 stratum chunks, and
   accumulate = 1;
 * which kernel runs: rtk_instance_attrs, which picks through the launcher's own
   selector, reports another kernel for FLAT | DIFFUSE than for FLAT (fewer
   registers), and the same one with and without the bit for every other key;
 * against the oracle's counter mode at tests/test_flat_table.py's bar (1e-4
   per channel, equal NaN masks);
 * the general paths: the STATS instance (which has no diffuse form) counts
   the same events for a diffuse world and its twin, and a checker-textured
   Lambertian world runs the general instance and equals its oracle render.
"""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from rtx import abi
from rtx.render import Renderer, camera_frame
from rtx.scene import load_scene
from test_flat_static import NATIVE, SCENES, SEED, check_oracle
from test_flat_table import spheres

FLAT, DIFFUSE = abi.RT_FEAT_FLAT, abi.RT_FEAT_DIFFUSE
SIZES = {"64x40": (64, 40), "60x36": (60, 36)}
SEEDS = (SEED, 1234567)


def with_unused_metal(S):
    S.add_material(abi.RT_MAT_METAL, albedo=(0.8, 0.6, 0.2), fuzz=0.25)
    return S


def with_unused_checker(S):
    even = S.add_texture(abi.RT_TEX_SOLID, color=(0.2, 0.3, 0.1))
    odd = S.add_texture(abi.RT_TEX_SOLID, color=(0.9, 0.9, 0.9))
    t = S.add_texture(abi.RT_TEX_CHECKER, scale=0.32, even=even, odd=odd)
    S.add_material(abi.RT_MAT_LAMBERTIAN, texture=t)
    return S


def checker_world():
    """three_spheres with a checker-textured ground."""
    with open(os.path.join(SCENES, "three_spheres.json")) as f:
        d = json.load(f)
    d["textures"] = {"check": {"type": "checker", "scale": 0.32, "even": [0.2, 0.3, 0.1], "odd": [0.9, 0.9, 0.9]}}
    d["materials"]["ground"] = {"type": "lambertian", "texture": "check"}
    return d


def quad_world():
    """Two Lambertian spheres and two Lambertian quads: flat, diffuse, no root table."""
    d = spheres(2)
    d["world"] += [{"type": "quad", "Q": [-2, -0.5, -3], "u": [4, 0, 0], "v": [0, 2, 0], "material": "left"},
                   {"type": "quad", "Q": [1.5, -0.5, -3], "u": [0, 0, 2], "v": [0, 2, 0], "material": "center"}]
    return d


# ---- the scene compiler (host only)
@pytest.fixture(scope="module")
def bits():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "diffuse.mk"], check=True)
    L = C.CDLL(os.path.join(NATIVE, "build", "libdiffuse_emu.so"))
    L.diffuse_bits.argtypes = [C.POINTER(abi.SceneDesc), C.c_void_p]
    L.diffuse_bits.restype = C.c_int

    def get(S):
        desc = S.desc()
        info = np.zeros(6, np.int32)
        assert L.diffuse_bits(C.byref(desc), info.ctypes.data) == 0
        return dict(features=int(info[0]), diffuse=int(info[1]), mats=int(info[2]), texs=int(info[3]),
                    root_is_leaf=int(info[4]), quads=int(info[5]))
    return get


def test_bit_set_for_three_spheres(bits):
    r = bits(load_scene(os.path.join(SCENES, "three_spheres.json")))
    assert r["mats"] == 3 and r["root_is_leaf"] == 1
    assert r["diffuse"] == 1 and r["features"] == FLAT | DIFFUSE


def test_bit_clear_with_an_unused_metal_material(bits):
    r = bits(with_unused_metal(load_scene(os.path.join(SCENES, "three_spheres.json"))))
    assert r["mats"] == 4  # the compiler keeps the table as given
    assert r["diffuse"] == 0 and r["features"] == FLAT


def test_bit_clear_with_a_checker_textured_lambertian(bits):
    r = bits(with_unused_checker(load_scene(os.path.join(SCENES, "three_spheres.json"))))
    assert r["mats"] == 4 and r["texs"] == 6
    assert r["diffuse"] == 0 and r["features"] == FLAT
    r = bits(load_scene(checker_world()))
    assert r["diffuse"] == 0 and r["features"] == FLAT


def test_bit_clear_for_cornell(bits):
    r = bits(load_scene(os.path.join(SCENES, "cornell.json")))
    assert r["diffuse"] == 0 and not r["features"] & DIFFUSE


def test_bit_set_for_a_lambertian_world_with_quads(bits):
    r = bits(load_scene(quad_world()))
    assert r["quads"] == 2 and r["root_is_leaf"] == 1
    assert r["diffuse"] == 1 and r["features"] == FLAT | DIFFUSE


# ---- the two instances on the GPU
def frame_of(S, size, spp=4):
    w, h = SIZES[size]
    cam = S.camera_desc(image_width=w, aspect_ratio=w / (h + 0.5), samples_per_pixel=spp, max_depth=8)
    f = camera_frame(cam)
    assert (f.image_width, f.image_height) == (w, h)
    return cam, f


def scene_pair(n):
    """(diffuse world, its twin that takes the general instance)."""
    return load_scene(spheres(n)), with_unused_metal(load_scene(spheres(n)))


@functools.lru_cache(maxsize=None)
def _frames(n, size, seed):
    """Per scene of the pair: the frame, the 2-chunk tile layout and an accumulated frame."""
    import torch
    out = []
    for S, want in zip(scene_pair(n), (FLAT | DIFFUSE, FLAT)):
        _, f = frame_of(S, size)
        with Renderer(S) as R:
            assert R.info()["features"] == want
            frame = R.render(f, seed=seed, output=abi.RT_OUT_SUM)
            tiles = R.render(f, seed=seed, output=abi.RT_OUT_SUM, layout=abi.RT_LAYOUT_TILES, chunks=2)
            acc = torch.full((f.image_height, f.image_width, 3), 0.375, dtype=torch.float64, device="cuda")
            R.render_device(f, acc.data_ptr(), 0, seed=seed, output=abi.RT_OUT_SUM, accumulate=1)
            torch.cuda.synchronize()
            out.append((frame, tiles, acc.cpu().numpy()))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("n", [1, 3, 7])
def test_diffuse_instance_gives_the_general_instance_its_bits(n, size, seed):
    (a, at, aa), (b, bt, ba) = _frames(n, size, seed)
    w, h = SIZES[size]
    assert a.shape == (h, w, 3) and at.shape == (((w + 7) // 8) * ((h + 7) // 8), 2, 64, 3)
    assert np.isfinite(a).all() and a.max() > 0
    assert np.array_equal(a, b)    # the frame launch
    assert np.array_equal(at, bt)  # RT_LAYOUT_TILES, 2 stratum chunks
    assert np.array_equal(aa, ba)  # accumulate = 1
    assert np.array_equal(aa, 0.375 + a)


@pytest.mark.gpu
def test_diffuse_instance_matches_oracle():
    S = load_scene(spheres(3))
    cam, f = frame_of(S, "64x40", spp=16)
    with Renderer(S) as R:
        assert R.info()["features"] == FLAT | DIFFUSE
        got = R.render(f, seed=SEED)
    check_oracle(got, S, cam, 1e-4)


@pytest.mark.gpu
def test_instance_attrs_report_the_lambertian_only_kernel():
    """The launcher and rtk_instance_attrs pick the kernel through one function
    (rt_kernel.hip render_instance), so what the runtime reports about the
    instance of FLAT | DIFFUSE shows which kernel such a scene runs: another
    one than FLAT's, with fewer registers (113 against 128 VGPRs in the build's
    resource remarks) and the same static LDS.  Every other key ignores the bit."""
    from rtx.lib import load

    class KernelAttrs(C.Structure):
        _fields_ = [("num_regs", C.c_int32), ("static_lds", C.c_int32)]

    L = load()
    L.rtk_instance_attrs.argtypes = [C.c_int, C.c_int, C.POINTER(KernelAttrs)]
    L.rtk_instance_attrs.restype = C.c_int

    def attrs(features):
        a = KernelAttrs()
        assert L.rtk_instance_attrs(features, 0, C.byref(a)) == 0
        return a.num_regs, a.static_lds

    general, diffuse = attrs(FLAT), attrs(FLAT | DIFFUSE)
    print("FLAT %s, FLAT | DIFFUSE %s" % (general, diffuse))
    assert 0 < diffuse[0] < general[0] and diffuse[1] == general[1]
    for key in (0, abi.RT_FEAT_BVH4, FLAT | abi.RT_FEAT_LIGHTS, FLAT | abi.RT_FEAT_NOISE):
        assert attrs(key | DIFFUSE) == attrs(key)
    with Renderer(load_scene(spheres(3))) as R:  # the scene's plan was made from that kernel's attributes
        assert R.info()["features"] == FLAT | DIFFUSE and R.info()["waves_per_simd"] == 4


@pytest.mark.gpu
def test_stats_instance_counts_the_same_for_both():
    st = []
    for S in scene_pair(3):
        _, f = frame_of(S, "60x36")
        with Renderer(S) as R:
            st.append(R.stats(f, seed=SEED))
    a, b = ({k: v for k, v in s.items() if not k.startswith("cyc_")} for s in st)
    assert a["samples"] == 60 * 36 * 4 and a["shade_events"] > 0
    assert a == b


@pytest.mark.gpu
def test_checker_world_takes_the_general_instance_and_matches_oracle():
    S = load_scene(checker_world())
    cam, f = frame_of(S, "64x40", spp=16)
    with Renderer(S) as R:
        assert R.info()["features"] == FLAT
        got = R.render(f, seed=SEED)
    check_oracle(got, S, cam, 1e-4)
