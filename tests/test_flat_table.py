"""Flat worlds: the packed root-item table (rt_layout.h DRoot, DScene::roots).

A flat world whose root items are all static, untransformed spheres gets one
48-B record per root item -- {c0, rr} for the walk, {inv_r, mat} for the hit
record -- and the plain flat instance (F_FLAT alone) walks that table instead
of items[] -> spheres[] (rt_path.h trace, trace_tail).  Every other world gets
no table (count 0) and runs the item walk.  Checked here:

 * table against no table, bit for bit: a twin world with one more, last item,
   a unit quad through the ground sphere's centre.  A ray that could reach it
   hits the ground sphere first, and the ground sphere is tested first, so the
   quad never touches a pixel; but the twin is mixed, gets no table and runs
   the static item walk.  Worlds of 1, 2, 3 and 7 spheres (7 + the quad = 8 =
   RT_FLAT_MAX, the last size that is flat): the ends of the walk's loop.
 * against the oracle's counter mode at the project's bars (1e-4 per channel
   with equal NaN masks on the GPU, 1e-10 in the host emulator), 1, 3 and 8
   spheres (8 = RT_FLAT_MAX, the table's largest).
 * the scene compiler, host only: the table's fields equal
   spheres[items[i].idx] and items[i].mat bit for bit in item order, and the
   count is 0 for a quad among the root items, a `center2`, a transform on a
   root item and a world above RT_FLAT_MAX.
"""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from rtx import abi
from rtx.scene import load_scene
from test_flat_static import NATIVE, SCENES, check_oracle, emu, emu_frame, gpu_frame  # noqa: F401

RT_FLAT_MAX = 8
# spheres beyond three_spheres.json's three, all in view, with its materials
EXTRA = [
    ([1, 0, -1], 0.5, "center"),
    ([0.5, -0.35, -0.6], 0.15, "left"),
    ([-0.5, -0.35, -0.6], 0.15, "center"),
    ([0, 1.0, -1.5], 0.4, "ground"),
    ([-2, 0.2, -2], 0.7, "left"),
    ([2, 0.4, -2.5], 0.6, "center"),
]


def spheres(n, hidden_quad=False):
    """three_spheres cut or extended to n spheres, the ground sphere first."""
    with open(os.path.join(SCENES, "three_spheres.json")) as f:
        d = json.load(f)
    w = d["world"] + [{"type": "sphere", "center": c, "radius": r, "material": m} for c, r, m in EXTRA]
    d["world"] = w[:n]
    assert len(d["world"]) == n
    if hidden_quad:
        c = d["world"][0]["center"]
        d["world"].append({"type": "quad", "Q": [c[0] - 0.5, c[1], c[2] - 0.5], "u": [1, 0, 0],
                           "v": [0, 0, 1], "material": "left"})
    return d


# ---- the scene compiler (host only)
@pytest.fixture(scope="module")
def tab():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "root_table.mk"], check=True)
    L = C.CDLL(os.path.join(NATIVE, "build", "libroot_table_emu.so"))
    L.root_table_dump.argtypes = [C.POINTER(abi.SceneDesc), C.c_int] + [C.c_void_p] * 5
    L.root_table_dump.restype = C.c_int

    def dump(d):
        S = load_scene(d)
        desc = S.desc()
        cap = 16
        t, s = np.full((cap, 5), np.nan), np.full((cap, 5), np.nan)
        tm, sm = np.full(cap, -7, np.int32), np.full(cap, -9, np.int32)
        info = np.zeros(6, np.int32)
        assert L.root_table_dump(C.byref(desc), cap, t.ctypes.data, tm.ctypes.data, s.ctypes.data,
                                 sm.ctypes.data, info.ctypes.data) == 0
        return dict(records=int(info[0]), n_roots=int(info[1]), root_is_leaf=int(info[2]),
                    n_root_items=int(info[3]), items=int(info[4]), bound=int(info[5]),
                    tab=t, tab_mat=tm, src=s, src_mat=sm)
    return dump


@pytest.mark.parametrize("n", [1, 2, 3, 7, RT_FLAT_MAX])
def test_table_copies_the_spheres_and_items_bit_for_bit(tab, n):
    r = tab(spheres(n))
    assert r["root_is_leaf"] == 1 and r["n_root_items"] == n == r["items"]
    assert r["records"] == n and r["n_roots"] == n and r["bound"] == 1
    # bits, not values: the doubles are copies (-0.0 and NaN payloads included)
    assert np.array_equal(r["tab"][:n].view(np.uint64), r["src"][:n].view(np.uint64))
    assert np.array_equal(r["tab_mat"][:n], r["src_mat"][:n])
    # item order: the ground sphere (r = 100: rr = 1e4) first, then the scene's order
    d = spheres(n)
    for i, o in enumerate(d["world"]):
        assert list(r["tab"][i, :3]) == [float(x) for x in o["center"]]
        assert r["tab"][i, 3] == float(o["radius"]) * float(o["radius"])
        assert r["tab"][i, 4] == 1.0 / float(o["radius"])


def test_no_table_with_a_quad_among_the_root_items(tab):
    r = tab(spheres(3, hidden_quad=True))
    assert r["root_is_leaf"] == 1 and r["n_root_items"] == 4
    assert r["records"] == 0 and r["n_roots"] == 0


def test_no_table_with_a_moving_sphere(tab):
    d = spheres(3)
    d["world"][1]["center2"] = [0, 0.25, -1.2]
    r = tab(d)
    assert r["root_is_leaf"] == 1 and r["n_root_items"] == 3
    assert r["records"] == 0 and r["n_roots"] == 0


def test_no_table_with_a_transform_on_a_root_item(tab):
    d = spheres(3)
    d["world"][2] = {"type": "translate", "offset": [0.25, 0, 0], "object": d["world"][2]}
    r = tab(d)
    assert r["root_is_leaf"] == 1 and r["n_root_items"] == 3
    assert r["records"] == 0 and r["n_roots"] == 0


def test_no_table_above_flat_max(tab):
    r = tab(spheres(RT_FLAT_MAX + 1))
    assert r["root_is_leaf"] == 0 and r["items"] == RT_FLAT_MAX + 1
    assert r["records"] == 0 and r["n_roots"] == 0


# ---- the kernel source compiled for the host (no GPU): 32 x 18
@functools.lru_cache(maxsize=None)
def _emu_cached(L, n, quad):
    return emu_frame(L, spheres(n, hidden_quad=quad), width=32, spp=9)


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_emulator_table_gives_the_item_walk_its_bits(emu, n):  # noqa: F811
    _, _, a = _emu_cached(emu, n, False)
    _, _, b = _emu_cached(emu, n, True)
    assert a.shape == (18, 32, 3)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert np.array_equal(a, b)


@pytest.mark.parametrize("n", [1, 3, RT_FLAT_MAX])
def test_emulator_table_matches_oracle(emu, n):  # noqa: F811
    S, cam, out = _emu_cached(emu, n, False)
    check_oracle(out, S, cam, 1e-10)  # tests/test_emulator.py's host bound


# ---- the plain flat instance on the GPU: 64 x 36
@functools.lru_cache(maxsize=None)
def _gpu_cached(n, quad):
    return gpu_frame(spheres(n, hidden_quad=quad), width=64, spp=16)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_table_gives_the_item_walk_its_bits(n):
    _, _, a = _gpu_cached(n, False)
    _, _, b = _gpu_cached(n, True)
    assert a.shape == (36, 64, 3)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, RT_FLAT_MAX])
def test_table_matches_oracle(n):
    S, cam, got = _gpu_cached(n, False)
    check_oracle(got, S, cam, 1e-4)
