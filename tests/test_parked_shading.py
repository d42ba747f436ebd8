"""Parked shading in the plain flat world (rt_kernel.hip RT_PARK_MIN).

Every render_tiles instance of F == F_FLAT traces first and shades later: a
lane whose ray hit keeps (closest, best) -- it is parked -- and the wave shades
only once RT_PARK_K lanes are parked or no refill can add to them.  A parked
lane may sit through several refills.  Every sample keeps its value; what moves
is the order in which a pixel's samples reach its fp64 sum.  Checked here, on
small flat worlds (no BVH, at most 8 items):

 1. exact accounting: worlds of integer diffuse lights (and perfect mirrors)
    over an integer background -- every sample an integer triple, every sum
    exact in any order -- equal the oracle's COUNTER frame bit for bit: a lane
    shaded twice, never, or with another trace's (closest, best) is a wrong
    integer.  One world's sphere covers 2-3 pixels of one tile (its lanes stay
    parked until the tile's items run out), one's covers the image (nothing
    ever waits), one bounces between mirrors;
 2. Lambertian parity: C2's three spheres at 24x16, 1 / 4 / 16 strata, against
    the oracle at the project's GPU bar (1e-4 per
    channel); at 1 stratum (64 items per unit: no refill, nothing parked) the
    frame equals, bit for bit, that of the twin with a hidden quad, which has
    no root table and takes the item walk -- the split of trace / record
    preserves values;
 3. the end of the queue: 8x8 pixels, 2 and 3 strata, depth 1 and 8, rendered
    in a child process under a time limit (a loop that does not end is killed
    and reported): finite, the oracle's frame within the same bar, and the
    STATS launch's samples, segments and shade events those of the twin;
 4. determinism: a launch repeated, a tile subset against the same tiles of
    the whole launch, and a tile-list launch repeated, bit for bit.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # the child of test 3
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_root, "real-time-ray-tracing-engine_amd"), os.path.join(_root, "tests")]

from rtx import abi
from rtx.render import Renderer, camera_frame
from rtx.scene import load_scene
import oracle_lib as O
from test_flat_table import spheres

FLAT, DIFFUSE = abi.RT_FEAT_FLAT, abi.RT_FEAT_DIFFUSE
SEED = 31
BAR = 1e-4


def sized(S, w, h, spp, depth=8, **cam):
    c = S.camera_desc(image_width=w, aspect_ratio=w / (h + 0.5), samples_per_pixel=spp, max_depth=depth, **cam)
    f = camera_frame(c)
    assert (f.image_width, f.image_height) == (w, h)
    return c, f


# ---------------------------------------------------------------- 1. exact accounting
W1, H1, SPP1 = 20, 12, 16
BG = [3.0, 1.0, 2.0]
PIXEL = 2 * 10 * np.tan(np.radians(20.0)) / H1  # a pixel's width at distance 10 (vfov 40 over 12 rows)


def _light(k):
    return {"type": "diffuse_light", "emit": [float(5 + k), float(17 + 2 * k), float(40 + 3 * k)]}


MIRROR = {"type": "metal", "albedo": [1.0, 1.0, 1.0], "fuzz": 0.0}


def light_world(kind):
    if kind == "speck":    # a sphere 0.9 pixels wide inside tile (0, 0), on the edge between pixels (3, 3) and (3, 4)
        world = [{"type": "sphere", "center": [-6.0 * PIXEL, 2.5 * PIXEL, -10.0], "radius": 0.45 * PIXEL,
                  "material": _light(0)}]
    elif kind == "wall":   # one sphere over the whole image
        world = [{"type": "sphere", "center": [0, 0, -10], "radius": 8.0, "material": _light(0)}]
    elif kind == "mirrors":  # lights seen directly and over up to seven mirror bounces
        world = [{"type": "sphere", "center": [0, -102.0, -10], "radius": 100.0, "material": MIRROR},
                 {"type": "sphere", "center": [-2.5, 0, -10], "radius": 1.6, "material": MIRROR},
                 {"type": "sphere", "center": [2.5, 0.2, -9], "radius": 1.4, "material": MIRROR},
                 {"type": "sphere", "center": [0, 0.5, -12], "radius": 1.2, "material": _light(1)},
                 {"type": "sphere", "center": [0.3, -1.2, -7], "radius": 0.5, "material": _light(2)}]
    else:
        raise KeyError(kind)
    return {"world": world, "lights": [], "use_bvh": True,
            "camera": {"aspect_ratio": W1 / (H1 + 0.5), "image_width": W1, "samples_per_pixel": SPP1, "max_depth": 8,
                       "defocus_angle": 0, "focus_dist": 10, "background": BG, "vup": [0, 1, 0],
                       "lookfrom": [0, 0, 0], "lookat": [0, 0, -1], "vfov": 40}}


@functools.lru_cache(maxsize=None)
def light_reference(kind):
    S = load_scene(light_world(kind))
    cam, _ = sized(S, W1, H1, SPP1)
    ref = O.oracle_render(S, cam, O.MODE_COUNTER, SEED, output=abi.RT_OUT_SUM)
    assert np.array_equal(ref, np.round(ref))
    ref.setflags(write=False)
    return ref


def test_light_worlds_are_what_the_cases_need():
    """Host only: the speck covers 2-3 pixels of tile (0, 0) alone, the wall every
    pixel, and the mirror world has paths of more than one segment."""
    sky = SPP1 * np.asarray(BG)
    speck = (light_reference("speck") != sky).any(axis=2)
    assert 2 <= speck.sum() <= 3 and speck[:8, :8].sum() == speck.sum()
    wall = light_reference("wall")
    assert np.array_equal(wall, np.broadcast_to(SPP1 * np.asarray(_light(0)["emit"]), wall.shape))
    m = light_reference("mirrors")
    seen = {tuple(v) for v in m.reshape(-1, 3)}
    assert len(seen) > 8 and (m != sky).any(axis=2).sum() > W1 * H1 // 8  # a mirror that shows sky equals it


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["speck", "wall", "mirrors"])
def test_integer_worlds_equal_the_oracle_bit_for_bit(kind):
    S = load_scene(light_world(kind))
    _, f = sized(S, W1, H1, SPP1)
    with Renderer(S) as R:
        assert R.info()["features"] == FLAT
        got = R.render(f, seed=SEED, output=abi.RT_OUT_SUM)
    ref = light_reference(kind)
    bad = np.argwhere((got != ref).any(axis=2))
    assert len(bad) == 0, "%s: %d pixels differ, first (row, col) %s: %s vs %s" % (
        kind, len(bad), tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])])
    assert np.array_equal(got, ref)


# ---------------------------------------------------------------- 2. Lambertian parity
W2, H2 = 24, 16


def twin():
    """three_spheres with a quad hidden in the ground: no root table, the item walk."""
    return load_scene(spheres(3, hidden_quad=True))


@functools.lru_cache(maxsize=None)
def lambert_reference(spp):
    S = load_scene(spheres(3))
    cam, _ = sized(S, W2, H2, spp)
    ref = O.oracle_render(S, cam, O.MODE_COUNTER, SEED)
    ref.setflags(write=False)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 4, 16])
def test_lambertian_world_matches_the_oracle(spp):
    S = load_scene(spheres(3))
    _, f = sized(S, W2, H2, spp)
    with Renderer(S) as R:
        assert R.info()["features"] == FLAT | DIFFUSE
        got = R.render(f, seed=SEED)
    ref = lambert_reference(spp)
    d = np.abs(got - ref)
    print("%d strata: max |gpu - oracle| = %g" % (spp, d.max()))
    assert np.isfinite(got).all() and got.max() > 0
    assert d.max() <= BAR
    if spp == 1:  # nothing is ever parked: the bits of the item walk
        T = twin()
        _, ft = sized(T, W2, H2, spp)
        with Renderer(T) as R:
            assert R.info()["features"] & FLAT
            other = R.render(ft, seed=SEED)
        assert np.array_equal(got, other)


# ---------------------------------------------------------------- 3. the end of the queue
QUEUE = [(strata, depth) for strata in (2, 3) for depth in (1, 8)]
COUNTS = ("samples", "segments", "shade_events")


def _queue_case(S, strata, depth):
    _, f = sized(S, 8, 8, 4, depth)
    with Renderer(S) as R:
        assert R.info()["features"] & FLAT
        frame = R.render(f, seed=SEED, samples=(0, strata), output=abi.RT_OUT_SUM)
        st = R.stats(f, seed=SEED, samples=(0, strata))
    return frame, np.array([st[k] for k in COUNTS], dtype=np.int64)


def _child(path):
    out = {}
    for strata, depth in QUEUE:
        for name, S in (("scene", load_scene(spheres(3))), ("twin", twin())):
            frame, counts = _queue_case(S, strata, depth)
            out["%s_frame_%d_%d" % (name, strata, depth)] = frame
            out["%s_counts_%d_%d" % (name, strata, depth)] = counts
    np.savez(path, **out)


@functools.lru_cache(maxsize=None)
def queue_results(tmp):
    path = os.path.join(tmp, "queue.npz")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return dict(np.load(path))


@pytest.fixture(scope="module")
def queue(tmp_path_factory):
    return queue_results(str(tmp_path_factory.mktemp("parked")))


@pytest.mark.gpu
@pytest.mark.parametrize("strata,depth", QUEUE)
def test_queue_end_is_shaded_and_counted(queue, strata, depth):
    got = queue["scene_frame_%d_%d" % (strata, depth)]
    S = load_scene(spheres(3))
    cam, _ = sized(S, 8, 8, 4, depth)
    ref = O.oracle_render(S, cam, O.MODE_COUNTER, SEED, samples=(0, strata), output=abi.RT_OUT_SUM)
    d = np.abs(got - ref) / strata  # per-sample means, the bar's scale
    print("%d strata, depth %d: max |gpu - oracle| = %g" % (strata, depth, d.max()))
    assert np.isfinite(got).all()
    assert d.max() <= BAR
    counts = dict(zip(COUNTS, queue["scene_counts_%d_%d" % (strata, depth)]))
    other = dict(zip(COUNTS, queue["twin_counts_%d_%d" % (strata, depth)]))
    print(counts)
    assert counts["samples"] == 64 * strata
    assert counts["segments"] >= counts["samples"] and counts["shade_events"] > 0
    assert counts == other
    if depth == 1:
        assert counts["segments"] == counts["samples"]


# ---------------------------------------------------------------- 4. determinism
@pytest.mark.gpu
def test_launches_reproduce_their_bits():
    import torch
    S = load_scene(spheres(3))
    _, f = sized(S, 60, 36, 16)
    n_tiles = 8 * 5
    with Renderer(S) as R:
        assert R.info()["features"] == FLAT | DIFFUSE
        a = R.render(f, seed=SEED, output=abi.RT_OUT_SUM)
        b = R.render(f, seed=SEED, output=abi.RT_OUT_SUM)
        assert np.isfinite(a).all() and np.array_equal(a, b)
        # a unit's result depends on the unit alone: every other tile, launched
        # without its neighbours, against the same tiles of the whole launch
        kw = dict(seed=SEED, output=abi.RT_OUT_SUM, layout=abi.RT_LAYOUT_TILES)
        whole = R.render(f, tiles=(0, 1), **kw)
        odd = R.render(f, tiles=(1, 2), **kw)
        assert whole.shape == (n_tiles, 64, 3) and odd.shape == (n_tiles // 2, 64, 3)
        assert np.array_equal(odd, whole[1::2])
        assert np.array_equal(odd, R.render(f, tiles=(1, 2), **kw))
        # a tile-list launch, twice
        lst = torch.tensor([0, 3, 7, 8, 21, 39], dtype=torch.int32, device="cuda")
        bufs = [torch.zeros((36, 60, 3), dtype=torch.float64, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        for buf in bufs:
            R.render_tiles_device(f, lst.data_ptr(), len(lst), buf.data_ptr(), None, seed=SEED, accumulate=0)
        torch.cuda.synchronize()
        x, y = (buf.cpu().numpy() for buf in bufs)
        assert x.any() and np.array_equal(x, y)


if __name__ == "__main__":
    _child(sys.argv[1])
