"""Camera-ray batches traced where they are generated (rt_kernel.hip, rt_camq.h).

Every render_tiles instance of F == F_FLAT generates a stratum of its tile's 64
camera rays with the whole wave.  Without a defocus disk, in a world with a
root table, it traces the batch right there and keeps (closest, best) in the
ring entry; a popped hit arrives parked, a popped miss adds the background at
once and leaves its lane idle for the next pass of the refill loop.  With a
disk, or without a table (the hidden-quad twins), nothing changes.  A sample keeps
its value; what the new flow can get wrong is the accounting -- a miss added
twice or never, a hit shaded with another entry's root, a counter off, a loop
that does not end.  A unit of one batch keeps the old flow (it is popped by
all 64 lanes at once), and the default plan cuts a small frame into one-stratum
units, so the frames below are rendered in whole-tile units (whole_units): 9
or 16 batches per unit in test 3, 4 in tests 4 and 5, up to 16 in test 2.
Checked here:

 1. the flow on the host (no GPU): host/rtx_batch_check replays the refill and
    parking rules over seeded outcomes and checks itself -- every item settled
    once as a miss or handed once to the lane of its rank, no entry read before
    it is written or after it is overwritten, a trip after one that waited takes
    an item, every trip makes progress, the loop ends;
 2. all-sky and all-hit tiles: a 16x8 frame whose camera looks away from the
    only sphere equals strata x background exactly, with no shade event; the
    same camera inside one large integer light equals the oracle bit for bit;
 3. mixed ragged tiles: the integer light worlds of test_parked_shading at
    20x12 and 21x13, 9 and 16 strata, depth 1, 2 and 8, equal the oracle's
    COUNTER frame bit for bit; segments == samples at depth 1, and sphere_tests
    == n_roots x segments (every world here has a root table);
 4. counters: Lambertian worlds of 1, 3 and 7 spheres at 24x16, 4 strata: the
    STATS launch counts what the host twin of the kernel source counts, and the
    Lambertian-only and the general instance render the same bits, the
    oracle's frame at the GPU bar;
 5. beside the origin table: a world with a defocus disk (not traced at
    generation) and one of 7 roots (more than the table of the camera-origin
    root form holds, rt_path.h kRootOriginMax: the general test at generation),
    at 24x16 and 1 / 4 strata against the oracle at the GPU bar; at 1 stratum
    each equals its hidden-quad twin bit for bit;
 6. unit boundaries: a tile subset in 2 stratum chunks equals the same tiles of
    the whole launch, and a launch repeated equals itself, bit for bit; the
    chunks' sums add up to the oracle's frame at the GPU bar and to the
    whole-tile units' frame up to the order of the adds.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from rtx import abi
from rtx.render import Renderer
from rtx.scene import load_scene
import material_worlds as MW
import oracle_lib as O
from test_flat_table import spheres
from test_parked_shading import BAR, BG, SEED, _light, light_world, sized

FLAT, DIFFUSE = abi.RT_FEAT_FLAT, abi.RT_FEAT_DIFFUSE
CHECK = os.path.join(O.ROOT, "real-time-ray-tracing-engine_amd", "build", "rtx_batch_check")


def whole_units(S):
    """A renderer whose frame launches run one work unit per tile, all strata in
    it (rt_tuning.chunk_target < 0).  The default plan cuts frames this small
    into one-stratum units -- one batch each, which the kernel leaves on the
    old flow -- so only whole-tile units put the generation-time trace under a
    frame's assertions."""
    return Renderer(S, tuning={"chunk_target": -1})


# ---------------------------------------------------------------- 1. the flow on the host
FLOW = [(n, t, k) for n in (64, 128, 192, 576) for t in (1, 16) for k in (1, 48)]


def replay(n_items, threshold, k, seed, mode):
    r = subprocess.run([CHECK, str(n_items), str(threshold), str(k), str(seed), mode], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, "%s %d/%d/%d seed %d: %s" % (mode, n_items, threshold, k, seed, r.stderr)
    w = r.stdout.split()
    assert w[0] == "OK"
    return dict(zip(w[1::2], (int(x) for x in w[2::2])))


@pytest.mark.parametrize("n_items,threshold,k", FLOW)
def test_refill_and_parking_flow_settles_every_item_once_and_ends(n_items, threshold, k):
    repeats = 0
    for seed in (1, 2, 3, 4):
        c = replay(n_items, threshold, k, seed, "mixed")
        assert c["items"] == n_items == c["hits"] + c["misses"] + c["outside"]
        assert c["hits"] > 0 and c["misses"] > 0
        repeats = max(repeats, c["max_passes"])
    if n_items >= 192:  # what the replay is for: misses leave lanes idle and the refill loop repeats
        assert repeats > 1
    c = replay(n_items, threshold, k, 5, "allmiss")
    assert c["hits"] == 0 and c["misses"] + c["outside"] == n_items and c["shades"] == 0
    c = replay(n_items, threshold, k, 6, "allhit")
    assert c["misses"] == 0 and c["hits"] + c["outside"] == n_items
    c = replay(n_items, threshold, k, 7, "lens")  # untraced pops: the path loop's trace site decides
    assert c["hits"] + c["misses"] + c["outside"] == n_items


# ---------------------------------------------------------------- 2. all-sky and all-hit tiles
W2, H2 = 16, 8


def away(world):
    d = light_world("speck")
    d["world"] = world
    d["camera"]["lookat"] = [0, 0, 1]  # every sphere of light_world lies at z < 0
    return d


SKY = away(light_world("speck")["world"])
INSIDE = away([{"type": "sphere", "center": [0, 0, 0], "radius": 50.0, "material": _light(3)}])


@pytest.mark.gpu
@pytest.mark.parametrize("strata", [1, 3, 16])
def test_all_sky_and_all_hit_tiles_are_exact(strata):
    kw = dict(seed=SEED, samples=(0, strata))  # the first strata of a 16-stratum frame
    S = load_scene(SKY)
    _, f = sized(S, W2, H2, 16)
    with whole_units(S) as R:
        assert R.info()["features"] == FLAT
        got = R.render(f, output=abi.RT_OUT_SUM, **kw)
        st = R.stats(f, **kw)
    assert np.array_equal(got, np.broadcast_to(strata * np.asarray(BG), got.shape))
    assert st["samples"] == W2 * H2 * strata == st["segments"] and st["shade_events"] == 0
    # every camera ray hits: from inside the light (its back face, which the
    # oracle decides), and the wall of light_world seen from outside (its front)
    for doc in (INSIDE, light_world("wall")):
        S = load_scene(doc)
        cam, f = sized(S, W2, H2, 16)
        with whole_units(S) as R:
            assert R.info()["features"] == FLAT
            got = R.render(f, output=abi.RT_OUT_SUM, **kw)
            st = R.stats(f, **kw)
        ref = O.oracle_render(S, cam, O.MODE_COUNTER, SEED, samples=(0, strata), output=abi.RT_OUT_SUM)
        assert np.array_equal(ref, np.round(ref)) and (ref == ref[0, 0]).all()
        assert np.array_equal(got, ref)
        assert st["samples"] == W2 * H2 * strata == st["segments"] == st["shade_events"]
    assert ref.min() > 0  # the wall's front face emits


# ---------------------------------------------------------------- 3. mixed ragged tiles
N_ROOTS = {"speck": 1, "wall": 1, "mirrors": 5}
RAGGED = [(kind, w, h, spp, depth) for kind in ("speck", "wall", "mirrors") for (w, h) in ((20, 12), (21, 13))
          for spp in (9, 16) for depth in (1, 2, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,w,h,spp,depth", RAGGED)
def test_ragged_integer_worlds_equal_the_oracle_at_every_depth(kind, w, h, spp, depth):
    S = load_scene(light_world(kind))
    cam, f = sized(S, w, h, spp, depth)
    ref = O.oracle_render(S, cam, O.MODE_COUNTER, SEED, output=abi.RT_OUT_SUM)
    assert np.array_equal(ref, np.round(ref))
    with whole_units(S) as R:
        assert R.info()["features"] == FLAT
        got = R.render(f, seed=SEED, output=abi.RT_OUT_SUM)
        st = R.stats(f, seed=SEED)
    bad = np.argwhere((got != ref).any(axis=2))
    assert len(bad) == 0, "%s %dx%d, %d strata, depth %d: %d pixels differ, first (row, col) %s: %s vs %s" % (
        kind, w, h, spp, depth, len(bad), tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])])
    assert st["samples"] == w * h * spp
    if depth == 1:
        assert st["segments"] == st["samples"]
    else:
        assert st["segments"] >= st["samples"]
    assert st["sphere_tests"] == N_ROOTS[kind] * st["segments"] and st["quad_tests"] == 0


# ---------------------------------------------------------------- 4. counters
W4, H4, SPP4 = 24, 16, 4
COUNTERS = ("samples", "segments", "shade_events", "sphere_tests", "quad_tests", "node_visits")


@pytest.fixture(scope="module")
def emu():
    return MW.load_emu()


def host_stats(emu, S, f):
    d = S.desc()
    p = abi.RenderParams()
    p.seed, p.sample_count, p.output = SEED, -1, abi.RT_OUT_SCALED
    st = abi.PathStats()
    out = np.zeros((f.image_height, f.image_width, 3))
    assert emu.emu_render_stats(C.byref(d), C.byref(f), C.byref(p), 0, out.ctypes.data_as(C.POINTER(C.c_double)),
                                C.byref(st)) == 0
    return {k: getattr(st, k) for k in COUNTERS}


def general_twin(n):
    """The same world with an unused metal in its materials table: the general flat instance."""
    S = load_scene(spheres(n))
    S.add_material(abi.RT_MAT_METAL, albedo=(0.8, 0.6, 0.2), fuzz=0.25)
    return S


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 7])
def test_counters_are_the_host_twins_and_both_flat_instances_agree(emu, n):
    S, G = load_scene(spheres(n)), general_twin(n)
    cam, f = sized(S, W4, H4, SPP4)
    host = host_stats(emu, S, f)
    frames, stats = [], []
    for scene, want in ((S, FLAT | DIFFUSE), (G, FLAT)):
        with whole_units(scene) as R:
            assert R.info()["features"] == want
            frames.append(R.render(f, seed=SEED, output=abi.RT_OUT_SUM))
            st = R.stats(f, seed=SEED)
            stats.append({k: st[k] for k in COUNTERS})
    print("n=%d gpu  %s\nn=%d host %s" % (n, stats[0], n, host))
    assert stats[0] == stats[1] == host
    assert host["samples"] == W4 * H4 * SPP4 and host["sphere_tests"] == n * host["segments"]
    assert host["node_visits"] == 0 and host["shade_events"] > 0
    assert np.isfinite(frames[0]).all() and frames[0].max() > 0
    assert np.array_equal(frames[0], frames[1])
    ref = O.oracle_render(S, cam, O.MODE_COUNTER, SEED, output=abi.RT_OUT_SUM)
    d = np.abs(frames[0] - ref) / SPP4  # per-sample means, the bar's scale
    print("n=%d: max |gpu - oracle| = %g" % (n, d.max()))
    assert d.max() <= BAR


# ---------------------------------------------------------------- 5. beside the origin table
def off_table(kind, hidden_quad=False):
    if kind == "lens":  # a defocus disk: generation does not trace, the path loop does
        d = spheres(3, hidden_quad=hidden_quad)
        d["camera"].update(defocus_angle=4.0, focus_dist=1.0)
        return d
    assert kind == "seven"  # more roots than kRootOriginMax (rt_path.h): the general test at generation
    return spheres(7, hidden_quad=hidden_quad)


@functools.lru_cache(maxsize=None)
def off_table_reference(kind, spp):
    S = load_scene(off_table(kind))
    cam, _ = sized(S, W4, H4, spp)
    ref = O.oracle_render(S, cam, O.MODE_COUNTER, SEED)
    ref.setflags(write=False)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lens", "seven"])
@pytest.mark.parametrize("spp", [1, 4])
def test_lens_and_above_the_cap_worlds_match_the_oracle(kind, spp):
    S = load_scene(off_table(kind))
    _, f = sized(S, W4, H4, spp)
    with whole_units(S) as R:
        assert R.info()["features"] & ~DIFFUSE == FLAT
        got = R.render(f, seed=SEED)
    d = np.abs(got - off_table_reference(kind, spp))
    print("%s, %d strata: max |gpu - oracle| = %g" % (kind, spp, d.max()))
    assert np.isfinite(got).all() and got.max() > 0
    assert d.max() <= BAR
    if spp == 1:
        T = load_scene(off_table(kind, hidden_quad=True))
        _, ft = sized(T, W4, H4, spp)
        with Renderer(T) as R:
            assert R.info()["features"] & FLAT
            other = R.render(ft, seed=SEED)
        assert np.array_equal(got, other)


# ---------------------------------------------------------------- 6. unit boundaries
def frame_of_tiles(t, w, h):
    """Tile-layout sums [tiles, 64, 3] (tile ty * tiles_x + tx, slot 8 (y & 7) + (x & 7)) as a frame."""
    tx = (w + 7) // 8
    out = np.zeros((h, w, 3))
    for y in range(h):
        for x in range(w):
            out[y, x] = t[(y // 8) * tx + x // 8, 8 * (y & 7) + (x & 7)]
    return out


@pytest.mark.gpu
def test_chunked_tile_subsets_and_repeats_reproduce_their_bits():
    S = load_scene(spheres(3))
    w, h, spp = 21, 13, 9
    cam, f = sized(S, w, h, spp)
    n_tiles = 3 * 2
    kw = dict(seed=SEED, output=abi.RT_OUT_SUM)
    ref = O.oracle_render(S, cam, O.MODE_COUNTER, SEED, output=abi.RT_OUT_SUM)
    with whole_units(S) as R:
        assert R.info()["features"] == FLAT | DIFFUSE
        whole = R.render(f, **kw)
        assert np.isfinite(whole).all() and whole.max() > 0
        assert np.abs(whole - ref).max() / spp <= BAR  # whole-tile units: 9 batches each
        assert np.array_equal(whole, R.render(f, **kw))
        # 2 stratum chunks of 5 and 4 strata: units of more than one batch, other boundaries
        tl = dict(layout=abi.RT_LAYOUT_TILES, chunks=2, **kw)
        tiles = R.render(f, tiles=(0, 1), **tl)
        odd = R.render(f, tiles=(1, 2), **tl)
        assert tiles.shape == (n_tiles, 2, 64, 3) and odd.shape == (n_tiles // 2, 2, 64, 3)
        assert tiles[:, 0].any() and tiles[:, 1].any()
        assert np.array_equal(odd, tiles[1::2])
        assert np.array_equal(tiles, R.render(f, tiles=(0, 1), **tl))
        # ... and their values: the chunks of a tile add up to the oracle's sums, and to the whole-tile
        # unit's up to the order of 9 adds (2 (n - 1) 2^-53 relative, non-negative terms)
        summed = frame_of_tiles(tiles.sum(axis=1), w, h)
        assert np.abs(summed - ref).max() / spp <= BAR
        assert (np.abs(summed - whole) <= 2 * (spp - 1) * 2.0 ** -53 * whole).all()
