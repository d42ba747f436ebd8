"""rt_occluded_device / rt_occluded / rt_multi_occluded on gfx950 against the
host build of the same source (csrc/rt_occlusion.h through
tests/native/rt_occlusion_emu.cpp): byte for byte over every walk the library
takes, guards, grouping, unaligned output, the wave shapes an early exit can
get wrong, refusals, the live scene (visible, edit, visible again), rebuilds,
scene lifetime and the render frames around a query."""
import ctypes as C

import numpy as np
import pytest
import torch

from rtx import abi
from rtx.lib import load
from rtx.render import RAY_DTYPE, MultiRenderer, Renderer, camera_frame, pixel_ray, segment_ray
from rtx.scene import load_scene
from test_device_bvh import random_spheres
from test_occlusion import host_occluded, limited, verdicts
from test_ray_queries import make_rays
from test_ray_queries_gpu import N, TAIL, WALKS, committed, scene_rays, to_device, walk

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 4096  # bytes on each side of the verdicts
SHORT = 0.3   # the fixed short t_max of limited(), in units of the rays' directions


def _stream():
    return torch.cuda.current_stream().cuda_stream


class GuardedBytes:
    """n verdict bytes between two sentinel-filled guards, `shift` bytes into the allocation."""

    def __init__(self, n, shift=0):
        self.n = n
        self.lo = GUARD + shift
        self.all = torch.full((self.lo + n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.ptr = self.all.data_ptr() + self.lo

    def read(self, written=None):
        """The first `written` bytes (default all); the guards and the bytes after them keep the sentinel."""
        w = self.n if written is None else written
        a = self.all.cpu().numpy()
        assert np.all(a[:self.lo] == SENTINEL), "guard below overwritten"
        assert np.all(a[self.lo + w:] == SENTINEL), "written past byte %d" % w
        return a[self.lo:self.lo + w].copy()


def device_occluded(R, rays, n=None, stream=None, shift=0):
    n = len(rays) if n is None else n
    keep, ptr = to_device(rays)
    buf = GuardedBytes(len(rays), shift)
    torch.cuda.synchronize()  # the fills ran on the current stream
    R.occluded_device(ptr, buf.ptr, n, stream if stream is not None else _stream())
    torch.cuda.synchronize()
    return buf.read(n)


_cache = {}


def occ_walk(name):
    """(description, rays with limits, the occlusion twin's bytes): built once per scene, read-only."""
    if name not in _cache:
        S, rays, free = walk(name)
        lim = limited(rays, free["t"], 5, SHORT)
        want = host_occluded(S, lim)
        # the reference twin of tests/test_ray_queries.py says the same (tests/test_occlusion.py's subject)
        cut = ((free["t"] < np.inf) & (want == 0)).sum()
        assert 200 < want.sum() < N - 200 and cut > 200, (name, want.sum(), cut)  # teeth
        lim.setflags(write=False)
        want.setflags(write=False)
        _cache[name] = (S, lim, want)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(WALKS))
def test_device_bytes_equal_the_host_build(name):
    S, rays, want = occ_walk(name)
    _, must, must_not, builder = WALKS[name]
    with Renderer(S) as R:
        info = R.info()
        assert info["features"] & must == must and not info["features"] & must_not, info
        if builder is not None:
            assert info["bvh_builder"] == builder, info
        got = device_occluded(R, rays)
        differ = np.nonzero(got != want)[0]
        assert got.tobytes() == want.tobytes(), "%d of %d bytes differ, first %s" % (len(differ), N, differ[:8])
        # n = 130 of the same arrays writes 130 bytes: two full waves and a tail of two lanes
        assert device_occluded(R, rays, n=TAIL).tobytes() == want[:TAIL].tobytes()
        # the host arrays' entry point, and the records' verdicts from the device itself
        occ = R.occluded(rays)
        assert occ.dtype == np.bool_ and occ.view(np.uint8).tobytes() == want.tobytes()
        assert verdicts(R.trace(rays)).tobytes() == want.tobytes()


def test_grouping_alignment_and_entry_points_give_the_same_bytes():
    S, rays, want = occ_walk("bouncing_seed42")
    other = torch.cuda.Stream()
    with Renderer(S) as R:
        for n in (1, 63, 64, 65):
            assert device_occluded(R, rays[:n]).tobytes() == want[:n].tobytes(), n
            assert device_occluded(R, rays, n=n).tobytes() == want[:n].tobytes(), n
        assert device_occluded(R, rays[1000:1001])[0] == want[1000]  # alone = at position 1,000
        for shift in (1, 3):  # the bytes need no alignment
            assert device_occluded(R, rays[:300], shift=shift).tobytes() == want[:300].tobytes(), shift
            assert device_occluded(R, rays, shift=shift).tobytes() == want.tobytes(), shift
        assert device_occluded(R, rays, stream=other.cuda_stream).tobytes() == want.tobytes()  # any stream
        # a torch.bool buffer as the output
        keep, rp = to_device(rays)
        out = torch.zeros(N, dtype=torch.bool, device="cuda")
        torch.cuda.synchronize()
        R.occluded_device(rp, out.data_ptr(), N, _stream())
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want.astype(bool))
        assert R.occluded(rays[:65]).view(np.uint8).tobytes() == want[:65].tobytes()
        rows = np.ascontiguousarray(rays).view(np.float64).reshape(-1, 8)[:7]
        assert R.occluded(rows).view(np.uint8).tobytes() == want[:7].tobytes()
        assert len(R.occluded(rays[:0])) == 0
        R.occluded_device(0, 0, 0)  # n = 0: nothing queued, RT_OK
    with MultiRenderer(S, devices=(0,), shards=2) as M:
        assert M.occluded(rays).view(np.uint8).tobytes() == want.tobytes()


# ---------------------------------------------------------------- wave shapes
def _wave_scenes():
    flat = committed("three_spheres")
    tree = committed("bouncing_seed42")
    tree4 = committed("bouncing_seed42")
    tree4.bvh_arity = 4
    return {"flat": flat, "tree": tree, "tree4": tree4}


@pytest.mark.parametrize("which", ["flat", "tree", "tree4"])
def test_wave_shapes_an_early_exit_can_get_wrong(which):
    S = _wave_scenes()[which]
    f = camera_frame(S.camera_desc(image_width=16, samples_per_pixel=1))
    # a ray that the first thing it meets blocks (the ground under the frame's lower edge) ...
    block = pixel_ray(f, f.image_width / 2, f.image_height - 1)
    # ... and one that meets nothing: straight up from the camera
    free = make_rays(block["origin"], [0.0, 1.0, 0.0])
    nan = np.array(block)
    nan["origin"][0, 1] = np.nan
    assert host_occluded(S, block)[0] == 1 and host_occluded(S, free)[0] == 0 and host_occluded(S, nan)[0] == 0
    shapes = {
        "63 blocked, the last lane free": np.concatenate([np.repeat(block, 63), free]),
        "63 blocked, the first lane free": np.concatenate([free, np.repeat(block, 63)]),
        "all 64 blocked": np.repeat(block, 64),
        "all 64 free": np.repeat(free, 64),
        "all 64 invalid": np.repeat(nan, 64),
        "one blocked among the invalid": np.concatenate([np.repeat(nan, 40), block, np.repeat(nan, 23)]),
    }
    with Renderer(S) as R:
        for what, rays in shapes.items():
            want = host_occluded(S, rays)
            assert device_occluded(R, rays).tobytes() == want.tobytes(), what
            # the wave after it is split between n and past n: 64 + 37 rays of 128
            two = np.concatenate([rays, rays[::-1]])
            got = device_occluded(R, two, n=64 + 37)
            assert got.tobytes() == np.concatenate([want, want[::-1]])[:64 + 37].tobytes(), what
        assert device_occluded(R, shapes["63 blocked, the last lane free"]).tolist() == [1] * 63 + [0]
        assert not device_occluded(R, shapes["all 64 invalid"]).any()


def test_refusals_leave_the_buffer_untouched():
    S, rays, _ = occ_walk("three_spheres")
    L = load()
    keep, rp = to_device(rays)
    buf = GuardedBytes(N)
    torch.cuda.synchronize()
    host = np.full(8, SENTINEL, dtype=np.uint8)
    with Renderer(S) as R:
        for n, r, o in ((-1, rp, buf.ptr), (N, None, buf.ptr), (N, rp, None), (2 ** 36 + 1, rp, buf.ptr)):
            assert L.rt_occluded_device(R.handle, n, r, o, C.c_void_p(_stream())) == abi.RT_ERR_INVALID, n
            assert L.rt_last_error(), n
        assert L.rt_occluded_device(None, N, rp, buf.ptr, C.c_void_p(_stream())) == abi.RT_ERR_INVALID
        assert L.rt_occluded(R.handle, -1, rays.ctypes.data, host.ctypes.data) == abi.RT_ERR_INVALID
        assert L.rt_occluded(R.handle, 8, None, host.ctypes.data) == abi.RT_ERR_INVALID
        torch.cuda.synchronize()
    assert len(buf.read(0)) == 0  # every byte still the sentinel
    assert (host == SENTINEL).all()


# ---------------------------------------------------------------- the live scene
def row_of_spheres():
    """Twelve spheres in a row along x (a tree, not a flat leaf); sphere 5
    stands between the two points of the test below."""
    mat = {"type": "lambertian", "albedo": [0.5, 0.5, 0.5]}
    world = [{"type": "sphere", "center": [3.0 * k, 0.0, 0.0], "radius": 1.0, "material": mat} for k in range(12)]
    return load_scene({"camera": {"lookfrom": [15.0, 2.0, 30.0], "lookat": [15.0, 0.0, 0.0], "vfov": 40.0},
                       "world": world})


def test_visible_across_a_sphere_that_moves_away_and_back():
    S = row_of_spheres()
    ids = [i for i, o in enumerate(S.objects) if o.kind == abi.RT_OBJ_SPHERE]
    o = ids[5]
    home = np.array([[S.objects[o].a.x, S.objects[o].a.y, S.objects[o].a.z]])
    assert home.tolist() == [[15.0, 0.0, 0.0]]
    away = home + [0.0, 500.0, 0.0]
    a = np.array([[15.0, 0.0, 8.0], [15.0, 3.0, 8.0], [13.5, 0.0, 8.0]])
    b = np.array([[15.0, 0.0, -8.0], [15.0, 3.0, -8.0], [13.5, 0.0, -8.0]])  # through it, over it, between two
    st = torch.cuda.Stream()
    with Renderer(S) as R:
        assert R.info()["n_nodes"] > 0
        assert R.visible(a, b).tolist() == [False, True, True]
        R.move_spheres([o], away)
        assert R.visible(a, b).tolist() == [True, True, True]
        with Renderer(S) as F:  # the description followed the move: a fresh scene says the same
            assert F.visible(a, b).tolist() == [True, True, True]
        R.move_spheres([o], home)
        assert R.visible(a, b).tolist() == [False, True, True]
        with Renderer(S) as F:
            assert F.visible(a, b).tolist() == [False, True, True]
        # the edit and the query on one stream, no host wait between them
        rays = np.repeat(segment_ray(a, b), 50)
        keep, rp = to_device(rays)
        one, two = GuardedBytes(len(rays)), GuardedBytes(len(rays))
        idt = torch.tensor([o], dtype=torch.int32, device="cuda")
        c_away, c_home = torch.from_numpy(away).cuda(), torch.from_numpy(home).cuda()
        torch.cuda.synchronize()
        R.move_spheres_device(idt.data_ptr(), c_away.data_ptr(), 1, st.cuda_stream)
        R.occluded_device(rp, one.ptr, len(rays), st.cuda_stream)
        R.move_spheres_device(idt.data_ptr(), c_home.data_ptr(), 1, st.cuda_stream)
        R.occluded_device(rp, two.ptr, len(rays), st.cuda_stream)
        st.synchronize()
        assert not one.read().any()
        assert two.read().tolist() == np.repeat([1, 0, 0], 50).tolist()


def test_visible_across_a_box_by_its_transform_and_a_wall_by_its_quad():
    S = committed("cornell")
    f = camera_frame(S.camera_desc(image_width=40, aspect_ratio=1.0, samples_per_pixel=1))
    with Renderer(S) as R:
        # a box: the first pixel of a row below the middle whose hit stands under a chain
        j = f.image_height // 2 + 6
        i, h1 = next((i, h) for i, h in ((i, R.pick(f, i, j)) for i in range(f.image_width)) if h["chain_object"] >= 0)
        c = int(h1["chain_object"])
        ray = pixel_ray(f, i, j)
        a = ray["origin"]
        b = a + 1.02 * h1["t"] * ray["direction"]  # a little behind the face the ray meets
        home = np.array([[S.objects[c].a.x, S.objects[c].a.y, S.objects[c].a.z]])
        assert not R.visible(a, b)[0]
        R.set_transforms([c], home + [0.0, 2000.0, 0.0])
        assert R.visible(a, b)[0]
        with Renderer(S) as F:
            assert F.visible(a, b)[0]
        R.set_transforms([c], home)
        assert not R.visible(a, b)[0]
        with Renderer(S) as F:
            assert not F.visible(a, b)[0]
        # a wall: the quad under the frame's left edge, and a point behind it
        w1 = R.pick(f, 2, f.image_height // 2)
        q = int(w1["object"])
        assert S.objects[q].kind == abi.RT_OBJ_QUAD and w1["chain_object"] == -1
        ray = pixel_ray(f, 2, f.image_height // 2)
        a = ray["origin"]
        b = a + 1.05 * w1["t"] * ray["direction"]
        corner = np.array([[S.objects[q].a.x, S.objects[q].a.y, S.objects[q].a.z]])
        assert not R.visible(a, b)[0]
        R.move_quads([q], corner + [0.0, 5000.0, 0.0])
        assert R.visible(a, b)[0]
        with Renderer(S) as F:
            assert F.visible(a, b)[0]
        R.move_quads([q], corner)
        assert not R.visible(a, b)[0]


def test_a_rebuild_leaves_every_byte_as_it_was():
    """After a third of a 70,000-sphere cloud has moved, the refitted tree and
    the rebuilt one give the same bytes, and the host build's."""
    _, rays, want = occ_walk("cloud_70000")
    S = load_scene(random_spheres(70000))  # this test moves its own copy
    ids = np.array([i for i, o in enumerate(S.objects) if o.kind == abi.RT_OBJ_SPHERE], dtype=np.int32)[:-1][::3]
    rng = np.random.default_rng(3)
    new = np.array([[S.objects[i].a.x, S.objects[i].a.y, S.objects[i].a.z] for i in ids]) + rng.uniform(-3, 3, (len(ids), 3))
    with Renderer(S) as R:
        assert R.occluded(rays).view(np.uint8).tobytes() == want.tobytes()
        R.move_spheres(ids, new)
        refitted = R.occluded(rays)
        assert refitted.view(np.uint8).tobytes() != want.tobytes()
        assert R.rebuild_bvh()
        assert R.occluded(rays).tobytes() == refitted.tobytes()
        assert verdicts(R.trace(rays)).tobytes() == refitted.view(np.uint8).tobytes()


def test_scene_destroyed_right_after_the_query_leaves_every_byte():
    S, rays, want = occ_walk("bouncing_seed42")
    st = torch.cuda.Stream()
    keep, rp = to_device(rays)
    buf = GuardedBytes(N)
    torch.cuda.synchronize()
    R = Renderer(S)
    R.occluded_device(rp, buf.ptr, N, st.cuda_stream)
    R.close()  # waits for the scene's own launch (the launch chain), and only for it
    assert st.query(), "destroy returned before its scene's query finished"
    assert buf.read().tobytes() == want.tobytes()


@pytest.mark.parametrize("name", ["cornell_fog", "bouncing_seed42"])
def test_a_query_does_not_disturb_the_render(name):
    S, rays, want = occ_walk(name)
    f = camera_frame(S.camera_desc(image_width=40, samples_per_pixel=4, max_depth=6))
    H, W = f.image_height, f.image_width
    other = torch.cuda.Stream()
    with Renderer(S) as R:
        def frame():
            out = torch.full((H, W, 3), -7.25, dtype=torch.float64, device="cuda")
            R.render_device(f, out.data_ptr(), _stream(), seed=3, samples=(0, 4), accumulate=0)
            return out.cpu().numpy()

        first = frame()
        keep, rp = to_device(rays)
        buf = GuardedBytes(N)
        torch.cuda.synchronize()
        R.occluded_device(rp, buf.ptr, N, other.cuda_stream)
        second = frame()
        other.synchronize()
        assert np.array_equal(first, second, equal_nan=True)
        assert buf.read().tobytes() == want.tobytes()
