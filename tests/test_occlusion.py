"""Occlusion queries (csrc/rt_occlusion.h) on the host: the occlusion kernel's
per-ray source compiled by g++ (tests/native/rt_occlusion_emu.cpp) against the
query twin of tests/test_ray_queries.py -- verdict == (record.t < inf), exactly
and for every ray -- over trees, t_max drawn three ways, t_max at and one ulp
around every hit, bad rays and media; rt_segment_ray; the ABI.  No GPU:
tests/test_occlusion_gpu.py holds the gfx950 bytes to this host build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rtx import abi
from rtx.lib import LIB_PATH, load
from rtx.render import RAY_DTYPE, camera_frame, pixel_ray, ray_array, segment_ray
from rtx.scene import load_scene
import oracle_lib as O
from test_ray_queries import (SCENES, bad_rays, cloud_hits, cloud_rays, cloud_scene, frame_rays, host_trace,
                              make_rays)

NATIVE = os.path.join(os.path.dirname(__file__), "native")
INF = float("inf")
SENTINEL = 7

_emu = None


def occlusion_emu():
    """tests/native/build/libocclusion_emu.so (built on first use: occlusion.mk)."""
    global _emu
    if _emu is None:
        subprocess.run(["make", "-s", "-C", NATIVE, "-f", "occlusion.mk"], check=True)
        L = C.CDLL(os.path.join(NATIVE, "build", "libocclusion_emu.so"))
        L.emu_occluded.argtypes = [C.POINTER(abi.SceneDesc), C.c_longlong, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        _emu = L
    return _emu


def host_occluded(S, rays, features=None):
    """rt_occlusion.h on the host: a uint8 array [n] of 0 / 1, written over a sentinel."""
    rays = ray_array(rays)
    d = S.desc()
    out = np.full(len(rays), SENTINEL, dtype=np.uint8)
    feat = C.c_int(0)
    assert occlusion_emu().emu_occluded(C.byref(d), len(rays), rays.ctypes.data, out.ctypes.data, C.byref(feat)) == 0
    if features is not None:
        features.append(feat.value)
    assert set(np.unique(out)) <= {0, 1}
    return out


def verdicts(hits):
    """What the contract makes of rt_trace's records: 1 where the record is a hit."""
    v = (hits["t"] < INF).astype(np.uint8)
    assert np.array_equal(v, (hits["object"] >= 0).astype(np.uint8))
    return v


def limited(rays, t_free, seed, short):
    """The rays with a t_max drawn per ray in one of three ways, a third each:
    +inf; a uniform fraction in (0, 2) of the ray's own unlimited hit distance
    `t_free` (+inf where it has none); the fixed length `short`."""
    rng = np.random.default_rng(seed)
    r = np.array(rays)
    how = rng.integers(0, 3, len(r))
    frac = rng.uniform(0.0, 2.0, len(r))
    frac[frac == 0.0] = 1.0  # (0, 2)
    r["t_max"] = np.where(how == 0, INF, np.where(how == 1, frac * t_free, short))
    assert (r["t_max"] > 0).all()
    return r


def check_against_the_query_twin(S, rays, free, what, teeth=True):
    """verdict == (record.t < inf) for every ray.  `free`: the query twin's
    records of the same rays without a limit.  teeth: a constant answer cannot
    pass -- judged on the reference twin alone."""
    want = verdicts(host_trace(S, rays))
    if teeth:
        share = want.mean()
        cut = ((free["t"] < INF) & (want == 0)).mean()
        print("%s: %d rays, occluded share %.3f, hit without a limit but not within t_max %.3f" % (
            what, len(rays), share, cut))
        assert 0.2 <= share <= 0.8, (what, share)
        assert cut >= 0.10, (what, cut)
    got = host_occluded(S, rays)
    differ = np.nonzero(got != want)[0]
    assert got.tobytes() == want.tobytes(), "%s: %d of %d verdicts differ, first %s" % (
        what, len(differ), len(rays), differ[:8])
    return got


# The fixed short lengths, in units of the rays' directions, chosen on the CPU
# from the reference twin alone so that the two conditions above hold.
CLOUD_SHORT = 0.4


@pytest.mark.parametrize("arity,use_bvh", [(0, 0), (2, 1), (4, 1)])
def test_cloud_verdicts_equal_the_records_on_every_tree(arity, use_bvh):
    free = cloud_hits()
    rays = limited(cloud_rays(), free["t"], 21, CLOUD_SHORT)
    S = cloud_scene(arity, use_bvh)
    feats = []
    host_occluded(S, rays[:1], feats)
    assert bool(feats[0] & abi.RT_FEAT_BVH4) == (arity == 4)
    got = check_against_the_query_twin(S, rays, free, "cloud %d/%d" % (arity, use_bvh))
    # the tree does not matter: the default tree's verdicts
    assert got.tobytes() == host_occluded(cloud_scene(), rays).tobytes()
    # without a limit: the unlimited records' verdicts
    assert host_occluded(S, cloud_rays()).tobytes() == verdicts(free).tobytes()


# scene -> the fixed short length: about the median t of the frame's unlimited hits (t counts in the
# length of the pixel rays' directions, which differs from scene to scene)
COMMITTED = {"three_spheres": 0.07, "cornell": 100.0, "bouncing_seed42": 0.9, "cornell_fog": 100.0}


@pytest.mark.parametrize("name", sorted(COMMITTED))
def test_committed_scenes(name):
    S = load_scene(os.path.join(SCENES, name + ".json"))
    f = camera_frame(S.camera_desc(image_width=32, samples_per_pixel=1))
    rays = frame_rays(f, 0.37, 0.21)
    rays["time"] = np.random.default_rng(2).uniform(0, 1, len(rays))
    feats = []
    free = host_trace(S, rays, feats)
    assert bool(feats[0] & abi.RT_FEAT_FLAT) == (name in ("three_spheres", "cornell_fog"))  # both flat walks, both trees
    check_against_the_query_twin(S, limited(rays, free["t"], 22, COMMITTED[name]), free, name)
    assert host_occluded(S, rays).tobytes() == verdicts(free).tobytes()
    for arity in (2, 4):
        S.bvh_arity = arity
        lim = limited(rays, free["t"], 23, COMMITTED[name])
        assert host_occluded(S, lim).tobytes() == verdicts(host_trace(S, lim)).tobytes(), arity


def _kinds(S, hits):
    return np.array([S.objects[o].kind if o >= 0 else -1 for o in hits["object"]])


@pytest.mark.parametrize("kind", ["sphere", "quad"])
def test_t_max_at_and_one_ulp_around_each_hit(kind):
    """sphere_root's open interval and quad_t's closed one both come to
    `t <= t_max`, as rt_trace's comparison after the search does."""
    S, rays, free = cloud_scene(), cloud_rays(), cloud_hits()
    pick = _kinds(S, free) == (abi.RT_OBJ_SPHERE if kind == "sphere" else abi.RT_OBJ_QUAD)
    assert pick.sum() > 100
    r, t = np.array(rays[pick]), free["t"][pick]
    for tree in ((0, 0), (2, 1), (4, 1)):
        T = cloud_scene(*tree)
        for t_max, want in ((t, 1), (np.nextafter(t, INF), 1), (np.nextafter(t, 0.0), 0)):
            r["t_max"] = t_max
            ref = verdicts(host_trace(T, r))
            assert (ref == want).all()  # the reference itself: the nearest hit is at exactly t
            assert host_occluded(T, r).tobytes() == ref.tobytes(), (kind, tree, want)


def test_t_max_around_the_far_root_from_inside_a_sphere():
    """An origin inside a sphere: the near root is at or below tmin, the far
    root counts, and t_max at, above and below it decides."""
    S = cloud_scene()
    rng = np.random.default_rng(31)
    spheres = [o for o in S.objects if o.kind == abi.RT_OBJ_SPHERE and not o.moving and o.s < 10]
    assert len(spheres) > 20
    org = np.concatenate([[[o.a.x, o.a.y, o.a.z]] + 0.3 * o.s * rng.uniform(-1, 1, (8, 3)) for o in spheres])
    r = make_rays(org, rng.normal(size=(len(org), 3)) * rng.uniform(0.3, 2.0, (len(org), 1)))
    free = host_trace(S, r)
    inside = (_kinds(S, free) == abi.RT_OBJ_SPHERE) & (free["front"] == 0)  # met from within: a far root
    assert inside.sum() > 100
    r, t = np.array(r[inside]), free["t"][inside]
    for tree in ((0, 0), (2, 1), (4, 1)):
        T = cloud_scene(*tree)
        for t_max, want in ((t, 1), (np.nextafter(t, INF), 1), (np.nextafter(t, 0.0), 0), (0.5 * t, 0)):
            r["t_max"] = t_max
            ref = verdicts(host_trace(T, r))
            assert (ref == want).all()
            assert host_occluded(T, r).tobytes() == ref.tobytes(), (tree, want)


def test_no_limit_values_and_nan():
    S, rays, free = cloud_scene(), cloud_rays(), cloud_hits()
    for no_limit in (0.0, -0.0, -1.0, -INF, INF):
        r = np.array(rays)
        r["t_max"] = no_limit
        assert host_occluded(S, r).tobytes() == verdicts(free).tobytes(), no_limit
    r = np.array(rays)
    r["t_max"] = np.nan
    assert not host_occluded(S, r).any()


def test_bad_rays_are_unoccluded():
    S, rays, free = cloud_scene(), cloud_rays(), cloud_hits()
    k = int(np.nonzero(free["object"] >= 0)[0][0])
    for T, good in [(cloud_scene(a, u), rays[k:k + 1]) for a, u in ((0, 0), (2, 1), (4, 1))]:
        assert host_occluded(T, good)[0] == 1
        bad = bad_rays(good)
        assert len(bad) == 2 + 3 * 7 + 1
        assert not host_occluded(T, bad).any()
        short = np.array(bad)
        short["t_max"] = np.where(np.isnan(bad["t_max"]), np.nan, 1e9)  # a limit changes nothing
        assert not host_occluded(T, short).any()
    for name in ("three_spheres", "cornell"):  # the flat walks and the transform chains too
        T = load_scene(os.path.join(SCENES, name + ".json"))
        f = camera_frame(T.camera_desc(image_width=8, samples_per_pixel=1))
        good = pixel_ray(f, f.image_width / 2, f.image_height / 2)
        assert host_occluded(T, good)[0] == 1
        assert not host_occluded(T, bad_rays(good)).any()


def test_media_are_passed_through():
    S = load_scene(os.path.join(SCENES, "cornell_fog.json"))
    f = camera_frame(S.camera_desc(image_width=36, aspect_ratio=1.0, samples_per_pixel=1))
    rays = frame_rays(f)
    feats = []
    free = host_trace(S, rays, feats)
    assert feats[0] & abi.RT_FEAT_MEDIA
    lim = limited(rays, free["t"], 24, COMMITTED["cornell_fog"])
    fog = check_against_the_query_twin(S, lim, free, "cornell_fog")
    # the same description, the medium objects taken out of the world list: every table stays
    T = load_scene(os.path.join(SCENES, "cornell_fog.json"))
    w = T.objects[T.world]
    kids = [T.children[w.child + k] for k in range(w.count)]
    solid = [k for k in kids if T.objects[k].kind != abi.RT_OBJ_MEDIUM]
    assert 0 < len(solid) < len(kids)
    T.world = T.add_list(solid)
    feats = []
    clear = host_occluded(T, lim, feats)
    assert not feats[0] & abi.RT_FEAT_MEDIA
    assert fog.tobytes() == clear.tobytes()
    # a segment that ends inside the fog box, before any surface: unoccluded
    assert host_occluded(S, rays).tobytes() == verdicts(free).tobytes()


def test_a_ray_alone_equals_the_ray_in_its_batch():
    S, free = cloud_scene(), cloud_hits()
    rays = limited(cloud_rays(), free["t"], 21, CLOUD_SHORT)
    ref = host_occluded(S, rays)
    for n in (1, 63, 64, 65, 130):
        assert host_occluded(S, rays[:n]).tobytes() == ref[:n].tobytes()
    for k in (0, 77, 1000, 1999):
        assert host_occluded(S, rays[k:k + 1])[0] == ref[k]
    perm = np.random.default_rng(1).permutation(len(rays))
    assert host_occluded(S, rays[perm]).tobytes() == ref[perm].tobytes()
    assert len(host_occluded(S, rays[:0])) == 0


# ---------------------------------------------------------------- rt_segment_ray
def test_segment_ray_is_the_stated_expression_bit_for_bit():
    rng = np.random.default_rng(8)
    a = rng.normal(size=(50, 3)) * 10.0 ** rng.integers(-3, 6, (50, 1))
    b = rng.normal(size=(50, 3)) * 10.0 ** rng.integers(-3, 6, (50, 1))
    r = segment_ray(a, b, 0.625)
    assert r.dtype == RAY_DTYPE and r.shape == (50,)
    assert r["origin"].tobytes() == a.tobytes()
    assert r["direction"].tobytes() == (b - a).tobytes()
    assert (r["time"] == 0.625).all() and (r["t_max"] == 0.999).all()
    one = segment_ray([1.0, 2.0, 3.0], [1.5, 2.0, -3.0])
    assert one.shape == (1,) and one["direction"][0].tolist() == [0.5, 0.0, -6.0] and one["time"][0] == 0.0
    with pytest.raises(ValueError):
        segment_ray(np.zeros((3, 3)), np.zeros((2, 3)))
    # a == b: a zero direction, unoccluded; non-finite input goes through and is caught by the same rule
    S = cloud_scene()
    p = np.array([[0.0, 0.5, 0.0], [1.0, 1.0, 1.0]])
    same = segment_ray(p, p)
    assert (same["direction"] == 0.0).all() and not host_occluded(S, same).any()
    q = np.array([[np.nan, 0.0, 0.0], [0.0, INF, 0.0]])
    bad = segment_ray(q, p)
    assert np.isnan(bad["origin"][0, 0]) and np.isnan(bad["direction"][0, 0]) and bad["origin"][1, 1] == INF
    assert not host_occluded(S, bad).any()
    assert not host_occluded(S, segment_ray(p, p, time=np.nan)).any()
    L = load()
    v = (C.c_double * 3)(0.0, 0.0, 0.0)
    assert L.rt_segment_ray(None, v, 0.0, C.byref(abi.Ray())) == abi.RT_ERR_INVALID
    assert L.rt_segment_ray(v, None, 0.0, C.byref(abi.Ray())) == abi.RT_ERR_INVALID
    assert L.rt_segment_ray(v, v, 0.0, None) == abi.RT_ERR_INVALID
    assert b"null" in L.rt_last_error()


def test_segments_across_a_sphere():
    """Through the sphere: blocked; past it: visible; ending on its surface
    from outside: visible (0.999 stops short of it); starting on it: visible."""
    S = load_scene({"camera": {"lookfrom": [0.0, 0.0, 5.0], "lookat": [0.0, 0.0, 0.0], "vfov": 40.0},
                    "world": [{"type": "sphere", "center": [0.0, 0.0, 0.0], "radius": 1.0,
                               "material": {"type": "lambertian", "albedo": [0.5, 0.5, 0.5]}}]})
    a = np.array([[-3.0, 0.0, 0.0], [-3.0, 2.0, 0.0], [-3.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-3.0, 0.0, 0.0]])
    b = np.array([[3.0, 0.0, 0.0], [3.0, 2.0, 0.0], [-1.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    rays = segment_ray(a, b)
    got = host_occluded(S, rays)
    assert got.tolist() == [1, 0, 0, 0, 1]
    assert got.tobytes() == verdicts(host_trace(S, rays)).tobytes()


def test_visible_negates_occluded_over_segment_rays():
    """Renderer.visible is ~occluded(segment_ray(a, b, time)): checked on a
    stand-in that records what occluded is given (the device side is
    tests/test_occlusion_gpu.py's)."""
    from rtx.render import Renderer
    S = cloud_scene()
    rng = np.random.default_rng(4)
    a, b = rng.uniform(-6, 6, (40, 3)) + [0, 6, 0], rng.uniform(-6, 6, (40, 3)) + [0, 6, 0]
    seen = []

    class Stand(Renderer):
        def __init__(self):
            self.handle = None

        def occluded(self, rays):
            seen.append(ray_array(rays).copy())
            return host_occluded(S, rays).astype(np.bool_)

    vis = Stand().visible(a, b, time=0.25)
    assert len(seen) == 1 and seen[0].tobytes() == segment_ray(a, b, 0.25).tobytes()
    assert vis.dtype == np.bool_ and np.array_equal(vis, host_occluded(S, seen[0]) == 0)
    assert vis.any() and not vis.all()


# ---------------------------------------------------------------- ABI
def test_struct_sizes_exports_and_argtypes():
    assert C.sizeof(abi.Ray) == 64 == RAY_DTYPE.itemsize and np.dtype(np.bool_).itemsize == 1
    names = ("rt_occluded_device", "rt_occluded", "rt_multi_occluded", "rt_segment_ray")
    raw = C.CDLL(LIB_PATH)
    hdr = open(os.path.join(O.ROOT, "include", "rt_api.h")).read()
    for name in names:
        assert hasattr(raw, name) and name in abi.EXPORTS and ("int %s(" % name) in hdr
    L = load()
    assert L.rt_occluded_device.argtypes == [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.rt_occluded.argtypes == [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    assert L.rt_multi_occluded.argtypes == [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    assert L.rt_segment_ray.argtypes == [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.POINTER(abi.Ray)]
    for name in names:
        assert getattr(L, name).restype == C.c_int
    assert L.rt_abi_version() == 5


def test_refusals_need_no_device():
    """What is refused before anything is queued is refused before the scene
    is looked at: RT_ERR_INVALID with a message, on a machine without a GPU too."""
    L = load()
    rays = cloud_rays(n=4)
    out = np.full(4, SENTINEL, dtype=np.uint8)
    rp, op = C.c_void_p(rays.ctypes.data), C.c_void_p(out.ctypes.data)
    cases = [(-1, rp, op, b"negative"), (4, None, op, b"null ray or hit"), (4, rp, None, b"null ray or hit"),
             (4, rp, op, b"null scene"), (0, None, None, b"null scene"), (2 ** 36 + 1, rp, op, b"2^36")]
    for n, r, o, msg in cases:
        for call in (lambda: L.rt_occluded(None, n, r, o), lambda: L.rt_multi_occluded(None, n, r, o),
                     lambda: L.rt_occluded_device(None, n, r, o, None)):
            assert call() == abi.RT_ERR_INVALID, (n, msg)
            assert msg in L.rt_last_error(), (n, msg, L.rt_last_error())
    assert (out == SENTINEL).all()


def test_without_a_device_an_occlusion_scene_fails_like_every_other():
    from rtx.lib import RtError, device_count
    from rtx.render import Renderer
    if device_count() > 0:  # a device is present: the entry point runs (tests/test_occlusion_gpu.py has the rest)
        with Renderer(cloud_scene()) as R:
            assert len(R.occluded(cloud_rays(n=0))) == 0
        return
    with pytest.raises(RtError) as e:
        Renderer(cloud_scene())
    assert e.value.code == abi.RT_ERR_DEVICE
