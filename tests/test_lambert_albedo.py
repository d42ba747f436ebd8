"""The albedo as a Lambertian hit's weight (rt_path.h RT_LAMBERT_ALBEDO_F), host half.

In a world without lights the weight of a Lambertian event is spdf / pdf * att
= att * (cn / cw), cn = dot(h.n, gd), cw = dot(gd, unitv(h.n)), up to a few
roundings.  The plain flat instances take att itself where cw >= 2^-20 and
|cn - cw| <= 2^-43 cw, and run the general form otherwise.  Checked here,
without a GPU:

 * event by event (tests/native/rt_lambert_emu.cpp: the product's
   shade<false, F_FLAT, M_DIFFUSE> and <..., M_ANY> beside the general form,
   the plain BVH instance's shade), 100 k seeded events with the normals
   sphere_record forms, inv_r * (p - c), on spheres of radius 0.5 and 100:
   every event takes the albedo (T * att bit for bit), its direction is the
   general form's bits, and |T_new / T_general - 1| <= 2^-43;
 * normals the guard must refuse -- scaled by 1 +- 2^-30 and 1 +- 2^-42, NaN,
   zero, infinite -- give the general form's bits, NaN masks included; normals
   scaled by 1 +- 2^-46 give T * att; a NaN or infinite T or att gives the
   general form's NaN mask;
 * exact accounting in the host emulator: worlds of 1, 3 and 7 spheres with
   albedos 1, 0.5, 0.25 and the background (3, 1, 2) * 2^14 at depth 8, where
   every sample is an integer and every sum exact in any order.  The frame
   equals round(oracle) bit for bit; a lane that kept the general form's
   rounded weight, was weighted twice or took another lane's albedo gives a
   non-integer or another sum.  tests/test_lambert_albedo_gpu.py runs the same
   worlds on the GPU;
 * tight parity: spheres(3) at 24x16 and 1, 4 and 16 strata within 1e-12 of the
   oracle (DESIGN.md section 5's host bar; eight events at 2^-43 each stay
   under it by construction).
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from rtx import abi
from rtx.render import camera_frame
from rtx.scene import load_scene
import oracle_lib as O
from test_flat_static import NATIVE, emu  # noqa: F401
from test_flat_table import spheres

SEED = 31
SIZES = {"24x16": (24, 16), "20x12": (20, 12)}
N_EVENTS = 100000
BOUND = 2.0 ** -43


# ---- shade, event by event
@pytest.fixture(scope="module")
def twin():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "lambert.mk"], check=True)
    L = C.CDLL(os.path.join(NATIVE, "build", "liblambert_emu.so"))
    L.lambert_events.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_uint64, C.c_void_p]
    L.lambert_events.restype = C.c_int

    def run(p, nrm, T, att, seed=7):
        n = len(p)
        a = [np.ascontiguousarray(np.broadcast_to(x, (n, 3)), dtype=np.float64) for x in (p, nrm, T, att)]
        out = np.zeros((n, 3, 8))
        assert L.lambert_events(n, *(x.ctypes.data for x in a), seed, out.ctypes.data) == 0
        # per form: T after, the next direction, continues, bounce after
        return out
    return run


@functools.lru_cache(maxsize=None)
def events():
    """Hit points and sphere_record's normals on spheres of radius 0.5 and 100, throughputs and albedos."""
    g = np.random.default_rng(20240531)
    d = g.standard_normal((N_EVENTS, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    big = (np.arange(N_EVENTS) & 1).astype(bool)[:, None]
    r = np.where(big, 100.0, 0.5)
    c = np.where(big, np.array([0.0, -100.5, -1.0]), np.array([-1.0, 0.0, -1.0]))
    p = c + r * d
    n = (1.0 / r) * (p - c)
    T = 0.25 + g.random((N_EVENTS, 3))
    att = 0.05 + 0.9 * g.random((N_EVENTS, 3))
    for a in (p, n, T, att):
        a.setflags(write=False)
    return p, n, T, att


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_unit_normals_take_the_albedo(twin):
    p, n, T, att = events()
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-15
    out = twin(p, n, T, att)
    gen = out[:, 2]
    assert (gen[:, 6] == 1).all() and np.isfinite(gen).all()
    for f in (0, 1):  # the diffuse and the general flat instance
        new = out[:, f]
        assert np.array_equal(bits(new[:, :3]), bits(T * att))         # the albedo path, every event
        assert np.array_equal(bits(new[:, 3:]), bits(gen[:, 3:]))      # direction, continues, bounce
        dev = np.abs(new[:, :3] / gen[:, :3] - 1)
        print("form %d: max |T_new / T_general - 1| = %.3g (2^-43 = %.3g)" % (f, dev.max(), BOUND))
        assert dev.max() <= BOUND
    # the general form is not the albedo: the test above would pass emptily otherwise
    assert not np.array_equal(bits(gen[:, :3]), bits(T * att))


@pytest.mark.parametrize("scale", [1 + 2.0 ** -30, 1 - 2.0 ** -30, 1 + 2.0 ** -42, 1 - 2.0 ** -42,
                                   np.nan, 0.0, np.inf], ids=["1+2^-30", "1-2^-30", "1+2^-42", "1-2^-42", "nan", "zero", "inf"])
def test_refused_normals_keep_the_general_form(twin, scale):
    p, n, T, att = events()
    with np.errstate(invalid="ignore"):
        nrm = np.copysign(np.inf, n) if np.isinf(scale) else scale * n
    out = twin(p, nrm, T, att)
    for f in (0, 1):
        assert np.array_equal(bits(out[:, f]), bits(out[:, 2]))
    if np.isfinite(scale) and scale != 0:  # ... and that form is not the albedo
        assert not np.array_equal(bits(out[:, 2, :3]), bits(T * att))


@pytest.mark.parametrize("scale", [1 + 2.0 ** -46, 1 - 2.0 ** -46], ids=["1+2^-46", "1-2^-46"])
def test_nearly_unit_normals_take_the_albedo(twin, scale):
    p, n, T, att = events()
    out = twin(p, scale * n, T, att)
    for f in (0, 1):
        assert np.array_equal(bits(out[:, f, :3]), bits(T * att))
        assert np.array_equal(bits(out[:, f, 3:]), bits(out[:, 2, 3:]))


@pytest.mark.parametrize("what", ["T", "att"])
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_non_finite_throughput_and_albedo_keep_the_nan_mask(twin, what, value):
    p, n, T, att = events()
    T, att = T.copy(), att.copy()
    bad = T if what == "T" else att
    k = np.arange(N_EVENTS)
    bad[k, k % 3] = value  # one channel per event
    bad[::5] = value       # ... and whole events
    with np.errstate(invalid="ignore"):
        out = twin(p, n, T, att)
    gen = out[:, 2]
    assert np.isnan(gen[:, :3]).any() or np.isinf(gen[:, :3]).any()
    for f in (0, 1):
        assert np.array_equal(np.isnan(out[:, f]), np.isnan(gen))
        assert np.array_equal(np.isinf(out[:, f]), np.isinf(gen))
        assert np.array_equal(bits(out[:, f, 3:]), bits(gen[:, 3:]))


# ---- whole frames: exact accounting and tight parity (the GPU half imports these)
ALBEDO = {"ground": [1.0, 0.5, 0.25], "center": [0.5, 0.25, 1.0], "left": [0.25, 1.0, 0.5]}
BACKGROUND = [3.0 * 2 ** 14, 1.0 * 2 ** 14, 2.0 * 2 ** 14]


def exact_world(n):
    """spheres(n) with power-of-two albedos and background: at depth 8 every sample is an integer."""
    d = spheres(n)
    for name, a in ALBEDO.items():
        d["materials"][name] = {"type": "lambertian", "albedo": a}
    d["camera"]["background"] = BACKGROUND
    return d


def with_unused_metal(S):
    S.add_material(abi.RT_MAT_METAL, albedo=(0.8, 0.6, 0.2), fuzz=0.25)
    return S


def frame_of(S, size, spp):
    w, h = SIZES[size]
    cam = S.camera_desc(image_width=w, aspect_ratio=w / (h + 0.5), samples_per_pixel=spp, max_depth=8)
    f = camera_frame(cam)
    assert (f.image_width, f.image_height) == (w, h) and f.sqrt_spp ** 2 == spp
    return cam, f


@functools.lru_cache(maxsize=None)
def exact_reference(n, size):
    """round(oracle COUNTER frame of sums), after the oracle is shown to be that close to integers."""
    S = load_scene(exact_world(n))
    cam, _ = frame_of(S, size, 16)
    ref = O.oracle_render(S, cam, O.MODE_COUNTER, SEED, output=abi.RT_OUT_SUM)
    want = np.round(ref)
    print("oracle: max |sum - round(sum)| = %.3g, max sum %g" % (np.abs(ref - want).max(), want.max()))
    assert np.abs(ref - want).max() <= 1e-3
    assert want.max() > 0 and (want == 0).sum() < want.size
    want.setflags(write=False)
    return want


def emu_render(L, S, f, spp_output, seed=SEED):
    desc = S.desc()
    p = abi.RenderParams()
    p.seed, p.sample_count, p.output = seed, -1, spp_output
    out = np.zeros((f.image_height, f.image_width, 3))
    assert L.emu_render(C.byref(desc), C.byref(f), C.byref(p), 0, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return out


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("n", [1, 3, 7])
def test_emulator_exact_accounting(emu, n, size):  # noqa: F811
    want = exact_reference(n, size)
    for S in (load_scene(exact_world(n)), with_unused_metal(load_scene(exact_world(n)))):
        _, f = frame_of(S, size, 16)
        got = emu_render(emu, S, f, abi.RT_OUT_SUM)
        off = got != want
        print("emulator: %d of %d sums differ from round(oracle), max |diff| %g" % (off.sum(), off.size, np.abs(got - want).max()))
        assert np.array_equal(got, want)


# ---- both forms in one wave: small far spheres beside a near one
SILHOUETTE = np.degrees(np.arcsin(0.5 / 1.2))  # of three_spheres' centre sphere, seen from the origin
PIXEL = 1.0 / 24                                # degrees per pixel: vfov 1 degree over 24 rows
AIM = SILHOUETTE + 4 * PIXEL                    # the silhouette runs down pixel column 12 of 32
PEBBLES = [(12.8, 9.3), (13.9, 11.2), (14.6, 13.4), (13.2, 14.1)]  # (column, row): all in tile (1, 1)


def pebble_world(extra=None, exact=False):
    """three_spheres seen through a 1-degree lens along the centre sphere's
    right edge, with four pebbles of radius 0.01 at distance 20 just beyond
    that edge: the near sphere's normals pass the guard, the pebbles' mostly do
    not (|oc|^2 - rr rounds at 400 for rr = 1e-4), and both lie in the same
    8x8 tile.  extra: "sphere0" a zero-radius sphere, "quad0" a zero-area quad."""
    d = exact_world(3) if exact else spheres(3)
    az, el = np.radians(AIM), 0.0
    d["camera"].update(vfov=1.0, lookfrom=[0, 0, 0], lookat=[float(np.sin(az)), el, float(-np.cos(az))])
    for k, (col, row) in enumerate(PEBBLES):
        a, e = np.radians(AIM + (col - 16) * PIXEL), np.radians((12 - row) * PIXEL)
        c = 20 * np.array([np.sin(a) * np.cos(e), np.sin(e), -np.cos(a) * np.cos(e)])
        d["world"].append({"type": "sphere", "center": [float(x) for x in c], "radius": 0.01,
                           "material": ("left", "center")[k & 1]})
    if extra == "sphere0":
        d["world"].append({"type": "sphere", "center": [0.6, 0.1, -1.0], "radius": 0, "material": "left"})
    elif extra == "quad0":
        d["world"].append({"type": "quad", "Q": [0.6, 0.1, -1.0], "u": [0, 0, 0], "v": [0, 1, 0], "material": "left"})
    assert len(d["world"]) <= 8 and not d.get("use_bvh", False)
    return d


def pebble_frame(S, spp=16):
    cam = S.camera_desc(image_width=32, aspect_ratio=32 / 24.5, samples_per_pixel=spp, max_depth=8)
    f = camera_frame(cam)
    assert (f.image_width, f.image_height) == (32, 24)
    return cam, f


def test_emulator_pebble_world_runs_both_forms(emu):  # noqa: F811
    """With power-of-two albedos a sum is an integer unless one of its events
    kept the general form's rounded weight: the near sphere's columns are all
    integers, some pixel of the pebbles' tile is not."""
    S = load_scene(pebble_world(exact=True))
    _, f = pebble_frame(S)
    got = emu_render(emu, S, f, abi.RT_OUT_SUM)
    frac = got != np.round(got)
    print("non-integer sums: %d, in columns %s" % (frac.sum(), sorted(set(np.nonzero(frac)[1]))))
    assert frac.any() and np.isfinite(got).all()


@pytest.mark.parametrize("extra", [None, "sphere0", "quad0"])
def test_emulator_pebble_world_matches_oracle(emu, extra):  # noqa: F811
    S = load_scene(pebble_world(extra))
    cam, f = pebble_frame(S)
    got = emu_render(emu, S, f, abi.RT_OUT_SCALED)
    ref = O.oracle_render(S, cam, O.MODE_COUNTER, SEED)
    d = np.abs(np.nan_to_num(got) - np.nan_to_num(ref))
    print("emulator vs oracle: max |diff| = %.3g" % d.max())
    assert d.max() <= 1e-10 and np.array_equal(np.isnan(got), np.isnan(ref))  # tests/test_emulator.py's host bound


@pytest.mark.parametrize("spp", [1, 4, 16])
def test_emulator_tight_parity(emu, spp):  # noqa: F811
    S = load_scene(spheres(3))
    cam, f = frame_of(S, "24x16", spp)
    got = emu_render(emu, S, f, abi.RT_OUT_SCALED)
    ref = O.oracle_render(S, cam, O.MODE_COUNTER, SEED)
    d = np.abs(got - ref)
    print("emulator vs oracle, %d strata: max |diff| = %.3g" % (spp, d.max()))
    assert np.isfinite(got).all() and d.max() <= 1e-12
