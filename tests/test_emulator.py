"""The kernel's own per-path source (csrc/rt_path.h), compiled for the HOST by
g++ (tests/native, test-only), against the oracle's counter mode — for every
kernel feature instance.  Runs without a GPU; a failure here is a logic error
in the kernel source, while a GPU-only failure (tests/test_gpu_instances.py)
points at gfx950 code generation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rtx import abi
from rtx.render import camera_frame
from rtx.scene import load_scene
import oracle_lib as O
import slab_cases as SC
from test_gpu_instances import feature_scene

NATIVE = os.path.join(os.path.dirname(__file__), "native")


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-C", NATIVE], check=True)
    L = C.CDLL(os.environ.get("RTX_EMU_LIB", os.path.join(NATIVE, "build", "libemu.so")))
    L.emu_render.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.Frame),
                             C.POINTER(abi.RenderParams), C.c_int, C.POINTER(C.c_double)]
    return L


@pytest.mark.parametrize("F", list(range(32)))
def test_kernel_source_on_host_matches_oracle(emu, F):
    """F >= 16: the flat instances' host build (the emulator adds FLAT itself
    for a world whose root is one leaf, so F & 15 is passed)."""
    S = load_scene(feature_scene(F))
    d = S.desc()
    cam = S.camera_desc(image_width=32, samples_per_pixel=9, max_depth=8)
    f = camera_frame(cam)
    p = abi.RenderParams()
    p.seed, p.sample_count, p.output = 77, -1, abi.RT_OUT_SCALED
    out = np.zeros((f.image_height, f.image_width, 3))
    assert emu.emu_render(C.byref(d), C.byref(f), C.byref(p), F & 15,
                          out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    ref = O.oracle_render(S, cam, O.MODE_COUNTER, 77)
    assert np.array_equal(np.isnan(out), np.isnan(ref))
    # 1e-10: the kernel's sincos_2pi is within 1.4e-16 of sin/cos(2 pi u) while the
    # oracle calls libm on fl(2 pi u) (up to 4.4e-16 apart); bounces amplify that
    # to ~1e-12 on bright pixels.  Still eight orders below the GPU parity bar (1e-4).
    np.testing.assert_allclose(np.nan_to_num(out), np.nan_to_num(ref), rtol=0, atol=1e-10)


@pytest.mark.parametrize("F", list(range(16)))
def test_kernel_source_bvh4_walk_matches_oracle(emu, F):
    """The 4-wide walk (F_BVH4, rt_path.h trace) over the collapsed tree
    (rt_scene.cpp collapse_bvh4) against the oracle, for every feature set of
    a non-flat world."""
    S = load_scene(feature_scene(F))
    d = S.desc()
    cam = S.camera_desc(image_width=32, samples_per_pixel=9, max_depth=8)
    f = camera_frame(cam)
    p = abi.RenderParams()
    p.seed, p.sample_count, p.output = 78, -1, abi.RT_OUT_SCALED
    out = np.zeros((f.image_height, f.image_width, 3))
    assert emu.emu_render(C.byref(d), C.byref(f), C.byref(p), F | abi.RT_FEAT_BVH4,
                          out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    ref = O.oracle_render(S, cam, O.MODE_COUNTER, 78)
    assert np.array_equal(np.isnan(out), np.isnan(ref))
    np.testing.assert_allclose(np.nan_to_num(out), np.nan_to_num(ref), rtol=0, atol=1e-10)


def random_spheres(n, seed=3):
    """A world of n small random spheres in a box, plus a ground quad."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-50, 50, size=(n, 3))
    r = rng.uniform(0.2, 1.5, size=n)
    world = [{"type": "sphere", "center": list(map(float, c[i])), "radius": float(r[i]),
              "material": ["m0", "m1", "m2"][i % 3]} for i in range(n)]
    world.append({"type": "quad", "Q": [-80, -60, -80], "u": [160, 0, 0], "v": [0, 0, 160],
                  "material": "m0"})
    return {"materials": {"m0": {"type": "lambertian", "albedo": [0.7, 0.6, 0.5]},
                          "m1": {"type": "metal", "albedo": [0.8, 0.8, 0.9], "fuzz": 0.1},
                          "m2": {"type": "dielectric", "refraction_index": 1.5}},
            "world": world, "lights": [],
            "camera": {"aspect_ratio": 1.0, "image_width": 24, "samples_per_pixel": 4,
                       "max_depth": 6, "vfov": 40, "lookfrom": [0, 20, 140],
                       "lookat": [0, 0, 0], "vup": [0, 1, 0], "defocus_angle": 0,
                       "focus_dist": 10, "background": [0.7, 0.8, 1.0]}}


@pytest.mark.parametrize("n", [9, 40, 3000])
def test_bvh4_collapse_structure(emu, n):
    """collapse_bvh4: the 4-wide tree has the binary tree's leaves in the same
    depth-first order, child boxes taken from the binary tree, BFS (forward)
    inner entries, about half the levels and at most one node per binary node.
    Measured: 3000 spheres -> 1786 binary nodes, 898 4-wide (2.99 of 4 slots
    used), 13 -> 7 levels."""
    S = load_scene(random_spheres(n))
    d = S.desc()
    info = (C.c_longlong * 10)()
    emu.emu_bvh4_info.argtypes = [C.c_void_p, C.c_void_p]
    assert emu.emu_bvh4_info(C.addressof(d), info) == 0
    nb, n4, db, d4, lb, l4, same, foreign, empty, fwd = list(info)
    assert same == 1 and lb == l4 and foreign == 0 and fwd == 1
    assert n4 <= nb and d4 <= (db + 2) // 2 + 1
    if n >= 1000:  # about half the nodes; ~3 of 4 slots used (leaves cap the fill)
        assert n4 < 0.55 * nb and empty < 0.3 * 4 * n4


def test_bvh4_walk_equals_binary_walk(emu):
    """On a 3000-sphere world the 4-wide walk renders the binary walk's image
    (the closest hit does not depend on the visiting order; 1e-12 allows for an
    exact tie between two surfaces being resolved the other way round)."""
    S = load_scene(random_spheres(3000))
    d = S.desc()
    cam = S.camera_desc(image_width=24, samples_per_pixel=4, max_depth=6)
    f = camera_frame(cam)
    p = abi.RenderParams()
    p.seed, p.sample_count, p.output = 5, -1, abi.RT_OUT_SCALED
    a = np.zeros((f.image_height, f.image_width, 3))
    b = np.zeros_like(a)
    P = C.POINTER(C.c_double)
    assert emu.emu_render(C.byref(d), C.byref(f), C.byref(p), 0, a.ctypes.data_as(P)) == 0
    assert emu.emu_render(C.byref(d), C.byref(f), C.byref(p), abi.RT_FEAT_BVH4, b.ctypes.data_as(P)) == 0
    assert a.sum() > 0
    np.testing.assert_allclose(b, a, rtol=0, atol=1e-12)


def test_sincos_2pi_accuracy(emu):
    """sincos_2pi (rt_path.h) against sin/cos(2 pi u) in long double, for u = k 2^-32
    (random k, both ends of the range, every quadrant boundary)."""
    rng = np.random.default_rng(5)
    k = np.concatenate([rng.integers(0, 2**32, size=200000), np.arange(4096), 2**32 - 1 - np.arange(4096),
                        np.arange(0, 2**32, 2**24),
                        (np.arange(1, 4)[:, None] * 2**30 + np.arange(-64, 64)[None, :]).ravel()])
    k = np.unique(k % 2**32)
    u = k.astype(np.float64) * 2.0**-32
    s, c = np.zeros_like(u), np.zeros_like(u)
    P = C.POINTER(C.c_double)
    emu.emu_sincos_2pi.argtypes = [P, C.c_int, P, P]
    emu.emu_sincos_2pi(u.ctypes.data_as(P), len(u), s.ctypes.data_as(P), c.ctypes.data_as(P))
    ang = 2 * np.longdouble("3.14159265358979323846264338327950288") * k.astype(np.longdouble) * np.longdouble(2.0)**-32
    assert float(np.abs(s - np.sin(ang)).max()) < 3e-16
    assert float(np.abs(c - np.cos(ang)).max()) < 3e-16
    assert np.all(np.abs(s) <= 1) and np.all(np.abs(c) <= 1)
    assert s[0] == 0.0 and c[0] == 1.0


def test_sin_n_within_one_ulp(emu):
    """sin_n (rt_path.h, NoiseTexture's sin: Cody-Waite reduction + fdlibm
    kernels below 2^20, the library sin beyond) against sin in long double:
    at most 1 ulp on random arguments over the noise texture's range and
    beyond, arguments next to multiples of pi/2 (hardest reductions), tiny,
    huge, signed zeros and non-finite values."""
    rng = np.random.default_rng(8)
    k = rng.integers(-600000, 600000, size=200000).astype(np.float64)
    near = (k * (np.pi / 2)).astype(np.float64)  # next to multiples of pi/2
    near = np.concatenate([near, np.nextafter(near, np.inf), np.nextafter(near, -np.inf)])
    x = np.concatenate([rng.uniform(-4000, 4000, 300000), rng.uniform(-2**20, 2**20, 100000),
                        rng.uniform(-1, 1, 50000), near,
                        np.exp2(rng.uniform(-1000, 19.99, 50000)) * rng.choice([-1, 1], 50000),
                        rng.uniform(2**20, 1e300, 2000), [0.0, -0.0, 2**20, -2**20, np.pi / 4,
                                                          np.inf, -np.inf, np.nan]])
    out = np.zeros_like(x)
    P = C.POINTER(C.c_double)
    emu.emu_sin_n.argtypes = [P, C.c_int, P]
    emu.emu_sin_n(x.ctypes.data_as(P), len(x), out.ctypes.data_as(P))
    fin = np.isfinite(x)
    assert np.all(np.isnan(out[~fin]))
    assert out[x == 0].tolist() == [0.0, -0.0] and np.signbit(out[x == 0]).tolist() == [False, True]
    want = np.sin(x[fin].astype(np.longdouble))
    ulp = np.spacing(np.abs(want.astype(np.float64)))
    err = np.abs(out[fin].astype(np.longdouble) - want) / ulp.astype(np.longdouble)
    assert float(err.max()) <= 1.0, (x[fin][np.argmax(err)], float(err.max()))
    assert np.all(np.abs(out[fin]) <= 1)


def test_div_mk_equals_division(emu):
    """div_mk (rt_path.h: x * RN(1/b) plus one FMA correction, used for the sphere
    roots and ct/pi) returns the IEEE division's double, bit for bit, on random
    operands over the kernel's range, divisors with all-ones / all-zeros
    significands, pi, and the ray-tracing magnitudes (|d|^2 ~ 1, roots ~ 1e-3..1e3)."""
    rng = np.random.default_rng(11)
    n = 400000

    def rand_f64(lo_exp, hi_exp, m):
        sig = rng.uniform(1.0, 2.0, size=m)
        return sig * np.exp2(rng.integers(lo_exp, hi_exp, size=m).astype(np.float64))

    x = rand_f64(-900, 900, n) * rng.choice([-1.0, 1.0], size=n)
    b = rand_f64(-90, 90, n)
    ones = np.nextafter(np.exp2(rng.integers(-60, 60, size=20000).astype(np.float64) + 1), 0)  # 1.111...1 x 2^e
    pows = np.exp2(rng.integers(-60, 60, size=20000).astype(np.float64))
    xb = rand_f64(-30, 30, 40000 + 20000) * rng.choice([-1.0, 1.0], size=60000)
    bb = np.concatenate([ones, pows, np.full(20000, np.pi)])
    x = np.concatenate([x, xb, rng.uniform(-1, 1, 100000)])
    b = np.concatenate([b, bb, np.full(100000, np.pi)])
    q = np.zeros_like(x)
    P = C.POINTER(C.c_double)
    emu.emu_div_mk.argtypes = [P, P, C.c_int, P]
    emu.emu_div_mk(x.ctypes.data_as(P), b.ctypes.data_as(P), len(x), q.ctypes.data_as(P))
    want = x / b
    bad = q.view(np.uint64) != want.view(np.uint64)
    assert not bad.any(), (x[bad][:4], b[bad][:4], q[bad][:4], want[bad][:4])


@pytest.fixture(scope="module")
def slab_cs():
    return SC.make_cases()


def test_slab_tests_are_conservative(emu, slab_cs):
    """Both fp32 slab forms of rt_path.h (subtract form: flat instances' medium cull;
    FMA form with absolute slack: BVH instances) pass every box that the exact
    slab test (long double) hits within the window — on the cases of
    tests/slab_cases.py, inside the domain stated there: random, grazing
    (origin on a face plane), axis-parallel, tiny-component, denormal and
    below-fp32 components, huge components, scaled directions, large-coordinate
    rays and finite closest-hit bounds around the exact interval.  Visiting
    more boxes is allowed; dropping one is not."""
    cs = slab_cs
    n = len(cs["kind"])
    hit = cs["hit"] & cs["domain"]
    out = np.zeros(n, dtype=np.int32)
    PD, PF = C.POINTER(C.c_double), C.POINTER(C.c_float)
    emu.emu_slab.argtypes = [PD, PD, PF, PF, PF, PF, C.c_int, C.POINTER(C.c_int)]
    emu.emu_slab(cs["o"].ctypes.data_as(PD), cs["d"].ctypes.data_as(PD), cs["lo"].ctypes.data_as(PF),
                 cs["hi"].ctypes.data_as(PF), cs["tmin"].ctypes.data_as(PF), cs["cl"].ctypes.data_as(PF), n,
                 out.ctypes.data_as(C.POINTER(C.c_int)))
    assert hit.sum() > n // 4                            # the cases do exercise hits
    for bit, form in ((1, "subtract"), (2, "fma")):
        dropped = hit & ((out & bit) == 0)
        assert not dropped.any(), "%s form dropped %d boxes, e.g. o=%s d=%s lo=%s hi=%s" % (
            form, dropped.sum(), cs["o"][dropped][0], cs["d"][dropped][0], cs["lo"][dropped][0],
            cs["hi"][dropped][0])
    # and they are not vacuous: most exact misses are culled
    assert ((out & 2) == 0)[cs["domain"] & ~cs["hit"]].mean() > 0.5


def test_every_slab_form_is_conservative_and_the_fma_family_agrees(emu, slab_cs):
    """Every box-test form the walks run (tests/native/slab_forms.h: slab<>,
    slab_hit, slab_hit2 on a DNode, slab2_planes on the staged DNodeL,
    slab_planes<2> and <4> through plane_offsets / load_planes, the box in every
    child slot) on the host build: none drops an exact hit inside the domain
    (pins kSlabGrow, the slack and the clamps), and the forms of the FMA family
    agree in verdict and entry-distance bits on every case -- rt_path.h's
    "min / max of the two plane distances ARE these picks, value for value"
    (pins the plane offsets, the DNodeL / DNode / DNode4 layouts and the
    near / far pick per sign).  tests/test_gpu_slab.py is the gfx950 twin."""
    verdict, tl = SC.run_forms(emu.emu_slab_forms, slab_cs)
    SC.check_forms(slab_cs, verdict, tl, "host")


def test_axis_aligned_quad_formulas_equal_full_formulas(emu):
    """quad_t_aa (rt_path.h: the axis-aligned quad's Plane::hit with the
    zero-product terms dropped) gives the full formulas' hit flag and t bit for
    bit: Cornell walls and the rotated box's faces (in their local frame), on
    random, grazing, axis-parallel, zero-component and non-finite rays, over
    the kernel's intervals [0.001, inf) and (-inf, inf) (medium boundary)."""
    import ctypes as C
    import json
    from rtx.scene import load_scene
    S = load_scene(os.path.join(O.ROOT, "real-time-ray-tracing-engine_amd", "scenes", "cornell.json"))
    d = S.desc()
    rng = np.random.default_rng(17)
    n = 300000
    o = rng.uniform(-100, 650, size=(n, 3))
    tgt = rng.uniform(0, 555, size=(n, 3))
    dirs = tgt - o
    k = rng.integers(0, 3, size=n)
    sel = rng.uniform(size=n)
    dirs[sel < 0.1, :] *= rng.uniform(-1, 1, size=(int((sel < 0.1).sum()), 1))
    zero = (sel >= 0.1) & (sel < 0.25)
    dirs[zero, k[zero]] = 0.0                                   # axis-parallel rays
    tiny = (sel >= 0.25) & (sel < 0.35)
    dirs[tiny, k[tiny]] = rng.choice([1e-9, -1e-9, 1e-300, 5e-324], size=int(tiny.sum()))
    onp = (sel >= 0.35) & (sel < 0.45)
    o[onp, 1] = 555.0                                           # origins on a wall plane
    bad = (sel >= 0.45) & (sel < 0.5)
    vals = np.array([np.inf, -np.inf, np.nan, 1e308])
    dirs[bad, k[bad]] = rng.choice(vals, size=int(bad.sum()))
    bado = (sel >= 0.5) & (sel < 0.53)
    o[bado, k[bado]] = rng.choice(vals, size=int(bado.sum()))
    o = np.ascontiguousarray(o)
    dirs = np.ascontiguousarray(dirs)
    P = C.POINTER(C.c_double)
    emu.emu_quad_forms.argtypes = [C.c_void_p, P, P, C.c_double, C.c_double, C.c_int, P,
                                   C.POINTER(C.c_int)]
    for tmin, tmax in ((0.001, np.inf), (-np.inf, np.inf)):
        out = np.zeros((n, 4))
        naa = C.c_int()
        assert emu.emu_quad_forms(C.addressof(d), o.ctypes.data_as(P), dirs.ctypes.data_as(P),
                                  tmin, tmax, n, out.ctypes.data_as(P), C.byref(naa)) == 0
        assert naa.value >= 12  # 6 walls/light + the box's 6 faces are all axis-aligned
        assert np.array_equal(out[:, 0], out[:, 2])
        assert np.array_equal(out[:, 1].view(np.uint64), out[:, 3].view(np.uint64))
        assert out[:, 0].sum() > 1000
