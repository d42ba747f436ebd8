"""The Lambertian-only flat instance's basis without its exact zeros (rt_path.h
onb_axis_gd, RT_ONB_AXIS_MS), host half.

The general form builds ONB(n) from cross products with a = (1,0,0) or (0,1,0)
and carries the resulting exact zeros through a squared length, a scale, a
second cross product and the direction's sums; the reduced form drops those
terms.  tests/native/rt_onb_emu.cpp runs the product's shade<false, F_FLAT,
M_DIFFUSE> beside the general form, shade<false, F_FLAT, M_ANY>, event by
event, and the two forms of the basis alone on given draws.  Checked here,
without a GPU:

 * 200 k seeded normals as sphere_record forms them, inv_r * (p - c), radius
   0.5 and 100: the direction, the weight, the return and the bounce count are
   equal as values, with equal NaN and infinity masks; at least 99 % take the
   reduced form (the count is printed).  The same normals scaled by 1 +- 2^-30
   fail the albedo guard and fall to the general weight: equal again;
 * |w.x| at 0.9 and one ulp either side, both signs; axis normals and normals
   with one or two exactly zero components of either sign; each over the draws
   d0, d1 in {0, 2^-32, 0.25, 0.5, 1 - 2^-32};
 * zero, NaN and infinite normals take the general branch and give its bits.

Bits may differ in the sign of a zero only: where they differ, both values are
zero.
"""
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

NATIVE = os.path.join(os.path.dirname(__file__), "native")
N_EVENTS = 200000
EXTREMES = [0.0, 2.0 ** -32, 0.25, 0.5, 1 - 2.0 ** -32]


@pytest.fixture(scope="module")
def twin():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "onb.mk", "build/libonb_emu.so"], check=True)
    L = C.CDLL(os.path.join(NATIVE, "build", "libonb_emu.so"))
    L.onb_events.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_uint64, C.c_void_p, C.c_void_p]
    L.onb_events.restype = C.c_int
    L.onb_dirs.argtypes = [C.c_int] + [C.c_void_p] * 4
    L.onb_dirs.restype = C.c_int
    return L


def run_events(L, p, nrm, T, att, seed=7):
    n = len(p)
    a = [np.ascontiguousarray(np.broadcast_to(x, (n, 3)), dtype=np.float64) for x in (p, nrm, T, att)]
    out, fast = np.zeros((n, 2, 8)), np.zeros(n, np.int32)
    taken = L.onb_events(n, *(x.ctypes.data for x in a), seed, out.ctypes.data, fast.ctypes.data)
    assert taken == fast.sum()
    return out, fast.astype(bool)  # per form: T after, the next direction, continues, bounce after


def run_dirs(L, nrm, d):
    nrm, d = np.ascontiguousarray(nrm, np.float64), np.ascontiguousarray(d, np.float64)
    n = len(nrm)
    assert nrm.shape == (n, 3) and d.shape == (n, 2)
    out, fast = np.zeros((n, 2, 8)), np.zeros(n, np.int32)
    taken = L.onb_dirs(n, nrm.ctypes.data, d.ctypes.data, out.ctypes.data, fast.ctypes.data)
    assert taken == fast.sum()
    return out, fast.astype(bool)  # per form: w, gd, the albedo guard's verdict, 0


@functools.lru_cache(maxsize=None)
def events():
    """Hit points and sphere_record's normals on spheres of radius 0.5 and 100, throughputs and albedos."""
    g = np.random.default_rng(20240607)
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


def assert_equal_values(new, gen):
    """== with the same NaN and infinity masks; bits differ only between two zeros."""
    assert np.array_equal(np.isnan(new), np.isnan(gen))
    assert np.array_equal(np.isinf(new), np.isinf(gen))
    assert np.array_equal(new, gen, equal_nan=True)
    off = bits(new) != bits(gen)
    off &= ~np.isnan(new)
    print("values whose bits differ: %d of %d" % (off.sum(), off.size))
    assert (new[off] == 0).all() and (gen[off] == 0).all()


def test_sphere_normals_take_the_reduced_form_with_equal_values(twin):
    p, n, T, att = events()
    out, fast = run_events(twin, p, n, T, att)
    print("reduced form: %d of %d seeded sphere normals" % (fast.sum(), len(fast)))
    assert fast.sum() >= 0.99 * len(fast)
    new, gen = out[:, 0], out[:, 1]
    assert (gen[:, 6] == 1).all() and np.isfinite(gen).all()
    assert np.array_equal(bits(gen[:, :3]), bits(T * att))  # these events take the albedo form ...
    assert np.abs(np.linalg.norm(gen[:, 3:6], axis=1)).min() > 0.1  # ... and have a direction to compare
    assert_equal_values(new, gen)


@pytest.mark.parametrize("scale", [1 + 2.0 ** -30, 1 - 2.0 ** -30], ids=["1+2^-30", "1-2^-30"])
def test_events_that_fall_to_the_general_weight(twin, scale):
    p, n, T, att = events()
    out, fast = run_events(twin, p, scale * n, T, att)
    assert fast.all()
    new, gen = out[:, 0], out[:, 1]
    assert not np.array_equal(bits(gen[:, :3]), bits(T * att))  # the guard refused: the general weight
    assert_equal_values(new, gen)


@pytest.mark.parametrize("scale", [0.0, np.nan, np.inf], ids=["zero", "nan", "inf"])
def test_refused_normals_take_the_general_branch_bit_for_bit(twin, scale):
    p, n, T, att = events()
    k = 20000
    with np.errstate(invalid="ignore"):
        nrm = np.copysign(np.inf, n[:k]) if np.isinf(scale) else scale * n[:k]
        nrm = np.concatenate([nrm, np.where(np.arange(k)[:, None] % 3 == np.arange(3), scale, n[:k])])  # one component
    if scale == 0.0:
        nrm = nrm[:k]  # one zero component is an ordinary normal: below
    out, fast = run_events(twin, np.concatenate([p[:k]] * 2)[:len(nrm)], nrm, T[:1], att[:1])
    assert not fast.any()
    assert np.array_equal(bits(out[:, 0]), bits(out[:, 1]))
    lc = np.tile(np.array(list(itertools.product(EXTREMES, EXTREMES))), (len(nrm) // 25 + 1, 1))[:len(nrm)]
    out, fast = run_dirs(twin, nrm, lc)
    assert not fast.any()
    assert np.array_equal(bits(out[:, 0]), bits(out[:, 1]))


def edge_normals():
    """|w.x| about 0.9, axis normals, one or two exact zeros of either sign; unit and as a radius-0.5 record."""
    x9 = [np.nextafter(0.9, 0), 0.9, np.nextafter(0.9, 1)]
    out = []
    for x in x9:
        rest = np.sqrt(1 - x * x)
        for sx, t in itertools.product((1, -1), (0.0, 0.3, 1.0, 2.2, np.pi, 4.0)):
            out.append([sx * x, rest * np.cos(t), rest * np.sin(t)])
    z = [0.0, -0.0]
    for a in range(3):  # axis normals: two exact zeros
        for s, z1, z2 in itertools.product((1.0, -1.0), z, z):
            v = [z1, z2]
            v.insert(a, s)
            out.append(v)
    for a in range(3):  # one exact zero
        for zz, t in itertools.product(z, (0.2, 0.45, 1.0, 2.0, 2.7, 3.5, 4.4, 5.9)):
            v = [np.cos(t), np.sin(t)]
            v.insert(a, zz)
            out.append(v)
    out = np.array(out)
    return np.concatenate([out, out * (1 + 2.0 ** -52), out * (1 - 2.0 ** -53), 0.5 * out, 3.0 * out])


def test_axis_threshold_and_exact_zeros_over_the_extreme_draws(twin):
    nrm = edge_normals()
    d = np.array(list(itertools.product(EXTREMES, EXTREMES)))
    nn = np.repeat(nrm, len(d), axis=0)
    dd = np.tile(d, (len(nrm), 1))
    out, fast = run_dirs(twin, nn, dd)
    print("reduced form: %d of %d edge events" % (fast.sum(), len(fast)))
    assert fast.all()
    new, gen = out[:, 0], out[:, 1]
    assert np.isfinite(gen).all()
    big = np.abs(gen[:, 0]) > 0.9
    assert big.any() and (~big).any()  # both axes
    assert (gen[:, 6] == 1).any() and (gen[:, 6] == 0).any()  # the albedo form and the general weight
    assert_equal_values(new, gen)
    # ... and through shade, with its own draws
    p = np.array([-1.0, 0.0, -1.0]) + 0.5 * nrm
    out, fast = run_events(twin, p, nrm, np.array([0.5, 1.0, 0.75]), np.array([0.5, 0.25, 0.8]))
    assert fast.all()
    assert_equal_values(out[:, 0], out[:, 1])


def test_seeded_normals_over_seeded_draws(twin):
    _, n, _, _ = events()
    g = np.random.default_rng(5)
    d = g.integers(0, 2 ** 32, (N_EVENTS, 2)).astype(np.float64) * 2.0 ** -32
    out, fast = run_dirs(twin, n, d)
    assert fast.all()
    assert_equal_values(out[:, 0], out[:, 1])
