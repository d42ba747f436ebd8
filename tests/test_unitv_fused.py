"""unitv's one-transcendental form (csrc/rt_path.h unitv_fused: sqrt_h, rcp_h,
rcp_from_h) -- a measured variant (make EXTRA=-DRT_UNITV_FUSED=1), not what the
product build runs; kept buildable, and checked here.

The form takes the root of the squared length and its reciprocal from the one
v_rsq_f64 of sqrt_n: the reciprocal's seed is the h that the root's Goldschmidt
step leaves, followed by one Newton step, Markstein's correction, and a one-ulp
nudge of the remainder at the one exact tie (l with an all-ones significand).
It must give what sqrt_n followed by rcp_n gives, bit for bit, for every input.

 * GPU: tests/native/rt_unitv_devcheck.hip runs rcp_h(sqrt_h(x)) and
   rcp_n(sqrt_n(x)) (the root-then-reciprocal form that unitv runs) over arrays
   of squared lengths, and unitv_fused / unitv_2t over vectors; every output
   must be bit-equal (NaN equal to NaN), no case left out.
 * CPU: tests/native/rt_unitv_check.cpp, the same sequence compiled for the
   host with perturbed seeds against sqrt and division; it also shows that
   without the nudge the all-ones family fails, so the nudge cannot be removed
   unnoticed.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

NATIVE = os.path.join(os.path.dirname(__file__), "native")
LIB = os.path.join(NATIVE, "build", "libunitv_devcheck.so")
CHECK = os.path.join(NATIVE, "build", "rt_unitv_check")


# ---- host
def test_fused_sequence_on_the_host_and_the_nudge_is_needed():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "unitv.mk", "build/rt_unitv_check"], check=True)
    r = subprocess.run([CHECK, "500000"], stdout=subprocess.PIPE, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    m = re.search(r"cases (\d+) sqrt_bad (\d+) rcp_cases (\d+) rcp_bad (\d+)", r.stdout)
    cases, sqrt_bad, rcp_cases, rcp_bad = map(int, m.groups())
    assert cases > 4_000_000 and rcp_cases > 0.9 * cases and sqrt_bad == 0 and rcp_bad == 0
    m = re.search(r"unnudged: all_ones_cases (\d+) bad (\d+) bad_elsewhere (\d+) bad_not_one_ulp_low (\d+)", r.stdout)
    ones, bad, elsewhere, not_low = map(int, m.groups())
    assert ones >= 527 * 8 and bad > 0 and elsewhere == 0 and not_low == 0


# ---- gfx950
@pytest.fixture(scope="module")
def dev():
    assert os.path.exists(LIB), "build tests/native first (make -C tests/native -f unitv.mk)"
    # one HIP runtime per process (rtx/lib.py load): torch's copy first, so that a
    # test that runs after this one in the same process can still use torch.cuda
    import torch  # noqa: F401
    L = C.CDLL(LIB)
    P = C.POINTER(C.c_double)
    L.unitv_devcheck.argtypes = [P, C.c_int, C.c_int, P, P]
    L.unitv_devcheck.restype = C.c_int
    return L


def run(dev, a):
    a = np.ascontiguousarray(a, np.float64)
    width = 1 if a.ndim == 1 else a.shape[1]
    fused, ref = np.full_like(a, 7.0), np.full_like(a, 9.0)
    P = C.POINTER(C.c_double)
    rc = dev.unitv_devcheck(a.ctypes.data_as(P), len(a), width, fused.ctypes.data_as(P), ref.ctypes.data_as(P))
    assert rc == 0, rc
    return fused, ref


def same_bits(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def neighbours(x, k=3):
    """x and its +-k neighbours in the doubles' order (x > 0, finite)."""
    u = np.asarray(x, np.float64).view(np.int64)
    return np.concatenate([(u + d).view(np.float64) for d in range(-k, k + 1)])


def squared_lengths():
    rng = np.random.default_rng(11)
    e = np.arange(-26, 501, dtype=np.float64)
    ones = np.nextafter(np.exp2(e + 1), 0)  # all-ones l
    pows = np.exp2(e)
    pows1 = np.exp2(e) * (1 + 2.0**-52)
    k = np.arange(0, 4097, dtype=np.float64)
    u = rng.integers(0, 2**32, 100_000).astype(np.float64) * 2.0**-32
    fam = {
        "random 2^-52..2^1000": rng.uniform(1.0, 2.0, 1_000_000) * np.exp2(rng.integers(-52, 1001, 1_000_000).astype(np.float64)),
        "1 + k 2^-53": 1.0 + k * 2.0**-53,
        "1 - k 2^-53": 1.0 - k * 2.0**-53,
        "all-ones l": neighbours(ones * ones),
        "l = 2^e": neighbours(pows * pows),
        "l = 2^e (1 + 2^-52)": neighbours(pows1 * pows1),
        "k 2^-32": u,
        "1 - (k 2^-32)^2": 1.0 - u * u,
        "threshold": np.array([0.0, -0.0, 1e-17, 1e-16, np.nextafter(1e-16, 0), np.nextafter(1e-16, 1)]),
        "special": np.array([np.inf, np.nan, -1.0, -np.inf, 2.0**-767]),
    }
    return fam


@pytest.mark.gpu
def test_fused_scale_equals_root_then_reciprocal_on_device(dev):
    fam = squared_lengths()
    x = np.concatenate(list(fam.values()))
    fused, ref = run(dev, x)
    # the reference is what it is claimed to be: -1 at or below the threshold
    # (and for NaN / negative x), 0 for +inf, else 1 / sqrt(x) to an ulp or so
    t = np.sqrt(np.where(x > 0, x, np.nan))
    no_scale = ~(t > 1e-8)
    assert (ref[no_scale] == -1.0).all() and (ref[~no_scale] >= 0.0).all()
    fin = ~no_scale & np.isfinite(x)
    assert np.allclose(ref[fin] * t[fin], 1.0, rtol=0, atol=1e-15)
    assert ref[x == np.inf] == 0.0
    ok = same_bits(fused, ref)
    at = 0
    for name, v in fam.items():
        o = ok[at:at + len(v)]
        assert o.all(), (name, v[~o][:4], fused[at:at + len(v)][~o][:4], ref[at:at + len(v)][~o][:4])
        at += len(v)
    assert at == len(x)


@pytest.mark.gpu
def test_fused_unitv_equals_root_then_reciprocal_on_device(dev):
    rng = np.random.default_rng(12)
    n = 100_000
    a = rng.uniform(-1, 1, (n, 3)) * np.exp2(rng.integers(-40, 41, (n, 1)).astype(np.float64))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    j = rng.integers(-64, 65, (n, 1)).astype(np.float64)
    near = d * (1.0 + 2.0**-52 * j)  # nearly-unit vectors
    edge = np.array([[0, 0, 0], [1e-9, 0, 0], [6e-9, 6e-9, 5e-9], [1e-8, 0, 0], [0, np.nextafter(1e-8, 1), 0],
                     [1, 0, 0], [0, -1, 0], [0.6, 0.8, 0], [np.inf, 1, 1], [np.nan, 1, 1], [1e200, 1e200, 0]])
    v = np.concatenate([a, near, edge])
    fused, ref = run(dev, v)
    assert np.array_equal(ref[2 * n], [1.0, 0.0, 0.0]) and np.array_equal(ref[2 * n + 1], [1.0, 0.0, 0.0])
    assert np.abs(np.linalg.norm(ref[:2 * n], axis=1) - 1.0).max() < 1e-15
    ok = same_bits(fused, ref).all(axis=1)
    assert ok.all(), (v[~ok][:4], fused[~ok][:4], ref[~ok][:4])
