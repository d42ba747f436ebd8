"""Temporal variance: the statement of record (rtx.temporal.NumpyOps.temporal_variance,
rtx.denoise.NumpyOps.denoise_given_variance), the g++ build of the per-pixel
source (csrc/rt_temporal.h temporal_variance_pixel through
tests/native/rt_temporal_variance_emu.cpp), the ABI's argument checks, and what
the composition is for: a display that after a camera move beats the blend
alone, the blend behind the shipped filter and a restarted variance-guided
filter.  No GPU: tests/test_temporal_variance_gpu.py holds the gfx950 kernels
to all of it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from rtx import abi, adaptive, denoise, temporal
from rtx.cpu import CpuRenderer
from rtx.lib import load
from rtx.render import camera_frame
from rtx.scene import load_scene
from rtx.temporal import NumpyOps
import oracle_lib as O
from test_denoise import H, W, frame_of, random_case
from test_guides import SCENES, host_guides
from test_temporal import (HEADER_DIR, NATIVE, PG, PH, PW, START, ULP32, assert_matches_numpy, camera, history_of,
                           host_temporal, linear, moved_random_case, plane_case, random_cases, same_pose)
from test_variance import BATCH, TX, TY, mixed_strata, random_moments, rmse

FOps = denoise.NumpyOps


# ---- inputs ---------------------------------------------------------------------
def random_variances(seed=31, h=H, w=W, bad=True):
    """(variance_now [h, w] float64, previous var plane [h, w] float32), with
    NaN, negative and infinite entries in both when `bad`."""
    rng = np.random.default_rng(seed)
    v_now = rng.uniform(0.0, 0.05, (h, w))
    var = rng.uniform(0.0, 0.02, (h, w)).astype(np.float32)
    if bad:
        v_now[3, 5], v_now[9, 20], v_now[15, 33] = np.nan, -1.0, np.inf
        var[4, 6], var[10, 21], var[16, 34] = np.nan, -2.0, np.inf
    return v_now, var


def strata_of_random_case():
    return ((np.arange(TX * TY) * 7) % 6).astype(np.int32)


def poses(S, **cam):
    """tests/test_temporal_gpu.py _poses (that module needs no GPU to import, but this one stays clear of it):
    pose A, and pose B a lateral step of 2 % of the distance to the look-at point and a yaw of about 1 degree."""
    a, b = S.camera_desc(**cam), S.camera_desc(**cam)
    frm, at = np.array(a.lookfrom.tolist()), np.array(a.lookat.tolist())
    fwd = at - frm
    dist = np.linalg.norm(fwd)
    right = np.cross(fwd / dist, np.array(a.vup.tolist()))
    right /= np.linalg.norm(right)
    b.lookfrom = abi.Vec3.of(frm + 0.02 * dist * right)
    b.lookat = abi.Vec3.of(at + 0.037 * dist * right)
    return camera_frame(a), camera_frame(b)


# ---- the host twin -----------------------------------------------------------------
_emu = None


def variance_emu():
    """tests/native/build/libtemporal_variance_emu.so (built on first use: temporal_variance.mk)."""
    global _emu
    if _emu is None:
        subprocess.run(["make", "-s", "-C", NATIVE, "-f", "temporal_variance.mk"], check=True)
        L = C.CDLL(os.path.join(NATIVE, "build", "libtemporal_variance_emu.so"))
        L.emu_history_variance_bytes.restype = C.c_int64
        L.emu_history_variance_bytes.argtypes = [C.POINTER(abi.Frame)]
        L.emu_temporal_variance.argtypes = [C.POINTER(abi.Frame), C.c_void_p, C.c_double, C.c_void_p, C.c_int32,
                                            C.c_void_p, C.c_int32, C.POINTER(abi.Frame), C.c_void_p, C.c_void_p,
                                            C.POINTER(abi.TemporalParams), C.c_void_p, C.c_void_p, C.c_void_p]
        _emu = L
    return _emu


def host_temporal_variance(f, rgb, scale, tile_strata, strata_now, guides, g, v_now, f_prev=None, hist=None,
                           params=None):
    """temporal_variance_pixel on the host -> (out, (col, geo, var), variance_out)."""
    L = variance_emu()
    assert L.emu_history_variance_bytes(C.byref(f)) == temporal.history_variance_bytes(f)
    rgb, guides = np.ascontiguousarray(rgb, dtype=np.float64), np.ascontiguousarray(guides, dtype=np.float64)
    v_now = np.ascontiguousarray(v_now, dtype=np.float64)
    ts = np.ascontiguousarray(tile_strata, dtype=np.int32) if tile_strata is not None else None
    prev = temporal.pack_variance_history(f, hist) if hist is not None else None
    h_out = np.zeros(temporal.history_variance_bytes(f), dtype=np.uint8)
    out, v_out = np.zeros_like(rgb), np.zeros_like(v_now)
    p = abi.temporal_params(params)
    rc = L.emu_temporal_variance(C.byref(f), rgb.ctypes.data, scale, ts.ctypes.data if ts is not None else None,
                                 strata_now, guides.ctypes.data, g, C.byref(f_prev) if f_prev is not None else None,
                                 prev.ctypes.data if prev is not None else None, v_now.ctypes.data,
                                 C.byref(p) if p is not None else None, h_out.ctypes.data, out.ctypes.data,
                                 v_out.ctypes.data)
    assert rc == 0
    return out, temporal.unpack_variance_history(f, h_out), v_out


def assert_variance_matches_numpy(got, ref, what, worst=None):
    """`got` = (out, (col, geo, var), variance_out) against NumpyOps' (out, (col,
    geo, var), variance_out, margin): out, col and geo by
    test_temporal.assert_matches_numpy; variance_out within 1e-9 max(|numpy|,
    mean |numpy|), the var plane within one fp32 ulp; pixels on a threshold
    (margin < 1e-6) are left out (at most 0.5 % of the frame)."""
    out, (col, geo, var), v_out = got
    r_out, (r_col, r_geo, r_var), r_v, margin = ref
    assert_matches_numpy((out, (col, geo)), (r_out, (r_col, r_geo), margin), what, worst)
    use = margin >= 1e-6
    assert not np.isnan(r_v).any() and not np.isnan(v_out).any(), what
    assert np.array_equal(np.isfinite(v_out), np.isfinite(r_v)), what
    fin = np.isfinite(r_v)
    bound = np.maximum(np.abs(r_v), max(float(np.abs(r_v[fin]).mean()), 1e-300))
    m = fin & use
    ratio = float((np.abs(v_out[m] - r_v[m]) / bound[m]).max()) / 1e-9
    a, b = var[use].astype(np.float64), r_var[use].astype(np.float64)
    assert np.array_equal(np.isfinite(a), np.isfinite(b)), what
    ok = np.isfinite(b)
    ulps = float((np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1e-300)).max()) / ULP32
    if worst is not None:
        worst["v"], worst["var ulp"] = max(worst.get("v", 0.0), ratio), max(worst.get("var ulp", 0.0), ulps)
    print("temporal variance %-30s |variance_out diff| / bound = %.3g, var plane %.3g ulp (limits 1, 1)"
          % (what, ratio, ulps))
    assert ratio <= 1.0 and ulps <= 1.0, what


# ---- the colour is untouched ----------------------------------------------------------
def test_colour_is_untouched_on_every_random_case():
    fA, fB, rgb, scale, guides, g, hist = moved_random_case()
    v_now, var = random_variances()
    cases = random_cases(fA, fB, hist, strata_of_random_case())
    for what, (f, ts, fp, hp, params) in cases.items():
        hp3 = hp + (var,) if hp is not None else None
        plain = NumpyOps().temporal(f, rgb, scale, ts, g, guides, g, fp, hp, params)
        got = NumpyOps().temporal_variance(f, rgb, scale, ts, g, guides, g, v_now, fp, hp3, params)
        assert np.array_equal(got[0], plain[0], equal_nan=True), what
        assert np.array_equal(got[1][0], plain[1][0], equal_nan=True), what
        assert np.array_equal(got[1][1], plain[1][1], equal_nan=True), what
        assert np.array_equal(got[3], plain[2]), what
        # ... and the twin's is the plain twin's, bit for bit
        twin = host_temporal_variance(f, rgb, scale, ts, g, guides, g, v_now, fp, hp3, params)
        twin_plain = host_temporal(f, rgb, scale, ts, g, guides, g, fp, hp, params)
        assert np.array_equal(twin[0], twin_plain[0], equal_nan=True), what
        assert np.array_equal(twin[1][0].view(np.uint32), twin_plain[1][0].view(np.uint32)), what
        assert np.array_equal(twin[1][1].view(np.uint32), twin_plain[1][1].view(np.uint32)), what


def test_history_kinds_are_not_mixed_up():
    fA, fB, rgb, scale, guides, g, hist = moved_random_case()
    v_now, var = random_variances()
    with pytest.raises(ValueError):
        NumpyOps().temporal_variance(fB, rgb, scale, None, g, guides, g, v_now, fA, hist)  # no var plane
    with pytest.raises(ValueError):
        NumpyOps().temporal(fB, rgb, scale, None, g, guides, g, fA, hist + (var,))
    with pytest.raises(ValueError):
        NumpyOps().temporal_variance(fB, rgb, scale, None, g, guides, g, v_now[:-1], fA, hist + (var,))


# ---- the variance's own rules -----------------------------------------------------------
def test_no_history_hands_the_current_variance_on():
    f, rgb, scale, guides, g = random_case()
    f = camera(f)
    v_now, _ = random_variances(bad=False)
    strata = strata_of_random_case()
    assert (strata == 0).any()
    n_c = np.repeat(np.repeat(strata.reshape(TY, TX), 8, 0), 8, 1)[:H, :W]
    out, (col, geo, var), v_out, _ = NumpyOps().temporal_variance(f, rgb, 1.0, strata, 99, guides, g, v_now)
    assert np.array_equal(v_out[n_c > 0], v_now[n_c > 0])  # b = 1: v_c exactly
    assert (v_out[n_c == 0] == 0).all()
    assert (var[col[..., 3] == 0] == 0).all() and (col[..., 3] == 0).any()
    kept = col[..., 3] > 0
    assert np.array_equal(var[kept], v_now[kept].astype(np.float32))


def same_pose_variance(N, M, params=None, bad=False):
    f, rgb, scale, guides, g, hist, out, hist_out = same_pose(N, M, params)
    v_now, var = random_variances(bad=bad)
    got = NumpyOps().temporal_variance(f, rgb, scale, None, M, guides, g, v_now, f, hist + (var,), params)
    assert np.array_equal(got[0], out, equal_nan=True)
    keeps = guides[..., 7] / g >= abi.RT_TEMPORAL_HIT_MIN
    return got, v_now, var.astype(np.float64), keeps


def test_same_pose_blends_by_the_squared_count_shares():
    N, M = 12.0, 4
    (out, (col, geo, var_out), v_out, _), v_now, var, keeps = same_pose_variance(N, M)
    assert keeps.any() and (~keeps).any()
    want = (N * N * var + M * M * v_now) / (N + M) ** 2
    np.testing.assert_allclose(v_out[keeps], want[keeps], rtol=1e-6, atol=0)
    assert np.array_equal(v_out[~keeps], v_now[~keeps])  # below hit_min: no history, v_c itself
    np.testing.assert_allclose(var_out[keeps], want[keeps], rtol=1e-6)
    assert (var_out[~keeps] == 0).all()  # ... and nothing handed on


def test_max_history_caps_the_count_and_not_the_variance():
    N, M = 100.0, 4
    (out, (col, geo, var_out), v_out, _), v_now, var, keeps = same_pose_variance(N, M, dict(max_history=5))
    np.testing.assert_allclose(col[..., 3][keeps], 5 + M, rtol=1e-6)
    want = (25.0 * var + M * M * v_now) / (5.0 + M) ** 2  # n_h = 5, v_h = v'
    np.testing.assert_allclose(v_out[keeps], want[keeps], rtol=1e-6, atol=0)


@pytest.mark.parametrize("tilt", [0.0, 30.0])
def test_a_constant_history_variance_reprojects_to_itself(tilt):
    fA, fB, gA, gB, (x, y) = plane_case(tilt)
    jj, ii = np.mgrid[0:PH, 0:PW]
    N, vp = 9.0, np.float32(0.02)
    hist = history_of(linear(ii.astype(np.float64), jj.astype(np.float64)), N, gA, PG)
    hist3 = hist + (np.full((PH, PW), vp, dtype=np.float32),)
    rgb, v_now = np.zeros((PH, PW, 3)), np.full((PH, PW), 7.0)
    inner = (x >= 0) & (x <= PW - 1 - 1e-9) & (y >= -1e-9) & (y <= PH - 1 + 1e-9)
    assert inner.sum() > 0.8 * PW * PH
    out, (col, geo, var), v_out, _ = NumpyOps().temporal_variance(fB, rgb, 1.0, None, 0, gB, PG, v_now, fA, hist3)
    np.testing.assert_allclose(col[..., 3][inner], N, rtol=1e-6)  # every interior tap was accepted
    # linear interpolation keeps a constant; n_c = 0: the current variance (7) is dropped
    np.testing.assert_allclose(v_out[inner], float(vp), rtol=1e-12, atol=0)
    np.testing.assert_allclose(var[inner], vp, rtol=ULP32)
    nothing = col[..., 3] == 0  # off the previous image: no history and no samples
    assert nothing.any() and (v_out[nothing] == 0).all() and (var[nothing] == 0).all()


def test_invalid_taps_renormalise_the_variance_and_not_the_count():
    fA, fB, gA, gB, (x, y) = plane_case(0.0)
    N, M, vp = 10.0, 2, np.float32(0.03)
    count = np.full((PH, PW), N)
    count[:, 1::2] = 0.0  # every other column holds no history: one of the two x taps, weight 0.5 each
    hist = history_of(np.full((PH, PW, 3), 0.7), count, gA, PG)
    var = np.full((PH, PW), vp, dtype=np.float32)
    var[:, 1::2] = 50.0  # what the invalid taps hold must not be read
    rgb, v_now = np.full((PH, PW, 3), 0.1 * M), np.full((PH, PW), 0.01)
    out, (col, geo, var_out), v_out, _ = NumpyOps().temporal_variance(fB, rgb, 1.0 / M, None, M, gB, PG, v_now, fA,
                                                                      hist + (var,))
    inner = (x >= 0) & (x <= PW - 1 - 1e-9)
    n_h = 0.5 * N
    np.testing.assert_allclose(col[..., 3][inner], n_h + M, rtol=1e-6)  # the count is not renormalised ...
    want = (n_h ** 2 * float(vp) + M ** 2 * 0.01) / (n_h + M) ** 2    # ... v_h = v' is
    np.testing.assert_allclose(v_out[inner], want, rtol=1e-6, atol=0)


def test_bad_variances_and_a_nan_sample():
    N, M = 12.0, 4
    f, rgb, scale, guides, g, hist, _, _ = same_pose(N, M)
    keeps = guides[..., 7] / g >= abi.RT_TEMPORAL_HIT_MIN
    ok = keeps.copy()
    ok[[0, -1], :] = ok[:, [0, -1]] = False
    px = [tuple(p) for p in np.argwhere(ok)[::37][:7]]  # seven kept pixels, apart from each other
    assert len(px) == 7
    v_now, var = random_variances(bad=False)
    v_now[px[0]], v_now[px[1]], v_now[px[2]] = np.nan, -1.0, np.inf
    var[px[3]], var[px[4]], var[px[5]] = np.nan, -2.0, np.inf
    rgb = rgb.copy()
    rgb[px[6] + (1,)] = np.nan
    for fn in (NumpyOps().temporal_variance, host_temporal_variance):
        got = fn(f, rgb, scale, None, M, guides, g, v_now, f, hist + (var,))
        out, (col, geo, var_out), v_out = got[:3]
        a, b = (N / (N + M)) ** 2, (M / (N + M)) ** 2
        for p in px[0:2]:  # a NaN or negative current variance is 0
            np.testing.assert_allclose(v_out[p], a * float(var[p]), rtol=1e-6)
        for p in px[3:5]:  # ... and so is a NaN or negative history variance
            np.testing.assert_allclose(v_out[p], b * v_now[p], rtol=1e-6)
        assert v_out[px[2]] == np.inf and v_out[px[5]] == np.inf and var_out[px[2]] == np.inf
        assert not np.isnan(v_out).any() and not np.isnan(var_out).any()
        assert (v_out[np.isfinite(v_out)] >= 0).all()
        assert np.isnan(out[px[6]][1]) and col[px[6]][3] == 0 and var_out[px[6]] == 0


def test_a_zero_weight_tap_adds_nothing_even_an_infinite_one():
    """Pose B is pose A shifted by a whole number of pixels: two taps weigh exactly 0."""
    fA, fB, gA, gB, (x, y) = plane_case(0.0, shift_px=2.0)
    hist = history_of(np.full((PH, PW, 3), 0.5), 8.0, gA, PG)
    var = np.full((PH, PW), 0.01, dtype=np.float32)
    var[:, 20] = np.inf
    v_now = np.zeros((PH, PW))
    for fn in (NumpyOps().temporal_variance, host_temporal_variance):
        v_out = fn(fB, np.zeros((PH, PW, 3)), 1.0, None, 0, gB, PG, v_now, fA, hist + (var,))[2]
        assert not np.isnan(v_out).any()
        assert 1 <= np.isinf(v_out).any(0).sum() <= 2  # the column itself (and, off by a rounding, one neighbour)


# ---- the twin against NumPy ---------------------------------------------------------------
def test_host_twin_matches_numpy_on_the_moved_random_case():
    fA, fB, rgb, scale, guides, g, hist = moved_random_case()
    v_now, var = random_variances()
    cases = random_cases(fA, fB, hist, strata_of_random_case())
    for what, (f, ts, fp, hp, params) in cases.items():
        hp3 = hp + (var,) if hp is not None else None
        ref = NumpyOps().temporal_variance(f, rgb, scale, ts, g, guides, g, v_now, fp, hp3, params)
        got = host_temporal_variance(f, rgb, scale, ts, g, guides, g, v_now, fp, hp3, params)
        assert_variance_matches_numpy(got, ref, what)
    # teeth: with history the variance is not the current one
    moved = NumpyOps().temporal_variance(fB, rgb, scale, None, g, guides, g, v_now, fA, hist + (var,), START)
    fin = np.isfinite(moved[2]) & np.isfinite(v_now)
    assert (np.abs(moved[2][fin] - v_now[fin]) > 1e-4).mean() > 0.2


@pytest.mark.parametrize("tilt", [0.0, 30.0])
def test_host_twin_matches_numpy_on_the_planes(tilt):
    fA, fB, gA, gB, _ = plane_case(tilt)
    rng = np.random.default_rng(2)
    hist = history_of(rng.uniform(0.0, 3.0, (PH, PW, 3)), 9.0, gA, PG)
    v_now, var = random_variances(h=PH, w=PW)
    rgb = rng.uniform(0.0, 2.0, (PH, PW, 3)) * PG
    args = (fB, rgb, 1.0 / PG, None, PG, gB, PG, v_now, fA, hist + (var,), START)
    assert_variance_matches_numpy(host_temporal_variance(*args), NumpyOps().temporal_variance(*args),
                                  "plane %g" % tilt)


# ---- the filter on a given variance ----------------------------------------------------------
def filter_cases():
    """label -> (tile strata, s1, s2, batch, scale) on test_denoise.random_case: moments everywhere, none, mixed."""
    f, rgb, scale, guides, g = random_case()
    full = np.full(TX * TY, 16, dtype=np.int32)
    mixed = mixed_strata()
    return (f, rgb, guides, g), {
        "moments": (full,) + random_moments(rgb, full) + (BATCH, 1.0),
        "spatial only": (None, None, None, 0, scale),
        "mixed tiles": (mixed,) + random_moments(rgb, mixed) + (BATCH, 99.0),
    }


def test_given_the_estimated_variance_the_filter_is_the_variance_guided_one():
    (f, rgb, guides, g), cases = filter_cases()
    ops = FOps()
    for what, (strata, s1, s2, batch, scale) in cases.items():
        for params in (None, dict(passes=2, sigma_lum=2.0)):
            est = dict(params or {}, passes=-1)
            _, v0 = ops.denoise_variance(f, rgb, scale, strata, guides, g, s1, s2, batch, est, with_variance=True)
            want = ops.denoise_variance(f, rgb, scale, strata, guides, g, s1, s2, batch, params, with_variance=True)
            got = ops.denoise_given_variance(f, rgb, scale, strata, guides, g, v0, params, with_variance=True)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
            # min_batches is ignored
            p = dict(params or {}, min_batches=99)
            assert np.array_equal(ops.denoise_given_variance(f, rgb, scale, strata, guides, g, v0, p), want[0])


def test_a_zero_variance_plane_lets_every_pixel_go():
    """tests/test_variance.py test_zero_variance_moments_let_every_pixel_go, the plane given."""
    f, rgb, scale, guides, g = random_case()
    strata = np.full(TX * TY, 16, dtype=np.int32)
    ops = FOps()
    out, v = ops.denoise_given_variance(f, rgb, 1.0, strata, guides, g, np.zeros((H, W)), with_variance=True)
    np.testing.assert_allclose(out, rgb / 16, rtol=1e-12, atol=0)
    assert (v == 0).all()
    # NaN and negative entries are zeros
    bad = np.zeros((H, W))
    bad[::2], bad[1::2] = np.nan, -3.0
    assert np.array_equal(ops.denoise_given_variance(f, rgb, 1.0, strata, guides, g, bad), out)
    # ... and a real variance filters
    wide = ops.denoise_given_variance(f, rgb, 1.0, strata, guides, g, np.full((H, W), 0.5))
    assert np.abs(wide - rgb / 16).max() > 1e-3


def test_given_variance_with_the_luminance_term_off_is_the_shipped_filter_without_its_colour_term():
    f, rgb, scale, guides, g = random_case()
    v, _ = random_variances()
    for passes in (0, 1, 8):
        ref = FOps().denoise(f, rgb, scale, None, guides, g, dict(passes=passes, sigma_color=-1))
        out = FOps().denoise_given_variance(f, rgb, scale, None, guides, g, v, dict(passes=passes, sigma_lum=-1))
        assert np.array_equal(out, ref)


def test_given_variance_keeps_a_nan_sample_from_spreading():
    f, rgb, scale, guides, g = random_case()
    rgb[20, 30, 1] = np.nan
    v, _ = random_variances()
    v[20, 30] = 0.3  # the variance of a non-finite e is 0 whatever the plane says
    out, v1 = FOps().denoise_given_variance(f, rgb, scale, None, guides, g, v, dict(passes=-1), with_variance=True)
    assert v1[20, 30] == 0 and np.isnan(out[20, 30, 1])
    out, v1 = FOps().denoise_given_variance(f, rgb, scale, None, guides, g, v, with_variance=True)
    assert np.isfinite(out).all() and not np.isnan(v1).any()
    with pytest.raises(ValueError):
        FOps().denoise_given_variance(f, rgb, scale, None, guides, g, v[:-1])
    with pytest.raises(ValueError):
        FOps().denoise_given_variance(f, rgb, scale, None, guides, 0, v)


# ---- ABI (no device call is reached) -------------------------------------------------------
def test_history_variance_bytes():
    L = load()
    f = frame_of(36, 35)
    n = C.c_int64(-1)
    assert L.rt_history_variance_bytes(C.byref(f), C.byref(n)) == abi.RT_OK
    assert n.value == temporal.history_variance_bytes(f) == 2 * 20224 + 5120
    assert n.value % 256 == 0 and n.value >= 36 * 36 * 35
    assert temporal.history_variance_bytes(frame_of(3, 3)) == 768
    assert L.rt_history_variance_bytes(C.byref(f), None) == abi.RT_ERR_INVALID and b"null" in L.rt_last_error()
    assert L.rt_history_variance_bytes(C.byref(frame_of(0, 36)), C.byref(n)) == abi.RT_ERR_INVALID
    assert L.rt_history_variance_bytes(None, C.byref(n)) == abi.RT_ERR_INVALID and b"frame" in L.rt_last_error()
    # the first rt_history_bytes bytes are a plain history
    col = np.arange(36 * 35 * 4, dtype=np.float32).reshape(35, 36, 4)
    var = np.arange(36 * 35, dtype=np.float32).reshape(35, 36)
    buf = temporal.pack_variance_history(f, (col, -col, var))
    back = temporal.unpack_variance_history(f, buf)
    assert all(np.array_equal(a, b) for a, b in zip(back, (col, -col, var)))
    plain = temporal.unpack_history(f, buf[:temporal.history_bytes(f)])
    assert np.array_equal(plain[0], col) and np.array_equal(plain[1], -col)


def test_temporal_variance_refusals_before_any_device_call():
    L = load()
    f = camera(frame_of(36, 36))
    # addresses that are never dereferenced: every call below is refused on its arguments
    rgb, guides, hp, ho, out, vn, vo = (0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000,
                                        0x70000000)
    hb, plain = temporal.history_variance_bytes(f), temporal.history_bytes(f)
    assert hb - plain >= 256
    NONE = object()

    def call(rgb=rgb, guides=guides, hp=hp, ho=ho, out=out, vn=vn, vo=vo, g=4, strata=4, params=None, frame=f,
             prev=f):
        p = abi.temporal_params(params)
        return L.rt_temporal_variance_device(
            C.byref(frame) if frame is not NONE else None, C.c_void_p(rgb), 1.0, None, strata, C.c_void_p(guides), g,
            C.byref(prev) if prev is not NONE else None, C.c_void_p(hp), C.c_void_p(vn),
            C.byref(p) if p is not None else None, C.c_void_p(ho), C.c_void_p(out), C.c_void_p(vo), None)

    cases = {
        # rt_temporal_device's
        "null frame": (dict(frame=NONE), b"frame"),
        "empty frame": (dict(frame=frame_of(36, 0)), b"frame"),
        "null rgb": (dict(rgb=0), b"null"),
        "null guides": (dict(guides=0), b"null"),
        "null history_out": (dict(ho=0), b"null"),
        "null out": (dict(out=0), b"null"),
        "guide_strata 0": (dict(g=0), b"guide_strata"),
        "strata_now -1": (dict(strata=-1), b"strata_now"),
        "a frame without a history": (dict(hp=0), b"both or neither"),
        "a history without a frame": (dict(prev=NONE), b"both or neither"),
        "frame_prev of another size": (dict(prev=camera(frame_of(36, 35))), b"another size"),
        "unaligned history_out": (dict(ho=ho + 16), b"aligned"),
        "unaligned history_prev": (dict(hp=hp + 128), b"aligned"),
        "history_out is history_prev": (dict(ho=hp), b"overlaps device_history_prev"),
        # ... with the larger history: these two lie past a plain history's end
        "history_out in history_prev's var plane": (dict(ho=hp + plain), b"overlaps device_history_prev"),
        "out in history_out's var plane": (dict(out=ho + plain + 8), b"overlaps a history"),
        "out inside history_prev": (dict(out=hp + 8), b"overlaps a history"),
        "max_history -1": (dict(params=dict(max_history=-1)), b"max_history"),
        "NaN sigma": (dict(params=dict(sigma_depth=float("nan"))), b"NaN"),
        # ... and this function's own
        "null variance_now": (dict(vn=0), b"null"),
        "null variance_out": (dict(vo=0), b"null"),
        "variance_out is variance_now": (dict(vo=vn), b"overlaps device_variance_now"),
        "variance_out inside variance_now": (dict(vo=vn + 36 * 36 * 8 - 8), b"overlaps device_variance_now"),
        "variance_out in history_out's var plane": (dict(vo=ho + plain), b"device_variance_out overlaps a history"),
        "variance_out inside history_prev": (dict(vo=hp + hb - 8), b"device_variance_out overlaps a history"),
        "variance_out inside out": (dict(vo=out + 1024), b"overlaps device_out"),
    }
    for what, (kw, word) in cases.items():
        assert call(**kw) == abi.RT_ERR_INVALID, what
        assert word in L.rt_last_error(), (what, L.rt_last_error())


def test_given_variance_refusals_before_any_device_call():
    L = load()
    f = frame_of(36, 36)
    rgb, guides, ws, out, strata, given, var = (0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000,
                                                0x60000000, 0x80000000)

    def call(rgb=rgb, guides=guides, ws=ws, out=out, g=4, strata=strata, given=given, var=var, params=None,
             frame=f):
        p = abi.denoise_variance_params(params)
        return L.rt_denoise_given_variance_device(
            C.byref(frame), C.c_void_p(rgb), 1.0, C.c_void_p(strata), C.c_void_p(guides), g, C.c_void_p(given),
            C.byref(p) if p is not None else None, C.c_void_p(ws), C.c_void_p(out), C.c_void_p(var), None)

    nan = float("nan")
    cases = {
        # rt_denoise_variance_device's
        "passes 9": dict(params=dict(passes=9)),
        "guide_strata 0": dict(g=0),
        "null rgb": dict(rgb=0),
        "null guides": dict(guides=0),
        "null workspace": dict(ws=0),
        "null out": dict(out=0),
        "unaligned workspace": dict(ws=ws + 8),
        "out inside the workspace": dict(out=ws + 256),
        "empty frame": dict(frame=frame_of(36, 0)),
        "variance_out inside the workspace": dict(var=ws + 4 * 20736),
        "variance_out ending in the workspace": dict(var=ws - 8),
        "variance_out inside the output": dict(var=out + 1024),
        "NaN sigma_lum": dict(params=dict(sigma_lum=nan)),
        "NaN sigma_normal": dict(params=dict(sigma_normal=nan)),
        "NaN sigma_depth": dict(params=dict(sigma_depth=nan)),
        "NaN sigma_hit": dict(params=dict(sigma_hit=nan)),
        # ... and this function's own
        "null variance": dict(given=0),
        "variance inside the workspace": dict(given=ws + 4 * 20736),
        "variance inside the output": dict(given=out + 8),
        "variance is variance_out": dict(given=var),
        "variance ending in variance_out": dict(given=var - 8),
    }
    for what, kw in cases.items():
        assert call(**kw) == abi.RT_ERR_INVALID, what
        assert L.rt_last_error(), what
    assert b"device_variance overlaps device_variance_out" in L.rt_last_error()


def test_a_c_program_sees_the_three_prototypes(tmp_path):
    """The header declares the three functions with the argument lists rtx/lib.py binds; the library exports them."""
    src = tmp_path / "protos.c"
    src.write_text("\n".join([
        '#include "rt_api.h"',
        "int (*a)(const rt_frame *, int64_t *) = rt_history_variance_bytes;",
        "int (*b)(const rt_frame *, const double *, double, const int32_t *, int32_t, const double *, int32_t,",
        "         const rt_frame *, const void *, const double *, const rt_temporal_params *, void *, double *,",
        "         double *, void *) = rt_temporal_variance_device;",
        "int (*c)(const rt_frame *, const double *, double, const int32_t *, const double *, int32_t,",
        "         const double *, const rt_denoise_variance_params *, void *, double *, double *, void *)",
        "    = rt_denoise_given_variance_device;",
        "int main(void) { return RT_ABI_VERSION == 5 && a && b && c ? 0 : 1; }"]))
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", "-I", HEADER_DIR, str(src), "-o",
                    str(tmp_path / "protos.o")], check=True, capture_output=True)
    L = load()
    for name in ("rt_history_variance_bytes", "rt_temporal_variance_device", "rt_denoise_given_variance_device"):
        assert name in abi.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None
    assert len(L.rt_temporal_variance_device.argtypes) == 15
    assert len(L.rt_denoise_given_variance_device.argtypes) == 12
    assert abi.RT_ABI_VERSION == 5


# ---- quality: the composition after a camera move ------------------------------------------------
COLUMNS = ("raw", "restart + shipped", "restart + variance-guided", "blend alone", "blend + shipped",
           "blend + carried variance")


def accumulate(render, f, batches, bs):
    """`batches` batches of `bs` strata folded as AdaptiveRenderer.step folds them -> (acc, s1, s2, tile strata)."""
    h, w = f.image_height, f.image_width
    tiles = np.arange(((w + 7) // 8) * ((h + 7) // 8), dtype=np.int32)
    acc, s1, s2 = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
    tile_strata = np.zeros(tiles.size, dtype=np.int32)
    for k in range(batches):
        adaptive.NumpyOps().update(render(f, k * bs, bs), bs, tiles, tiles.size, f, acc, s1, s2, tile_strata)
    return acc, s1, s2, tile_strata


def display_chain(f, state, guides, g, bs, f_prev=None, hist=None, params=None):
    """TemporalVarianceDisplay.image() in NumPy: the three calls -> (image, blend, variance history, v_out)."""
    acc, s1, s2, ts = state
    _, v_now = FOps().denoise_variance(f, acc, 1.0, ts, guides, g, s1, s2, bs, dict(passes=-1), with_variance=True)
    blend, hist_out, v_out, _ = NumpyOps().temporal_variance(f, acc, 1.0, ts, 0, guides, g, v_now, f_prev, hist,
                                                             params)
    return FOps().denoise_given_variance(f, blend, 1.0, None, guides, g, v_out), blend, hist_out, v_out


def six_columns(fB, state, guides, g, bs, fA, histA, ref, params=None):
    """The six RMSEs of COLUMNS at pose B; histA: pose A's variance history."""
    acc, s1, s2, ts = state
    n = np.repeat(np.repeat(np.maximum(1, ts).reshape(-1, (fB.image_width + 7) // 8), 8, 0), 8, 1)
    raw = acc / n[:fB.image_height, :fB.image_width, None]
    new, blend, _, _ = display_chain(fB, state, guides, g, bs, fA, histA, params)
    plain, _, _ = NumpyOps().temporal(fB, acc, 1.0, ts, 0, guides, g, fA, histA[:2], params)
    assert np.array_equal(plain, blend, equal_nan=True)
    imgs = (raw, FOps().denoise(fB, acc, 1.0, ts, guides, g),
            FOps().denoise_variance(fB, acc, 1.0, ts, guides, g, s1, s2, bs), blend,
            FOps().denoise(fB, blend, 1.0, None, guides, g), new)
    return tuple(rmse(i, ref) for i in imgs)


def assert_orderings(e, what):
    print("\n%s: RMSE against the reference at pose B" % what)
    for name, v in zip(COLUMNS, e):
        print("  %-28s %.5f" % (name, v))
    assert e[5] < e[3], "the composed display must beat the blend alone"
    assert e[5] < e[4], "the composed display must beat the blend behind the shipped filter"
    assert e[5] < e[2], "the composed display must beat a restarted variance-guided filter"


def test_the_composition_beats_its_parts_after_a_camera_move():
    """Cornell 64 x 64, depth 8, seed 5, all on the host: 64 strata at pose A
    in 8 batches of 8, then 4 at pose B in 2 batches of 2, against 1,024
    strata at B of seed 1234; the shipped RT_TEMPORAL_* and RT_DENOISE_*
    defaults.  Measured (raw / restart + shipped filter / restart +
    variance-guided / blend alone / blend + shipped filter / blend + carried
    variance): 0.11386 / 0.06151 / 0.06752 / 0.03781 / 0.06052 / 0.02825."""
    S = load_scene(os.path.join(SCENES, "cornell.json"))
    cam = dict(image_width=64, aspect_ratio=1.0, max_depth=8)
    fA, _ = poses(S, samples_per_pixel=64, **cam)
    _, fB = poses(S, samples_per_pixel=4, **cam)
    _, fBref = poses(S, samples_per_pixel=1024, **cam)
    R = CpuRenderer(S)

    def render(f, first, count, seed=5):
        out = torch.zeros((f.image_height, f.image_width, 3), dtype=torch.float64)
        R.render_device(f, out.data_ptr(), seed=seed, samples=(first, count), output=abi.RT_OUT_SUM)
        return out.numpy()

    ref = render(fBref, 0, 1024, seed=1234) / 1024.0
    stateA = accumulate(render, fA, 8, 8)
    _, _, histA, vA = display_chain(fA, stateA, host_guides(S, fA, samples=(0, 16), seed=5), 16, 8)
    assert (histA[0][..., 3] == 64).mean() > 0.5 and (vA > 0).mean() > 0.5
    stateB = accumulate(render, fB, 2, 2)
    e = six_columns(fB, stateB, host_guides(S, fB, samples=(0, 4), seed=5), 4, 2, fA, histA, ref)
    assert_orderings(e, "cornell 64x64 (host), 64 strata at A then 4 at B")
