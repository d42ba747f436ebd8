"""The temporal reprojection's statement of record (rtx.temporal.NumpyOps.temporal),
the g++ build of its per-pixel source (csrc/rt_temporal.h through
tests/native/rt_temporal_emu.cpp) and the ABI's argument checks.  No GPU:
tests/test_temporal_gpu.py holds the gfx950 kernel to both.

Analytic scenes: a pinhole camera looking down -z (or yawed about y) and
planes whose ray intersections are closed forms, so that where a pixel of the
new pose lands in the previous image is known without the code under test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rtx import abi, temporal
from rtx.temporal import NumpyOps
from rtx.lib import load
import oracle_lib as O
from test_denoise import H, W, frame_of, random_case

HEADER_DIR = os.path.join(O.ROOT, "include")
NATIVE = os.path.join(os.path.dirname(__file__), "native")
ULP32 = 2.0 ** -23
# the parameters the sweep started from: both validity tests on, and tight (the shipped defaults are looser)
START = dict(max_history=32, sigma_depth=0.02, sigma_normal=0.35, hit_min=0.75)


# ---- cameras and analytic guides ----------------------------------------------
def camera(f, center=(0.0, 0.0, 0.0), yaw=0.0, half_width=1.0):
    """A copy of `f` with a pinhole camera at `center`, looking down -z turned
    by `yaw` about y, its viewport 2 half_width wide at distance 1."""
    f = abi.Frame.from_buffer_copy(f)
    w, h = f.image_width, f.image_height
    px = 2.0 * half_width / w
    c, s = np.cos(yaw), np.sin(yaw)
    center = np.asarray(center, dtype=np.float64)
    du, dv, fwd = px * np.array([c, 0.0, -s]), px * np.array([0.0, -1.0, 0.0]), np.array([-s, 0.0, -c])
    f.center, f.pixel_delta_u, f.pixel_delta_v = abi.Vec3.of(center), abi.Vec3.of(du), abi.Vec3.of(dv)
    f.pixel00_loc = abi.Vec3.of(center + fwd - 0.5 * (w - 1) * du - 0.5 * (h - 1) * dv)
    return f


def rays(f):
    """(centre, unit directions [H, W, 3]) of the pixel-centre rays."""
    c, p00, du, dv = temporal._cam(f)
    jj, ii = np.mgrid[0:f.image_height, 0:f.image_width]
    d = p00 + ii[..., None] * du + jj[..., None] * dv - c
    return c, d / np.linalg.norm(d, axis=-1, keepdims=True)


def plane_guides(f, g, planes):
    """Guide sums of `g` identical strata over `planes` = [(point, unit normal,
    half size or None)]: axis-aligned squares (in x, y about `point`) or
    unbounded planes, nearest hit first; albedo 1.  Also the hit index map."""
    c, d = rays(f)
    h, w = d.shape[:2]
    best, which = np.full((h, w), np.inf), np.full((h, w), -1)
    for k, (x0, n, half) in enumerate(planes):
        x0, n = np.asarray(x0, dtype=np.float64), np.asarray(n, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((x0 - c) @ n) / (d @ n)
        ok = t > 0
        if half is not None:
            p = c + t[..., None] * d
            ok &= (np.abs(p[..., 0] - x0[0]) <= half) & (np.abs(p[..., 1] - x0[1]) <= half)
        ok &= t < best
        best, which = np.where(ok, t, best), np.where(ok, k, which)
    hit = which >= 0
    guides = np.zeros((h, w, 8))
    guides[..., 0:3] = g
    for k, (x0, n, half) in enumerate(planes):
        guides[which == k, 3:6] = np.asarray(n) * g
    guides[..., 6] = np.where(hit, best, 0.0) * g
    guides[..., 7] = hit * float(g)
    return guides, which


def history_of(e, count, guides, g):
    """A history ((col, geo) float32) holding the signal `e` with `count`, on the geometry of `guides`."""
    h, w = e.shape[:2]
    col = np.concatenate([e, np.broadcast_to(np.asarray(count, dtype=np.float64), (h, w))[..., None]], -1)
    z = guides[..., 6] / np.maximum(guides[..., 7], 1.0)
    geo = np.concatenate([guides[..., 3:6] / g, z[..., None]], -1)
    return col.astype(np.float32), geo.astype(np.float32)


LIN = np.array([[0.30, 0.011, 0.007], [0.80, -0.004, 0.013], [0.50, 0.009, -0.006]])  # per channel: a + b x + c y


def linear(x, y):
    return LIN[:, 0] + x[..., None] * LIN[:, 1] + y[..., None] * LIN[:, 2]


PW, PH, PG, HALF = 48, 20, 4, 0.25  # the plane frames: 48 x 20, viewport half width 0.25
D = 10.0


def plane_case(tilt_deg, shift_px=2.5):
    """Pose A at the origin, pose B stepped sideways so that a fronto-parallel
    plane at distance D shifts by `shift_px` pixels; the plane is tilted by
    `tilt_deg` about y.  -> (fA, fB, guides A, guides B, analytic (x, y) in A
    of every B pixel)."""
    base = frame_of(PW, PH)
    fA = camera(base, half_width=HALF)
    px = 2.0 * HALF / PW
    fB = camera(base, center=(shift_px * D * px, 0.0, 0.0), half_width=HALF)
    t = np.radians(tilt_deg)
    plane = [((0.0, 0.0, -D), (np.sin(t), 0.0, np.cos(t)), None)]
    gA, _ = plane_guides(fA, PG, plane)
    gB, _ = plane_guides(fB, PG, plane)
    cB, dB = rays(fB)
    P = cB + (gB[..., 6] / PG)[..., None] * dB
    # A looks down -z from the origin with its image plane at z = -1
    x = (P[..., 0] / -P[..., 2]) / px + 0.5 * (PW - 1)
    y = -(P[..., 1] / -P[..., 2]) / px + 0.5 * (PH - 1)
    return fA, fB, gA, gB, (x, y)


# ---- same pose ------------------------------------------------------------------
def same_pose(N=12.0, M=4, params=None, tile_strata=None, seed=5):
    f, rgb, _, guides, g = random_case()
    f = camera(f)
    rng = np.random.default_rng(seed)
    e_hist = rng.uniform(0.0, 3.0, (H, W, 3))
    hist = history_of(e_hist, N, guides, g)
    scale = 1.0 / M
    out, hist_out, margin = NumpyOps().temporal(f, rgb, scale, tile_strata, M, guides, g, f, hist, params)
    return f, rgb, scale, guides, g, hist, out, hist_out


def test_same_pose_is_the_count_weighted_mean():
    N, M = 12.0, 4
    f, rgb, scale, guides, g, hist, out, hist_out = same_pose(N, M)
    a_d = np.maximum(guides[..., 0:3] / g, 0.01)
    e = rgb * scale / a_d
    keeps = guides[..., 7] / g >= abi.RT_TEMPORAL_HIT_MIN
    assert keeps.any() and (~keeps).any()
    want = (N * hist[0][..., :3].astype(np.float64) + M * e) / (N + M) * a_d
    np.testing.assert_allclose(out[keeps], want[keeps], rtol=1e-6, atol=0)
    np.testing.assert_allclose(out[~keeps], (rgb * scale)[~keeps], rtol=1e-12, atol=0)
    np.testing.assert_allclose(hist_out[0][..., 3][keeps], N + M, rtol=1e-6)
    assert np.all(hist_out[0][..., 3][~keeps] == 0)  # below hit_min: nothing to hand on
    assert np.array_equal(hist_out[1], hist[1])
    # no previous history: the current image, and a first history
    out0, h0, margin = NumpyOps().temporal(f, rgb, scale, None, M, guides, g)
    np.testing.assert_allclose(out0, rgb * scale, rtol=1e-12, atol=0)
    assert np.all(h0[0][..., 3][keeps] == M) and np.all(h0[0][..., 3][~keeps] == 0) and np.all(np.isinf(margin))
    np.testing.assert_allclose(h0[0][..., :3], e, rtol=ULP32)


# ---- analytic planes ---------------------------------------------------------------
@pytest.mark.parametrize("tilt", [0.0, 70.0])
def test_a_plane_reprojects_a_linear_history_exactly(tilt):
    fA, fB, gA, gB, (x, y) = plane_case(tilt)
    jj, ii = np.mgrid[0:PH, 0:PW]
    N = 9.0
    hist = history_of(linear(ii.astype(np.float64), jj.astype(np.float64)), N, gA, PG)
    rgb = np.zeros((PH, PW, 3))
    # every pixel whose four taps lie inside the previous image (1e-9: an integer y may floor either way)
    inner = (x >= 0) & (x <= PW - 1 - 1e-9) & (y >= -1e-9) & (y <= PH - 1 + 1e-9)
    assert inner.sum() > 0.8 * PW * PH
    if tilt == 0.0:
        np.testing.assert_allclose(x, ii + 2.5, rtol=0, atol=1e-9)
    else:  # teeth: neighbouring pixels' depths differ by more than sigma_depth of the distance
        z = gA[..., 6] / PG
        assert (np.abs(np.diff(z, axis=1)) > START["sigma_depth"] * z[:, 1:]).mean() > 0.5
    for params in (None, START):  # the default sigma_depth, and the tight one
        out, hist_out, margin = NumpyOps().temporal(fB, rgb, 1.0, None, 0, gB, PG, fA, hist, params)  # n_c = 0
        np.testing.assert_allclose(out[inner], linear(x, y)[inner], rtol=1e-5, atol=0)
        # every interior tap was accepted: the whole count arrives
        np.testing.assert_allclose(hist_out[0][..., 3][inner], N, rtol=1e-6)
        assert margin[inner].min() > 0.5


def occluder_case():
    """The plane at D behind a square of half size 1 at distance 5, pose B 0.5 to the right of pose A."""
    base = frame_of(PW, PH)
    fA, fB = camera(base, half_width=HALF), camera(base, center=(0.5, 0.0, 0.0), half_width=HALF)
    scene = [((0.0, 0.0, -D), (0.0, 0.0, 1.0), None), ((0.0, 0.0, -5.0), (0.0, 0.0, 1.0), 1.0)]
    gA, idA = plane_guides(fA, PG, scene)
    gB, idB = plane_guides(fB, PG, scene)
    return fA, fB, gA, gB, idA, idB


def test_disocclusion_and_image_border_leave_the_current_image():
    fA, fB, gA, gB, idA, idB = occluder_case()
    rng = np.random.default_rng(3)
    M = 4  # a power of two: (M e) / M is e exactly
    rgb = rng.uniform(0.0, 2.0, (PH, PW, 3)) * M
    hist = history_of(rng.uniform(0.0, 3.0, (PH, PW, 3)), 20.0, gA, PG)
    ops = NumpyOps()
    out, hist_out, _ = ops.temporal(fB, rgb, 1.0 / M, None, M, gB, PG, fA, hist, START)
    current, _, _ = ops.temporal(fB, rgb, 1.0 / M, None, M, gB, PG)
    # where every B pixel lands in A, analytically (both planes are fronto-parallel)
    px = 2.0 * HALF / PW
    cB, dB = rays(fB)
    P = cB + (gB[..., 6] / PG)[..., None] * dB
    x = (P[..., 0] / -P[..., 2]) / px + 0.5 * (PW - 1)
    x0 = np.floor(x + 1e-9).astype(int)
    jj = np.mgrid[0:PH, 0:PW][0]
    inside = (x0 >= 0) & (x0 + 1 <= PW - 1)
    on_occluder = np.zeros((PH, PW), dtype=bool)
    on_occluder[inside] = (idA[jj[inside], x0[inside]] == 1) & (idA[jj[inside], x0[inside] + 1] == 1)
    rows = (np.abs(jj - 0.5 * (PH - 1)) < 0.5 * PH - 2)  # rows whose neighbours above and below see the same
    disoccluded = (idB == 0) & on_occluder & rows
    outside = (idB == 0) & (x > PW)
    assert disoccluded.sum() >= 20 and outside.sum() >= 20
    for sel in (disoccluded, outside):
        assert np.array_equal(out[sel], current[sel])
        assert np.all(hist_out[0][..., 3][sel] == M)  # n_h = 0
    kept = (idB == 0) & inside & ~on_occluder & (idA[jj, np.clip(x0, 0, PW - 1)] == 0)
    assert (hist_out[0][..., 3][kept] > M).mean() > 0.9  # elsewhere the plane keeps its history
    # a half turn: nothing lies in front of the previous camera
    fT = camera(fB, center=(0.5, 0.0, 0.0), yaw=np.pi, half_width=HALF)
    out, hist_out, _ = ops.temporal(fB, rgb, 1.0 / M, None, M, gB, PG, fT, hist)
    assert np.array_equal(out, current) and np.all(hist_out[0][..., 3] == M)


# ---- count rules --------------------------------------------------------------------
def test_max_history_caps_the_history_count():
    for mh, N in ((0, 100.0), (8, 100.0), (8, 5.0)):
        f, rgb, scale, guides, g, hist, out, hist_out = same_pose(N, 4, dict(max_history=mh))
        keeps = guides[..., 7] / g >= abi.RT_TEMPORAL_HIT_MIN
        want = min(N, mh or abi.RT_TEMPORAL_MAX_HISTORY) + 4
        np.testing.assert_allclose(hist_out[0][..., 3][keeps], want, rtol=1e-6)


def test_a_half_valid_footprint_halves_the_history_weight():
    fA, fB, gA, gB, (x, y) = plane_case(0.0)
    N, M = 10.0, 2
    count = np.full((PH, PW), N)
    count[:, 1::2] = 0.0  # every other column holds no history: one of the two x taps, weight 0.5 each
    hist = history_of(np.full((PH, PW, 3), 0.7), count, gA, PG)
    rgb = np.full((PH, PW, 3), 0.1 * M)
    out, hist_out, _ = NumpyOps().temporal(fB, rgb, 1.0 / M, None, M, gB, PG, fA, hist)
    inner = (x >= 0) & (x <= PW - 1 - 1e-9)
    np.testing.assert_allclose(hist_out[0][..., 3][inner], 0.5 * N + M, rtol=1e-6)
    np.testing.assert_allclose(out[inner], (0.5 * N * 0.7 + M * 0.1) / (0.5 * N + M), rtol=1e-6)
    # a NaN tap is skipped like an empty one
    e = np.full((PH, PW, 3), 0.7)
    e[:, 1::2, 1] = np.nan
    hist = history_of(e, N, gA, PG)
    out2, hist_out2, _ = NumpyOps().temporal(fB, rgb, 1.0 / M, None, M, gB, PG, fA, hist)
    assert np.isfinite(out2).all()
    np.testing.assert_allclose(out2[inner], out[inner], rtol=1e-6)
    np.testing.assert_allclose(hist_out2[0][..., 3][inner], 0.5 * N + M, rtol=1e-6)


def test_tile_strata_give_per_tile_counts():
    tx, ty = (W + 7) // 8, (H + 7) // 8
    strata = ((np.arange(tx * ty) * 7) % 6).astype(np.int32)  # mixed counts, 0 included
    assert (strata == 0).any()
    N = 12.0
    f, rgb, scale, guides, g, hist, out, hist_out = same_pose(N, 99, None, strata)
    n_c = np.repeat(np.repeat(strata.reshape(ty, tx), 8, 0), 8, 1)[:H, :W].astype(np.float64)
    a_d = np.maximum(guides[..., 0:3] / g, 0.01)
    e = rgb / np.maximum(1.0, n_c)[..., None] / a_d
    keeps = guides[..., 7] / g >= abi.RT_TEMPORAL_HIT_MIN
    np.testing.assert_allclose(hist_out[0][..., 3][keeps], (N + n_c)[keeps], rtol=1e-6)
    want = (N * hist[0][..., :3].astype(np.float64) + n_c[..., None] * e) / (N + n_c)[..., None] * a_d
    np.testing.assert_allclose(out[keeps], want[keeps], rtol=1e-6)
    empty = keeps & (n_c == 0)  # no sample yet: the history alone
    assert empty.any()
    np.testing.assert_allclose(out[empty], (hist[0][..., :3].astype(np.float64) * a_d)[empty], rtol=1e-6)


def test_non_finite_samples_and_taps():
    f, rgb, _, guides, g = random_case()
    f = camera(f)
    M, N = 4, 12.0
    rng = np.random.default_rng(5)
    e_hist = rng.uniform(0.0, 3.0, (H, W, 3))
    e_hist[20, 10, 2] = np.nan        # a NaN history tap: skipped
    hist = history_of(e_hist, N, guides, g)
    rgb[25, 40, 1] = np.nan           # a NaN current sample: passes through, stored with count 0
    rgb[26, 41, 0] = np.inf
    out, hist_out, _ = NumpyOps().temporal(f, rgb, 1.0 / M, None, M, guides, g, f, hist)
    current, _, _ = NumpyOps().temporal(f, rgb, 1.0 / M, None, M, guides, g)
    assert np.isfinite(out[20, 10]).all()
    np.testing.assert_allclose(out[20, 10], current[20, 10], rtol=1e-9)
    np.testing.assert_allclose(hist_out[0][20, 10, 3], M, rtol=1e-6)
    assert np.isnan(out[25, 40, 1]) and np.isfinite(out[25, 40, [0, 2]]).all()
    assert np.isinf(out[26, 41, 0])
    assert hist_out[0][25, 40, 3] == 0 and hist_out[0][26, 41, 3] == 0
    bad = ~np.isfinite(out).all(-1)
    assert bad.sum() == 2


def test_params_resolution_and_refusals():
    def on(v):
        return None if v < 0 else v
    assert temporal.resolve(None) == (abi.RT_TEMPORAL_MAX_HISTORY, on(abi.RT_TEMPORAL_SIGMA_DEPTH),
                                      on(abi.RT_TEMPORAL_SIGMA_NORMAL), abi.RT_TEMPORAL_HIT_MIN)
    assert temporal.resolve(START) == (32, 0.02, 0.35, 0.75)
    assert temporal.resolve(dict(max_history=5, sigma_depth=-1, sigma_normal=-2, hit_min=-1)) == (5, None, None, -1)
    with pytest.raises(ValueError):
        temporal.resolve(dict(max_history=-1))
    with pytest.raises(KeyError):
        abi.temporal_params(dict(sigma_colour=1.0))
    f, rgb, scale, guides, g = random_case()
    f = camera(f)
    hist = history_of(rgb, 1.0, guides, g)
    with pytest.raises(ValueError):
        NumpyOps().temporal(f, rgb, scale, None, 4, guides, 0)
    with pytest.raises(ValueError):
        NumpyOps().temporal(f, rgb, scale, None, 4, guides, g, f, None)
    with pytest.raises(ValueError):
        NumpyOps().temporal(f, rgb, scale, None, 4, guides, g, camera(frame_of(W, H + 1)), hist)
    # each test switched off admits what it refused
    fA, fB, gA, gB, idA, idB = occluder_case()
    hist = history_of(np.ones((PH, PW, 3)), 8.0, gA, PG)
    on = NumpyOps().temporal(fB, np.zeros((PH, PW, 3)), 1.0, None, 1, gB, PG, fA, hist, START)[1][0][..., 3]
    off = NumpyOps().temporal(fB, np.zeros((PH, PW, 3)), 1.0, None, 1, gB, PG, fA, hist,
                              dict(START, sigma_depth=-1))[1][0][..., 3]
    assert (off > on).sum() >= 20 and not (off < on).any()


# ---- the host twin -------------------------------------------------------------------
_emu = None


def temporal_emu():
    """tests/native/build/libtemporal_emu.so (built on first use: temporal.mk)."""
    global _emu
    if _emu is None:
        subprocess.run(["make", "-s", "-C", NATIVE, "-f", "temporal.mk"], check=True)
        L = C.CDLL(os.path.join(NATIVE, "build", "libtemporal_emu.so"))
        L.emu_history_bytes.restype = C.c_int64
        L.emu_history_bytes.argtypes = [C.POINTER(abi.Frame)]
        L.emu_temporal.argtypes = [C.POINTER(abi.Frame), C.c_void_p, C.c_double, C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_int32, C.POINTER(abi.Frame), C.c_void_p, C.POINTER(abi.TemporalParams),
                                   C.c_void_p, C.c_void_p]
        _emu = L
    return _emu


def host_temporal(f, rgb, scale, tile_strata, strata_now, guides, g, f_prev=None, hist=None, params=None):
    """rt_temporal.h on the host -> (out, (col, geo))."""
    L = temporal_emu()
    assert L.emu_history_bytes(C.byref(f)) == temporal.history_bytes(f)
    rgb, guides = np.ascontiguousarray(rgb, dtype=np.float64), np.ascontiguousarray(guides, dtype=np.float64)
    ts = np.ascontiguousarray(tile_strata, dtype=np.int32) if tile_strata is not None else None
    prev = temporal.pack_history(f, hist) if hist is not None else None
    h_out = np.zeros(temporal.history_bytes(f), dtype=np.uint8)
    out = np.zeros_like(rgb)
    p = abi.temporal_params(params)
    rc = L.emu_temporal(C.byref(f), rgb.ctypes.data, scale, ts.ctypes.data if ts is not None else None, strata_now,
                        guides.ctypes.data, g, C.byref(f_prev) if f_prev is not None else None,
                        prev.ctypes.data if prev is not None else None, C.byref(p) if p is not None else None,
                        h_out.ctypes.data, out.ctypes.data)
    assert rc == 0
    return out, temporal.unpack_history(f, h_out)


def assert_matches_numpy(got, ref, what, worst=None):
    """`got` = (out, (col, geo)) against NumpyOps' (out, (col, geo), margin):
    out within 1e-9 max(|numpy|, mean |numpy|) per channel, the history planes
    within one fp32 ulp; pixels on a threshold (margin < 1e-6) are left out,
    and they are at most 0.5 % of the frame."""
    out, (col, geo) = got
    r_out, (r_col, r_geo), margin = ref
    use = margin >= 1e-6
    share = 1.0 - use.mean()
    assert share <= 0.005, "%s: %.3f %% of the pixels sit on a threshold" % (what, 100 * share)
    assert np.array_equal(np.isfinite(out), np.isfinite(r_out)), what
    fin = np.isfinite(r_out)
    mean = np.array([np.abs(r_out[..., c][fin[..., c]]).mean() for c in range(3)])
    bound = np.maximum(np.abs(r_out), np.maximum(mean, 1e-300)[None, None, :])
    m = fin & use[..., None]
    ratio = float((np.abs(out - r_out)[m] / bound[m]).max()) / 1e-9
    ulps = 0.0
    for a, b in ((col, r_col), (geo, r_geo)):
        a, b = a[use].astype(np.float64), b[use].astype(np.float64)
        assert np.array_equal(np.isfinite(a), np.isfinite(b)), what
        ok = np.isfinite(b)
        ulps = max(ulps, float((np.abs(a - b)[ok] / np.maximum(np.abs(b[ok]), 1e-300)).max()) / ULP32)
    if worst is not None:
        worst["out"], worst["ulp"] = max(worst["out"], ratio), max(worst["ulp"], ulps)
    print("temporal %-30s on a threshold %.4f %%; |out diff| / bound = %.3g, history %.3g ulp (limits 1, 1)"
          % (what, 100 * share, ratio, ulps))
    assert ratio <= 1.0 and ulps <= 1.0, what


def moved_random_case(seed=11):
    """test_denoise.random_case seen from pose B with a history taken at pose A
    (a lateral step and a yaw), so that the footprints meet the normal edge, the
    depth step, the sky, the silhouette row and every image border."""
    f, rgb, scale, guides, g = random_case(seed)
    fA, fB = camera(f), camera(f, center=(0.35, 0.02, 0.0), yaw=0.04)
    rng = np.random.default_rng(seed + 1)
    e_hist = rng.uniform(0.0, 3.0, (H, W, 3))
    e_hist[7, 30, 0] = np.nan
    count = rng.uniform(0.0, 40.0, (H, W)) * (rng.uniform(size=(H, W)) > 0.05)
    return fA, fB, rgb, scale, guides, g, history_of(e_hist, count, guides, g)


def random_cases(fA, fB, hist, strata):
    """label -> (frame, tile strata, frame_prev, history_prev, params) on the moved random case."""
    return {
        "moved": (fB, None, fA, hist, START),
        "defaults": (fB, None, fA, hist, None),
        "identity": (fA, None, fA, hist, START),
        "no history": (fB, None, None, None, None),
        "tile strata": (fB, strata, fA, hist, START),
        "in place": (fB, None, fA, hist, START),
        "depth off": (fB, None, fA, hist, dict(START, sigma_depth=-1)),
        "normal off": (fB, None, fA, hist, dict(START, sigma_normal=-1)),
        "hit_min off, cap 5": (fB, None, fA, hist, dict(START, hit_min=-1, max_history=5)),
    }


def test_host_twin_matches_numpy_on_the_moved_random_case():
    fA, fB, rgb, scale, guides, g, hist = moved_random_case()
    tx, ty = (W + 7) // 8, (H + 7) // 8
    strata = ((np.arange(tx * ty) * 7) % 6).astype(np.int32)
    cases = random_cases(fA, fB, hist, strata)
    for what, (f, ts, fp, hp, params) in cases.items():
        ref = NumpyOps().temporal(f, rgb, scale, ts, g, guides, g, fp, hp, params)
        assert_matches_numpy(host_temporal(f, rgb, scale, ts, g, guides, g, fp, hp, params), ref, what)
    # teeth: the move keeps history at some pixels and refuses it at others, by either test
    n_h = NumpyOps().temporal(fB, rgb, scale, None, g, guides, g, fA, hist, START)[1][0][..., 3] - g
    assert 0.2 < (n_h > 0.5).mean() < 0.95
    for off in ("sigma_depth", "sigma_normal"):
        n_off = NumpyOps().temporal(fB, rgb, scale, None, g, guides, g, fA, hist, dict(START, **{off: -1}))[1][0]
        assert (n_off[..., 3] - g > n_h + 0.5).any(), off


@pytest.mark.parametrize("tilt", [0.0, 70.0])
def test_host_twin_matches_numpy_on_the_planes(tilt):
    fA, fB, gA, gB, _ = plane_case(tilt)
    rng = np.random.default_rng(2)
    hist = history_of(rng.uniform(0.0, 3.0, (PH, PW, 3)), 9.0, gA, PG)
    rgb = rng.uniform(0.0, 2.0, (PH, PW, 3)) * PG
    ref = NumpyOps().temporal(fB, rgb, 1.0 / PG, None, PG, gB, PG, fA, hist, START)
    assert_matches_numpy(host_temporal(fB, rgb, 1.0 / PG, None, PG, gB, PG, fA, hist, START), ref, "plane %g" % tilt)
    fA, fB, gA, gB, idA, idB = occluder_case()
    for params in (None, START):
        ref = NumpyOps().temporal(fB, rgb, 1.0 / PG, None, PG, gB, PG, fA, hist, params)
        assert_matches_numpy(host_temporal(fB, rgb, 1.0 / PG, None, PG, gB, PG, fA, hist, params), ref, "occluder")


# ---- ABI (no device call is reached) -------------------------------------------------------
def test_history_bytes():
    L = load()
    f = frame_of(36, 35)
    n = C.c_int64(-1)
    assert L.rt_history_bytes(C.byref(f), C.byref(n)) == abi.RT_OK
    assert n.value % 512 == 0 and n.value >= 32 * 36 * 35 and n.value == temporal.history_bytes(f)
    assert temporal.history_bytes(frame_of(3, 3)) == 512
    assert L.rt_history_bytes(C.byref(f), None) == abi.RT_ERR_INVALID and b"null" in L.rt_last_error()
    assert L.rt_history_bytes(C.byref(frame_of(0, 36)), C.byref(n)) == abi.RT_ERR_INVALID
    assert L.rt_history_bytes(None, C.byref(n)) == abi.RT_ERR_INVALID and b"frame" in L.rt_last_error()
    col = np.arange(36 * 35 * 4, dtype=np.float32).reshape(35, 36, 4)
    back = temporal.unpack_history(f, temporal.pack_history(f, (col, -col)))
    assert np.array_equal(back[0], col) and np.array_equal(back[1], -col)


def test_temporal_refusals_before_any_device_call():
    L = load()
    f = camera(frame_of(36, 36))
    # addresses that are never dereferenced: every call below is refused on its arguments
    rgb, guides, hp, ho, out = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
    hb = temporal.history_bytes(f)
    NONE = object()

    def call(rgb=rgb, guides=guides, hp=hp, ho=ho, out=out, g=4, strata=4, params=None, frame=f, prev=f):
        p = abi.temporal_params(params)
        return L.rt_temporal_device(C.byref(frame) if frame is not NONE else None, C.c_void_p(rgb), 1.0, None,
                                    strata, C.c_void_p(guides), g, C.byref(prev) if prev is not NONE else None,
                                    C.c_void_p(hp), C.byref(p) if p is not None else None, C.c_void_p(ho),
                                    C.c_void_p(out), None)

    cases = {
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
        "history_out inside history_prev": (dict(ho=hp + hb - 256), b"overlaps device_history_prev"),
        "out inside history_out": (dict(out=ho + 256), b"overlaps a history"),
        "out inside history_prev": (dict(out=hp + 8), b"overlaps a history"),
        "max_history -1": (dict(params=dict(max_history=-1)), b"max_history"),
        "NaN sigma": (dict(params=dict(sigma_depth=float("nan"))), b"NaN"),
    }
    for what, (kw, word) in cases.items():
        assert call(**kw) == abi.RT_ERR_INVALID, what
        assert word in L.rt_last_error(), (what, L.rt_last_error())


def test_temporal_params_mirror_and_defaults_match_the_header(tmp_path):
    """rt_temporal_params as gcc lays it out, and the RT_TEMPORAL_* defaults the
    Python side restates (rtx/abi.py)."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_api.h"', "int main(void) {",
             'printf("%zu\\n", sizeof(rt_temporal_params));']
    want = [C.sizeof(abi.TemporalParams)]
    for name, _ in abi.TemporalParams._fields_:
        lines.append('printf("%%zu\\n", offsetof(rt_temporal_params, %s));' % name)
        want.append(getattr(abi.TemporalParams, name).offset)
    consts = ["RT_TEMPORAL_MAX_HISTORY", "RT_TEMPORAL_SIGMA_DEPTH", "RT_TEMPORAL_SIGMA_NORMAL",
              "RT_TEMPORAL_HIT_MIN", "RT_ABI_VERSION"]
    for c in consts:
        lines.append('printf("%%.17g\\n", (double)%s);' % c)
        want.append(float(getattr(abi, c)))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", HEADER_DIR, str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [float(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [float(x) for x in want]
    assert abi.RT_ABI_VERSION == 5


def test_exports():
    L = load()
    for name in ("rt_history_bytes", "rt_temporal_device"):
        assert name in abi.EXPORTS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None
