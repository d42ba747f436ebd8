"""The variance-guided display filter's statement of record
(rtx.denoise.NumpyOps.denoise_variance), the ABI's argument checks, and what
the filter is for: an error that keeps falling as the samples arrive.  No GPU:
tests/test_variance_gpu.py holds the HIP kernels to NumpyOps."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from rtx import abi, adaptive, denoise
from rtx.cpu import CpuRenderer
from rtx.denoise import NumpyOps
from rtx.lib import load
from rtx.render import camera_frame
from rtx.scene import load_scene
import oracle_lib as O
from test_denoise import H, HEADER_DIR, W, frame_of, random_case
from test_guides import SCENES, host_guides

VOFF = dict(sigma_normal=-1, sigma_depth=-1, sigma_hit=-1, sigma_lum=-1)
TX, TY = (W + 7) // 8, (H + 7) // 8
BATCH = 2  # strata per batch of the random moments


def mixed_strata():
    """Tile strata of the 70 x 33 frame: 0, odd counts, and batch counts on both sides of min_batches = 4."""
    s = ((np.arange(TX * TY) * 5) % 13).astype(np.int32)
    b = s // BATCH
    assert (s == 0).any() and (b == 3).any() and (b == 4).any() and (b > 4).any() and (b == 1).any()
    return s


def random_moments(rgb, strata, seed=21, spread=0.2):
    """(s1, s2) of b = strata // BATCH batch means around the pixel's mean luminance."""
    rng = np.random.default_rng(seed)
    b = np.repeat(np.repeat((strata // BATCH).reshape(TY, TX), 8, 0), 8, 1)[:H, :W]
    n = np.repeat(np.repeat(np.maximum(1, strata).reshape(TY, TX), 8, 0), 8, 1)[:H, :W]
    mean = denoise.luminance(rgb) / n
    s1, s2 = np.zeros((H, W)), np.zeros((H, W))
    for k in range(int(b.max())):
        y = mean * (1.0 + spread * rng.normal(size=(H, W)))
        s1 += np.where(k < b, y, 0.0)
        s2 += np.where(k < b, y * y, 0.0)
    return s1, s2


def test_a_constant_image_stays_constant_and_its_variance_is_zero():
    f, rgb, scale, guides, g = random_case()
    guides[..., 0:3] = g  # albedo 1 everywhere: e = c
    rgb[...] = 0.37 * g
    for passes in (-1, 1, 5, 8):
        out, v = NumpyOps().denoise_variance(f, rgb, scale, None, guides, g, params=dict(passes=passes),
                                             with_variance=True)
        np.testing.assert_allclose(out, 0.37, rtol=1e-12, atol=0)
        assert (v == 0).all()


def test_zero_variance_moments_let_every_pixel_go():
    """s2 = s1^2 / b, b >= min_batches: v = 0, every unequal neighbour is cut
    to exp(-80), the output is the input."""
    f, rgb, scale, guides, g = random_case()
    strata = np.full(TX * TY, 16, dtype=np.int32)
    b = 16 // BATCH
    s1 = denoise.luminance(rgb) / 16 * b
    s2 = s1 * s1 / b
    out, v = NumpyOps().denoise_variance(f, rgb, 1.0, strata, guides, g, s1, s2, BATCH, None, with_variance=True)
    np.testing.assert_allclose(out, rgb / 16, rtol=1e-12, atol=0)
    assert v.max() <= 1e-25 and (v >= 0).all()  # (s2 - s1^2 / b) is rounding, if anything
    # the same frame without moments is filtered
    out = NumpyOps().denoise_variance(f, rgb, 1.0, strata, guides, g)
    assert np.abs(out - rgb / 16).max() > 1e-3


def test_luminance_term_off_is_the_shipped_filter_without_its_colour_term():
    f, rgb, scale, guides, g = random_case()
    strata = mixed_strata()
    s1, s2 = random_moments(rgb, strata)
    for passes in (0, 1, 8):
        ref = NumpyOps().denoise(f, rgb, scale, None, guides, g, dict(passes=passes, sigma_color=-1))
        out = NumpyOps().denoise_variance(f, rgb, scale, None, guides, g, params=dict(passes=passes, sigma_lum=-1))
        np.testing.assert_allclose(out, ref, rtol=1e-12, atol=0)
    ref = NumpyOps().denoise(f, rgb, 1.0, strata, guides, g, dict(sigma_color=-1))
    out = NumpyOps().denoise_variance(f, rgb, 1.0, strata, guides, g, s1, s2, BATCH, dict(sigma_lum=-1))
    np.testing.assert_allclose(out, ref, rtol=1e-12, atol=0)


def test_too_few_batches_is_the_spatial_estimate():
    f, rgb, scale, guides, g = random_case()
    strata = np.full(TX * TY, 3 * BATCH + 1, dtype=np.int32)  # 3 batches and a short one
    s1, s2 = random_moments(rgb, strata)
    a = NumpyOps().denoise_variance(f, rgb, 1.0, strata, guides, g, s1, s2, BATCH, None, with_variance=True)
    b = NumpyOps().denoise_variance(f, rgb, 1.0, strata, guides, g, with_variance=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # ... and min_batches = 3 (or anything below 2 with one batch more than one) switches the moments on
    c = NumpyOps().denoise_variance(f, rgb, 1.0, strata, guides, g, s1, s2, BATCH, dict(min_batches=3))
    assert not np.array_equal(c, b[0])
    d = NumpyOps().denoise_variance(f, rgb, 1.0, strata, guides, g, s1, s2, BATCH, dict(min_batches=-5))
    e = NumpyOps().denoise_variance(f, rgb, 1.0, strata, guides, g, s1, s2, BATCH, dict(min_batches=2))
    assert np.array_equal(d, e)


def test_mixed_tiles_take_each_path_per_tile():
    f, rgb, scale, guides, g = random_case()
    strata = mixed_strata()
    s1, s2 = random_moments(rgb, strata)
    ops = NumpyOps()
    passes, mb, sn, sz, sh, sl = denoise.resolve_variance(dict(passes=-1))
    assert (passes, mb, sl) == (0, abi.RT_DENOISE_MIN_BATCHES, abi.RT_DENOISE_SIGMA_LUM)
    _, v = ops.denoise_variance(f, rgb, 1.0, strata, guides, g, s1, s2, BATCH, dict(passes=-1), with_variance=True)
    e, a_d, n, z, h = ops.prepare(f, rgb, 1.0, strata, guides, g)
    spatial = ops.spatial_variance(e, n, z, h, sn, sz, sh)
    by_tile = np.repeat(np.repeat((strata // BATCH).reshape(TY, TX), 8, 0), 8, 1)[:H, :W]
    use = by_tile >= mb
    assert use.any() and (~use).any()
    np.testing.assert_array_equal(v[~use], spatial[~use])
    fb = by_tile[use].astype(np.float64)
    want = np.maximum(0.0, (s2[use] - s1[use] ** 2 / fb) / (fb - 1)) / fb / denoise.luminance(a_d)[use] ** 2
    np.testing.assert_allclose(v[use], want, rtol=1e-14, atol=0)
    assert (v[use] > 0).all() and np.abs(v[use] / spatial[use] - 1).min() > 1e-6  # the two paths differ


def test_spatial_variance_is_the_window_variance():
    """Every geometric term off: the plain variance of y over the clipped 7 x 7 window."""
    f, rgb, scale, guides, g = random_case()
    _, v = NumpyOps().denoise_variance(f, rgb, scale, None, guides, g, params=dict(VOFF, passes=-1),
                                       with_variance=True)
    e = rgb * scale / np.maximum(guides[..., 0:3] / g, 0.01)
    y = denoise.luminance(e)
    for j, i in ((0, 0), (16, 35), (H - 1, W - 2), (2, 41)):
        win = y[max(0, j - 3):j + 4, max(0, i - 3):i + 4]
        np.testing.assert_allclose(v[j, i], win.var(), rtol=1e-10)


def test_a_nan_sample_does_not_spread_and_the_variance_stays_finite():
    f, rgb, scale, guides, g = random_case()
    rgb[20, 30, 1] = np.nan        # one NaN in a finite neighbourhood
    rgb[2:11, 50:59] = np.nan      # a 9 x 9 block: its centre's 25 taps (step 1) are all NaN
    rgb[28, 5, 0] = np.inf
    strata = np.full(TX * TY, 16, dtype=np.int32)
    s1, s2 = random_moments(np.nan_to_num(rgb, nan=1.0, posinf=1.0), strata)
    s1[20, 30] = s2[28, 5] = np.nan  # moments of a NaN delta
    for moments in ((None, None, 0), (s1, s2, BATCH)):
        for params in (dict(VOFF, passes=1), dict(passes=1), None):
            out, v = NumpyOps().denoise_variance(f, rgb, 1.0 / 16, strata, guides, g, *moments, params,
                                                 with_variance=True)
            bad_in, bad_out = ~np.isfinite(rgb).all(-1), ~np.isfinite(out).all(-1)
            assert not (bad_out & ~bad_in).any()                   # nothing finite went bad
            assert np.isfinite(out[20, 30]).all() and np.isfinite(out[28, 5]).all()
            if params is not None:
                assert bad_out[4:9, 52:57].all() and bad_out.sum() == 25  # all taps NaN: the pixel keeps its NaN
            assert np.isfinite(v).all() and (v >= 0).all()
            assert (v[bad_out] == 0).all()


def test_params_resolution_and_refusals():
    assert denoise.resolve_variance(None) == (5, 4, abi.RT_DENOISE_SIGMA_NORMAL, abi.RT_DENOISE_SIGMA_DEPTH,
                                              abi.RT_DENOISE_SIGMA_HIT, abi.RT_DENOISE_SIGMA_LUM)
    assert denoise.resolve_variance(dict(passes=-3, min_batches=1, sigma_lum=-1))[0:2] == (0, 2)
    assert denoise.resolve_variance(dict(sigma_lum=-1))[5] is None
    assert denoise.resolve_variance(dict(sigma_lum=2.5, min_batches=9))[1::4] == (9, 2.5)
    with pytest.raises(ValueError):
        denoise.resolve_variance(dict(passes=9))
    with pytest.raises(KeyError):
        abi.denoise_variance_params(dict(sigma_color=1.0))
    f, rgb, scale, guides, g = random_case()
    strata = mixed_strata()
    s1, s2 = random_moments(rgb, strata)
    ops = NumpyOps()
    for bad in (dict(guide_strata=0), dict(s1=s1), dict(s2=s2), dict(s1=s1, s2=s2, batch_strata=0),
                dict(s1=s1, s2=s2, batch_strata=2, tile_strata=None)):
        kw = dict(frame=f, rgb=rgb, scale=1.0, tile_strata=strata, guides=guides, guide_strata=g)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.denoise_variance(**kw)


# ---- ABI (no device call is reached) ----------------------------------------
def test_workspace_bytes():
    L = load()
    f = frame_of(36, 36)
    n = C.c_int64(-1)
    assert L.rt_denoise_variance_workspace_bytes(C.byref(f), C.byref(n)) == abi.RT_OK
    assert n.value % 256 == 0 and n.value >= 68 * 36 * 36
    assert n.value == NumpyOps().variance_workspace_bytes(f) == 4 * 20736 + 5376
    assert L.rt_denoise_variance_workspace_bytes(C.byref(f), None) == abi.RT_ERR_INVALID
    assert L.rt_denoise_variance_workspace_bytes(C.byref(frame_of(0, 36)), C.byref(n)) == abi.RT_ERR_INVALID


def test_refusals_before_any_device_call():
    L = load()
    f = frame_of(36, 36)
    # addresses that are never dereferenced: every call below is refused on its arguments
    rgb, guides, ws, out, strata, s1, s2, var = (0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000,
                                                 0x60000000, 0x70000000, 0x80000000)

    def call(rgb=rgb, guides=guides, ws=ws, out=out, g=4, strata=strata, s1=s1, s2=s2, batch=2, var=var,
             params=None, frame=f):
        p = abi.denoise_variance_params(params)
        return L.rt_denoise_variance_device(C.byref(frame), C.c_void_p(rgb), 1.0, C.c_void_p(strata),
                                            C.c_void_p(guides), g, C.c_void_p(s1), C.c_void_p(s2), batch,
                                            C.byref(p) if p is not None else None, C.c_void_p(ws), C.c_void_p(out),
                                            C.c_void_p(var), None)

    nan = float("nan")
    cases = {
        # everything rt_denoise_device refuses
        "passes 9": dict(params=dict(passes=9)),
        "guide_strata 0": dict(g=0),
        "null rgb": dict(rgb=0),
        "null guides": dict(guides=0),
        "null workspace": dict(ws=0),
        "null out": dict(out=0),
        "unaligned workspace": dict(ws=ws + 8),
        "out inside the workspace": dict(out=ws + 256),
        "empty frame": dict(frame=frame_of(36, 0)),
        # ... and this function's own
        "s1 without s2": dict(s2=0),
        "s2 without s1": dict(s1=0),
        "moments without tile strata": dict(strata=0),
        "moments with batch_strata 0": dict(batch=0),
        "variance inside the workspace": dict(var=ws + 4 * 20736),  # the h plane
        "variance ending in the workspace": dict(var=ws - 8),
        "variance inside the output": dict(var=out + 1024),
        "NaN sigma_lum": dict(params=dict(sigma_lum=nan)),
        "NaN sigma_normal": dict(params=dict(sigma_normal=nan)),
        "NaN sigma_depth": dict(params=dict(sigma_depth=nan)),
        "NaN sigma_hit": dict(params=dict(sigma_hit=nan)),
    }
    for what, kw in cases.items():
        assert call(**kw) == abi.RT_ERR_INVALID, what
        assert L.rt_last_error(), what


def test_params_mirror_and_defaults_match_the_header(tmp_path):
    """rt_denoise_variance_params as gcc lays it out, and the defaults rtx/abi.py restates."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_api.h"', "int main(void) {",
             'printf("%zu\\n", sizeof(rt_denoise_variance_params));']
    want = [C.sizeof(abi.DenoiseVarianceParams)]
    for name, _ in abi.DenoiseVarianceParams._fields_:
        lines.append('printf("%%zu\\n", offsetof(rt_denoise_variance_params, %s));' % name)
        want.append(getattr(abi.DenoiseVarianceParams, name).offset)
    for c in ("RT_DENOISE_SIGMA_LUM", "RT_DENOISE_MIN_BATCHES", "RT_ABI_VERSION"):
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
    for name in ("rt_denoise_variance_workspace_bytes", "rt_denoise_variance_device"):
        assert name in abi.EXPORTS and hasattr(load(), name)


# ---- quality: the filter lets go as the estimate converges -------------------
QUALITY = ((4, 4), (16, 8), (64, 8), (256, 16))  # (strata, batches)


def rmse(img, ref):
    return float(np.sqrt(np.mean((np.clip(img, 0, 1) - np.clip(ref, 0, 1)) ** 2)))


def quality_rows(render, guides_fn, frame_fn, ref):
    """Per (strata, batches): RMSE raw / shipped filter / variance-guided from
    moments / spatial only.  render(frame, first, count) -> raw sums;
    guides_fn(frame, g) -> guide sums of strata [0, g)."""
    rows = []
    for strata, batches in QUALITY:
        f = frame_fn(strata)
        bs = strata // batches
        h, w = f.image_height, f.image_width
        tiles = np.arange(((w + 7) // 8) * ((h + 7) // 8), dtype=np.int32)
        acc, s1, s2 = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
        tile_strata = np.zeros(tiles.size, dtype=np.int32)
        for k in range(batches):  # folded as AdaptiveRenderer.step folds them
            adaptive.NumpyOps().update(render(f, k * bs, bs), bs, tiles, tiles.size, f, acc, s1, s2, tile_strata)
        g = min(strata, 16)
        guides = guides_fn(f, g)
        ops = NumpyOps()
        rows.append((strata, rmse(acc / strata, ref),
                     rmse(ops.denoise(f, acc, 1.0, tile_strata, guides, g), ref),
                     rmse(ops.denoise_variance(f, acc, 1.0, tile_strata, guides, g, s1, s2, bs), ref),
                     rmse(ops.denoise_variance(f, acc, 1.0, tile_strata, guides, g), ref)))
    return rows


def assert_quality(rows, what):
    """The three assertions of the feature, after printing every figure."""
    print("\n%s: RMSE against the reference, sigma_lum %g" % (what, abi.RT_DENOISE_SIGMA_LUM))
    print("strata      raw  shipped  variance-guided  spatial only")
    for r in rows:
        print("%6d  %.5f  %.5f  %.5f          %.5f" % r)
    raw, shipped, guided = ([r[i] for r in rows] for i in (1, 2, 3))
    assert guided[0] < raw[0], "4 strata: the filter must beat the raw frame"
    assert guided[3] < shipped[3], "256 strata: the filter must beat the shipped one"
    assert all(a > b for a, b in zip(guided, guided[1:])), "the error must fall with every count"


def test_the_error_falls_as_the_samples_arrive_on_the_cornell_box():
    """Cornell 64 x 64, depth 8, seed 5 against 4,096 strata of seed 1234, all
    on the host.  Measured at the shipped sigma_lum 4 (raw / shipped filter /
    variance-guided / spatial only): 4 strata 0.1159 / 0.0595 / 0.0558 /
    0.0702; 16: 0.0685 / 0.0527 / 0.0388 / 0.0523; 64: 0.0353 / 0.0532 /
    0.0300 / 0.0468; 256: 0.0188 / 0.0537 / 0.0226 / 0.0440.  (At 64 pixels
    the 256-strata frame is better left alone; sigma_lum is the 1080-pixel
    sweep's, where the filter still gains there: DESIGN.md §7f.)"""
    S = load_scene(os.path.join(SCENES, "cornell.json"))

    def frame_fn(spp):
        return camera_frame(S.camera_desc(image_width=64, aspect_ratio=1.0, samples_per_pixel=spp, max_depth=8))

    R = CpuRenderer(S)

    def render(f, first, count, seed=5, output=abi.RT_OUT_SUM):
        out = torch.zeros((f.image_height, f.image_width, 3), dtype=torch.float64)
        R.render_device(f, out.data_ptr(), seed=seed, samples=(first, count), output=output)
        return out.numpy()

    fr = frame_fn(4096)
    ref = render(fr, 0, 4096, seed=1234) / 4096.0
    rows = quality_rows(render, lambda f, g: host_guides(S, f, samples=(0, g), seed=5), frame_fn, ref)
    assert_quality(rows, "cornell 64x64 (host)")
