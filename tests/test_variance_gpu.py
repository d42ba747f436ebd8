"""rt_denoise_variance_device on gfx950 against rtx.denoise.NumpyOps.denoise_variance,
and the variance-guided display end to end.

Tolerance against NumpyOps (fp64), for the image per channel and for the
variance plane: |gpu - numpy| <= 1e-4 max(|numpy|, mean |numpy|) -- the bound
of tests/test_denoise_gpu.py, whose terms are all still here (fp32 planes, one
native exponential per tap: about 4e-5 over 25 taps and 8 passes).  What the
luminance term adds: its exponent |dy| / s, s = sigma_l
sqrt(v~) + 1e-6, carries the fp32 rounding of y, an absolute error delta of
about 4e-7 y, so a tap's weight is off by w delta / s; since
w |dy| / s <= 1 / e whatever s is, a pass moves the normalised sum by about
5 delta where the colour follows the luminance -- 2e-6, 1.5e-5 over 8 passes
-- and by (delta / s) |de| where it does not: with the variances of these
cases (s >= 0.02) at most 4e-5 for one tap and far less summed over signed
taps.  The variance plane starts within 1e-5 (fp64 moments rounded once; the
spatial sums are of y_q - y_p) and gathers twice a weight's relative error per
pass.  The sum stays below 1e-4.  Largest ratio observed over every case
below: 2.0e-5 (the variance plane of the 4-strata display frame), 5.4e-6 on
an image."""
import os

import numpy as np
import pytest
import torch

from rtx import abi, adaptive, progressive
from rtx.denoise import DenoisedDisplay, NumpyOps, VarianceGuidedDisplay
from rtx.ppm import to_bytes
from rtx.render import Renderer, camera_frame
from rtx.scene import load_scene
import oracle_lib as O
from test_denoise import random_case
from test_denoise_gpu import GuardedBytes, _cur, _dev, _ops
from test_guides import guide_frame
from test_variance import BATCH, QUALITY, TX, TY, VOFF, assert_quality, mixed_strata, random_moments, rmse

pytestmark = pytest.mark.gpu

PKG = os.path.join(O.ROOT, "real-time-ray-tracing-engine_amd")
worst = {"ratio": 0.0}


def gpu_variance(f, rgb, scale, tile_strata, guides, g, s1=None, s2=None, batch=0, params=None, in_place=False):
    """HipOps.denoise_variance between guards, run twice (bit-identical), inputs
    unmodified -> numpy ([H, W, 3] image, [H, W] variance)."""
    ops = _ops()
    h, w = f.image_height, f.image_width
    ws = GuardedBytes(ops.variance_workspace_bytes(f))
    ob, vb = GuardedBytes(h * w * 24), GuardedBytes(h * w * 8)
    out = ob.mid.view(torch.float64).view(h, w, 3)
    var = vb.mid.view(torch.float64).view(h, w)
    d_guides = _dev(guides)
    d_strata = _dev(tile_strata, torch.int32) if tile_strata is not None else None
    d_s1 = _dev(s1) if s1 is not None else None
    d_s2 = _dev(s2) if s2 is not None else None
    runs = []
    for _ in range(2):
        d_rgb = _dev(rgb)
        if in_place:
            out.copy_(d_rgb)
            d_rgb = out
        ops.denoise_variance(f, d_rgb, scale, d_strata, d_guides, g, d_s1, d_s2, batch, params, ws.mid, out, var)
        runs.append((out.cpu().numpy().copy(), var.cpu().numpy().copy()))
        if not in_place:
            assert np.array_equal(d_rgb.cpu().numpy(), rgb, equal_nan=True)  # the accumulator is only read
    assert np.array_equal(d_guides.cpu().numpy(), guides)
    if s1 is not None:
        assert np.array_equal(d_s1.cpu().numpy(), s1, equal_nan=True)
        assert np.array_equal(d_s2.cpu().numpy(), s2, equal_nan=True)
        assert np.array_equal(d_strata.cpu().numpy(), tile_strata)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(runs[0], runs[1])), "two runs differ"
    assert ws.guards_intact() and ob.guards_intact() and vb.guards_intact(), "guard overwritten"
    return runs[0]


def assert_close(got, ref, what):
    """|gpu - numpy| <= 1e-4 max(|numpy|, mean |numpy|) per channel; prints the largest ratio."""
    got, ref = (a[..., None] if a.ndim == 2 else a for a in (got, ref))
    assert np.array_equal(np.isfinite(got), np.isfinite(ref)), what
    ok = np.isfinite(ref)
    mean = np.array([np.abs(ref[..., c][ok[..., c]]).mean() for c in range(ref.shape[-1])])
    bound = np.maximum(np.abs(ref), mean[None, None, :])
    ratio = float((np.abs(got - ref)[ok] / bound[ok]).max())
    worst["ratio"] = max(worst["ratio"], ratio)
    print("variance gpu/numpy %-44s max |diff| / bound-base = %.3g (limit 1e-4; worst so far %.3g)"
          % (what, ratio, worst["ratio"]))
    assert ratio <= 1e-4, what


def check_case(what, f, rgb, scale, strata, guides, g, s1=None, s2=None, batch=0, params=None, in_place=False):
    ref = NumpyOps().denoise_variance(f, rgb, scale, strata, guides, g, s1, s2, batch, params, with_variance=True)
    got = gpu_variance(f, rgb, scale, strata, guides, g, s1, s2, batch, params, in_place)
    assert_close(got[0], ref[0], what + ", image")
    assert (got[1][np.isfinite(got[1])] >= 0).all()
    assert_close(got[1], ref[1], what + ", variance")
    return got, ref


RANDOM_PARAMS = {
    "defaults": None,
    "passes 1": dict(passes=1),
    "passes 8": dict(passes=8),  # step 128 exceeds the frame
    "no pass": dict(passes=-1),
    "plain blur": dict(VOFF),
    "normal only": dict(VOFF, sigma_normal=0.35),
    "depth only": dict(VOFF, sigma_depth=0.02),
    "hit only": dict(VOFF, sigma_hit=0.1),
    "luminance only": dict(VOFF, sigma_lum=2.0),
    "passes 3, luminance 4, min_batches 2": dict(sigma_lum=4.0, passes=3, min_batches=2),
}


@pytest.mark.parametrize("label", sorted(RANDOM_PARAMS))
def test_filter_on_random_data_matches_numpy(label):
    """Spatial only (no moments), and tiles of mixed batch counts, 0 included, with moments."""
    f, rgb, scale, guides, g = random_case()
    params = RANDOM_PARAMS[label]
    check_case(label + " / spatial", f, rgb, scale, None, guides, g, params=params)
    strata = mixed_strata()
    s1, s2 = random_moments(rgb, strata)
    check_case(label + " / mixed tiles", f, rgb, 99.0, strata, guides, g, s1, s2, BATCH, params)


def test_filter_with_moments_everywhere_in_place_and_non_finite_samples():
    f, rgb, scale, guides, g = random_case()
    strata = np.full(TX * TY, 16, dtype=np.int32)
    s1, s2 = random_moments(rgb, strata)
    for passes in (1, 5, 8):
        check_case("moments, passes %d" % passes, f, rgb, 1.0, strata, guides, g, s1, s2, BATCH, dict(passes=passes))
    # tile strata without moments: the per-tile scale, the spatial estimate
    check_case("tile strata, no moments", f, rgb, 1.0, mixed_strata(), guides, g)
    # device_out == device_rgb
    check_case("in place", f, rgb, 1.0, strata, guides, g, s1, s2, BATCH, None, in_place=True)
    check_case("in place, spatial", f, rgb, scale, None, guides, g, in_place=True)
    # NaN / inf samples and moments: replaced where a finite tap exists, kept where none does, v finite
    rgb[20, 30, 1] = np.nan
    rgb[2:11, 50:59] = np.nan
    rgb[28, 5, 0] = np.inf
    s1[20, 30] = s2[28, 5] = np.nan
    for moments in ((None, None, 0), (s1, s2, BATCH)):
        for params in (dict(passes=1), None):
            got, _ = check_case("non-finite %r moments %s" % (params, moments[2] > 0), f, rgb, 1.0 / 16, strata,
                                guides, g, *moments, params)
            assert np.isfinite(got[1]).all()


def test_luminance_term_off_is_rt_denoise_device_without_its_colour_term():
    f, rgb, scale, guides, g = random_case()
    strata = mixed_strata()
    s1, s2 = random_moments(rgb, strata)
    ops = _ops()
    for passes in (1, 5, 8):
        want = ops.denoise(f, _dev(rgb), 1.0, _dev(strata, torch.int32), _dev(guides), g,
                           dict(passes=passes, sigma_color=-1)).cpu().numpy()
        got, _ = gpu_variance(f, rgb, 1.0, strata, guides, g, s1, s2, BATCH, dict(passes=passes, sigma_lum=-1))
        assert_close(got, want, "luminance off against rt_denoise_device, passes %d" % passes)
        # both are instances of one pass template (rt_denoise.hip pass_kernel): the same arithmetic
        assert np.array_equal(got, want), "luminance off differs from rt_denoise_device, passes %d" % passes


@pytest.mark.parametrize("name", ["cornell_fog", "bouncing_seed42"])
def test_filter_on_real_renders_matches_numpy(name):
    """36x36 (ragged tiles, fog) and 72x40: 4 batches of 2 strata of the render,
    its real guides and moments, the defaults; from moments and spatial only."""
    S, f = guide_frame(name, samples_per_pixel=16)
    h, w = f.image_height, f.image_width
    with Renderer(S) as R:
        ar = adaptive.for_renderer(R, f, seed=9, threshold=0.0, batch_strata=2)
        for _ in range(4):
            ar.step()
        guides = torch.zeros((h, w, abi.RT_GUIDE_CHANNELS), dtype=torch.float64, device="cuda")
        R.render_guides_device(f, guides.data_ptr(), _cur().cuda_stream, seed=9, samples=(0, 8), accumulate=0)
        rgb, guides, strata = ar.acc.cpu().numpy(), guides.cpu().numpy(), ar.tile_strata.cpu().numpy()
        s1, s2 = ar.s1.cpu().numpy(), ar.s2.cpu().numpy()
    assert (strata == 8).all()
    got, ref = check_case(name + " moments", f, rgb, 1.0, strata, guides, 8, s1, s2, 2)
    assert np.abs(ref[0] - rgb / 8).max() > 1e-3  # the filter did something
    check_case(name + " spatial", f, rgb, 1.0 / 8, None, guides, 8)


def test_variance_guided_display_end_to_end_on_the_cornell_box():
    """The three quality assertions of tests/test_variance.py on the device,
    and what the display promises about the renderer it wraps."""
    S = load_scene(os.path.join(PKG, "scenes", "cornell.json"))

    def frame_fn(spp):
        return camera_frame(S.camera_desc(image_width=64, aspect_ratio=1.0, samples_per_pixel=spp, max_depth=8))

    rows = []
    with Renderer(S) as R:
        ref = R.render(frame_fn(4096), seed=1234)  # another seed
        f4 = frame_fn(4)
        before = R.render(f4, seed=9)
        for strata, batches in QUALITY:
            f, bs = frame_fn(strata), strata // batches
            alone = adaptive.for_renderer(R, f, seed=5, threshold=0, batch_strata=bs)
            while not alone.done:
                alone.step()
            ar = adaptive.for_renderer(R, f, seed=5, threshold=0, batch_strata=bs)
            vd = VarianceGuidedDisplay(ar)
            while not vd.converged:
                assert vd.step() == bs
                vd.image()  # a display frame per batch: it must not disturb the accumulation
            assert vd.samples_taken == strata and vd.guides_done == min(16, strata)
            # the wrapped accumulator and moments are the renderer's run alone, bit for bit
            for a, b in ((ar.acc, alone.acc), (ar.s1, alone.s1), (ar.s2, alone.s2), (ar.tile_strata, alone.tile_strata)):
                assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
            img = vd.image().cpu().numpy()
            shipped = vd.ops.denoise(f, ar.acc, 1.0, ar.tile_strata, vd.guides, vd.guides_done).cpu().numpy()
            want = NumpyOps().denoise_variance(f, ar.acc.cpu().numpy(), 1.0, ar.tile_strata.cpu().numpy(),
                                               vd.guides.cpu().numpy(), vd.guides_done, ar.s1.cpu().numpy(),
                                               ar.s2.cpu().numpy(), bs, with_variance=True)
            assert_close(img, want[0], "display %d strata, image" % strata)
            assert_close(vd.variance().cpu().numpy(), want[1], "display %d strata, variance" % strata)
            spatial = vd.ops.denoise_variance(f, ar.acc, 1.0, ar.tile_strata, vd.guides, vd.guides_done).cpu().numpy()
            rows.append((strata, rmse(ar.image().cpu().numpy(), ref), rmse(shipped, ref), rmse(img, ref),
                         rmse(spatial, ref)))
        assert_quality(rows, "cornell 64x64 (gfx950)")
        # a render frame taken before and after: the display left the scene as it was
        assert np.array_equal(R.render(f4, seed=9), before)
        # bytes() is rt_to_bytes_device of image(); DisplayPipeline(bytes_fn) delivers the same
        want = to_bytes(img)
        assert np.array_equal(vd.bytes().cpu().numpy(), want)
        vd.reset()
        assert vd.guides_done == 0 and vd.samples_taken == 0
        for a in (vd.guides, vd.var, ar.acc, ar.s1, ar.s2, ar.tile_strata):
            assert float(a.abs().sum()) == 0.0
        pipe = progressive.DisplayPipeline(vd, bytes_fn=vd.bytes_into)
        while not vd.converged:
            pipe.frame(2)
        assert np.array_equal(pipe.flush().numpy(), want)
        # DenoisedDisplay over the same renderer is what it was: the shipped filter
        dd = DenoisedDisplay(ar)
        assert np.array_equal(dd.image().cpu().numpy(), shipped)


def test_variance_guided_display_over_a_progressive_renderer_is_the_spatial_statement():
    S, f = guide_frame("cornell", samples_per_pixel=16)
    with Renderer(S) as R:
        vd = VarianceGuidedDisplay(progressive.for_renderer(R, f, seed=5), guide_strata=6, params=dict(passes=3))
        assert vd.step(4) == 4 and vd.step(4) == 4 and vd.guides_done == 6
        img = vd.image().cpu().numpy()
        ref = NumpyOps().denoise_variance(f, vd.pr.acc.cpu().numpy(), 1.0 / 8, None, vd.guides.cpu().numpy(), 6,
                                          params=dict(passes=3), with_variance=True)
        assert_close(img, ref[0], "progressive display, image")
        assert_close(vd.variance().cpu().numpy(), ref[1], "progressive display, variance")
        assert np.array_equal(vd.bytes().cpu().numpy(), to_bytes(img))
        vd.reset()
        assert vd.guides_done == 0 and float(vd.guides.abs().sum()) == 0.0 and float(vd.var.abs().sum()) == 0.0
