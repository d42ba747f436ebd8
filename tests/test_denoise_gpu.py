"""rt_denoise_device on gfx950 against rtx.denoise.NumpyOps, the denoised
display end to end, and rtx_render --denoise.

Tolerance of the filter against NumpyOps (fp64): per channel
|gpu - numpy| <= 1e-4 max(|numpy|, mean |numpy|).  The kernels hold e, n, z, h
as fp32 and take one native exponential per tap whose argument reaches 80: a
relative weight error of about 80 x 2^-24 = 5e-6; 25 normalised taps and at
most 8 passes make that about 4e-5; the bound leaves 2.5x."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from rtx import abi, adaptive, progressive
from rtx.denoise import DenoisedDisplay, HipOps, NumpyOps
from rtx.lib import load
from rtx.ppm import to_bytes
from rtx.render import Renderer, camera_frame
from rtx.scene import load_scene
import oracle_lib as O
from test_denoise import G, H, OFF, W, random_case
from test_guides import guide_frame

pytestmark = pytest.mark.gpu

PKG = os.path.join(O.ROOT, "real-time-ray-tracing-engine_amd")
CLI = os.path.join(PKG, "build", "rtx_render")
SENTINEL = -7.25
GUARD = 4096


def _cur():
    return torch.cuda.current_stream()


def _ops():
    return HipOps(torch.device("cuda", 0), _cur())


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


class GuardedBytes:
    """n bytes (256-B aligned start) between two sentinel-filled guards of GUARD doubles."""

    def __init__(self, n):
        self.n, self.g = n, 8 * GUARD
        self.all = torch.full((n + 2 * self.g,), 0xA5, dtype=torch.uint8, device="cuda")
        assert (self.all.data_ptr() + self.g) % 256 == 0
        self.mid = self.all[self.g:self.g + n]

    def guards_intact(self):
        a = self.all.cpu().numpy()
        return bool(np.all(a[:self.g] == 0xA5) and np.all(a[self.g + self.n:] == 0xA5))


def gpu_denoise(f, rgb, scale, tile_strata, guides, g, params, in_place=False):
    """HipOps.denoise between guards, run twice (bit-identical), -> numpy [H, W, 3]."""
    ops = _ops()
    h, w = f.image_height, f.image_width
    ws = GuardedBytes(ops.workspace_bytes(f))
    ob = GuardedBytes(h * w * 24)
    out = ob.mid.view(torch.float64).view(h, w, 3)
    d_guides = _dev(guides)
    d_strata = _dev(tile_strata, torch.int32) if tile_strata is not None else None
    runs = []
    for _ in range(2):
        d_rgb = _dev(rgb)
        if in_place:
            out.copy_(d_rgb)
            d_rgb = out
        ops.denoise(f, d_rgb, scale, d_strata, d_guides, g, params, ws.mid, out)
        runs.append(out.cpu().numpy().copy())
        if not in_place:
            assert np.array_equal(d_rgb.cpu().numpy(), rgb, equal_nan=True)  # the accumulator is only read
    assert np.array_equal(runs[0], runs[1], equal_nan=True), "two runs differ"
    assert ws.guards_intact() and ob.guards_intact(), "guard overwritten"
    return runs[0]


worst = {"ratio": 0.0}


def assert_close(got, ref, what):
    """|gpu - numpy| <= 1e-4 max(|numpy|, mean |numpy|) per channel; prints the largest ratio."""
    assert np.array_equal(np.isfinite(got), np.isfinite(ref)), what
    ok = np.isfinite(ref)
    mean = np.array([np.abs(ref[..., c][ok[..., c]]).mean() for c in range(3)])
    bound = np.maximum(np.abs(ref), mean[None, None, :])
    ratio = float((np.abs(got - ref)[ok] / bound[ok]).max())
    worst["ratio"] = max(worst["ratio"], ratio)
    print("denoise gpu/numpy %-34s max |diff| / bound-base = %.3g (limit 1e-4; worst so far %.3g)"
          % (what, ratio, worst["ratio"]))
    assert ratio <= 1e-4, what


@pytest.mark.parametrize("name", ["cornell_fog", "bouncing_seed42"])
def test_filter_on_real_renders_matches_numpy(name):
    """36x36 (ragged tiles, fog) and 72x40: 4 strata of the render, its real guides, the defaults."""
    S, f = guide_frame(name)
    h, w = f.image_height, f.image_width
    with Renderer(S) as R:
        rgb = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
        guides = torch.zeros((h, w, abi.RT_GUIDE_CHANNELS), dtype=torch.float64, device="cuda")
        st = _cur().cuda_stream
        R.render_device(f, rgb.data_ptr(), st, seed=9, samples=(0, 4), accumulate=0)
        R.render_guides_device(f, guides.data_ptr(), st, seed=9, samples=(0, 4), accumulate=0)
        rgb, guides = rgb.cpu().numpy(), guides.cpu().numpy()
    ref = NumpyOps().denoise(f, rgb, 0.25, None, guides, 4, None)
    assert_close(gpu_denoise(f, rgb, 0.25, None, guides, 4, None), ref, name + " defaults")
    assert np.abs(ref - rgb * 0.25).max() > 1e-3  # the filter did something


RANDOM_PARAMS = {
    "defaults": None,
    "passes 1": dict(passes=1),
    "passes 8": dict(passes=8),  # step 128 exceeds the frame
    "no pass": dict(passes=-1),
    "plain blur": dict(OFF),
    "normal only": dict(OFF, sigma_normal=0.35),
    "depth only": dict(OFF, sigma_depth=0.02),
    "hit only": dict(OFF, sigma_hit=0.1),
    "colour only": dict(OFF, sigma_color=4.0),
    "passes 3, colour 2": dict(sigma_color=2.0, passes=3),
}


@pytest.mark.parametrize("label", sorted(RANDOM_PARAMS))
def test_filter_on_random_data_matches_numpy(label):
    f, rgb, scale, guides, g = random_case()
    params = RANDOM_PARAMS[label]
    ref = NumpyOps().denoise(f, rgb, scale, None, guides, g, params)
    assert_close(gpu_denoise(f, rgb, scale, None, guides, g, params), ref, label)


def test_filter_with_tile_strata_in_place_and_non_finite_samples():
    f, rgb, scale, guides, g = random_case()
    tx, ty = (W + 7) // 8, (H + 7) // 8
    strata = ((np.arange(tx * ty) * 7) % 6).astype(np.int32)  # mixed counts, 0 included
    assert (strata == 0).any()
    ref = NumpyOps().denoise(f, rgb, 99.0, strata, guides, g, None)
    assert_close(gpu_denoise(f, rgb, 99.0, strata, guides, g, None), ref, "tile strata")
    # device_out == device_rgb
    ref = NumpyOps().denoise(f, rgb, scale, None, guides, g, None)
    assert_close(gpu_denoise(f, rgb, scale, None, guides, g, None, in_place=True), ref, "in place")
    # NaN / inf samples: replaced where a finite tap exists, kept where none does
    rgb[20, 30, 1] = np.nan
    rgb[2:11, 50:59] = np.nan
    rgb[28, 5, 0] = np.inf
    for params in (dict(passes=1), None):
        ref = NumpyOps().denoise(f, rgb, scale, None, guides, g, params)
        assert_close(gpu_denoise(f, rgb, scale, None, guides, g, params), ref, "non-finite %r" % (params,))


def _rmse(img, ref):
    return float(np.sqrt(np.mean((np.clip(img, 0, 1) - np.clip(ref, 0, 1)) ** 2)))


def test_denoised_display_beats_four_spp_noise_on_the_cornell_box():
    S = load_scene(os.path.join(PKG, "scenes", "cornell.json"))
    f4 = camera_frame(S.camera_desc(image_width=64, aspect_ratio=1.0, samples_per_pixel=4, max_depth=8))
    fr = camera_frame(S.camera_desc(image_width=64, aspect_ratio=1.0, samples_per_pixel=1024, max_depth=8))
    with Renderer(S) as R:
        ref = R.render(fr, seed=1234)  # 1,024 strata, another seed
        plain = progressive.for_renderer(R, f4, seed=5)
        plain.step(2)  # the same launches as below: another split of the strata regroups the fp64 sums
        plain.step(2)
        dd =DenoisedDisplay(progressive.for_renderer(R, f4, seed=5))
        assert dd.step(2) == 2 and dd.step(2) == 2 and dd.step(1) == 0 and dd.converged
        assert dd.guides_done == 4
        den = dd.image().cpu().numpy()
        raw = dd.pr.image().cpu().numpy()
        # the wrapped accumulator is a plain progressive run's, bit for bit
        assert np.array_equal(dd.pr.acc.cpu().numpy(), plain.acc.cpu().numpy(), equal_nan=True)
        e_raw, e_den = _rmse(raw, ref), _rmse(den, ref)
        print("cornell 64x64, 4 spp: RMSE raw %.5f, denoised %.5f, ratio %.3f" % (e_raw, e_den, e_den / e_raw))
        assert e_den < e_raw
        # bytes() is rt_to_bytes_device of image(); DisplayPipeline(bytes_fn) delivers the same
        want = to_bytes(den)
        assert np.array_equal(dd.bytes().cpu().numpy(), want)
        dd.reset()
        assert dd.guides_done == 0 and float(dd.guides.abs().sum()) == 0.0 and dd.samples_taken == 0
        pipe = progressive.DisplayPipeline(dd, bytes_fn=dd.bytes_into)
        while not dd.converged:
            pipe.frame(2)
        assert np.array_equal(pipe.flush().numpy(), want)
        # the default bytes_fn is unchanged: the raw frame's bytes
        pipe = progressive.DisplayPipeline(plain)
        pipe.frame()
        assert np.array_equal(pipe.flush().numpy(), to_bytes(plain.image().cpu().numpy()))


def test_denoised_display_over_an_adaptive_renderer():
    S, f = guide_frame("cornell_fog", samples_per_pixel=16)
    with Renderer(S) as R:
        ar = adaptive.for_renderer(R, f, seed=5, threshold=0.05, min_batches=2, batch_strata=2)
        dd = DenoisedDisplay(ar, guide_strata=6)
        while not dd.converged:
            dd.step()
        assert dd.guides_done == min(6, dd.samples_taken)
        img = dd.image().cpu().numpy()
        assert np.isfinite(img).all()
        assert np.array_equal(dd.bytes().cpu().numpy(), to_bytes(img))
        # against NumpyOps with the tiles' own scales
        ref = NumpyOps().denoise(f, ar.acc.cpu().numpy(), 1.0, ar.tile_strata.cpu().numpy(),
                                 dd.guides.cpu().numpy(), dd.guides_done, None)
        assert_close(img, ref, "adaptive display")
        dd.reset()
        assert dd.guides_done == 0 and float(dd.guides.abs().sum()) == 0.0
        assert float(ar.acc.abs().sum()) == 0.0


def _ppm(path):
    data = open(path).read().split()
    return data[:4], np.array([int(x) for x in data[4:]], dtype=np.int64)


def test_cli_denoise(tmp_path):
    """rtx_render --denoise writes rt_to_bytes_device of HipOps.denoise over the
    same frame, guides (every stratum) and defaults; without the flag the PPM
    is the raw frame's, as before."""
    path = os.path.join(PKG, "scenes", "cornell.json")
    S = load_scene(path)
    f = camera_frame(S.camera_desc(image_width=64, samples_per_pixel=16))
    h, w = f.image_height, f.image_width
    ops = _ops()
    with Renderer(S) as R:
        rgb = _dev(R.render(f, seed=5, output=abi.RT_OUT_SUM))
        guides = torch.zeros((h, w, abi.RT_GUIDE_CHANNELS), dtype=torch.float64, device="cuda")
        R.render_guides_device(f, guides.data_ptr(), _cur().cuda_stream, seed=5, samples=(0, 16), accumulate=0)
        raw = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
        assert load().rt_to_bytes_device(C.c_void_p(rgb.data_ptr()), h * w, f.pixel_samples_scale,
                                         C.c_void_p(raw.data_ptr()), C.c_void_p(_cur().cuda_stream)) == 0
        want = {(): raw.cpu().numpy().astype(np.int64).ravel()}
        for passes in (0, 2):
            img = ops.denoise(f, rgb, f.pixel_samples_scale, None, guides, 16, dict(passes=passes))
            want[passes] = ops.bytes(img).cpu().numpy().astype(np.int64).ravel()
    assert not np.array_equal(want[0], want[()]) and not np.array_equal(want[0], want[2])
    runs = {(): [], 0: ["--denoise"], 2: ["--denoise", "--denoise-passes", "2"]}
    for key, extra in runs.items():
        r = subprocess.run([CLI, "--scene", path, "--width", "64", "--samples", "16", "--seed", "5", "--output",
                            "t.ppm", *extra], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
        assert r.returncode == 0, r.stderr
        head, got = _ppm(tmp_path / "output" / "t.ppm")
        assert head == ["P3", str(w), str(h), "255"]
        assert np.array_equal(got, want[key]), extra
    for extra in (["--backend", "cpu"], ["--shards", "2"], ["--denoise-passes", "9"]):
        r = subprocess.run([CLI, "--scene", path, "--denoise", *extra], capture_output=True, text=True,
                           cwd=str(tmp_path), timeout=120)
        assert r.returncode == 2 and "denoise" in r.stderr, extra
