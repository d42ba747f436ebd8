"""The a-trous filter's statement of record (rtx.denoise.NumpyOps.denoise) and
the ABI's argument checks.  No GPU: tests/test_denoise_gpu.py holds the HIP
kernels to NumpyOps."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rtx import abi, denoise
from rtx.denoise import NumpyOps
from rtx.lib import load
import oracle_lib as O

HEADER_DIR = os.path.join(O.ROOT, "include")
W, H, G = 70, 33, 4  # the random frame: 70 x 33 pixels, 4 strata in the guides
OFF = dict(sigma_normal=-1, sigma_depth=-1, sigma_hit=-1, sigma_color=-1)


def frame_of(w, h):
    f = abi.Frame()
    f.image_width, f.image_height, f.sqrt_spp, f.max_depth = w, h, 2, 8
    f.pixel_samples_scale = 0.25
    return f


def random_case(seed=11, w=W, h=H, g=G):
    """(frame, rgb sums, scale, guide sums, g): smooth regions with two edges,
    noisy colour, a few missed and half-hit pixels, a few tiny albedos."""
    rng = np.random.default_rng(seed)
    f = frame_of(w, h)
    rgb = rng.uniform(0.0, 2.0, (h, w, 3)) * g
    n = rng.normal(size=(h, w, 3)) * 0.05 + np.array([0.0, 0.0, 1.0])
    n[:, w // 2:] = rng.normal(size=(h, w - w // 2, 3)) * 0.05 + np.array([1.0, 0.0, 0.0])
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    hits = np.full((h, w), float(g))
    hits[: h // 4, : w // 5] = 0.0          # sky
    hits[h // 4, : w // 5] = g / 2.0        # a silhouette row: half the strata hit
    depth = (5.0 + 0.02 * np.arange(w)[None, :] + 0.3 * (np.arange(h)[:, None] > h // 2)) * hits
    depth *= 1.0 + 0.001 * rng.normal(size=(h, w))
    alb = rng.uniform(0.2, 0.9, (h, w, 3))
    alb[3:6, 40:44] = 0.001                 # below the 0.01 floor
    guides = np.zeros((h, w, 8))
    guides[..., 0:3] = np.where(hits[..., None] > 0, alb, 1.0) * g
    guides[..., 3:6] = n * hits[..., None]
    guides[..., 6] = depth
    guides[..., 7] = hits
    return f, rgb, 1.0 / g, guides, g


def test_a_constant_image_stays_constant():
    f, rgb, scale, guides, g = random_case()
    guides[..., 0:3] = g  # albedo 1 everywhere: e = c
    rgb[...] = 0.37 * g
    for passes in (-1, 1, 2, 5, 8):
        out = NumpyOps().denoise(f, rgb, scale, None, guides, g, dict(passes=passes))
        np.testing.assert_allclose(out, 0.37, rtol=1e-12, atol=0)


def test_no_pass_returns_the_input():
    f, rgb, scale, guides, g = random_case()
    assert (guides[..., 0:3] / g < 0.01).any()  # a_d both demodulates and remodulates
    out = NumpyOps().denoise(f, rgb, scale, None, guides, g, dict(passes=-1))
    np.testing.assert_allclose(out, rgb * scale, rtol=1e-12, atol=0)
    # ... and with the per-tile scale of an adaptive frame (strata 0 shows as 1)
    tx, ty = (W + 7) // 8, (H + 7) // 8
    strata = (np.arange(tx * ty, dtype=np.int32) % 5) * 2
    s = np.repeat(np.repeat((1.0 / np.maximum(1, strata)).reshape(ty, tx), 8, 0), 8, 1)[:H, :W]
    out = NumpyOps().denoise(f, rgb, 123.0, strata, guides, g, dict(passes=-1))
    np.testing.assert_allclose(out, rgb * s[..., None], rtol=1e-12, atol=0)


def test_a_normal_edge_is_preserved():
    f = frame_of(W, H)
    g = 2
    rgb = np.zeros((H, W, 3))
    rgb[:, : W // 2] = 1.0 * g
    guides = np.zeros((H, W, 8))
    guides[..., 0:3] = g
    guides[:, : W // 2, 5] = g  # left: normal (0, 0, 1)
    guides[:, W // 2:, 3] = g   # right: (1, 0, 0); |dn|^2 = 2, exponent 200 -> clamped to 80
    guides[..., 6], guides[..., 7] = 3.0 * g, g
    p = dict(OFF, sigma_normal=0.1)
    out = NumpyOps().denoise(f, rgb, 1.0 / g, None, guides, g, p)
    np.testing.assert_allclose(out, rgb / g, rtol=0, atol=1e-6)
    assert np.abs(out - rgb / g).max() > 0  # exp(-80), not a hard cut


def plain_atrous(e, passes):
    """B3 a-trous blur with border renormalisation, by clipped gathers."""
    h, w = e.shape[:2]
    for k in range(passes):
        num, den = np.zeros_like(e), np.zeros((h, w, 1))
        for dj, bj in zip(range(-2, 3), denoise.B3):
            for di, bi in zip(range(-2, 3), denoise.B3):
                ys, xs = np.arange(h) + dj * 2 ** k, np.arange(w) + di * 2 ** k
                m = (((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :])[..., None]
                num += bi * bj * m * e[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)]
                den += bi * bj * m
        e = num / den
    return e


def test_every_term_off_is_the_plain_b3_blur():
    f, rgb, scale, guides, g = random_case()
    a_d = np.maximum(guides[..., 0:3] / g, 0.01)
    out = NumpyOps().denoise(f, rgb, scale, None, guides, g, dict(OFF))  # passes 0: the default 5
    np.testing.assert_allclose(out, plain_atrous(rgb * scale / a_d, 5) * a_d, rtol=1e-12, atol=0)
    out = NumpyOps().denoise(f, rgb, scale, None, guides, g, dict(OFF, passes=8))  # step 128 > the frame
    np.testing.assert_allclose(out, plain_atrous(rgb * scale / a_d, 8) * a_d, rtol=1e-12, atol=0)


def test_a_nan_sample_does_not_spread():
    f, rgb, scale, guides, g = random_case()
    rgb[20, 30, 1] = np.nan        # one NaN in a finite neighbourhood
    rgb[2:11, 50:59] = np.nan      # a 9 x 9 block: its centre's 25 taps (step 1) are all NaN
    rgb[28, 5, 0] = np.inf
    for params in (dict(OFF, passes=1), dict(passes=1)):
        out = NumpyOps().denoise(f, rgb, scale, None, guides, g, params)
        bad_in, bad_out = ~np.isfinite(rgb).all(-1), ~np.isfinite(out).all(-1)
        assert not (bad_out & ~bad_in).any()                   # nothing finite went bad
        assert np.isfinite(out[20, 30]).all() and np.isfinite(out[28, 5]).all()
        assert bad_out[4:9, 52:57].all() and bad_out.sum() == 25  # all taps NaN: the pixel keeps its NaN
    # every term off: the single NaN is replaced by its neighbourhood's weighted mean
    out = NumpyOps().denoise(f, rgb, scale, None, guides, g, dict(OFF, passes=1))
    a_d = np.maximum(guides[..., 0:3] / g, 0.01)
    e = rgb * scale / a_d
    num, den = np.zeros(3), 0.0
    for dj in range(-2, 3):
        for di in range(-2, 3):
            if di or dj:
                w = denoise.B3[di + 2] * denoise.B3[dj + 2]
                num, den = num + w * e[20 + dj, 30 + di], den + w
    np.testing.assert_allclose(out[20, 30], num / den * a_d[20, 30], rtol=1e-12)
    # five passes: the block shrinks or stays, and never grows
    out5 = NumpyOps().denoise(f, rgb, scale, None, guides, g, None)
    assert not (~np.isfinite(out5).all(-1) & np.isfinite(rgb).all(-1)).any()


def test_output_is_non_negative_for_non_negative_input():
    f, rgb, scale, guides, g = random_case(seed=12)
    for params in (None, dict(passes=3, sigma_color=0.5), dict(OFF, sigma_depth=0.02)):
        out = NumpyOps().denoise(f, rgb, scale, None, guides, g, params)
        assert np.isfinite(out).all() and (out.sum(-1) >= 0).all() and (out >= 0).all()


def test_params_resolution_and_refusals():
    assert denoise.resolve(None) == (5, abi.RT_DENOISE_SIGMA_NORMAL, abi.RT_DENOISE_SIGMA_DEPTH, 0.1,
                                     abi.RT_DENOISE_SIGMA_COLOR)
    assert denoise.resolve(dict(passes=-3, sigma_hit=-1, sigma_color=2.5))[0::3] == (0, None)
    assert denoise.resolve(dict(sigma_color=2.5))[4] == 2.5
    with pytest.raises(ValueError):
        denoise.resolve(dict(passes=9))
    with pytest.raises(KeyError):
        abi.denoise_params(dict(sigma_colour=1.0))
    f, rgb, scale, guides, g = random_case()
    with pytest.raises(ValueError):
        NumpyOps().denoise(f, rgb, scale, None, guides, 0)


# ---- ABI (no device call is reached) ----------------------------------------
def test_workspace_bytes():
    L = load()
    f = frame_of(36, 36)
    n = C.c_int64(-1)
    assert L.rt_denoise_workspace_bytes(C.byref(f), C.byref(n)) == abi.RT_OK
    assert n.value > 0 and n.value % 256 == 0
    assert n.value >= 64 * 36 * 36 and n.value == NumpyOps().workspace_bytes(f)
    assert L.rt_denoise_workspace_bytes(C.byref(f), None) == abi.RT_ERR_INVALID
    assert L.rt_denoise_workspace_bytes(C.byref(frame_of(0, 36)), C.byref(n)) == abi.RT_ERR_INVALID


def test_denoise_refusals_before_any_device_call():
    L = load()
    f = frame_of(36, 36)
    # addresses that are never dereferenced: every call below is refused on its arguments
    rgb, guides, ws, out = 0x10000000, 0x20000000, 0x30000000, 0x40000000

    def call(rgb=rgb, guides=guides, ws=ws, out=out, g=4, params=None, frame=f):
        p = abi.denoise_params(params)
        return L.rt_denoise_device(C.byref(frame), C.c_void_p(rgb), 1.0, None, C.c_void_p(guides), g,
                                   C.byref(p) if p is not None else None, C.c_void_p(ws), C.c_void_p(out), None)

    cases = {
        "passes 9": dict(params=dict(passes=9)),
        "guide_strata 0": dict(g=0),
        "null rgb": dict(rgb=0),
        "null guides": dict(guides=0),
        "null workspace": dict(ws=0),
        "null out": dict(out=0),
        "unaligned workspace": dict(ws=ws + 8),
        "out inside the workspace": dict(out=ws + 256),
        "empty frame": dict(frame=frame_of(36, 0)),
    }
    for what, kw in cases.items():
        assert call(**kw) == abi.RT_ERR_INVALID, what
        assert L.rt_last_error(), what


def test_guide_refusals_need_no_scene():
    L = load()
    f = frame_of(36, 36)
    p = abi.RenderParams()
    assert L.rt_render_guides_device(None, C.byref(f), C.byref(p), C.c_void_p(0x1000), None) == abi.RT_ERR_INVALID
    assert b"null" in L.rt_last_error()


def test_denoise_params_mirror_and_defaults_match_the_header(tmp_path):
    """rt_denoise_params as gcc lays it out, and the RT_DENOISE_* defaults the
    Python side restates (rtx/abi.py)."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_api.h"', "int main(void) {",
             'printf("%zu\\n", sizeof(rt_denoise_params));']
    want = [C.sizeof(abi.DenoiseParams)]
    for name, _ in abi.DenoiseParams._fields_:
        lines.append('printf("%%zu\\n", offsetof(rt_denoise_params, %s));' % name)
        want.append(getattr(abi.DenoiseParams, name).offset)
    consts = ["RT_GUIDE_CHANNELS", "RT_DENOISE_PASSES", "RT_DENOISE_MAX_PASSES", "RT_DENOISE_SIGMA_NORMAL",
              "RT_DENOISE_SIGMA_DEPTH", "RT_DENOISE_SIGMA_HIT", "RT_DENOISE_SIGMA_COLOR", "RT_ABI_VERSION"]
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
    for name in ("rt_render_guides_device", "rt_denoise_workspace_bytes", "rt_denoise_device"):
        assert name in abi.EXPORTS and hasattr(load(), name)
