"""Denoised display: first-hit guide buffers and an edge-avoiding a-trous filter.

rtx.progressive shows one more stratum of every pixel per frame; what the
viewer sees in the first frames after a camera move is 1-16 spp Monte-Carlo
noise.  Here the displayed frame is filtered, steered by per-pixel first-hit
features (rt_render_guides_device: albedo, normal, depth, hit fraction) so
that it blurs noise and not edges.  The fp64 accumulator stays the source of
truth: the filter reads it and writes a separate image.

The filter (rt_denoise_device).  With g strata summed into the guides, per
pixel p: c = rgb * scale; a = albedo / g, a_d = max(a, 0.01) per channel,
e = c / a_d (the filter runs on this demodulated signal, so texture detail
carried by the albedo is not blurred); n = normal / g (not renormalised: a
pixel straddling an edge has a short normal on purpose); h = hits / g;
z = depth / max(hits, 1); y = the Rec. 709 luminance of e.  Pass k of
`passes`, step s = 2^k: taps q = p + s (di, dj), di, dj in -2..2, B3-spline
weights b = (1/16, 1/4, 3/8, 1/4, 1/16), taps outside the image skipped.  The
centre tap weighs b2 b2; every other tap b_di b_dj exp(-min(x, 80)), x the
sum of the enabled terms

    |n_p - n_q|^2 / sigma_n^2
    |z_p - z_q| / (sigma_z max(z_p, z_q, 1e-30) s max(|di|, |dj|))
    (h_p - h_q)^2 / sigma_h^2
    |e_p - e_q|^2 / ((sigma_c 2^-k)^2 (y_p^2 + 1e-4))

with e, y the pass's input.  A tap whose e is not finite weighs 0 (and a
non-finite e_p has no colour term); e'_p = sum w e_q / sum w, or e_p itself
when sum w = 0.  out = e a_d.

NumpyOps states this in fp64 NumPy -- the specification.  The HIP kernels
round e, n, z, h, a_d to fp32 once and run the passes in fp32 with the native
exponential (tests/test_denoise_gpu.py holds them to 1e-4 of NumpyOps).

The variance-guided filter (rt_denoise_variance_device).  The colour term
above is normalised by the pixel's own luminance, so it blurs a converged
frame as much as a noisy one.  This filter normalises by the standard
deviation of the pixel's estimate instead, and narrows as that falls.  Per
pixel a luminance variance v of e:

    from moments   where the caller passes an AdaptiveRenderer's s1, s2,
                   tile_strata and batch_strata and the pixel's tile has
                   b = tile_strata // batch_strata >= min_batches batches:
                   v_c = max(0, (s2 - s1^2 / b) / (b - 1)) / b, the variance of
                   the mean of c's luminance, and v = v_c / lum(a_d)^2 (exact
                   for a grey albedo, an approximation for a coloured one);
    spatial        everywhere else: over the 7x7 window at step 1, weights
                   exp(-min(x, 80)) with x the normal, depth and hit terms
                   above (s = 1), the centre 1, taps outside the image or with
                   a non-finite e skipped: m1 = sum w d / sum w,
                   m2 = sum w d^2 / sum w, d = y_q - y_p, v = max(0, m2 - m1^2)
                   (the variance of y over the window: the shift by y_p drops
                   out, and keeps the fp32 kernel exact on a flat window);

and v = 0 where e is not finite.  The passes are the ones above with the
colour term replaced by

    |y_p - y_q| / (sigma_l sqrt(v~_p) + 1e-6)

v~_p the 3x3 Gaussian (1/4, 1/2, 1/4 per axis, step 1) of the pass's input v
over the in-image pixels with a finite e, renormalised (not halved per pass:
v itself shrinks).  The variance is filtered with the colour:
v'_p = sum w^2 v_q / (sum w)^2, or v_p when sum w = 0.  out = e a_d, and
optionally the final v.

The same filter on a variance the caller gives (rt_denoise_given_variance_device,
NumpyOps.denoise_given_variance): no estimation stage -- v is the given plane
(a NaN or negative entry: 0), 0 where e is not finite -- and the same passes.
rtx.temporal.TemporalVarianceDisplay feeds it the variance its blend carries
across camera moves.
"""
import ctypes as C

import numpy as np

from . import abi
from .lib import check, load
from .ppm import to_bytes

LUMA = (0.2126, 0.7152, 0.0722)
B3 = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)
G3 = (1.0 / 4, 1.0 / 2, 1.0 / 4)  # the variance's 3x3 blur
SPATIAL_RADIUS = 3                # the spatial variance estimate's 7x7 window


def resolve(params=None):
    """(passes, sigma_n, sigma_z, sigma_h, sigma_c) of None / a dict / an
    abi.DenoiseParams: 0 = the default, a sigma < 0 = its term off (returned
    as None), passes < 0 = no pass (returned as 0)."""
    p = abi.denoise_params(params) or abi.DenoiseParams()
    if p.passes > abi.RT_DENOISE_MAX_PASSES:
        raise ValueError("passes must be at most %d" % abi.RT_DENOISE_MAX_PASSES)
    passes = abi.RT_DENOISE_PASSES if p.passes == 0 else max(0, p.passes)

    def pick(v, d):
        v = d if v == 0 else v
        return None if v < 0 else float(v)

    return (passes, pick(p.sigma_normal, abi.RT_DENOISE_SIGMA_NORMAL),
            pick(p.sigma_depth, abi.RT_DENOISE_SIGMA_DEPTH), pick(p.sigma_hit, abi.RT_DENOISE_SIGMA_HIT),
            pick(p.sigma_color, abi.RT_DENOISE_SIGMA_COLOR))


def resolve_variance(params=None):
    """(passes, min_batches, sigma_n, sigma_z, sigma_h, sigma_l) of None / a
    dict / an abi.DenoiseVarianceParams, by resolve's conventions; min_batches
    0 = the default, below 2 = 2."""
    p = abi.denoise_variance_params(params) or abi.DenoiseVarianceParams()
    passes, sn, sz, sh, _ = resolve(dict(passes=p.passes, sigma_normal=p.sigma_normal, sigma_depth=p.sigma_depth,
                                         sigma_hit=p.sigma_hit))
    mb = abi.RT_DENOISE_MIN_BATCHES if p.min_batches == 0 else p.min_batches
    sl = abi.RT_DENOISE_SIGMA_LUM if p.sigma_lum == 0 else p.sigma_lum
    return passes, max(2, mb), sn, sz, sh, None if sl < 0 else float(sl)


def _workspace_bytes(frame, variance):
    """Four float4 planes, each padded to 256 B; the variance layout: and one float plane."""
    n = frame.image_width * frame.image_height
    return 4 * ((n * 16 + 255) & ~255) + (((n * 4 + 255) & ~255) if variance else 0)


def workspace_bytes(frame):
    """rt_denoise_workspace_bytes: 64 B per pixel."""
    return _workspace_bytes(frame, False)


def variance_workspace_bytes(frame):
    """rt_denoise_variance_workspace_bytes: 68 B per pixel."""
    return _workspace_bytes(frame, True)


def _pixel_scale(tile_strata, frame):
    tx, ty = (frame.image_width + 7) // 8, (frame.image_height + 7) // 8
    s = 1.0 / np.maximum(1, np.asarray(tile_strata)).astype(np.float64)
    s = np.repeat(np.repeat(s.reshape(ty, tx), 8, axis=0), 8, axis=1)
    return s[:frame.image_height, :frame.image_width]


def luminance(e):
    """Rec. 709 luminance of [..., 3]."""
    with np.errstate(invalid="ignore", over="ignore"):
        return LUMA[0] * e[..., 0] + LUMA[1] * e[..., 1] + LUMA[2] * e[..., 2]


def _shifted(H, W, oy, ox):
    """(P, Q): the pixels whose tap at offset (oy, ox) lies inside the image, and those taps."""
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y0 >= y1 or x0 >= x1:
        return None, None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


class NumpyOps:
    """rt_denoise_device and rt_denoise_variance_device on host arrays, in
    fp64: the statements of record."""

    workspace_bytes = staticmethod(workspace_bytes)
    variance_workspace_bytes = staticmethod(variance_workspace_bytes)

    def prepare(self, frame, rgb, scale, tile_strata, guides, guide_strata):
        """(e, a_d, n, z, h) of the definition above."""
        g = float(guide_strata)
        rgb = np.asarray(rgb, dtype=np.float64)
        G = np.asarray(guides, dtype=np.float64)
        s = _pixel_scale(tile_strata, frame)[..., None] if tile_strata is not None else float(scale)
        c = rgb * s
        a_d = np.maximum(G[..., 0:3] / g, 0.01)
        e = c / a_d
        n = G[..., 3:6] / g
        h = G[..., 7] / g
        z = G[..., 6] / np.maximum(G[..., 7], 1.0)
        return e, a_d, n, z, h

    def geo_terms(self, n, z, h, P, Q, d, sn, sz, sh):
        """The normal, depth and hit terms of the taps Q of the pixels P, d = s max(|di|, |dj|)."""
        x = np.zeros(z[P].shape)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if sn is not None:
                x = x + ((n[P] - n[Q]) ** 2).sum(-1) / sn ** 2
            if sz is not None:
                x = x + np.abs(z[P] - z[Q]) / (sz * np.maximum(np.maximum(z[P], z[Q]), 1e-30) * d)
            if sh is not None:
                x = x + (h[P] - h[Q]) ** 2 / sh ** 2
        return x

    def one_pass(self, e, n, z, h, k, sn, sz, sh, sc, v=None, sl=None):
        """Pass k.  With v (the variance-guided filter: sc is None) the colour
        term is |y_p - y_q| / (sl sqrt(v~_p) + 1e-6) unless sl is None, and
        (e', v') is returned, v' = sum w^2 v_q / (sum w)^2."""
        H, W = e.shape[:2]
        s = 1 << k
        y = luminance(e)
        ok = np.isfinite(e).all(-1)
        sw = np.zeros((H, W))
        se = np.zeros((H, W, 3))
        sv = np.zeros((H, W))
        sd = sl * np.sqrt(self.blur3(v, ok)) + 1e-6 if v is not None and sl is not None else None
        for dj in range(-2, 3):
            for di in range(-2, 3):
                oy, ox = dj * s, di * s
                y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
                if y0 >= y1 or x0 >= x1:
                    continue  # the whole tap plane lies outside the image
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                w = np.full((y1 - y0, x1 - x0), B3[di + 2] * B3[dj + 2])
                if di or dj:
                    x = self.geo_terms(n, z, h, P, Q, float(s * max(abs(di), abs(dj))), sn, sz, sh)
                    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                        if sc is not None:
                            ck = sc * 2.0 ** -k
                            t = ((e[P] - e[Q]) ** 2).sum(-1) / (ck ** 2 * (y[P] ** 2 + 1e-4))
                            x = x + np.where(ok[P], t, 0.0)
                        if sd is not None:
                            x = x + np.where(ok[P], np.abs(y[P] - y[Q]) / sd[P], 0.0)
                        w = w * np.exp(-np.minimum(x, 80.0))
                    w = np.where(np.isnan(x), 0.0, w)
                w = np.where(ok[Q], w, 0.0)
                sw[P] += w
                se[P] += w[..., None] * np.where(ok[Q][..., None], e[Q], 0.0)
                if v is not None:
                    sv[P] += w * w * np.where(ok[Q], v[Q], 0.0)
        some = sw > 0
        div = np.where(some, sw, 1.0)
        e1 = np.where(some[..., None], se / div[..., None], e)
        return e1 if v is None else (e1, np.where(some, sv / (div * div), v))

    def denoise(self, frame, rgb, scale, tile_strata, guides, guide_strata, params=None):
        """-> [H, W, 3] float64: the filtered, scaled radiance."""
        if guide_strata < 1:
            raise ValueError("guide_strata must be >= 1")
        passes, sn, sz, sh, sc = resolve(params)
        e, a_d, n, z, h = self.prepare(frame, rgb, scale, tile_strata, guides, guide_strata)
        for k in range(passes):
            e = self.one_pass(e, n, z, h, k, sn, sz, sh, sc)
        return e * a_d

    # ---- the variance-guided filter (rt_denoise_variance_device) ----
    def blur3(self, v, ok):
        """v~: the 3x3 Gaussian (1/4, 1/2, 1/4 per axis) of v over the in-image
        pixels whose e is finite, renormalised; 0 where there is none."""
        H, W = v.shape
        num, den = np.zeros((H, W)), np.zeros((H, W))
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                P, Q = _shifted(H, W, dj, di)
                if P is None:
                    continue
                g = G3[di + 1] * G3[dj + 1] * ok[Q]
                num[P] += g * np.where(ok[Q], v[Q], 0.0)
                den[P] += g
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)

    def moments_variance(self, frame, a_d, tile_strata, s1, s2, batch_strata, min_batches):
        """(v, use): the variance of e's luminance from the batch moments, and
        the pixels whose tile has b = strata / batch_strata >= min_batches."""
        tx, ty = (frame.image_width + 7) // 8, (frame.image_height + 7) // 8
        b = (np.asarray(tile_strata).astype(np.int64) // int(batch_strata)).reshape(ty, tx)
        b = np.repeat(np.repeat(b, 8, axis=0), 8, axis=1)[:frame.image_height, :frame.image_width]
        use = b >= min_batches
        fb = np.where(use, b, 2).astype(np.float64)
        s1, s2 = np.asarray(s1, dtype=np.float64), np.asarray(s2, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            var = (s2 - s1 * s1 / fb) / (fb - 1.0)
            var = np.where(var > 0.0, var, 0.0)  # a NaN moment: 0
            la = luminance(a_d)
            return var / fb / (la * la), use

    def spatial_variance(self, e, n, z, h, sn, sz, sh):
        """The weighted variance of y over the 7x7 window at step 1: weights
        exp(-min(x, 80)) with x the pass's normal, depth and hit terms, the
        centre 1, taps outside the image or with a non-finite e skipped.  The
        moments are taken of y_q - y_p: the variance does not see the shift,
        and the fp32 kernel is exact on a flat window."""
        H, W = e.shape[:2]
        y = luminance(e)
        ok = np.isfinite(e).all(-1)
        sw, m1, m2 = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
        for dj in range(-SPATIAL_RADIUS, SPATIAL_RADIUS + 1):
            for di in range(-SPATIAL_RADIUS, SPATIAL_RADIUS + 1):
                P, Q = _shifted(H, W, dj, di)
                if P is None:
                    continue
                w = np.ones(y[P].shape)
                if di or dj:
                    x = self.geo_terms(n, z, h, P, Q, float(max(abs(di), abs(dj))), sn, sz, sh)
                    w = np.where(np.isnan(x), 0.0, np.exp(-np.minimum(x, 80.0)))
                w = np.where(ok[Q] & ok[P], w, 0.0)
                with np.errstate(invalid="ignore", over="ignore"):
                    d = np.where(w > 0, y[Q] - y[P], 0.0)
                sw[P] += w
                m1[P] += w * d
                m2[P] += w * d * d
        some = sw > 0
        div = np.where(some, sw, 1.0)
        v = m2 / div - (m1 / div) ** 2
        return np.where(some & (v > 0.0), v, 0.0)

    def denoise_variance(self, frame, rgb, scale, tile_strata, guides, guide_strata, s1=None, s2=None,
                         batch_strata=0, params=None, with_variance=False):
        """-> [H, W, 3] float64 (with_variance: and the final variance plane [H, W])."""
        if guide_strata < 1:
            raise ValueError("guide_strata must be >= 1")
        if (s1 is None) != (s2 is None):
            raise ValueError("s1 and s2 go together")
        if s1 is not None and (tile_strata is None or batch_strata < 1):
            raise ValueError("moments need tile strata and batch_strata >= 1")
        passes, min_batches, sn, sz, sh, sl = resolve_variance(params)
        e, a_d, n, z, h = self.prepare(frame, rgb, scale, tile_strata, guides, guide_strata)
        v = self.spatial_variance(e, n, z, h, sn, sz, sh)
        if s1 is not None:
            vm, use = self.moments_variance(frame, a_d, tile_strata, s1, s2, batch_strata, min_batches)
            v = np.where(use, vm, v)
        return self._variance_passes(e, a_d, n, z, h, v, passes, sn, sz, sh, sl, with_variance)

    def _variance_passes(self, e, a_d, n, z, h, v, passes, sn, sz, sh, sl, with_variance):
        """The shared tail: v = 0 where e is not finite, the passes, out = e a_d."""
        v = np.where(np.isfinite(e).all(-1), v, 0.0)
        for k in range(passes):
            e, v = self.one_pass(e, n, z, h, k, sn, sz, sh, None, v, sl)
        return (e * a_d, v) if with_variance else e * a_d

    def denoise_given_variance(self, frame, rgb, scale, tile_strata, guides, guide_strata, variance, params=None,
                               with_variance=False):
        """rt_denoise_given_variance_device: denoise_variance without its
        estimation stage.  v is `variance` ([H, W]; a NaN or negative entry is
        0), and 0 where e is not finite; min_batches is ignored."""
        if guide_strata < 1:
            raise ValueError("guide_strata must be >= 1")
        passes, _, sn, sz, sh, sl = resolve_variance(params)
        e, a_d, n, z, h = self.prepare(frame, rgb, scale, tile_strata, guides, guide_strata)
        v = np.asarray(variance, dtype=np.float64)
        if v.shape != e.shape[:2]:
            raise ValueError("variance must be [H, W]")
        with np.errstate(invalid="ignore"):
            v = np.where(v > 0.0, v, 0.0)
        return self._variance_passes(e, a_d, n, z, h, v, passes, sn, sz, sh, sl, with_variance)

    def bytes(self, image):
        return to_bytes(image)


class HipOps:
    """rt_denoise_device / rt_to_bytes_device on torch CUDA tensors, on one stream."""

    def __init__(self, device, stream):
        import torch
        self.torch = torch
        self.device = device
        self.stream = stream
        self.lib = load()

    def _sp(self):
        return C.c_void_p(self.stream.cuda_stream)

    @staticmethod
    def _ptr(a):
        """The device pointer of a tensor, null for None."""
        return C.c_void_p(a.data_ptr() if a is not None else 0)

    def _image(self, frame, out=None):
        """`out`, or a new [H, W, 3] float64 image on the stream."""
        if out is not None:
            return out
        t = self.torch
        with t.cuda.stream(self.stream):
            return t.empty((frame.image_height, frame.image_width, 3), dtype=t.float64, device=self.device)

    def _bytes(self, fn, frame):
        n = C.c_int64(0)
        check(fn(C.byref(frame), C.byref(n)))
        return n.value

    def _workspace(self, nbytes):
        """A workspace tensor of `nbytes` (torch allocations are 512-B aligned)."""
        t = self.torch
        with t.cuda.stream(self.stream):
            return t.empty((nbytes,), dtype=t.uint8, device=self.device)

    def workspace_bytes(self, frame):
        return self._bytes(self.lib.rt_denoise_workspace_bytes, frame)

    def workspace(self, frame):
        return self._workspace(self.workspace_bytes(frame))

    def variance_workspace_bytes(self, frame):
        return self._bytes(self.lib.rt_denoise_variance_workspace_bytes, frame)

    def variance_workspace(self, frame):
        return self._workspace(self.variance_workspace_bytes(frame))

    def denoise(self, frame, rgb, scale, tile_strata, guides, guide_strata, params=None, workspace=None,
                out=None):
        ptr = self._ptr
        workspace = self.workspace(frame) if workspace is None else workspace
        out = self._image(frame, out)
        p = abi.denoise_params(params)
        check(self.lib.rt_denoise_device(
            C.byref(frame), ptr(rgb), C.c_double(scale), ptr(tile_strata), ptr(guides), int(guide_strata),
            C.byref(p) if p is not None else None, ptr(workspace), ptr(out), self._sp()))
        return out

    def denoise_variance(self, frame, rgb, scale, tile_strata, guides, guide_strata, s1=None, s2=None,
                         batch_strata=0, params=None, workspace=None, out=None, variance_out=None):
        """rt_denoise_variance_device; `variance_out` ([H, W] float64) takes the final variance plane."""
        ptr = self._ptr
        workspace = self.variance_workspace(frame) if workspace is None else workspace
        out = self._image(frame, out)
        p = abi.denoise_variance_params(params)
        check(self.lib.rt_denoise_variance_device(
            C.byref(frame), ptr(rgb), C.c_double(scale), ptr(tile_strata), ptr(guides), int(guide_strata),
            ptr(s1), ptr(s2), int(batch_strata), C.byref(p) if p is not None else None, ptr(workspace), ptr(out),
            ptr(variance_out), self._sp()))
        return out

    def denoise_given_variance(self, frame, rgb, scale, tile_strata, guides, guide_strata, variance, params=None,
                               workspace=None, out=None, variance_out=None):
        """rt_denoise_given_variance_device: the passes on the caller's `variance` plane ([H, W] float64)."""
        ptr = self._ptr
        workspace = self.variance_workspace(frame) if workspace is None else workspace
        out = self._image(frame, out)
        p = abi.denoise_variance_params(params)
        check(self.lib.rt_denoise_given_variance_device(
            C.byref(frame), ptr(rgb), C.c_double(scale), ptr(tile_strata), ptr(guides), int(guide_strata),
            ptr(variance), C.byref(p) if p is not None else None, ptr(workspace), ptr(out), ptr(variance_out),
            self._sp()))
        return out

    def bytes(self, image, out=None):
        """rt_to_bytes_device (scale 1) of a filtered image."""
        t = self.torch
        if out is None:
            with t.cuda.stream(self.stream):
                out = t.empty(image.shape, dtype=t.uint8, device=self.device)
        check(self.lib.rt_to_bytes_device(C.c_void_p(image.data_ptr()), image.numel() // 3, C.c_double(1.0),
                                          C.c_void_p(out.data_ptr()), self._sp()))
        return out


class DenoisedDisplay:
    """The filtered display of a progressive.for_renderer ProgressiveRenderer
    or an adaptive.for_renderer AdaptiveRenderer `pr` (both carry the Renderer
    and the stream they launch on).

    step(n) steps the wrapped renderer; while fewer than `guide_strata` strata
    have guides, the same strata's guides are added on the same stream.
    image() is the filtered frame ([H, W, 3] float64 CUDA tensor), bytes() its
    write_color bytes.  The wrapped accumulator is only read.  The guides, the
    workspace and the output are allocated once per frame size.

        dd = DenoisedDisplay(progressive.for_renderer(R, frame, seed=5))
        pipe = progressive.DisplayPipeline(dd, bytes_fn=dd.bytes_into)
    """

    def __init__(self, pr, guide_strata=16, params=None):
        import torch
        self.torch = torch
        self.pr = pr
        self.renderer = pr.renderer
        self.stream = pr.stream
        self.guide_strata = max(1, int(guide_strata))
        self.params = abi.denoise_params(params)
        self.ops = HipOps(pr.acc.device, self.stream)
        self._adaptive = hasattr(pr, "tile_strata")
        self._allocate()

    def _allocate(self):
        t, f = self.torch, self.pr.frame
        with t.cuda.stream(self.stream):
            self.guides = t.zeros((f.image_height, f.image_width, abi.RT_GUIDE_CHANNELS), dtype=t.float64,
                                  device=self.pr.acc.device)
            self.out = t.empty((f.image_height, f.image_width, 3), dtype=t.float64, device=self.pr.acc.device)
        self.workspace = self._new_workspace(f)
        self._shape = (f.image_width, f.image_height)
        self.guides_done = 0

    def _new_workspace(self, f):
        return self.ops.workspace(f)

    # what DisplayPipeline reads of a renderer
    @property
    def acc(self):
        return self.pr.acc

    @property
    def frame(self):
        return self.pr.frame

    @property
    def samples_taken(self):
        return self.pr.strata_done if self._adaptive else self.pr.samples_taken

    @property
    def converged(self):
        return self.pr.done if self._adaptive else self.pr.converged

    def _catch_up(self):
        """Guides for the strata the wrapped renderer has traced and the guides lack."""
        hi = min(self.samples_taken, self.guide_strata)
        if hi > self.guides_done:
            self.renderer.render_guides_device(self.pr.frame, self.guides.data_ptr(), self.stream.cuda_stream,
                                               seed=self.pr.seed, samples=(self.guides_done, hi - self.guides_done),
                                               accumulate=1)
            self.guides_done = hi

    def step(self, n=1):
        """Steps the wrapped renderer (an AdaptiveRenderer: n batches); returns the strata traced."""
        traced = sum(self.pr.step() for _ in range(n)) if self._adaptive else self.pr.step(n)
        self._catch_up()
        return traced

    def image(self):
        self._catch_up()
        pr = self.pr
        return self.ops.denoise(pr.frame, pr.acc, 1.0 if self._adaptive else pr.scale,
                                pr.tile_strata if self._adaptive else None, self.guides,
                                max(1, self.guides_done), self.params, self.workspace, self.out)

    def bytes(self, out=None):
        return self.ops.bytes(self.image(), out)

    def bytes_into(self, pr, out):
        """DisplayPipeline's bytes_fn: the filtered frame's bytes into `out`."""
        return self.bytes(out)

    def reset(self, frame=None):
        """Camera moved: the wrapped renderer restarts, the guides are cleared.
        Also after Renderer.move_spheres: the accumulator and the guide sums
        describe the old scene, and nothing here notices the move -- the caller
        calls reset()."""
        self.pr.reset(frame)
        if (self.pr.frame.image_width, self.pr.frame.image_height) != self._shape:
            self._allocate()
            return
        with self.torch.cuda.stream(self.stream):
            self.guides.zero_()
        self.guides_done = 0


class VarianceGuidedDisplay(DenoisedDisplay):
    """DenoisedDisplay with the variance-guided filter (rt_denoise_variance_device):
    the display narrows as the estimate converges instead of blurring a
    1,024-strata frame like a 4-strata one.

    Over an AdaptiveRenderer the filter takes the renderer's own batch moments
    (s1, s2, tile_strata, batch_strata): the variance of each pixel's mean, as
    soon as its tile has `min_batches` batches; before that, and in a tile whose
    last batch was a short one, the spatial estimate stands in.  Over a
    ProgressiveRenderer there are no moments and every pixel runs on the spatial
    estimate, the luminance variance of its 7x7 neighbourhood.  That estimate
    holds the signal's own variation over the window as well as the noise, so
    it stops falling once the noise is below it: the filter then keeps blurring
    gradients and soft shadows however many strata arrive.  At the default
    sigma_lum (chosen from moments) the Cornell scenes at 1080 pixels come out
    0.23-0.47 of the raw frame's error up to 16 strata, 1.0-1.5 times it at 256
    and 1.8-2.7 times at 1,024 -- still better than DenoisedDisplay there;
    sigma_lum 1.5 is the best single value without moments (worse than raw only
    at 1,024).  adaptive.for_renderer(..., threshold=0) samples
    what a progressive renderer samples -- only a tile without any variance
    retires -- and is the way to get moments.

    variance() is the final variance plane of the last image() ([H, W] float64).

        ar = adaptive.for_renderer(R, frame, seed=5, threshold=0, batch_strata=4)
        vd = VarianceGuidedDisplay(ar)
        pipe = progressive.DisplayPipeline(vd, bytes_fn=vd.bytes_into)
    """

    def __init__(self, pr, guide_strata=16, params=None):
        super().__init__(pr, guide_strata=guide_strata, params=None)
        self.params = abi.denoise_variance_params(params)

    def _allocate(self):
        super()._allocate()
        t, f = self.torch, self.pr.frame
        with t.cuda.stream(self.stream):
            self.var = t.zeros((f.image_height, f.image_width), dtype=t.float64, device=self.pr.acc.device)

    def _new_workspace(self, f):
        return self.ops.variance_workspace(f)

    def image(self):
        self._catch_up()
        pr, ad = self.pr, self._adaptive
        return self.ops.denoise_variance(pr.frame, pr.acc, 1.0 if ad else pr.scale, pr.tile_strata if ad else None,
                                         self.guides, max(1, self.guides_done), pr.s1 if ad else None,
                                         pr.s2 if ad else None, pr.batch_strata if ad else 0, self.params,
                                         self.workspace, self.out, self.var)

    def variance(self):
        return self.var

    def reset(self, frame=None):
        """Camera moved: the wrapped renderer restarts (its moments with it), guides and variance are cleared."""
        super().reset(frame)
        with self.torch.cuda.stream(self.stream):
            self.var.zero_()
