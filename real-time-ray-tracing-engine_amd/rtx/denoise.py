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
"""
import ctypes as C

import numpy as np

from . import abi
from .lib import check, load
from .ppm import to_bytes

LUMA = (0.2126, 0.7152, 0.0722)
B3 = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)


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


def workspace_bytes(frame):
    """rt_denoise_workspace_bytes: four float4 planes, each padded to 256 B."""
    plane = (frame.image_width * frame.image_height * 16 + 255) & ~255
    return 4 * plane


def _pixel_scale(tile_strata, frame):
    tx, ty = (frame.image_width + 7) // 8, (frame.image_height + 7) // 8
    s = 1.0 / np.maximum(1, np.asarray(tile_strata)).astype(np.float64)
    s = np.repeat(np.repeat(s.reshape(ty, tx), 8, axis=0), 8, axis=1)
    return s[:frame.image_height, :frame.image_width]


class NumpyOps:
    """rt_denoise_device on host arrays, in fp64: the statement of record."""

    def workspace_bytes(self, frame):
        return workspace_bytes(frame)

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

    def one_pass(self, e, n, z, h, k, sn, sz, sh, sc):
        H, W = e.shape[:2]
        s = 1 << k
        with np.errstate(invalid="ignore", over="ignore"):
            y = LUMA[0] * e[..., 0] + LUMA[1] * e[..., 1] + LUMA[2] * e[..., 2]
        ok = np.isfinite(e).all(-1)
        sw = np.zeros((H, W))
        se = np.zeros((H, W, 3))
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
                    d = float(s * max(abs(di), abs(dj)))
                    x = np.zeros_like(w)
                    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                        if sn is not None:
                            x = x + ((n[P] - n[Q]) ** 2).sum(-1) / sn ** 2
                        if sz is not None:
                            x = x + np.abs(z[P] - z[Q]) / (sz * np.maximum(np.maximum(z[P], z[Q]), 1e-30) * d)
                        if sh is not None:
                            x = x + (h[P] - h[Q]) ** 2 / sh ** 2
                        if sc is not None:
                            ck = sc * 2.0 ** -k
                            t = ((e[P] - e[Q]) ** 2).sum(-1) / (ck ** 2 * (y[P] ** 2 + 1e-4))
                            x = x + np.where(ok[P], t, 0.0)
                        w = w * np.exp(-np.minimum(x, 80.0))
                    w = np.where(np.isnan(x), 0.0, w)
                w = np.where(ok[Q], w, 0.0)
                sw[P] += w
                se[P] += w[..., None] * np.where(ok[Q][..., None], e[Q], 0.0)
        some = sw > 0
        return np.where(some[..., None], se / np.where(some, sw, 1.0)[..., None], e)

    def denoise(self, frame, rgb, scale, tile_strata, guides, guide_strata, params=None):
        """-> [H, W, 3] float64: the filtered, scaled radiance."""
        if guide_strata < 1:
            raise ValueError("guide_strata must be >= 1")
        passes, sn, sz, sh, sc = resolve(params)
        e, a_d, n, z, h = self.prepare(frame, rgb, scale, tile_strata, guides, guide_strata)
        for k in range(passes):
            e = self.one_pass(e, n, z, h, k, sn, sz, sh, sc)
        return e * a_d

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

    def workspace_bytes(self, frame):
        n = C.c_int64(0)
        check(self.lib.rt_denoise_workspace_bytes(C.byref(frame), C.byref(n)))
        return n.value

    def workspace(self, frame):
        """A workspace tensor for `frame` (torch allocations are 512-B aligned)."""
        t = self.torch
        with t.cuda.stream(self.stream):
            return t.empty((self.workspace_bytes(frame),), dtype=t.uint8, device=self.device)

    def denoise(self, frame, rgb, scale, tile_strata, guides, guide_strata, params=None, workspace=None,
                out=None):
        t = self.torch
        if workspace is None:
            workspace = self.workspace(frame)
        if out is None:
            with t.cuda.stream(self.stream):
                out = t.empty((frame.image_height, frame.image_width, 3), dtype=t.float64, device=self.device)
        p = abi.denoise_params(params)
        check(self.lib.rt_denoise_device(
            C.byref(frame), C.c_void_p(rgb.data_ptr()), C.c_double(scale),
            C.c_void_p(tile_strata.data_ptr() if tile_strata is not None else 0),
            C.c_void_p(guides.data_ptr()), int(guide_strata), C.byref(p) if p is not None else None,
            C.c_void_p(workspace.data_ptr()), C.c_void_p(out.data_ptr()), self._sp()))
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
        self.workspace = self.ops.workspace(f)
        self._shape = (f.image_width, f.image_height)
        self.guides_done = 0

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
        """Camera moved: the wrapped renderer restarts, the guides are cleared."""
        self.pr.reset(frame)
        if (self.pr.frame.image_width, self.pr.frame.image_height) != self._shape:
            self._allocate()
            return
        with self.torch.cuda.stream(self.stream):
            self.guides.zero_()
        self.guides_done = 0
