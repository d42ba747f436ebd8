"""Adaptive sampling: progressive accumulation that stops tracing what has converged.

rtx.progressive traces every stratum of every pixel.  Here the frame's 8x8
tiles carry a convergence estimate, and a tile whose estimate falls below a
threshold is retired: later batches are launched over the list of tiles still
active (rt_render_tiles_device), so smooth regions stop costing samples while
fog boundaries, glass and penumbrae go on.

Estimator.  Strata are traced in batches of `batch_strata`; a batch gives each
pixel one batch mean y (the luminance 0.2126 r + 0.7152 g + 0.0722 b of the
batch's sample sum / batch_strata).  Per pixel the moments s1 = sum y and
s2 = sum y^2 over b batches give mean = s1 / b, the sample variance
var = max(0, (s2 - s1^2 / b) / (b - 1)) and the standard error of the mean
se = sqrt(var / b).  A tile's error is the average over its pixels inside the
image of se / (mean + floor); `floor` keeps dark pixels from dominating.
The batches are consecutive strata of one stratified grid, not independent
draws: stratification makes the true error of the mean smaller than the
batch-to-batch scatter suggests, so the estimate errs high -- tiles retire
late, never early on that account.

Retirement.  After an update, every `check_every` batches, a tile is retired
when it has b >= max(2, min_batches) batches and its error <= threshold.  A
retired tile is never traced again (no re-activation); its pixels hold exactly
the static render's sample sum over strata [0, n_t) -- the random stream is
keyed by (seed, pixel, stratum) -- and are displayed with the tile's own scale
1 / n_t.  The renderer stops when no tile is active or every stratum has been
traced.  A last batch shorter than batch_strata is added to the accumulator
and the tiles' counts, not to the moments.

One host synchronisation: after each reselection the host reads the 4-byte
count of active tiles back -- it sizes the next launch.  Everything else is
queued on the stream.

The arithmetic is pluggable (`ops`), like the render function: NumpyOps below
states it in plain NumPy -- the specification the HIP kernels are tested
against (tests/test_adaptive_gpu.py), and what tests run on the CPU with the
oracle as the render function; `for_renderer` wires the HIP entry points.
"""
import ctypes as C

import numpy as np

from . import abi
from .lib import check, load
from .ppm import to_bytes

LUMA = (0.2126, 0.7152, 0.0722)


def tile_grid(frame):
    """(tiles_x, tiles_y) of the frame's 8x8 tiles; tile t = ty * tiles_x + tx."""
    return (frame.image_width + 7) // 8, (frame.image_height + 7) // 8


def _tile_box(frame, t):
    tx, _ = tile_grid(frame)
    x0, y0 = (t % tx) * 8, (t // tx) * 8
    return slice(y0, min(y0 + 8, frame.image_height)), slice(x0, min(x0 + 8, frame.image_width))


class NumpyOps:
    """include/rt_api.h's adaptive entry points on host arrays, operation by
    operation (the kernels match acc / s1 / s2 bit for bit, the tile error to
    rounding: its 64-lane sum is grouped differently)."""

    def zeros(self, shape, dtype):
        return np.zeros(shape, dtype=dtype)

    def fill(self, a, v):
        a[...] = v

    def set_all_tiles(self, lst):
        lst[:] = np.arange(lst.shape[0], dtype=np.int32)

    def host(self, a):
        return np.array(a)

    def add_strata(self, tile_strata, tiles, n, count):
        """tile_strata[t] += count for the listed tiles (a final short batch)."""
        tile_strata[tiles[:n]] += count

    def update(self, delta, batch_strata, tiles, n, frame, acc, s1, s2, tile_strata):
        """rt_adaptive_update_device."""
        bs = float(batch_strata)
        for t in tiles[:n]:
            ys, xs = _tile_box(frame, int(t))
            d = delta[ys, xs]
            acc[ys, xs] += d
            y = (LUMA[0] * d[..., 0] + LUMA[1] * d[..., 1] + LUMA[2] * d[..., 2]) / bs
            s1[ys, xs] += y
            s2[ys, xs] += y * y
            tile_strata[t] += batch_strata

    def tile_error_of(self, s1, s2, b, frame, t, floor):
        """One tile's error from b batches: the average over its pixels inside
        the image (the box is clipped to it) of se / (mean + floor)."""
        if b < 2:
            return np.inf
        ys, xs = _tile_box(frame, int(t))
        a1, a2, fb = s1[ys, xs], s2[ys, xs], float(b)
        mean = a1 / fb
        var = (a2 - a1 * a1 / fb) / (fb - 1.0)
        var = np.where(var > 0.0, var, 0.0)
        se = np.sqrt(var / fb)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = se / (mean + floor)
        return float(rel.sum() / rel.size)

    def select(self, s1, s2, tile_strata, batch_strata, frame, threshold, floor, min_batches,
               tiles_in, n_in, tiles_out, tile_error):
        """rt_adaptive_select_device; returns the number of tiles kept."""
        kept = 0
        for t in tiles_in[:n_in]:
            b = int(tile_strata[t]) // int(batch_strata)
            e = self.tile_error_of(s1, s2, b, frame, t, floor)
            if tile_error is not None:
                tile_error[t] = e
            if not (b >= max(2, int(min_batches)) and e <= threshold):
                tiles_out[kept] = t
                kept += 1
        return kept

    def pixel_scale(self, tile_strata, frame):
        """[H, W] map of 1 / max(1, tile_strata[tile of the pixel])."""
        tx, ty = tile_grid(frame)
        s = 1.0 / np.maximum(1, np.asarray(tile_strata)).astype(np.float64)
        s = np.repeat(np.repeat(s.reshape(ty, tx), 8, axis=0), 8, axis=1)
        return s[:frame.image_height, :frame.image_width]

    def image(self, acc, tile_strata, frame):
        return self.pixel_scale(tile_strata, frame)[..., None] * acc

    def bytes(self, acc, tile_strata, frame):
        """rt_to_bytes_tiles_device."""
        return to_bytes(self.image(acc, tile_strata, frame))


class AdaptiveRenderer:
    """render_tiles_fn(frame, out, seed, (first_stratum, count), tiles, n_tiles,
    accumulate) must write (accumulate 0) or add (1) the raw sample sums of
    those strata for the pixels of the listed tiles of `out` ([H, W, 3]
    float64) and touch no other pixel; `tiles` is an ascending int32 list of
    row-major tile indices, of which the first n_tiles count."""

    def __init__(self, render_tiles_fn, ops, frame, seed=0, threshold=0.0, floor=1e-3, min_batches=8,
                 batch_strata=1, check_every=1):
        if batch_strata < 1 or check_every < 1:
            raise ValueError("batch_strata and check_every must be >= 1")
        self.render_tiles_fn = render_tiles_fn
        self.ops = ops
        self.frame = frame
        self.seed = seed
        self.threshold = float(threshold)
        self.floor = float(floor)
        self.min_batches = int(min_batches)
        self.batch_strata = int(batch_strata)
        self.check_every = int(check_every)
        self._allocate()

    def _allocate(self):
        f, o = self.frame, self.ops
        tx, ty = tile_grid(f)
        self.n_tiles = tx * ty
        hw = (f.image_height, f.image_width)
        self.acc = o.zeros(hw + (3,), np.float64)
        self.delta = o.zeros(hw + (3,), np.float64)
        self.s1 = o.zeros(hw, np.float64)
        self.s2 = o.zeros(hw, np.float64)
        self.tile_strata = o.zeros((self.n_tiles,), np.int32)
        self.tile_error = o.zeros((self.n_tiles,), np.float64)
        self._lists = [o.zeros((self.n_tiles,), np.int32), o.zeros((self.n_tiles,), np.int32)]
        self._shape = (f.image_width, f.image_height)
        self._restart()

    def _restart(self):
        o = self.ops
        self._cur = 0
        o.set_all_tiles(self._lists[0])
        o.fill(self.tile_error, float("inf"))
        self.n_active = self.n_tiles
        self.strata_done = 0   # strata every active tile has traced
        self.batches = 0       # full batches in the moments of the active tiles

    @property
    def total_strata(self):
        return self.frame.sqrt_spp * self.frame.sqrt_spp

    @property
    def done(self):
        return self.n_active == 0 or self.strata_done >= self.total_strata

    @property
    def active_tiles(self):
        """The active tiles, ascending (a host copy: waits for the stream)."""
        return self.ops.host(self._lists[self._cur])[:self.n_active]

    @property
    def strata_traced(self):
        """Pixel-strata paid for so far: sum over tiles of strata x 64 (whole
        wavefronts trace edge tiles too).  Reads the counts back."""
        return int(self.ops.host(self.tile_strata).astype(np.int64).sum()) * 64

    def step(self):
        """Trace the next batch of the active tiles; returns the strata per
        pixel traced (0 once done).  Every check_every-th batch ends with the
        reselection and its one host synchronisation (the count read back)."""
        if self.done:
            return 0
        o, f = self.ops, self.frame
        tiles = self._lists[self._cur]
        n = min(self.batch_strata, self.total_strata - self.strata_done)
        strata = (self.strata_done, n)
        if n == self.batch_strata:
            self.render_tiles_fn(f, self.delta, self.seed, strata, tiles, self.n_active, 0)
            o.update(self.delta, n, tiles, self.n_active, f, self.acc, self.s1, self.s2, self.tile_strata)
            self.batches += 1
            if self.batches % self.check_every == 0:
                out = self._lists[self._cur ^ 1]
                self.n_active = int(o.select(self.s1, self.s2, self.tile_strata, self.batch_strata, f,
                                             self.threshold, self.floor, self.min_batches, tiles,
                                             self.n_active, out, self.tile_error))
                self._cur ^= 1
        else:  # the last, shorter batch: samples count, the moments keep whole batches
            self.render_tiles_fn(f, self.acc, self.seed, strata, tiles, self.n_active, 1)
            o.add_strata(self.tile_strata, tiles, self.n_active, n)
        self.strata_done += n
        return n

    def reselect(self, fn):
        """A selection rule from outside (rtx.guided): fn(tiles_in, n_in,
        tiles_out) -> kept writes the tiles of tiles_in[:n_in] that stay, in
        order, into tiles_out; the lists are swapped and n_active set.
        Returns the number kept.  step()'s own rule is untouched."""
        tiles, out = self._lists[self._cur], self._lists[self._cur ^ 1]
        self.n_active = int(fn(tiles, self.n_active, out))
        self._cur ^= 1
        return self.n_active

    def image(self):
        """The displayed radiance: every pixel scaled by 1 / max(1, its tile's strata)."""
        return self.ops.image(self.acc, self.tile_strata, self.frame)

    def bytes(self):
        """write_color bytes [H, W, 3] of image() (uint8)."""
        return self.ops.bytes(self.acc, self.tile_strata, self.frame)

    def reset(self, frame=None):
        """Camera moved: clear every buffer, all tiles active again.
        Also after Renderer.move_spheres: what was accumulated (the sums and the moments) describes the old
        scene, and nothing here notices the move -- the caller calls reset()."""
        if frame is not None:
            self.frame = frame
        if (self.frame.image_width, self.frame.image_height) != self._shape:
            self._allocate()
            return
        for a in (self.acc, self.delta, self.s1, self.s2, self.tile_strata):
            self.ops.fill(a, 0)
        self._restart()


class HipOps:
    """The ops on torch CUDA tensors: the hot arithmetic in librtx_hip's
    kernels (rt_adaptive_*_device, rt_to_bytes_tiles_device) on one stream."""

    _DT = {np.float64: "float64", np.int32: "int32"}

    def __init__(self, device, stream):
        import torch
        self.torch = torch
        self.device = device
        self.stream = stream
        self.lib = load()
        with torch.cuda.stream(stream):
            self._count = torch.zeros((1,), dtype=torch.int32, device=device)

    def _sp(self):
        return C.c_void_p(self.stream.cuda_stream)

    def zeros(self, shape, dtype):
        t = self.torch
        with t.cuda.stream(self.stream):
            return t.zeros(shape, dtype=getattr(t, self._DT[dtype]), device=self.device)

    def fill(self, a, v):
        with self.torch.cuda.stream(self.stream):
            a.fill_(v)

    def set_all_tiles(self, lst):
        t = self.torch
        with t.cuda.stream(self.stream):
            lst.copy_(t.arange(lst.shape[0], dtype=t.int32, device=self.device))

    def host(self, a):
        with self.torch.cuda.stream(self.stream):
            return a.cpu().numpy()

    def add_strata(self, tile_strata, tiles, n, count):
        with self.torch.cuda.stream(self.stream):  # once per run: bookkeeping, not a hot path
            tile_strata[tiles[:n].long()] += count

    def update(self, delta, batch_strata, tiles, n, frame, acc, s1, s2, tile_strata):
        check(self.lib.rt_adaptive_update_device(
            C.c_void_p(delta.data_ptr()), int(batch_strata), C.c_void_p(tiles.data_ptr()), int(n),
            C.byref(frame), C.c_void_p(acc.data_ptr()), C.c_void_p(s1.data_ptr()),
            C.c_void_p(s2.data_ptr()), C.c_void_p(tile_strata.data_ptr()), self._sp()))

    def select(self, s1, s2, tile_strata, batch_strata, frame, threshold, floor, min_batches,
               tiles_in, n_in, tiles_out, tile_error):
        check(self.lib.rt_adaptive_select_device(
            C.c_void_p(s1.data_ptr()), C.c_void_p(s2.data_ptr()), C.c_void_p(tile_strata.data_ptr()),
            int(batch_strata), C.byref(frame), float(threshold), float(floor), int(min_batches),
            C.c_void_p(tiles_in.data_ptr()), int(n_in), C.c_void_p(tiles_out.data_ptr()),
            C.c_void_p(self._count.data_ptr()),
            C.c_void_p(tile_error.data_ptr() if tile_error is not None else 0), self._sp()))
        with self.torch.cuda.stream(self.stream):
            return int(self._count.item())  # the one host synchronisation

    def image(self, acc, tile_strata, frame):
        t = self.torch
        tx, ty = tile_grid(frame)
        with t.cuda.stream(self.stream):
            s = 1.0 / t.clamp(tile_strata, min=1).to(t.float64)
            s = s.reshape(ty, tx).repeat_interleave(8, 0).repeat_interleave(8, 1)
            return s[:frame.image_height, :frame.image_width, None] * acc

    def bytes(self, acc, tile_strata, frame, out=None):
        t = self.torch
        if out is None:
            with t.cuda.stream(self.stream):
                out = t.empty(acc.shape, dtype=t.uint8, device=self.device)
        check(self.lib.rt_to_bytes_tiles_device(
            C.c_void_p(acc.data_ptr()), C.c_void_p(tile_strata.data_ptr()), C.byref(frame),
            C.c_void_p(out.data_ptr()), self._sp()))
        return out


def for_renderer(renderer, frame, seed=0, threshold=0.0, floor=1e-3, min_batches=8, batch_strata=1,
                 check_every=1, device=None, stream=None):
    """An AdaptiveRenderer over librtx_hip on a torch CUDA device."""
    import torch
    dev = torch.device("cuda", renderer.device if device is None else device)
    st = stream if stream is not None else torch.cuda.current_stream(dev)

    def render_tiles_fn(fr, out, sd, strata, tiles, n, accumulate):
        renderer.render_tiles_device(fr, tiles.data_ptr(), n, out.data_ptr(), st.cuda_stream, seed=sd,
                                     samples=strata, output=abi.RT_OUT_SUM, accumulate=accumulate)

    ar = AdaptiveRenderer(render_tiles_fn, HipOps(dev, st), frame, seed, threshold, floor, min_batches,
                          batch_strata, check_every)
    ar.stream = st
    ar.renderer = renderer  # rtx.denoise.DenoisedDisplay launches its guides on it
    return ar
