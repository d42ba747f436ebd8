"""Guided sampling: tiles retire by the error of the displayed estimate.

rtx.temporal's TemporalVarianceDisplay carries the colour and the variance of
the displayed estimate across a camera move; the sampler (rtx.adaptive) knows
nothing of it: reset makes every tile active, and its retirement rule reads the
new pose's own batch moments, so no tile retires before min_batches batches --
a tile showing 64 strata of reprojected history included.  Here the displayed
frame's own error steers the samples: after a step the display is blended
(rt_temporal_variance_device), and a tile whose blend is good enough leaves the
active list (rt_guided_select_device), so the new pose's samples go to the
disocclusions and to whatever keeps no history.

The rule (NumpyOps.select, fp64: the statement of record).  Inputs: the col
plane of the displayed frame's variance history, fp32 (e.r, e.g, e.b, count);
the variance plane v_out of the same call; the frame; tile_strata (or
strata_now where there is none); an ascending tile list.  Per pixel p inside
the image:

    y       = 0.2126 e.r + 0.7152 e.g + 0.0722 e.b
    v       = v_out[p], 0 when that is NaN or negative (rtx.temporal's step 7)
    rel     = sqrt(v) / (y + floor), +inf when a channel of e is not finite or
              the quotient is NaN
    count_p = max(col.count, n_c), n_c the pixel's tile's strata or strata_now:
              the stored count is 0 where the hit fraction is below hit_min, and
              such a pixel still holds its own samples

Per tile: e_t is the mean of rel and c_t the minimum of count_p over the
tile's pixels inside the image; the tile is dropped when c_t >= min_count and
e_t <= threshold (a NaN e_t keeps it).  The kept tiles go to the output list in
input order.  The minimum over the counts is what makes the rule safe without a
validity mask: a tile with one disoccluded pixel has c_t = n_c and must earn
min_count samples at the new pose like any tile of rtx.adaptive.  Without a
history v_out = v_c and count = n_c: the rule then stands on the display's own
variance estimate.

List entries outside [0, tiles - 1] are clamped, as everywhere in
csrc/rt_adaptive.hip.  Retired tiles are never re-activated, and the
renderer's own moments rule keeps running as configured: a tile leaves when
either rule drops it.

Where guiding loses: a long stay at one pose.  A retired tile stops at the
error the threshold allows, so a run that would have gone on to hundreds of
strata ends worse than the plain one.
"""
import ctypes as C

import numpy as np

from . import abi
from .adaptive import LUMA, tile_grid
from .lib import check, load
from .temporal import TemporalVarianceDisplay, _pixel_tiles


class NumpyOps:
    """rt_guided_select_device on host arrays, in fp64, operation by operation
    (the kernel's 64-lane sum is a butterfly: e_t agrees to rounding; the
    counts and the list are equal)."""

    def pixel_terms(self, col, v_out, frame, tile_strata, strata_now, floor):
        """(rel, count_p), [H, W] float64 each."""
        H, W = frame.image_height, frame.image_width
        col = np.asarray(col, dtype=np.float32)
        if col.shape != (H, W, 4):
            raise ValueError("col must be [H, W, 4]")
        v = np.asarray(v_out, dtype=np.float64)
        if v.shape != (H, W):
            raise ValueError("v_out must be [H, W]")
        e = col[..., :3].astype(np.float64)
        y = LUMA[0] * e[..., 0] + LUMA[1] * e[..., 1] + LUMA[2] * e[..., 2]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            v = np.where(v > 0.0, v, 0.0)  # a NaN or negative variance: 0
            rel = np.sqrt(v) / (y + floor)
            rel = np.where(np.isfinite(e).all(-1) & ~np.isnan(rel), rel, np.inf)
            n_c = _pixel_tiles(tile_strata, frame) if tile_strata is not None else np.full((H, W), float(strata_now))
            stored = col[..., 3].astype(np.float64)
            count = np.where(stored > n_c, stored, n_c)  # a stored count of 0 (or NaN): the pixel's own samples
        return rel, count

    def select(self, col, v_out, frame, tile_strata, strata_now, threshold, floor, min_count, tiles_in, n_in,
               tiles_out, tile_error=None, tile_count=None):
        """rt_guided_select_device; returns the number of tiles kept."""
        for name, x in (("threshold", threshold), ("floor", floor), ("min_count", min_count)):
            if x != x:
                raise ValueError("%s is NaN" % name)
        if not floor > 0:
            raise ValueError("floor must be > 0")
        if tile_strata is None and strata_now < 0:
            raise ValueError("strata_now must be >= 0")
        tx, ty = tile_grid(frame)
        if n_in < 0 or n_in > tx * ty:
            raise ValueError("n_in outside [0, tiles of the frame]")
        rel, count = self.pixel_terms(col, v_out, frame, tile_strata, strata_now, floor)
        H, W = frame.image_height, frame.image_width
        kept = 0
        for t in tiles_in[:n_in]:
            t = min(max(int(t), 0), tx * ty - 1)
            x0, y0 = (t % tx) * 8, (t // tx) * 8
            box = (slice(y0, min(y0 + 8, H)), slice(x0, min(x0 + 8, W)))
            with np.errstate(invalid="ignore"):  # +inf and -inf in one tile: NaN, the tile stays
                e_t = float(rel[box].sum() / rel[box].size)
            c_t = float(count[box].min())
            if tile_error is not None:
                tile_error[t] = e_t
            if tile_count is not None:
                tile_count[t] = c_t
            if not (c_t >= min_count and e_t <= threshold):
                tiles_out[kept] = t
                kept += 1
        return kept


class HipOps:
    """rt_guided_select_device on torch CUDA tensors, on one stream."""

    def __init__(self, device, stream):
        import torch
        self.torch = torch
        self.device = device
        self.stream = stream
        self.lib = load()
        with torch.cuda.stream(stream):
            self._count = torch.zeros((1,), dtype=torch.int32, device=device)

    def select(self, history, v_out, frame, tile_strata, strata_now, threshold, floor, min_count, tiles_in, n_in,
               tiles_out, tile_error=None, tile_count=None):
        """`history`: the variance history tensor rt_temporal_variance_device
        wrote (uint8), `v_out` its variance plane; returns the number of tiles
        kept -- the one host synchronisation, 4 bytes read back."""
        def ptr(a):
            return C.c_void_p(a.data_ptr() if a is not None else 0)

        check(self.lib.rt_guided_select_device(
            C.byref(frame), ptr(history), ptr(v_out), ptr(tile_strata), int(strata_now), float(threshold),
            float(floor), float(min_count), ptr(tiles_in), int(n_in), ptr(tiles_out), ptr(self._count),
            ptr(tile_error), ptr(tile_count), C.c_void_p(self.stream.cuda_stream)))
        with self.torch.cuda.stream(self.stream):
            return int(self._count.item())


class GuidedDisplay(TemporalVarianceDisplay):
    """TemporalVarianceDisplay that also steers the sampler: over an
    adaptive.for_renderer AdaptiveRenderer `ar` only (a ProgressiveRenderer has
    no tile list: TypeError).

    step(n) steps as TemporalVarianceDisplay does; after every `check_every`-th
    step it runs blended() and rt_guided_select_device over the renderer's
    active list, and hands the kept list to the renderer
    (AdaptiveRenderer.reselect).  Each selection reads one 4-byte count back.
    blended() returns the cached blend when nothing was stepped or reset since
    it last ran, so step(); image() costs one blend.  The renderer's own
    moments rule keeps running as configured (threshold=0 leaves the guiding
    alone): a tile leaves when either rule drops it, and none comes back.
    tile_error / tile_count hold e_t / c_t of every tile's last selection (inf
    / 0 before its first).  reset, clear, bytes_into and DisplayPipeline use
    are TemporalVarianceDisplay's; the other arguments are its own.

        ar = adaptive.for_renderer(R, frame, seed=5, threshold=0, batch_strata=2)
        gd = GuidedDisplay(ar, threshold=0.2)
        pipe = progressive.DisplayPipeline(gd, bytes_fn=gd.bytes_into)
    """

    def __init__(self, ar, threshold, min_count=abi.RT_GUIDED_MIN_COUNT, floor=abi.RT_GUIDED_FLOOR, check_every=1,
                 guide_strata=16, params=None, denoise=None, filter=True):
        if not hasattr(ar, "reselect"):
            raise TypeError("GuidedDisplay runs over an adaptive.for_renderer AdaptiveRenderer: "
                            "a %s has no tile list" % type(ar).__name__)
        if check_every < 1:
            raise ValueError("check_every must be >= 1")
        if threshold != threshold or not floor > 0 or min_count != min_count:
            raise ValueError("threshold and min_count must not be NaN, floor must be > 0")
        self.threshold = float(threshold)
        self.min_count = float(min_count)
        self.floor = float(floor)
        self.check_every = int(check_every)
        super().__init__(ar, guide_strata=guide_strata, params=params, denoise=denoise, filter=filter)
        self.guided = HipOps(ar.acc.device, self.stream)

    def _allocate(self):
        super()._allocate()
        t = self.torch
        with t.cuda.stream(self.stream):
            self.tile_error = t.full((self.pr.n_tiles,), float("inf"), dtype=t.float64, device=self.pr.acc.device)
            self.tile_count = t.zeros((self.pr.n_tiles,), dtype=t.float64, device=self.pr.acc.device)
        self._fresh = False  # the blend is the current accumulator's
        self._steps = 0

    def blended(self):
        if not self._fresh:
            super().blended()
            self._fresh = True
        return self.blend

    def step(self, n=1):
        traced = super().step(n)
        if traced:
            self._fresh = False
            self._steps += 1
            if self._steps % self.check_every == 0 and self.pr.n_active > 0:
                self.select()
        return traced

    def select(self):
        """blended() and the selection over the active list; returns the number of tiles kept."""
        self.blended()
        pr = self.pr

        def fn(tiles_in, n_in, tiles_out):
            return self.guided.select(self.hist[1], self.v_out, pr.frame, pr.tile_strata, self.samples_taken,
                                      self.threshold, self.floor, self.min_count, tiles_in, n_in, tiles_out,
                                      self.tile_error, self.tile_count)
        return pr.reselect(fn)

    def reset(self, frame=None):
        shape = self._shape
        super().reset(frame)
        if self._shape == shape:  # a new size: _allocate has run
            with self.torch.cuda.stream(self.stream):
                self.tile_error.fill_(float("inf"))
                self.tile_count.zero_()
        self._fresh = False
        self._steps = 0

    def clear(self):
        super().clear()
        self._fresh = False
