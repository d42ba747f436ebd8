"""Temporal reprojection: the display keeps its history across camera moves.

rtx.progressive, rtx.adaptive and rtx.denoise clear everything when the camera
moves, as the reference does, and the viewer is back at 1-spp noise behind the
filter.  Here the image displayed at the previous pose is carried into the new
pose wherever the same first-hit surface is still visible, and blended with
the new pose's samples by sample count (rt_temporal_device); the a-trous filter
then runs on the blend.  The fp64 accumulator stays the source of truth and is
only read; the library keeps no state.

A history is two fp32 float4 planes of the frame's size, each padded to 256 B:
col = (e.r, e.g, e.b, count), geo = (n.x, n.y, n.z, z).  It always travels
with the rt_frame it was taken at.

The definition (NumpyOps.temporal, fp64).  With the filter's quantities (see
rtx.denoise: c, a_d = max(albedo / g, 0.01), e = c / a_d, n, h, z) and the
current count n_c = strata_now, or with tile_strata the pixel's tile's strata,
per pixel p = (i, j):

 1. position: d = pixel00_loc + i pixel_delta_u + j pixel_delta_v - center,
    P = center + z d / |d|.  This is the pixel-centre ray; z is the mean
    first-hit distance of jittered (and, with defocus, lens-sampled) rays, so
    with jitter or defocus P is an approximation of where the samples hit.
 2. projection into the previous frame (c', pixel00', du', dv'): v = P - c',
    N' = du' x dv', num = (pixel00' - c') . N', den = v . N'.  History is
    possible only if den num > 0 (P in front of the previous camera) and
    h >= hit_min.  q = c' + (num / den) v - pixel00', x = q . du' / du' . du',
    y = q . dv' / dv' . dv', r = |v|.
 3. four bilinear taps (floor x + a, floor y + b), a, b in {0, 1}, weight w.
    A tap is valid when it lies inside the image, its count' > 0, its e' is
    finite, |n - n'_q|^2 <= sigma_normal^2, and the surface test passes: with
    |n|^2 >= 0.25, P'_q = c' + z'_q d'_q / |d'_q| (the tap's own pixel-centre
    ray) lies within sigma_depth r of the plane through P with normal n / |n|
    (a plane distance: a surface seen at a grazing angle survives, where a
    plain depth difference between neighbouring pixels would not); with
    |n|^2 < 0.25 (a medium: its guide normal is 0) |z'_q - r| <= sigma_depth r.
 4. Wv = sum of the valid w.  Wv > 0: e_h = sum w e'_q / Wv,
    n_h = min(sum w count'_q, max_history) -- the count sum is not
    renormalised, so a partly valid footprint weighs less and Wv needs no
    threshold.  Otherwise n_h = 0.
 5. e_out = (n_h e_h + n_c e) / (n_h + n_c), 0 when both counts are 0;
    out = e_out a_d -- what rt_denoise_device takes as device_rgb with
    rgb_scale 1 and no tile strata.  history_out: col = fp32(e_out, n_h + n_c),
    the count stored as 0 when h < hit_min or e_out is not finite (a
    non-finite current e passes through to out); geo = fp32(n, z).
 6. without a previous history n_h = 0 everywhere, out = c up to the division
    and multiplication by a_d, and a first history is written.

Stateless by construction: history_prev is the snapshot committed at the last
camera move; every displayed frame at the current pose is computed from it and
the current accumulator, so nothing compounds from frame to frame.  On a move
the host swaps: the last displayed frame's history_out becomes history_prev
(TemporalDisplay.reset).

Temporal variance (NumpyOps.temporal_variance, rt_temporal_variance_device;
TemporalVarianceDisplay).  TemporalDisplay's filter knows nothing of how
converged the blend is, and VarianceGuidedDisplay forgets it on a move.  A
variance history has a third plane, var (fp32 [H, W], padded to 256 B, behind
col and geo: its first history_bytes are a plain history): the variance v of
the Rec. 709 luminance of e, rtx.denoise's unit.  Everything above is unchanged,
bit for bit; added per pixel:

 7. v_c = variance_now[p], 0 when that is NaN or negative.  With Wv > 0,
    v_h = sum w max(v'_q, 0) / Wv over the valid taps (a NaN v'_q is 0; a tap
    of weight 0 adds nothing, an infinite one included).  Linear in w, not
    sum w^2 v' / Wv^2: after one reprojection neighbouring history pixels
    share taps and are correlated, crediting the interpolation with a variance
    reduction would compound over moves, and an overestimate only keeps the
    filter wider.  max_history caps n_h and leaves v_h alone.
 8. with a = n_h / total, b = n_c / total: v_out = a^2 v_h + b^2 v_c, a term
    whose count is 0 dropped (not multiplied), 0 when total = 0; without
    history b = 1 and v_out = v_c exactly.  variance_out = v_out (float64);
    history var = fp32(v_out), 0 wherever the count is stored as 0.

rtx.denoise's denoise_given_variance then filters the blend with v_out.

Object motion (NumpyOps.temporal(motion=) / temporal_variance(motion=),
rt_temporal_motion_device / rt_temporal_variance_motion_device;
TemporalDisplay.edited).  After Renderer.move_spheres, set_transforms or
move_quads the history describes the scene before the edit.  A pose
(Renderer.pose_device) is a device snapshot of what those edits write;
Renderer.motion_device gives per pixel a render.MOTION_DTYPE record: d, where
the surface point under the pixel centre stood at the pose minus where it is,
dn, the same for its unit normal, and trace's t / object / chain_object.

 9. with a motion plane, a pixel with |n|^2 >= 0.25 (a surface), a hit record
    (object >= 0) and d, dn not all zero substitutes P_m = P + d for P in step
    2 (v, den, x, y, r) and in step 3's plane test, n_m = n + dn for n in the
    normal test, and n_m / |n_m| for n / |n| as the plane's normal.  What is
    written is unchanged: geo = (n, z) is the current pose's.  Every other
    pixel -- media, misses, unmoved surfaces -- takes steps 1 to 8 as they
    are, so an all-zero plane gives the same bits; a non-finite d gives a NaN
    x and no history.

Out of scope: moving media (fog pixels keep the camera-only reprojection: a
caller who moves a medium's transform still calls clear()); lighting that
changes under a static pixel -- a moved shadow or reflection -- lags by at
most max_history, as reflections and refractions, reprojected at their
first-hit point, already do; motion-blurred spheres carry their blur in every
frame's time average and move as their time-0 centre does.
"""
import ctypes as C

import numpy as np

from . import abi
from .denoise import DenoisedDisplay, VarianceGuidedDisplay
from .denoise import NumpyOps as _FilterOps
from .lib import check, load


def resolve(params=None):
    """(max_history, sigma_depth, sigma_normal, hit_min) of None / a dict / an
    abi.TemporalParams: 0 = the default, a sigma < 0 = its test off (returned
    as None)."""
    p = abi.temporal_params(params) or abi.TemporalParams()
    if p.max_history < 0:
        raise ValueError("max_history must be >= 0")

    def pick(v, d):
        return d if v == 0 else float(v)

    sz = pick(p.sigma_depth, abi.RT_TEMPORAL_SIGMA_DEPTH)
    sn = pick(p.sigma_normal, abi.RT_TEMPORAL_SIGMA_NORMAL)
    return (float(p.max_history or abi.RT_TEMPORAL_MAX_HISTORY), None if sz < 0 else sz, None if sn < 0 else sn,
            pick(p.hit_min, abi.RT_TEMPORAL_HIT_MIN))


def history_bytes(frame):
    """rt_history_bytes: two float4 planes, each padded to 256 B."""
    return 2 * ((frame.image_width * frame.image_height * 16 + 255) & ~255)


def pack_history(frame, history):
    """(col, geo) float32 [H, W, 4] arrays -> the device layout, a uint8 array of history_bytes."""
    n = frame.image_width * frame.image_height * 16
    buf = np.zeros(history_bytes(frame), dtype=np.uint8)
    for k, a in enumerate(history):
        a = np.ascontiguousarray(a, dtype=np.float32)
        buf[k * (len(buf) // 2):k * (len(buf) // 2) + n] = a.reshape(-1).view(np.uint8)
    return buf


def unpack_history(frame, buf):
    """The device layout -> (col, geo) float32 [H, W, 4]."""
    h, w = frame.image_height, frame.image_width
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    half = len(buf) // 2
    return tuple(buf[k * half:k * half + h * w * 16].view(np.float32).reshape(h, w, 4).copy() for k in range(2))


def history_variance_bytes(frame):
    """rt_history_variance_bytes: a history and the var plane (fp32 scalars, padded to 256 B) behind it."""
    return history_bytes(frame) + ((frame.image_width * frame.image_height * 4 + 255) & ~255)


def pack_variance_history(frame, history):
    """(col, geo, var) -> the device layout, a uint8 array of history_variance_bytes."""
    n = frame.image_width * frame.image_height * 4
    hb = history_bytes(frame)
    buf = np.zeros(history_variance_bytes(frame), dtype=np.uint8)
    buf[:hb] = pack_history(frame, history[:2])
    buf[hb:hb + n] = np.ascontiguousarray(history[2], dtype=np.float32).reshape(-1).view(np.uint8)
    return buf


def unpack_variance_history(frame, buf):
    """The device layout -> (col, geo, var): float32 [H, W, 4] twice and [H, W]."""
    h, w = frame.image_height, frame.image_width
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    hb = history_bytes(frame)
    return unpack_history(frame, buf[:hb]) + (buf[hb:hb + h * w * 4].view(np.float32).reshape(h, w).copy(),)


def _cam(frame):
    def v(a):
        return np.array([a.x, a.y, a.z], dtype=np.float64)
    return v(frame.center), v(frame.pixel00_loc), v(frame.pixel_delta_u), v(frame.pixel_delta_v)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _centre_points(cam, ii, jj, z):
    """c + z d / |d| along the pixel-centre rays of pixels (ii, jj)."""
    c, p00, du, dv = cam
    d = p00 + ii[..., None] * du + jj[..., None] * dv - c
    with np.errstate(invalid="ignore", over="ignore"):
        return c + (z / np.sqrt(_dot(d, d)))[..., None] * d


def _pixel_tiles(tile_strata, frame):
    tx, ty = (frame.image_width + 7) // 8, (frame.image_height + 7) // 8
    s = np.maximum(0, np.asarray(tile_strata)).astype(np.float64).reshape(ty, tx)
    return np.repeat(np.repeat(s, 8, axis=0), 8, axis=1)[:frame.image_height, :frame.image_width]


class NumpyOps:
    """rt_temporal_device on host arrays, in fp64: the statement of record."""

    def history_bytes(self, frame):
        return history_bytes(frame)

    def history_variance_bytes(self, frame):
        return history_variance_bytes(frame)

    def temporal(self, frame_now, rgb, scale, tile_strata, strata_now, guides, guide_strata, frame_prev=None,
                 history_prev=None, params=None, motion=None):
        """-> (out [H, W, 3] float64, (col, geo) float32 [H, W, 4] each, margin [H, W]).
        motion: rt_temporal_motion_device's plane, a render.MOTION_DTYPE array
        [H, W] (step 9 of the module's definition); None: rt_temporal_device.

        margin: the smallest |lhs - rhs| / rhs over the surface and normal
        comparisons of the pixel's taps with w > 1e-6 (inf where it has none):
        a pixel with a tiny margin sits on a threshold, where another rounding
        of the same arithmetic may decide the other way."""
        return self._temporal(frame_now, rgb, scale, tile_strata, strata_now, guides, guide_strata, frame_prev,
                              history_prev, params, None, motion)

    def temporal_variance(self, frame_now, rgb, scale, tile_strata, strata_now, guides, guide_strata, variance_now,
                          frame_prev=None, history_prev=None, params=None, motion=None):
        """rt_temporal_variance_device -> (out, (col, geo, var), variance_out
        [H, W] float64, margin); history_prev is a (col, geo, var) triple, var
        float32 [H, W].  out, col, geo and margin are temporal()'s; motion as there."""
        return self._temporal(frame_now, rgb, scale, tile_strata, strata_now, guides, guide_strata, frame_prev,
                              history_prev, params, variance_now, motion)

    def _temporal(self, frame_now, rgb, scale, tile_strata, strata_now, guides, guide_strata, frame_prev,
                  history_prev, params, variance_now, motion=None):
        """temporal() and, with variance_now, temporal_variance(): the colour is stated once."""
        if guide_strata < 1:
            raise ValueError("guide_strata must be >= 1")
        if (frame_prev is None) != (history_prev is None):
            raise ValueError("frame_prev and history_prev go together")
        mh, sz, sn, hmin = resolve(params)
        H, W = frame_now.image_height, frame_now.image_width
        e, a_d, n, z, h = _FilterOps().prepare(frame_now, rgb, scale, tile_strata, guides, guide_strata)
        n_c = _pixel_tiles(tile_strata, frame_now) if tile_strata is not None else np.full((H, W), float(strata_now))
        n_h, e_h, margin = np.zeros((H, W)), np.zeros((H, W, 3)), np.full((H, W), np.inf)
        with_var = variance_now is not None
        v_h = np.zeros((H, W))
        if history_prev is not None:
            if (frame_prev.image_width, frame_prev.image_height) != (W, H):
                raise ValueError("frame_prev has another size than frame_now")
            if len(history_prev) != (3 if with_var else 2):
                raise ValueError("a variance history is (col, geo, var), a plain one (col, geo)")
            col, geo = (np.asarray(a, dtype=np.float64) for a in history_prev[:2])
            if with_var:
                var = np.asarray(history_prev[2], dtype=np.float64)
                with np.errstate(invalid="ignore"):
                    var = np.where(var > 0.0, var, 0.0)  # a NaN or negative v': 0
            sv = np.zeros((H, W))
            jj, ii = np.mgrid[0:H, 0:W]
            prev = _cam(frame_prev)
            cp, p00p, dup, dvp = prev
            P = _centre_points(_cam(frame_now), ii, jj, z)
            nn = _dot(n, n)
            plane = nn >= 0.25
            nu = (1.0 / np.sqrt(np.where(plane, nn, 1.0)))[..., None] * n
            n_t = n  # the normal the taps' normals are held to
            if motion is not None:  # step 9: a moved surface pixel projects where its point stood
                motion = np.asarray(motion)
                if motion.shape != (H, W):
                    raise ValueError("motion must be a MOTION_DTYPE array [H, W]")
                d, dn = motion["d"].astype(np.float64), motion["dn"].astype(np.float64)
                moved = plane & (motion["object"] >= 0) & ((d != 0).any(-1) | (dn != 0).any(-1))
                with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                    P = np.where(moved[..., None], P + d, P)  # selected, not added: P + 0 is not always P's bits
                    n_t = np.where(moved[..., None], n + dn, n)
                    nn_t = _dot(n_t, n_t)
                    nu = np.where(moved[..., None], (1.0 / np.sqrt(np.where(moved, nn_t, 1.0)))[..., None] * n_t, nu)
            Np = np.cross(dup, dvp)
            with np.errstate(invalid="ignore", over="ignore"):  # a non-finite d: a NaN x, no history
                v = P - cp
                num, den = _dot(p00p - cp, Np), _dot(v, Np)
                r = np.sqrt(_dot(v, v))
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                q = cp + (num / den)[..., None] * v - p00p
                x, y = _dot(q, dup) / _dot(dup, dup), _dot(q, dvp) / _dot(dvp, dvp)
                possible = (den * num > 0) & (h >= hmin) & (x > -1) & (x < W) & (y > -1) & (y < H)
            x, y = np.where(possible, x, 0.0), np.where(possible, y, 0.0)
            fx, fy = np.floor(x), np.floor(y)
            x0, y0, wx, wy = fx.astype(np.int64), fy.astype(np.int64), x - fx, y - fy
            Wv, cnt, se = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W, 3))
            for b in (0, 1):
                for a in (0, 1):
                    qx, qy = x0 + a, y0 + b
                    inside = possible & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                    w = (wx if a else 1.0 - wx) * (wy if b else 1.0 - wy)
                    cq, gq = col[cy, cx], geo[cy, cx]
                    ok = inside & (cq[..., 3] > 0) & np.isfinite(cq[..., :3]).all(-1)
                    near = inside & (w > 1e-6)
                    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                        if sn is not None:
                            dq = n_t - gq[..., :3]
                            lhs = _dot(dq, dq)
                            ok &= lhs <= sn * sn
                            margin = np.fmin(margin, np.where(near, np.abs(lhs - sn * sn) / (sn * sn), np.inf))
                        if sz is not None:
                            Pq = _centre_points(prev, cx, cy, gq[..., 3])
                            dist = np.where(plane, np.abs(_dot(nu, Pq - P)), np.abs(gq[..., 3] - r))
                            ok &= dist <= sz * r
                            margin = np.fmin(margin, np.where(near, np.abs(dist - sz * r) / (sz * r), np.inf))
                    w = np.where(ok, w, 0.0)
                    Wv += w
                    cnt += w * np.where(ok, cq[..., 3], 0.0)
                    se += w[..., None] * np.where(ok[..., None], cq[..., :3], 0.0)
                    if with_var:  # linear in w, not w^2: neighbouring history pixels share taps
                        sv += w * np.where(w > 0, var[cy, cx], 0.0)  # w = 0: nothing, an infinite v' included
            some = Wv > 0
            n_h = np.where(some, np.minimum(cnt, mh), 0.0)
            e_h = np.where(some[..., None], se / np.where(some, Wv, 1.0)[..., None], 0.0)
            v_h = np.where(some, sv / np.where(some, Wv, 1.0), 0.0)  # the cap bounds the count, not the variance
        total = n_h + n_c
        with np.errstate(invalid="ignore", over="ignore"):
            e_out = (n_h[..., None] * e_h + n_c[..., None] * e) / np.where(total > 0, total, 1.0)[..., None]
            e_out = np.where((total > 0)[..., None], e_out, 0.0)
            out = e_out * a_d
            count = np.where((h >= hmin) & np.isfinite(e_out).all(-1), total, 0.0)
            col_out = np.concatenate([e_out, count[..., None]], axis=-1).astype(np.float32)
            geo_out = np.concatenate([n, z[..., None]], axis=-1).astype(np.float32)
        if not with_var:
            return out, (col_out, geo_out), margin
        v_c = np.asarray(variance_now, dtype=np.float64)
        if v_c.shape != (H, W):
            raise ValueError("variance_now must be [H, W]")
        with np.errstate(invalid="ignore", over="ignore"):
            v_c = np.where(v_c > 0.0, v_c, 0.0)  # a NaN or negative variance: 0
            div = np.where(total > 0, total, 1.0)
            a, b = n_h / div, n_c / div
            # a term whose count is 0 is dropped, not multiplied (0 inf); no history: b = 1, v_c itself
            v_out = np.where(n_h > 0, (a * a) * np.where(n_h > 0, v_h, 0.0), 0.0) \
                + np.where(n_c > 0, (b * b) * np.where(n_c > 0, v_c, 0.0), 0.0)
            v_out = np.where(total > 0, v_out, 0.0)
            var_out = np.where(count > 0, v_out, 0.0).astype(np.float32)
        return out, (col_out, geo_out, var_out), v_out, margin


class HipOps:
    """rt_history_bytes / rt_temporal_device on torch CUDA tensors, on one stream."""

    def __init__(self, device, stream):
        import torch
        self.torch = torch
        self.device = device
        self.stream = stream
        self.lib = load()

    def history_bytes(self, frame):
        n = C.c_int64(0)
        check(self.lib.rt_history_bytes(C.byref(frame), C.byref(n)))
        return n.value

    def history(self, frame):
        """A history tensor for `frame` (torch allocations are 512-B aligned)."""
        t = self.torch
        with t.cuda.stream(self.stream):
            return t.empty((self.history_bytes(frame),), dtype=t.uint8, device=self.device)

    def temporal(self, frame_now, rgb, scale, tile_strata, strata_now, guides, guide_strata, frame_prev=None,
                 history_prev=None, params=None, history_out=None, out=None, motion=None):
        """-> (out [H, W, 3] float64, history_out uint8), both CUDA tensors.
        motion: a CUDA tensor holding motion_device's plane for this frame
        (rt_temporal_motion_device); None: rt_temporal_device."""
        t = self.torch
        if history_out is None:
            history_out = self.history(frame_now)
        if out is None:
            with t.cuda.stream(self.stream):
                out = t.empty((frame_now.image_height, frame_now.image_width, 3), dtype=t.float64,
                              device=self.device)
        p = abi.temporal_params(params)
        if motion is not None:
            check(self.lib.rt_temporal_motion_device(
                C.byref(frame_now), C.c_void_p(rgb.data_ptr()), C.c_double(scale),
                C.c_void_p(tile_strata.data_ptr() if tile_strata is not None else 0), int(strata_now),
                C.c_void_p(guides.data_ptr()), int(guide_strata),
                C.byref(frame_prev) if frame_prev is not None else None,
                C.c_void_p(history_prev.data_ptr() if history_prev is not None else 0),
                C.c_void_p(motion.data_ptr()), C.byref(p) if p is not None else None,
                C.c_void_p(history_out.data_ptr()), C.c_void_p(out.data_ptr()),
                C.c_void_p(self.stream.cuda_stream)))
            return out, history_out
        check(self.lib.rt_temporal_device(
            C.byref(frame_now), C.c_void_p(rgb.data_ptr()), C.c_double(scale),
            C.c_void_p(tile_strata.data_ptr() if tile_strata is not None else 0), int(strata_now),
            C.c_void_p(guides.data_ptr()), int(guide_strata),
            C.byref(frame_prev) if frame_prev is not None else None,
            C.c_void_p(history_prev.data_ptr() if history_prev is not None else 0),
            C.byref(p) if p is not None else None, C.c_void_p(history_out.data_ptr()),
            C.c_void_p(out.data_ptr()), C.c_void_p(self.stream.cuda_stream)))
        return out, history_out

    def history_variance_bytes(self, frame):
        n = C.c_int64(0)
        check(self.lib.rt_history_variance_bytes(C.byref(frame), C.byref(n)))
        return n.value

    def variance_history(self, frame):
        """A variance-history tensor for `frame`."""
        t = self.torch
        with t.cuda.stream(self.stream):
            return t.empty((self.history_variance_bytes(frame),), dtype=t.uint8, device=self.device)

    def temporal_variance(self, frame_now, rgb, scale, tile_strata, strata_now, guides, guide_strata, variance_now,
                          frame_prev=None, history_prev=None, params=None, history_out=None, out=None,
                          variance_out=None, motion=None):
        """rt_temporal_variance_device -> (out [H, W, 3] float64, history_out uint8, variance_out [H, W] float64);
        with `motion` (as for temporal) rt_temporal_variance_motion_device."""
        t = self.torch
        h, w = frame_now.image_height, frame_now.image_width
        if history_out is None:
            history_out = self.variance_history(frame_now)
        with t.cuda.stream(self.stream):
            if out is None:
                out = t.empty((h, w, 3), dtype=t.float64, device=self.device)
            if variance_out is None:
                variance_out = t.empty((h, w), dtype=t.float64, device=self.device)
        p = abi.temporal_params(params)
        if motion is not None:
            check(self.lib.rt_temporal_variance_motion_device(
                C.byref(frame_now), C.c_void_p(rgb.data_ptr()), C.c_double(scale),
                C.c_void_p(tile_strata.data_ptr() if tile_strata is not None else 0), int(strata_now),
                C.c_void_p(guides.data_ptr()), int(guide_strata),
                C.byref(frame_prev) if frame_prev is not None else None,
                C.c_void_p(history_prev.data_ptr() if history_prev is not None else 0),
                C.c_void_p(motion.data_ptr()), C.c_void_p(variance_now.data_ptr()),
                C.byref(p) if p is not None else None, C.c_void_p(history_out.data_ptr()),
                C.c_void_p(out.data_ptr()), C.c_void_p(variance_out.data_ptr()),
                C.c_void_p(self.stream.cuda_stream)))
            return out, history_out, variance_out
        check(self.lib.rt_temporal_variance_device(
            C.byref(frame_now), C.c_void_p(rgb.data_ptr()), C.c_double(scale),
            C.c_void_p(tile_strata.data_ptr() if tile_strata is not None else 0), int(strata_now),
            C.c_void_p(guides.data_ptr()), int(guide_strata),
            C.byref(frame_prev) if frame_prev is not None else None,
            C.c_void_p(history_prev.data_ptr() if history_prev is not None else 0),
            C.c_void_p(variance_now.data_ptr()), C.byref(p) if p is not None else None,
            C.c_void_p(history_out.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(variance_out.data_ptr()),
            C.c_void_p(self.stream.cuda_stream)))
        return out, history_out, variance_out


class TemporalDisplay:
    """The reprojected (and, with `filter`, a-trous-filtered) display of a
    progressive.for_renderer ProgressiveRenderer or an adaptive.for_renderer
    AdaptiveRenderer `pr`.

    It drives a DenoisedDisplay over `pr` for the guides, their catch-up, the
    filter and the bytes.  image() blends the current accumulator with the
    history committed at the last camera move and, with `filter`, passes the
    blend through rt_denoise_device (`denoise`: its rt_denoise_params).
    reset(frame) is the camera move: the last displayed frame's history and
    its rt_frame are committed, the wrapped renderer and the guides restart,
    and the history is kept; a frame of another size drops it.  edited() is
    the scene edit's counterpart (after Renderer.move_spheres, set_transforms
    or move_quads): the history is committed in the same way and marked as
    moved, and until the next camera-only reset() every frame reprojects along
    the objects' motion as well (rt_motion_device once per pose, then
    rt_temporal_motion_device).  clear() forgets the history (a change no
    motion vector describes: a moved medium, another scene).  Two histories,
    two poses, the motion plane, the blend and DenoisedDisplay's buffers are
    allocated once per frame size.

        td = TemporalDisplay(progressive.for_renderer(R, frame, seed=5))
        pipe = progressive.DisplayPipeline(td, bytes_fn=td.bytes_into)
    """

    def __init__(self, pr, guide_strata=16, params=None, denoise=None, filter=True):
        self.dd = DenoisedDisplay(pr, guide_strata=guide_strata, params=denoise)
        self.pr = pr
        self.torch = self.dd.torch
        self.stream = pr.stream
        self.params = abi.temporal_params(params)
        self.filter = bool(filter)
        self.ops = HipOps(pr.acc.device, self.stream)
        self._adaptive = self.dd._adaptive
        self._allocate()

    def _allocate(self):
        t, f = self.torch, self.pr.frame
        self.hist = [self.ops.history(f), self.ops.history(f)]  # [0]: committed (prev), [1]: the displayed frame's
        with t.cuda.stream(self.stream):
            self.blend = t.empty((f.image_height, f.image_width, 3), dtype=t.float64, device=self.pr.acc.device)
        self._shape = (f.image_width, f.image_height)
        self.frame_prev = None   # the rt_frame hist[0] was taken at; None: no history
        self._shown = None       # the rt_frame hist[1] was written at by the last image()
        self._allocate_motion()

    # while the history is marked as moved and the caller's params leave these at 0: the set
    # include/rt_api.h recommends for larger per-frame motion (the shipped 0.5 depth tolerance
    # would let an uncovered floor pixel keep the sphere that stood on it)
    MOVED_PARAMS = dict(max_history=32, sigma_depth=0.02, sigma_normal=0.35)

    def _allocate_motion(self):
        """The poses (once: they belong to the scene, not to the frame size) and the motion plane."""
        t, f, R = self.torch, self.pr.frame, self.dd.renderer
        with t.cuda.stream(self.stream):
            if not hasattr(self, "pose"):  # [0]: the scene hist[0] shows, [1]: the scene as it stands
                self.pose = [t.empty((R.pose_bytes(),), dtype=t.uint8, device=self.pr.acc.device) for _ in range(2)]
                self._save_pose()
            self.motion = t.empty((f.image_height * f.image_width * 64,), dtype=t.uint8, device=self.pr.acc.device)
        self._moved = False         # hist[0] shows another pose of the scene than the current one
        self._motion_ready = False  # self.motion holds pr.frame's plane against pose[0]

    def _save_pose(self):
        self.dd.renderer.pose_device(self.pose[1].data_ptr(), self.stream.cuda_stream)

    def _motion_plane(self):
        """The motion plane of the current frame while the history is marked as moved (computed once per pose), else None."""
        if not (self._moved and self.has_history):
            return None
        if not self._motion_ready:
            self.dd.renderer.motion_device(self.pr.frame, self.pose[0].data_ptr(), self.motion.data_ptr(),
                                           self.stream.cuda_stream)
            self._motion_ready = True
        return self.motion

    def _params_now(self, moved):
        if not moved:
            return self.params
        p = abi.TemporalParams.from_buffer_copy(self.params) if self.params is not None else abi.TemporalParams()
        for k, v in self.MOVED_PARAMS.items():
            if getattr(p, k) == 0:
                setattr(p, k, v)
        return p

    # what DisplayPipeline reads of a renderer
    @property
    def acc(self):
        return self.pr.acc

    @property
    def frame(self):
        return self.pr.frame

    @property
    def samples_taken(self):
        return self.dd.samples_taken

    @property
    def converged(self):
        return self.dd.converged

    @property
    def guides(self):
        return self.dd.guides

    @property
    def guides_done(self):
        return self.dd.guides_done

    @property
    def has_history(self):
        return self.frame_prev is not None

    def step(self, n=1):
        """Steps the wrapped renderer and its guides; returns the strata traced."""
        return self.dd.step(n)

    def blended(self):
        """The blend alone ([H, W, 3] float64 CUDA tensor); writes the displayed frame's history."""
        dd, pr = self.dd, self.pr
        dd._catch_up()
        motion = self._motion_plane()
        self.ops.temporal(pr.frame, pr.acc, 1.0 if self._adaptive else pr.scale,
                          pr.tile_strata if self._adaptive else None, self.samples_taken, dd.guides,
                          max(1, dd.guides_done), self.frame_prev, self.hist[0] if self.has_history else None,
                          self._params_now(motion is not None), self.hist[1], self.blend, motion=motion)
        self._shown = abi.Frame.from_buffer_copy(pr.frame)
        return self.blend

    def image(self):
        img = self.blended()
        if not self.filter:
            return img
        dd = self.dd
        return dd.ops.denoise(self.pr.frame, img, 1.0, None, dd.guides, max(1, dd.guides_done), dd.params,
                              dd.workspace, dd.out)

    def bytes(self, out=None):
        return self.dd.ops.bytes(self.image(), out)

    def bytes_into(self, pr, out):
        """DisplayPipeline's bytes_fn: the displayed frame's bytes into `out`."""
        return self.bytes(out)

    def reset(self, frame=None):
        """Camera moved: commit the last displayed frame's history, restart the renderer and the guides."""
        if self._shown is not None:  # the poses swap exactly when the histories do
            self.hist.reverse()
            self.pose.reverse()
            self.frame_prev, self._shown = self._shown, None
            self._save_pose()
            self._moved = False  # the committed history shows the scene as it stands
        self._motion_ready = False
        self.dd.reset(frame)
        if (self.pr.frame.image_width, self.pr.frame.image_height) != self._shape:
            self._allocate()

    def edited(self):
        """The scene was edited (Renderer.move_spheres, set_transforms, move_quads, or their
        _device forms queued on any stream before this call): commit the last displayed frame's
        history exactly as reset() does -- with nothing shown, nothing swaps -- save the
        scene's new pose, restart the renderer and the guides, and mark the history as moved:
        until the next camera-only reset() commits a history of the scene as it stands,
        blended() reprojects along the objects' motion too, with MOVED_PARAMS where the
        caller's params are 0.  A moved medium has no motion vectors: clear() after it."""
        self.reset()
        self._save_pose()  # reset() saved one only if it committed; the edit may have come since
        self._moved = self.has_history

    def clear(self):
        """Forget the history: the next frames start from the samples alone.  For a change
        edited() cannot follow -- a medium's transform moved (fog pixels keep the camera-only
        reprojection), another scene behind the same display -- after reset()."""
        self.frame_prev = self._shown = None
        self._moved = self._motion_ready = False


class TemporalVarianceDisplay(TemporalDisplay):
    """TemporalDisplay and VarianceGuidedDisplay composed: the variance of the
    displayed estimate travels across camera moves with its colour, and the
    variance-guided filter runs on the blend with the blend's own variance --
    a blend that holds 64 strata of history is filtered as a 64-strata frame,
    not as the 1-stratum frame the new pose has so far.

    image() is three calls on the renderer's stream:
     1. the current variance: rt_denoise_variance_device with passes -1 and
        device_variance_out = v_now -- over an AdaptiveRenderer the batch
        moments where a tile has `min_batches` batches and the spatial estimate
        elsewhere, over a ProgressiveRenderer the spatial estimate alone;
     2. rt_temporal_variance_device: the blend, its variance v_out and the
        displayed frame's variance history;
     3. with `filter`, rt_denoise_given_variance_device(blend, scale 1, no tile
        strata, v_out).
    `denoise`: the filter's rt_denoise_variance_params.  step, blended, bytes,
    bytes_into, reset (the history swap), edited (object motion, through
    rt_temporal_variance_motion_device), clear and has_history are
    TemporalDisplay's; a frame of another size drops the history.  variance()
    is the displayed frame's variance plane ([H, W] float64): the filter's
    final v, or v_out with filter off.  Every buffer is allocated once per
    frame size.

        ar = adaptive.for_renderer(R, frame, seed=5, threshold=0, batch_strata=4)
        tv = TemporalVarianceDisplay(ar)
        pipe = progressive.DisplayPipeline(tv, bytes_fn=tv.bytes_into)
    """

    def __init__(self, pr, guide_strata=16, params=None, denoise=None, filter=True):
        self.dd = VarianceGuidedDisplay(pr, guide_strata=guide_strata, params=denoise)
        self.pr = pr
        self.torch = self.dd.torch
        self.stream = pr.stream
        self.params = abi.temporal_params(params)
        self.filter = bool(filter)
        self.ops = HipOps(pr.acc.device, self.stream)
        self._adaptive = self.dd._adaptive
        # call 1: the filter's own parameters, no pass
        q = self.dd.params
        self._estimate = abi.DenoiseVarianceParams.from_buffer_copy(q) if q is not None \
            else abi.DenoiseVarianceParams()
        self._estimate.passes = -1
        self._allocate()

    def _allocate(self):
        t, f = self.torch, self.pr.frame
        self.hist = [self.ops.variance_history(f), self.ops.variance_history(f)]
        with t.cuda.stream(self.stream):
            self.blend = t.empty((f.image_height, f.image_width, 3), dtype=t.float64, device=self.pr.acc.device)
            self.v_now = t.zeros((f.image_height, f.image_width), dtype=t.float64, device=self.pr.acc.device)
            self.v_out = t.zeros((f.image_height, f.image_width), dtype=t.float64, device=self.pr.acc.device)
        self._shape = (f.image_width, f.image_height)
        self.frame_prev = None
        self._shown = None
        self._filtered = False
        self._allocate_motion()

    def blended(self):
        """The blend alone; writes v_out and the displayed frame's variance history."""
        dd, pr, ad = self.dd, self.pr, self._adaptive
        dd._catch_up()
        g = max(1, dd.guides_done)
        scale, strata = (1.0, pr.tile_strata) if ad else (pr.scale, None)
        dd.ops.denoise_variance(pr.frame, pr.acc, scale, strata, dd.guides, g, pr.s1 if ad else None,
                                pr.s2 if ad else None, pr.batch_strata if ad else 0, self._estimate, dd.workspace,
                                dd.out, self.v_now)
        motion = self._motion_plane()
        self.ops.temporal_variance(pr.frame, pr.acc, scale, strata, self.samples_taken, dd.guides, g, self.v_now,
                                   self.frame_prev, self.hist[0] if self.has_history else None,
                                   self._params_now(motion is not None), self.hist[1], self.blend, self.v_out,
                                   motion=motion)
        self._shown = abi.Frame.from_buffer_copy(pr.frame)
        self._filtered = False
        return self.blend

    def image(self):
        img = self.blended()
        if not self.filter:
            return img
        dd = self.dd
        self._filtered = True
        return dd.ops.denoise_given_variance(self.pr.frame, img, 1.0, None, dd.guides, max(1, dd.guides_done),
                                             self.v_out, dd.params, dd.workspace, dd.out, dd.var)

    def variance(self):
        return self.dd.var if self._filtered else self.v_out
