"""Host-side mirror of the reference's StaticCamera for the HIP path.

    StaticCamera(config, out).render(world, lights)   (StaticCamera.cpp:25-30)
 -> Renderer(scene).render(camera) / render_ppm(...)

Camera setup, scene upload, the render launch and the PPM writer are the
reference's steps; the per-pixel work runs in the HIP kernel behind the C ABI.
"""
import ctypes as C

import numpy as np

from . import abi
from .lib import check, load
from .ppm import write_ppm


def _move_arrays(ids, centres):
    ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1, 3)
    if len(ids) != len(centres):
        raise ValueError("%d ids, %d centres" % (len(ids), len(centres)))
    return ids, centres


def describe_move(scene, ids, centres):
    """The move in the SceneDescription: the centre, and for a sphere given by
    its two centres the second one shifted by the same vector (the device keeps
    the displacement c1 - c0; the stored form holds that displacement itself)."""
    for i, c in zip(ids, centres):
        o = scene.objects[int(i)]
        if o.moving == 1:
            o.b = abi.Vec3.of([o.b.x + (c[0] - o.a.x), o.b.y + (c[1] - o.a.y), o.b.z + (c[2] - o.a.z)])
        o.a = abi.Vec3.of([float(c[0]), float(c[1]), float(c[2])])


def rotate_y_row(degrees):
    """The set_transforms row of a rotate_y by `degrees`: (sin, cos, 0) exactly
    as scene creation computes them (rt_rotate_y_sincos)."""
    sn, cs = C.c_double(), C.c_double()
    check(load().rt_rotate_y_sincos(float(degrees), C.byref(sn), C.byref(cs)))
    return [sn.value, cs.value, 0.0]


def describe_transforms(scene, ids, values):
    """set_transforms in the SceneDescription: a translate gets its offset, a
    rotate_y becomes the stored form (moving = RT_STORED_FORM, a = (sin, cos, 0))."""
    for i, v in zip(ids, values):
        o = scene.objects[int(i)]
        if o.kind == abi.RT_OBJ_ROTATE_Y:
            o.moving = abi.RT_STORED_FORM
            o.a = abi.Vec3.of([float(v[0]), float(v[1]), 0.0])
        else:
            o.a = abi.Vec3.of([float(v[0]), float(v[1]), float(v[2])])


def describe_quads(scene, ids, corners):
    """move_quads in the SceneDescription: the corner Q."""
    for i, c in zip(ids, corners):
        scene.objects[int(i)].a = abi.Vec3.of([float(c[0]), float(c[1]), float(c[2])])


# rt_ray / rt_ray_hit as NumPy records (the layouts of abi.Ray / abi.RayHit)
RAY_DTYPE = np.dtype([("origin", "<f8", 3), ("direction", "<f8", 3), ("time", "<f8"), ("t_max", "<f8")])
HIT_DTYPE = np.dtype([("t", "<f8"), ("p", "<f8", 3), ("n", "<f8", 3), ("object", "<i4"),
                      ("chain_object", "<i4"), ("material", "<i4"), ("front", "<i4")])
# rt_motion as a NumPy record (the layout of abi.Motion)
MOTION_DTYPE = np.dtype([("d", "<f8", 3), ("dn", "<f8", 3), ("t", "<f8"), ("object", "<i4"), ("chain_object", "<i4")])


def ray_array(rays):
    """Rays as a contiguous RAY_DTYPE array [n]: from one, or from an [n, 8]
    float64 array of rows (origin xyz, direction xyz, time, t_max)."""
    a = np.asarray(rays)
    if a.dtype == RAY_DTYPE:
        return np.ascontiguousarray(a).reshape(-1)
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 8:
        raise ValueError("rays: an [n, 8] float64 array or a RAY_DTYPE array, not shape %r" % (a.shape,))
    return a.view(RAY_DTYPE).reshape(-1)


def pixel_ray(frame, x, y):
    """rt_pixel_ray: the ray through the point (x, y) of the frame's pixel grid
    ((i, j): the centre of pixel (i, j)); no jitter, no defocus, time 0, no
    t_max.  A RAY_DTYPE array [1]."""
    r = abi.Ray()
    check(load().rt_pixel_ray(C.byref(frame), float(x), float(y), C.byref(r)))
    return np.frombuffer(bytes(r), dtype=RAY_DTYPE).copy()


def _trace(fn, handle, rays):
    rays = ray_array(rays)
    hits = np.empty(len(rays), dtype=HIT_DTYPE)
    check(fn(handle, len(rays), C.c_void_p(rays.ctypes.data), C.c_void_p(hits.ctypes.data)))
    return hits


def segment_ray(a, b, time=0.0):
    """rt_segment_ray for each pair of points: the rays that ask whether b[k]
    is visible from a[k] (origin a, direction b - a, t_max 0.999).  a, b: [n, 3]
    (or [3]) float64; a RAY_DTYPE array [n]."""
    a = np.ascontiguousarray(np.atleast_2d(np.asarray(a, dtype=np.float64)))
    b = np.ascontiguousarray(np.atleast_2d(np.asarray(b, dtype=np.float64)))
    if a.shape != b.shape or a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("a, b: two [n, 3] arrays, not %r and %r" % (a.shape, b.shape))
    rays = np.empty(len(a), dtype=RAY_DTYPE)
    fn, D = load().rt_segment_ray, C.POINTER(C.c_double)
    r = abi.Ray()
    for k in range(len(a)):
        check(fn(a[k].ctypes.data_as(D), b[k].ctypes.data_as(D), float(time), C.byref(r)))
        rays[k:k + 1] = np.frombuffer(bytes(r), dtype=RAY_DTYPE)
    return rays


def _occluded(fn, handle, rays):
    rays = ray_array(rays)
    out = np.empty(len(rays), dtype=np.bool_)
    check(fn(handle, len(rays), C.c_void_p(rays.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out


def camera_rays(frame, seed, stratum, rows=(0, 0)):
    """rt_camera_rays: the render's own camera ray of stratum `stratum` for
    every pixel of rows [rows[0], rows[1]) ((0, 0): the whole frame), row-major
    -- jitter, defocus origin and ray time from Key{seed; j * W + i, stratum},
    t_max = inf.  A RAY_DTYPE array [rows * W]."""
    r0, r1 = int(rows[0]), int(rows[1])
    n_rows = frame.image_height if (r0 == 0 and r1 == 0) else r1 - r0
    rays = np.empty(max(0, n_rows) * max(0, frame.image_width), dtype=RAY_DTYPE)
    check(load().rt_camera_rays(C.byref(frame), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stratum), r0, r1,
                                C.c_void_p(rays.ctypes.data)))
    return rays


def radiance_params(samples=1, seed=0, max_depth=50, background=(0, 0, 0), first_key=0, first_sample=0,
                    accumulate=0):
    """An abi.RadianceParams (rt_radiance_params)."""
    p = abi.RadianceParams()
    p.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    p.first_key = int(first_key) & 0xFFFFFFFF
    p.first_sample, p.samples, p.max_depth = int(first_sample), int(samples), int(max_depth)
    p.accumulate = int(accumulate)
    p.background = abi.Vec3.of(background.tolist() if isinstance(background, abi.Vec3) else background)
    return p


def _radiance(fn, handle, rays, out, **kw):
    rays = ray_array(rays)
    accumulate = out is not None  # a caller's array is added onto
    if out is None:
        out = np.empty((len(rays), 3), dtype=np.float64)
    if out.dtype != np.float64 or not out.flags.c_contiguous or out.shape != (len(rays), 3):
        raise ValueError("out: a C-contiguous float64 array [%d, 3]" % len(rays))
    p = radiance_params(accumulate=1 if accumulate else 0, **kw)
    check(fn(handle, len(rays), C.c_void_p(rays.ctypes.data), C.byref(p), C.c_void_p(out.ctypes.data)))
    return out


def camera_frame(cam):
    """Camera::initialize (Camera.cpp:31-73) via rt_camera_setup."""
    f = abi.Frame()
    check(load().rt_camera_setup(C.byref(cam), C.byref(f)))
    return f


class Renderer:
    """Owns one device-side scene (rt_scene) on one GPU.  `tuning`: None (the
    default plan), an abi.Tuning or a dict of its fields (rt_scene_create_tuned)."""

    def __init__(self, scene, device=0, tuning=None):
        self.lib = load()
        self.scene_desc = scene
        self._desc = scene.desc()
        self._tuning = abi.tuning(tuning)
        h = C.c_void_p()
        t = C.byref(self._tuning) if self._tuning is not None else None
        check(self.lib.rt_scene_create_tuned(C.byref(self._desc), int(device), t, C.byref(h)))
        self.handle = h
        self.device = device

    def close(self):
        if self.handle:
            self.lib.rt_scene_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        i = abi.SceneInfo()
        check(self.lib.rt_scene_info_get(self.handle, C.byref(i)))
        return {k: getattr(i, k) for k, _ in abi.SceneInfo._fields_}

    @staticmethod
    def params(seed=0, rows=(0, 0), samples=(0, -1), output=abi.RT_OUT_SCALED, accumulate=0,
               tiles=(0, 1), layout=abi.RT_LAYOUT_FRAME, chunks=1):
        p = abi.RenderParams()
        p.row_begin, p.row_end = int(rows[0]), int(rows[1])
        p.sample_begin, p.sample_count = int(samples[0]), int(samples[1])
        p.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        p.output = int(output)
        p.accumulate = int(accumulate)
        p.tile_first, p.tile_stride = int(tiles[0]), int(tiles[1])
        p.layout = int(layout)
        p.strata_chunks = int(chunks)
        return p

    @staticmethod
    def local_tiles(frame, rows=(0, 0), tiles=(0, 1)):
        """Number of 8x8 tiles a launch with this tile subset renders."""
        r0, r1 = rows
        if r0 == 0 and r1 == 0:
            r1 = frame.image_height
        n = ((frame.image_width + 7) // 8) * ((r1 - r0 + 7) // 8)
        first, stride = tiles[0], max(1, tiles[1])
        return max(0, (n - first + stride - 1) // stride)

    def render(self, frame, seed=0, rows=(0, 0), samples=(0, -1), output=abi.RT_OUT_SCALED,
               tiles=(0, 1), layout=abi.RT_LAYOUT_FRAME, chunks=1):
        """Synchronous render -> float64 array [rows, W, 3] (frame layout),
        [tiles, 64, 3] (tile layout) or [tiles, chunks, 64, 3] (chunks > 1), on
        the host."""
        r0, r1 = rows
        if r0 == 0 and r1 == 0:  # the ABI's "whole image"
            r1 = frame.image_height
        if layout == abi.RT_LAYOUT_TILES:
            n = self.local_tiles(frame, rows, tiles)
            shape = (n, 64, 3) if chunks <= 1 else (n, chunks, 64, 3)
            out = np.zeros(shape, dtype=np.float64)
        else:
            out = np.empty((max(0, r1 - r0), frame.image_width, 3), dtype=np.float64)
        p = self.params(seed, (r0, r1), samples, output, 0, tiles, layout, chunks)
        check(self.lib.rt_render(self.handle, C.byref(frame), C.byref(p),
                                 out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def render_into(self, frame, host_ptr, seed=0, rows=(0, 0), samples=(0, -1),
                    output=abi.RT_OUT_SCALED):
        """rt_render into caller host memory at `host_ptr` (e.g. a pinned torch
        tensor's data_ptr(), or a numpy buffer's address): kernel + D2H copy,
        synchronous -- the reference's render_gpu batch loop."""
        p = self.params(seed, rows, samples, output, 0)
        check(self.lib.rt_render(self.handle, C.byref(frame), C.byref(p),
                                 C.cast(C.c_void_p(host_ptr), C.POINTER(C.c_double))))

    def render_device(self, frame, dev_ptr, stream_ptr=None, seed=0, rows=(0, 0), samples=(0, -1),
                      output=abi.RT_OUT_SUM, accumulate=1, tiles=(0, 1), layout=abi.RT_LAYOUT_FRAME,
                      chunks=1):
        """Asynchronous render into a device buffer (e.g. a torch.cuda tensor's
        data_ptr()) on `stream_ptr` (0/None = the HIP null stream)."""
        p = self.params(seed, rows, samples, output, accumulate, tiles, layout, chunks)
        check(self.lib.rt_render_device(self.handle, C.byref(frame), C.byref(p),
                                        C.c_void_p(dev_ptr), C.c_void_p(stream_ptr or 0)))

    def render_tiles_device(self, frame, tiles_ptr, n_tiles, dev_ptr, stream_ptr=None, seed=0,
                            rows=(0, 0), samples=(0, -1), output=abi.RT_OUT_SUM, accumulate=1):
        """render_device (frame layout) restricted to the `n_tiles` 8x8 tiles
        whose row-major indices stand, ascending, in the device int32 array at
        `tiles_ptr` (rt_render_tiles_device); other pixels stay untouched."""
        p = self.params(seed, rows, samples, output, accumulate, chunks=0)
        check(self.lib.rt_render_tiles_device(self.handle, C.byref(frame), C.byref(p),
                                              C.c_void_p(tiles_ptr), int(n_tiles),
                                              C.c_void_p(dev_ptr), C.c_void_p(stream_ptr or 0)))

    def render_guides_device(self, frame, dev_ptr, stream_ptr=None, seed=0, rows=(0, 0), samples=(0, -1),
                             accumulate=1):
        """First-hit guide sums of those strata (rt_render_guides_device) into
        the device buffer [rows, W, abi.RT_GUIDE_CHANNELS] float64 at `dev_ptr`:
        albedo r,g,b; normal x,y,z; depth; hits -- added (accumulate 1) or
        written (0), asynchronously on `stream_ptr`."""
        p = self.params(seed, rows, samples, abi.RT_OUT_SUM, accumulate, chunks=0)
        check(self.lib.rt_render_guides_device(self.handle, C.byref(frame), C.byref(p),
                                               C.c_void_p(dev_ptr), C.c_void_p(stream_ptr or 0)))

    def stats(self, frame, seed=0, rows=(0, 0), samples=(0, -1), tiles=(0, 1),
              layout=abi.RT_LAYOUT_FRAME, chunks=1):
        s = abi.PathStats()
        p = self.params(seed, rows, samples, tiles=tiles, layout=layout, chunks=chunks)
        check(self.lib.rt_render_stats(self.handle, C.byref(frame), C.byref(p), C.byref(s)))
        return {k: getattr(s, k) for k, _ in abi.PathStats._fields_}

    def bvh_cost(self):
        """SAH cost of the world BVH relative to the root box (rt_scene_bvh_cost)."""
        c = C.c_double()
        check(self.lib.rt_scene_bvh_cost(self.handle, C.byref(c)))
        return c.value

    def last_kernel_ms(self):
        ms = C.c_double()
        check(self.lib.rt_last_kernel_ms(self.handle, C.byref(ms)))
        return ms.value

    def move_spheres(self, ids, centres):
        """rt_scene_move_spheres: the world spheres `ids` (object indices of the
        description) get the centres `centres` ([n, 3]); the world BVH is
        refitted on the device.  Synchronous.  The SceneDescription the
        renderer was made from is updated too, so a later Renderer(scene) or
        dump_scene(scene) describes the moved scene.  Whatever was accumulated
        before the move (progressive.py, adaptive.py, the display classes)
        describes the old scene: reset() it -- the temporal displays through
        edited(), which keeps their history along the objects' motion."""
        ids, centres = _move_arrays(ids, centres)
        check(self.lib.rt_scene_move_spheres(self.handle, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                             centres.ctypes.data_as(C.POINTER(C.c_double))))
        describe_move(self.scene_desc, ids, centres)

    def move_spheres_device(self, ids_ptr, centres_ptr, n, stream_ptr=None):
        """rt_scene_move_spheres_device: the same from device arrays (int32 [n],
        float64 [n, 3]) asynchronously on `stream_ptr`; an entry move_spheres
        would refuse is skipped.  The SceneDescription is not touched: the
        host does not see the arrays."""
        check(self.lib.rt_scene_move_spheres_device(self.handle, int(n), C.c_void_p(ids_ptr),
                                                    C.c_void_p(centres_ptr), C.c_void_p(stream_ptr or 0)))

    def _edit(self, fn, ids, values):
        ids, values = _move_arrays(ids, values)
        check(fn(self.handle, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                 values.ctypes.data_as(C.POINTER(C.c_double))))
        return ids, values

    def set_transforms(self, ids, values):
        """rt_scene_set_transforms: the translate / rotate_y objects `ids` get
        `values` ([n, 3]: an offset, or (sin, cos, ignored) -- rotate_y_row
        gives the row of an angle); every medium's world box and the world BVH
        follow on the device.  Synchronous.  The SceneDescription follows as
        with move_spheres, and as there whatever was accumulated before
        describes the old scene: reset() it, the temporal displays through
        edited()."""
        describe_transforms(self.scene_desc, *self._edit(self.lib.rt_scene_set_transforms, ids, values))

    def set_transforms_device(self, ids_ptr, values_ptr, n, stream_ptr=None):
        """rt_scene_set_transforms_device: the same from device arrays (int32
        [n], float64 [n, 3]) asynchronously on `stream_ptr`; an entry
        set_transforms would refuse is skipped.  The SceneDescription is not
        touched."""
        check(self.lib.rt_scene_set_transforms_device(self.handle, int(n), C.c_void_p(ids_ptr),
                                                      C.c_void_p(values_ptr), C.c_void_p(stream_ptr or 0)))

    def move_quads(self, ids, corners):
        """rt_scene_move_quads: the quads `ids` (world primitives or entries of
        the lights list) get the corners Q `corners` ([n, 3]); u and v stay.
        Synchronous; the SceneDescription follows."""
        describe_quads(self.scene_desc, *self._edit(self.lib.rt_scene_move_quads, ids, corners))

    def move_quads_device(self, ids_ptr, corners_ptr, n, stream_ptr=None):
        """rt_scene_move_quads_device: the same from device arrays,
        asynchronously on `stream_ptr`; the SceneDescription is not touched."""
        check(self.lib.rt_scene_move_quads_device(self.handle, int(n), C.c_void_p(ids_ptr),
                                                  C.c_void_p(corners_ptr), C.c_void_p(stream_ptr or 0)))

    def rebuild_bvh(self):
        """rt_scene_rebuild_bvh: a new world BVH over the spheres where they
        are now, built on the device -- the tree, info() and bvh_cost() of a
        Renderer freshly made from the moved description with the device SAH
        builder.  Synchronous.  True when the new tree was taken; False when
        the scene keeps its refitted tree (a flat world, a tree too deep)."""
        took = C.c_int32(0)
        check(self.lib.rt_scene_rebuild_bvh(self.handle, C.byref(took)))
        return bool(took.value)

    def trace(self, rays):
        """rt_trace: the closest surface along each ray ([n, 8] float64 rows of
        origin, direction, time, t_max, or a RAY_DTYPE array) as a HIT_DTYPE
        array [n]: t, p, n, and the hit's `object` (what move_spheres /
        move_quads take), `chain_object` (what set_transforms takes; -1: none),
        `material` and `front`.  Constant media are passed through; a miss has
        object -1 and t = inf.  Synchronous."""
        return _trace(self.lib.rt_trace, self.handle, rays)

    def trace_device(self, rays_ptr, hits_ptr, n, stream_ptr=None):
        """rt_trace_device: the same from a device array of n rt_ray into a
        device array of n rt_ray_hit, asynchronously on `stream_ptr`, after
        every edit queued before it."""
        check(self.lib.rt_trace_device(self.handle, int(n), C.c_void_p(rays_ptr), C.c_void_p(hits_ptr),
                                       C.c_void_p(stream_ptr or 0)))

    def pose_bytes(self):
        """rt_scene_pose_bytes: the size of one pose of this scene (a multiple of 256)."""
        n = C.c_int64(0)
        check(self.lib.rt_scene_pose_bytes(self.handle, C.byref(n)))
        return n.value

    def pose_device(self, ptr, stream_ptr=None):
        """rt_scene_pose_device: the scene's movable state -- what move_spheres,
        set_transforms and move_quads write -- as it stands after every edit
        queued so far, into the device buffer of pose_bytes() at `ptr` (256-B
        aligned), asynchronously on `stream_ptr`.  Only motion_device reads it;
        it survives rebuild_bvh()."""
        check(self.lib.rt_scene_pose_device(self.handle, C.c_void_p(ptr), C.c_void_p(stream_ptr or 0)))

    def motion_device(self, frame, pose_ptr, out_ptr, stream_ptr=None):
        """rt_motion_device: per pixel of `frame`, row-major, one MOTION_DTYPE
        record into the device array at `out_ptr` -- where the surface under the
        pixel centre stood when the pose at `pose_ptr` was taken, minus where it
        is (d), the same for its unit normal (dn), and trace's t, object and
        chain_object of pixel_ray(frame, i, j).  Asynchronous on `stream_ptr`,
        after every edit queued before it."""
        check(self.lib.rt_motion_device(self.handle, C.byref(frame), C.c_void_p(pose_ptr), C.c_void_p(out_ptr),
                                        C.c_void_p(stream_ptr or 0)))

    def pick(self, frame, x, y):
        """What lies under the point (x, y) of the frame: the hit of
        pixel_ray(frame, x, y), one HIT_DTYPE record."""
        return self.trace(pixel_ray(frame, x, y))[0]

    def occluded(self, rays):
        """rt_occluded: for each ray (as for trace) whether anything stands in
        (0.001, t_max] of it -- True exactly where trace's record is a hit --
        as an np.bool_ array [n].  An any-hit search: it stops at the first
        blocker and never looks beyond t_max.  Synchronous."""
        return _occluded(self.lib.rt_occluded, self.handle, rays)

    def occluded_device(self, rays_ptr, out_ptr, n, stream_ptr=None):
        """rt_occluded_device: the same from a device array of n rt_ray into n
        device bytes (0 or 1; a bool buffer does), asynchronously on
        `stream_ptr`, after every edit queued before it."""
        check(self.lib.rt_occluded_device(self.handle, int(n), C.c_void_p(rays_ptr), C.c_void_p(out_ptr),
                                          C.c_void_p(stream_ptr or 0)))

    def visible(self, a, b, time=0.0):
        """Whether b[k] is seen from a[k] ([n, 3] each): not occluded along
        segment_ray(a, b, time).  An np.bool_ array [n]."""
        return ~self.occluded(segment_ray(a, b, time))

    def radiance(self, rays, samples=1, seed=0, max_depth=50, background=(0, 0, 0), first_key=0,
                 first_sample=0, out=None):
        """rt_radiance: the path-traced light arriving along each ray (as for
        trace; t_max is not read) as a float64 array [n, 3] of raw sums over
        `samples` samples -- sample s of ray k is the render's own path under
        Key{seed; first_key + k, first_sample + s}, with the render's
        max_depth rule and `background` for a miss.  The caller scales.  `out`:
        an [n, 3] float64 array the samples are added onto (accumulate); it
        is returned.  With camera_rays(frame, seed, k), first_sample=k and the
        frame's max_depth and background this is stratum k of
        render(..., output=RT_OUT_SUM).  Synchronous."""
        return _radiance(self.lib.rt_radiance, self.handle, rays, out, samples=samples, seed=seed,
                         max_depth=max_depth, background=background, first_key=first_key,
                         first_sample=first_sample)

    def radiance_device(self, rays_ptr, rgb_ptr, n, samples=1, seed=0, max_depth=50, background=(0, 0, 0),
                        first_key=0, first_sample=0, accumulate=0, stream_ptr=None):
        """rt_radiance_device: the same from a device array of n rt_ray into a
        device array of 3 n doubles (written, or added onto with accumulate),
        asynchronously on `stream_ptr`, after every edit queued before it."""
        p = radiance_params(samples, seed, max_depth, background, first_key, first_sample, accumulate)
        check(self.lib.rt_radiance_device(self.handle, int(n), C.c_void_p(rays_ptr), C.byref(p),
                                          C.c_void_p(rgb_ptr), C.c_void_p(stream_ptr or 0)))


class MultiRenderer:
    """rt_multi_*: one device scene per shard (shard k on devices[k % len]),
    one host thread per shard, 8x8 tiles dealt round-robin; the multi-device
    form of StaticCamera::render_gpu (StaticCamera.cpp:136-313)."""

    def __init__(self, scene, devices=(0,), shards=None, tuning=None):
        self.lib = load()
        self.scene_desc = scene
        self._desc = scene.desc()
        self._tuning = abi.tuning(tuning)
        devs = (C.c_int32 * len(devices))(*devices)
        self.n_shards = int(shards or len(devices))
        h = C.c_void_p()
        t = C.byref(self._tuning) if self._tuning is not None else None
        check(self.lib.rt_multi_create_tuned(C.byref(self._desc), devs, len(devices),
                                             self.n_shards, t, C.byref(h)))
        self.handle = h

    def close(self):
        if self.handle:
            self.lib.rt_multi_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def render(self, frame, seed=0, rows=(0, 0), samples=(0, -1), output=abi.RT_OUT_SCALED,
               chunks=0):
        r0, r1 = rows
        if r0 == 0 and r1 == 0:
            r1 = frame.image_height
        out = np.empty((max(0, r1 - r0), frame.image_width, 3), dtype=np.float64)
        p = Renderer.params(seed, (r0, r1), samples, output, 0, (0, 1), abi.RT_LAYOUT_FRAME, chunks)
        check(self.lib.rt_multi_render(self.handle, C.byref(frame), C.byref(p),
                                       out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def move_spheres(self, ids, centres):
        """rt_multi_move_spheres: Renderer.move_spheres on every shard's scene."""
        ids, centres = _move_arrays(ids, centres)
        check(self.lib.rt_multi_move_spheres(self.handle, len(ids), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                             centres.ctypes.data_as(C.POINTER(C.c_double))))
        describe_move(self.scene_desc, ids, centres)

    _edit = Renderer._edit

    def set_transforms(self, ids, values):
        """rt_multi_set_transforms: Renderer.set_transforms on every shard's scene."""
        describe_transforms(self.scene_desc, *self._edit(self.lib.rt_multi_set_transforms, ids, values))

    def move_quads(self, ids, corners):
        """rt_multi_move_quads: Renderer.move_quads on every shard's scene."""
        describe_quads(self.scene_desc, *self._edit(self.lib.rt_multi_move_quads, ids, corners))

    def trace(self, rays):
        """rt_multi_trace: Renderer.trace on shard 0's scene."""
        return _trace(self.lib.rt_multi_trace, self.handle, rays)

    def occluded(self, rays):
        """rt_multi_occluded: Renderer.occluded on shard 0's scene."""
        return _occluded(self.lib.rt_multi_occluded, self.handle, rays)

    def radiance(self, rays, samples=1, seed=0, max_depth=50, background=(0, 0, 0), first_key=0,
                 first_sample=0, out=None):
        """rt_multi_radiance: Renderer.radiance on shard 0's scene."""
        return _radiance(self.lib.rt_multi_radiance, self.handle, rays, out, samples=samples,
                         seed=seed, max_depth=max_depth, background=background, first_key=first_key,
                         first_sample=first_sample)

    def rebuild_bvh(self):
        """rt_multi_rebuild_bvh: Renderer.rebuild_bvh on every shard's scene;
        True only if every shard took its new tree."""
        took = C.c_int32(0)
        check(self.lib.rt_multi_rebuild_bvh(self.handle, C.byref(took)))
        return bool(took.value)

    def shard_ms(self):
        ms = (C.c_double * self.n_shards)()
        check(self.lib.rt_multi_shard_ms(self.handle, ms))
        return list(ms)

    def gather_ms(self):
        """Host ms of the last render's device exchange (slowest shard's render
        end -> frame assembled on shard 0's device; D2H excluded)."""
        ms = C.c_double()
        check(self.lib.rt_multi_gather_ms(self.handle, C.byref(ms)))
        return ms.value


def render_ppm(scene, path, device=0, seed=0, **cam_overrides):
    """StaticCamera::render on the HIP path: camera setup, render, PPM."""
    cam = scene.camera_desc(**cam_overrides)
    frame = camera_frame(cam)
    with Renderer(scene, device) as R:
        img = R.render(frame, seed=seed)
    write_ppm(path, img)
    return img
