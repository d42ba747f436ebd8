"""rt_radiance_device / rt_radiance / rt_multi_radiance on gfx950
(csrc/rt_radiance.hip): bit for bit the render along the render's own camera
rays in every instance, the in-lane sample loop and the position invariants
under real divergence, the host build of the same source
(tests/native/rt_radiance_emu.cpp) along rays no camera makes, the launch
chain behind an edit, and a caller's stream."""
import os

import numpy as np
import pytest
import torch

from rtx import abi
from rtx.render import RAY_DTYPE, MultiRenderer, Renderer, camera_frame, camera_rays, describe_move
from rtx.scene import load_scene
import material_worlds as MW
import oracle_lib as O
from test_material_worlds_gpu import IDS, INSTANCES, want_features
from test_radiance import SENTINEL, diffuse_flat_scene, frame_args, host_radiance, same_bytes

pytestmark = pytest.mark.gpu

SCENES = os.path.join(O.ROOT, "real-time-ray-tracing-engine_amd", "scenes")
N = 777  # not a multiple of 64 or 256: the last wave and the last block are ragged
PAD = 64  # rays' worth of sentinel after the sums


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------- the render's bits
def strata_equal_the_render(R, f, seed):
    """Every stratum of the frame: one radiance sample along rt_camera_rays'
    ray under the render's key against the render's RT_OUT_SUM of that stratum
    alone -- one sample per pixel, so no order of additions is involved."""
    H, W = f.image_height, f.image_width
    for k in range(f.sqrt_spp * f.sqrt_spp):
        want = R.render(f, seed=seed, samples=(k, 1), output=abi.RT_OUT_SUM)
        got = R.radiance(camera_rays(f, seed, k), samples=1, seed=seed, first_sample=k, **frame_args(f))
        got = got.reshape(H, W, 3)
        differ = ~((got == want) | (np.isnan(got) & np.isnan(want))).all(axis=2)
        assert np.array_equal(got, want, equal_nan=True), "stratum %d: %d of %d pixels differ, first %s, by %g" % (
            k, differ.sum(), H * W, np.argwhere(differ)[:4].tolist(),
            np.abs(np.nan_to_num(got) - np.nan_to_num(want)).max())
        assert (np.nan_to_num(want) > 0).any()  # teeth: every world has its lamp or its sky in view


@pytest.mark.parametrize("F,arity", INSTANCES, ids=IDS)
def test_radiance_along_the_renders_rays_has_the_renders_bits(F, arity):
    S = load_scene(MW.material_scene(F))
    S.bvh_arity = arity
    _, f = MW.sized(S)
    with Renderer(S) as R:
        assert R.info()["features"] == want_features(F, arity)
        strata_equal_the_render(R, f, MW.SEED)


def test_the_diffuse_twin_has_the_renders_bits():
    S = diffuse_flat_scene()
    f = camera_frame(S.camera_desc(image_width=37, aspect_ratio=1.76, samples_per_pixel=4, max_depth=6))
    assert (f.image_width, f.image_height) == (37, 21)
    with Renderer(S) as R:
        assert R.info()["features"] == abi.RT_FEAT_FLAT | abi.RT_FEAT_DIFFUSE
        strata_equal_the_render(R, f, 5)


# ---------------------------------------------------------------- guarded device calls
class Guarded:
    """n rays' sums followed by PAD rays' worth of sentinel, every byte the sentinel before the call."""

    def __init__(self, n, fill=None):
        self.n = n
        self.all = torch.full(((n + PAD) * 24,), SENTINEL, dtype=torch.uint8, device="cuda")
        if fill is not None:
            self.all[:n * 24] = torch.from_numpy(np.ascontiguousarray(fill).view(np.uint8).reshape(-1)).cuda()
        self.ptr = self.all.data_ptr()

    def read(self, written=None):
        w = self.n if written is None else written
        a = self.all.cpu().numpy()
        assert np.all(a[w * 24:] == SENTINEL), "written past ray %d" % w
        return a[:w * 24].view(np.float64).reshape(w, 3).copy()


def device_radiance(R, rays, n=None, stream=None, fill=None, **kw):
    """radiance_device on the rays' bytes; the sums of the first n, the rest of
    the buffer and the rays themselves checked untouched."""
    n = len(rays) if n is None else n
    raw = np.ascontiguousarray(rays).view(np.uint8).reshape(-1)
    d_rays = torch.from_numpy(raw.copy()).cuda()
    buf = Guarded(len(rays), fill)
    torch.cuda.synchronize()  # the fills ran on the current stream
    R.radiance_device(d_rays.data_ptr(), buf.ptr, n, stream_ptr=stream if stream is not None else _stream(), **kw)
    torch.cuda.synchronize()
    assert np.array_equal(d_rays.cpu().numpy(), raw), "the ray buffer was written"
    return buf.read(n)


def probe_rays(n=N, seed=3):
    """Rays no camera makes: origins inside the 555 room, uniform directions of
    any length, random times."""
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=RAY_DTYPE)
    r["origin"] = rng.uniform(30, 525, (n, 3))
    d = rng.normal(size=(n, 3))
    r["direction"] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.3, 2.5, (n, 1))
    r["time"] = rng.uniform(0, 1, n)
    r["t_max"] = np.inf
    r.setflags(write=False)
    return r


def room(F, arity=0):
    S = load_scene(MW.material_scene(F))
    S.bvh_arity = arity
    return S, MW.sized(S)[1]


# ---------------------------------------------------------------- invariants on the device
@pytest.mark.parametrize("F,arity", [(31, 0), (16, 0), (5, 4)], ids=["F31", "F16", "F5-bvh4"])
def test_sample_ranges_and_positions_on_the_device(F, arity):
    S, f = room(F, arity)
    rays = probe_rays()
    kw = dict(seed=9, first_key=1000, **frame_args(f))
    with Renderer(S) as R:
        whole = device_radiance(R, rays, samples=4, first_sample=3, **kw)
        assert np.abs(np.nan_to_num(whole)).max() > 0.1
        # one call with four samples = four single-sample calls chained with accumulate
        chained = np.zeros((N, 3))
        for s in range(4):
            chained = device_radiance(R, rays, samples=1, first_sample=3 + s, fill=chained, accumulate=1, **kw)
        assert same_bytes(whole, chained)
        # [3, 7) = [3, 5) then [5, 7)
        halves = device_radiance(R, rays, samples=2, first_sample=3, **kw)
        halves = device_radiance(R, rays, samples=2, first_sample=5, fill=halves, accumulate=1, **kw)
        assert same_bytes(whole, halves)
        # a slice of the call = the call on the slice under its keys; n short of the arrays
        for a, b in ((0, 1), (63, 65), (300, 777), (776, 777)):
            part = device_radiance(R, rays[a:b], samples=4, first_sample=3, **dict(kw, first_key=1000 + a))
            assert same_bytes(part, whole[a:b]), (a, b)
        assert same_bytes(device_radiance(R, rays, n=130, samples=4, first_sample=3, **kw), whole[:130])
        # the host arrays' entry points
        assert same_bytes(R.radiance(rays, samples=4, first_sample=3, **kw), whole)
        onto = R.radiance(rays, samples=2, first_sample=5, out=R.radiance(rays, samples=2, first_sample=3, **kw), **kw)
        assert same_bytes(onto, whole)
        # nothing to do: nothing queued, nothing written
        R.radiance_device(0, 0, 0)
        assert len(device_radiance(R, rays, n=0, samples=4, **kw)) == 0
        keep = device_radiance(R, rays, samples=0, fill=whole, accumulate=1, **kw)
        assert same_bytes(keep, whole)
        assert same_bytes(device_radiance(R, rays, samples=0, **kw), np.zeros((N, 3)))
        assert same_bytes(device_radiance(R, rays, samples=4, **dict(kw, max_depth=0)), np.zeros((N, 3)))
        # bad rays among good ones: 0 for them, the others unchanged
        mixed = rays.copy()
        mixed["direction"][5] = 0.0
        mixed["origin"][70, 1] = np.nan
        mixed["time"][776] = np.inf
        mixed["t_max"][9] = np.nan  # not read
        got = device_radiance(R, mixed, samples=4, first_sample=3, **kw)
        bad = [5, 70, 776]
        assert same_bytes(got[bad], np.zeros((3, 3)))
        assert same_bytes(np.delete(got, bad, 0), np.delete(whole, bad, 0))
    if F == 31:
        with MultiRenderer(S, devices=(0,), shards=2) as M:
            assert same_bytes(M.radiance(rays, samples=4, first_sample=3, **kw), whole)


# ---------------------------------------------------------------- the host build
@pytest.mark.parametrize("F,arity", [(31, 0), (16, 0), (5, 4)], ids=["F31", "F16", "F5-bvh4"])
def test_device_against_the_host_build_on_probe_rays(F, arity):
    """DESIGN.md section 5 item 3's bar for gfx950 against the host: the mean
    of 16 samples within 1e-4 per channel, equal NaN masks."""
    S, f = room(F, arity)
    rays = probe_rays()
    kw = dict(samples=16, seed=21, first_key=5, **frame_args(f))
    with Renderer(S) as R:
        assert R.info()["features"] == want_features(F, arity)
        gpu = device_radiance(R, rays, **kw) / 16
    host = host_radiance(S, rays, **kw) / 16
    d = np.abs(np.nan_to_num(gpu) - np.nan_to_num(host))
    print("F=%d arity %d: max |gpu - host| of the 16-sample mean = %.3g over %d rays (%d lit)" % (
        F, arity, d.max(), N, (np.nan_to_num(host) > 0).any(axis=1).sum()))
    assert np.array_equal(np.isnan(gpu), np.isnan(host))
    assert not (d > 1e-4).any(), "%d channels off, max %g" % ((d > 1e-4).sum(), d.max())
    assert (np.nan_to_num(host) > 0).any(axis=1).sum() > N // 2


# ---------------------------------------------------------------- the launch chain
def test_an_edit_queued_before_a_radiance_call_is_seen_by_it():
    S, f = room(0)
    rays = probe_rays()
    kw = dict(samples=2, seed=4, **frame_args(f))
    o = next(i for i, ob in enumerate(S.objects) if ob.kind == abi.RT_OBJ_SPHERE)
    new = np.array([[S.objects[o].a.x + 60.0, S.objects[o].a.y + 40.0, S.objects[o].a.z - 30.0]])
    st = torch.cuda.Stream()
    with Renderer(S) as R:
        before = R.radiance(rays, **kw)
        ids = torch.tensor([o], dtype=torch.int32, device="cuda")
        cen = torch.from_numpy(new).cuda()
        d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()).cuda()
        buf = Guarded(N)
        torch.cuda.synchronize()
        # the edit and the query on one stream, no host wait between them
        R.move_spheres_device(ids.data_ptr(), cen.data_ptr(), 1, st.cuda_stream)
        R.radiance_device(d_rays.data_ptr(), buf.ptr, N, stream_ptr=st.cuda_stream, **kw)
        st.synchronize()
        moved = buf.read()
        assert same_bytes(R.radiance(rays, **kw), moved)
    assert not same_bytes(moved, before)
    describe_move(S, [o], new)
    with Renderer(S) as R2:  # a scene created where the sphere now is
        assert same_bytes(R2.radiance(rays, **kw), moved)


def test_radiance_device_on_a_callers_stream():
    S = load_scene(os.path.join(SCENES, "cornell_fog.json"))
    f = camera_frame(S.camera_desc(image_width=37, aspect_ratio=1.76, samples_per_pixel=4, max_depth=6))
    assert (f.image_width, f.image_height) == (37, 21)
    rays = camera_rays(f, 8, 1)
    assert len(rays) == N
    kw = dict(samples=3, seed=8, first_sample=1, **frame_args(f))
    other = torch.cuda.Stream()
    with Renderer(S) as R:
        want = R.radiance(rays, **kw)
        with torch.cuda.stream(other):
            d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()).cuda()
            rgb = torch.full((N, 3), -7.25, dtype=torch.float64, device="cuda")
            R.radiance_device(d_rays.data_ptr(), rgb.data_ptr(), N, stream_ptr=other.cuda_stream, **kw)
        other.synchronize()
        assert same_bytes(rgb.cpu().numpy(), want)
        # destroyed right after the call: destroy waits for the scene's own launch
        rgb.fill_(-7.25)
        torch.cuda.synchronize()
        R.radiance_device(d_rays.data_ptr(), rgb.data_ptr(), N, stream_ptr=other.cuda_stream, **kw)
    assert other.query(), "destroy returned before its scene's radiance call finished"
    assert same_bytes(rgb.cpu().numpy(), want)
    assert np.abs(want).max() > 0.1
