"""rt_render_guides_device on gfx950 against the host build of the same source
(csrc/rt_guides.h through tests/native/rt_guides_emu.cpp): bit for bit, the
accumulate split, guards, refusals, scene lifetime, and the render frames
around a guide launch.

Frames (tests/test_guides.py FRAMES): cornell_fog 36x36 (5x5 tiles, ragged
last row and column, the rich instance), three_spheres 72x40 (flat),
bouncing_seed42 72x40 (BVH, moving spheres), cornell 40x40 (quads, boxes
under RotateY / Translate, lights)."""
import ctypes as C

import numpy as np
import pytest
import torch

from rtx import abi
from rtx.lib import load
from rtx.render import Renderer
from test_guides import FRAMES, SEED, guide_frame, host_guides

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
GUARD = 4096  # doubles on each side of the buffer
CH = abi.RT_GUIDE_CHANNELS


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """A guide buffer [H, W, 8] between two sentinel-filled guards."""

    def __init__(self, f):
        self.n = f.image_height * f.image_width * CH
        self.shape = (f.image_height, f.image_width, CH)
        self.all = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        self.ptr = self.all.data_ptr() + 8 * GUARD

    def read(self):
        a = self.all.cpu().numpy()
        assert np.all(a[:GUARD] == SENTINEL) and np.all(a[GUARD + self.n:] == SENTINEL), "guard overwritten"
        return a[GUARD:GUARD + self.n].reshape(self.shape).copy()


_host = {}


def host_ref(name, S, f, samples):
    """The host build's guides, computed once per (frame, strata) and shared."""
    key = (name, samples)
    if key not in _host:
        _host[key] = host_guides(S, f, samples=samples)
        _host[key].setflags(write=False)
    return _host[key]


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_device_guides_equal_the_host_build(name):
    S, f = guide_frame(name)
    if name == "cornell_fog":
        assert (f.image_width, f.image_height) == (36, 36)  # ragged tiles: the last column / row 4 pixels
    ref = host_ref(name, S, f, (0, 4))
    with Renderer(S) as R:
        buf = Guarded(f)
        R.render_guides_device(f, buf.ptr, _stream(), seed=SEED, samples=(0, 4), accumulate=0)
        whole = buf.read()
        assert not (whole == SENTINEL).any()  # every pixel of the image written
        if name == "cornell_fog":
            # The fog's albedo is the noise texture and its free-flight distance a
            # logarithm: the device blends a Perlin octave by FMA lerps where the
            # host keeps the reference's products (rt_path.h perlin_noise), and
            # log() is each side's own library -- rounding-level differences, so
            # this frame is compared at 1e-12 relative (hits exactly)
            assert np.array_equal(whole[..., 7], ref[..., 7])
            np.testing.assert_allclose(whole, ref, rtol=1e-12, atol=0)
        else:
            assert np.array_equal(whole, ref), "%d values differ" % (whole != ref).sum()
        # [0,4) in one call = [0,2) then [2,4) accumulated, bit for bit
        buf2 = Guarded(f)
        R.render_guides_device(f, buf2.ptr, _stream(), seed=SEED, samples=(0, 2), accumulate=0)
        R.render_guides_device(f, buf2.ptr, _stream(), seed=SEED, samples=(2, 2), accumulate=1)
        assert np.array_equal(buf2.read(), whole)
        # two runs are identical; accumulate 0 overwrites what was there
        R.render_guides_device(f, buf2.ptr, _stream(), seed=SEED, samples=(0, 4), accumulate=0)
        assert np.array_equal(buf2.read(), whole)
        # a row range writes its rows only, at the buffer's start
        buf3 = Guarded(f)
        R.render_guides_device(f, buf3.ptr, _stream(), seed=SEED, rows=(8, 19), samples=(0, 4), accumulate=0)
        part = buf3.read().reshape(-1)
        n = 11 * f.image_width * CH
        assert np.array_equal(part[:n].reshape(11, f.image_width, CH), whole[8:19])
        assert np.all(part[n:] == SENTINEL)


def test_guide_refusals_leave_the_buffer_untouched():
    S, f = guide_frame("cornell_fog")
    L = load()
    with Renderer(S) as R:
        buf = Guarded(f)
        bad = [dict(output=abi.RT_OUT_SCALED), dict(tiles=(1, 2)), dict(tiles=(0, 2)),
               dict(layout=abi.RT_LAYOUT_TILES), dict(chunks=1), dict(chunks=abi.RT_CHUNKS_AUTO),
               dict(samples=(3, 2)), dict(rows=(0, 37))]
        for kw in bad:
            args = dict(seed=SEED, rows=(0, 0), samples=(0, 4), output=abi.RT_OUT_SUM, accumulate=0, chunks=0)
            args.update(kw)
            p = Renderer.params(**args)
            rc = L.rt_render_guides_device(R.handle, C.byref(f), C.byref(p), C.c_void_p(buf.ptr),
                                           C.c_void_p(_stream()))
            assert rc == abi.RT_ERR_INVALID, kw
            assert L.rt_last_error(), kw
        p = Renderer.params(SEED, samples=(0, 4), output=abi.RT_OUT_SUM, chunks=0)
        assert L.rt_render_guides_device(R.handle, C.byref(f), C.byref(p), None, None) == abi.RT_ERR_INVALID
        torch.cuda.synchronize()
        assert np.all(buf.read() == SENTINEL)


def test_scene_destroyed_right_after_the_guide_launch_leaves_the_whole_frame():
    S, f = guide_frame("bouncing_seed42")
    ref = host_ref("bouncing_seed42", S, f, (0, 4))
    st = torch.cuda.Stream()
    buf = Guarded(f)
    torch.cuda.synchronize()
    R = Renderer(S)
    R.render_guides_device(f, buf.ptr, st.cuda_stream, seed=SEED, samples=(0, 4), accumulate=0)
    R.close()  # waits for the scene's own launch (the launch chain), and only for it
    assert st.query(), "destroy returned before its scene's guide launch finished"
    assert np.array_equal(buf.read(), ref)


@pytest.mark.parametrize("name", ["cornell_fog", "bouncing_seed42"])
def test_guide_launch_does_not_disturb_the_render(name):
    """An rt_render_device frame before and after a guide launch is the same
    bit for bit (dispatch orders, scratch and the unit counter untouched),
    guides on another stream included (the launch chain orders them)."""
    S, f = guide_frame(name)
    H, W = f.image_height, f.image_width
    other = torch.cuda.Stream()
    with Renderer(S) as R:
        def frame():
            out = torch.full((H, W, 3), SENTINEL, dtype=torch.float64, device="cuda")
            R.render_device(f, out.data_ptr(), _stream(), seed=SEED, samples=(0, 4), accumulate=0)
            return out.cpu().numpy()

        before = frame()
        buf = Guarded(f)
        torch.cuda.synchronize()  # the sentinel fill ran on the current stream
        R.render_guides_device(f, buf.ptr, other.cuda_stream, seed=SEED, samples=(0, 4), accumulate=0)
        after = frame()
        other.synchronize()
        assert np.array_equal(before, after, equal_nan=True)
        assert not (buf.read() == SENTINEL).any()
