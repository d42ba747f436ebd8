"""rt_temporal_motion_device / rt_temporal_variance_motion_device on gfx950
against the host twins (tests/native/rt_temporal_motion_emu.cpp) and
rtx.temporal.NumpyOps(motion=); an all-zero motion plane against the parent
kernels bit for bit; TemporalDisplay.edited() and TemporalVarianceDisplay's
against a restart and against the ghost a camera-only reset leaves."""
import os

import numpy as np
import pytest
import torch

from rtx import abi, adaptive, progressive, temporal
from rtx.render import MOTION_DTYPE, Renderer
from rtx.scene import load_scene
from rtx.temporal import HipOps, NumpyOps, TemporalDisplay, TemporalVarianceDisplay
import oracle_lib as O
from test_denoise import H, W
from test_denoise_gpu import GuardedBytes, _cur, _dev
from test_motion import host_temporal_motion, random_motion
from test_motion_gpu import device_motion, device_pose
from test_ray_queries import frame_rays
from test_temporal import START, assert_matches_numpy, moved_random_case
from test_temporal_gpu import _poses, gpu_temporal
from test_temporal_variance import assert_variance_matches_numpy, random_variances
from test_temporal_variance_gpu import gpu_temporal_variance

pytestmark = pytest.mark.gpu

PKG = os.path.join(O.ROOT, "real-time-ray-tracing-engine_amd")
ROOM = 555.0


def gpu_temporal_motion(f, rgb, scale, tile_strata, strata_now, guides, g, f_prev, hist, motion, params=None,
                        v_now=None):
    """HipOps.temporal(motion=) -- with v_now HipOps.temporal_variance(motion=) -- between guards, run twice
    (bit-identical), the motion plane only read -> the host twin's tuple (test_motion.host_temporal_motion)."""
    ops = HipOps(torch.device("cuda", 0), _cur())
    h, w = f.image_height, f.image_width
    var = v_now is not None
    hb = ops.history_variance_bytes(f) if var else ops.history_bytes(f)
    pack, unpack = ((temporal.pack_variance_history, temporal.unpack_variance_history) if var else
                    (temporal.pack_history, temporal.unpack_history))
    ho, ob, vb = GuardedBytes(hb), GuardedBytes(h * w * 24), GuardedBytes(h * w * 8)
    out = ob.mid.view(torch.float64).view(h, w, 3)
    v_out = vb.mid.view(torch.float64).view(h, w)
    d_guides, d_rgb = _dev(guides), _dev(rgb)
    d_strata = _dev(tile_strata, torch.int32) if tile_strata is not None else None
    d_vnow = _dev(v_now) if var else None
    raw = np.ascontiguousarray(motion, dtype=MOTION_DTYPE).view(np.uint8).reshape(-1)
    d_motion = torch.as_tensor(raw).cuda()
    hp = None
    if hist is not None:
        hp = GuardedBytes(hb)
        hp.mid.copy_(torch.as_tensor(pack(f, hist)))
    runs = []
    for _ in range(2):
        ho.mid.fill_(0x5A)
        if var:
            ops.temporal_variance(f, d_rgb, scale, d_strata, strata_now, d_guides, g, d_vnow, f_prev,
                                  hp.mid if hp is not None else None, params, ho.mid, out, v_out, motion=d_motion)
        else:
            ops.temporal(f, d_rgb, scale, d_strata, strata_now, d_guides, g, f_prev,
                         hp.mid if hp is not None else None, params, ho.mid, out, motion=d_motion)
        runs.append((out.cpu().numpy().copy(), ho.mid.cpu().numpy().copy(), v_out.cpu().numpy().copy()))
    assert np.array_equal(d_motion.cpu().numpy(), raw), "the motion plane was written"
    assert np.array_equal(d_rgb.cpu().numpy(), rgb, equal_nan=True) and np.array_equal(d_guides.cpu().numpy(), guides)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(runs[0], runs[1])), "two runs differ"
    assert ho.guards_intact() and ob.guards_intact() and vb.guards_intact(), "guard overwritten"
    if var:
        return runs[0][0], unpack(f, runs[0][1]), runs[0][2]
    assert np.all(vb.mid.cpu().numpy() == 0xA5)  # the plain form writes no variance
    return runs[0][0], unpack(f, runs[0][1])


def same_bits(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def check_three_ways(f, rgb, scale, g, guides, fp, hist, motion, params, what, v_now=None, var=None):
    """The kernel against NumPy and against the twin (test_temporal's / test_temporal_variance's bounds; the
    twin itself is NumPy's bits: tests/test_motion.py)."""
    if v_now is None:
        ref = NumpyOps().temporal(f, rgb, scale, None, g, guides, g, fp, hist, params, motion=motion)
        host = host_temporal_motion(f, rgb, scale, None, g, guides, g, fp, hist, motion, params)
        got = gpu_temporal_motion(f, rgb, scale, None, g, guides, g, fp, hist, motion, params)
        assert_matches_numpy(got, ref, what + " gpu/numpy")
        assert_matches_numpy(got, host + (ref[2],), what + " gpu/twin")
        return got, ref
    hv = hist + (var,)
    ref = NumpyOps().temporal_variance(f, rgb, scale, None, g, guides, g, v_now, fp, hv, params, motion=motion)
    host = host_temporal_motion(f, rgb, scale, None, g, guides, g, fp, hv, motion, params, v_now=v_now)
    got = gpu_temporal_motion(f, rgb, scale, None, g, guides, g, fp, hv, motion, params, v_now=v_now)
    assert_variance_matches_numpy(got, ref, what + " variance gpu/numpy")
    assert_variance_matches_numpy(got, host + (ref[3],), what + " variance gpu/twin")
    return got, ref


def box_and_lamp(S):
    """(the tall box's translate, its new offset: 5 % of the room along x; the lamp quad, its new corner: a step
    of a tenth of its edges)."""
    tr = [k for k, o in enumerate(S.objects) if o.kind == abi.RT_OBJ_TRANSLATE]
    lamp = [k for k, o in enumerate(S.objects) if o.kind == abi.RT_OBJ_QUAD and o.a.y == 554.0 and o.b.x == 130.0]
    assert len(tr) == 1 and len(lamp) == 1
    off = np.array(S.objects[tr[0]].a.tolist()) + np.array([0.05 * ROOM, 0.0, 0.0])
    ob = S.objects[lamp[0]]
    corner = np.array(ob.a.tolist()) + 0.1 * np.array(ob.b.tolist()) + 0.1 * np.array(ob.c.tolist())
    return tr[0], off, lamp[0], corner


def test_kernels_match_the_twins_and_numpy_on_real_guides_and_a_random_plane():
    """Cornell 64 x 64: 4 strata of render and guides at pose A, the tall box and the lamp moved, 4 strata at
    pose B, the motion plane rt_motion_device gives; then the random case under a random plane with NaN and
    infinite entries."""
    S = load_scene(os.path.join(PKG, "scenes", "cornell.json"))
    fA, fB = _poses(S, image_width=64, aspect_ratio=1.0, samples_per_pixel=4, max_depth=8)
    h, w = fA.image_height, fA.image_width
    box, off, lamp, corner = box_and_lamp(S)
    with Renderer(S) as R:
        def frame_data(f):
            rgb = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
            guides = torch.zeros((h, w, abi.RT_GUIDE_CHANNELS), dtype=torch.float64, device="cuda")
            st = _cur().cuda_stream
            R.render_device(f, rgb.data_ptr(), st, seed=9, samples=(0, 4), accumulate=0)
            R.render_guides_device(f, guides.data_ptr(), st, seed=9, samples=(0, 4), accumulate=0)
            return rgb.cpu().numpy(), guides.cpu().numpy()
        rgbA, gA = frame_data(fA)
        pose, _ = device_pose(R)
        R.set_transforms([box], [off])
        R.move_quads([lamp], [corner])
        rgbB, gB = frame_data(fB)
        motion = device_motion(R, fB, pose)
    moved = (np.abs(motion["d"]).sum(-1) > 0)
    assert 0.02 < moved.mean() < 0.5, moved.mean()
    first = NumpyOps().temporal(fA, rgbA, 0.25, None, 4, gA, 4)
    hist = first[1]
    got, ref = check_three_ways(fB, rgbB, 0.25, 4, gB, fA, hist, motion, START, "cornell")
    plain = NumpyOps().temporal(fB, rgbB, 0.25, None, 4, gB, 4, fA, hist, START)
    kept, kept_plain = got[1][0][..., 3] > 4.5, plain[1][0][..., 3] > 4.5
    print("cornell 64x64, box and lamp moved: %.1f %% of the moved pixels keep history with the motion, %.1f %% without"
          % (100 * kept[moved].mean(), 100 * kept_plain[moved].mean()))
    assert kept[moved].mean() >= kept_plain[moved].mean() and kept[moved].any()
    v_now, var = random_variances(h=h, w=w)
    check_three_ways(fB, rgbB, 0.25, 4, gB, fA, hist, motion, START, "cornell", v_now, var)
    # the random case, a random plane
    fA, fB, rgb, scale, guides, g, hist = moved_random_case()
    motion = random_motion(guides, g)
    v_now, var = random_variances()
    for params in (START, None):
        check_three_ways(fB, rgb, scale, g, guides, fA, hist, motion, params, "random")
        check_three_ways(fB, rgb, scale, g, guides, fA, hist, motion, params, "random", v_now, var)


def test_an_all_zero_plane_gives_the_parent_kernels_bits():
    fA, fB, rgb, scale, guides, g, hist = moved_random_case()
    rgb = rgb.copy()
    rgb[25, 40, 1] = np.nan
    v_now, var = random_variances()
    zero = np.zeros((H, W), dtype=MOTION_DTYPE)
    zero["object"] = 3  # hits that nothing moved
    zero["t"] = 1.0
    for params in (START, None):
        got = gpu_temporal_motion(fB, rgb, scale, None, g, guides, g, fA, hist, zero, params)
        want = gpu_temporal(fB, rgb, scale, None, g, guides, g, fA, hist, params)
        assert same_bits((got[0],) + got[1], (want[0],) + want[1])
        hv = hist + (var,)
        got = gpu_temporal_motion(fB, rgb, scale, None, g, guides, g, fA, hv, zero, params, v_now=v_now)
        want = gpu_temporal_variance(fB, rgb, scale, None, g, guides, g, v_now, fA, hv, params)
        assert same_bits((got[0],) + got[1] + (got[2],), (want[0],) + want[1] + (want[2],))


def _rmse(img, ref, mask=None):
    d = (np.clip(img, 0, 1) - np.clip(ref, 0, 1)) ** 2
    return float(np.sqrt(np.mean(d[mask] if mask is not None else d)))


def displays_after_a_move(make_display, make_plain, step64, step4):
    """64 strata, image(), the tall box moved by 5 % of the room, then 4 strata: through edited(), through
    reset() + clear() (a restart) and through reset() alone (the ghost).  The reference is a 1,024-strata
    render of the moved scene with another seed.  Orderings only."""
    S = load_scene(os.path.join(PKG, "scenes", "cornell.json"))
    cam = dict(image_width=64, aspect_ratio=1.0, max_depth=8)
    f, _ = _poses(S, samples_per_pixel=64, **cam)
    fref, _ = _poses(S, samples_per_pixel=1024, **cam)
    box, off, _, _ = box_and_lamp(S)
    rays = frame_rays(f)
    with Renderer(S) as R:
        shows = {k: make_display(R, f) for k in ("edited", "restart", "ghost")}
        for d in shows.values():
            step64(d)
            d.image()
        on_box = R.trace(rays)["chain_object"] == box
        R.set_transforms([box], [off])
        on_box = (on_box | (R.trace(rays)["chain_object"] == box)).reshape(f.image_height, f.image_width)
        untouched = R.render(f, seed=77)
        ref = R.render(fref, seed=1234)
        shows["edited"].edited()
        shows["restart"].reset()
        shows["restart"].clear()
        shows["ghost"].reset()
        assert shows["edited"].has_history and shows["edited"]._moved and not shows["ghost"]._moved
        assert shows["edited"].samples_taken == 0 and shows["edited"].guides_done == 0
        img = {}
        for k, d in shows.items():
            step4(d)
            img[k] = d.image().cpu().numpy().copy()
        plain = make_plain(R, f)
        step4(plain)
        assert np.array_equal(shows["edited"].pr.acc.cpu().numpy(), plain.acc.cpu().numpy(), equal_nan=True), \
            "the wrapped accumulator is not a plain run's"
        e = {k: (_rmse(v, ref), _rmse(v, ref, on_box)) for k, v in img.items()}
        print("cornell 64x64, 64 strata, the box moved, 4 strata: RMSE whole frame / box pixels (%d): edited %.5f / %.5f, "
              "reset + clear %.5f / %.5f, reset alone %.5f / %.5f; edited is %.3f of the restart (frame), %.3f of the "
              "ghost (box)" % (on_box.sum(), *e["edited"], *e["restart"], *e["ghost"], e["edited"][0] / e["restart"][0],
                               e["edited"][1] / e["ghost"][1]))
        assert on_box.sum() > 100
        assert e["edited"][0] < e["restart"][0]
        assert e["edited"][1] < e["ghost"][1]
        # a camera-only reset afterwards commits a history of the scene as it stands: the plain call again
        d = shows["edited"]
        d.reset()
        assert d.has_history and not d._moved
        step4(d)
        d.image()
        # clear() keeps its meaning
        d.clear()
        assert not d.has_history
        assert np.array_equal(R.render(f, seed=77), untouched, equal_nan=True)


def test_temporal_display_keeps_its_history_when_an_object_moves():
    displays_after_a_move(lambda R, f: TemporalDisplay(progressive.for_renderer(R, f, seed=5)),
                          lambda R, f: progressive.for_renderer(R, f, seed=5),
                          lambda d: d.step(64), lambda d: d.step(4))


def test_temporal_variance_display_keeps_its_history_when_an_object_moves():
    def make(R, f):
        return adaptive.for_renderer(R, f, seed=5, threshold=0, batch_strata=4)

    def steps(n):
        def run(d):
            for _ in range(n // 4):
                d.step()
        return run
    displays_after_a_move(lambda R, f: TemporalVarianceDisplay(make(R, f)), make, steps(64), steps(4))
