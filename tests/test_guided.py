"""Guided sampling on the host: the statement of record
(rtx.guided.NumpyOps.select) against explicit per-tile loops, the behaviours it
pins, the ABI's argument checks, AdaptiveRenderer.reselect, and what the rule
is for: after a camera move the tiles whose displayed blend is good enough stop
costing samples.  No GPU: tests/test_guided_gpu.py holds the gfx950 kernel and
GuidedDisplay to all of it."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from rtx import abi, adaptive
from rtx.adaptive import AdaptiveRenderer, tile_grid
from rtx.cpu import CpuRenderer
from rtx.guided import NumpyOps
from rtx.lib import load
from rtx.scene import load_scene
from test_denoise import H, W, frame_of
from test_guides import SCENES, host_guides
from test_temporal import HEADER_DIR
from test_temporal_variance import accumulate, display_chain, poses
from test_variance import rmse

FLOOR, MIN_COUNT = abi.RT_GUIDED_FLOOR, abi.RT_GUIDED_MIN_COUNT
SIZES = ((W, H), (8, 8), (1, 1))  # 70 x 33: the last tile column 6 wide, the last tile row 1 high


# ---- inputs ---------------------------------------------------------------------
def guided_case(w, h, seed=41, bad=True):
    """(frame, col [h, w, 4] float32, v_out [h, w], tile strata): a displayed
    frame's history and variance with per-tile noise levels (distinct tile
    errors), tiles of 0 to 12 strata, stored counts of 0, below and above the
    tiles' strata, and with `bad` (frames of at least 24 x 24) NaN, negative and
    infinite variances and a NaN and an infinite colour."""
    rng = np.random.default_rng(seed)
    f = frame_of(w, h)
    tx, ty = tile_grid(f)
    strata = ((np.arange(tx * ty) * 7) % 13).astype(np.int32)
    level = np.repeat(np.repeat(rng.uniform(0.002, 0.2, (ty, tx)), 8, 0), 8, 1)[:h, :w]
    col = np.empty((h, w, 4), dtype=np.float32)
    col[..., :3] = rng.uniform(0.05, 2.0, (h, w, 3))
    col[..., 3] = rng.choice([0.0, 3.5, 9.25, 40.0, 64.0], size=(h, w), p=[0.05, 0.05, 0.2, 0.4, 0.3])
    v = (level * rng.uniform(0.5, 1.5, (h, w))) ** 2
    if bad and w >= 24 and h >= 24:
        v[3, 5], v[9, 20], v[15, 13] = np.nan, -1.0, np.inf
        col[20, 3, 1], col[21, 17, 2] = np.nan, np.inf
    return f, col, v, strata


def lists_of(f):
    """label -> (list, n_in): the full list, an ascending subset, and nothing."""
    tiles = tile_grid(f)[0] * tile_grid(f)[1]
    full = np.arange(tiles, dtype=np.int32)
    return {"full": (full, tiles), "subset": (np.concatenate([full[::3], full[:1]]).astype(np.int32), len(full[::3])),
            "empty": (full, 0)}


def loops(col, v_out, f, strata, strata_now, threshold, floor, min_count, tiles):
    """The rule, pixel by pixel in plain Python -> (kept, {t: e_t}, {t: c_t})."""
    tx, _ = tile_grid(f)
    kept, err, cnt = [], {}, {}
    for t in tiles:
        t = int(t)
        n_c = float(max(int(strata[t]), 0)) if strata is not None else float(strata_now)
        total, c_t, n_px = 0.0, math.inf, 0
        for j in range((t // tx) * 8, min((t // tx) * 8 + 8, f.image_height)):
            for i in range((t % tx) * 8, min((t % tx) * 8 + 8, f.image_width)):
                r, g, b, stored = (float(x) for x in col[j, i])
                y = 0.2126 * r + 0.7152 * g + 0.0722 * b
                v = float(v_out[j, i])
                v = v if v > 0.0 else 0.0
                q = y + floor
                if q != 0.0:
                    rel = math.sqrt(v) / q if not math.isinf(q) or not math.isinf(v) else math.nan
                else:
                    rel = math.nan if v == 0.0 else math.inf
                if not all(math.isfinite(x) for x in (r, g, b)) or math.isnan(rel):
                    rel = math.inf
                total += rel
                c_t = min(c_t, stored if stored > n_c else n_c)
                n_px += 1
        err[t], cnt[t] = total / n_px, c_t
        if not (c_t >= min_count and err[t] <= threshold):
            kept.append(t)
    return kept, err, cnt


def clear_threshold(errs, counts, min_count=MIN_COUNT):
    """A threshold between two neighbouring tile errors of the tiles the count
    admits, near their median and at least 1e-9 (relative) clear of every one."""
    e = np.sort([errs[t] for t in errs if counts[t] >= min_count and np.isfinite(errs[t])])
    if len(e) < 2:
        return 0.05
    k = len(e) // 2
    thr = 0.5 * (e[k - 1] + e[k])
    assert all(abs(x - thr) > 1e-9 * thr for x in errs.values()), "a tile sits on the threshold"
    return float(thr)


# ---- NumpyOps.select against explicit loops ----------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_numpy_select_against_explicit_loops(size):
    f, col, v, strata = guided_case(*size)
    tiles = tile_grid(f)[0] * tile_grid(f)[1]
    if size == (W, H):
        assert tile_grid(f) == (9, 5) and W - 8 * 8 == 6 and H - 4 * 8 == 1
    _, errs, counts = loops(col, v, f, strata, 0, 0.0, FLOOR, MIN_COUNT, range(tiles))
    thr = clear_threshold(errs, counts)
    for what, (lst, n) in lists_of(f).items():
        for ts, now in ((strata, 0), (None, 9), (None, 2)):
            want, errs, counts = loops(col, v, f, ts, now, thr, FLOOR, MIN_COUNT, lst[:n])
            out = np.full(tiles, -7, dtype=np.int32)
            e, c = np.full(tiles, -1.0), np.full(tiles, -1.0)
            k = NumpyOps().select(col, v, f, ts, now, thr, FLOOR, MIN_COUNT, lst, n, out, e, c)
            assert k == len(want) and out[:k].tolist() == want and np.all(out[k:] == -7), what
            listed = sorted(errs)
            np.testing.assert_allclose(e[listed], [errs[t] for t in listed], rtol=1e-12, atol=0, err_msg=what)
            assert c[listed].tolist() == [counts[t] for t in listed], what
            unlisted = np.setdiff1d(np.arange(tiles), listed)
            assert np.all(e[unlisted] == -1.0) and np.all(c[unlisted] == -1.0), what  # only listed tiles are written
            # no per-tile buffers: the same list
            out2 = np.full(tiles, -7, dtype=np.int32)
            assert NumpyOps().select(col, v, f, ts, now, thr, FLOOR, MIN_COUNT, lst, n, out2) == k
            assert np.array_equal(out2, out), what
    if size == (W, H):  # teeth: the rule both drops and keeps, and the bad pixels are in listed tiles
        want, errs, counts = loops(col, v, f, strata, 0, thr, FLOOR, MIN_COUNT, range(tiles))
        assert 5 < len(want) < tiles - 5
        assert any(np.isinf(x) for x in errs.values())


# ---- pinned behaviours -----------------------------------------------------------------
def flat_case(w=24, h=16, count=64.0, e=0.5, v=1e-6, strata=2):
    """Six whole tiles, every pixel e, `count` stored, variance v: rel = 1e-3 / (e + floor)."""
    f = frame_of(w, h)
    col = np.empty((h, w, 4), dtype=np.float32)
    col[..., :3], col[..., 3] = e, count
    tiles = tile_grid(f)[0] * tile_grid(f)[1]
    return f, col, np.full((h, w), v), np.full(tiles, strata, dtype=np.int32), tiles


def run(f, col, v, strata, thr=0.05, now=0, min_count=MIN_COUNT, lst=None, floor=FLOOR):
    tiles = tile_grid(f)[0] * tile_grid(f)[1]
    lst = np.arange(tiles, dtype=np.int32) if lst is None else np.asarray(lst, dtype=np.int32)
    out, e, c = np.full(tiles, -7, dtype=np.int32), np.full(tiles, -1.0), np.full(tiles, -1.0)
    k = NumpyOps().select(col, v, f, strata, now, thr, floor, min_count, lst, len(lst), out, e, c)
    return out[:k].tolist(), e, c


def test_a_tile_below_min_count_stays_whatever_its_error():
    f, col, v, strata, tiles = flat_case()
    assert run(f, col, v, strata)[0] == []  # 64 strata of history, a tiny error: every tile leaves
    col[9, 17, 3] = 5.0  # one pixel of tile 5 with 5 < 8 strata behind it
    kept, e, c = run(f, col, v, strata, thr=1e9)
    assert kept == [5] and c[5] == 5.0 and e[5] < 0.01
    assert run(f, col, v, strata, thr=1e9, min_count=5)[0] == []  # c_t >= min_count: equality admits
    # an error above the threshold keeps a tile however many samples it holds
    v[0:8, 8:16] = 1.0
    assert run(f, col, v, strata, min_count=5)[0] == [1]


def test_a_stored_count_of_zero_falls_back_to_the_tiles_strata():
    f, col, v, strata, tiles = flat_case()
    col[3, 3, 3] = 0.0  # below hit_min: no count stored; the pixel holds its tile's own 2 strata
    kept, _, c = run(f, col, v, strata)
    assert kept == [0] and c[0] == 2.0
    strata[0] = 8  # ... and with 8 strata of its own the tile may leave
    kept, _, c = run(f, col, v, strata)
    assert kept == [] and c[0] == 8.0
    # without tile strata strata_now stands in
    assert run(f, col, v, None, now=7)[0] == [0] and run(f, col, v, None, now=8)[0] == []
    # a negative tile count is 0 strata, a NaN stored count the tile's strata
    strata[0] = -3
    col[3, 3, 3] = np.nan
    kept, _, c = run(f, col, v, strata)
    assert kept == [0] and c[0] == 0.0


def test_nan_and_negative_variances_count_as_zero():
    f, col, v, strata, tiles = flat_case(v=1.0)
    assert run(f, col, v, strata)[0] == list(range(tiles))  # rel = 1 / 0.51
    v[:8, :8] = np.nan
    v[:8, 8:16] = -4.0
    kept, e, _ = run(f, col, v, strata)
    assert kept == [2, 3, 4, 5] and e[0] == 0.0 and e[1] == 0.0
    v[8:, :8] = np.inf  # an infinite variance is an infinite error
    assert np.isinf(run(f, col, v, strata, thr=1e300)[1][3])


def test_a_non_finite_e_keeps_the_tile():
    for bad in (np.nan, np.inf, -np.inf):
        f, col, v, strata, tiles = flat_case()
        col[12, 20, 1] = bad
        kept, e, _ = run(f, col, v, strata, thr=1e300)
        assert kept == [5] and e[5] == np.inf, bad
    # +inf and -inf in one tile: a NaN error, and the tile stays
    f, col, v, strata, tiles = flat_case()
    col[0, 0, :3] = -10.0  # y + floor < 0 ...
    v[0, 0] = np.inf       # ... under an infinite variance: rel = -inf
    col[0, 1, 0] = np.nan  # rel = +inf
    kept, e, _ = run(f, col, v, strata, thr=1e300)
    assert kept == [0] and np.isnan(e[0])
    # y + floor = 0 under v = 0: the quotient is NaN, the error +inf
    f, col, v, strata, tiles = flat_case(v=0.0)
    col[0, 0, :3] = -1.0
    kept, e, _ = run(f, col, v, strata, thr=1e300, floor=1.0)
    assert kept == [0] and e[0] == np.inf


def test_order_is_preserved_and_entries_are_clamped():
    f, col, v, strata, tiles = flat_case()
    v[:, :] = 1.0  # every tile stays
    assert run(f, col, v, strata, lst=[1, 3, 4])[0] == [1, 3, 4]
    kept, e, c = run(f, col, v, strata, lst=[-5, 2, tiles + 9])
    assert kept == [0, 2, tiles - 1]
    assert np.all(e[[1, 3, 4]] == -1.0) and np.all(c[[1, 3, 4]] == -1.0)


def test_numpy_refusals():
    f, col, v, strata, tiles = flat_case()
    nan = float("nan")
    for kw in (dict(thr=nan), dict(floor=nan), dict(min_count=nan), dict(floor=0.0), dict(floor=-1.0)):
        with pytest.raises(ValueError):
            run(f, col, v, strata, **kw)
    with pytest.raises(ValueError):
        run(f, col, v, None, now=-1)
    with pytest.raises(ValueError):
        run(f, col, v[:-1], strata)
    with pytest.raises(ValueError):
        NumpyOps().select(col, v, f, strata, 0, 0.1, FLOOR, 8, np.zeros(tiles + 1, np.int32), tiles + 1,
                          np.zeros(tiles + 1, np.int32))


# ---- ABI (no device call is reached) -------------------------------------------------------
def test_refusals_before_any_device_call():
    L = load()
    f = frame_of(36, 36)  # 25 tiles
    # addresses that are never dereferenced: every call below is refused on its arguments
    hist, var, strata, tin, tout, cnt = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000
    NONE = object()
    nan = float("nan")

    def call(frame=f, hist=hist, var=var, now=4, thr=0.2, floor=FLOOR, mc=8.0, tin=tin, n=25, tout=tout, cnt=cnt):
        return L.rt_guided_select_device(
            C.byref(frame) if frame is not NONE else None, C.c_void_p(hist), C.c_void_p(var), C.c_void_p(strata), now,
            thr, floor, mc, C.c_void_p(tin), n, C.c_void_p(tout), C.c_void_p(cnt), None, None, None)

    cases = {
        "null frame": (dict(frame=NONE), b"frame"),
        "empty frame": (dict(frame=frame_of(36, 0)), b"frame"),
        "null history": (dict(hist=0), b"null"),
        "null variance": (dict(var=0), b"null"),
        "null tiles_out": (dict(tout=0), b"null"),
        "null count": (dict(cnt=0), b"null"),
        "null tiles_in": (dict(tin=0), b"null tile list"),
        "n_in -1": (dict(n=-1), b"n_in"),
        "n_in above the tile count": (dict(n=26), b"n_in"),
        "misaligned history": (dict(hist=hist + 128), b"aligned"),
        "history aligned to 16 only": (dict(hist=hist + 16), b"aligned"),
        "tiles_out is tiles_in": (dict(tout=tin), b"alias"),
        "NaN threshold": (dict(thr=nan), b"NaN"),
        "NaN floor": (dict(floor=nan), b"NaN"),
        "NaN min_count": (dict(mc=nan), b"NaN"),
        "floor 0": (dict(floor=0.0), b"floor"),
        "floor -1": (dict(floor=-1.0), b"floor"),
        "strata_now -1": (dict(now=-1), b"strata_now"),
    }
    for what, (kw, word) in cases.items():
        assert call(**kw) == abi.RT_ERR_INVALID, what
        assert word in L.rt_last_error(), (what, L.rt_last_error())


def test_a_c_program_sees_the_prototype_and_the_defaults(tmp_path):
    """The header declares the function with the argument list rtx/lib.py
    binds, below everything else, under ABI 5; the library exports it; the
    RT_GUIDED_* defaults are the ones rtx/abi.py restates."""
    src = tmp_path / "proto.c"
    src.write_text("\n".join([
        '#include <stdio.h>',
        '#include "rt_api.h"',
        "int (*a)(const rt_frame *, const void *, const double *, const int32_t *, int32_t, double, double, double,",
        "         const int32_t *, int32_t, int32_t *, int32_t *, double *, double *, void *)",
        "    = rt_guided_select_device;",
        'int main(void) { printf("%.17g %.17g %d\\n", (double)RT_GUIDED_FLOOR, (double)RT_GUIDED_MIN_COUNT,',
        "                        RT_ABI_VERSION); return a ? 0 : 1; }"]))
    exe = tmp_path / "proto"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", "-I", HEADER_DIR, str(src), "-o",
                    str(tmp_path / "proto.o")], check=True, capture_output=True)
    L = load()
    subprocess.run(["gcc", str(tmp_path / "proto.o"), "-o", str(exe), "-L", os.path.dirname(L._name), "-lrtx_hip",
                    "-Wl,-rpath," + os.path.dirname(L._name)], check=True, capture_output=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [float(x) for x in got] == [abi.RT_GUIDED_FLOOR, float(abi.RT_GUIDED_MIN_COUNT), 5.0]
    assert (abi.RT_GUIDED_FLOOR, abi.RT_GUIDED_MIN_COUNT, abi.RT_ABI_VERSION) == (1e-2, 8, 5)
    assert "rt_guided_select_device" in abi.EXPORTS and len(L.rt_guided_select_device.argtypes) == 15
    header = open(os.path.join(HEADER_DIR, "rt_api.h")).read()
    where = {name: header.index("%s(" % name) for name in abi.EXPORTS}  # "name(": the declaration, not the prose
    assert max(where, key=where.get) == "rt_guided_select_device", "declared below everything else"


# ---- AdaptiveRenderer.reselect -----------------------------------------------------------
def test_reselect_swaps_the_lists_and_leaves_step_alone():
    f = frame_of(20, 20)  # 3 x 3 tiles
    f.sqrt_spp = 4
    calls = []

    def render_tiles_fn(frame, out, seed, rng, tiles, n, accumulate):
        calls.append(np.array(tiles[:n]))
        out[...] = 0.0

    ar = AdaptiveRenderer(render_tiles_fn, adaptive.NumpyOps(), f, threshold=0.0)
    ar.step()
    assert calls[-1].tolist() == list(range(9))
    seen = []

    def every_second(tiles_in, n_in, tiles_out):
        seen.append((np.array(tiles_in[:n_in]), tiles_out))
        keep = tiles_in[:n_in][::2]
        tiles_out[:len(keep)] = keep
        return len(keep)

    before = ar._lists[ar._cur]
    assert ar.reselect(every_second) == 5 and ar.n_active == 5
    assert seen[0][0].tolist() == list(range(9)) and seen[0][1] is ar._lists[ar._cur] and seen[0][1] is not before
    assert ar.active_tiles.tolist() == [0, 2, 4, 6, 8]
    assert ar.step() == 1 and calls[-1].tolist() == [0, 2, 4, 6, 8]  # the next batch traces the kept list
    assert ar.tile_strata.tolist() == [2, 1, 2, 1, 2, 1, 2, 1, 2]
    assert ar.reselect(every_second) == 3 and ar.active_tiles.tolist() == [0, 4, 8]
    assert ar.reselect(lambda a, n, b: 0) == 0 and ar.done and ar.step() == 0
    ar.reset()
    assert ar.n_active == 9 and ar.active_tiles.tolist() == list(range(9))


# ---- end to end on the host ---------------------------------------------------------------
THRESHOLD, BATCHES_B, BS_B = 0.2, 8, 2
_scenes = {}


def host_scene(name):
    """(scene, render(f, first, count, seed), pose B's frame, the 1,024-strata
    reference at B of seed 1234, pose A's frame, pose A's displayed variance
    history: 64 strata in 8 batches of 8, seed 5), 64 x 64, depth 8, once per scene."""
    if name not in _scenes:
        S = load_scene(os.path.join(SCENES, name + ".json"))
        cam = dict(image_width=64, aspect_ratio=1.0, max_depth=8)
        fA, _ = poses(S, samples_per_pixel=64, **cam)
        _, fB = poses(S, samples_per_pixel=16, **cam)
        _, fBref = poses(S, samples_per_pixel=1024, **cam)
        R = CpuRenderer(S)

        def render(f, first, count, seed=5):
            out = torch.zeros((f.image_height, f.image_width, 3), dtype=torch.float64)
            R.render_device(f, out.data_ptr(), seed=seed, samples=(first, count), output=abi.RT_OUT_SUM)
            return out.numpy()

        ref = render(fBref, 0, 1024, seed=1234) / 1024.0
        stateA = accumulate(render, fA, 8, 8)
        _, _, histA, _ = display_chain(fA, stateA, host_guides(S, fA, samples=(0, 16), seed=5), 16, 8)
        assert (histA[0][..., 3] == 64).mean() > 0.5
        _scenes[name] = (S, render, fB, ref, fA, histA)
    return _scenes[name]


def host_run(name, guide):
    """8 batches of 2 at pose B of an AdaptiveRenderer (threshold 0) on
    adaptive.NumpyOps whose tile-list render is the CPU backend's, displayed
    after every batch as TemporalVarianceDisplay displays it
    (test_temporal_variance.display_chain); with `guide` NumpyOps.select runs
    on each batch's blend and AdaptiveRenderer.reselect takes the kept list,
    as GuidedDisplay does on the device.  -> dict(active = tiles active after
    each batch, strata = tile-strata traced, rmse = the last displayed
    frame's, low_kept = every tile with a pixel of count_p < 8 was active
    after every selection)."""
    S, render, fB, ref, fA, histA = host_scene(name)

    def render_tiles_fn(frame, out, seed, rng, tiles, n, accumulate):
        img = render(frame, rng[0], rng[1], seed)  # keyed by (seed, pixel, stratum): the frame masked is the tile list
        for t in tiles[:n]:
            box = adaptive._tile_box(frame, int(t))
            out[box] = out[box] + img[box] if accumulate else img[box]

    ar = AdaptiveRenderer(render_tiles_fn, adaptive.NumpyOps(), fB, seed=5, threshold=0.0, batch_strata=BS_B)
    assert ar.n_tiles == 64 and ar.total_strata == BATCHES_B * BS_B
    tx = tile_grid(fB)[0]
    guides, res = None, dict(active=[], low_kept=True)
    for k in range(BATCHES_B):
        assert ar.step() == BS_B
        guides = host_guides(S, fB, samples=(k * BS_B, BS_B), seed=5, into=guides)
        img, _, hist, v_out = display_chain(fB, (ar.acc, ar.s1, ar.s2, ar.tile_strata), guides, (k + 1) * BS_B, BS_B,
                                            fA, histA)
        if guide and ar.n_active:
            ar.reselect(lambda tin, n, tout: NumpyOps().select(hist[0], v_out, fB, ar.tile_strata, 0, THRESHOLD, FLOOR,
                                                               MIN_COUNT, tin, n, tout))
            _, count = NumpyOps().pixel_terms(hist[0], v_out, fB, ar.tile_strata, 0, FLOOR)
            jj, ii = np.nonzero(count < MIN_COUNT)
            low = np.unique((jj // 8) * tx + ii // 8)
            res["low_kept"] &= bool(np.isin(low, ar.active_tiles).all())
        res["active"].append(ar.n_active)
    res["strata"] = int(ar.tile_strata.sum())
    res["rmse"] = rmse(img, ref)
    return res


@pytest.mark.parametrize("name", ["cornell", "cornell_fog"])
def test_guiding_spends_fewer_samples_for_the_same_display_after_a_camera_move(name):
    """Cornell and Cornell with fog, 64 x 64, depth 8, seed 5, all on the host:
    64 strata at pose A in 8 batches of 8, the move, 8 batches of 2 at pose B
    (frame: samples_per_pixel 16; the wrapped renderer's own rule at threshold
    0), threshold 0.2, min_count 8, floor 1e-2, against 1,024 strata at B of
    seed 1234.  Measured (active tiles of 64 after each batch; tile-strata
    traced, of the baseline's 1,024; displayed RMSE guided / baseline):
    Cornell           59, 57, 57, 41, 40, 40, 38, 37;  792 (0.773x);  0.02763 / 0.02751 (1.0043x)
    Cornell with fog  43, 42, 42, 26, 26, 25, 25, 24;  586 (0.572x);  0.02747 / 0.02698 (1.0183x)
    The baseline keeps all 64 tiles through every batch."""
    guided_run, plain = host_run(name, True), host_run(name, False)
    print("\n%s: active tiles after each batch %r (baseline %r)" % (name, guided_run["active"], plain["active"]))
    print("%s: tile-strata traced %d (baseline %d: %.3fx), displayed RMSE %.5f (baseline %.5f: %.4fx)"
          % (name, guided_run["strata"], plain["strata"], guided_run["strata"] / plain["strata"], guided_run["rmse"],
             plain["rmse"], guided_run["rmse"] / plain["rmse"]))
    assert plain["active"][:BATCHES_B - 1] == [64] * (BATCHES_B - 1) and plain["strata"] == 64 * BATCHES_B * BS_B
    assert guided_run["active"][0] < 64                       # 1: tiles leave after the first batch
    assert guided_run["low_kept"]                             # 2: a tile with a pixel of count_p < 8 stays
    assert guided_run["strata"] <= 0.9 * plain["strata"]      # 3
    assert guided_run["rmse"] <= 1.02 * plain["rmse"]         # 4
    assert all(a >= b for a, b in zip(guided_run["active"], guided_run["active"][1:]))  # none comes back
