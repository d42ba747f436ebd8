"""The albedo as a Lambertian hit's weight (rt_path.h RT_LAMBERT_ALBEDO_F), GPU half.

tests/test_lambert_albedo.py holds the worlds and their host checks; the same
worlds run here through the library:

 * exact accounting: worlds of 1, 3 and 7 spheres whose samples are integers
   (power-of-two albedos and background, depth 8), 24x16 and 20x12, 16 strata,
   RT_OUT_SUM, through the frame launch, RT_LAYOUT_TILES in 2 chunks and the
   twin with an unused metal material (the general flat instance).  Every
   frame equals round(oracle) bit for bit: the host emulator is exact for these
   seeds and worlds, that is, every event passes the guard;
 * both forms in one wave: four pebbles of radius 0.01 at distance 20 beside
   the near sphere's edge, alone, with a zero-radius sphere and with a
   zero-area quad: the oracle at 1e-4 with equal NaN masks, the twin bit for
   bit, equal STATS counters; with power-of-two albedos the pebbles' tile holds
   non-integer sums (the general form ran) beside integer ones;
 * tight parity: spheres(3) at 24x16 and 1, 4 and 16 strata within 1e-12 of the
   oracle.
"""
import functools

import numpy as np
import pytest

from rtx import abi
from rtx.render import Renderer
from rtx.scene import load_scene
import oracle_lib as O
from test_flat_table import spheres
from test_lambert_albedo import (SEED, SIZES, exact_reference, exact_world, frame_of, pebble_frame,
                                 pebble_world, with_unused_metal)

FLAT, DIFFUSE = abi.RT_FEAT_FLAT, abi.RT_FEAT_DIFFUSE


def untile(tiles, w, h):
    """[tiles, chunks, 64, 3] partial sums -> the frame, chunks added in order."""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    out = np.zeros((ty * 8, tx * 8, 3))
    for c in range(tiles.shape[1]):
        out += tiles[:, c].reshape(ty, tx, 8, 8, 3).transpose(0, 2, 1, 3, 4).reshape(ty * 8, tx * 8, 3)
    return out[:h, :w]


@pytest.mark.gpu
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("n", [1, 3, 7])
def test_exact_accounting(n, size):
    want = exact_reference(n, size)
    w, h = SIZES[size]
    for twin in (False, True):
        S = load_scene(exact_world(n))
        if twin:
            S = with_unused_metal(S)
        _, f = frame_of(S, size, 16)
        with Renderer(S) as R:
            assert R.info()["features"] == (FLAT if twin else FLAT | DIFFUSE)
            frame = R.render(f, seed=SEED, output=abi.RT_OUT_SUM)
            tiles = R.render(f, seed=SEED, output=abi.RT_OUT_SUM, layout=abi.RT_LAYOUT_TILES, chunks=2)
        for name, got in (("frame", frame), ("tiles", untile(tiles, w, h))):
            off = got != want
            print("%s%s: %d of %d sums differ from round(oracle), max |diff| %g"
                  % (name, " (twin)" if twin else "", off.sum(), off.size, np.abs(got - want).max()))
        assert np.array_equal(frame, want)
        assert np.array_equal(untile(tiles, w, h), want)


@functools.lru_cache(maxsize=None)
def _pebbles(extra):
    """Per scene of the pair (the world, its unused-metal twin): frame, STATS counters."""
    out = []
    for twin, want in ((False, FLAT | DIFFUSE), (True, FLAT)):
        S = load_scene(pebble_world(extra))
        if twin:
            S = with_unused_metal(S)
        cam, f = pebble_frame(S)
        with Renderer(S) as R:
            assert R.info()["features"] == want
            out.append((R.render(f, seed=SEED), R.stats(f, seed=SEED)))
    return S, cam, out


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [None, "sphere0", "quad0"])
def test_pebble_world_both_forms(extra):
    S, cam, ((a, sa), (b, sb)) = _pebbles(extra)
    ref = O.oracle_render(S, cam, O.MODE_COUNTER, SEED)
    d = np.abs(np.nan_to_num(a) - np.nan_to_num(ref))
    print("max |gpu - oracle| = %.3g" % d.max())
    assert d.max() <= 1e-4 and np.array_equal(np.isnan(a), np.isnan(ref))
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(np.isnan(a), np.isnan(b))
    sa, sb = ({k: v for k, v in s.items() if not k.startswith("cyc_")} for s in (sa, sb))
    assert sa["samples"] == 32 * 24 * 16 and sa["shade_events"] > 0
    assert sa == sb


@pytest.mark.gpu
def test_pebble_world_runs_both_forms():
    S = load_scene(pebble_world(exact=True))
    _, f = pebble_frame(S)
    with Renderer(S) as R:
        assert R.info()["features"] == FLAT | DIFFUSE
        got = R.render(f, seed=SEED, output=abi.RT_OUT_SUM)
    frac = got != np.round(got)
    cols = sorted(set(int(c) for c in np.nonzero(frac)[1]))
    print("non-integer sums: %d, in columns %s" % (frac.sum(), cols))
    assert np.isfinite(got).all() and frac.any()
    assert cols and min(cols) >= 12 and max(cols) <= 15  # the pebbles' tile; the near sphere's sums are integers
    assert not frac[8:16, 8:12].any() and (got[8:16, 8:12] > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 4, 16])
def test_tight_parity(spp):
    S = load_scene(spheres(3))
    cam, f = frame_of(S, "24x16", spp)
    with Renderer(S) as R:
        assert R.info()["features"] == FLAT | DIFFUSE
        got = R.render(f, seed=SEED)
    ref = O.oracle_render(S, cam, O.MODE_COUNTER, SEED)
    d = np.abs(got - ref)
    print("gpu vs oracle, %d strata: max |diff| = %.3g" % (spp, d.max()))
    assert np.isfinite(got).all() and d.max() <= 1e-12
