"""rt_scene_rebuild_bvh / rt_multi_rebuild_bvh through the ABI.

A rebuilt scene IS a fresh one: after a move and a rebuild, the scene info, the
SAH cost and the frame are those of a scene created from the moved description
with the device SAH builder and the same arity and tuning -- equal fields, equal
doubles, bit-identical pixels (same tree, same walk, same tie outcomes).  Where
the new tree cannot be taken the scene stays exactly as it was.  48 x 48, 4 spp,
depth 6, as in tests/test_move_spheres_gpu.py.
"""
import os

import numpy as np
import pytest

from rtx import abi
from rtx.render import MultiRenderer, Renderer
from rtx.scene import load_scene
from test_device_bvh import compare, random_spheres
from test_move_spheres_gpu import SCENES, SEED, a_third, centres_of, frame_of, same_bits, sphere_ids, world_id

pytestmark = pytest.mark.gpu

# spheres, bvh_builder, bvh_arity, the arity the scene must report, tuning
WORLDS = [(300, abi.RT_BVH_HOST, 0, 2, None), (300, abi.RT_BVH_DEVICE, 0, 2, None),
          (300, abi.RT_BVH_DEVICE_SAH, 0, 2, None), (300, abi.RT_BVH_HOST, 4, 4, None),
          (5000, abi.RT_BVH_AUTO, 0, 4, None),
          # leaves of up to four items: the host's tree has fewer nodes than any the device builder makes
          (300, abi.RT_BVH_HOST, 0, 2, dict(sah_leaf_max=4, sah_leaf_split=8))]
GROWS = WORLDS[-1]
TREE_FIELDS = ("n_nodes", "bvh_depth", "stack_depth", "bvh_arity", "features", "lds_nodes", "lds_nodes_persistent",
               "persistent_block_waves", "waves_per_simd", "bvh_builder")


def wid(w):
    return world_id(w) + ("-wide-leaves" if w[4] else "")


def make_world(w, builder=None):
    S = load_scene(random_spheres(w[0], seed=11))
    S.bvh_builder, S.bvh_arity = w[1] if builder is None else builder, w[2]
    return S


def fresh_device_sah(S, w, f):
    """info, cost and frame of a scene created from S as it stands by the device SAH builder."""
    S.bvh_builder = abi.RT_BVH_DEVICE_SAH
    with Renderer(S, tuning=w[4]) as F:
        return F.info(), F.bvh_cost(), F.render(f, seed=SEED)


def assert_same_tree(info, want):
    for k in TREE_FIELDS:
        assert info[k] == want[k], (k, info[k], want[k])


@pytest.mark.parametrize("w", WORLDS, ids=wid)
def test_rebuilt_is_fresh(w):
    S = make_world(w)
    f = frame_of(S)
    ids, new = a_third(S, reach=3.0)
    with Renderer(S, tuning=w[4]) as R:
        created = R.info()
        assert created["bvh_arity"] == w[3] and not created["features"] & abi.RT_FEAT_FLAT, created
        R.move_spheres(ids, new)
        refitted = R.render(f, seed=SEED)
        assert R.rebuild_bvh() is True
        info, cost, frame = R.info(), R.bvh_cost(), R.render(f, seed=SEED)
    want_info, want_cost, want = fresh_device_sah(S, w, f)
    assert want_info["bvh_builder"] == abi.RT_BVH_DEVICE_SAH, "the fresh scene fell back to the host builder"
    assert_same_tree(info, want_info)
    assert cost == want_cost, (cost, want_cost)
    assert same_bits(frame, want)
    compare(frame, refitted, 1e-12)  # and the hits are the refitted tree's
    if w is GROWS:
        assert info["n_nodes"] > created["n_nodes"], (info["n_nodes"], created["n_nodes"])
        assert info["device_bytes"] > created["device_bytes"]  # the new node range is accounted for
    elif w[1] in (abi.RT_BVH_DEVICE, abi.RT_BVH_DEVICE_SAH):
        assert info["device_bytes"] == created["device_bytes"]  # a device-built scene's range fits any rebuild


@pytest.mark.parametrize("w", [WORLDS[2], (5000, abi.RT_BVH_DEVICE_SAH, 0, 4, None)], ids=wid)
def test_rebuilding_an_unmoved_device_sah_scene_changes_nothing(w):
    S = make_world(w)
    f = frame_of(S)
    with Renderer(S) as R:
        info, cost, frame = R.info(), R.bvh_cost(), R.render(f, seed=SEED)
        assert info["bvh_builder"] == abi.RT_BVH_DEVICE_SAH and info["bvh_arity"] == w[3]
        assert R.rebuild_bvh() is True
        assert R.info() == info and R.bvh_cost() == cost
        assert same_bits(R.render(f, seed=SEED), frame)


@pytest.mark.parametrize("w", [WORLDS[0], WORLDS[3], GROWS], ids=wid)
def test_moves_after_a_rebuild_use_the_new_links(w):
    S = make_world(w)
    f = frame_of(S)
    every = sphere_ids(S)
    home = centres_of(S, every)
    ids, away = a_third(S, reach=3.0)
    with Renderer(S, tuning=w[4]) as R:
        original = R.render(f, seed=SEED)
        R.move_spheres(ids, away)
        assert R.rebuild_bvh()
        R.move_spheres(every, home)  # refits the rebuilt tree: needs its parent links
        compare(R.render(f, seed=SEED), original, 1e-12)
        assert R.rebuild_bvh()
        info, cost, frame = R.info(), R.bvh_cost(), R.render(f, seed=SEED)
    want_info, want_cost, want = fresh_device_sah(S, w, f)
    assert np.array_equal(centres_of(S, every), home)
    assert_same_tree(info, want_info)
    assert cost == want_cost and same_bits(frame, want)


def kept(S, f, tuning=None, moved=None):
    """A rebuild that must keep the tree: rebuilt == 0, info and frame as before."""
    with Renderer(S, tuning=tuning) as R:
        if moved is not None:
            R.move_spheres(*moved)
        info, cost, frame = R.info(), R.bvh_cost(), R.render(f, seed=SEED)
        assert R.rebuild_bvh() is False
        assert R.info() == info and R.bvh_cost() == cost
        assert same_bits(R.render(f, seed=SEED), frame)
        return info


def test_a_flat_world_keeps_its_leaf():
    S = load_scene(os.path.join(SCENES, "three_spheres.json"))
    info = kept(S, frame_of(S))
    assert info["features"] & abi.RT_FEAT_FLAT and info["n_nodes"] == 0


def test_a_tree_the_builder_would_make_one_leaf_is_kept():
    """Three items under the linear builder: two nodes; the SAH builder's answer is a root leaf, and
    the scene's instance walks a tree."""
    S = load_scene(os.path.join(SCENES, "three_spheres.json"))
    S.bvh_builder = abi.RT_BVH_DEVICE
    info = kept(S, frame_of(S))
    assert not info["features"] & abi.RT_FEAT_FLAT and info["n_nodes"] == 2


def test_a_tree_deeper_than_the_tuning_allows_is_kept():
    S = make_world(WORLDS[0])
    info = kept(S, frame_of(S), tuning=dict(lbvh_max_depth=3), moved=a_third(S, reach=3.0))
    assert info["bvh_builder"] == abi.RT_BVH_HOST and info["bvh_depth"] > 3


def test_tile_orders_still_apply_after_a_rebuild():
    import torch
    S = make_world(WORLDS[4])
    f = frame_of(S)
    ids, new = a_third(S, reach=3.0)
    tiles = ((f.image_width + 7) // 8) * ((f.image_height + 7) // 8)
    shape = (f.image_height, f.image_width, 3)
    with Renderer(S) as R:
        R.render(f, seed=SEED)  # measures the shape's order on creation's tree
        R.move_spheres(ids, new)
        assert R.rebuild_bvh()
        first = R.render(f, seed=SEED)
        assert same_bits(R.render(f, seed=SEED), first)
        whole = torch.zeros(shape, dtype=torch.float64, device="cuda")
        listed = torch.zeros(shape, dtype=torch.float64, device="cuda")
        every = torch.arange(tiles, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        kw = dict(seed=SEED, samples=(0, 1), output=abi.RT_OUT_SUM, accumulate=0)
        R.render_device(f, whole.data_ptr(), None, **kw)
        R.render_tiles_device(f, every.data_ptr(), tiles, listed.data_ptr(), None, **kw)
        torch.cuda.synchronize()
        assert same_bits(listed.cpu().numpy(), whole.cpu().numpy())


def test_multi_rebuild_equals_one_scene():
    w = WORLDS[0]
    A, M = make_world(w), make_world(w)
    f = frame_of(A)
    ids, new = a_third(A, reach=3.0)
    with Renderer(A) as R:
        R.move_spheres(ids, new)
        assert R.rebuild_bvh()
        one = R.render(f, seed=SEED)
    with MultiRenderer(M, devices=(0,), shards=2) as R:
        R.move_spheres(ids, new)
        refitted = R.render(f, seed=SEED)
        assert R.rebuild_bvh() is True
        multi = R.render(f, seed=SEED)
    assert same_bits(multi, one)
    compare(multi, refitted, 1e-12)
