"""rt_scene_move_quads / _device / rt_multi_move_quads through the ABI.

A scene with moved quads has to render what a Renderer freshly made from the
edited description renders, to tests/test_device_bvh.py's figure for "same
hits, another tree" (same NaN pattern, atol 1e-12), no pixel excluded; a move
that changes nothing leaves the frame bit-identical.  48 pixels wide, 4 spp,
depth 6; the scenes are tests/test_live_edits.py's.
"""
import numpy as np
import pytest

from rtx import abi
from rtx.lib import RtError
from rtx.render import MultiRenderer, Renderer, describe_quads
from rtx.scene import load_scene
from test_device_bvh import compare
from test_move_spheres_gpu import SEED, frame_of, fresh, same_bits
from test_rebuild_gpu import assert_same_tree
import test_live_edits as E

pytestmark = pytest.mark.gpu


def wall(S):
    return E.find(S, abi.RT_OBJ_QUAD, a=(0, 0, 555), b=(555, 0, 0))  # room()'s back wall


def lamp_pair(S):
    """The ceiling panel: the world's quad and the lights list's, two objects."""
    world = [i for i, o in enumerate(S.objects)
             if o.kind == abi.RT_OBJ_QUAD and o.a.tolist() == [343.0, 554.0, 332.0] and o.material >= 0]
    light = E.find(S, abi.RT_OBJ_QUAD, a=(343, 554, 332), material=-1)
    assert len(world) == 1
    return world[0], light


def box_face(S):
    """A face of the first placed box: an axis-aligned quad under a translate and a rotation."""
    rot = E.find(S, abi.RT_OBJ_ROTATE_Y, s=15.0)
    faces = S.objects[S.objects[rot].child]
    assert faces.kind == abi.RT_OBJ_LIST and faces.count == 6
    return S.children[faces.child + 2]


def moved_against_fresh(S, move, expect=None):
    f = frame_of(S)
    with Renderer(S) as R:
        if expect:
            expect(R.info())
        before = R.render(f, seed=SEED)
        R.move_quads(list(move), list(move.values()))
        after = R.render(f, seed=SEED)
    assert not same_bits(before, after), "the move changed no pixel: the test would see nothing"
    compare(after, fresh(S, f), 1e-12)
    for i, c in move.items():
        assert S.objects[i].a.tolist() == [float(x) for x in c]  # the description followed


# ---------------------------------------------------------------- moved against fresh
@pytest.mark.parametrize("builder,arity", [(abi.RT_BVH_HOST, 0), (abi.RT_BVH_DEVICE_SAH, 0), (abi.RT_BVH_HOST, 4)])
def test_a_wall_moves(builder, arity):
    S = load_scene(E.two_boxes())
    S.bvh_builder, S.bvh_arity = builder, arity

    def expect(info):
        assert info["n_nodes"] > 0 and info["bvh_arity"] == (arity or 2) and info["bvh_builder"] == builder, info

    moved_against_fresh(S, {wall(S): [0.0, 0.0, 470.5]}, expect)


def test_the_lamp_pair_moves():
    S = load_scene(E.two_boxes())
    world, light = lamp_pair(S)
    to = [300.0, 540.0, 420.0]
    moved_against_fresh(S, {world: to, light: to}, lambda info: info["n_light_leaves"] >= 1 or pytest.fail("no light"))


def test_an_axis_aligned_quad_under_a_chain_moves():
    S = load_scene(E.two_boxes())
    face = box_face(S)
    with E.Compiled(S) as T:
        assert T.table("quads")["aa"][T.table("quad_of")[face]] >= 0
    o = S.objects[face].a
    moved_against_fresh(S, {face: [o.x + 40.0, o.y + 25.0, o.z - 30.0]})


def test_a_skew_quad_moves():
    S = load_scene(E.skew_quad())
    q = E.find(S, abi.RT_OBJ_QUAD, a=(150, 60, 250))
    with E.Compiled(S) as T:
        assert T.table("quads")["aa"][T.table("quad_of")[q]] < 0
    moved_against_fresh(S, {q: [210.25, 90.5, 130.0]})


def test_a_quad_of_a_flat_world_moves():
    S = load_scene(E.room([]))
    moved_against_fresh(S, {wall(S): [0.0, 0.0, 430.0]},
                        lambda info: info["features"] & abi.RT_FEAT_FLAT or pytest.fail("not flat"))


# ---------------------------------------------------------------- round trips
@pytest.mark.parametrize("builder,arity", [(abi.RT_BVH_HOST, 0), (abi.RT_BVH_DEVICE_SAH, 0), (abi.RT_BVH_HOST, 4)])
def test_round_trips_leave_the_frame_bit_identical(builder, arity):
    S = load_scene(E.two_boxes())
    S.bvh_builder, S.bvh_arity = builder, arity
    f = frame_of(S)
    with E.Compiled(S) as T:
        movable = [int(i) for i in np.flatnonzero(T.table("quad_of") >= 0)]
    assert len(movable) == 6 + 12 + 1  # the room, two boxes, the light-only panel
    home = [S.objects[i].a.tolist() for i in movable]
    world, light = lamp_pair(S)
    some = {wall(S): [0.0, 0.0, 470.5], world: [300.0, 540.0, 420.0], light: [300.0, 540.0, 420.0]}
    back = [S.objects[i].a.tolist() for i in some]
    with Renderer(S) as R:
        before = R.render(f, seed=SEED)
        R.move_quads(movable, home)
        assert same_bits(R.render(f, seed=SEED), before)
        R.move_quads(list(some), list(some.values()))
        assert not same_bits(R.render(f, seed=SEED), before)
        R.move_quads(list(some), back)
        assert same_bits(R.render(f, seed=SEED), before)
        R.move_quads([], np.zeros((0, 3)))  # n = 0: a no-op
        assert same_bits(R.render(f, seed=SEED), before)


# ---------------------------------------------------------------- device arrays, ordering, multi
def some_moves(S):
    world, light = lamp_pair(S)
    return {wall(S): [0.0, 0.0, 470.5], world: [300.0, 540.0, 420.0], light: [300.0, 540.0, 420.0]}


def test_device_array_variant_equals_the_host_variant():
    import torch
    A, D = load_scene(E.two_boxes()), load_scene(E.two_boxes())
    f = frame_of(A)
    move = some_moves(A)
    with Renderer(A) as R:
        R.move_quads(list(move), list(move.values()))
        host = R.render(f, seed=SEED)
    side = torch.cuda.Stream()
    d_ids = torch.tensor(list(move), dtype=torch.int32, device="cuda")
    d_val = torch.tensor(list(move.values()), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with Renderer(D) as R:
        R.move_quads_device(d_ids.data_ptr(), d_val.data_ptr(), len(move), side.cuda_stream)
        dev = R.render(f, seed=SEED)  # on the scene's own stream: ordered after the move by the launch chain
        side.synchronize()
    assert same_bits(dev, host)


def test_device_variant_skips_what_the_host_variant_refuses():
    import torch
    A, who = E.refusal_scene()
    D, _ = E.refusal_scene()
    f = frame_of(A)
    n, p, nan, inf = len(A.objects), [1.0, 2.0, 3.0], float("nan"), float("inf")
    good = some_moves(A)
    with Renderer(A) as R:
        unmoved = R.render(f, seed=SEED)
        R.move_quads(list(good), list(good.values()))
        want = R.render(f, seed=SEED)
    assert not same_bits(want, unmoved)
    floor, left, right = (E.find(A, abi.RT_OBJ_QUAD, a=(0, 0, 0), b=(555, 0, 0)), E.find(A, abi.RT_OBJ_QUAD, a=(0, 0, 0), b=(0, 555, 0)),
                          E.find(A, abi.RT_OBJ_QUAD, a=(555, 0, 0)))
    g = list(good.items())
    entries = [(-1, p), g[0], (n, p), (who["translate"], p), (who["sphere"], p), (floor, p), (who["idle_quad"], p), g[1],
               (who["fog_face"], p), (who["world"], p), (left, [nan, 0.0, 0.0]), (right, [0.0, -inf, 0.0]), (floor, [5.0, 5.0, 5.0]),
               g[2], (who["medium"], p)]
    d_ids = torch.tensor([e[0] for e in entries], dtype=torch.int32, device="cuda")
    d_val = torch.tensor([e[1] for e in entries], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with Renderer(D) as R:
        R.move_quads_device(d_ids.data_ptr(), d_val.data_ptr(), len(entries))
        got = R.render(f, seed=SEED)
        torch.cuda.synchronize()
    assert same_bits(got, want)


def test_a_move_waits_for_the_render_before_it():
    import torch
    S = load_scene(E.two_boxes())
    f = frame_of(S, samples_per_pixel=64)
    move = some_moves(S)
    shape = (f.image_height, f.image_width, 3)
    first, racing, after = (torch.full(shape, -1.0, dtype=torch.float64, device="cuda") for _ in range(3))
    d_ids = torch.tensor(list(move), dtype=torch.int32, device="cuda")
    d_val = torch.tensor(list(move.values()), dtype=torch.float64, device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with Renderer(S) as R:
        kw = dict(seed=SEED, output=abi.RT_OUT_SCALED, accumulate=0)
        R.render_device(f, first.data_ptr(), s1.cuda_stream, **kw)
        s1.synchronize()
        R.render_device(f, racing.data_ptr(), s1.cuda_stream, **kw)
        R.move_quads_device(d_ids.data_ptr(), d_val.data_ptr(), len(move), s2.cuda_stream)
        R.render_device(f, after.data_ptr(), s1.cuda_stream, **kw)
        s1.synchronize()
        s2.synchronize()
        first, racing, after = first.cpu().numpy(), racing.cpu().numpy(), after.cpu().numpy()
    assert same_bits(racing, first)
    assert not same_bits(after, first)
    S2 = load_scene(E.two_boxes())
    describe_quads(S2, list(move), list(move.values()))
    compare(after, fresh(S2, f), 1e-12)


def test_multi_move_quads_equals_one_device():
    A, M = load_scene(E.two_boxes()), load_scene(E.two_boxes())
    f = frame_of(A)
    move = some_moves(A)
    with Renderer(A) as R:
        R.move_quads(list(move), list(move.values()))
        one = R.render(f, seed=SEED)
    with MultiRenderer(M, devices=(0,), shards=3) as R:
        unmoved = R.render(f, seed=SEED)
        R.move_quads(list(move), list(move.values()))
        multi = R.render(f, seed=SEED)
    assert same_bits(multi, one) and not same_bits(unmoved, one)
    assert [o.a.tolist() for o in M.objects] == [o.a.tolist() for o in A.objects]


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_scene_untouched():
    S, who = E.refusal_scene()
    f = frame_of(S)
    cases = [c for c in E.refusals(S, who) if c[0] == "move_quads"]
    assert len(cases) >= 9 and any(c[4] == abi.RT_ERR_UNSUPPORTED for c in cases)
    was = [o.a.tolist() for o in S.objects]
    with Renderer(S) as R:
        before = R.render(f, seed=SEED)
        for _, what, ids, corners, code in cases:
            with pytest.raises(RtError) as e:
                R.move_quads(ids, corners)
            assert e.value.code == code, what
            assert len(str(e.value)) > len("rt error %d: " % code), what
            assert same_bits(R.render(f, seed=SEED), before), what
        assert was == [o.a.tolist() for o in S.objects]
        R.move_quads([who["wall"]], [[0.0, 0.0, 480.0]])  # and the scene still moves
        assert not same_bits(R.render(f, seed=SEED), before)


def test_a_corner_whose_plane_constant_overflows_is_refused():
    S = load_scene(E.skew_quad())
    q = E.find(S, abi.RT_OBJ_QUAD, a=(150, 60, 250))
    with E.Compiled(S) as T:
        n = T.table("quads")["n"][T.table("quad_of")[q]]
    big = (np.sign(n) * 1.7e308).tolist()
    f = frame_of(S)
    with Renderer(S) as R:
        before = R.render(f, seed=SEED)
        with pytest.raises(RtError) as e:
            R.move_quads([q], [big])
        assert e.value.code == abi.RT_ERR_INVALID and "plane constant" in str(e.value)
        assert same_bits(R.render(f, seed=SEED), before)
    assert S.objects[q].a.tolist() == [150.0, 60.0, 250.0]


# ---------------------------------------------------------------- rebuild
def test_a_rebuild_after_a_move_is_a_fresh_device_sah_scene():
    S = load_scene(E.two_boxes())
    S.bvh_builder = abi.RT_BVH_HOST
    f = frame_of(S)
    move = some_moves(S)
    with Renderer(S) as R:
        R.move_quads(list(move), list(move.values()))
        refitted = R.render(f, seed=SEED)
        assert R.rebuild_bvh() is True
        info, cost, frame = R.info(), R.bvh_cost(), R.render(f, seed=SEED)
    S.bvh_builder = abi.RT_BVH_DEVICE_SAH
    with Renderer(S) as F:
        want_info, want_cost, want = F.info(), F.bvh_cost(), F.render(f, seed=SEED)
    assert want_info["bvh_builder"] == abi.RT_BVH_DEVICE_SAH
    assert_same_tree(info, want_info)
    assert cost == want_cost, (cost, want_cost)
    assert same_bits(frame, want)
    compare(frame, refitted, 1e-12)
