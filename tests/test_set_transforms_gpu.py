"""rt_scene_set_transforms / _device / rt_multi_set_transforms through the ABI.

An edited scene has to render what a Renderer freshly made from the edited
description renders: the closest hit does not depend on the tree, so every
pixel agrees to tests/test_device_bvh.py's figure for "same hits, another tree"
(same NaN pattern, atol 1e-12), none excluded.  An edit that changes nothing
leaves the frame bit-identical.  48 pixels wide, 4 spp, depth 6; the scenes are
tests/test_live_edits.py's, which holds the shared source to the compiler
without a GPU.
"""
import ctypes as C

import numpy as np
import pytest

from rtx import abi
from rtx.lib import RtError
from rtx.render import MultiRenderer, Renderer, describe_transforms, rotate_y_row
from rtx.scene import load_scene
from test_device_bvh import compare
from test_move_spheres_gpu import SEED, frame_of, fresh, room, same_bits, sphere
from test_rebuild_gpu import assert_same_tree
import test_live_edits as E

pytestmark = pytest.mark.gpu

TREES = [(abi.RT_BVH_HOST, 0, 2), (abi.RT_BVH_DEVICE, 0, 2), (abi.RT_BVH_DEVICE_SAH, 0, 2), (abi.RT_BVH_HOST, 4, 4)]


def tree_id(t):
    return "builder%d-arity%d" % t[:2]


def boxes_edit(S):
    """One translate and one rotation of two_boxes()."""
    return {E.find(S, abi.RT_OBJ_TRANSLATE, a=(265, 0, 295)): [300.5, 12.25, 240.0],
            E.find(S, abi.RT_OBJ_ROTATE_Y, s=-18.0): rotate_y_row(33.0)}


def values_now(S, ids):
    """The rows that set each transform to what it is."""
    rows = []
    for i in ids:
        o = S.objects[i]
        if o.kind == abi.RT_OBJ_TRANSLATE or o.moving == abi.RT_STORED_FORM:
            rows.append([o.a.x, o.a.y, o.a.z])
        else:
            rows.append(rotate_y_row(o.s))
    return rows


def edited_against_fresh(S, edit, expect=None):
    """before, after: the frames around R.set_transforms(edit); after is held to a fresh Renderer's."""
    f = frame_of(S)
    with Renderer(S) as R:
        if expect:
            expect(R.info())
        before = R.render(f, seed=SEED)
        R.set_transforms(list(edit), list(edit.values()))
        after = R.render(f, seed=SEED)
    assert not same_bits(before, after), "the edit changed no pixel: the test would see nothing"
    compare(after, fresh(S, f), 1e-12)
    return before, after


# ---------------------------------------------------------------- edited against fresh
@pytest.mark.parametrize("t", TREES, ids=tree_id)
def test_two_boxes_follow_a_translate_and_a_rotation(t):
    S = load_scene(E.two_boxes())
    S.bvh_builder, S.bvh_arity = t[0], t[1]
    edit = boxes_edit(S)

    def expect(info):
        assert info["bvh_builder"] == t[0] and info["bvh_arity"] == t[2] and info["n_nodes"] > 0, info
        assert not info["features"] & abi.RT_FEAT_FLAT

    edited_against_fresh(S, edit, expect)
    rot = S.objects[list(edit)[1]]  # the description followed: the stored form
    assert rot.moving == abi.RT_STORED_FORM and [rot.a.x, rot.a.y] == rotate_y_row(33.0)[:2]


def test_a_flat_world_with_a_translated_sphere():
    S = load_scene(room([{"type": "translate", "offset": [200, 120, 200], "object": sphere([0, 0, 0], 90, "glass")}]))
    t = E.find(S, abi.RT_OBJ_TRANSLATE, a=(200, 120, 200))

    def expect(info):
        assert info["features"] & abi.RT_FEAT_FLAT and info["n_nodes"] == 0 and info["n_leaf_refs"] <= 8, info

    edited_against_fresh(S, {t: [330.0, 200.5, 310.0]}, expect)


def test_the_fog_box_of_cornell_fog_leaves_its_old_box():
    """The medium's new world box is disjoint from the old one (the twin's
    boxes say so): a stale mbox would cull the fog wherever it now stands."""
    old, new = E.fog_boxes_before_and_after()
    assert (new[0, :3] > old[0, 3:]).any() or (new[0, 3:] < old[0, :3]).any()
    S = E.fog_scene()
    edited_against_fresh(S, {E.find(S, abi.RT_OBJ_TRANSLATE, a=(265, 0, 295)): E.FOG_AWAY},
                         lambda info: info["features"] & abi.RT_FEAT_MEDIA or pytest.fail("no medium"))


def test_a_sphere_bounded_medium_under_a_translate_inside_its_boundary():
    S = load_scene(E.fog_ball())
    edited_against_fresh(S, {E.find(S, abi.RT_OBJ_TRANSLATE, a=(180, 150, 200)): [370.0, 300.0, 330.0]})


def test_a_medium_wrapped_in_a_translate_of_its_own():
    S = load_scene(E.fog_wrapped())
    edited_against_fresh(S, {E.find(S, abi.RT_OBJ_TRANSLATE, a=(120, 0, 150)): [330.0, 60.0, 280.0]})


def test_a_translated_lamp_the_world_and_the_lights_share():
    S = load_scene(E.translated_lamp())
    lamp = E.shared_lamp(S)
    edited_against_fresh(S, {lamp: [120.0, 500.0, 300.0]},
                         lambda info: info["n_light_leaves"] == 1 or pytest.fail("no light leaf"))


def test_a_transform_shared_by_two_chains():
    S = load_scene(E.shared_transform())
    edited_against_fresh(S, {E.find(S, abi.RT_OBJ_TRANSLATE, a=(200, 0, 180)): [300.0, 40.0, 90.0]})


# ---------------------------------------------------------------- round trips
@pytest.mark.parametrize("t", [TREES[0], TREES[2], TREES[3]], ids=tree_id)
def test_round_trips_leave_the_frame_bit_identical(t):
    S = load_scene(E.two_boxes())
    S.bvh_builder, S.bvh_arity = t[0], t[1]
    f = frame_of(S)
    every = [i for i, o in enumerate(S.objects) if o.kind in (abi.RT_OBJ_TRANSLATE, abi.RT_OBJ_ROTATE_Y)]
    assert len(every) == 4
    edit = boxes_edit(S)
    home = values_now(S, list(edit))
    with Renderer(S) as R:
        before = R.render(f, seed=SEED)
        R.set_transforms(every, values_now(S, every))
        assert same_bits(R.render(f, seed=SEED), before)
        R.set_transforms(list(edit), list(edit.values()))
        assert not same_bits(R.render(f, seed=SEED), before)
        R.set_transforms(list(edit), home)
        assert same_bits(R.render(f, seed=SEED), before)
        R.set_transforms([], np.zeros((0, 3)))  # n = 0: a no-op
        assert same_bits(R.render(f, seed=SEED), before)


def test_a_fog_round_trip_leaves_the_frame_bit_identical():
    S = E.fog_scene()
    f = frame_of(S)
    t = E.find(S, abi.RT_OBJ_TRANSLATE, a=(265, 0, 295))
    with Renderer(S) as R:
        before = R.render(f, seed=SEED)
        R.set_transforms([t], [E.FOG_AWAY])
        assert not same_bits(R.render(f, seed=SEED), before)
        R.set_transforms([t], [[265.0, 0.0, 295.0]])
        assert same_bits(R.render(f, seed=SEED), before)


# ---------------------------------------------------------------- device arrays, ordering, multi
def test_device_array_variant_equals_the_host_variant():
    import torch
    A, D = load_scene(E.two_boxes()), load_scene(E.two_boxes())
    f = frame_of(A)
    edit = boxes_edit(A)
    with Renderer(A) as R:
        R.set_transforms(list(edit), list(edit.values()))
        host = R.render(f, seed=SEED)
    side = torch.cuda.Stream()
    d_ids = torch.tensor(list(edit), dtype=torch.int32, device="cuda")
    d_val = torch.tensor(list(edit.values()), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with Renderer(D) as R:
        R.set_transforms_device(d_ids.data_ptr(), d_val.data_ptr(), len(edit), side.cuda_stream)
        dev = R.render(f, seed=SEED)  # on the scene's own stream: ordered after the edit by the launch chain
        side.synchronize()
    assert same_bits(dev, host)


def test_device_variant_skips_what_the_host_variant_refuses():
    import torch
    A, who = E.refusal_scene()
    D, _ = E.refusal_scene()
    f = frame_of(A)
    n, p, nan = len(A.objects), [1.0, 2.0, 3.0], float("nan")
    good = {who["translate"]: [300.5, 12.25, 240.0], who["rotate"]: rotate_y_row(-35.0), who["other"]: [90.0, 30.0, 100.0]}
    with Renderer(A) as R:
        unedited = R.render(f, seed=SEED)
        R.set_transforms(list(good), list(good.values()))
        want = R.render(f, seed=SEED)
    assert not same_bits(want, unedited)
    twice, third_t, third_r = who["other_rotate"], who["third"], who["third_rotate"]
    g = list(good.items())
    entries = [g[0], (-5, p), (n + 3, p), (who["wall"], p), (who["sphere"], p), (twice, [0.6, 0.8, 0.0]), g[1],
               (who["world"], p), (who["medium"], p), (who["idle_translate"], p), (twice, [0.8, 0.6, 0.0]),
               (third_t, [1.0, nan, 3.0]), (third_r, [float("inf"), 0.5, 0.0]), g[2], (who["fog_face"], p)]
    d_ids = torch.tensor([e[0] for e in entries], dtype=torch.int32, device="cuda")
    d_val = torch.tensor([e[1] for e in entries], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with Renderer(D) as R:
        R.set_transforms_device(d_ids.data_ptr(), d_val.data_ptr(), len(entries))
        got = R.render(f, seed=SEED)
        torch.cuda.synchronize()
    assert same_bits(got, want)


def test_an_edit_waits_for_the_render_before_it():
    """render_device on one stream, the edit right behind it on another: the
    render's frame is the unedited scene's, complete; the next is the edited scene's."""
    import torch
    S = load_scene(E.two_boxes())
    f = frame_of(S, samples_per_pixel=64)
    edit = boxes_edit(S)
    shape = (f.image_height, f.image_width, 3)
    first, racing, after = (torch.full(shape, -1.0, dtype=torch.float64, device="cuda") for _ in range(3))
    d_ids = torch.tensor(list(edit), dtype=torch.int32, device="cuda")
    d_val = torch.tensor(list(edit.values()), dtype=torch.float64, device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with Renderer(S) as R:
        kw = dict(seed=SEED, output=abi.RT_OUT_SCALED, accumulate=0)
        R.render_device(f, first.data_ptr(), s1.cuda_stream, **kw)
        s1.synchronize()
        R.render_device(f, racing.data_ptr(), s1.cuda_stream, **kw)
        R.set_transforms_device(d_ids.data_ptr(), d_val.data_ptr(), len(edit), s2.cuda_stream)
        R.render_device(f, after.data_ptr(), s1.cuda_stream, **kw)
        s1.synchronize()
        s2.synchronize()
        first, racing, after = first.cpu().numpy(), racing.cpu().numpy(), after.cpu().numpy()
    assert same_bits(racing, first)
    assert not same_bits(after, first)
    S2 = load_scene(E.two_boxes())
    describe_transforms(S2, list(edit), list(edit.values()))
    compare(after, fresh(S2, f), 1e-12)


def test_multi_set_transforms_equals_one_device():
    A, M = E.fog_scene(), E.fog_scene()
    f = frame_of(A)
    edit = {E.find(A, abi.RT_OBJ_TRANSLATE, a=(265, 0, 295)): [230.0, 40.0, 200.0],
            E.find(A, abi.RT_OBJ_ROTATE_Y, s=15.0): rotate_y_row(-20.0)}
    with Renderer(A) as R:
        R.set_transforms(list(edit), list(edit.values()))
        one = R.render(f, seed=SEED)
    with MultiRenderer(M, devices=(0,), shards=3) as R:
        unedited = R.render(f, seed=SEED)
        R.set_transforms(list(edit), list(edit.values()))
        multi = R.render(f, seed=SEED)
    assert same_bits(multi, one) and not same_bits(unedited, one)
    assert [(o.a.x, o.a.y, o.a.z, o.moving) for o in M.objects] == [(o.a.x, o.a.y, o.a.z, o.moving) for o in A.objects]


# ---------------------------------------------------------------- refusals
def described(S):
    return [(o.kind, o.moving, o.s, o.a.x, o.a.y, o.a.z) for o in S.objects]


def test_refusals_leave_the_scene_untouched():
    S, who = E.refusal_scene()
    f = frame_of(S)
    cases = [c for c in E.refusals(S, who) if c[0] == "set_transforms"]
    assert len(cases) >= 9
    was = described(S)
    with Renderer(S) as R:
        before = R.render(f, seed=SEED)
        for _, what, ids, values, code in cases:
            with pytest.raises(RtError) as e:
                R.set_transforms(ids, values)
            assert e.value.code == code, what
            assert len(str(e.value)) > len("rt error %d: " % code), what
            assert same_bits(R.render(f, seed=SEED), before), what
        assert described(S) == was
        R.set_transforms([who["rotate"]], [[0.6, 0.8, float("nan")]])  # the third value of a rotate_y row is not looked at
        R.set_transforms([who["translate"]], [[300.0, 10.0, 250.0]])  # and the scene still follows
        assert not same_bits(R.render(f, seed=SEED), before)


# ---------------------------------------------------------------- rebuild
@pytest.mark.parametrize("t", [TREES[0], TREES[3]], ids=tree_id)
def test_a_rebuild_after_an_edit_is_a_fresh_device_sah_scene(t):
    S = load_scene(E.two_boxes())
    S.bvh_builder, S.bvh_arity = t[0], t[1]
    f = frame_of(S)
    edit = boxes_edit(S)
    with Renderer(S) as R:
        R.set_transforms(list(edit), list(edit.values()))
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


# ---------------------------------------------------------------- the kernels against the twin
def kernels():
    from rtx.lib import load
    L = load()
    vp = C.c_void_p
    L.rtk_medium_boxes.argtypes, L.rtk_medium_boxes.restype = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp], C.c_int
    L.rtk_item_boxes.argtypes, L.rtk_item_boxes.restype = [vp, C.c_int, vp, vp, vp, vp, vp], C.c_int
    return L


def upload(table):
    import torch
    raw = np.frombuffer(table.tobytes() or b"\0", dtype=np.uint8).copy()
    return torch.from_numpy(raw).cuda()


GUARD, FILL = 4096, 0xCD


@pytest.mark.parametrize("name", ["cornell_fog", "fog_ball", "fog_wrapped"])
def test_medium_boxes_kernel_gives_the_twins_bytes(name):
    import torch
    S = E.fog_scene() if name == "cornell_fog" else load_scene(E.MEDIA_SCENES[name]())
    with E.Compiled(S) as T:
        tables = {k: upload(T.table(k)) for k in ("mitems", "media", "bitems", "spheres", "quads", "xforms")}
        n, want = len(T.table("mitems")), T.medium_boxes()
        assert want.tobytes() == T.table("mbox").tobytes()
    out = torch.full((24 * n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    rc = kernels().rtk_medium_boxes(tables["mitems"].data_ptr(), n, tables["media"].data_ptr(), tables["bitems"].data_ptr(),
                                    tables["spheres"].data_ptr(), tables["quads"].data_ptr(), tables["xforms"].data_ptr(),
                                    out.data_ptr(), st.cuda_stream)
    st.synchronize()
    got = out.cpu().numpy()
    assert rc == 0 and n > 0
    assert got[:24 * n].tobytes() == want.tobytes() and (got[24 * n:] == FILL).all()


def test_item_boxes_kernel_gives_the_twins_bytes_after_an_edit():
    import torch
    S = load_scene(E.two_boxes())
    edit = boxes_edit(S)
    with E.Compiled(S) as T:
        built = T.item_boxes(leaf_order=True)
        assert T.set_transforms(list(edit), list(edit.values()))[0] == 0
        tables = {k: upload(T.table(k)) for k in ("items", "spheres", "quads", "xforms")}
        n, want = len(T.table("items")), T.item_boxes(leaf_order=True)
    assert want.tobytes() != built.tobytes()
    out = torch.full((48 * n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    rc = kernels().rtk_item_boxes(tables["items"].data_ptr(), n, tables["spheres"].data_ptr(), tables["quads"].data_ptr(),
                                  tables["xforms"].data_ptr(), out.data_ptr(), st.cuda_stream)
    st.synchronize()
    got = out.cpu().numpy()
    assert rc == 0 and got[:48 * n].tobytes() == want.tobytes() and (got[48 * n:] == FILL).all()
