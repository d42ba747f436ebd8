"""Live transforms and quads (csrc/rt_live.h, rt_live_check.h, rt_refit.h
medium_box), without a GPU: the shared source compiled by g++ beside the scene
compiler (tests/native/rt_live_emu.cpp).

  * medium_box over the compiled tables is the compiler's HostScene::mbox, byte
    for byte, on every committed scene with a medium and on the media scenes
    below (the committed scenes hold one medium, bounded by a box whose
    transforms stand inside the boundary; a sphere-bounded medium and a medium
    with a chain of its own are described here);
  * an edit applied to the compiled tables gives the tables, the item boxes and
    the medium boxes of compiling the edited description, byte for byte;
  * a full refit of the host tree from the edited boxes is numpy_refit's;
  * rt_rotate_y_sincos returns the pair creation computes;
  * the host variants' refusals, which need no device.

tests/test_set_transforms_gpu.py and tests/test_move_quads_gpu.py hold the
library to fresh scenes on the device.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from rtx import abi
from rtx.render import describe_quads, describe_transforms, rotate_y_row
from rtx.scene import load_scene
import bvh_reference as B
from test_move_spheres_gpu import filler, room, sphere
from test_refit import collapse, committed_scenes, numpy_refit, twin_refit

NATIVE = os.path.join(os.path.dirname(__file__), "native")
DXFORM = np.dtype([("kind", "<i4"), ("pad", "<i4"), ("a", "<f8"), ("b", "<f8"), ("c", "<f8")])
DQUAD = np.dtype([("Q", "<f8", (3,)), ("u", "<f8", (3,)), ("v", "<f8", (3,)), ("n", "<f8", (3,)), ("w", "<f8", (3,)),
                  ("D", "<f8"), ("area", "<f8"), ("aa", "<i4"), ("pad", "<i4")])
DMEDIUM = np.dtype([("neg_inv_density", "<f8"), ("phase", "<i4"), ("id", "<i4"), ("b_first", "<i4"),
                    ("b_count", "<i4"), ("box", "<i4"), ("bxf_first", "<i4"), ("bxf_count", "<i4"), ("pad", "<i4"),
                    ("bnk", "<f8", (3, 2)), ("bD", "<f8", (3, 2)), ("bB", "<f8", (3,))])
DSPHERE = np.dtype([("c0", "<f8", (3,)), ("dir", "<f8", (3,)), ("inv_r", "<f8"), ("rr", "<f8")])
DLIGHT = np.dtype([("kind", "<i4"), ("idx", "<i4"), ("xf_first", "<i4"), ("xf_count", "<i4"), ("weight", "<f8"),
                   ("cum", "<f8"), ("pad", "<f8", (2,))])
assert (DXFORM.itemsize, DQUAD.itemsize, DMEDIUM.itemsize, DSPHERE.itemsize, DLIGHT.itemsize) == (32, 144, 160, 64, 48)
TABLES = {"xforms": (0, DXFORM), "quads": (1, DQUAD), "mbox": (2, np.dtype("<f4")), "nodes": (3, B.DNODE),
          "items": (4, B.DITEM), "mitems": (5, B.DITEM), "bitems": (6, B.DITEM), "media": (7, DMEDIUM),
          "spheres": (8, DSPHERE), "compile_items": (9, B.DITEM), "xf_kind": (10, np.dtype("<i4")),
          "xf_first": (11, np.dtype("<i4")), "xf_recs": (12, np.dtype("<i4")), "quad_of": (13, np.dtype("<i4")),
          "lights": (14, DLIGHT)}
X_TRANSLATE, X_ROTATE_Y = 0, 1


# ---------------------------------------------------------------- the twin
@functools.lru_cache(maxsize=None)
def twin():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "live.mk"], check=True)
    L = C.CDLL(os.path.join(NATIVE, "build", "liblive_emu.so"))
    vp = C.c_void_p
    L.live_emu_open.argtypes, L.live_emu_open.restype = [C.POINTER(abi.SceneDesc), C.c_char_p, C.c_int], vp
    L.live_emu_close.argtypes, L.live_emu_close.restype = [vp], None
    L.live_emu_table.argtypes, L.live_emu_table.restype = [vp, C.c_int, C.POINTER(C.c_longlong)], vp
    L.live_emu_root_is_leaf.argtypes, L.live_emu_root_is_leaf.restype = [vp], C.c_int
    L.live_emu_item_boxes.argtypes, L.live_emu_item_boxes.restype = [vp, C.c_int, vp], None
    L.live_emu_medium_boxes.argtypes, L.live_emu_medium_boxes.restype = [vp, vp], None
    for name in ("live_emu_set_transforms", "live_emu_move_quads"):
        getattr(L, name).argtypes = [vp, C.c_int, vp, vp, C.c_char_p, C.c_int]
        getattr(L, name).restype = C.c_int
    L.rt_rotate_y_sincos.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.rt_rotate_y_sincos.restype = C.c_int
    return L


class Compiled:
    """One compiled scene in the twin: its tables (copies, as they are now) and
    the edits applied to them."""

    def __init__(self, S):
        d = S.desc()
        msg = C.create_string_buffer(512)
        self.h = twin().live_emu_open(C.byref(d), msg, len(msg))
        assert self.h, msg.value.decode()

    def close(self):
        if self.h:
            twin().live_emu_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def table(self, name):
        which, dt = TABLES[name]
        n = C.c_longlong()
        p = twin().live_emu_table(self.h, which, C.byref(n))
        if not n.value:
            return np.zeros(0, dtype=dt)
        return np.frombuffer(C.string_at(p, n.value), dtype=dt).copy()

    def root_is_leaf(self):
        return bool(twin().live_emu_root_is_leaf(self.h))

    def item_boxes(self, leaf_order=False):
        out = np.zeros((len(self.table("items")), 6))
        twin().live_emu_item_boxes(self.h, int(leaf_order), out.ctypes.data)
        return out

    def medium_boxes(self):
        out = np.zeros((len(self.table("mitems")), 6), dtype=np.float32)
        twin().live_emu_medium_boxes(self.h, out.ctypes.data)
        return out

    def _edit(self, fn, ids, values):
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        values = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, 3)
        assert len(ids) == len(values)
        msg = C.create_string_buffer(512)
        rc = fn(self.h, len(ids), ids.ctypes.data, values.ctypes.data, msg, len(msg))
        return rc, msg.value.decode()

    def set_transforms(self, ids, values):
        return self._edit(twin().live_emu_set_transforms, ids, values)

    def move_quads(self, ids, corners):
        return self._edit(twin().live_emu_move_quads, ids, corners)

    def state(self):
        """Everything an edit may change and a recompile gives again."""
        return {"xforms": self.table("xforms").tobytes(), "quads": self.table("quads").tobytes(),
                "spheres": self.table("spheres").tobytes(), "media": self.table("media").tobytes(),
                "item boxes": self.item_boxes().tobytes(), "medium boxes": self.medium_boxes().tobytes()}


# ---------------------------------------------------------------- scenes
def placed_box(offset, angle, size, material="white"):
    return {"type": "translate", "offset": offset,
            "object": {"type": "rotate_y", "angle": angle,
                       "object": {"type": "box", "a": [0, 0, 0], "b": size, "material": material}}}


LAMP = {"type": "quad", "Q": [343, 554, 332], "u": [-130, 0, 0], "v": [0, 0, -105]}  # room()'s ceiling panel


def two_boxes():
    """room() with two Cornell boxes, each a translate(rotate_y(box)), plus filler: a world with a tree."""
    return room([placed_box([265, 0, 295], 15.0, [165, 330, 165]), placed_box([130, 0, 65], -18.0, [165, 165, 165])]
                + filler(), lights=[LAMP])


def shared_transform():
    """One translate above a sphere and a rotated box: it stands in the chains [T] and [T, R]."""
    inner = {"type": "list", "objects": [sphere([60, 230, 60], 50, "glass"),
                                         {"type": "rotate_y", "angle": 25.0,
                                          "object": {"type": "box", "a": [0, 0, 0], "b": [120, 180, 120],
                                                     "material": "white"}}]}
    return room([{"type": "translate", "offset": [200, 0, 180], "object": inner}] + filler())


def fog_ball():
    """A sphere-bounded medium whose boundary stands under a translate."""
    return room([{"type": "constant_medium", "density": 0.02, "albedo": [0.9, 0.9, 0.9],
                  "boundary": {"type": "translate", "offset": [180, 150, 200], "object": sphere([0, 0, 0], 110, None)}}]
                + filler())


def fog_wrapped():
    """A box-bounded medium wrapped in a translate of its own (the medium item has a chain)."""
    fog = {"type": "constant_medium", "density": 0.02, "albedo": [0.9, 0.9, 0.9],
           "boundary": {"type": "rotate_y", "angle": 20.0,
                        "object": {"type": "box", "a": [0, 0, 0], "b": [150, 250, 150], "material": "white"}}}
    return room([{"type": "translate", "offset": [120, 0, 150], "object": fog}] + filler())


def translated_lamp():
    """room() without its panel; the lamp is a translate over a quad that the
    world and the lights list both name (see shared_lamp)."""
    doc = room([{"type": "translate", "offset": [213, 554, 227],
                 "object": {"type": "quad", "Q": [0, 0, 0], "u": [130, 0, 0], "v": [0, 0, 105], "material": "light"}}]
               + filler(), lights=[{"type": "quad", "Q": [0, 0, 0], "u": [1, 0, 0], "v": [0, 0, 1]}])
    del doc["world"][5]
    return doc


def lamp_in_a_light_leaf():
    """The lights list holds its own translate(quad): a transform that stands in a light leaf only."""
    return room(filler(), lights=[{"type": "translate", "offset": [213, 0, 227],
                                   "object": {"type": "quad", "Q": [0, 554, 0], "u": [130, 0, 0], "v": [0, 0, 105]}}])


def skew_quad():
    """room() with a quad on no axis (aa < 0) among the filler."""
    return room([{"type": "quad", "Q": [150, 60, 250], "u": [200, 40, 60], "v": [-30, 220, 50], "material": "green"}]
                + filler(), lights=[LAMP])


MEDIA_SCENES = {"fog_ball": fog_ball, "fog_wrapped": fog_wrapped}


def shared_lamp(S):
    """translated_lamp(): the lights list's one entry becomes the world's translate object itself."""
    lamp = find(S, abi.RT_OBJ_TRANSLATE, a=(213, 554, 227))
    lights = S.objects[S.lights]
    assert lights.count == 1
    S.children[lights.child] = lamp
    return lamp


def find(S, kind, **want):
    """The one object of `kind` whose fields equal `want` (a / b / c as tuples, s)."""
    def same(o):
        for k, v in want.items():
            got = getattr(o, k)
            if (tuple(got.tolist()) if isinstance(got, abi.Vec3) else got) != (tuple(map(float, v)) if isinstance(v, tuple) else v):
                return False
        return True
    hits = [i for i, o in enumerate(S.objects) if o.kind == kind and same(o)]
    assert len(hits) == 1, (kind, want, hits)
    return hits[0]


def fog_scene():
    return load_scene(committed_scenes()["cornell_fog"])


# ---------------------------------------------------------------- medium_box against the compiler
def scenes_with_media():
    docs = dict(committed_scenes())
    docs.update({name: make() for name, make in MEDIA_SCENES.items()})
    return docs


@functools.lru_cache(maxsize=None)
def media_survey():
    """name -> (compiled mbox bytes, medium_box bytes, boundary kinds, media with a chain) of every scene with a medium."""
    out = {}
    for name, doc in scenes_with_media().items():
        with Compiled(load_scene(doc)) as T:
            mitems = T.table("mitems")
            if len(mitems) == 0:
                continue
            media, bitems = T.table("media"), T.table("bitems")
            kinds = set()
            for m in media[mitems["idx"]]:
                b = bitems[m["b_first"]:m["b_first"] + m["b_count"]]
                kinds.add("box" if m["box"] else "sphere" if (b["kind"] == 0).all() else "other")
            out[name] = (T.table("mbox").tobytes(), T.medium_boxes().tobytes(), kinds, int((mitems["xf_count"] > 0).sum()))
    return out


def test_medium_box_is_the_compilers_on_every_scene_with_a_medium():
    survey = media_survey()
    assert "cornell_fog" in survey  # the committed scene with a medium
    for name, (compiled, restated, _, _) in survey.items():
        assert len(compiled) > 0 and compiled == restated, name
    kinds = set().union(*(s[2] for s in survey.values()))
    assert {"box", "sphere"} <= kinds, kinds
    assert any(s[3] > 0 for s in survey.values()), "no medium with a chain of its own"


# ---------------------------------------------------------------- edits against a recompile
def edit_cases():
    """name -> (SceneDescription, transforms {id: row}, quads {id: corner})."""
    cases = {}
    S = load_scene(two_boxes())
    cases["a translate"] = (S, {find(S, abi.RT_OBJ_TRANSLATE, a=(265, 0, 295)): [300.5, 12.25, 240.0]}, {})
    S = load_scene(two_boxes())
    cases["a rotate_y given by rt_rotate_y_sincos"] = (S, {find(S, abi.RT_OBJ_ROTATE_Y, s=-18.0): rotate_y_row(33.0)}, {})
    S = load_scene(two_boxes())
    cases["a translate and a rotate_y"] = (S, {find(S, abi.RT_OBJ_TRANSLATE, a=(130, 0, 65)): [100.0, 20.0, 90.0],
                                               find(S, abi.RT_OBJ_ROTATE_Y, s=15.0): rotate_y_row(-40.0)}, {})
    S = load_scene(shared_transform())
    cases["a transform shared by two chains"] = (S, {find(S, abi.RT_OBJ_TRANSLATE, a=(200, 0, 180)): [260.0, 15.0, 120.0]}, {})
    S = fog_scene()
    cases["a translate inside a medium's boundary"] = (S, {find(S, abi.RT_OBJ_TRANSLATE, a=(265, 0, 295)): [40.0, 100.0, 60.0]}, {})
    S = fog_scene()
    cases["a rotate_y inside a medium's boundary"] = (S, {find(S, abi.RT_OBJ_ROTATE_Y, s=15.0): rotate_y_row(50.0)}, {})
    S = load_scene(fog_ball())
    cases["a translate above a medium's sphere"] = (S, {find(S, abi.RT_OBJ_TRANSLATE, a=(180, 150, 200)): [330.0, 260.0, 300.0]}, {})
    S = load_scene(fog_wrapped())
    cases["a transform above a medium"] = (S, {find(S, abi.RT_OBJ_TRANSLATE, a=(120, 0, 150)): [300.0, 40.0, 260.0]}, {})
    S = load_scene(lamp_in_a_light_leaf())
    cases["a transform in a light leaf"] = (S, {find(S, abi.RT_OBJ_TRANSLATE, a=(213, 0, 227)): [100.0, -3.0, 300.0]}, {})
    S = load_scene(translated_lamp())
    cases["a lamp the world and the lights share"] = (S, {shared_lamp(S): [120.0, 500.0, 300.0]}, {})
    S = load_scene(two_boxes())
    cases["a world quad"] = (S, {}, {find(S, abi.RT_OBJ_QUAD, a=(0, 0, 555), b=(555, 0, 0)): [0.0, 0.0, 470.5]})
    S = load_scene(two_boxes())
    cases["a light-only quad"] = (S, {}, {find(S, abi.RT_OBJ_QUAD, a=(343, 554, 332), material=-1): [300.0, 540.0, 400.0]})
    S = load_scene(skew_quad())
    cases["a skew quad"] = (S, {}, {find(S, abi.RT_OBJ_QUAD, a=(150, 60, 250)): [210.25, 90.5, 130.0]})
    return cases


EDITS = sorted(edit_cases())


@pytest.mark.parametrize("builder", [abi.RT_BVH_HOST, abi.RT_BVH_DEVICE], ids=["leaf-order", "scene-order"])
@pytest.mark.parametrize("what", EDITS)
def test_an_edit_of_the_tables_equals_a_recompile(what, builder):
    S, transforms, quads = edit_cases()[what]
    S.bvh_builder = builder  # the items in leaf order, or as compiled: the boxes are compared in compile order
    with Compiled(S) as T:
        before = T.state()
        if transforms:
            rc, msg = T.set_transforms(list(transforms), list(transforms.values()))
            assert rc == 0, msg
        if quads:
            rc, msg = T.move_quads(list(quads), list(quads.values()))
            assert rc == 0, msg
        edited = T.state()
    describe_transforms(S, list(transforms), list(transforms.values()))
    describe_quads(S, list(quads), list(quads.values()))
    with Compiled(S) as F:
        fresh = F.state()
        compiled_mbox = F.table("mbox").tobytes()
    assert edited != before, "the edit changed nothing: the test would see nothing"
    for key in fresh:
        assert edited[key] == fresh[key], key
    assert edited["medium boxes"] == compiled_mbox
    # what no edit may touch
    assert edited["spheres"] == before["spheres"] and edited["media"] == before["media"]


def test_the_edit_cases_cover_what_they_name():
    cases = edit_cases()
    S, tr, _ = cases["a transform shared by two chains"]
    with Compiled(S) as T:
        first, kind = T.table("xf_first"), T.table("xf_kind")
        t = list(tr)[0]
        assert first[t + 1] - first[t] == 2 and kind[t] == X_TRANSLATE
        # ... and both records changed
        before = T.table("xforms")
        assert T.set_transforms([t], [tr[t]])[0] == 0
        recs = T.table("xf_recs")[first[t]:first[t + 1]]
        changed = np.flatnonzero(before != T.table("xforms"))
        assert sorted(changed) == sorted(recs) and len(recs) == 2
    S, tr, _ = cases["a transform in a light leaf"]
    with Compiled(S) as T:
        t = list(tr)[0]
        recs = T.table("xf_recs")[T.table("xf_first")[t]:T.table("xf_first")[t + 1]]
        assert len(recs) == 1
        assert recs[0] in T.table("lights")["xf_first"] and (T.table("items")["xf_count"] == 0).all()
    S, tr, _ = cases["a lamp the world and the lights share"]
    with Compiled(S) as T:  # one chain [T], shared by the world item and the light leaf
        t = list(tr)[0]
        first = T.table("xf_first")
        assert first[t + 1] - first[t] == 1 and len(T.table("lights")) > 0 and (T.table("lights")["xf_count"] == 1).all()
    S, _, q = cases["a light-only quad"]
    with Compiled(S) as T:
        rec = T.table("quad_of")[list(q)[0]]
        assert rec >= 0 and rec not in T.table("items")["idx"][T.table("items")["kind"] == 1]
        assert rec in T.table("lights")["idx"]
    S, _, q = cases["a skew quad"]
    with Compiled(S) as T:
        quads = T.table("quads")
        assert quads["aa"][T.table("quad_of")[list(q)[0]]] < 0 and (quads["aa"] >= 0).any()
    S, tr, _ = cases["a transform above a medium"]
    with Compiled(S) as T:
        assert (T.table("mitems")["xf_count"] == 1).all() and len(T.table("mitems")) == 1
    S, tr, _ = cases["a translate inside a medium's boundary"]
    with Compiled(S) as T:
        assert (T.table("mitems")["xf_count"] == 0).all() and (T.table("bitems")["xf_count"] == 2).all()
        assert T.table("media")["box"].all()


def test_the_fog_box_can_leave_its_old_world_box():
    """What tests/test_set_transforms_gpu.py rests on: the fog's translate moved
    this far, the medium's new world box and the old one are disjoint."""
    old, new = fog_boxes_before_and_after()
    assert (new[0, :3] > old[0, 3:]).any() or (new[0, 3:] < old[0, :3]).any()


FOG_AWAY = [20.0, 340.0, 40.0]  # above and beside where cornell_fog's box stands, inside the room


def fog_boxes_before_and_after():
    S = fog_scene()
    with Compiled(S) as T:
        old = T.medium_boxes()
        assert T.set_transforms([find(S, abi.RT_OBJ_TRANSLATE, a=(265, 0, 295))], [FOG_AWAY])[0] == 0
        return old, T.medium_boxes()


# ---------------------------------------------------------------- a full refit
@pytest.mark.parametrize("what", ["a translate and a rotate_y", "a transform shared by two chains", "a world quad"])
def test_a_full_refit_from_the_edited_boxes_is_numpy_refits(what):
    S, transforms, quads = edit_cases()[what]
    S.bvh_builder = abi.RT_BVH_HOST
    with Compiled(S) as T:
        nodes = T.table("nodes")
        assert len(nodes) > 0 and not T.root_is_leaf()
        built = T.item_boxes(leaf_order=True)
        assert twin_refit(nodes, built).tobytes() == nodes.tobytes()  # the compiler's own tree
        if transforms:
            assert T.set_transforms(list(transforms), list(transforms.values()))[0] == 0
        if quads:
            assert T.move_quads(list(quads), list(quads.values()))[0] == 0
        boxes = T.item_boxes(leaf_order=True)
    assert boxes.tobytes() != built.tobytes()
    want = numpy_refit(nodes, boxes)
    assert want.tobytes() != nodes.tobytes()
    assert twin_refit(nodes, boxes).tobytes() == want.tobytes()
    wide = collapse(nodes)
    assert twin_refit(wide, boxes).tobytes() == numpy_refit(wide, boxes).tobytes()


# ---------------------------------------------------------------- rt_rotate_y_sincos
@pytest.mark.parametrize("degrees", [15.0, -18.0, 0.0, 90.0, 1e-300])
def test_rotate_y_sincos_is_the_pair_creation_holds(degrees):
    S = load_scene(room([{"type": "rotate_y", "angle": degrees, "object": sphere([100, 100, 100], 50, "white")}]))
    with Compiled(S) as T:
        x = T.table("xforms")
    assert len(x) == 1 and x["kind"][0] == X_ROTATE_Y
    want = np.array([x["a"][0], x["b"][0]])
    sn, cs = C.c_double(), C.c_double()
    assert twin().rt_rotate_y_sincos(degrees, C.byref(sn), C.byref(cs)) == 0
    assert np.array([sn.value, cs.value]).tobytes() == want.tobytes()
    row = rotate_y_row(degrees)  # the library's own, through rtx.render
    assert np.array(row[:2]).tobytes() == want.tobytes() and row[2] == 0.0
    assert twin().rt_rotate_y_sincos(degrees, None, C.byref(cs)) == abi.RT_ERR_INVALID


# ---------------------------------------------------------------- refusals
def refusal_scene():
    """two_boxes() plus a third placed box, a box-bounded fog, a translate nothing uses and a quad nothing uses."""
    doc = two_boxes()
    doc["world"].append(placed_box([380, 0, 120], 40.0, [80, 120, 80]))
    doc["world"].append({"type": "constant_medium", "density": 0.01, "albedo": [1, 1, 1],
                         "boundary": {"type": "box", "a": [400, 0, 400], "b": [500, 100, 500], "material": "white"}})
    S = load_scene(doc)
    q = S.add_object(abi.RT_OBJ_QUAD, material=0, a=(1, 2, 3), b=(1, 0, 0), c=(0, 1, 0))
    who = dict(idle_translate=S.add_object(abi.RT_OBJ_TRANSLATE, child=q, a=(1, 1, 1)), idle_quad=q,
               translate=find(S, abi.RT_OBJ_TRANSLATE, a=(265, 0, 295)), rotate=find(S, abi.RT_OBJ_ROTATE_Y, s=15.0),
               other=find(S, abi.RT_OBJ_TRANSLATE, a=(130, 0, 65)), other_rotate=find(S, abi.RT_OBJ_ROTATE_Y, s=-18.0),
               third=find(S, abi.RT_OBJ_TRANSLATE, a=(380, 0, 120)), third_rotate=find(S, abi.RT_OBJ_ROTATE_Y, s=40.0),
               wall=find(S, abi.RT_OBJ_QUAD, a=(0, 0, 555), b=(555, 0, 0)),
               lamp=find(S, abi.RT_OBJ_QUAD, a=(343, 554, 332), material=-1),
               sphere=[i for i, o in enumerate(S.objects) if o.kind == abi.RT_OBJ_SPHERE][0],
               medium=[i for i, o in enumerate(S.objects) if o.kind == abi.RT_OBJ_MEDIUM][0], world=S.world)
    who["fog_face"] = S.children[S.objects[S.objects[who["medium"]].child].child]  # the boundary box's first quad
    assert S.objects[who["fog_face"]].kind == abi.RT_OBJ_QUAD
    return S, who


def refusals(S, who):
    """(function, what, ids, values, code): every refusal the host variants list."""
    p, n, nan, inf = [1.0, 2.0, 3.0], len(S.objects), float("nan"), float("inf")
    t, r, w = who["translate"], who["rotate"], who["wall"]
    I, U = abi.RT_ERR_INVALID, abi.RT_ERR_UNSUPPORTED
    return [("set_transforms", "below range", [t, -1], [p, p], I), ("set_transforms", "above range", [t, n], [p, p], I),
            ("set_transforms", "a quad", [t, w], [p, p], I), ("set_transforms", "a sphere", [t, who["sphere"]], [p, p], I),
            ("set_transforms", "a list", [t, who["world"]], [p, p], I),
            ("set_transforms", "a medium", [t, who["medium"]], [p, p], I),
            ("set_transforms", "a transform in no chain", [t, who["idle_translate"]], [p, p], I),
            ("set_transforms", "named twice", [t, r, t], [p, p, p], I),
            ("set_transforms", "NaN", [t, r], [p, [0.6, nan, 0.0]], I),
            ("set_transforms", "an infinite offset", [r, t], [[0.6, 0.8, 0.0], [1.0, 2.0, inf]], I),
            ("move_quads", "below range", [w, -1], [p, p], I), ("move_quads", "above range", [w, n], [p, p], I),
            ("move_quads", "a translate", [w, t], [p, p], I), ("move_quads", "a sphere", [w, who["sphere"]], [p, p], I),
            ("move_quads", "a quad with no record", [w, who["idle_quad"]], [p, p], I),
            ("move_quads", "named twice", [w, who["lamp"], w], [p, p, p], I),
            ("move_quads", "NaN", [w, who["lamp"]], [p, [nan, 1.0, 1.0]], I),
            ("move_quads", "infinite", [w, who["lamp"]], [p, [1.0, -inf, 1.0]], I),
            ("move_quads", "a medium's boundary", [w, who["fog_face"]], [p, p], U)]


def test_the_host_check_refuses_without_a_device():
    S, who = refusal_scene()
    with Compiled(S) as T:
        before = T.state()
        for fn, what, ids, values, code in refusals(S, who):
            rc, msg = getattr(T, fn)(ids, values)
            assert rc == code, (fn, what, rc, msg)
            assert len(msg) > 0 and "object" in msg, (fn, what)
            assert T.state() == before, (fn, what)
        # a rotate_y row's third value is not looked at; n = 0 is a no-op
        assert T.set_transforms([who["rotate"]], [[0.6, 0.8, float("nan")]])[0] == 0
        assert T.set_transforms([], np.zeros((0, 3)))[0] == 0 and T.move_quads([], np.zeros((0, 3)))[0] == 0
        assert T.move_quads([who["wall"], who["lamp"]], [[0.0, 0.0, 500.0], [300.0, 554.0, 300.0]])[0] == 0
        assert T.state() != before


def test_a_corner_whose_plane_constant_overflows_is_refused():
    """The wall's unit normal is (0, 0, 1) up to sign: |D| = 1.7e308 is finite.  A skew quad's D is a
    sum of three products, which overflows where no coordinate does."""
    S = load_scene(skew_quad())
    q = find(S, abi.RT_OBJ_QUAD, a=(150, 60, 250))
    with Compiled(S) as T:
        n = T.table("quads")["n"][T.table("quad_of")[q]]
        big = np.sign(n) * 1.7e308
        with np.errstate(over="ignore"):
            assert np.isfinite(big).all() and not np.isfinite(n[0] * big[0] + n[1] * big[1] + n[2] * big[2])
        rc, msg = T.move_quads([q], [big])
        assert rc == abi.RT_ERR_INVALID and "plane constant" in msg
