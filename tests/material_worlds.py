"""Worlds that put every material and texture in front of every render instance.

test_gpu_instances.feature_scene(F) selects instance F with three Lambertian
colours, one lamp, one glass sphere and at most one noise texture.
material_scene(F) keeps its items (so the item counts and the feature set stay
what they are) and changes materials, the camera and one offset:

  brushed   metal, fuzz 0.3: the x = 0 wall, and the translated sphere of the
            flat transform worlds
  mirror    metal, fuzz 0: the back wall (z = 555)
  tiled     Lambertian over the checker `tiles` (scale 70): the x = 555 wall
  nested    Lambertian over the checker `nested` (scale 200) whose even side is
            `tiles` and whose odd side is the noise texture where F has NOISE:
            the ceiling (y = 555)
  medium    a medium without noise scatters with `tiles` as its albedo
  lamp      emits a checker (scale 50) of (15, 15, 15) and (4, 4, 4)
  bubble    dielectric of index 0.6667: the second filler sphere of the worlds
            that have three spheres
  moving    the world's last sphere moves by (20, 15, 0) over the shutter
  lens      defocus_angle 0.8, focus_dist 900

Checkers stay on planes at 555 or 554: floor(p / scale) of a coordinate that
is 0 up to rounding takes its parity from the hit point's last bit, and two
correct renderers then disagree by whole colours.  With
scales 70, 200 and 50 no cell boundary is near such a plane.  The translated
box of the tree worlds stands at (330, 0, 300): at feature_scene's (130, 0, 65)
it reaches into the sphere light, and shading points inside a light are NaN in
the reference too, which hides a quarter of the frame.

`without` names one ingredient to take out again (plain white Lambertian, or
switched off): test_material_worlds.py shows that each one changes the frame.
"""
import json

from test_gpu_instances import feature_scene, MEDIA, XFORM, LIGHTS, NOISE, FLAT  # noqa: F401

WHITE = {"type": "lambertian", "albedo": [0.73, 0.73, 0.73]}
INGREDIENTS = ("brushed", "mirror", "tiled", "nested", "glass", "lens", "moving", "bubble")
TWO_TABLE_F = (8, 9, 24, 31)

X555, X0, CEILING, FLOOR, BACK, LAMP = range(6)  # feature_scene's world order


def _is_sphere(o):
    return o["type"] == "sphere" or (o["type"] == "translate" and o["object"]["type"] == "sphere")


def has_bubble(F):
    """The worlds with three spheres: a tree without a transformed item."""
    return not F & (XFORM | FLAT)


def ingredients(F):
    return tuple(k for k in INGREDIENTS if k != "bubble" or has_bubble(F))


def material_scene(F, without=None):
    assert without is None or without in ingredients(F), without
    d = json.loads(json.dumps(feature_scene(F)))
    on = lambda name: without != name  # noqa: E731
    M = d["materials"]
    M["brushed"] = {"type": "metal", "albedo": [0.8, 0.7, 0.6], "fuzz": 0.3} if on("brushed") else WHITE
    M["mirror"] = {"type": "metal", "albedo": [0.9, 0.9, 0.9], "fuzz": 0.0} if on("mirror") else WHITE
    M["tiled"] = {"type": "lambertian", "texture": "tiles"} if on("tiled") else WHITE
    M["nested"] = {"type": "lambertian", "texture": "nested"} if on("nested") else WHITE
    M["bubble"] = {"type": "dielectric", "refraction_index": 0.6667} if on("bubble") else WHITE
    if not on("glass"):
        M["glass"] = WHITE
    M["light"] = {"type": "diffuse_light", "texture": "lamp"}
    T = d.setdefault("textures", {})
    T["tiles"] = {"type": "checker", "scale": 70, "even": [0.2, 0.3, 0.1], "odd": [0.9, 0.9, 0.9]}
    T["nested"] = {"type": "checker", "scale": 200, "even": "tiles",
                   "odd": "fog" if F & NOISE else [0.3, 0.4, 0.7]}
    T["lamp"] = {"type": "checker", "scale": 50, "even": [15, 15, 15], "odd": [4, 4, 4]}

    w = d["world"]
    w[X0]["material"] = "brushed"
    w[BACK]["material"] = "mirror"
    w[X555]["material"] = "tiled"
    w[CEILING]["material"] = "nested"
    for o in w:
        if o["type"] == "constant_medium" and "texture" not in o:
            o.pop("albedo")
            o["texture"] = "tiles"
        if o["type"] == "translate" and o["object"]["type"] == "sphere":
            o["object"]["material"] = "brushed"
        elif o["type"] == "translate":  # the box: out of the sphere light
            o["offset"] = [330, 0, 300]
    spheres = [o for o in w if _is_sphere(o)]
    if has_bubble(F):
        assert len(spheres) == 3
        spheres[2]["material"] = "bubble"
    if on("moving"):
        s = spheres[-1]
        s = s["object"] if s["type"] == "translate" else s
        c = s["center"]
        s["center2"] = [c[0] + 20, c[1] + 15, c[2]]
    if on("lens"):
        d["camera"]["defocus_angle"] = 0.8
        d["camera"]["focus_dist"] = 900
    return d


def two_table_scene(F):
    """material_scene(F) with a second Perlin table (the first one's arrays,
    each reversed) under a second noise texture on the floor, the one wall that
    is still white: a scene of two tables keeps them in memory (rt_lds_plan.cpp)
    and tex_value reads S.perlin[1]."""
    assert F in TWO_TABLE_F
    d = material_scene(F)
    fog = d["perlin"]["fog"]
    d["perlin"]["fog2"] = {k: fog[k][::-1] for k in ("rand_vec", "perm_x", "perm_y", "perm_z")}
    d["textures"]["fog2"] = {"type": "noise", "scale": 0.05, "perlin": "fog2"}
    d["materials"]["marble2"] = {"type": "lambertian", "texture": "fog2"}
    assert d["world"][FLOOR]["material"] == "white"
    d["world"][FLOOR]["material"] = "marble2"
    return d


W, SPP, DEPTH, SEED = 32, 9, 8, 77  # 32 x 18 pixels: a ragged tile row
_oracle_frames = {}


def sized(S):
    """(camera description, frame) of scene S at the tests' size."""
    from rtx.render import camera_frame
    cam = S.camera_desc(image_width=W, samples_per_pixel=SPP, max_depth=DEPTH)
    return cam, camera_frame(cam)


def oracle_frame(key, doc):
    """The oracle's frame of world `doc` (counter mode, seed SEED): computed
    once per key, shared by the tests of a process, read-only."""
    import oracle_lib as O
    from rtx.scene import load_scene
    if key not in _oracle_frames:
        S = load_scene(doc)
        a = O.oracle_render(S, sized(S)[0], O.MODE_COUNTER, SEED)
        a.setflags(write=False)
        _oracle_frames[key] = a
    return _oracle_frames[key]


def load_emu():
    """The host build of the kernel source (tests/native/build/libemu.so, made
    here if it is stale: it depends on sources only)."""
    import ctypes as C
    import os
    import subprocess
    from rtx import abi
    native = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
    subprocess.run(["make", "-s", "-C", native, "build/libemu.so"], check=True)
    L = C.CDLL(os.environ.get("RTX_EMU_LIB", os.path.join(native, "build", "libemu.so")))
    P = C.POINTER
    L.emu_render.argtypes = [P(abi.SceneDesc), P(abi.Frame), P(abi.RenderParams), C.c_int,
                             P(C.c_double)]
    L.emu_render_stats.argtypes = L.emu_render.argtypes + [P(abi.PathStats)]
    return L


def structure(d):
    """What selects the feature set, read off the document: the structural key
    of test_feature_scenes_select_distinct_feature_sets."""
    has_medium = any(o["type"] == "constant_medium" for o in d["world"])
    has_xf = any(o["type"] == "translate" for o in d["world"])
    has_noise = "perlin" in d
    n_items = sum(6 if o["type"] == "translate" and o["object"]["type"] == "rotate_y" else 1
                  for o in d["world"] if o["type"] != "constant_medium")
    return (has_medium, has_xf, bool(d["lights"]), has_noise, n_items <= 8)
