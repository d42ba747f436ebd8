"""Object motion vectors on the host: the motion kernel's per-pixel source
compiled by g++ (csrc/rt_motion.h through tests/native/rt_motion_emu.cpp)
against a NumPy restatement of `place`, its exact-zero rule, the motion forms of
the temporal twins (tests/native/rt_temporal_motion_emu.cpp) against
rtx.temporal.NumpyOps(motion=), and the ABI.  No GPU: tests/test_motion_gpu.py
and tests/test_temporal_motion_gpu.py hold the gfx950 kernels to these twins."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rtx import abi, temporal
from rtx.lib import load
from rtx.render import (MOTION_DTYPE, describe_move, describe_quads, describe_transforms, rotate_y_row)
from rtx.scene import load_scene, make_box_quads
from rtx.temporal import NumpyOps
import oracle_lib as O
from test_denoise import H, W, frame_of
from test_temporal import (HALF, HEADER_DIR, NATIVE, PG, PH, PW, START, camera, history_of, host_temporal, linear,
                           moved_random_case, plane_guides, rays)
from test_temporal_variance import host_temporal_variance, random_variances

INF = float("inf")
_emu = {}


# ---- the twins ------------------------------------------------------------------------
def motion_emu():
    """tests/native/build/libmotion_emu.so (built on first use: motion.mk)."""
    if "motion" not in _emu:
        subprocess.run(["make", "-s", "-C", NATIVE, "-f", "motion.mk"], check=True)
        L = C.CDLL(os.path.join(NATIVE, "build", "libmotion_emu.so"))
        L.emu_pose_bytes.restype = C.c_longlong
        L.emu_pose_bytes.argtypes = [C.POINTER(abi.SceneDesc)]
        L.emu_pose.argtypes = [C.POINTER(abi.SceneDesc), C.c_void_p]
        L.emu_motion.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.Frame), C.c_void_p, C.c_longlong, C.c_void_p,
                                 C.POINTER(C.c_int)]
        _emu["motion"] = L
    return _emu["motion"]


def host_pose(S):
    """rt_scene_pose_device of the described scene: a uint8 array of rt_scene_pose_bytes."""
    d = S.desc()
    n = motion_emu().emu_pose_bytes(C.byref(d))
    assert n >= 256 and n % 256 == 0
    pose = np.zeros(n, dtype=np.uint8)
    assert motion_emu().emu_pose(C.byref(d), pose.ctypes.data) == 0
    return pose


def host_motion(S, f, pose, features=None):
    """rt_motion.h on the host: a MOTION_DTYPE array [H, W] of `S` against `pose`, written over a sentinel."""
    d = S.desc()
    n = f.image_width * f.image_height
    out = np.frombuffer(b"\xa5" * (MOTION_DTYPE.itemsize * n), dtype=MOTION_DTYPE).copy()
    feat = C.c_int(0)
    pose = np.ascontiguousarray(pose, dtype=np.uint8)
    assert motion_emu().emu_motion(C.byref(d), C.byref(f), pose.ctypes.data, len(pose), out.ctypes.data,
                                   C.byref(feat)) == 0
    if features is not None:
        features.append(feat.value)
    return out.reshape(f.image_height, f.image_width)


def temporal_motion_emu():
    """tests/native/build/libtemporal_motion_emu.so (built on first use: temporal_motion.mk)."""
    if "temporal" not in _emu:
        subprocess.run(["make", "-s", "-C", NATIVE, "-f", "temporal_motion.mk"], check=True)
        L = C.CDLL(os.path.join(NATIVE, "build", "libtemporal_motion_emu.so"))
        F, P = C.POINTER(abi.Frame), C.POINTER(abi.TemporalParams)
        L.emu_temporal_motion.argtypes = [F, C.c_void_p, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, F,
                                          C.c_void_p, C.c_void_p, P, C.c_void_p, C.c_void_p]
        L.emu_temporal_variance_motion.argtypes = [F, C.c_void_p, C.c_double, C.c_void_p, C.c_int32, C.c_void_p,
                                                   C.c_int32, F, C.c_void_p, C.c_void_p, C.c_void_p, P, C.c_void_p,
                                                   C.c_void_p, C.c_void_p]
        _emu["temporal"] = L
    return _emu["temporal"]


def host_temporal_motion(f, rgb, scale, tile_strata, strata_now, guides, g, f_prev, hist, motion, params=None,
                         v_now=None):
    """temporal_motion_pixel on the host -> (out, (col, geo)); with v_now temporal_variance_motion_pixel
    -> (out, (col, geo, var), variance_out).  hist is (col, geo) or (col, geo, var) accordingly."""
    L = temporal_motion_emu()
    rgb, guides = np.ascontiguousarray(rgb, dtype=np.float64), np.ascontiguousarray(guides, dtype=np.float64)
    motion = np.ascontiguousarray(motion, dtype=MOTION_DTYPE)
    ts = np.ascontiguousarray(tile_strata, dtype=np.int32) if tile_strata is not None else None
    var = v_now is not None
    pack, unpack, size = ((temporal.pack_variance_history, temporal.unpack_variance_history,
                           temporal.history_variance_bytes) if var else
                          (temporal.pack_history, temporal.unpack_history, temporal.history_bytes))
    prev = pack(f, hist) if hist is not None else None
    h_out = np.zeros(size(f), dtype=np.uint8)
    out = np.zeros_like(rgb)
    p = abi.temporal_params(params)
    head = (C.byref(f), rgb.ctypes.data, scale, ts.ctypes.data if ts is not None else None, strata_now,
            guides.ctypes.data, g, C.byref(f_prev) if f_prev is not None else None,
            prev.ctypes.data if prev is not None else None, motion.ctypes.data)
    pp = C.byref(p) if p is not None else None
    if not var:
        assert L.emu_temporal_motion(*head, pp, h_out.ctypes.data, out.ctypes.data) == 0
        return out, unpack(f, h_out)
    v_now = np.ascontiguousarray(v_now, dtype=np.float64)
    v_out = np.zeros_like(v_now)
    assert L.emu_temporal_variance_motion(*head, v_now.ctypes.data, pp, h_out.ctypes.data, out.ctypes.data,
                                          v_out.ctypes.data) == 0
    return out, unpack(f, h_out), v_out


# ---- the described worlds ---------------------------------------------------------------
LAM = {"type": "lambertian", "albedo": [0.5, 0.5, 0.5]}
UNIT = [1.5, 1.0, -2.0]  # the unit-radius sphere under the rotate_y that starts at 0 degrees


def motion_doc(flat=False):
    """A ground sphere, spheres (every third moving), a unit sphere under a rotate_y of 0 degrees, a free
    quad and a translate(rotate_y(box)) instance: 19 world primitives; flat: 7 (a flat world with transforms)."""
    rng = np.random.default_rng(3)
    world = [{"type": "sphere", "center": [0.0, -100.5, -1.0], "radius": 100.0, "material": LAM}]
    for k in range(3 if flat else 10):
        c = [float(rng.uniform(-3, 3)), float(rng.uniform(0.0, 2.5)), float(rng.uniform(-4, 0))]
        s = {"type": "sphere", "center": c, "radius": float(rng.uniform(0.3, 0.6)), "material": LAM}
        if k % 3 == 2:
            s["center2"] = [c[0], c[1] + 0.3, c[2]]
        world.append(s)
    world.append({"type": "rotate_y", "angle": 0.0,
                  "object": {"type": "sphere", "center": UNIT, "radius": 1.0, "material": LAM}})
    world.append({"type": "quad", "Q": [-3.0, 0.0, -5.0], "u": [2.0, 0.0, 0.0], "v": [0.0, 2.0, 0.5], "material": LAM})
    box = ([{"type": "quad", "Q": [0.0, 0.0, 0.0], "u": [1.0, 0.0, 0.0], "v": [0.0, 1.5, 0.0], "material": LAM}] if flat
           else [{"type": "quad", "Q": q, "u": u, "v": v, "material": LAM}
                 for q, u, v in make_box_quads([0, 0, 0], [1.0, 1.5, 1.0])])
    world.append({"type": "translate", "offset": [-1.5, 0.0, -1.5],
                  "object": {"type": "rotate_y", "angle": 20.0, "object": {"type": "list", "objects": box}}})
    return {"camera": {"lookfrom": [0.0, 1.5, 9.0], "lookat": [0.0, 1.0, 0.0], "vfov": 40.0}, "world": world}


WORLDS = {"flat": dict(flat=True, arity=0), "binary": dict(flat=False, arity=2), "wide": dict(flat=False, arity=4),
          "auto": dict(flat=False, arity=0)}


def world(which):
    S = load_scene(motion_doc(WORLDS[which]["flat"]))
    S.bvh_arity = WORLDS[which]["arity"]
    return S


def find(S):
    """The objects the edits name: a static and a moving free sphere, the free quad, the instance's
    translate and rotate_y, the unit sphere and its rotate_y."""
    o = {}
    for k, ob in enumerate(S.objects):
        if ob.kind == abi.RT_OBJ_SPHERE and ob.s == 1.0:
            o["unit"] = k
        elif ob.kind == abi.RT_OBJ_SPHERE and ob.s < 1.0:
            o.setdefault("moving" if ob.moving else "static", k)
        elif ob.kind == abi.RT_OBJ_QUAD and ob.b.x == 2.0:  # the free quad, by its u
            o["quad"] = k
        elif ob.kind == abi.RT_OBJ_TRANSLATE:
            o["translate"] = k
        elif ob.kind == abi.RT_OBJ_ROTATE_Y:
            o["unit_rot" if ob.s == 0.0 else "rotate"] = k
    assert len(o) == 7, o
    return o


SPHERE_STEP = np.array([0.25, -0.125, 0.0625])


def edit(S, kinds=("spheres", "quads", "transforms")):
    """One edit of each kind in the description `S`, as Renderer.move_spheres / move_quads / set_transforms
    leave it: both free spheres stepped by SPHERE_STEP, the free quad's corner moved, the instance's
    translate and rotate_y set, the unit sphere's rotate_y set to 10 degrees."""
    o = find(S)
    if "spheres" in kinds:
        ids = [o["static"], o["moving"]]
        describe_move(S, ids, [np.array(S.objects[i].a.tolist()) + SPHERE_STEP for i in ids])
    if "quads" in kinds:
        describe_quads(S, [o["quad"]], [[-3.25, 0.125, -5.5]])
    if "transforms" in kinds:
        describe_transforms(S, [o["translate"], o["rotate"], o["unit_rot"]],
                            [[-1.25, 0.25, -1.75], rotate_y_row(27.0), rotate_y_row(10.0)])
    return S


def view(w=64, h=64):
    """A pinhole camera in front of the worlds, looking down -z."""
    return camera(frame_of(w, h), center=(0.0, 1.5, 9.0), half_width=0.45)


_shared = {}


def case(which):
    """(scene before, scene now, frame, the twin's records), computed once and left unchanged."""
    if which not in _shared:
        before, now = world(which), edit(world(which))
        f = view()
        feat = []
        m = host_motion(now, f, host_pose(before), feat)
        m.setflags(write=False)
        _shared[which] = (before, now, f, m, feat[0])
    return _shared[which]


# ---- the NumPy restatement of place -------------------------------------------------------
def chains(S):
    """primitive object -> its transform objects, outermost first."""
    out = {}

    def walk(o, above):
        ob = S.objects[o]
        if ob.kind == abi.RT_OBJ_LIST:
            for k in range(ob.count):
                walk(S.children[ob.child + k], above)
        elif ob.kind in (abi.RT_OBJ_TRANSLATE, abi.RT_OBJ_ROTATE_Y):
            walk(ob.child, above + [o])
        elif ob.kind in (abi.RT_OBJ_SPHERE, abi.RT_OBJ_QUAD):
            out[o] = above

    walk(S.world, [])
    return out


def xform(S, o):
    """('t', offset) or ('r', sin, cos) of transform object o, as the tables hold it."""
    ob = S.objects[o]
    if ob.kind == abi.RT_OBJ_TRANSLATE:
        return "t", np.array(ob.a.tolist())
    if ob.moving == abi.RT_STORED_FORM:
        return "r", ob.a.x, ob.a.y
    sn, cs, _ = rotate_y_row(ob.s)
    return "r", sn, cs


def rot_in(s, c, p):
    return np.stack([c * p[..., 0] - s * p[..., 2], p[..., 1], s * p[..., 0] + c * p[..., 2]], -1)


def rot_out(s, c, p):
    return np.stack([c * p[..., 0] + s * p[..., 2], p[..., 1], -s * p[..., 0] + c * p[..., 2]], -1)


def place(S, chain, anchor, q, nl):
    """anchor + q and nl through the chain, innermost first (rt_motion.h place)."""
    p, n = anchor + q, nl
    for o in reversed(chain):
        x = xform(S, o)
        if x[0] == "t":
            p = p + x[1]
        else:
            p, n = rot_out(x[1], x[2], p), rot_out(x[1], x[2], n)
    return p, n


def anchor_of(S, o):
    return np.array(S.objects[o].a.tolist())


def restated(before, now, f, rec):
    """d and dn of every hit record, from the descriptions alone and the records' t and object."""
    c, p00, du, dv = temporal._cam(f)
    jj, ii = np.mgrid[0:f.image_height, 0:f.image_width]
    direction = p00 + ii[..., None] * du + jj[..., None] * dv - c
    d, dn = np.zeros(rec.shape + (3,)), np.zeros(rec.shape + (3,))
    ch = chains(now)
    for o in np.unique(rec["object"][rec["object"] >= 0]):
        sel = rec["object"] == o
        ro, rd, t = np.broadcast_to(c, direction[sel].shape), direction[sel], rec["t"][sel]
        for x in (xform(now, k) for k in ch[o]):  # to_local, outermost first
            if x[0] == "t":
                ro = ro - x[1]
            else:
                ro, rd = rot_in(x[1], x[2], ro), rot_in(x[1], x[2], rd)
        pl = ro + t[..., None] * rd
        ob = now.objects[o]
        if ob.kind == abi.RT_OBJ_SPHERE:
            nl = (pl - anchor_of(now, o)) / ob.s
        else:
            n = np.cross(np.array(ob.b.tolist()), np.array(ob.c.tolist()))
            nl = np.broadcast_to(n / np.linalg.norm(n), pl.shape)
        nl = np.where((temporal._dot(rd, nl) < 0)[..., None], nl, -nl)
        q = pl - anchor_of(now, o)
        p_now, n_now = place(now, ch[o], anchor_of(now, o), q, nl)
        p_prev, n_prev = place(before, ch[o], anchor_of(before, o), q, nl)
        d[sel], dn[sel] = p_prev - p_now, n_prev - n_now
    return d, dn


# Every coordinate here is below 128 in magnitude (the ground sphere's centre and radius are the largest), so
# one rounding is at most 2^-46 = 1.4e-14.  The restatement differs from the twin in how a normal is
# formed (a division by r where the tables hold 1 / r; a quad normal normalised by NumPy) and from
# there on runs the same at most 3 chain records of at most 10 operations each on both sides: fewer than 64
# roundings, 9.1e-13; a sphere normal divides a position error by r >= 0.3, 3.1e-12.
PLACE_BOUND = 4e-12


@pytest.mark.parametrize("which", list(WORLDS))
def test_twin_matches_the_restated_place(which):
    before, now, f, m, feat = case(which)
    assert bool(feat & abi.RT_FEAT_FLAT) == (which == "flat") and bool(feat & abi.RT_FEAT_BVH4) == (which == "wide")
    assert feat & abi.RT_FEAT_XFORM
    d, dn = restated(before, now, f, m)
    hit = m["object"] >= 0
    ed, en = float(np.abs(m["d"] - d)[hit].max()), float(np.abs(m["dn"] - dn)[hit].max())
    print("%s: features %d, %d hits, max |d - restated| %.3g, |dn - restated| %.3g (bound %g)"
          % (which, feat, hit.sum(), ed, en, PLACE_BOUND))
    assert ed <= PLACE_BOUND and en <= PLACE_BOUND
    # every edited object is seen, and moved
    o = find(now)
    for key in ("static", "quad", "unit"):
        on = m["object"] == o[key]
        assert on.sum() >= 4, key
        assert (np.abs(m["d"][on]).sum(-1) > 0).all(), key
    under = m["chain_object"] == o["translate"]
    assert under.sum() >= 10 and (np.abs(m["dn"][under]).sum(-1) > 0).all()
    # a miss: zeros, +inf, -1, -1
    miss = ~hit
    if miss.any():
        assert np.all(m["t"][miss] == INF) and np.all(m["chain_object"][miss] == -1)
        assert not m["d"][miss].view(np.uint64).any() and not m["dn"][miss].view(np.uint64).any()


def test_the_trees_agree_byte_for_byte():
    ref = case("binary")[3]
    for which in ("wide", "auto"):
        assert case(which)[3].tobytes() == ref.tobytes(), which


def test_a_translated_sphere_moves_by_the_negated_step():
    """d = (c_prev + q) - (c_now + q): two roundings at magnitudes below 8 (at most 2^-50 each) around an
    exact difference, so within 2^-49 of the negated step on every pixel of the sphere; the normal stays."""
    for which in ("flat", "binary"):
        before, now, f, m, _ = case(which)
        o = find(now)
        for key in ("static", "moving"):
            on = m["object"] == o[key]
            if key == "static":
                assert on.sum() >= 4
            err = float(np.abs(m["d"][on] + SPHERE_STEP).max()) if on.any() else 0.0
            print("%s %s sphere: %d pixels, max |d + step| = %.3g (bound %.3g)" % (which, key, on.sum(), err, 2.0 ** -49))
            assert err <= 2.0 ** -49
            assert not m["dn"][on].view(np.uint64).any()


def test_a_rotated_unit_sphere_turns_its_normals_by_the_angle():
    """rotate_y from 0 to 10 degrees: dn = N(0) - N(10), |dn| = 2 sin 5 |(n_x, n_z)| <= 2 sin 5, to the
    rounding of six products and sums of magnitude <= 1 (2^-52 each)."""
    before, now, f, m, _ = case("binary")
    o = find(now)
    on = m["object"] == o["unit"]
    assert on.sum() >= 50 and np.all(m["chain_object"][on] == o["unit_rot"])
    size = np.sqrt((m["dn"][on] ** 2).sum(-1))
    top = 2.0 * np.sin(np.radians(5.0))
    print("unit sphere: %d pixels, |dn| in [%.4f, %.4f], 2 sin 5 = %.4f" % (on.sum(), size.min(), size.max(), top))
    assert size.max() <= top + 8 * 2.0 ** -52
    assert size.max() > 0.9 * top  # teeth: normals near the horizontal great circle are seen
    assert np.all(m["dn"][on][:, 1] == 0.0)
    # the point turns about the y axis too: |d| = 2 sin 5 times its distance from the axis
    _, d_ref = None, restated(before, now, f, m)[0]
    np.testing.assert_allclose(m["d"][on], d_ref[on], rtol=0, atol=PLACE_BOUND)
    assert np.abs(m["d"][on]).sum(-1).min() > 0


def test_what_no_edit_touched_has_zero_bits():
    for which in WORLDS:
        before, now, f, m, _ = case(which)
        o = find(now)
        touched = np.isin(m["object"], [o["static"], o["moving"], o["quad"], o["unit"]]) | \
            (m["chain_object"] == o["translate"])
        still = (m["object"] >= 0) & ~touched
        assert still.sum() > 1000, which
        assert not m["d"][still].view(np.uint64).any() and not m["dn"][still].view(np.uint64).any(), which
        # and against the scene's own pose every record is still, moved objects included
        own = host_motion(now, f, host_pose(now))
        assert not own["d"].view(np.uint64).any() and not own["dn"].view(np.uint64).any(), which
        assert own["t"].tobytes() == m["t"].tobytes() and np.array_equal(own["object"], m["object"])
    # one kind of edit at a time moves its own objects only
    for kind, keys in (("spheres", ("static", "moving")), ("quads", ("quad",))):
        now = edit(world("binary"), (kind,))
        m = host_motion(now, view(), host_pose(world("binary")))
        o = find(now)
        moved = (np.abs(m["d"]).sum(-1) > 0) | (np.abs(m["dn"]).sum(-1) > 0)
        assert moved.any() and np.isin(m["object"][moved], [o[k] for k in keys]).all(), kind


def test_a_ragged_frame_and_a_single_pixel():
    before, now = world("binary"), edit(world("binary"))
    pose = host_pose(before)
    f = view(67, 35)
    m = host_motion(now, f, pose)
    assert m.shape == (35, 67) and (m["object"] >= 0).any() and (np.abs(m["d"]).sum(-1) > 0).any()
    one = host_motion(now, view(1, 1), pose)
    assert one.shape == (1, 1) and one["t"][0, 0] > 0


def test_a_pose_is_indexed_by_record_and_padded():
    S = world("binary")
    pose = host_pose(S).view(np.float64)
    o = find(S)
    c = np.array(S.objects[o["static"]].a.tolist())
    assert (np.abs(pose.reshape(-1, 3) - c).sum(-1) == 0).sum() == 1  # the sphere's centre is one record of it
    assert (np.abs(pose.reshape(-1, 3) - np.array([-1.5, 0.0, -1.5])).sum(-1) == 0).any()  # the translate's offset
    moved = host_pose(edit(world("binary"))).view(np.float64)
    assert moved.shape == pose.shape and (moved != pose).sum() >= 8


# ---- the temporal twins' motion forms ---------------------------------------------------
def random_motion(guides, g, seed=17, bad=True):
    """A motion plane [H, W] for test_temporal.moved_random_case: a third of the pixels still (all-zero
    bits), a few misses that carry values (ignored), the rest moved by up to a few pixels with a small dn;
    with `bad`, NaN and infinite entries."""
    rng = np.random.default_rng(seed)
    h, w = guides.shape[:2]
    m = np.zeros((h, w), dtype=MOTION_DTYPE)
    m["t"] = guides[..., 6] / np.maximum(guides[..., 7], 1.0)
    m["object"] = rng.integers(0, 9, (h, w))
    m["chain_object"] = -1
    m["d"] = rng.uniform(-0.3, 0.3, (h, w, 3)) * np.array([1.0, 1.0, 0.2])
    m["dn"] = rng.uniform(-0.05, 0.05, (h, w, 3))
    still = rng.uniform(size=(h, w)) < 0.33
    m["d"][still] = 0.0
    m["dn"][still] = 0.0
    only_dn = rng.uniform(size=(h, w)) < 0.05
    m["d"][only_dn] = 0.0
    m["object"][rng.uniform(size=(h, w)) < 0.05] = -1
    if bad:
        m["d"][6, 9, 0], m["d"][12, 31, 2], m["d"][18, 40, 1] = np.nan, np.inf, -np.inf
        m["dn"][21, 11, 1], m["dn"][27, 45, 0] = np.nan, np.inf
    return m


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_bits(got, ref, what):
    """(out, planes[, variance_out]) against NumpyOps' tuple of the same (its margin last): every array bit for bit."""
    assert same_bits(got[0], ref[0]), what + ": out"
    for k, (a, b) in enumerate(zip(got[1], ref[1])):
        assert same_bits(a, b), "%s: history plane %d" % (what, k)
    if len(got) > 2:
        assert same_bits(got[2], ref[2]), what + ": variance_out"


def motion_cases(fA, fB, hist):
    return {"moved": (fB, fA, hist, START), "defaults": (fB, fA, hist, None), "same pose": (fA, fA, hist, START),
            "tests off": (fB, fA, hist, dict(START, sigma_depth=-1, sigma_normal=-1)),
            "no history": (fB, None, None, None)}


def test_motion_twins_match_numpy_bit_for_bit():
    fA, fB, rgb, scale, guides, g, hist = moved_random_case()
    motion = random_motion(guides, g)
    v_now, var = random_variances()
    for what, (f, fp, hp, params) in motion_cases(fA, fB, hist).items():
        ref = NumpyOps().temporal(f, rgb, scale, None, g, guides, g, fp, hp, params, motion=motion)
        got = host_temporal_motion(f, rgb, scale, None, g, guides, g, fp, hp, motion, params)
        assert_same_bits(got, ref, what)
        hv = hp + (var,) if hp is not None else None
        ref = NumpyOps().temporal_variance(f, rgb, scale, None, g, guides, g, v_now, fp, hv, params, motion=motion)
        got = host_temporal_motion(f, rgb, scale, None, g, guides, g, fp, hv, motion, params, v_now=v_now)
        assert_same_bits(got, ref, what + ", variance")
    # teeth: the motion changes what the moved pixels keep, and a non-finite d keeps nothing
    plain = NumpyOps().temporal(fB, rgb, scale, None, g, guides, g, fA, hist, START)
    moved = NumpyOps().temporal(fB, rgb, scale, None, g, guides, g, fA, hist, START, motion=motion)
    assert (plain[1][0][..., 3] != moved[1][0][..., 3]).mean() > 0.1
    assert same_bits(plain[1][1], moved[1][1])  # geo is the current pose's
    for j, i in ((6, 9), (12, 31), (18, 40)):
        if guides[j, i, 7] / g >= 0.75 and (guides[j, i, 3:6] ** 2).sum() / g ** 2 >= 0.25 and motion["object"][j, i] >= 0:
            assert moved[1][0][j, i, 3] == g, (j, i)  # n_h = 0: the current count alone


def test_an_all_zero_plane_gives_the_parent_twins_bytes():
    fA, fB, rgb, scale, guides, g, hist = moved_random_case()
    v_now, var = random_variances()
    zero = np.zeros((H, W), dtype=MOTION_DTYPE)
    zero["object"] = 3  # hits that nothing moved
    zero["t"] = 1.0
    tx, ty = (W + 7) // 8, (H + 7) // 8
    strata = ((np.arange(tx * ty) * 7) % 6).astype(np.int32)
    for ts in (None, strata):
        for params in (None, START):
            got = host_temporal_motion(fB, rgb, scale, ts, g, guides, g, fA, hist, zero, params)
            assert_same_bits(got, host_temporal(fB, rgb, scale, ts, g, guides, g, fA, hist, params), "plain")
            hv = hist + (var,)
            got = host_temporal_motion(fB, rgb, scale, ts, g, guides, g, fA, hv, zero, params, v_now=v_now)
            assert_same_bits(got, host_temporal_variance(fB, rgb, scale, ts, g, guides, g, v_now, fA, hv, params),
                             "variance")
    # and so does a plane whose moved records are all misses or lie on media pixels (|n|^2 < 0.25)
    m = random_motion(guides, g)
    surface = (guides[..., 3:6] ** 2).sum(-1) / g ** 2 >= 0.25
    m["object"][surface] = -1
    got = host_temporal_motion(fB, rgb, scale, None, g, guides, g, fA, hist, m, START)
    assert_same_bits(got, host_temporal(fB, rgb, scale, None, g, guides, g, fA, hist, START), "misses and media")


@pytest.mark.parametrize("tilt", [0.0, 70.0])
def test_a_plane_slid_along_itself_reprojects_a_linear_history_exactly(tilt):
    """test_temporal.test_a_plane_reprojects_a_linear_history_exactly with the camera still and the plane
    moved: it slid along itself by `step`, so the point under a pixel stood at P + d, d = -step, and the
    history is read where P + d projects."""
    base = frame_of(PW, PH)
    f = camera(base, half_width=HALF)
    px = 2.0 * HALF / PW
    t = np.radians(tilt)
    D = 10.0
    plane = [((0.0, 0.0, -D), (np.sin(t), 0.0, np.cos(t)), None)]
    guides, _ = plane_guides(f, PG, plane)
    step = 2.5 * D * px * np.array([np.cos(t), 0.0, -np.sin(t)])  # in the plane
    c, dirs = rays(f)
    P = c + (guides[..., 6] / PG)[..., None] * dirs
    Pm = P - step
    x = (Pm[..., 0] / -Pm[..., 2]) / px + 0.5 * (PW - 1)
    y = -(Pm[..., 1] / -Pm[..., 2]) / px + 0.5 * (PH - 1)
    jj, ii = np.mgrid[0:PH, 0:PW]
    N = 9.0
    hist = history_of(linear(ii.astype(np.float64), jj.astype(np.float64)), N, guides, PG)
    motion = np.zeros((PH, PW), dtype=MOTION_DTYPE)
    motion["d"] = -step
    motion["t"] = guides[..., 6] / PG
    rgb = np.zeros((PH, PW, 3))
    inner = (x >= 0) & (x <= PW - 1 - 1e-9) & (y >= -1e-9) & (y <= PH - 1 + 1e-9)
    assert inner.sum() > 0.8 * PW * PH
    if tilt == 0.0:
        np.testing.assert_allclose(x, ii - 2.5, rtol=0, atol=1e-9)
    for params in (None, START):
        out, hist_out, margin = NumpyOps().temporal(f, rgb, 1.0, None, 0, guides, PG, f, hist, params, motion=motion)
        np.testing.assert_allclose(out[inner], linear(x, y)[inner], rtol=1e-5, atol=0)
        np.testing.assert_allclose(hist_out[0][..., 3][inner], N, rtol=1e-6)
        assert margin[inner].min() > 0.5
        twin = host_temporal_motion(f, rgb, 1.0, None, 0, guides, PG, f, hist, motion, params)
        assert_same_bits(twin, (out, hist_out), "plane %g" % tilt)
        # without the motion the still camera reads the history in place: another image
        still = NumpyOps().temporal(f, rgb, 1.0, None, 0, guides, PG, f, hist, params)[0]
        assert np.abs(still - out)[inner].max() > 0.01


# ---- ABI (no device call is reached) ----------------------------------------------------------
def test_refusals_before_any_device_call():
    L = load()
    f = camera(frame_of(36, 36))
    n = C.c_int64(-1)
    assert L.rt_scene_pose_bytes(None, C.byref(n)) == abi.RT_ERR_INVALID and b"null" in L.rt_last_error()
    assert L.rt_scene_pose_device(None, C.c_void_p(0x10000000), None) == abi.RT_ERR_INVALID
    assert b"null scene" in L.rt_last_error()
    # a scene that is never dereferenced: every call below is refused on its other arguments first
    fake = C.c_void_p(0x7000000)
    assert L.rt_scene_pose_device(fake, None, None) == abi.RT_ERR_INVALID and b"null" in L.rt_last_error()
    assert L.rt_scene_pose_device(fake, C.c_void_p(0x10000080), None) == abi.RT_ERR_INVALID
    assert b"aligned" in L.rt_last_error()
    pose, out = 0x10000000, 0x20000000
    for kw, word in ((dict(scene=None), b"null"), (dict(frame=None), b"null"), (dict(pose=0), b"null"),
                     (dict(out=0), b"null"), (dict(frame=frame_of(36, 0)), b"frame"),
                     (dict(pose=pose + 128), b"256-B aligned"), (dict(out=out + 4), b"8-B aligned")):
        a = dict(scene=fake, frame=f, pose=pose, out=out)
        a.update(kw)
        rc = L.rt_motion_device(a["scene"], C.byref(a["frame"]) if a["frame"] is not None else None,
                                C.c_void_p(a["pose"]), C.c_void_p(a["out"]), None)
        assert rc == abi.RT_ERR_INVALID and word in L.rt_last_error(), (kw, L.rt_last_error())
    # the temporal forms: the parents' refusals, and the motion plane's
    rgb, guides, hp, ho, dst, mo, vn, vo = (0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000,
                                            0x70000000, 0x80000000)
    px = 36 * 36

    def call(variance, rgb=rgb, hp=hp, ho=ho, dst=dst, mo=mo, vo=vo, g=4):
        head = (C.byref(f), C.c_void_p(rgb), 1.0, None, 4, C.c_void_p(guides), g, C.byref(f), C.c_void_p(hp),
                C.c_void_p(mo))
        if variance:
            return L.rt_temporal_variance_motion_device(*head, C.c_void_p(vn), None, C.c_void_p(ho), C.c_void_p(dst),
                                                        C.c_void_p(vo), None)
        return L.rt_temporal_motion_device(*head, None, C.c_void_p(ho), C.c_void_p(dst), None)

    for variance in (False, True):
        cases = {"null motion": (dict(mo=0), b"null device_motion"),
                 "motion inside out": (dict(mo=dst + 64), b"device_motion overlaps device_out"),
                 "out inside motion": (dict(dst=mo + 64 * px - 8), b"device_motion overlaps device_out"),
                 "motion inside history_out": (dict(mo=ho + 256), b"device_motion overlaps device_history_out"),
                 "null rgb": (dict(rgb=0), b"null"), "guide_strata 0": (dict(g=0), b"guide_strata"),
                 "unaligned history": (dict(ho=ho + 16), b"aligned"),
                 "history_out is history_prev": (dict(ho=hp), b"overlaps device_history_prev")}
        if variance:
            cases["motion inside variance_out"] = (dict(mo=vo + 8), b"device_motion overlaps device_variance_out")
            cases["null variance_out"] = (dict(vo=0), b"null")
        for what, (kw, word) in cases.items():
            assert call(variance, **kw) == abi.RT_ERR_INVALID, what
            assert word in L.rt_last_error(), (what, L.rt_last_error())
    with pytest.raises(ValueError):
        NumpyOps().temporal(f, np.zeros((36, 36, 3)), 1.0, None, 1, np.zeros((36, 36, 8)), 1, f,
                            (np.zeros((36, 36, 4), np.float32),) * 2, None, motion=np.zeros((3, 3), MOTION_DTYPE))


def test_exports():
    L = load()
    for name in ("rt_scene_pose_bytes", "rt_scene_pose_device", "rt_motion_device", "rt_temporal_motion_device",
                 "rt_temporal_variance_motion_device"):
        assert name in abi.EXPORTS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None
    from rtx.render import Renderer
    from rtx.temporal import HipOps, TemporalDisplay
    for cls, names in ((Renderer, ("pose_bytes", "pose_device", "motion_device")), (TemporalDisplay, ("edited",))):
        for name in names:
            assert callable(getattr(cls, name))
    import inspect
    for fn in (HipOps.temporal, HipOps.temporal_variance, NumpyOps.temporal, NumpyOps.temporal_variance):
        assert "motion" in inspect.signature(fn).parameters


def test_rt_motion_is_64_bytes_as_gcc_lays_it_out(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_api.h"', "int main(void) {",
             'printf("%zu\\n", sizeof(rt_motion));']
    want = [C.sizeof(abi.Motion)]
    for name, _ in abi.Motion._fields_:
        lines.append('printf("%%zu\\n", offsetof(rt_motion, %s));' % name)
        want.append(getattr(abi.Motion, name).offset)
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", HEADER_DIR, str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want and got[0] == 64 == MOTION_DTYPE.itemsize
    assert [MOTION_DTYPE.fields[n][1] for n, _ in abi.Motion._fields_] == want[1:]
