"""The device BVH builders, read back node by node.

rtk_build_sah (rt_bvh_sah.hip) and rtk_build_lbvh (rt_bvh_build.hip) build
over torch buffers on torch's current stream; the host then holds the result to

  * the return code, 4 KiB guards behind the nodes, the items, the temp layout
    (and the linear BVH's depth word), and node records past n_nodes -- all
    pre-filled with 0xCD -- staying untouched;
  * check_tree / check_sah_choice (tests/bvh_reference.py): what any correct
    tree has to satisfy, derived from neither builder;
  * the NumPy restatement of the kernels, bit for bit: node bytes, item order,
    n_nodes, depth, root_leaf;
  * two builds of one input giving the same bytes.

The inputs are tests/bvh_reference.py's families, where such builders break;
tests/test_bvh_builders.py runs the same restatements without a GPU.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bvh_reference as B

pytestmark = pytest.mark.gpu
GUARD, FILL = 4096, 0xCD


def _id(case):
    return "-".join(str(v) for v in case)


@functools.lru_cache(maxsize=None)
def library():
    from rtx.lib import load
    L = load()
    vp = C.c_void_p
    for f in (L.rtk_sah_temp_bytes, L.rtk_lbvh_temp_bytes):
        f.argtypes, f.restype = [C.c_int], C.c_size_t
    L.rtk_build_sah.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_size_t, C.c_int, C.POINTER(C.c_int),
                                C.POINTER(C.c_int), C.POINTER(C.c_int), vp]
    L.rtk_build_sah.restype = C.c_int
    L.rtk_build_lbvh.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), vp, vp, vp, vp,
                                 C.c_size_t, vp]
    L.rtk_build_lbvh.restype = C.c_int
    return L


class Built:
    """One build, downloaded: nodes (all max(n - 1, 1) records), items_out,
    n_nodes, depth, root_leaf, and `guards`, the names of overwritten regions."""


def device_build(builder, family, n, budget=B.SAH_BUDGET):
    import torch
    L = library()
    boxes, items = B.case_boxes(family, n), B.make_items(n)
    room = max(n - 1, 1) * B.DNODE.itemsize
    temp_bytes = int(L.rtk_sah_temp_bytes(n) if builder == "sah" else L.rtk_lbvh_temp_bytes(n))

    def filled(nbytes):
        return torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")

    d_boxes = torch.from_numpy(np.array(boxes)).cuda()
    d_items = torch.from_numpy(items.view(np.uint8).copy()).cuda()
    bufs = {"nodes": (filled(room), room), "items_out": (filled(n * B.DITEM.itemsize), n * B.DITEM.itemsize),
            "temp": (filled(temp_bytes), temp_bytes), "depth": (filled(4), 4)}
    ptr = {k: v[0].data_ptr() for k, v in bufs.items()}
    stream = torch.cuda.current_stream()
    r = Built()
    if builder == "sah":
        n_nodes, depth, root_leaf = C.c_int(-7), C.c_int(-7), C.c_int(-7)
        r.rc = L.rtk_build_sah(d_boxes.data_ptr(), d_items.data_ptr(), n, ptr["nodes"], ptr["items_out"], ptr["temp"],
                               temp_bytes, budget, C.byref(n_nodes), C.byref(depth), C.byref(root_leaf),
                               stream.cuda_stream)
        stream.synchronize()
        r.n_nodes, r.depth, r.root_leaf = n_nodes.value, depth.value, root_leaf.value
    else:
        c = 0.5 * (boxes[:, :3] + boxes[:, 3:])  # rt_scene.cpp: the centroid bounds
        lo, hi = (C.c_double * 3)(*c.min(axis=0)), (C.c_double * 3)(*c.max(axis=0))
        r.rc = L.rtk_build_lbvh(d_boxes.data_ptr(), d_items.data_ptr(), n, lo, hi, ptr["nodes"], ptr["items_out"],
                                ptr["depth"], ptr["temp"], temp_bytes, stream.cuda_stream)
        stream.synchronize()
        r.n_nodes, r.root_leaf = n - 1, 0
        r.depth = int(bufs["depth"][0][:4].cpu().numpy().view(np.int32)[0])
    host = {k: v[0].cpu().numpy() for k, v in bufs.items()}
    r.guards = [k for k, (_, size) in bufs.items() if (host[k][size:] != FILL).any()]
    if builder == "sah" and (host["depth"] != FILL).any():
        r.guards.append("depth")
    r.nodes = host["nodes"][:room].view(B.DNODE)
    r.items_out = host["items_out"][:n * B.DITEM.itemsize].view(B.DITEM)
    r.boxes, r.items_in = boxes, items
    return r


device = functools.lru_cache(maxsize=None)(device_build)


@functools.lru_cache(maxsize=None)
def restated(builder, family, n, budget=B.SAH_BUDGET):
    boxes = B.case_boxes(family, n)
    if builder == "sah":
        return B.sah_reference(boxes, budget)
    nodes, order, depth = B.lbvh_reference(boxes)
    return nodes, order, n - 1, depth, 0


def assert_sound(r):
    assert r.rc == 0
    assert r.guards == [], "written outside their range: %s" % r.guards
    assert 0 <= r.n_nodes <= len(r.nodes)
    assert (r.nodes[r.n_nodes:].view(np.uint8) == FILL).all(), "a node record past n_nodes was written"
    B.check_tree(r.boxes, r.items_in, r.nodes, r.items_out, r.n_nodes, r.depth, r.root_leaf)


def assert_equal(r, want):
    nodes, order, n_nodes, depth, root_leaf = want
    assert (r.n_nodes, r.depth, r.root_leaf) == (n_nodes, depth, root_leaf)
    assert np.array_equal(r.items_out["id"], order)
    assert r.items_out.tobytes() == r.items_in[order].tobytes()
    got = r.nodes[:n_nodes]
    for f in ("entry", "lo", "hi", "pad"):
        a, b = got[f].view(np.uint32), nodes[f].view(np.uint32)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, "%s%s: device %r, restatement %r (%d words differ)" % (
            f, tuple(bad[0]), got[f][tuple(bad[0])], nodes[f][tuple(bad[0])], len(bad))
    assert got.tobytes() == nodes.tobytes()


@pytest.mark.parametrize("case", B.SAH_CASES, ids=_id)
def test_sah_device_tree_is_sound_and_takes_the_cheapest_planes(case):
    r = device("sah", *case)
    assert_sound(r)
    B.check_sah_choice(r.boxes, r.items_in, r.nodes, r.items_out, r.n_nodes, case[2])


@pytest.mark.parametrize("case", B.SAH_CASES, ids=_id)
def test_sah_device_tree_equals_the_restatement(case):
    r = device("sah", *case)
    assert r.rc == 0
    if case in B.FORCED_CASES:
        print("forced splits: %s n = %d, budget %d: depth %d, %d inner nodes" % (case + (r.depth, r.n_nodes)))
    assert_equal(r, restated("sah", *case))


@pytest.mark.parametrize("case", B.LBVH_CASES, ids=_id)
def test_lbvh_device_tree_is_sound(case):
    assert_sound(device("lbvh", *case))


@pytest.mark.parametrize("case", B.LBVH_CASES, ids=_id)
def test_lbvh_device_tree_equals_the_restatement(case):
    r = device("lbvh", *case)
    assert r.rc == 0
    assert_equal(r, restated("lbvh", *case))


@pytest.mark.parametrize("family", list(B.FAMILIES))
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_two_builds_give_the_same_bytes(builder, family):
    """rt_bvh_sah.hip's LDS min / max atomics and the linear BVH's refit race
    (which sibling arrives second) are order independent."""
    a, b = device(builder, family, 1000), device_build(builder, family, 1000)
    assert a.rc == 0 and b.rc == 0
    assert (a.n_nodes, a.depth, a.root_leaf) == (b.n_nodes, b.depth, b.root_leaf)
    assert a.nodes.tobytes() == b.nodes.tobytes()
    assert a.items_out.tobytes() == b.items_out.tobytes()


def test_builders_refuse_what_they_cannot_build():
    import torch
    L = library()
    buf = torch.full((GUARD,), FILL, dtype=torch.uint8, device="cuda")
    p, z = buf.data_ptr(), C.c_int(0)
    lo = (C.c_double * 3)(0, 0, 0)
    s = torch.cuda.current_stream().cuda_stream
    assert L.rtk_build_sah(p, p, 0, p, p, p, GUARD, 30, C.byref(z), C.byref(z), C.byref(z), s) != 0
    assert L.rtk_build_sah(p, p, 9, p, p, p, int(L.rtk_sah_temp_bytes(9)) - 1, 30, C.byref(z), C.byref(z),
                           C.byref(z), s) != 0
    assert L.rtk_build_lbvh(p, p, 1, lo, lo, p, p, p, p, GUARD, s) != 0
    assert L.rtk_build_lbvh(p, p, 9, lo, lo, p, p, p, p, int(L.rtk_lbvh_temp_bytes(9)) - 1, s) != 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == FILL).all()
