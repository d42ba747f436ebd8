"""rtk_refit (rt_refit.hip) over torch buffers, read back node by node.

The trees are the device builders' own (rtk_build_sah, rtk_build_lbvh, through
tests/test_bvh_builders_gpu.py's cached builds: SAH leaves of several items,
linear BVHs that are not in BFS order), uploaded again beside their items into
buffers pre-filled with 0xCD with 4 KiB guards behind the nodes, the items and
the temp.  A refit from the boxes the tree was built from has to give the built
bytes back; one from other boxes has to satisfy bvh_reference.check_tree, leave
entries, pads and items alone, equal tests/test_refit.py's numpy_refit bit for
bit, do so twice, and stay inside its buffers.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bvh_reference as B
from test_bvh_builders_gpu import FILL, GUARD, device, library as builders_library
from test_refit import CASES, DNODE4, case_id, collapse, numpy_refit, second_boxes

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def library():
    L = builders_library()
    vp = C.c_void_p
    L.rtk_refit_temp_bytes.argtypes, L.rtk_refit_temp_bytes.restype = [C.c_int, C.c_int], C.c_size_t
    L.rtk_refit.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, C.c_size_t, vp]
    L.rtk_refit.restype = C.c_int
    return L


class Refitted:
    """One rtk_refit, downloaded: rc, nodes, items, and `guards`, the names of
    the regions written outside their range."""


def device_refit(nodes, root_leaf, items, boxes, temp_short=0):
    import torch
    L = library()
    arity = nodes["entry"].shape[1] if len(nodes) else 2
    n_nodes, n = len(nodes), len(items)
    temp_bytes = int(L.rtk_refit_temp_bytes(n, n_nodes))
    sizes = {"nodes": max(n_nodes, 1) * nodes.dtype.itemsize, "items": n * B.DITEM.itemsize, "temp": temp_bytes}
    bufs = {k: torch.full((v + GUARD,), FILL, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
    if n_nodes:
        bufs["nodes"][:n_nodes * nodes.dtype.itemsize] = torch.from_numpy(nodes.view(np.uint8).copy()).cuda()
    bufs["items"][:sizes["items"]] = torch.from_numpy(items.view(np.uint8).copy()).cuda()
    d_boxes = torch.from_numpy(np.array(boxes, dtype=np.float64)).cuda()
    stream = torch.cuda.current_stream()
    r = Refitted()
    r.rc = L.rtk_refit(bufs["nodes"].data_ptr(), arity, n_nodes, root_leaf, bufs["items"].data_ptr(), n,
                       d_boxes.data_ptr(), bufs["temp"].data_ptr(), temp_bytes - temp_short, stream.cuda_stream)
    stream.synchronize()
    host = {k: v.cpu().numpy() for k, v in bufs.items()}
    r.guards = [k for k, size in sizes.items() if (host[k][size:] != FILL).any()]
    r.nodes = host["nodes"][:sizes["nodes"]].view(nodes.dtype)
    r.items = host["items"][:sizes["items"]].view(B.DITEM)
    r.temp = host["temp"][:temp_bytes]
    return r


def built(case):
    builder, family, n = case
    r = device(builder, family, n, B.SAH_BUDGET) if builder == "sah" else device(builder, family, n)
    assert r.rc == 0
    return r


def leaf_order(r):
    """The input index of each output item (the items carry it as their id)."""
    return r.items_out["id"].astype(np.int64)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_refit_from_the_built_boxes_reproduces_the_built_nodes(case):
    r = built(case)
    nodes = r.nodes[:r.n_nodes]
    got = device_refit(nodes, r.root_leaf, r.items_out, r.boxes[leaf_order(r)])
    assert got.rc == 0 and got.guards == []
    if r.n_nodes == 0:
        assert (got.nodes.view(np.uint8) == FILL).all() and (got.temp == FILL).all()
    else:
        assert got.nodes.tobytes() == nodes.tobytes()
    assert got.items.tobytes() == r.items_out.tobytes()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_refit_from_other_boxes_is_sound_and_equals_the_restatement(case):
    r = built(case)
    family, n = case[1], case[2]
    nodes, order = r.nodes[:r.n_nodes], leaf_order(r)
    new = second_boxes(family, n)
    got = device_refit(nodes, r.root_leaf, r.items_out, new[order])
    assert got.rc == 0 and got.guards == []
    assert got.items.tobytes() == r.items_out.tobytes()
    if r.n_nodes == 0:
        assert (got.nodes.view(np.uint8) == FILL).all()
        return
    B.check_tree(new, r.items_in, got.nodes, got.items, r.n_nodes, r.depth, r.root_leaf)
    assert np.array_equal(got.nodes["entry"], nodes["entry"]) and np.array_equal(got.nodes["pad"], nodes["pad"])
    want = numpy_refit(nodes, new[order])
    for f in ("lo", "hi"):
        a, b = got.nodes[f].view(np.uint32), want[f].view(np.uint32)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, "%s%s: device %r, restatement %r (%d words differ)" % (
            f, tuple(bad[0]), got.nodes[f][tuple(bad[0])], want[f][tuple(bad[0])], len(bad))
    assert got.nodes.tobytes() == want.tobytes()
    again = device_refit(nodes, r.root_leaf, r.items_out, new[order])
    assert again.rc == 0 and again.nodes.tobytes() == got.nodes.tobytes()


@pytest.mark.parametrize("case", [("sah", "uniform", 65), ("sah", "uniform", 1000), ("lbvh", "uniform", 65)],
                         ids=case_id)
def test_refit_of_a_4_wide_tree(case):
    """The collapse (rt_scene.cpp collapse_bvh4, as the library uploads it) of
    the device-built tree, refitted with arity 4: empty slots (entry -1) keep
    their empty boxes, every other slot is the restatement's."""
    r = built(case)
    wide = collapse(r.nodes[:r.n_nodes])
    assert wide.dtype == DNODE4 and (wide["entry"] == -1).any()
    new = second_boxes(case[1], case[2])[leaf_order(r)]
    got = device_refit(wide, 0, r.items_out, new)
    assert got.rc == 0 and got.guards == []
    assert got.nodes.tobytes() == numpy_refit(wide, new).tobytes()
    back = device_refit(got.nodes, 0, r.items_out, r.boxes[leaf_order(r)])
    assert back.rc == 0 and back.nodes.tobytes() == wide.tobytes()


def test_refit_refuses_what_it_cannot_do():
    r = built(("sah", "uniform", 65))
    nodes, boxes = r.nodes[:r.n_nodes], r.boxes[leaf_order(r)]
    short = device_refit(nodes, 0, r.items_out, boxes, temp_short=1)
    assert short.rc != 0 and short.guards == [] and (short.temp == FILL).all()
    assert short.nodes.tobytes() == nodes.tobytes()
    L = library()
    import torch
    buf = torch.full((GUARD,), FILL, dtype=torch.uint8, device="cuda")
    p, s = buf.data_ptr(), torch.cuda.current_stream().cuda_stream
    assert L.rtk_refit(p, 3, 1, 0, p, 2, p, p, GUARD, s) != 0  # no such arity
    assert L.rtk_refit(p, 2, -1, 0, p, 2, p, p, GUARD, s) != 0
    assert L.rtk_refit(p, 2, 1, -1, p, 2, p, p, GUARD, s) != 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == FILL).all()
