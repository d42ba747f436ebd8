"""rtk_collapse4 (rt_collapse.hip) over torch buffers, read back byte by byte.

The binary trees are tests/test_collapse.py's: the builders' restatements over
tests/test_refit.py's cases and the hand-made ones.  Output and temp are
pre-filled with 0xCD with 4 KiB guards behind them (tests/test_refit_gpu.py's
harness): the written records have to be the host collapse's bytes, the counts
right, everything past them untouched, the input unchanged, and a second run
the same.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bvh_reference as B
from test_bvh_builders_gpu import FILL, GUARD, library as builders_library
from test_collapse import HAND_MADE, longest_path
from test_refit import CASES, DNODE4, case_id, collapse, reference_tree

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def library():
    L = builders_library()
    vp = C.c_void_p
    L.rtk_collapse4_temp_bytes.argtypes, L.rtk_collapse4_temp_bytes.restype = [C.c_int], C.c_size_t
    L.rtk_collapse4.argtypes = [vp, C.c_int, vp, vp, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), vp]
    L.rtk_collapse4.restype = C.c_int
    return L


class Collapsed:
    """One rtk_collapse4, downloaded: rc, n_nodes4, levels, out (all n records),
    temp, the input as it is afterwards, and `guards`, the regions written
    outside their range."""


def device_collapse(nodes, temp_short=0, claim=None):
    import torch
    L = library()
    n = len(nodes)
    temp_bytes = int(L.rtk_collapse4_temp_bytes(n))
    sizes = {"out": n * DNODE4.itemsize, "temp": temp_bytes}
    bufs = {k: torch.full((v + GUARD,), FILL, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
    d_in = torch.from_numpy(np.ascontiguousarray(nodes).view(np.uint8).copy()).cuda()
    stream = torch.cuda.current_stream()
    n4, levels = C.c_int(-7), C.c_int(-7)
    r = Collapsed()
    r.rc = L.rtk_collapse4(d_in.data_ptr(), n if claim is None else claim, bufs["out"].data_ptr(),
                           bufs["temp"].data_ptr(), temp_bytes - temp_short, C.byref(n4), C.byref(levels),
                           stream.cuda_stream)
    stream.synchronize()
    host = {k: v.cpu().numpy() for k, v in bufs.items()}
    r.guards = [k for k, size in sizes.items() if (host[k][size:] != FILL).any()]
    r.out = host["out"][:sizes["out"]].view(DNODE4)
    r.temp = host["temp"][:temp_bytes]
    r.input = d_in.cpu().numpy().view(B.DNODE)
    r.n_nodes4, r.levels = n4.value, levels.value
    return r


def check(nodes):
    want = collapse(nodes)
    got = device_collapse(nodes)
    assert got.rc == 0 and got.guards == []
    assert got.n_nodes4 == len(want) and got.levels == longest_path(want)
    a, b = got.out[:len(want)], want
    for f in ("entry", "pad"):
        assert np.array_equal(a[f], b[f]), f
    for f in ("lo", "hi"):
        bad = np.argwhere(a[f].view(np.uint32) != b[f].view(np.uint32))
        assert len(bad) == 0, "%s%s: device %r, host %r (%d words differ)" % (
            f, tuple(bad[0]), a[f][tuple(bad[0])], b[f][tuple(bad[0])], len(bad))
    assert a.tobytes() == b.tobytes()
    assert (got.out[len(want):].view(np.uint8) == FILL).all(), "records past n_nodes4 were written"
    assert got.input.tobytes() == np.ascontiguousarray(nodes).tobytes()
    again = device_collapse(nodes)
    assert again.rc == 0 and again.out.tobytes() == got.out.tobytes()
    assert (again.n_nodes4, again.levels) == (got.n_nodes4, got.levels)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_device_collapse_gives_the_host_bytes(case):
    nodes, _, n_nodes, _, root_leaf = reference_tree(*case)
    if n_nodes == 0:
        assert root_leaf > 0  # one leaf: the library never collapses it
        return
    check(nodes[:n_nodes])


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_hand_made_trees(name):
    check(HAND_MADE[name])


def test_collapse_refuses_what_it_cannot_do():
    nodes = reference_tree("sah", "uniform", 65)[0]
    nodes = nodes[:reference_tree("sah", "uniform", 65)[2]]
    for r in (device_collapse(nodes, temp_short=1), device_collapse(nodes, claim=0), device_collapse(nodes, claim=-3)):
        assert r.rc != 0 and r.guards == []
        assert (r.out.view(np.uint8) == FILL).all() and (r.temp == FILL).all()
        assert r.input.tobytes() == nodes.tobytes()
        assert (r.n_nodes4, r.levels) == (-7, -7)
    # the output may not be the input
    import torch
    L = library()
    n = len(nodes)
    buf = torch.full((n * DNODE4.itemsize,), FILL, dtype=torch.uint8, device="cuda")
    temp = torch.full((int(L.rtk_collapse4_temp_bytes(n)),), FILL, dtype=torch.uint8, device="cuda")
    n4, levels = C.c_int(-7), C.c_int(-7)
    rc = L.rtk_collapse4(buf.data_ptr(), n, buf.data_ptr(), temp.data_ptr(), temp.numel(), C.byref(n4),
                         C.byref(levels), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and (buf.cpu().numpy() == FILL).all() and (temp.cpu().numpy() == FILL).all()
