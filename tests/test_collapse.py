"""The 4-wide collapse, level by level (csrc/rt_collapse.h, rt_collapse.hip), without a GPU.

numpy_collapse() states the device collapse in NumPy -- per 4-wide level: (a)
every node of the level expanded from its source binary node on its own, (b) an
exclusive scan of the nodes' inner-child counts, (c) the inner slots numbered
next_level_base + rank + j and the next level's source list written -- and has
to give the bytes of test_refit.collapse(), the g++ build of rt_scene.cpp's
collapse_bvh4 (a BFS with one queue), on the builders' trees and on hand-made
ones.  tests/test_collapse_gpu.py holds rtk_collapse4 to the same bytes.

Also here: the two entry points of the rebuild are exported and refuse a null
scene (tests/test_rebuild_gpu.py has the rest).
"""
import ctypes as C

import numpy as np
import pytest

from rtx import abi
import bvh_reference as B
from test_refit import CASES, DNODE4, case_id, collapse, reference_tree


def leaf(first, count):
    return ~((first << 3) | count)


def binary_tree(entries):
    """DNODE records with the given entry pairs and distinct, nested-looking
    boxes: child k of node i is [i + k, i + k + w] per axis, w shrinking with i,
    so the areas differ and the larger child is the earlier node's."""
    nodes = np.zeros(len(entries), dtype=B.DNODE)
    for i, pair in enumerate(entries):
        for k, e in enumerate(pair):
            nodes["entry"][i, k] = e
            nodes["lo"][i, :, k] = np.float32(i + k)
            nodes["hi"][i, :, k] = np.float32(i + k) + np.float32(8.0 / (1 + i + k))
    return nodes


HAND_MADE = {
    # one binary node: two leaves, two empty slots
    "one-node": binary_tree([(leaf(0, 2), leaf(2, 1))]),
    # two: the inner child is opened, one empty slot
    "two-nodes": binary_tree([(leaf(0, 1), 1), (leaf(1, 2), leaf(3, 2))]),
    # three: both children opened, a full node
    "three-nodes": binary_tree([(1, 2), (leaf(0, 1), leaf(1, 1)), (leaf(2, 2), leaf(4, 1))]),
    # three in a chain: the second opening is of a child the first one brought in
    "three-chain": binary_tree([(leaf(0, 1), 1), (2, leaf(3, 1)), (leaf(1, 1), leaf(2, 1))]),
}


def half_area(lo, hi):
    x, y, z = (np.float64(hi[a]) - np.float64(lo[a]) for a in range(3))
    return x * y + y * z + z * x


def expand(nodes, src):
    """(a) for one node: [(lo, hi, entry)] of its 2 to 4 children, in slot order."""
    def child(i, k):
        return nodes["lo"][i, :, k].copy(), nodes["hi"][i, :, k].copy(), int(nodes["entry"][i, k])

    c = [child(src, 0), child(src, 1)]
    while len(c) < 4:
        pick, best = -1, np.float64(-1.0)
        for i, (lo, hi, e) in enumerate(c):
            if e >= 0 and half_area(lo, hi) > best:  # strict: the first maximum wins
                pick, best = i, half_area(lo, hi)
        if pick < 0:
            break
        opened = c[pick][2]
        c[pick:pick + 1] = [child(opened, 0), child(opened, 1)]  # in its place: the leaf order is kept
    return c


def numpy_collapse(nodes):
    """The DNODE4 records and the number of levels."""
    levels, out = 0, []
    src, base = np.zeros(1, dtype=np.int64), 0
    while len(src):
        levels += 1
        q = np.zeros(len(src), dtype=DNODE4)
        q["lo"], q["hi"], q["entry"] = np.inf, -np.inf, -1
        inner = np.zeros(len(src), dtype=np.int64)
        for t in range(len(src)):  # (a): no node reads what another one writes
            for i, (lo, hi, e) in enumerate(expand(nodes, int(src[t]))):
                q["lo"][t, :, i], q["hi"][t, :, i], q["entry"][t, i] = lo, hi, e
                inner[t] += e >= 0
        rank = np.cumsum(inner) - inner  # (b)
        next_base, nxt = base + len(src), np.zeros(int(inner.sum()), dtype=np.int64)
        for t in range(len(src)):  # (c)
            r = int(rank[t])
            for i in range(4):
                e = int(q["entry"][t, i])
                if e >= 0:
                    nxt[r], q["entry"][t, i] = e, next_base + r
                    r += 1
        out.append(q)
        src, base = nxt, next_base
    return np.concatenate(out), levels


def longest_path(wide):
    """Nodes on the longest root-to-node path of a 4-wide tree."""
    depth = np.zeros(len(wide), dtype=np.int64)
    depth[0] = 1
    for i in range(len(wide)):  # BFS order: a parent comes before its children
        for e in wide["entry"][i]:
            if e >= 0:
                assert e > i
                depth[e] = depth[i] + 1
    return int(depth.max())


def check(nodes):
    want = collapse(nodes)
    got, levels = numpy_collapse(nodes)
    assert got.dtype == want.dtype and len(got) == len(want)
    assert got.tobytes() == want.tobytes()
    assert levels == longest_path(want)
    return want


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_level_parallel_collapse_gives_the_host_bytes(case):
    nodes, _, n_nodes, _, root_leaf = reference_tree(*case)
    if n_nodes == 0:
        assert root_leaf > 0  # the whole world is one leaf: no tree to collapse
        return
    wide = check(nodes[:n_nodes])
    assert len(wide) <= n_nodes


def test_the_cases_reach_ties_and_unordered_trees():
    """What the parametrised test relies on: families whose child boxes have
    equal areas (the first maximum has to win on both sides), linear BVHs that
    are not in BFS order, and trees of several levels."""
    tied = 0
    for family in ("coincident", "line-x", "sheet"):
        nodes, _, n_nodes, _, _ = reference_tree("sah", family, 65)
        lo, hi = nodes["lo"][:n_nodes].astype(np.float64), nodes["hi"][:n_nodes].astype(np.float64)
        x, y, z = (hi[:, a, :] - lo[:, a, :] for a in range(3))
        area = x * y + y * z + z * x
        both_inner = (nodes["entry"][:n_nodes] >= 0).all(axis=1)
        tied += int((both_inner & (area[:, 0] == area[:, 1])).sum())
    assert tied > 0
    lb = reference_tree("lbvh", "uniform", 1000)[0]["entry"]
    assert ((lb >= 0) & (lb < np.arange(len(lb))[:, None])).any()
    assert numpy_collapse(reference_tree("sah", "uniform", 1000)[0])[1] >= 4


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_hand_made_trees(name):
    wide = check(HAND_MADE[name])
    empty = {"one-node": 2, "two-nodes": 1, "three-nodes": 0, "three-chain": 0}[name]
    assert len(wide) == 1 and int((wide["entry"][0] == -1).sum()) == empty
    gone = wide["entry"][0] == -1
    assert (wide["lo"][0][:, gone] == np.inf).all() and (wide["hi"][0][:, gone] == -np.inf).all()
    assert not wide["pad"].any()
    # leaf order kept: the leaves' first items ascend across the slots
    firsts = [(~int(e)) >> 3 for e in wide["entry"][0] if e < -1]
    assert firsts == sorted(firsts) and len(firsts) == 4 - empty


def test_the_rebuild_is_exported_and_refuses_a_null_scene():
    from rtx.lib import load
    assert "rt_scene_rebuild_bvh" in abi.EXPORTS and "rt_multi_rebuild_bvh" in abi.EXPORTS
    L = load()
    for f in (L.rt_scene_rebuild_bvh, L.rt_multi_rebuild_bvh):
        took = C.c_int32(7)
        assert f(None, C.byref(took)) == abi.RT_ERR_INVALID and took.value == 0
        assert f(None, None) == abi.RT_ERR_INVALID
        assert L.rt_last_error()
