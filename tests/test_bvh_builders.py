"""The device BVH builders' NumPy restatements and the tree checker, on the host.

tests/bvh_reference.py restates rt_bvh_build.hip (linear BVH) and
rt_bvh_sah.hip (binned SAH); tests/test_bvh_builders_gpu.py holds the kernels to
those restatements bit for bit.  Here, without a GPU: the restatements' trees
satisfy every invariant of check_tree / check_sah_choice on the inputs where
such builders break (n at 2, 3, 8, 9 and around the 64-lane chunks, coincident
centroids, collinear and planar sets, zero-thickness boxes, coordinates on both
sides of zero, large offsets, forced balanced splits), the checker rejects
each way a tree can be subtly wrong, and f32_lo / f32_hi keep their margins.
"""
from fractions import Fraction

import numpy as np
import pytest

import bvh_reference as B


def _id(case):
    return "-".join(str(v) for v in case)


def built(builder, family, n, budget=B.SAH_BUDGET):
    """(boxes, items_in, nodes, items_out, n_nodes, depth, root_leaf) of a restatement."""
    boxes, items = B.case_boxes(family, n), B.make_items(n)
    if builder == "sah":
        nodes, order, n_nodes, depth, root_leaf = B.sah_reference(boxes, budget)
    else:
        nodes, order, depth = B.lbvh_reference(boxes)
        n_nodes, root_leaf = n - 1, 0
    return boxes, items, nodes, items[order], n_nodes, depth, root_leaf


@pytest.mark.parametrize("case", B.LBVH_CASES, ids=_id)
def test_lbvh_restatement_builds_a_correct_tree(case):
    t = built("lbvh", *case)
    B.check_tree(*t)
    assert (t[3]["id"] == np.sort(B.morton_keys(t[0])) & np.uint64(0xFFFFFFFF)).all()


@pytest.mark.parametrize("case", B.SAH_CASES, ids=_id)
def test_sah_restatement_builds_a_correct_tree_with_cheapest_splits(case):
    boxes, items, nodes, out, n_nodes, depth, root_leaf = built("sah", *case)
    B.check_tree(boxes, items, nodes, out, n_nodes, depth, root_leaf)
    judged = B.check_sah_choice(boxes, items, nodes, out, n_nodes, case[2])
    n = case[1]
    assert (n_nodes == 0) == (n <= B.RT_FLAT_MAX) and root_leaf == (n if n <= B.RT_FLAT_MAX else 0)
    if case[2] == B.SAH_BUDGET:
        assert judged == n_nodes  # nothing is forced at the library's budget
    elif case[2] == 4:
        assert judged == 0        # 4 levels for 1000 items: forced from the root down


def test_families_hold_the_edges_they_are_named_for():
    for name, n in B.SHAPES:
        b = B.case_boxes(name, n)
        assert b.shape == (n, 6) and np.isfinite(b).all() and (b[:, :3] <= b[:, 3:]).all()
    c = lambda b: 0.5 * (b[:, :3] + b[:, 3:])
    assert (np.ptp(c(B.case_boxes("coincident", 65)), axis=0) == 0).all()
    assert (np.ptp(c(B.case_boxes("line-x", 65)), axis=0) > 0).tolist() == [True, False, False]
    assert (np.ptp(c(B.case_boxes("line-z", 65)), axis=0) > 0).tolist() == [False, False, True]
    s = B.case_boxes("sheet", 1000)
    assert (s[:, 1] == s[:, 4]).all() and (s[1::2, 0] == s[1::2, 3]).all()
    assert s[:, 0].min() < 0 < s[:, 0].max() and (s[:, 0] == 0).any() and (s[:, 2] == 0).any()
    k = np.sort(B.morton_keys(B.case_boxes("line-x", 3000))) >> np.uint64(32)
    assert len(np.unique(k)) < 3000 * 0.4  # many items share a Morton cell
    assert np.abs(B.case_boxes("far", 65)).max() > 2.9e4
    items = B.make_items(1000)
    assert (items["id"] == np.arange(1000)).all()
    for f in ("kind", "idx", "xf_first", "xf_count", "mat"):
        assert len(np.unique(items[f])) == 1000
    assert len(np.unique(items["pad"], axis=0)) == 1000


# ---------------------------------------------------------------- the checker can fail
def _a_leaf(nodes):
    i, k = np.argwhere(nodes["entry"] < -1)[-1]
    return int(i), int(k)


def _inward(t):
    t[2]["lo"][3, 1, 0] = np.nextafter(t[2]["lo"][3, 1, 0], np.float32(np.inf))


def _inward_hi(t):
    t[2]["hi"][0, 2, 1] = np.nextafter(t[2]["hi"][0, 2, 1], np.float32(-np.inf))


def _swap_in_node(t):
    t[2]["entry"][0] = t[2]["entry"][0][::-1].copy()


def _swap_across(t):
    i, k = _a_leaf(t[2])
    t[2]["entry"][i, k], t[2]["entry"][0, 0] = t[2]["entry"][0, 0], t[2]["entry"][i, k]


def _unwritten(t):
    i, k = _a_leaf(t[2])
    t[2]["entry"][i, k] = -1


def _unlinked(t):
    t[2]["entry"][0, 1] = t[2]["entry"][0, 0]


def _duplicate(t):
    t[3][5] = t[3][6]


def _foreign_item(t):
    t[3]["pad"][7, 1] ^= 1


def _wrong_item(t):
    t[3][[5, 100]] = t[3][[100, 5]]


def _shorten(t):
    i, k = _a_leaf(t[2])
    t[2]["entry"][i, k] += 1  # ~(first << 3 | count): one item fewer


def _shallow(t):
    t[5] -= 1


def _pad(t):
    t[2]["pad"][7, 1] = 1


def _past_the_nodes(t):
    t[2]["entry"][1, 0] = t[4]


MUTATIONS = [_inward, _inward_hi, _swap_in_node, _swap_across, _unwritten, _unlinked, _duplicate, _foreign_item,
             _wrong_item, _shorten, _shallow, _pad, _past_the_nodes]


@pytest.fixture(scope="module")
def trees():
    return {b: built(b, "uniform", 129) for b in ("lbvh", "sah")}


@pytest.mark.parametrize("mutate", MUTATIONS, ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("builder", ["lbvh", "sah"])
def test_check_tree_rejects(trees, builder, mutate):
    t = [v.copy() if isinstance(v, np.ndarray) else v for v in trees[builder]]
    B.check_tree(*t)
    mutate(t)
    with pytest.raises(B.TreeError):
        B.check_tree(*t)


def test_check_tree_rejects_a_reordered_root_leaf():
    t = [v.copy() if isinstance(v, np.ndarray) else v for v in built("sah", "uniform", 8)]
    B.check_tree(*t)
    t[3][[0, 1]] = t[3][[1, 0]]
    with pytest.raises(B.TreeError):
        B.check_tree(*t)
    with pytest.raises(B.TreeError):
        B.check_tree(*built("sah", "uniform", 8)[:6], 7)


def _items_under(nodes, entry):
    if entry < 0:
        return (~int(entry)) & 7
    return sum(_items_under(nodes, e) for e in nodes["entry"][entry])


def _root_cost(boxes, nodes, order):
    """float64 cost of the root's split, from the items on either side."""
    nl = _items_under(nodes, nodes["entry"][0, 0])
    lo, hi = B.f32_lo(boxes[:, :3])[order].astype(np.float64), B.f32_hi(boxes[:, 3:])[order].astype(np.float64)
    cost = 0.0
    for s in (slice(0, nl), slice(nl, None)):
        d = hi[s].max(axis=0) - lo[s].min(axis=0)
        cost += 2.0 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0]) * len(lo[s])
    return cost


def test_check_sah_choice_rejects_a_split_one_bin_over():
    """The root of line-x-129 (some eight items per bin) split one bin beside the
    arg-min's plane: still a correct tree, but dearer than the cheapest candidate
    by more than 1e-5."""
    boxes, items = B.case_boxes("line-x", 129), B.make_items(129)
    trace = []
    nodes, order, n_nodes, depth, root_leaf = B.sah_reference(boxes, trace=trace)
    assert trace[0][0] == (0, 0)
    axis, k = trace[0][1]
    base = _root_cost(boxes, nodes, order)
    B.check_sah_choice(boxes, items, nodes, items[order], n_nodes)
    moved = 0
    for k2 in (k - 1, k + 1):
        if not 1 <= k2 < B.K_BINS:
            continue
        nodes, order, n_nodes, depth, root_leaf = B.sah_reference(boxes, override={(0, 0): (axis, k2)})
        assert _root_cost(boxes, nodes, order) > (1 + 1e-5) * base, "an empty bin beside the plane?"
        B.check_tree(boxes, items, nodes, items[order], n_nodes, depth, root_leaf)
        with pytest.raises(B.TreeError, match="node 0: split cost"):
            B.check_sah_choice(boxes, items, nodes, items[order], n_nodes)
        moved += 1
    assert moved == 2


def test_check_sah_choice_rejects_a_split_no_plane_makes():
    """The boxes of the first and the last output item change places under an
    unchanged tree: its root now has an item from the far end on either side,
    which no bin boundary separates."""
    boxes, items, nodes, out, n_nodes, depth, root_leaf = built("sah", "line-x", 65)
    B.check_sah_choice(boxes, items, nodes, out, n_nodes)
    swapped = boxes.copy()
    a, b = out["id"][0], out["id"][64]
    swapped[[a, b]] = swapped[[b, a]]  # the same tree over boxes that now sit on the wrong sides
    with pytest.raises(B.TreeError):
        B.check_sah_choice(swapped, items, nodes, out, n_nodes)


# ---------------------------------------------------------------- margins
def test_rounded_planes_keep_their_margins():
    """f32_lo(x) < x < f32_hi(x), both at least |x| 2^-20 + 1e-7 away (exactly:
    in rational arithmetic on the doubles) -- the distance the fp32 slab test's
    error analysis (tests/slab_cases.py) takes for granted."""
    rng = np.random.default_rng(5)
    xs = [0.0, 1e-7, -1e-7, 1.0, -1.0, 3e4, -3e4, 1e6, -1e6]
    xs += list(rng.uniform(-1, 1, 500) * 10.0 ** rng.uniform(-9, 6, 500)) + list(rng.uniform(-5e4, 5e4, 500))
    lo, hi = B.f32_lo(np.array(xs)), B.f32_hi(np.array(xs))
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    for x, l, h in zip(xs, lo, hi):
        margin = abs(Fraction(x)) / 2 ** 20 + Fraction(1e-7)
        assert float(l) < x < float(h)
        assert Fraction(x) - Fraction(float(l)) >= margin, x
        assert Fraction(float(h)) - Fraction(x) >= margin, x
