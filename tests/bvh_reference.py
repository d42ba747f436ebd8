"""The device BVH builders, restated in NumPy, and a checker that trusts neither.

rt_bvh_build.hip (Morton / Karras linear BVH) and rt_bvh_sah.hip (binned SAH)
are compiled with -ffp-contract=off, so their fp64 and fp32 arithmetic can be
written down operation by operation: lbvh_reference() and sah_reference() give
the tree the kernels must give, byte for byte.  check_tree() and
check_sah_choice() derive nothing from either restatement: they state what any
correct tree over the items has to satisfy (so a rule misread by kernel and
restatement alike still fails), and the mutation tests of
tests/test_bvh_builders.py show that they can fail.

Layouts are rt_layout.h's: DNode (64 B: lo[3][2], hi[3][2], entry[2], pad[2]),
DItem (32 B, opaque to the builders).  FAMILIES / SHAPES / *_CASES are the inputs both
test files share.  A plain helper module: no HIP, no rtx.
"""
import bisect

import numpy as np

F32 = np.float32
DNODE = np.dtype([("lo", "<f4", (3, 2)), ("hi", "<f4", (3, 2)), ("entry", "<i4", (2,)), ("pad", "<i4", (2,))])
DITEM = np.dtype([("kind", "<i4"), ("idx", "<i4"), ("xf_first", "<i4"), ("xf_count", "<i4"), ("mat", "<i4"),
                  ("id", "<i4"), ("pad", "<i4", (2,))])
assert DNODE.itemsize == 64 and DITEM.itemsize == 32

RT_STACK_DEPTH = 32   # rt_layout.h
RT_FLAT_MAX = 8
SAH_BUDGET = RT_STACK_DEPTH - 2  # rt_api.cpp sah_stack_budget()
K_BINS = 16


# ---------------------------------------------------------------- margins
def f32_lo(x):
    """fp64 -> fp32 below x by at least |x| 2^-20 + 1e-7 (rt_scene.cpp f32_lo)."""
    x = np.asarray(x, dtype=np.float64)
    m = x - (np.abs(x) * 2.0 ** -20 + 1e-7)
    f = m.astype(F32)
    inward = f.astype(np.float64) > m
    return np.where(inward, np.nextafter(f, F32(-np.inf)), f).astype(F32)


def f32_hi(x):
    x = np.asarray(x, dtype=np.float64)
    m = x + (np.abs(x) * 2.0 ** -20 + 1e-7)
    f = m.astype(F32)
    inward = f.astype(np.float64) < m
    return np.where(inward, np.nextafter(f, F32(np.inf)), f).astype(F32)


def leaf_entry(first, count):
    return ~((first << 3) | count)


# ---------------------------------------------------------------- linear BVH
def _expand_bits(v):
    v = (v * 0x00010001) & 0xFF0000FF
    v = (v * 0x00000101) & 0x0F00F00F
    v = (v * 0x00000011) & 0xC30C30C3
    v = (v * 0x00000005) & 0x49249249
    return v


def morton_keys(boxes):
    """(morton30 << 32) | i per item, unsorted (rt_bvh_build.hip morton_keys with
    rt_scene.cpp's centroid bounds and rtk_build_lbvh's 1 / extent)."""
    boxes = np.asarray(boxes, dtype=np.float64)
    c = 0.5 * (boxes[:, :3] + boxes[:, 3:])
    lo, hi = c.min(axis=0), c.max(axis=0)
    ext = hi - lo
    sc = np.where(ext > 0, 1.0 / np.where(ext > 0, ext, 1.0), 0.0)
    u = (c - lo) * sc
    u = np.where(u > 0, np.where(u < 1, u, 1.0), 0.0)
    x = u * 1024.0
    q = np.where(x < 1023.0, x, 1023.0).astype(np.uint32).astype(np.uint64)
    m = (_expand_bits(q[:, 0]) << np.uint64(2)) | (_expand_bits(q[:, 1]) << np.uint64(1)) | _expand_bits(q[:, 2])
    return (m << np.uint64(32)) | np.arange(len(boxes), dtype=np.uint64)


def lbvh_reference(boxes):
    """nodes (n - 1 DNODE), item_order (the input index of each output item), depth."""
    boxes = np.asarray(boxes, dtype=np.float64)
    n = len(boxes)
    assert n >= 2
    keys = np.sort(morton_keys(boxes))
    order = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    key = [int(k) for k in keys]
    slo, shi = boxes[order, :3], boxes[order, 3:]
    nodes = np.zeros(n - 1, dtype=DNODE)
    nodes["entry"] = -1
    # top-down over [l, r]; the inner node over a range is numbered by the end
    # of the range that touches its parent's split (Karras 2012)
    todo = [(0, 0, n - 1, 1)]
    depth = 0
    while todo:
        me, l, r, dep = todo.pop()
        depth = max(depth, dep)
        top = (key[l] ^ key[r]).bit_length() - 1
        gamma = bisect.bisect_left(key, ((key[l] >> top) | 1) << top, l, r + 1) - 1
        for k, (a, b, idx) in enumerate(((l, gamma, gamma), (gamma + 1, r, gamma + 1))):
            nodes["lo"][me, :, k] = f32_lo(slo[a:b + 1].min(axis=0))
            nodes["hi"][me, :, k] = f32_hi(shi[a:b + 1].max(axis=0))
            if a == b:
                nodes["entry"][me, k] = leaf_entry(a, 1)
            else:
                nodes["entry"][me, k] = idx
                todo.append((idx, a, b, dep + 1))
    return nodes, order, depth


# ---------------------------------------------------------------- binned SAH
def _area32(lo, hi):
    x, y, z = hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]
    return F32(2.0) * ((x * y + y * z) + z * x)


def _bin_of(c, clo, scale):
    with np.errstate(invalid="ignore"):
        k = ((c - clo) * scale).astype(np.int32)  # truncates, as (int) does
    return np.clip(k, 0, K_BINS - 1)


def _plane_unions(lo, hi, bins):
    """Per plane k (the split before bin k; index 0 unused): the item count left
    of it and the unions of the item boxes on either side, from per-bin counts
    and unions as sah_decide keeps them.  min / max are exact, so the prefix and
    suffix unions are the unions of the items themselves."""
    cnt = np.bincount(bins, minlength=K_BINS)
    blo = np.full((K_BINS, 3), np.inf, dtype=lo.dtype)
    bhi = np.full((K_BINS, 3), -np.inf, dtype=lo.dtype)
    np.minimum.at(blo, bins, lo)
    np.maximum.at(bhi, bins, hi)
    pad_lo, pad_hi = blo[:1] * 0 + np.inf, bhi[:1] * 0 - np.inf
    llo = np.vstack([pad_lo, np.minimum.accumulate(blo, axis=0)[:-1]])
    lhi = np.vstack([pad_hi, np.maximum.accumulate(bhi, axis=0)[:-1]])
    rlo = np.minimum.accumulate(blo[::-1], axis=0)[::-1]
    rhi = np.maximum.accumulate(bhi[::-1], axis=0)[::-1]
    nl = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    return nl, llo, lhi, rlo, rhi


def _need(cnt):
    need = 0
    while (1 << need) < cnt:
        need += 1
    return need


def sah_reference(boxes, stack_budget=SAH_BUDGET, override=None, trace=None):
    """nodes (n_nodes DNODE, BFS order), item_order, n_nodes, depth, root_leaf:
    sah_prep / sah_decide / sah_apply in float32 with the kernels' operation
    order.  override {(level, slot): (axis, bin)} replaces the arg-min's choice
    at one node (for the mutation tests: a valid tree with a worse split); trace,
    a list, receives ((level, slot), (axis, bin) or None) per decided split."""
    boxes = np.asarray(boxes, dtype=np.float64)
    n = len(boxes)
    assert n >= 1
    override = override or {}
    blo, bhi = f32_lo(boxes[:, :3]), f32_hi(boxes[:, 3:])
    cen = F32(0.5) * (blo + bhi)
    refs = np.arange(n, dtype=np.int64)
    nodes = np.zeros(max(n - 1, 1), dtype=DNODE)
    root_leaf, level_base, lev = 0, 0, 0
    level = [(0, n, -1, 0, 0)]  # begin, count, parent, side, depth
    while level:
        # ---- sah_decide
        decisions = []
        for slot, (begin, cnt, parent, side, dep) in enumerate(level):
            idx = refs[begin:begin + cnt]
            c = cen[idx]
            clo, chi = c.min(axis=0), c.max(axis=0)
            if cnt <= 2 or (dep == 0 and cnt <= RT_FLAT_MAX):
                decisions.append(None)
                continue
            force = dep + _need(cnt) >= stack_budget
            ext = chi - clo
            scale = [F32(K_BINS) / ext[a] if ext[a] > F32(1e-12) else F32(0.0) for a in range(3)]
            bins = [_bin_of(c[:, a], clo[a], scale[a]) for a in range(3)]
            longest = (0 if ext[0] > ext[2] else 2) if ext[0] > ext[1] else (1 if ext[1] > ext[2] else 2)
            best, who = F32(np.inf), None
            for a in range(3):
                if scale[a] == 0:
                    continue
                nl, llo, lhi, rlo, rhi = _plane_unions(blo[idx], bhi[idx], bins[a])
                for k in range(K_BINS - 1, 0, -1):  # ties: lower axis, then higher k
                    if nl[k] == 0 or nl[k] == cnt:
                        continue
                    if not force:
                        cost = _area32(llo[k], lhi[k]) * F32(nl[k]) + _area32(rlo[k], rhi[k]) * F32(cnt - nl[k])
                    elif a == longest:
                        cost = F32(abs(2 * int(nl[k]) - cnt))
                    else:
                        continue
                    if cost < best:
                        best, who = cost, (a, k)
            if (lev, slot) in override:
                who = override[(lev, slot)]
            if trace is not None:
                trace.append(((lev, slot), who))
            if who is None:  # every centroid in one point: halve the range
                go_left = np.arange(cnt) < cnt // 2
            else:
                parent_area = _area32(blo[idx].min(axis=0), bhi[idx].max(axis=0))
                if not force and cnt <= 4 and parent_area > 0 and F32(1.0) + best / parent_area >= F32(cnt):
                    decisions.append(None)
                    continue
                go_left = bins[who[0]] < who[1]
            decisions.append(go_left)
        # ---- sah_apply
        nxt, rank = [], 0
        for (begin, cnt, parent, side, dep), go_left in zip(level, decisions):
            if go_left is None:
                if parent >= 0:
                    nodes["entry"][parent, side] = leaf_entry(begin, cnt)
                else:
                    root_leaf = cnt
                continue
            me = level_base + rank
            rank += 1
            if parent >= 0:
                nodes["entry"][parent, side] = me
            idx = refs[begin:begin + cnt]
            parts = (idx[go_left], idx[~go_left])  # stable
            refs[begin:begin + cnt] = np.concatenate(parts)
            for k in range(2):
                nodes["lo"][me, :, k] = blo[parts[k]].min(axis=0)
                nodes["hi"][me, :, k] = bhi[parts[k]].max(axis=0)
            nodes["entry"][me] = -1
            nl = len(parts[0])
            nxt.append((begin, nl, me, 0, dep + 1))
            nxt.append((begin + nl, cnt - nl, me, 1, dep + 1))
        level_base += rank
        level = nxt
        if level:
            lev += 1
    return nodes[:level_base].copy(), refs, level_base, lev, root_leaf


# ---------------------------------------------------------------- the checker
class TreeError(AssertionError):
    pass


def _fail(msg, *args):
    raise TreeError(msg % args)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _walk(nodes, n, n_nodes):
    """Inner nodes in an order that lists parents before children; per node and
    side the item range [first, first + count) below that entry."""
    seen = np.zeros(n_nodes, dtype=bool)
    cover = np.zeros(n, dtype=np.int64)
    seen[0] = True
    order, todo = [], [0]
    while todo:
        i = todo.pop()
        order.append(i)
        for k in range(2):
            e = int(nodes["entry"][i, k])
            if e == -1:
                _fail("node %d entry %d was never written (-1)", i, k)
            if e >= 0:
                if e >= n_nodes:
                    _fail("node %d entry %d = %d is not below n_nodes = %d", i, k, e, n_nodes)
                if seen[e]:
                    _fail("node %d is reached twice (again from node %d)", e, i)
                seen[e] = True
                todo.append(e)
            else:
                first, count = (~e) >> 3, (~e) & 7
                if not 1 <= count <= 4:
                    _fail("node %d entry %d: a leaf of %d items", i, k, count)
                if first + count > n:
                    _fail("node %d entry %d: leaf [%d, %d) past the %d items", i, k, first, first + count, n)
                cover[first:first + count] += 1
    if not seen.all():
        _fail("inner node %d is not reachable from the root", int(np.flatnonzero(~seen)[0]))
    if (cover != 1).any():
        j = int(np.flatnonzero(cover != 1)[0])
        _fail("item slot %d is in %d leaves", j, int(cover[j]))
    return order


def _sources(items_in, items_out):
    """src[i]: the input index of output item i, matched on all 32 bytes."""
    n = len(items_in)
    where = {items_in[j].tobytes(): j for j in range(n)}
    if len(where) != n:
        _fail("the input items are not distinct: the checker cannot tell them apart")
    src = np.empty(n, dtype=np.int64)
    for i in range(n):
        j = where.get(items_out[i].tobytes())
        if j is None:
            _fail("output item %d is none of the input items", i)
        src[i] = j
    if len(np.unique(src)) != n:
        _fail("the output items are not a permutation of the input (an item is there twice)")
    return src


def _subtrees(nodes, order, src, boxes):
    """Per inner node and side: first, count, depth below (inner nodes on the
    longest path under the entry) and the fp32 box the child must carry."""
    lo32, hi32 = f32_lo(boxes[:, :3])[src], f32_hi(boxes[:, 3:])[src]
    m = len(nodes)
    first = np.zeros((m, 2), dtype=np.int64)
    count = np.zeros((m, 2), dtype=np.int64)
    below = np.zeros((m, 2), dtype=np.int64)
    wlo = np.zeros((m, 3, 2), dtype=F32)
    whi = np.zeros((m, 3, 2), dtype=F32)
    for i in reversed(order):
        for k in range(2):
            e = int(nodes["entry"][i, k])
            if e >= 0:
                first[i, k] = first[e].min()
                count[i, k] = count[e].sum()
                below[i, k] = 1 + below[e].max()
                wlo[i, :, k] = wlo[e].min(axis=1)
                whi[i, :, k] = whi[e].max(axis=1)
            else:
                f, c = (~e) >> 3, (~e) & 7
                first[i, k], count[i, k] = f, c
                wlo[i, :, k] = lo32[f:f + c].min(axis=0)
                whi[i, :, k] = hi32[f:f + c].max(axis=0)
    return first, count, below, wlo, whi


def check_tree(boxes, items_in, nodes, items_out, n_nodes, depth, root_leaf):
    """Raises TreeError on the first violated invariant of a binary tree in the
    DNode / DItem layout over `boxes` (n x 6 fp64).  nodes holds at least
    n_nodes records; root_leaf is 0 for a builder that has no root leaf."""
    boxes = np.asarray(boxes, dtype=np.float64)
    n = len(boxes)
    if len(items_in) != n or len(items_out) != n:
        _fail("%d boxes, %d items in, %d items out", n, len(items_in), len(items_out))
    if n_nodes == 0:
        if not (root_leaf == n and n <= RT_FLAT_MAX):
            _fail("no inner node, but root_leaf = %d over %d items", root_leaf, n)
        if depth != 0:
            _fail("a root leaf of depth %d", depth)
        if items_out.tobytes() != items_in.tobytes():
            _fail("the root leaf's items are not in input order")
        return
    if root_leaf != 0:
        _fail("root_leaf = %d beside %d inner nodes", root_leaf, n_nodes)
    if not 1 <= n_nodes <= n - 1:
        _fail("%d inner nodes over %d items", n_nodes, n)
    nodes = nodes[:n_nodes]
    order = _walk(nodes, n, n_nodes)
    src = _sources(items_in, items_out)
    if nodes["pad"].any():
        _fail("node %d has a nonzero pad word", int(np.flatnonzero(nodes["pad"].any(axis=1))[0]))
    first, count, below, wlo, whi = _subtrees(nodes, order, src, boxes)
    for name, want, got in (("lo", wlo, nodes["lo"]), ("hi", whi, nodes["hi"])):
        bad = np.argwhere(_bits(want) != _bits(got))
        if len(bad):
            i, q, k = (int(v) for v in bad[0])
            _fail("node %d child %d: %s[%d] = %r, the items below it give %r", i, k, name, q,
                  float(got[i, q, k]), float(want[i, q, k]))
    # what the bit equality is for: every rounded item box strictly contains its
    # fp64 box, and a node box is the union of the rounded boxes below it
    if not ((f32_lo(boxes[:, :3]).astype(np.float64) < boxes[:, :3]).all()
            and (f32_hi(boxes[:, 3:]).astype(np.float64) > boxes[:, 3:]).all()):
        _fail("a rounded item box does not contain its fp64 box")
    true_depth = 1 + int(below[0].max())
    if depth != true_depth:
        _fail("reported depth %d, the longest root-to-leaf path has %d inner nodes", depth, true_depth)


def check_sah_choice(boxes, items_in, nodes, items_out, n_nodes, stack_budget=SAH_BUDGET, tol=1e-5):
    """Every unforced inner node of a (check_tree-clean) SAH tree took one of the
    binned candidates of its own item set -- a bin boundary on one axis separates
    left from right -- and no candidate is cheaper in float64 by more than tol
    (a cost is a sum of non-negative products of three singly rounded fp32
    differences: relative error < 16 2^-24 ~ 1e-6, and a decade).  One-sided,
    so ties need no exemption.  Returns the number of nodes judged."""
    boxes = np.asarray(boxes, dtype=np.float64)
    if n_nodes == 0:
        return 0
    nodes = nodes[:n_nodes]
    order = _walk(nodes, len(boxes), n_nodes)
    src = _sources(items_in, items_out)
    first, count, _, _, _ = _subtrees(nodes, order, src, boxes)
    for i in order:
        if first[i, 0] + count[i, 0] != first[i, 1]:
            _fail("node %d: its children's item ranges are not adjacent, left then right", i)
    lo32, hi32 = f32_lo(boxes[:, :3])[src], f32_hi(boxes[:, 3:])[src]
    cen = F32(0.5) * (lo32 + hi32)
    dep = {0: 0}
    judged = 0

    lo64, hi64 = lo32.astype(np.float64), hi32.astype(np.float64)

    def area(lo, hi):
        d = hi - lo
        return 2.0 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0])

    for i in order:
        for k in range(2):
            if nodes["entry"][i, k] >= 0:
                dep[int(nodes["entry"][i, k])] = dep[i] + 1
        b, cnt, nl = int(first[i, 0]), int(count[i].sum()), int(count[i, 0])
        if dep[i] + _need(cnt) >= stack_budget:
            continue  # forced: balanced by count, not by cost
        c = cen[b:b + cnt]
        clo, ext = c.min(axis=0), c.max(axis=0) - c.min(axis=0)
        costs, taken = [], None
        for a in range(3):
            if not ext[a] > F32(1e-12):
                continue
            bins = _bin_of(c[:, a], clo[a], F32(K_BINS) / ext[a])
            nleft, llo, lhi, rlo, rhi = _plane_unions(lo64[b:b + cnt], hi64[b:b + cnt], bins)
            for kk in range(1, K_BINS):
                if not 0 < nleft[kk] < cnt:
                    continue
                cost = area(llo[kk], lhi[kk]) * nleft[kk] + area(rlo[kk], rhi[kk]) * (cnt - nleft[kk])
                costs.append(cost)
                if nleft[kk] == nl and (bins[:nl] < kk).all():  # the output lists the left items first
                    taken = cost if taken is None else min(taken, cost)
        judged += 1
        if not costs:
            if nl != cnt // 2:
                _fail("node %d: no candidate plane, yet %d of %d items went left", i, nl, cnt)
            continue
        if taken is None:
            _fail("node %d: no bin boundary on any axis separates its left from its right items", i)
        if taken > (1.0 + tol) * min(costs):
            _fail("node %d: split cost %.9g, the cheapest candidate costs %.9g", i, taken, min(costs))
    return judged


# ---------------------------------------------------------------- inputs
def make_items(n):
    """id = i, and distinct bytes in every other field."""
    it = np.zeros(n, dtype=DITEM)
    i = np.arange(n, dtype=np.int64)
    for j, name in enumerate(("kind", "idx", "xf_first", "xf_count", "mat")):
        it[name] = (i * 8 + j + 1000003 * (j + 1)).astype(np.int32)
    it["id"] = i
    it["pad"][:, 0] = (0x5A000000 + i).astype(np.int32)
    it["pad"][:, 1] = (-1 - i).astype(np.int32)
    return it


def _centred(c, half):
    c = np.asarray(c, dtype=np.float64)
    half = np.broadcast_to(np.asarray(half, dtype=np.float64).reshape(len(c), -1), c.shape)
    return np.ascontiguousarray(np.hstack([c - half, c + half]))


def uniform(n, seed):
    """tests/test_device_bvh.py's random_spheres: small boxes in [-50, 50]^3 and the ground last."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-50, 50, size=(n, 3))
    r = rng.uniform(0.05, 0.4, size=n)
    c[-1], r[-1] = (0.0, -1000.0, 0.0), 940.0
    return _centred(c, r)


def far(n, seed):
    """tests/test_hit_identity.py's clouds: half-width 0.5, far from the origin."""
    rng = np.random.default_rng(seed)
    centre = np.where((np.arange(n) % 2 == 0)[:, None], (1000.0, 700.0, -1300.0), (30000.0, -20000.0, 10000.0))
    return _centred(centre + rng.uniform(-0.5, 0.5, size=(n, 3)), rng.uniform(0.004, 0.03, size=n))


def coincident(n, seed):
    return _centred(np.tile((1.5, -2.25, 3.0), (n, 1)), np.full(n, 0.3))


def _line(axis):
    def family(n, seed):
        rng = np.random.default_rng(seed)
        c = np.tile((0.25, -3.0, 7.5), (n, 1))
        c[:, axis] = rng.uniform(-50, 50, size=n)
        return _centred(c, np.full(n, 0.2))
    return family


def sheet(n, seed):
    """Unit cells of an integer grid in x and z around the origin, flat in y
    (lo == hi), every other one flat in x too: quads."""
    side = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    gx, gz = (i % side - side // 2).astype(np.float64), (i // side - side // 2).astype(np.float64)
    b = np.zeros((n, 6))
    b[:, 0], b[:, 2] = gx, gz
    b[:, 3], b[:, 5] = gx + (i % 2 == 0), gz + 1.0
    return b


def geometric(n, seed):
    """x = 1.5^(i mod 60): nearly every centroid in the first bin / Morton cell."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, size=(n, 3))
    c[:, 0] = 1.5 ** (np.arange(n) % 60)
    return _centred(c, np.full(n, 0.1))


FAMILIES = {"uniform": uniform, "far": far, "coincident": coincident, "line-x": _line(0), "line-z": _line(2),
            "sheet": sheet, "geometric": geometric}
UNIFORM_N = (2, 3, 8, 9, 63, 64, 65, 128, 129, 257, 1000, 4097)
# (family, n): both builders; the SAH builder also takes uniform at n = 1
SHAPES = [("uniform", n) for n in UNIFORM_N] + [(f, n) for f in FAMILIES if f != "uniform" for n in (65, 1000)] \
    + [("line-x", 3000)]
LBVH_CASES = list(SHAPES)
# (family, n, stack budget)
SAH_CASES = [("uniform", 1, SAH_BUDGET)] + [(f, n, SAH_BUDGET) for f, n in SHAPES] \
    + [(f, 1000, b) for f in ("uniform", "coincident", "geometric") for b in (8, 4)]
FORCED_CASES = [c for c in SAH_CASES if c[2] != SAH_BUDGET]


def case_boxes(family, n, seed=17):
    b = FAMILIES[family](n, seed)
    b.setflags(write=False)
    return b
