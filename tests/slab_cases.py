"""The claim behind the fp32 box tests of rt_path.h, stated once.

    A box that the exact slab test hits is never dropped: every fp32 form
    (slab<false>, slab<true>, slab_hit, slab_hit2, slab2_planes,
    slab_planes<2>, slab_planes<4>) passes it.  Visiting more boxes than the
    exact test is allowed.

Domain of the claim (also at kInvClamp in rt_path.h):

* o and d finite, with max_a |d_a| in [2^-64, 2^64].  The kernel's directions
  lie between Lambertian's 1e-8 guard and camera-ray lengths; measured, boxes
  start to be dropped when the whole direction is scaled below 2^-91 (entry
  distances beyond kInvClamp = 1e30).
* The box is finite fp32 with lo < hi on every axis.
* A ray lying exactly in a face plane (d_a == +-0 and o_a == lo_a or hi_a) is
  outside the "must pass" set: the clamped inverse treats +-0 as +-1e-30, so a
  ray leaving through the face it lies in gets far = -0 and the subtract form
  culls it.  Every box that reaches the kernel is padded outward by 2^-20
  relative + 1e-7 (rt_scene.cpp f32_lo / f32_hi, the device builders' copies
  of them, and mbox), so such a ray cannot touch a primitive.
* "Exact hit": with near / far the per-axis plane distances in long double,
  tl = max(near, tmin32), th = min(far, cl32), the box is hit when
  th - tl > 2^-40 max(|tl|, |th|).

make_cases() generates the rays and boxes, exact_interval() / exact_hit() are
the long-double test.  Used by tests/test_emulator.py (host build) and
tests/test_gpu_slab.py (gfx950 build); a plain helper module.
"""
import numpy as np

L = np.longdouble

# case kinds
RANDOM, ONFACE, PARALLEL, TINY, FAR, GRAZE, GRAZE2 = 0, 1, 2, 3, 4, 5, 6  # the original generator
ONE_COMPONENT = 7  # one direction component 1e-40 (fp32 denormal), 1e-50, 5e-324 (below fp32) or -0.0
INSIDE_TINY = 8    # origin strictly inside the box, one component +-1e-42
HUGE = 9           # one component 1e12 .. 1e60, the box long on that axis: the other axes decide
SCALED = 10        # whole direction scaled to max|d| in [2^k, 2^(k+1)), k in [-64, 63], or = 2^64
BELOW = 11         # whole direction scaled by 2^k, k in [-127, -92]: below the domain
FACEPLANE = 12     # origin on a face plane and that axis's direction +-0: outside the claim
N_KINDS = 13

# bit v / entry-distance column v of emu_slab_forms and devcheck_slab_forms
# (tests/native/slab_forms.h)
VARIANTS = ("slab<false>", "slab<true>", "slab_hit", "slab_hit2 child 0", "slab_hit2 child 1",
            "slab2_planes child 0", "slab2_planes child 1", "slab_planes<2> child 0",
            "slab_planes<2> child 1", "slab_planes<4> slot 0", "slab_planes<4> slot 1",
            "slab_planes<4> slot 2", "slab_planes<4> slot 3", "slab_planes<2> child 0, memory",
            "slab_planes<2> child 1, memory", "slab_planes<4> slot 0, memory",
            "slab_planes<4> slot 1, memory", "slab_planes<4> slot 2, memory",
            "slab_planes<4> slot 3, memory")
NV = len(VARIANTS)
FMA_FAMILY = tuple(range(1, NV))  # forms 2-7 of the list in slab_forms.h: all but the subtract form

TMIN32 = np.float32(0.001) - np.float32(1e-10)


def exact_interval(o, d, lo, hi):
    """Per case the exact (long double) parametric interval [near, far] of the
    ray inside the box, before the window [tmin32, cl32] is applied."""
    lo_l, hi_l, o_l, d_l = lo.astype(L), hi.astype(L), o.astype(L), d.astype(L)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t1 = (lo_l - o_l) / d_l
        t2 = (hi_l - o_l) / d_l
    near = np.minimum(t1, t2)
    far = np.maximum(t1, t2)
    zero = d_l == 0
    inside = (lo_l <= o_l) & (o_l <= hi_l)
    near = np.where(zero, np.where(inside, -np.inf, np.inf), near)
    far = np.where(zero, np.where(inside, np.inf, -np.inf), far)
    return near.max(axis=1), far.min(axis=1)


def exact_hit(o, d, lo, hi, tmin32, cl32):
    near, far = exact_interval(o, d, lo, hi)
    tl = np.maximum(near, tmin32.astype(L))
    th = np.minimum(far, cl32.astype(L))
    with np.errstate(invalid="ignore"):
        margin = L(2.0) ** -40 * np.maximum(np.abs(tl), np.abs(th))
        return th - tl > margin


def face_plane(o, d, lo, hi):
    """Rays lying exactly in one of the box's face planes."""
    return ((d == 0) & ((o == lo.astype(np.float64)) | (o == hi.astype(np.float64)))).any(axis=1)


def in_domain(o, d, lo, hi):
    md = np.abs(d).max(axis=1)
    ok = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (md >= 2.0**-64) & (md <= 2.0**64)
    ok &= np.isfinite(lo).all(axis=1) & np.isfinite(hi).all(axis=1) & (lo < hi).all(axis=1)
    return ok & ~face_plane(o, d, lo, hi)


def make_cases(n=400_000, seed=21):
    """n cases as a dict: o, d (float64 [n, 3]), lo, hi (float32 [n, 3]),
    tmin, cl (float32 [n]), kind (int [n]), domain (bool [n]: inside the
    domain of the claim), hit (bool [n]: the exact test hits)."""
    rng = np.random.default_rng(seed)
    scale = np.exp2(rng.uniform(-8, 20, n))[:, None]
    c = rng.uniform(-1, 1, (n, 3)) * scale
    ext = rng.uniform(1e-4, 1, (n, 3)) * scale * np.exp2(rng.uniform(-10, 0, n))[:, None]
    lo = (c - ext).astype(np.float32)
    hi = (c + ext).astype(np.float32)
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    o = rng.uniform(-3, 3, (n, 3)) * scale
    # the original seven kinds keep three quarters of the cases
    kind = np.where(rng.uniform(size=n) < 0.75, rng.integers(0, 7, n), rng.integers(7, N_KINDS, n))
    ax = rng.integers(0, 3, n)
    onface = kind == ONFACE                               # origin exactly on a face plane
    o[onface, ax[onface]] = lo[onface, ax[onface]]
    target = lo + rng.uniform(0, 1, (n, 3)) * (hi64 - lo)
    d = (target - o) * rng.uniform(0.5, 2, n)[:, None]
    par = kind == PARALLEL                                # axis-parallel rays
    d[par, ax[par]] = 0.0
    tiny = kind == TINY                                   # tiny components
    d[tiny, ax[tiny]] *= 1e-20
    big = kind == FAR                                     # far origin, small box
    o[big] = o[big] * 1e3
    d[big] = target[big] - o[big]
    graze = (kind == GRAZE) | (kind == GRAZE2)            # through a corner region, far origin:
    corner = np.where(rng.uniform(size=(n, 3)) < 0.5, lo, hi).astype(np.float64)  # tiny exact
    inward = np.where(corner == lo, 1.0, -1.0) * (hi64 - lo)                       # intervals, large
    target_g = corner + inward * np.exp2(rng.uniform(-30, -8, n))[:, None]         # |o / d|
    o[graze] = c[graze] + rng.uniform(-1, 1, (int(graze.sum()), 3)) * scale[graze] * 1e3
    d[graze] = target_g[graze] - o[graze]

    strictly_inside = lo64 + rng.uniform(0.05, 0.95, (n, 3)) * (hi64 - lo64)
    one = kind == ONE_COMPONENT   # half of them with that axis's origin inside the slab: hits exist
    ins = one & (rng.uniform(size=n) < 0.5)
    o[ins, ax[ins]] = strictly_inside[ins, ax[ins]]
    vals = np.array([1e-40, -1e-40, 1e-50, -1e-50, 5e-324, -5e-324, -0.0])
    d[one, ax[one]] = rng.choice(vals, int(one.sum()))
    it = kind == INSIDE_TINY
    o[it] = strictly_inside[it]
    d[it] = rng.uniform(-1, 1, (int(it.sum()), 3)) * scale[it]
    d[it, ax[it]] = rng.choice([1e-42, -1e-42], int(it.sum()))
    hg = kind == HUGE             # the box spans |t| <= 1..4 on the huge axis (up to fp32's range)
    mag = 10.0 ** rng.uniform(12, 60, n)
    half = np.minimum(mag * rng.uniform(1, 4, n), 3e38).astype(np.float32)
    lo[hg, ax[hg]] = -half[hg]
    hi[hg, ax[hg]] = half[hg]
    o[hg, ax[hg]] = rng.uniform(-0.5, 0.5, int(hg.sum())) * half[hg]
    d[hg, ax[hg]] = mag[hg] * rng.choice([-1.0, 1.0], int(hg.sum()))
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    for sel, k0, k1 in ((kind == SCALED, -64, 65), (kind == BELOW, -127, -91)):
        m = int(sel.sum())
        k = rng.integers(k0, k1, m)
        unit = d[sel] / np.exp2(np.floor(np.log2(np.abs(d[sel]).max(axis=1))))[:, None]  # max|d| in [1, 2)
        top = k == 64                                     # max|d| = 2^64 exactly, the domain's end
        unit[top] /= np.abs(unit[top]).max(axis=1)[:, None]
        d[sel] = unit * np.exp2(k.astype(np.float64))[:, None]
    fp = kind == FACEPLANE
    o[fp, ax[fp]] = np.where(rng.uniform(size=int(fp.sum())) < 0.5, lo64[fp, ax[fp]], hi64[fp, ax[fp]])
    d[fp, ax[fp]] = rng.choice([0.0, -0.0], int(fp.sum()))

    # window: tmin32 as the kernel's (a tiny one for half of the huge-component
    # rays, whose intervals lie next to 0); cl32 +inf (a ray's first box tests),
    # a random finite bound, or a finite bound before / inside / after the
    # exact interval
    tmin = np.full(n, TMIN32, dtype=np.float32)
    tmin[hg & (rng.uniform(size=n) < 0.5)] = np.float32(1e-30)
    cl = np.where(rng.uniform(size=n) < 0.5, np.inf, rng.uniform(0.1, 3, n))
    near, far = exact_interval(o, d, lo, hi)
    a = np.maximum(near, tmin.astype(L))
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.isfinite(a) & np.isfinite(far) & (far > a) & (far < 1e37) & (a > 0)
        pick = rng.integers(0, 6, n)                      # 0..2: keep the above
        u = rng.uniform(0.02, 0.98, n)
        a64, f64 = a.astype(np.float64), far.astype(np.float64)
        before = a64 * (0.3 + 0.69 * u)
        inside = a64 + u * (f64 - a64)
        after = f64 * (1.01 + 2 * u)
    cl = np.where(ok & (pick == 3), before, cl)
    cl = np.where(ok & (pick == 4), inside, cl)
    cl = np.where(ok & (pick == 5), after, cl)
    with np.errstate(over="ignore"):
        cl = cl.astype(np.float32)

    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    lo, hi = np.ascontiguousarray(lo), np.ascontiguousarray(hi)
    return {"o": o, "d": d, "lo": lo, "hi": hi, "tmin": tmin, "cl": cl, "kind": kind,
            "domain": in_domain(o, d, lo, hi), "hit": exact_hit(o, d, lo, hi, tmin, cl)}


def run_forms(fn, cs):
    """Call emu_slab_forms / devcheck_slab_forms (a ctypes function) on the
    cases: (verdict uint32 [n], tl float32 [n, NV])."""
    import ctypes as C
    n = len(cs["kind"])
    PD, PF = C.POINTER(C.c_double), C.POINTER(C.c_float)
    fn.argtypes = [PD, PD, PF, PF, PF, PF, C.c_int, C.POINTER(C.c_uint32), PF]
    fn.restype = C.c_int
    verdict = np.zeros(n, dtype=np.uint32)
    tl = np.zeros((n, NV), dtype=np.float32)
    rc = fn(cs["o"].ctypes.data_as(PD), cs["d"].ctypes.data_as(PD), cs["lo"].ctypes.data_as(PF),
            cs["hi"].ctypes.data_as(PF), cs["tmin"].ctypes.data_as(PF), cs["cl"].ctypes.data_as(PF), n,
            verdict.ctypes.data_as(C.POINTER(C.c_uint32)), tl.ctypes.data_as(PF))
    assert rc == 0, rc
    return verdict, tl


def check_forms(cs, verdict, tl, label):
    """The assertions both builds share; prints the counts that are reported
    but not asserted.  Returns them as a dict."""
    kind, dom, hit = cs["kind"], cs["domain"], cs["hit"]
    must = dom & hit
    assert must.sum() > len(kind) // 4                   # the cases do exercise hits
    for k in range(N_KINDS):                             # ... of every kind inside the domain
        if k not in (BELOW, FACEPLANE):
            assert (must & (kind == k)).sum() > 100, k
    passed = ((verdict[:, None] >> np.arange(NV)[None, :]) & 1).astype(bool)
    # 1. no form drops an exact hit inside the domain
    drops = {VARIANTS[v]: int((must & ~passed[:, v]).sum()) for v in range(NV)}
    for v in range(NV):
        dropped = must & ~passed[:, v]
        assert not dropped.any(), "%s: dropped boxes per form %s; %s e.g. kind %d o=%s d=%s lo=%s hi=%s tmin=%s cl=%s" % (
            label, {k: n for k, n in drops.items() if n}, VARIANTS[v], kind[dropped][0], cs["o"][dropped][0],
            cs["d"][dropped][0], cs["lo"][dropped][0], cs["hi"][dropped][0], cs["tmin"][dropped][0],
            cs["cl"][dropped][0])
    # 2. the FMA family agrees value for value: verdicts and entry-distance
    # bits, every child slot, every case (all operands here are finite but
    # cl32 = +inf, and no form makes a NaN of them, so nothing is excluded --
    # the rays below the domain and in a face plane are included)
    assert not np.isnan(tl).any()
    f0 = FMA_FAMILY[0]
    bits = tl.view(np.uint32)
    for v in FMA_FAMILY[1:]:
        diff = passed[:, v] != passed[:, f0]
        assert not diff.any(), "%s: verdicts of %s and %s differ on %d cases, e.g. kind %d" % (
            label, VARIANTS[v], VARIANTS[f0], diff.sum(), kind[diff][0])
        # slab<true> returns +inf for a miss; the others return the distance
        diff = (bits[:, v] != bits[:, f0]) & (passed[:, f0] if f0 == 1 else True)
        assert not diff.any(), "%s: entry distances of %s and %s differ on %d cases, e.g. %s vs %s" % (
            label, VARIANTS[v], VARIANTS[f0], diff.sum(), tl[diff, v][0], tl[diff, f0][0])
    for v in FMA_FAMILY[2:]:  # among the forms that return the distance on a miss too
        diff = bits[:, v] != bits[:, 2]
        assert not diff.any(), "%s: entry distances of %s and slab_hit differ on %d cases" % (
            label, VARIANTS[v], diff.sum())
    # 3. not vacuous: most exact misses inside the domain are culled, per form
    miss = dom & ~hit
    for v in range(NV):
        assert (~passed[miss, v]).mean() > 0.5, (label, VARIANTS[v])
    # reported, not asserted: rays outside the domain
    counts = {}
    for name, sel in (("face-plane", kind == FACEPLANE), ("below-domain", kind == BELOW),
                      ("above-domain (huge component)", (kind == HUGE) & ~dom)):
        h = sel & hit
        counts[name] = (int(sel.sum()), int(h.sum()), int((h & passed[:, 0]).sum()), int((h & passed[:, 1]).sum()))
        print("%s: %s rays: %d cases, %d exact hits, passed by the subtract form %d, by the FMA family %d"
              % ((label, name) + counts[name]))
    return counts
