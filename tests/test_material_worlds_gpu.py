"""Every render instance of rt_kernel.hip on the material worlds
(tests/material_worlds.py): fuzzy metal, a mirror, nested checkers, a checker
on a medium's phase function and on the lamp, a second dielectric, a moving
sphere and the lens, in each of the 32 feature sets and the 16 four-wide
ones; a second Perlin table; and the counted (STATS) twin of each instance
against the counted host build of the same source.

tests/test_material_worlds.py holds the host build of the kernel source to
the oracle on the same worlds at 1e-10.  What fails here and passes there is
gfx950 code generation or a device-only path."""
import ctypes as C

import numpy as np
import pytest

from rtx import abi
from rtx.render import Renderer
from rtx.scene import load_scene
import material_worlds as MW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emu():
    return MW.load_emu()


BAR = 1e-4
# (feature set, bvh_arity): the 32 instances, then the 16 four-wide ones
INSTANCES = [(F, 0) for F in range(32)] + [(F, 4) for F in range(16)]
IDS = ["F%d%s" % (F, "-bvh4" if a else "") for F, a in INSTANCES]


def want_features(F, arity):
    # a metal is in every world: RT_FEAT_DIFFUSE is never set
    return F | (abi.RT_FEAT_BVH4 if arity == 4 else 0)


def against_oracle(what, gpu, ref):
    d = np.abs(np.nan_to_num(gpu) - np.nan_to_num(ref))
    print("%s: max |gpu - oracle| = %.3g" % (what, d.max()))
    assert np.array_equal(np.isnan(gpu), np.isnan(ref)), what
    assert not (d > BAR).any(), "%s: %d channels off, max %g" % (what, (d > BAR).sum(), d.max())


@pytest.mark.parametrize("F,arity", INSTANCES, ids=IDS)
def test_each_instance_on_all_materials(F, arity):
    doc = MW.material_scene(F)
    S = load_scene(doc)
    S.bvh_arity = arity
    _, f = MW.sized(S)
    with Renderer(S) as R:
        assert R.info()["features"] == want_features(F, arity)
        gpu = R.render(f, seed=MW.SEED)
    against_oracle("instance F=%d arity %d" % (F, arity), gpu, MW.oracle_frame(F, doc))


@pytest.mark.parametrize("F", MW.TWO_TABLE_F)
def test_second_perlin_table(F):
    """Two tables stay in memory (rt_lds_plan.cpp): tex_value reads
    S.perlin[T.perlin] with T.perlin = 1 on the floor."""
    doc = MW.two_table_scene(F)
    S = load_scene(doc)
    _, f = MW.sized(S)
    with Renderer(S) as R:
        info = R.info()
        assert info["features"] == F and info["lds_perlin"] == 0
        gpu = R.render(f, seed=MW.SEED)
    against_oracle("two tables, F=%d" % F, gpu, MW.oracle_frame(("two", F), doc))


def test_one_perlin_table_read_from_memory():
    """The same path with the one table of F = 8 kept out of LDS by the tuning."""
    doc = MW.material_scene(8)
    S = load_scene(doc)
    _, f = MW.sized(S)
    with Renderer(S) as R:
        assert R.info()["lds_perlin"] == 1
    with Renderer(S, tuning={"no_lds_perlin": 1}) as R:
        info = R.info()
        assert info["features"] == 8 and info["lds_perlin"] == 0
        gpu = R.render(f, seed=MW.SEED)
    against_oracle("one table in memory, F=8", gpu, MW.oracle_frame(8, doc))


# what the paths alone decide: equal in every instance
PATH_COUNTERS = ("samples", "segments", "shade_events", "other_tests", "light_tests",
                 "noise_evals", "medium_box_tests", "medium_box_deferred")
# what the walk decides: equal in a flat world, one-sided in a tree
WALK_COUNTERS = ("node_visits", "sphere_tests", "quad_tests")


def host_stats(emu, S, f, features):
    d = S.desc()
    p = abi.RenderParams()
    p.seed, p.sample_count, p.output = MW.SEED, -1, abi.RT_OUT_SCALED
    st = abi.PathStats()
    out = np.zeros((f.image_height, f.image_width, 3))
    assert emu.emu_render_stats(C.byref(d), C.byref(f), C.byref(p), features,
                                out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st)) == 0
    return {k: getattr(st, k) for k, _ in abi.PathStats._fields_}, out


@pytest.mark.parametrize("F,arity", INSTANCES, ids=IDS)
def test_counted_instances_count_what_the_paths_do(emu, F, arity):
    """The counted instance against segment<true, F> on the host, one lane at a
    time (tests/native emu_render_stats).

    PATH_COUNTERS depend on the paths alone (media are tested after the walk,
    against the final distance: trace_tail) and must be equal: a discrete
    decision differs between the g++ and the gfx950 build only on an exact tie.

    In a flat world every item is tested on every segment, so the walk's
    counters are equal too and no node is visited.  In a tree they are
    one-sided.  A lane of a wave that holds its first leaf keeps walking while
    a wave mate still walks (wave_none(ln == 0)); the host's single lane tests
    that leaf at once.  Both visit nodes and leaves in the same depth-first,
    near-first order, which no bound changes, and at each node the device
    lane's closest-hit bound comes from a prefix of the leaves the host lane
    has tested by then.  Its bound is therefore never tighter: it visits every
    node and tests every leaf item the host does, and possibly more.

    The wave-level counters bound the lane-level ones by the wave's 64 lanes:
    these are the ratios bench.py --full reports.  model_trace_pair_max sums
    max over lanes of (a + b) per pair of trips and model_trace_max sums
    max a + max b, so pair <= single <= 2 * pair (max(a + b) >= each max)."""
    doc = MW.material_scene(F)
    S = load_scene(doc)
    S.bvh_arity = arity
    _, f = MW.sized(S)
    host, host_frame = host_stats(emu, S, f, (F & 15) | (abi.RT_FEAT_BVH4 if arity == 4 else 0))
    with Renderer(S) as R:
        assert R.info()["features"] == want_features(F, arity)
        gpu = R.stats(f, seed=MW.SEED)
        flat = bool(F & MW.FLAT)
        names = PATH_COUNTERS + (WALK_COUNTERS if flat else ())
        print("F=%d arity %d gpu  %s" % (F, arity, {k: gpu[k] for k in PATH_COUNTERS + WALK_COUNTERS}))
        print("F=%d arity %d host %s" % (F, arity, {k: host[k] for k in PATH_COUNTERS + WALK_COUNTERS}))
        off = [k for k in names if gpu[k] != host[k]]
        off += [k for k in WALK_COUNTERS if not flat and gpu[k] < host[k]]
        if off:  # did a path diverge (a tie resolved the other way), or is a count wrong?
            d = np.abs(np.nan_to_num(R.render(f, seed=MW.SEED)) - np.nan_to_num(host_frame))
            j, i, c = np.unravel_index(np.argmax(d), d.shape)
            pytest.fail("F=%d arity %d: %s; frames of the two builds differ by at most %g "
                        "(pixel %d, %d; above 1e-9 a path diverged, below it the count is wrong)"
                        % (F, arity, ", ".join("%s gpu %d host %d" % (k, gpu[k], host[k]) for k in off),
                           d.max(), i, j))
    assert gpu["samples"] == f.image_width * f.image_height * MW.SPP
    assert gpu["segments"] >= gpu["samples"] and gpu["shade_events"] > 0
    if flat:
        assert gpu["node_visits"] == 0
    else:
        assert gpu["node_visits"] > 0
    if F & MW.LIGHTS:
        assert gpu["light_tests"] > 0
    if F & MW.NOISE and F & MW.MEDIA:  # counted where the material's own texture is the noise
        assert gpu["noise_evals"] > 0
    if F & MW.MEDIA:
        assert gpu["medium_box_tests"] > 0
    assert gpu["node_visits"] <= 64 * gpu["wave_node_iters"]
    assert gpu["shade_events"] <= 64 * gpu["wave_shade_iters"]
    assert gpu["noise_evals"] <= 64 * gpu["wave_noise_iters"]
    assert gpu["segments"] <= 64 * gpu["wave_trips"]
    assert gpu["medium_box_deferred"] <= gpu["medium_box_tests"]
    if gpu["node_visits"] > 0:
        print("F=%d arity %d model_trace_max %d pair %d" % (F, arity, gpu["model_trace_max"],
                                                          gpu["model_trace_pair_max"]))
        assert gpu["model_trace_pair_max"] <= gpu["model_trace_max"] <= 2 * gpu["model_trace_pair_max"]
