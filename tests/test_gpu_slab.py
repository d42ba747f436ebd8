"""The fp32 box tests of rt_path.h as gfx950 runs them -- rcp32 is v_rcp_f32
(1 ulp, the hardware's denormal and zero behaviour), min3f / max3f and
slab_hit's far distance are inline-asm v_min3_f32 / v_max3_f32, the planes come
out of LDS and out of memory through load_planes_l / load_planes<W> -- on the
cases and with the assertions of tests/slab_cases.py, the host twin being
tests/test_emulator.py::test_every_slab_form_is_conservative_and_the_fma_family_agrees:

* no form drops a box the exact (long double) slab test hits, inside the
  stated domain;
* slab<true>, slab_hit, slab_hit2, slab2_planes, slab_planes<2> and
  slab_planes<4> agree in verdict and entry-distance bits for every child slot
  and both address spaces, on every case (no operand and no intermediate is a
  NaN, so no case is excluded);
* most exact misses are culled.

Rays in a face plane, below and above the domain are run and counted; the
device's and the host's verdicts may differ (rcp32) and are counted too.
One launch of tests/native/build/libdevcheck.so (test-only)."""
import ctypes as C
import os

import numpy as np
import pytest

import slab_cases as SC

pytestmark = pytest.mark.gpu

NATIVE = os.path.join(os.path.dirname(__file__), "native", "build")


def test_every_slab_form_on_device():
    lib = os.path.join(NATIVE, "libdevcheck.so")
    assert os.path.exists(lib), "build tests/native first (make -C tests/native)"
    cs = SC.make_cases()
    verdict, tl = SC.run_forms(C.CDLL(lib).devcheck_slab_forms, cs)
    SC.check_forms(cs, verdict, tl, "gfx950")
    hv, htl = SC.run_forms(C.CDLL(os.path.join(NATIVE, "libemu.so")).emu_slab_forms, cs)
    for v, name in ((0, "subtract form"), (1, "FMA family")):
        differ = ((verdict ^ hv) >> v) & 1 == 1
        print("gfx950 vs host verdicts, %s: %d of %d cases differ (%d inside the domain)"
              % (name, differ.sum(), len(differ), (differ & cs["domain"]).sum()))
    same = (tl.view(np.uint32)[:, 2] == htl.view(np.uint32)[:, 2])
    print("gfx950 vs host entry distances (slab_hit): %d of %d cases differ" % ((~same).sum(), len(same)))
