"""The camera-origin form of the static sphere root test (rt_path.h root_origin,
sphere_root_origin): rays that share an origin share oc = c0 - o and c = |oc|^2
- rr of a sphere, and the flat render loop forms them once per work unit for
the camera rays it traces where it generates them.  The form must be
sphere_root<false> from h = dot(d, oc) on: tests/native/rt_root_origin_check
holds it to the general form over 10^7 seeded rays per seed -- the same return
value, the same root bits -- with radii from 1e-3 to 1e3, origins on, at the
centre of and inside spheres, all-ones significands, and zero, inf and NaN
directions, with the division and with the shared reciprocal.  No GPU.
"""
import os
import subprocess

import pytest

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
CHECK = os.path.join(NATIVE, "build", "rt_root_origin_check")
N_RAYS = 10 ** 7


@pytest.fixture(scope="module")
def check():
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "root_origin.mk"], check=True)
    return CHECK


@pytest.mark.parametrize("seed", [1, 20261021])
def test_origin_form_has_the_general_forms_bits(check, seed):
    r = subprocess.run([check, str(N_RAYS), str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    w = r.stdout.split()
    assert w[0] == "OK"
    c = dict(zip(w[1::2], (int(x) for x in w[2::2])))
    print(c)
    assert c["rays"] == N_RAYS and c["tests"] == 4 * N_RAYS
    # the cases are there: roots found, found again under a bound, and the odd directions
    assert c["hits"] > N_RAYS // 10 and c["second"] > N_RAYS // 20 and c["special"] > N_RAYS // 20
