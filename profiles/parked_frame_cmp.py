"""frame_cmp.py A.npy B.npy MODE  (MODE: equal | order64)"""
import sys
import numpy as np
a, b = np.load(sys.argv[1]), np.load(sys.argv[2])
mode = sys.argv[3]
assert a.shape == b.shape
if mode == "equal":
    ok = np.array_equal(a, b, equal_nan=True)
    print("frame_sums", sys.argv[1], sys.argv[2], a.shape, "array_equal" if ok else "DIFFER", "nan", int(np.isnan(a).sum()), int(np.isnan(b).sum()))
    sys.exit(0 if ok else 1)
n = 64
bound = 2 * (n - 1) * 2.0 ** -53  # two summation orders of the same n non-negative terms, relative to the sum
assert np.isfinite(a).all() and np.isfinite(b).all() and (a >= 0).all()
rel = np.abs(a - b) / np.maximum(np.abs(a), 1e-300)
bad = int((rel > bound).sum())
print("frame_sums", sys.argv[1], sys.argv[2], a.shape, "array_equal" if np.array_equal(a, b) else "not array_equal",
      "differing channels %d of %d" % (int((a != b).sum()), a.size),
      "max relative difference %.3g (bound 2 (n - 1) 2^-53 = %.3g, n = 64)" % (rel.max(), bound), "outside the bound: %d" % bad)
sys.exit(0 if bad == 0 else 1)
