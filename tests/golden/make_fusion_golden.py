#!/usr/bin/env python3
"""Generate tests/golden/fusion_small.npz by running the REFERENCE's datasets.sdf_util.sdf_from_occupancy (imported read-only, as
make_visible_golden.py does) on the CPU, on small seeded occupancy grids.

Run in the build container only:
    python tests/golden/make_fusion_golden.py

Grids (tests/fusion_model.GRIDS): (12,9,7) at density 0.05, (33,17,5) at 0.3, (8,8,8) at 0.9 and (20,3,2) at 0.01, voxel sizes
0.05 and 0.07; each is asserted to hold both classes (the reference's result means nothing otherwise).  Stored per grid: the
occupancy bit-packed, the reference's float64 result, dims and voxel.  Only data is written."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from tests import fusion_model as fm  # noqa: E402


def main():
    mg.import_reference()
    from isdf.datasets import sdf_util
    out = {}
    for k, (dims, density, voxel) in enumerate(fm.GRIDS):
        rng = np.random.RandomState(10 + k)
        occ = (rng.uniform(size=dims) < density).astype(np.uint8)
        assert occ.any() and not occ.all(), dims
        sdf = sdf_util.sdf_from_occupancy(occ, voxel)
        assert sdf.dtype == np.float64 and sdf.shape == dims
        model = fm.occupancy_sdf(occ, voxel, np.float64)
        print("%s density %g voxel %g: %d occupied of %d, model == reference: %s" % (dims, density, voxel, occ.sum(), occ.size,
                                                                                  np.array_equal(model, sdf)))
        out["g%d/occ" % k], out["g%d/sdf" % k] = np.packbits(occ), sdf
        out["g%d/dims" % k], out["g%d/voxel" % k] = np.array(dims, np.int64), np.float64(voxel)
    path = os.path.join(HERE, "fusion_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
