"""Generates tests/golden/cylinder_vorticity.npz from a *data file* of the reference: the vorticity of the leading direct
mode of the cylinder that its outpost_ks wrote (examples/cylinder/stability/direct/dRv1cyl0.f00001; lx1 = 6, fp32).  Run once,
where the reference's tree is at hand:

    python tests/golden/make_vorticity_fixture.py <root of the reference's tree>

Stored: ``w`` = the first velocity component of the file (the vorticity; fp32, (1996, 6, 6), global element order as
nekio.read_fld returns it) and ``vy_is_zero`` = the file's second component is identically zero.  The mode itself is
cylinder_modes.npz:dRe_u (make_fixtures.py).  Nothing here copies reference source; the output is data only.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from nekstab_amd import nekio  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    f = nekio.read_fld(os.path.join(ref, "examples", "cylinder", "stability", "direct", "dRv1cyl0.f00001"))
    assert f.wdsize == 4 and f.nz == 1 and f.u.shape == (2, 1996, 1, 6, 6), (f.wdsize, f.u.shape)
    w = f.u[0, :, 0].astype(np.float32)
    assert np.array_equal(w.astype(np.float64), f.u[0, :, 0])                  # the file is fp32: nothing is lost
    np.savez_compressed(os.path.join(OUT, "cylinder_vorticity.npz"), w=w, vy_is_zero=np.array(not np.any(f.u[1])),
                        time=np.array(f.time), istep=np.array(f.istep), rdcode=np.array(f.rdcode))
    print("cylinder_vorticity.npz: max |w| %.4f, second component zero: %s, read code %s" % (np.abs(w).max(), not np.any(f.u[1]), f.rdcode))


if __name__ == "__main__":
    main(sys.argv[1])
