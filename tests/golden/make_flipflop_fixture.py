"""Generates tests/golden/flipflop_case.npz from the reference's *data files* of the flip-flop example
(examples/flip_flop/baseflow: two side-by-side cylinders between free-slip lateral boundaries): mesh vertices,
boundary codes ('SYM' on y = -50 and y = +50 among them), vertex ids and the committed base flow
BF_Re60_2cyl0.f00001, in the format of mesh.save_case_npz (which keeps the codes).  The mesh's 3128 midside-node ('m')
curved sides are not kept -- mesh.element_coords_2d builds circular arcs only -- so the fixture's elements are
straight-sided.  Run once in the build container:

    python tests/golden/make_flipflop_fixture.py

Nothing here copies reference source; the output is data only.  The base-flow velocity is stored in fp32 (the precision
nekStab's field files are written in) and its pressure, which no map reads, is left out, so that the fixture stays below
the size limit of a committed file.
"""
import os
import sys
from collections import Counter

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from nekstab_amd import mesh, nekio  # noqa: E402

REF = "/root/reference/examples/flip_flop/baseflow/"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "flipflop_case.npz")


def main():
    m = nekio.read_re2(REF + "2cyl.re2")
    vlex, _ = nekio.read_ma2(REF + "2cyl.ma2")
    bf = nekio.read_fld(REF + "BF_Re60_2cyl0.f00001")
    mesh.save_case_npz(OUT, m, vlex, bf.u[:, :, 0].astype(np.float32))
    print(OUT, os.path.getsize(OUT), "bytes;", m.nel, "elements, base flow at lx1 =", bf.nx,
          dict(Counter(b[3].strip() for b in m.bcs)))


if __name__ == "__main__":
    main()
