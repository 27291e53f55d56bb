"""Generates tests/golden/cylinder_bf_sensitivity.npz from the reference's committed output of bf_sensitivity
(examples/cylinder/postproc/steady_force_sensitivity/sr_1cyl0.f00001, si_1cyl0.f00001: the base-flow sensitivity of the
cylinder's leading mode at lx1 = 6, computed from the modes stored in cylinder_modes.npz).  Data only: the velocity fields,
fp32 as in the files.  Run once in the build container:

    python tests/golden/make_sensitivity_fixture.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from nekstab_amd import nekio  # noqa: E402

REF = "/root/reference/examples/cylinder/postproc/steady_force_sensitivity/"
OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    out = {}
    for k in ("sr", "si"):
        f = nekio.read_fld(REF + k + "_1cyl0.f00001")
        out[k + "_u"] = np.asarray(f.u[:, :, 0], dtype=np.float32)          # (2, nel, 6, 6), global element order
    np.savez_compressed(OUT + "/cylinder_bf_sensitivity.npz", **out)


if __name__ == "__main__":
    main()
