"""The form of a time step (StepForm, decided once per map by step_form in nsk.hip) as the counters of nsk_get_stats show it:
which settings run the deferred projection update, the fused convection + right-hand side, the packed velocity solve, the
compact argument blocks and the persistent tails.  Cylinder fixture at lx1 = 6, production context, maps of 6 time steps.  A map
that had to be redone counts again, so with retries > 0 a counter is "at least" and not "equal" (as _counts of
tests/test_lean_args_gpu.py)."""
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

NSTEPS, NMAPS = 6, 2
STEP_COUNTERS = ("convfuse_steps", "helmpack_steps", "leanargs_steps")
_CASE = []


def _case():
    if not _CASE:
        from nekstab_amd import mesh
        _CASE.append(mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), 6))
    return _CASE[0]


def _stats(options=(), **ctx):
    from nekstab_amd import seed
    from nekstab_amd.settings import production_context
    case = _case()
    h = production_context(case, **ctx)
    try:
        for k, val in options:
            h.set_option(k, val)
        h.set_nsteps(NSTEPS)
        v = h.alloc(NMAPS + 1)
        qx, qy = seed.add_noise(case)
        h.upload(v[0], qx, qy, np.zeros((case.nel, case.lx1 - 2, case.lx1 - 2)))
        h.scal(v[0], 1.0 / h.norm(v[0]))
        for k in range(NMAPS):
            h.matvec(v[k + 1], v[k], 0)
        assert np.all(np.isfinite(h.download(v[NMAPS])[0]))
        st = h.stats()
    finally:
        h.close()
    print({k: st[k] for k in ("absorb_maps", "tail_maps", "retries") + STEP_COUNTERS})
    return st


def _is(st, name, n):
    """counter `name` says n maps (or steps) ran the form; a redone map counts again"""
    if n == 0 or st["retries"] == 0:
        assert st[name] == n, (name, st[name], n)
    else:
        assert st[name] >= n, (name, st[name], n)


def test_default():
    st = _stats()
    _is(st, "absorb_maps", NMAPS)
    for k in STEP_COUNTERS:
        _is(st, k, NMAPS * NSTEPS)


def test_hostcheck():
    """eager host-checked steps: no deferred update, no tails, nothing to redo; the three per-step forms stay"""
    st = _stats([("hostcheck", 1)])
    assert st["absorb_maps"] == 0 and st["tail_maps"] == 0 and st["retries"] == 0
    for k in STEP_COUNTERS:
        assert st[k] == NMAPS * NSTEPS, (k, st[k])


def test_fuse2_off():
    """without the two-launch iteration no solve starts inside A_0, so nothing is deferred"""
    st = _stats([("fuse2", 0)])
    assert st["absorb_maps"] == 0
    for k in STEP_COUNTERS:
        _is(st, k, NMAPS * NSTEPS)


def test_fused():
    """the persistent velocity solve takes none of the four forms"""
    st = _stats(fused=1)
    assert st["absorb_maps"] == 0
    for k in STEP_COUNTERS:
        assert st[k] == 0, (k, st[k])


def test_lean_args_and_helm_pack_off():
    st = _stats([("lean_args", 0), ("helm_pack", 0)])
    assert st["leanargs_steps"] == 0 and st["helmpack_steps"] == 0
    _is(st, "convfuse_steps", NMAPS * NSTEPS)
