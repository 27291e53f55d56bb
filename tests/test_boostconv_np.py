"""np_boostconv_core (nekstab_amd/fixedp.py), the numpy restatement of boostconv_core (core/fixedp.f:331-468) the device is tested
against: it accelerates a linear fixed-point iteration the way the algorithm promises, it gives an empty column no weight, and
the driver's residu.dat line has the reference's format.  No GPU.

`linear_problem` is shared with tests/test_boostconv_gpu.py."""
import numpy as np


def linear_problem(shape, bm1, rank, seed=3):
    """r(v) = b - A v on fields of `shape` = (ndim, ...): A = sum_i lam_i u_i u_i^T bm1 with `rank` bm1-orthonormal u_i, b in
    their span with unit bm1 norm.  Plain iteration v <- v + r contracts the error by 1 - lam_i per call, lam_i spread over [0.1, 0.8]
    (well separated, so that the stored differences stay independent to rounding and the exact end shows);
    BoostConv with snp >= rank ends it once it holds `rank` independent differences.  Returns (residual function, bm1 norm)."""
    rng = np.random.default_rng(seed)
    w = np.broadcast_to(bm1, shape[1:])[None]
    ip = lambda a, b: float(np.sum(w * a * b))
    U = []
    for _ in range(rank):
        u = rng.standard_normal(shape)
        for _ in range(2):
            for q in U:
                u -= ip(u, q) * q
        U.append(u / np.sqrt(ip(u, u)))
    lam = np.linspace(0.1, 0.8, rank)
    b = sum(rng.uniform(0.5, 1.0) * u for u in U)
    b /= np.sqrt(ip(b, b))
    resid = lambda v: b - sum(l * ip(u, v) * u for l, u in zip(lam, U))
    return resid, lambda a: np.sqrt(ip(a, a))


def _run(snp, rank, ncalls, shape=(2, 7, 5)):
    from nekstab_amd import fixedp
    bm1 = np.random.default_rng(1).uniform(0.5, 2.0, shape[1:])
    resid, norm = linear_problem(shape, bm1, rank)
    v, vp, st = np.zeros(shape), np.zeros(shape), {}
    hist, plain = [], []
    for _ in range(ncalls):
        r = resid(v)
        hist.append(norm(r))
        v = v + fixedp.np_boostconv_core(st, r, bm1, snp)
        plain.append(norm(resid(vp)))
        vp = vp + resid(vp)
    return np.array(hist), np.array(plain), st


def test_rank_three_is_solved_at_the_fifth_call():
    """snp = 3, rank 3: calls 2 .. 4 store three independent differences, the residual of call 5 is at rounding level while
    the plain iteration is still at a third of its start (1.0, 0.51, 0.37, 0.24, 3.4e-15 against 0.30)."""
    hist, plain, _ = _run(3, 3, 5)
    print("BoostConv", hist, "plain", plain)
    assert hist[0] == 1.0 or abs(hist[0] - 1.0) < 1e-14
    assert hist[4] <= 1e-12
    assert plain[4] >= 0.1


def test_rank_eight_with_ten_columns_converges_and_stays():
    """snp = 10 > rank 8: once converged the stored differences are rounding noise, parallel or zero -- the calls after
    convergence are where an unguarded normal-equations solve fails; the reference's Gram-Schmidt form holds."""
    hist, plain, _ = _run(10, 8, 14)
    print("BoostConv", hist, "plain", plain)
    assert np.all(hist[9:] <= 1e-12) and len(hist[9:]) == 5
    assert plain[13] >= 0.1 * 0.9 ** 14


def test_an_empty_column_gets_no_weight():
    """At the second call of snp = 3 the columns 2 and 3 of Y are still zero: projected norm < 1e-60, q = 0, R_jj = 1, c_j = 0."""
    from nekstab_amd import fixedp
    shape = (2, 4, 3)
    bm1 = np.random.default_rng(1).uniform(0.5, 2.0, shape[1:])
    resid, _ = linear_problem(shape, bm1, 3)
    st, v = {}, np.zeros(shape)
    v = v + fixedp.np_boostconv_core(st, resid(v), bm1, 3)
    r = resid(v)
    xi = fixedp.np_boostconv_core(st, r, bm1, 3)
    assert st["rot"] == 2 and st["c"][0] != 0.0 and st["c"][1] == 0.0 and st["c"][2] == 0.0
    assert np.array_equal(st["Y"][1], r) and np.array_equal(st["X"][1], xi) and not np.any(st["Y"][2])


def test_residu_line_is_3e15_7():
    from nekstab_amd import fixedp
    assert fixedp.residu_line(12.5, 3.4567891e-5, -1.25e-3) == "  0.1250000E+02  0.3456789E-04 -0.1250000E-02"
    assert len(fixedp.residu_line(0.0, 1.0, 0.0)) == 45
