"""nekstab_amd/fourier.py: the numpy statement of the temporal Fourier convention of the device's Fourier orbits
(core/fourier.f), the amplitude report and the mode files.  No GPU."""
import numpy as np
import pytest

from nekstab_amd import fourier


@pytest.mark.parametrize("N", [12, 13])
def test_full_spectrum_reproduces_the_snapshots(N):
    """M = N // 2 reproduces every snapshot to rounding: even N carries the Nyquist term with weight 1 and B = 0, odd N has none."""
    rng = np.random.default_rng(N)
    U = rng.standard_normal((N, 2, 5, 4))
    M = N // 2
    A, B = fourier.np_dft_modes(U, M)
    assert A.shape == (M + 1, 2, 5, 4) and B.shape == (M, 2, 5, 4)
    if N % 2 == 0:
        assert np.all(B[M - 1] == 0.0)
    for n in range(N):
        r = fourier.np_reconstruct(A, B, n / N)
        err = np.linalg.norm(r - U[n]) / np.linalg.norm(U[n])
        assert err < 1e-12, (n, err)
    # periodic in s
    assert np.linalg.norm(fourier.np_reconstruct(A, B, 3 / N + 2.0) - U[3]) / np.linalg.norm(U[3]) < 1e-12


def test_band_limited_signal_is_recovered_with_its_modes():
    rng = np.random.default_rng(3)
    N, M = 16, 3
    A0 = rng.standard_normal((M + 1, 7))
    B0 = rng.standard_normal((M, 7))
    U = np.stack([fourier.np_reconstruct(A0, B0, n / N) for n in range(N)])
    A, B = fourier.np_dft_modes(U, M)
    assert np.abs(A - A0).max() < 1e-13 and np.abs(B - B0).max() < 1e-13
    for n in range(N):
        assert np.abs(fourier.np_reconstruct(A, B, n / N) - U[n]).max() < 1e-13
    with pytest.raises(ValueError):
        fourier.np_dft_modes(U, N // 2 + 1)


def test_amplitude_report_on_a_hand_made_list():
    # |A_0| = 7; harmonics: (3, 4) -> 5, (1, 0) -> 1, (0, 0.05) -> 0.05
    amp = [7.0, 3.0, 4.0, 1.0, 0.0, 0.0, 0.05]
    r = fourier.amplitude_report(amp)
    assert np.allclose(r["ampl"], [7.0, 5.0, 1.0, 0.05], rtol=0, atol=1e-15)
    assert np.allclose(r["share"], [5.0 / 6.05, 6.0 / 6.05, 1.0], rtol=0, atol=1e-15)
    assert r["m99"] == 2                     # 6 / 6.05 = 0.9917
    assert fourier.amplitude_report([2.0])["m99"] == 0
    with pytest.raises(ValueError):
        fourier.amplitude_report([1.0, 2.0])


class _StubHandle:
    """Vectors are dicts of numpy arrays; records what set_orbit_modes receives."""
    ndim, nel, lx1 = 2, 3, 4

    def __init__(self, A, B, period):
        self.npres = self.nel * 2 * 2
        self._A, self._B, self._period = A, B, period
        self.loaded = None
        self.live = 0

    def alloc(self, n=1):
        self.live += n
        return [dict(u=None) for _ in range(n)]

    def free(self, vecs):
        self.live -= len(vecs)

    def get_orbit_modes(self, A=None, B=None):
        if A is not None:
            for k, v in enumerate(A):
                v["u"] = self._A[k].copy()
            for k, v in enumerate(B):
                v["u"] = self._B[k].copy()
        return len(self._B), self._period

    def download(self, v):
        return v["u"][0], v["u"][1], np.zeros(self.npres)

    def upload(self, v, vx, vy, pr):
        assert pr.size == self.npres
        v["u"] = np.stack([np.asarray(vx).reshape(self.nel, self.lx1, self.lx1), np.asarray(vy).reshape(self.nel, self.lx1, self.lx1)])

    def norm(self, v):
        return float(np.sqrt(np.sum(v["u"] ** 2)))

    def set_orbit_modes(self, A, B, period):
        self.loaded = ([v["u"].copy() for v in A], [v["u"].copy() for v in B], period)


def test_mode_files_round_trip_exactly(tmp_path):
    rng = np.random.default_rng(5)
    M, period = 3, 5.123456789012345
    A = rng.standard_normal((M + 1, 2, 3, 4, 4))
    B = rng.standard_normal((M, 2, 3, 4, 4))
    src = _StubHandle(A, B, period)
    files = fourier.write_modes(src, str(tmp_path), session="tst")
    assert len(files) == 2 * M + 2 and src.live == 0
    dst = _StubHandle(None, None, None)
    m, per, amp = fourier.read_modes(dst, str(tmp_path), session="tst")
    assert m == M and per == period and dst.live == 0
    la, lb, lp = dst.loaded
    assert lp == period and len(la) == M + 1 and len(lb) == M
    for k in range(M + 1):
        assert np.array_equal(la[k], A[k])
    for k in range(M):
        assert np.array_equal(lb[k], B[k])
    want = [np.sqrt(np.sum(A[0] ** 2))]
    for k in range(1, M + 1):
        want += [np.sqrt(np.sum(A[k] ** 2)), np.sqrt(np.sum(B[k - 1] ** 2))]
    assert np.array_equal(amp, np.array(want))
