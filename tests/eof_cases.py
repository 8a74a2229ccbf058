"""
The series of the EOF tests (test_eof.py, test_gpu_eof.py).  Not a test module.

four_mode_series(): T fields on a (lat, lon) grid built from four orthogonal, centred, unit-variance PCs with amplitudes 8, 4, 2, 1
times random patterns of standard deviation 8, around 280, plus white noise of 0.05: eigenvalues near 4e3, 1e3, 2.6e2, 64 (the
patterns' weighted norms vary them a little), then a noise floor near 1e-4 (the weights sum to 1); the gaps are a factor of
about 4 apart, and every regression coefficient stays below 300, the scale of the bars of test_gpu_time_regression.py.
"""
import numpy as np

AMPLITUDES = (8.0, 4.0, 2.0, 1.0)
NOISE = 0.05
T, NLAT, NLON = 64, 18, 20


def latitudes(nlat=NLAT):
    return np.linspace(-85.0, 85.0, nlat)


def weights(nlat=NLAT, nlon=NLON):
    """cos(lat) over the grid"""
    return np.repeat(np.cos(np.deg2rad(latitudes(nlat)))[:, None], nlon, axis=1)


def four_mode_series(seed=0, n_rows=T, nlat=NLAT, nlon=NLON, scale=64.0):
    """(x (T, lat, lon) float32, pcs (T, 4) float64 with zero mean and unit variance at ddof = 1)"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n_rows, len(AMPLITUDES)))
    z -= z.mean(axis=0, keepdims=True)
    q, _ = np.linalg.qr(z)
    pcs = q * np.sqrt(n_rows - 1.0)
    # (a pattern of unit variance has a weighted norm near 1 under weights that sum to 1: the eigenvalues are near
    # amplitude^2 * scale)
    patterns = rng.standard_normal((len(AMPLITUDES), nlat, nlon)) * np.sqrt(scale)
    x = 280.0 + np.einsum('tk,k,kij->tij', pcs, np.array(AMPLITUDES), patterns) + NOISE * rng.standard_normal((n_rows, nlat, nlon))
    return x.astype(np.float32), pcs


def weight_root(w):
    """the float32 weight root of the analysis and the sum of its squares: weights scaled to sum 1, the root rounded once"""
    w = np.asarray(w, dtype=np.float64)
    r32 = np.sqrt(w / w.sum()).astype(np.float32)
    return r32, float((r32.astype(np.float64) ** 2).sum())
