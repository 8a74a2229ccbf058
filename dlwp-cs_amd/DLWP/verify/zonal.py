"""
Zonal spectra of DLWP.verify: power, cross-spectrum and coherence per zonal wavenumber.
"""
from collections import namedtuple

import numpy as np

from ..labelled import axes as _axes, axis_of, device_scope, host as _host, label, on_device as _on_device
from .scores import _check_labels, _dev_operand, _weights

# --------------------------------------------------------------------------------------------------------------------- #
# Zonal spectra: scores that depend on scale
# --------------------------------------------------------------------------------------------------------------------- #
#
# RMSE and ACC reward a forecast that has smoothed its small scales away.  The zonal power spectrum shows the loss of variance
# per wavenumber, the coherence how much of the verification's phase the forecast still holds at each scale.  For a row
# x[0..L-1] along longitude:  X_k = sum_j x_j exp(-2 pi i jk / L),  P_k = c_k |X_k|^2 / L^2 with c_k = 1 for k = 0 and for
# k = L/2 when L is even, else 2 -- so that sum_k P_k = mean_j x_j^2.  Rows are averaged with weights; a row counts only when all
# of its values are finite (in both arrays of a pair).  numpy inputs are transformed on the host (np.fft.rfft in float64),
# device tensors by dlwpcs_zonal_spectrum; neither path falls back to the other.

CrossSpectrum = namedtuple('CrossSpectrum', ['power_f', 'power_v', 'co', 'quad'])


def _row_weights(x, lon, weighted, weights):
    """float64 weights that broadcast against the leading shape (x's shape without longitude), or None"""
    lead = tuple(int(e) for i, e in enumerate(x.shape) if i != lon)
    w = None
    if weighted:
        full = np.asarray(_weights(x), dtype=np.float64)
        shape = tuple(int(e) for e in x.shape)
        full = full.reshape((1,) * (len(shape) - full.ndim) + full.shape) if full.ndim <= len(shape) else full
        if full.ndim != len(shape) or full.shape[lon] != 1 or any(e not in (1, s) for e, s in zip(full.shape, shape)):
            raise ValueError('the latitude weights %s must broadcast against %s and be constant along longitude'
                             % (full.shape, shape))
        w = np.squeeze(full, axis=lon)
    if weights is not None:
        ex = np.asarray(_host(weights), dtype=np.float64)
        np.broadcast_shapes(ex.shape, lead)                   # raises where they do not fit
        if ex.ndim > len(lead):
            raise ValueError('weights %s have more axes than the leading shape %s' % (ex.shape, lead))
        w = ex if w is None else w * ex
    if w is not None and not np.all(np.isfinite(w)):
        raise ValueError('the weights must be finite')
    return w


def _spectrum_host(f, v, lon, ax, w, n_wave, remove_mean):
    """numpy twin of dlwpcs_zonal_spectrum: (quantities (nq, kept..., K) float64, skipped rows (kept...) int32)"""
    arrs = [np.moveaxis(np.asarray(x, dtype=np.float64), lon, -1) for x in ((f,) if v is None else (f, v))]
    L = arrs[0].shape[-1]
    K = L // 2 + 1 if n_wave is None else int(n_wave)
    lead = arrs[0].shape[:-1]
    red = tuple(a if a < lon else a - 1 for a in ax)
    counted = np.ones(lead, dtype=bool)
    for x in arrs:
        counted &= np.isfinite(x).all(axis=-1)
    ck = np.full(K, 2.0)
    ck[0] = 1.0
    if L % 2 == 0 and K == L // 2 + 1:
        ck[-1] = 1.0
    spec, means = [], []
    for x in arrs:
        x = np.where(counted[..., None], x, 0.0)
        m = x.mean(axis=-1)
        means.append(m)
        spec.append(np.fft.rfft(x - m[..., None] if remove_mean else x, axis=-1)[..., :K])
    F, V = spec[0], spec[-1]
    q = [ck * (F.real ** 2 + F.imag ** 2) / L ** 2]
    if v is not None:
        cross = F * np.conj(V)
        q += [ck * (V.real ** 2 + V.imag ** 2) / L ** 2, ck * cross.real / L ** 2, ck * cross.imag / L ** 2]
    if remove_mean:
        q[0][..., 0] = means[0] ** 2
        if v is not None:
            q[1][..., 0], q[2][..., 0], q[3][..., 0] = means[1] ** 2, means[0] * means[1], 0.0
    wf = np.broadcast_to(1.0 if w is None else w, lead) * counted
    sw = wf.sum(axis=red) if red else wf.copy()
    with np.errstate(invalid='ignore', divide='ignore'):
        out = np.stack([np.where(sw[..., None] == 0, np.nan, (x * wf[..., None]).sum(axis=red) / sw[..., None]) for x in q])
    skipped = (~counted).sum(axis=red) if red else (~counted).astype(np.int64)
    return out, np.asarray(skipped, dtype=np.int32)


def _spectrum_device(f, v, lon, ax, w, n_wave, remove_mean):
    from .. import ops as dops
    with device_scope(f, v) as dev:
        ft = _dev_operand(f, dev)
        vt = _dev_operand(v, dev) if v is not None else None
        wt = _dev_operand(w, dev) if w is not None else None
        out, cnt = dops.zonal_spectrum(ft, vt, lon_axis=lon, reduced=ax, weights=wt, n_wave=n_wave, remove_mean=remove_mean,
                                       counts=True)
        out = out.cpu().numpy().astype(np.float64)
        return (out[None] if v is None else out), cnt.cpu().numpy()


def _spectrum(f, v, lon_axis, axis, weighted, weights, n_wave, remove_mean):
    """(quantities (nq, kept..., K) float64, skipped, what labels one of the quantities like f: (values, name) -> result)"""
    if v is not None:
        if len(v.shape) == len(f.shape) - 1:
            raise NotImplementedError('the lagged form against a continuous verification series (valid[f + t]) is not served: '
                                      'aligned arrays of one shape are')
        _check_labels(f, v)
        if tuple(f.shape) != tuple(v.shape):
            raise ValueError('forecast %s and verification %s must have one shape' % (tuple(f.shape), tuple(v.shape)))
    if len(f.shape) < 1:
        raise ValueError('the input needs a longitude axis')
    lon = axis_of(f, 'lon', lon_axis, 'lon_axis %d out of range of %d axes')
    L = int(f.shape[lon])
    if L < 2:
        raise ValueError('%d longitudes (at least 2)' % L)
    if n_wave is not None and not 1 <= int(n_wave) <= L // 2 + 1:
        raise ValueError('n_wave = %s outside 1 .. L // 2 + 1 = %d' % (n_wave, L // 2 + 1))
    ax = tuple(i for i in range(len(f.shape)) if i != lon) if axis is None else _axes(axis, len(f.shape), f)
    if lon in ax:
        raise ValueError('the longitude axis is transformed, it cannot be averaged over')
    w = _row_weights(f if v is None else v, lon, weighted, weights)
    if _on_device(f, v):
        out, skipped = _spectrum_device(f, v, lon, ax, w, n_wave, remove_mean)
    else:
        out, skipped = _spectrum_host(_host(f), None if v is None else _host(v), lon, ax, w, n_wave, remove_mean)
    return out, skipped, lambda values, name: label(f, values, name, drop=(lon,) + ax,
                                                    tail=[('wavenumber', np.arange(values.shape[-1]))])


def zonal_spectrum(x, lon_axis=-1, axis=None, weighted=False, weights=None, n_wave=None, remove_mean=False, return_count=False):
    """
    One-sided zonal power spectrum P_k = c_k |X_k|^2 / L^2 of `x` along longitude, averaged over `axis`.

    :param x: ndarray, device tensor or labelled array (its dim 'lon' is the longitude axis)
    :param lon_axis: the longitude axis of an unlabelled input
    :param axis: int, dim name, tuple or None: the axes averaged over besides longitude, which is transformed (None: all)
    :param weighted: weight the rows by cos(latitude) read from `x.lat`
    :param weights: row weights that broadcast against the leading axes (x's shape without longitude); a latitude band is a
        weight of zeros and ones, times cos(latitude) where wanted.  Multiplies the cos(latitude) weights of `weighted`.
    :param n_wave: return the first n_wave wavenumbers only (1 .. L // 2 + 1)
    :param remove_mean: subtract each row's zonal mean before the transform and report P_0 as that mean squared: the same
        numbers, but the rounding error of the other wavenumbers no longer scales with the offset squared (280 K temperatures)
    :param return_count: also return the number of rows per result that did not count (rows holding a NaN or an infinity)
    :return: float64 array (kept axes..., wavenumber), labelled like the input; NaN where no row counts or the weights sum to 0
    """
    out, skipped, lab = _spectrum(x, None, lon_axis, axis, weighted, weights, n_wave, remove_mean)
    res = lab(out[0], 'zonal_spectrum')
    return (res, skipped) if return_count else res


def zonal_cross_spectrum(forecast, valid, lon_axis=-1, axis=None, weighted=False, weights=None, n_wave=None, remove_mean=False,
                         return_count=False):
    """
    Zonal power spectra of a forecast and its verification (aligned arrays of one shape) and their cross-spectrum, averaged
    over `axis`: CrossSpectrum(power_f, power_v, co, quad) with co + i quad = c_k F_k conj(V_k) / L^2.  A row counts only when
    it is finite in both arrays.  Arguments as for `zonal_spectrum`; a continuous verification series (one axis fewer) raises
    NotImplementedError.
    """
    out, skipped, lab = _spectrum(forecast, valid, lon_axis, axis, weighted, weights, n_wave, remove_mean)
    res = CrossSpectrum(*[lab(out[i], n) for i, n in enumerate(CrossSpectrum._fields)])
    return (res, skipped) if return_count else res


def zonal_coherence(forecast, valid, lon_axis=-1, axis=None, weighted=False, weights=None, n_wave=None, remove_mean=False,
                    return_count=False):
    """
    Squared coherence (co^2 + quad^2) / (power_f power_v) per wavenumber, formed from the AVERAGED spectra of
    `zonal_cross_spectrum` (per row it would be identically 1): 1 where the forecast holds the verification's phase over the
    averaged rows, near 1 / rows where the two are unrelated.  NaN where either power is 0.  Arguments as for `zonal_spectrum`.
    """
    out, skipped, lab = _spectrum(forecast, valid, lon_axis, axis, weighted, weights, n_wave, remove_mean)
    with np.errstate(invalid='ignore', divide='ignore'):
        coh = (out[2] ** 2 + out[3] ** 2) / (out[0] * out[1])
    res = lab(coh, 'zonal_coherence')
    return (res, skipped) if return_count else res
