"""
Spherical harmonics of DLWP.verify: spectra per total wavenumber, analysis, synthesis and filtering, winds, vorticity and
divergence, gradients.  The `_transforms` and `_responses` caches live here and nowhere else.
"""
from collections import namedtuple

import numpy as np

from ..labelled import (axes as _axes, axis_of, device_f32, device_scope, host as _host, is_tensor as _is_tensor, label,
                        on_device as _on_device, raw as _raw)
from .scores import _check_labels, _dev_operand

# --------------------------------------------------------------------------------------------------------------------- #
# Spherical-harmonic spectra: power per total wavenumber
# --------------------------------------------------------------------------------------------------------------------- #
#
# The zonal spectrum treats a row at 80 N like a row at the equator and names no scale in kilometres.  The spherical-harmonic
# spectrum S_n = sum_{m<=n} c_m |a_n^m|^2 (DLWP/remap/spharm.py states the definitions) is the power per total wavenumber n that
# the literature reports: sum_n S_n is the area-weighted mean square of a band-limited field, S_0 its squared global mean, and
# degree n is a wavelength of 40 000 km / n.  The latitudes must be Gaussian, equally spaced with both poles, or equally spaced
# cell centres; the area weighting is inside the transform.  numpy inputs are transformed on the host (np.fft.rfft and the float64
# Legendre table), device tensors by dlwpcs_sht_spectrum; neither path falls back to the other.

SphericalCrossSpectrum = namedtuple('SphericalCrossSpectrum', ['power_f', 'power_v', 'co'])
_transforms = {}


def _spherical_transform(lat, n_lon, truncation):
    from ..remap.spharm import SphericalTransform
    lat = np.asarray(_host(lat), dtype=np.float64).reshape(-1)
    key = (lat.tobytes(), int(n_lon), None if truncation is None else int(truncation))
    hit = _transforms.get(key)
    if hit is None:
        hit = _transforms[key] = SphericalTransform(lat, n_lon, truncation)
    return hit


def _sht_host(f, v, la, lo, ax, tr):
    """numpy twin of ops.spherical_spectrum: (quantities (nq, kept..., T + 1) float64, skipped fields (kept...) int32)"""
    arrs = [np.moveaxis(np.asarray(x, dtype=np.float64), (la, lo), (-2, -1)) for x in ((f,) if v is None else (f, v))]
    lead_axes = [i for i in range(arrs[0].ndim) if i not in (la, lo)]
    red = tuple(lead_axes.index(a) for a in ax)
    counted = np.ones(arrs[0].shape[:-2], dtype=bool)
    for x in arrs:
        counted &= np.isfinite(x).all(axis=(-2, -1))
    arrs = [np.where(counted[..., None, None], x, 0.0) for x in arrs]
    q = tr.power(arrs[0], None if v is None else arrs[1])
    n = counted.sum(axis=red) if red else counted.astype(np.int64)
    with np.errstate(invalid='ignore', divide='ignore'):
        total = (q * counted[..., None]).sum(axis=tuple(r + 1 for r in red)) if red else q * counted[..., None]
        out = np.where(n[..., None] == 0, np.nan, total / np.maximum(n, 1)[..., None])
    skipped = (~counted).sum(axis=red) if red else (~counted).astype(np.int64)
    return out, np.asarray(skipped, dtype=np.int32)


def _sht_grid(f, lat, lat_axis, lon_axis, truncation):
    """(latitude axis, longitude axis, SphericalTransform) of the input f"""
    if len(f.shape) < 2:
        raise ValueError('the input needs a latitude and a longitude axis')
    la = axis_of(f, 'lat', lat_axis, 'lat_axis %d out of range of %d axes')
    lo = axis_of(f, 'lon', lon_axis, 'lon_axis %d out of range of %d axes')
    if la == lo:
        raise ValueError('the latitude and the longitude axis must differ')
    if lat is None:
        coords = getattr(f, 'coords', {})
        lat = coords['lat'] if 'lat' in coords else getattr(f, 'lat', None)
        if lat is None:
            raise ValueError("the latitudes are needed: pass lat=, or a labelled input with a 'lat' coordinate")
    lat = np.asarray(_host(lat), dtype=np.float64).reshape(-1)
    if lat.size != int(f.shape[la]):
        raise ValueError('%d latitudes for a latitude axis of %d' % (lat.size, int(f.shape[la])))
    return la, lo, _spherical_transform(lat, int(f.shape[lo]), truncation)


def _sht(f, v, lat, lat_axis, lon_axis, axis, truncation):
    """(quantities (nq, kept..., T + 1) float64, skipped, what labels one of the quantities like f: (values, name) -> result)"""
    if v is not None:
        if len(v.shape) == len(f.shape) - 1:
            raise NotImplementedError('the lagged form against a continuous verification series (valid[f + t]) is not served: '
                                      'aligned arrays of one shape are')
        _check_labels(f, v)
        if tuple(f.shape) != tuple(v.shape):
            raise ValueError('forecast %s and verification %s must have one shape' % (tuple(f.shape), tuple(v.shape)))
    la, lo, tr = _sht_grid(f, lat, lat_axis, lon_axis, truncation)
    nd = len(f.shape)
    ax = tuple(i for i in range(nd) if i not in (la, lo)) if axis is None else _axes(axis, nd, f)
    if la in ax or lo in ax:
        raise ValueError('the latitude and longitude axes are transformed, they cannot be averaged over')
    if _on_device(f, v):
        from .. import ops as dops
        with device_scope(f, v) as dev:
            ft = _dev_operand(f, dev)
            vt = _dev_operand(v, dev) if v is not None else None
            out, cnt = dops.spherical_spectrum(ft, vt, transform=tr, lat_axis=la, lon_axis=lo, reduced=ax, counts=True)
            out = out.cpu().numpy().astype(np.float64)
            out, skipped = (out[None] if v is None else out), cnt.cpu().numpy()
    else:
        out, skipped = _sht_host(_host(f), None if v is None else _host(v), la, lo, ax, tr)
    return out, skipped, lambda values, name: label(f, values, name, drop=(la, lo) + ax,
                                                    tail=[('degree', np.arange(values.shape[-1]))])


def spherical_spectrum(x, lat=None, lat_axis=-2, lon_axis=-1, axis=None, truncation=None, return_count=False):
    """
    Spherical-harmonic power spectrum S_n = sum_{m<=n} c_m |a_n^m|^2 of `x`, n = 0 .. truncation, averaged over `axis`.

    There is no `weighted=` argument: the area weighting is inside the transform (the quadrature weights of the latitudes).

    :param x: ndarray, device tensor or labelled array (its dims 'lat' and 'lon' are the grid axes, its coordinate 'lat' the
        latitudes)
    :param lat: the latitudes in degrees, either direction: Gaussian, equally spaced with both poles (181 latitudes), or equally
        spaced cell centres; any other vector is refused.  Needed for unlabelled inputs.
    :param lat_axis, lon_axis: the grid axes of an unlabelled input
    :param axis: int, dim name, tuple or None: the axes averaged over (None: all but the grid axes).  A field counts only when
        all of its values are finite.
    :param truncation: the largest degree; None: the largest the grid allows -- nlat - 1 for Gaussian latitudes,
        (nlat - 1) // 2 for the equally spaced ones, and (n_lon - 1) // 2.  A larger one is a ValueError.
    :param return_count: also return the number of fields per result that did not count
    :return: float64 array (kept axes..., degree), labelled like the input; NaN where no field counts
    """
    out, skipped, lab = _sht(x, None, lat, lat_axis, lon_axis, axis, truncation)
    res = lab(out[0], 'spherical_spectrum')
    return (res, skipped) if return_count else res


def spherical_cross_spectrum(forecast, valid, lat=None, lat_axis=-2, lon_axis=-1, axis=None, truncation=None, return_count=False):
    """
    Spherical-harmonic spectra of a forecast and its verification (aligned arrays of one shape) and their co-spectrum, averaged
    over `axis`: SphericalCrossSpectrum(power_f, power_v, co) with co_n = sum_m c_m Re(a_n^m(f) conj a_n^m(v)).  The imaginary
    part is not invariant under rotations and is not returned.  A field counts only when it is finite in both arrays.  Arguments as
    for `spherical_spectrum`; a continuous verification series (one axis fewer) raises NotImplementedError.
    """
    out, skipped, lab = _sht(forecast, valid, lat, lat_axis, lon_axis, axis, truncation)
    res = SphericalCrossSpectrum(*[lab(out[i], n) for i, n in enumerate(SphericalCrossSpectrum._fields)])
    return (res, skipped) if return_count else res


def spherical_correlation(forecast, valid, lat=None, lat_axis=-2, lon_axis=-1, axis=None, truncation=None, return_count=False):
    """
    Correlation per degree co / sqrt(power_f power_v), formed from the AVERAGED quantities of `spherical_cross_spectrum`: the
    anomaly correlation of the two fields restricted to total wavenumber n.  NaN where either power is 0.  Arguments as for
    `spherical_spectrum`.
    """
    out, skipped, lab = _sht(forecast, valid, lat, lat_axis, lon_axis, axis, truncation)
    with np.errstate(invalid='ignore', divide='ignore'):
        cor = out[2] / np.sqrt(out[0] * out[1])
    res = lab(cor, 'spherical_correlation')
    return (res, skipped) if return_count else res


# --------------------------------------------------------------------------------------------------------------------- #
# Spherical-harmonic analysis, synthesis and filtering
# --------------------------------------------------------------------------------------------------------------------- #
#
# The coefficients themselves, the inverse transform, and the chain analysis -> factor per degree -> synthesis: truncation to a
# coarser resolution (scale-separated verification: forecast_error(spherical_filter(f, cutoff=21), spherical_filter(v, cutoff=21))),
# the Laplacian and its inverse (height <-> vorticity), smoothing before a remap.  numpy inputs run on the host in float64 and
# return numpy; device tensors run through dlwpcs_sht_analysis / dlwpcs_sht_synthesis and return device tensors (float32 /
# complex64); neither path falls back to the other.  A field that holds a NaN or an infinity has NaN coefficients and comes back
# as a field of NaN.

_responses = {}             # (response bytes, device) -> float32 device vector


def _response_on(response, dev):
    """the float32 device copy of a host response, uploaded once per device (so that a later call can be captured)"""
    import torch
    if response is None or _is_tensor(response):
        return response
    r32 = np.ascontiguousarray(np.asarray(response, dtype=np.float64).reshape(-1).astype(np.float32))
    key = (r32.tobytes(), str(dev))
    hit = _responses.get(key)
    if hit is None:
        if torch.cuda.is_current_stream_capturing():
            from .. import _native as nat
            raise nat.NativeError('spherical_filter: first use of this response inside a graph capture (run it once eagerly first)')
        hit = _responses[key] = torch.from_numpy(r32).to(dev)
    return hit


_COEFFICIENT = [('coefficient', None)]         # the dim of packed coefficients that stands for the two grid dims; no coordinate


def _on_grid(coef, values, tr, name):
    """grid fields labelled like the coefficients `coef` they were synthesised from: 'lat' and 'lon' in place of the last dim"""
    grid = [('lat', tr.lat.copy()), ('lon', np.arange(tr.n_lon) * 360.0 / tr.n_lon)]
    return label(coef, values, name, drop=(len(coef.shape) - 1,), tail=grid)


def _analysis_host(x, la, lo, tr):
    """(complex128 coefficients (lead..., rows), int32 flags (lead...)) of the host array x"""
    arr = np.moveaxis(np.asarray(x, dtype=np.float64), (la, lo), (-2, -1))
    counted = np.isfinite(arr).all(axis=(-2, -1))
    coef = tr.coefficients(np.where(counted[..., None, None], arr, 0.0))
    coef[~counted] = complex(np.nan, np.nan)
    return coef, (~counted).astype(np.int32)


def spherical_analysis(x, lat=None, lat_axis=-2, lon_axis=-1, truncation=None, return_count=False):
    """
    The spherical-harmonic coefficients a_n^m of `x`, 0 <= m <= n <= truncation (DLWP/remap/spharm.py states the definitions).

    :param x: ndarray, device tensor or labelled array; grid axes, `lat` and `truncation` as for `spherical_spectrum`
    :param return_count: also return an int32 array (leading axes...) that holds 1 for a field with a NaN or an infinity
    :return: complex array (leading axes..., (T + 1)(T + 2) / 2) in the order of spharm.packed_row(m, n, T): complex128 numpy for
        host inputs, a complex64 device tensor for device inputs; a labelled input gives a Forecast whose last dim is
        'coefficient'.  A field that holds a NaN or an infinity has NaN coefficients.
    """
    la, lo, tr = _sht_grid(x, lat, lat_axis, lon_axis, truncation)
    if _on_device(x):
        from .. import ops as dops
        with device_scope(x):
            coef, flags = dops.spherical_analysis(device_f32(x), tr, lat_axis=la, lon_axis=lo, counts=True)
    else:
        coef, flags = _analysis_host(_host(x), la, lo, tr)
    res = label(x, coef, 'spherical_analysis', drop=(la, lo), tail=_COEFFICIENT)
    return (res, flags) if return_count else res


def _truncation_of_rows(rows):
    T = int(round((np.sqrt(8.0 * rows + 1.0) - 3.0) / 2.0))
    if T < 0 or (T + 1) * (T + 2) // 2 != rows:
        raise ValueError('%d coefficients per field are not (T + 1)(T + 2) / 2 for any truncation T' % rows)
    return T


def spherical_synthesis(coef, lat, n_lon, response=None):
    """
    The fields x[i, j] = sum_m c_m Re(e^{i m lon_j} sum_n r_n a_n^m Pbar_n^m(mu_i)) of the coefficients `coef`
    (leading axes..., (T + 1)(T + 2) / 2), as `spherical_analysis` returns them, on the latitudes `lat` (degrees) and n_lon longitudes.

    :param coef: complex ndarray, complex64 device tensor or labelled array (its last dim holds the coefficients)
    :param response: T + 1 real factors per degree (None: ones); see spharm.truncation_response, spharm.laplacian_response
    :return: (leading axes..., nlat, n_lon): float64 numpy for host inputs, a float32 device tensor for device inputs; a labelled
        input gives a Forecast with the dims 'lat' and 'lon' in place of the coefficient dim
    """
    if len(coef.shape) < 1:
        raise ValueError('the coefficients need an axis')
    T = _truncation_of_rows(int(coef.shape[-1]))
    tr = _spherical_transform(lat, n_lon, T)
    if response is not None and not _is_tensor(response) and np.asarray(response).size != T + 1:
        raise ValueError('a response of %d factors, truncation %d needs %d' % (np.asarray(response).size, T, T + 1))
    if _on_device(coef):
        import torch
        from .. import ops as dops
        with device_scope(coef) as dev:
            c = _raw(coef)
            out = dops.spherical_synthesis(c if c.dtype == torch.complex64 else c.to(torch.complex64), tr, _response_on(response, dev))
    else:
        out = tr.synthesis(_host(coef), None if response is None else _host(response))
    return _on_grid(coef, out, tr, 'spherical_synthesis')


def _filter(x, lat, lat_axis, lon_axis, truncation, response, name):
    """analysis, `response` (a function of the transform's truncation, or None) and synthesis back into x's shape and axis order"""
    la, lo, tr = _sht_grid(x, lat, lat_axis, lon_axis, truncation)
    T = tr.truncation
    r = response(T) if callable(response) else response
    if r is not None and not _is_tensor(r) and np.asarray(r).size != T + 1:
        raise ValueError('a response of %d factors, truncation %d needs %d' % (np.asarray(r).size, T, T + 1))
    nd = len(x.shape)
    lead_axes = [i for i in range(nd) if i not in (la, lo)]
    if _on_device(x):
        import torch
        from .. import ops as dops
        with device_scope(x) as dev:
            xt = device_f32(x)
            coef = dops.spherical_analysis(xt, tr, lat_axis=la, lon_axis=lo)
            # the result has x's shape and axis order, and longitude at unit stride whatever x's own layout
            order = [i for i in range(nd) if i != lo] + [lo]
            buf = torch.empty([int(xt.shape[i]) for i in order], dtype=torch.float32, device=dev)
            out = buf.permute([order.index(i) for i in range(nd)])
            dops.spherical_synthesis(coef, tr, _response_on(r, dev), out=out.permute(lead_axes + [la, lo]))
    else:
        coef, _ = _analysis_host(_host(x), la, lo, tr)
        out = np.moveaxis(tr.synthesis(coef, None if r is None else _host(r)), (-2, -1), (la, lo))
    return label(x, out, name)


def spherical_filter(x, lat=None, lat_axis=-2, lon_axis=-1, truncation=None, cutoff=None, response=None):
    """
    `x` with every spherical-harmonic degree n multiplied by a real factor: analysis up to `truncation`, the factor, synthesis.

    :param x: ndarray, device tensor or labelled array; grid axes, `lat` and `truncation` as for `spherical_spectrum`
    :param cutoff: keep the degrees n <= cutoff and drop the others (the field truncated to T`cutoff`)
    :param response: truncation + 1 real factors per degree (host array, or a float32 device vector for device inputs);
        `cutoff` and `response` are mutually exclusive, neither: the field band-limited to `truncation`
    :return: the filtered field with the shape, axis order and labels of `x`: float64 numpy for host inputs, a float32 device tensor
        for device inputs (four launches; after one eager call the call can be captured in a graph)
    """
    if cutoff is not None and response is not None:
        raise ValueError('cutoff and response are mutually exclusive')
    if cutoff is not None:
        from ..remap.spharm import truncation_response
        cut = int(cutoff)
        if cut < 0:
            raise ValueError('cutoff %d is negative' % cut)
        response = lambda T: truncation_response(T, cut)        # noqa: E731
    return _filter(x, lat, lat_axis, lon_axis, truncation, response, 'spherical_filter')


def spherical_laplacian(x, lat=None, lat_axis=-2, lon_axis=-1, truncation=None, radius=6371200., inverse=False):
    """
    The Laplacian of `x` on a sphere of `radius` metres, degree n multiplied by -n (n + 1) / radius^2 (height -> vorticity up to
    g / f); inverse=True: the inverse Laplacian, degree n >= 1 divided by that factor and the mean set to 0.  Arguments and
    result as for `spherical_filter`.
    """
    from ..remap.spharm import laplacian_response
    return _filter(x, lat, lat_axis, lon_axis, truncation, lambda T: laplacian_response(T, radius, inverse), 'spherical_laplacian')


# --------------------------------------------------------------------------------------------------------------------- #
# Vector spherical harmonics: winds, vorticity and divergence, gradients
# --------------------------------------------------------------------------------------------------------------------- #
#
# Winds from vorticity and divergence, vorticity and divergence from winds, and the gradient of a scalar, on a sphere of `radius`
# metres (DLWP/remap/spharm.py states the definitions).  numpy inputs run on the host in float64, device tensors through
# dlwpcs_sht_vector_synthesis / dlwpcs_sht_vector_analysis (float32 / complex64, device tensors come back); neither path falls
# back to the other.

def _uv_response(T, radius, dev=None):
    from ..remap.spharm import uv_response
    r = uv_response(T, radius)
    return r if dev is None else _response_on(r, dev)


def spherical_uv(vrt, div, lat, n_lon, radius=6371200.):
    """
    The wind (u, v) whose vorticity and divergence have the coefficients `vrt` and `div` (leading axes..., (T + 1)(T + 2) / 2), as
    `spherical_vrtdiv` returns them, on the latitudes `lat` (degrees) and n_lon longitudes: psi = lap^-1 vrt, chi = lap^-1 div,
    u = -dpsi/dphi / radius + dchi/dlambda / (radius cos), v = dpsi/dlambda / (radius cos) + dchi/dphi / radius.

    :param vrt, div: complex ndarrays, complex64 device tensors or labelled arrays of one shape; either may be None (taken as zero)
    :return: (u, v), each (leading axes..., nlat, n_lon): float64 numpy for host inputs, float32 device tensors for device inputs,
        Forecasts with the dims 'lat' and 'lon' in place of the coefficient dim for labelled inputs
    """
    if vrt is None and div is None:
        raise ValueError('spherical_uv: vorticity and divergence are both absent')
    first = vrt if vrt is not None else div
    if vrt is not None and div is not None and tuple(vrt.shape) != tuple(div.shape):
        raise ValueError('spherical_uv: vorticity %s and divergence %s must have one shape' % (tuple(vrt.shape), tuple(div.shape)))
    if len(first.shape) < 1:
        raise ValueError('the coefficients need an axis')
    T = _truncation_of_rows(int(first.shape[-1]))
    tr = _spherical_transform(lat, n_lon, T)
    if _on_device(*[c for c in (vrt, div) if c is not None]):
        import torch
        from .. import ops as dops
        with device_scope(first) as dev:
            cs = [None if c is None else (_raw(c) if _raw(c).dtype == torch.complex64 else _raw(c).to(torch.complex64)) for c in (vrt, div)]
            r = _uv_response(T, radius, dev)
            u, v = dops.spherical_vector_synthesis(cs[0], cs[1], tr, r, r)
    else:
        u, v = tr.uv_from_vrtdiv(None if vrt is None else _host(vrt), None if div is None else _host(div), radius)
    return _on_grid(first, u, tr, 'u'), _on_grid(first, v, tr, 'v')


def spherical_vrtdiv(u, v, lat=None, lat_axis=-2, lon_axis=-1, truncation=None, radius=6371200.):
    """
    The coefficients (vrt, div) of the vorticity and the divergence of the wind (u, v) on a sphere of `radius` metres.

    :param u, v: ndarrays, device tensors or labelled arrays of one shape; grid axes, `lat` and `truncation` as for
        `spherical_spectrum`
    :return: (vrt, div), complex (leading axes..., (T + 1)(T + 2) / 2) as `spherical_analysis` returns coefficients.  A field with
        a NaN or an infinity in u or in v has NaN coefficients in both.
    """
    _check_labels(u, v)
    if tuple(u.shape) != tuple(v.shape):
        raise ValueError('spherical_vrtdiv: u %s and v %s must have one shape' % (tuple(u.shape), tuple(v.shape)))
    la, lo, tr = _sht_grid(u, lat, lat_axis, lon_axis, truncation)
    if _on_device(u, v):
        from .. import ops as dops
        with device_scope(u, v) as dev:
            r = _response_on(np.full(tr.truncation + 1, 1.0 / float(radius)), dev)
            vrt, div = dops.spherical_vector_analysis(_dev_operand(u, dev), _dev_operand(v, dev), tr, r, lat_axis=la, lon_axis=lo)
    else:
        arrs = [np.moveaxis(np.asarray(_host(x), dtype=np.float64), (la, lo), (-2, -1)) for x in (u, v)]
        counted = np.isfinite(arrs[0]).all(axis=(-2, -1)) & np.isfinite(arrs[1]).all(axis=(-2, -1))
        arrs = [np.where(counted[..., None, None], x, 0.0) for x in arrs]
        vrt, div = tr.vrtdiv_from_uv(arrs[0], arrs[1], radius)
        vrt[~counted] = complex(np.nan, np.nan)
        div[~counted] = complex(np.nan, np.nan)
    return (label(u, vrt, 'vorticity', drop=(la, lo), tail=_COEFFICIENT),
            label(u, div, 'divergence', drop=(la, lo), tail=_COEFFICIENT))


def spherical_gradient(x, lat=None, lat_axis=-2, lon_axis=-1, truncation=None, radius=6371200.):
    """
    The gradient (dx/dlambda / (radius cos(phi)), dx/dphi / radius) of the scalar `x` on a sphere of `radius` metres: analysis up
    to `truncation`, then the vector synthesis of the potential chi = x.  Arguments as for `spherical_filter`; the two results
    have the shape, axis order and labels of `x`.
    """
    la, lo, tr = _sht_grid(x, lat, lat_axis, lon_axis, truncation)
    T = tr.truncation
    nd = len(x.shape)
    lead_axes = [i for i in range(nd) if i not in (la, lo)]
    if _on_device(x):
        import torch
        from .. import ops as dops
        with device_scope(x) as dev:
            xt = device_f32(x)
            coef = dops.spherical_analysis(xt, tr, lat_axis=la, lon_axis=lo)
            order = [i for i in range(nd) if i != lo] + [lo]
            outs = []
            for _ in range(2):
                buf = torch.empty([int(xt.shape[i]) for i in order], dtype=torch.float32, device=dev)
                outs.append(buf.permute([order.index(i) for i in range(nd)]))
            r = _response_on(np.full(T + 1, 1.0 / float(radius)), dev)
            dops.spherical_vector_synthesis(None, coef, tr, None, r, out_u=outs[0].permute(lead_axes + [la, lo]),
                                            out_v=outs[1].permute(lead_axes + [la, lo]))
    else:
        coef, _ = _analysis_host(_host(x), la, lo, tr)
        outs = [np.moveaxis(g, (-2, -1), (la, lo)) for g in tr.gradient(coef, radius)]
    return label(x, outs[0], 'gradient_lon'), label(x, outs[1], 'gradient_lat')
