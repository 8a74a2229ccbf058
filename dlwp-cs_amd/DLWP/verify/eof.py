"""
Relations between the rows (times) of a series across space in DLWP.verify: the weighted pattern covariance between two sets of
fields, and empirical orthogonal functions with their principal components (NAO / PNA / annular-mode indices, the leading modes
of a height series, the projection of a forecast onto observed modes).
"""
import numpy as np

from ..labelled import axis_of, coord, device_f32, device_scope, host as _host, label, on_device as _on_device, raw as _raw
from .timeseries import _fit, regression_fitted, REGRESSION_MAX_TERMS

EOF_MAX_ROWS = 4096         # the eigenproblem is solved on the host: T^2 doubles are downloaded (2.9 s of eigh at T = 4096)
EOF_MAX_MODES = REGRESSION_MAX_TERMS - 1


# --------------------------------------------------------------------------------------------------------------------- #
# The Gram matrix of the weighted anomalies, on the device (dlwpcs_row_gram) or by the same rules in numpy
# --------------------------------------------------------------------------------------------------------------------- #

def _weight_root(weights, cshape, name):
    """None, or the float32 root of the weights scaled to sum 1 over the columns where they are given: evaluated in float64,
    rounded to float32 once.  A weight that is not finite stays so (its column is excluded)."""
    if weights is None:
        return None
    w = np.asarray(getattr(weights, 'values', weights), dtype=np.float64)
    try:
        w = np.broadcast_to(w, cshape)
    except ValueError:
        raise ValueError('%s: weights of shape %s do not broadcast against the columns %s' % (name, w.shape, tuple(cshape)))
    given = np.isfinite(w)
    if np.any(w[given] < 0.):
        raise ValueError('%s: weights must not be negative' % name)
    total = float(w[given].sum())
    if not total > 0.:
        raise ValueError('%s: the weights must have a positive sum' % name)
    with np.errstate(invalid='ignore'):
        return np.ascontiguousarray(np.sqrt(w / total), dtype=np.float32)


def _gram_host(a, b, r32, axis, center_a, center_b):
    """the definition of dlwpcs_row_gram on the host: float32 anomalies y = r (x - mean) rounded as on the device, their products
    summed by numpy in float64 (no claim to the bits).  (G / sum of the kept weights, columns kept, float32 mean of a, kept)"""
    A = np.moveaxis(np.asarray(a, dtype=np.float32), axis, 0)
    cshape = A.shape[1:]
    A = A.reshape(A.shape[0], -1)
    B = None if b is None else np.moveaxis(np.asarray(b, dtype=np.float32), axis, 0).reshape(b.shape[axis], -1)
    r = np.ones(A.shape[1], dtype=np.float32) if r32 is None else r32.reshape(-1)
    bad = ~np.isfinite(r)
    ys, mean_a = [], None
    with np.errstate(all='ignore'):
        for X, (own, given) in ((A, center_a), (B, center_b)):
            if X is None:
                continue
            bad |= ~np.isfinite(X).all(axis=0)
            if given is not None:
                m = np.asarray(given, dtype=np.float32).reshape(-1)
                bad |= np.isnan(m)
            elif own:
                m = (X.astype(np.float64).sum(axis=0) / float(max(X.shape[0], 1))).astype(np.float32)
            else:
                m = np.zeros(X.shape[1], dtype=np.float32)
            if mean_a is None:
                mean_a = m.copy()
            ys.append((r[None] * (X - m[None])).astype(np.float64))
    for y in ys:
        y[:, bad] = 0.
    G = ys[0] @ ys[-1].T
    norm = float((r.astype(np.float64) ** 2)[~bad].sum()) if r32 is not None else float((~bad).sum())
    mean_a[bad] = np.nan
    with np.errstate(all='ignore'):
        return G / norm, int((~bad).sum()), mean_a.reshape(cshape), (~bad).reshape(cshape)


def _gram_device(a, b, r32, axis, center_a, center_b):
    """the same through ops.row_gram: (float64 device tensor G / sum of the kept weights, int64 device scalar, float32 device
    mean of a, bool device mask of the columns kept, device weight root or None)"""
    import torch
    from .. import ops as dops
    dev = a.device

    def arg(own, given):
        if given is None:
            return bool(own)
        return given if _on_device(given) else torch.from_numpy(np.ascontiguousarray(given, dtype=np.float32)).to(dev)

    r = None if r32 is None else (r32 if _on_device(r32) else torch.from_numpy(r32).to(dev))
    G, nv, mu = dops.row_gram(a, b, weight_root=r, row_axis=axis, center=arg(*center_a), center_b=arg(*center_b), counts=True,
                              mean=True)
    kept = ~torch.isnan(mu)
    norm = nv.to(torch.float64) if r is None else (r.to(torch.float64) ** 2)[kept].sum()
    return G / norm, nv, mu, kept, r


def _pair(a, b, axis, name):
    """the raw values of a and b (both on the device or both on the host), the axis, the columns' shape"""
    va = _raw(a)
    axis = axis_of(a, 'time', explicit=axis)
    vb = None if b is None else _raw(b)
    dev = _on_device(va)
    if vb is not None:
        if _on_device(vb) != dev:
            raise ValueError('%s: both operands must be on the device or both on the host' % name)
        sa, sb = tuple(va.shape), tuple(vb.shape)
        if len(sa) != len(sb) or sa[:axis] + sa[axis + 1:] != sb[:axis] + sb[axis + 1:]:
            raise ValueError('%s: the operands %s and %s differ in more than axis %d' % (name, sa, sb, axis))
    if dev:
        va, vb = device_f32(va), None if vb is None else device_f32(vb)
    else:
        va, vb = _host(va), None if vb is None else _host(vb)
    sa = tuple(va.shape)
    return va, vb, axis, dev, sa[:axis] + sa[axis + 1:]


def pattern_covariance(a, b=None, weights=None, axis=None, center=True, ddof=1, return_count=False):
    """
    The (Ta, Tb) matrix of weighted covariances between the fields (rows along time) of `a` and those of `b` (None: of `a`):
    sum over the grid points of w (a[s] - mean_a)(b[t] - mean_b) / (Ta - ddof), each operand centred on its own time mean.

    :param a, b: `Forecast`s, numpy arrays or torch tensors of one shape but for the time axis.  Values on a HIP device are
        multiplied there (dlwpcs_row_gram: fp32 matrix cores, fp64 sums in a stated order) and the float64 result stays there;
        numpy values give float64 numpy by the same rules with numpy's sums.  Neither path falls back to the other.
    :param weights: None, or values >= 0 that broadcast against the shape without the time axis (cos(lat), cell areas).  They
        are scaled to sum 1 over the grid points kept; their root is rounded to float32 once.
    :param axis: the time axis, a position or a dim name; None: the 'time' dim of a labelled input, else axis 0
    :param center: True: subtract each operand's time mean; False: nothing
    :param return_count: also return the number of grid points kept.  A grid point is left out where a value of `a` or `b` is
        not finite or its weight is not given (NaN).
    """
    va, vb, axis, dev, cshape = _pair(a, b, axis, 'pattern_covariance')
    if not isinstance(center, (bool, np.bool_)):
        raise ValueError('pattern_covariance: center must be True or False')
    r32 = _weight_root(weights, cshape, 'pattern_covariance')
    dof = int(va.shape[axis]) - int(ddof)
    if dof < 1:
        raise ValueError('pattern_covariance: %d rows leave no degree of freedom at ddof = %d' % (va.shape[axis], ddof))
    if dev:
        with device_scope(va):
            G, nv = _gram_device(va, vb, r32, axis, (center, None), (center, None))[:2]
            G = G / float(dof)
    else:
        G, nv = _gram_host(va, vb, r32, axis, (center, None), (center, None))[:2]
        G = G / float(dof)
    return (G, nv) if return_count else G


# --------------------------------------------------------------------------------------------------------------------- #
# Empirical orthogonal functions
# --------------------------------------------------------------------------------------------------------------------- #

class EOFAnalysis(object):
    """
    The leading modes of a series (`eof_analysis`):

    eigenvalues (K,), variance_fraction (eigenvalue / total_variance), total_variance (the trace of the covariance matrix of the
    rows), n_valid (grid points kept), pcs (T, K) float64 numpy with unit variance, eofs: the regression maps of the series on the
    PCs in physical units (float32, a 'mode' dim where time stood, on the device when the series was, NaN at a grid point left
    out), mean: the time mean subtracted.
    """

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def _basis(self, pcs):
        return np.concatenate([np.ones((pcs.shape[0], 1)), pcs], axis=1) if self._centred else pcs

    def north_errors(self):
        """the sampling error of the eigenvalues by North et al.'s rule of thumb, eigenvalue * sqrt(2 / T)"""
        return self.eigenvalues * np.sqrt(2. / self.pcs_values.shape[0])

    @property
    def pcs_values(self):
        return np.asarray(_raw(self.pcs))

    def project(self, y, axis=None):
        """
        Pseudo-PCs (R, K) float64 of the R fields of `y` (the shape of the analysed series but for time): the weighted inner
        product of y - mean with each pattern over the eigenvalue, so that project(x) returns the PCs.  Grid points left out of
        the analysis stay out.  `y` lies where the analysed series lay (device or host).
        """
        vy = _raw(y)
        ax = axis_of(y, 'time', explicit=axis) if axis is not None or hasattr(y, 'dims') else self._axis
        dev = _on_device(vy)
        if dev != _on_device(_raw(self.eofs)):
            raise ValueError('project: the fields must lie where the analysed series lay (device or host)')
        ev, mv = _raw(self.eofs), _raw(self.mean)
        if ax != self._axis or tuple(vy.shape[:ax]) + tuple(vy.shape[ax + 1:]) != tuple(mv.shape):
            raise ValueError('project: fields of shape %s do not match the patterns %s' % (tuple(vy.shape), tuple(ev.shape)))
        given = (None, mv) if self._centred else (False, None)
        if dev:
            with device_scope(vy):
                G = _gram_device(device_f32(vy), ev, self._root, ax, given, (False, None))[0]
                G = G.cpu().numpy()
        else:
            G = _gram_host(_host(vy), ev, self._root, ax, given, (False, None))[0]
        p = G / self.eigenvalues[None, :]
        K = p.shape[1]
        if not hasattr(y, 'dims'):
            return p
        return label(y, p, 'pseudo_pcs', drop=tuple(i for i in range(len(y.dims)) if i != ax), tail=(('mode', np.arange(K)),))

    def reconstruct(self, n_modes=None):
        """the series rebuilt from the mean and the first `n_modes` modes (None: all kept): float32, NaN where a grid point was
        left out"""
        K = len(self.eigenvalues)
        n = K if n_modes is None else int(n_modes)
        if not 0 <= n <= K:
            raise ValueError('reconstruct: %d modes, the analysis kept %d' % (n, K))
        ev, mv = _raw(self.eofs), _raw(self.mean)
        ax = self._axis
        if _on_device(ev):
            import torch
            with device_scope(ev):
                parts = ([mv.unsqueeze(ax)] if self._centred else []) + [ev.narrow(ax, 0, n)]
                coef = torch.cat(parts, dim=ax)
        else:
            parts = ([np.expand_dims(mv, ax)] if self._centred else []) + [np.take(ev, np.arange(n), axis=ax)]
            coef = np.concatenate(parts, axis=ax)
        if coef.shape[ax] == 0:
            raise ValueError('reconstruct: nothing to rebuild from (no mean, no modes)')
        basis = self._basis(self.pcs_values[:, :n])
        out = _raw(regression_fitted(coef, basis, term_axis=ax))
        if not hasattr(self.eofs, 'dims'):
            return out
        return label(self.eofs, out, 'reconstruction', replace={ax: (self._time_dim, self._times)}, lat=True)


def eof_analysis(x, n_modes, weights=None, axis=None, center=True, ddof=1):
    """
    Empirical orthogonal functions of the series `x` along time: the eigenvectors of the weighted covariance matrix of its T
    fields (`pattern_covariance`), which the series is read for once on the device; the T x T eigenproblem is solved on the host
    in float64 on either path (T at most EOF_MAX_ROWS).  Modes come by descending eigenvalue, each PC signed so that its entry of
    largest magnitude (the first such) is positive.

    :param x: a `Forecast`, a numpy array or a torch tensor; values on a HIP device are analysed there and eofs, mean and what
        `reconstruct` gives stay there.  numpy values are analysed on the host by the same rules.
    :param n_modes: modes to keep, at most REGRESSION_MAX_TERMS - 1 = 15 and at most T - 1 when centred (T otherwise)
    :param weights: as for `pattern_covariance`
    :param center: True: analyse the anomalies from the time mean; False: the values as they are
    :param ddof: the covariance divides by T - ddof, and the PCs have unit variance in that sense
    :return: an `EOFAnalysis`
    """
    vx, _, axis, dev, cshape = _pair(x, None, axis, 'eof_analysis')
    if not isinstance(center, (bool, np.bool_)):
        raise ValueError('eof_analysis: center must be True or False')
    T = int(vx.shape[axis])
    K = int(n_modes)
    if T > EOF_MAX_ROWS:
        raise NotImplementedError('eof_analysis: %d rows, the row form serves at most %d' % (T, EOF_MAX_ROWS))
    most = min(EOF_MAX_MODES, T - 1 if center else T)
    if not 1 <= K <= most:
        raise ValueError('eof_analysis: n_modes = %d outside 1 .. %d' % (K, most))
    dof = T - int(ddof)
    if dof < 1:
        raise ValueError('eof_analysis: %d rows leave no degree of freedom at ddof = %d' % (T, ddof))
    r32 = _weight_root(weights, cshape, 'eof_analysis')
    if dev:
        with device_scope(vx):
            G, nv, mean, kept, root = _gram_device(vx, None, r32, axis, (center, None), (center, None))
            C = G.cpu().numpy() / float(dof)
            nv = int(nv.item())
    else:
        G, nv, mean, kept = _gram_host(vx, None, r32, axis, (center, None), (center, None))
        C, root = G / float(dof), r32
    if nv < 1:
        raise ValueError('eof_analysis: no grid point is kept (every column holds a value that is not finite)')
    lam, vec = np.linalg.eigh(C)
    order = np.argsort(-lam, kind='stable')[:K]
    lam, vec = lam[order], vec[:, order]
    lead = np.argmax(np.abs(vec), axis=0)
    vec = vec * np.where(vec[lead, np.arange(K)] < 0., -1., 1.)[None, :]
    pcs = vec * np.sqrt(float(dof))
    total = float(np.trace(C))

    basis = np.concatenate([np.ones((T, 1)), pcs], axis=1) if center else pcs
    coef = _raw(_fit(vx, np.ascontiguousarray(basis, dtype=np.float32), axis, 'propagate', None, False, 'eofs'))
    first = 1 if center else 0
    if dev:
        import torch
        with device_scope(vx):
            nan = torch.full((), float('nan'), dtype=torch.float32, device=coef.device)
            eofs = torch.where(kept.unsqueeze(axis), coef.narrow(axis, first, K), nan)
    else:
        eofs = np.where(np.expand_dims(kept, axis), np.take(coef, np.arange(first, first + K), axis=axis), np.float32(np.nan))
    labelled = hasattr(x, 'dims')
    time_dim = x.dims[axis] if labelled else 'time'
    times = coord(x, time_dim) if labelled and time_dim in getattr(x, 'coords', {}) else None
    modes = np.arange(K)
    return EOFAnalysis(
        eigenvalues=lam, variance_fraction=lam / total, total_variance=total, n_valid=nv,
        pcs=label(x, pcs, 'pcs', drop=tuple(i for i in range(len(x.dims)) if i != axis), tail=(('mode', modes),)) if labelled else pcs,
        eofs=label(x, eofs, 'eofs', replace={axis: ('mode', modes)}, lat=True),
        mean=label(x, mean, 'mean', drop=(axis,), lat=True),
        _axis=axis, _centred=bool(center), _root=root, _time_dim=time_dim, _times=times)
