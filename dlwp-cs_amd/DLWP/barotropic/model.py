"""
A batched spectral barotropic vorticity model on the sphere.

The model integrates the non-divergent barotropic vorticity equation
    d zeta / dt = -div( (f + zeta) V ),      f = 2 omega sin(phi),
with the wind V = (u, v) of the streamfunction psi = lap^-1 zeta, by the spectral transform method on the grids of
DLWP.remap.spharm (Gaussian, equally spaced with both poles, equally spaced cell centres).  One step:
    tend  = -delta( (f + zeta) u, (f + zeta) v )                              (spectral divergence of the vorticity flux)
    d_n   = damping_coefficient (n (n + 1) / (T (T + 1)))^damping_order
    tend  = (tend - d_n zeta_prev) / (1 + d_n dt)
    first step:  new = zeta + dt tend,          zeta += rc (new - zeta)
    afterwards:  zeta += rc (zeta_prev - 2 zeta),  new = zeta_prev + 2 dt tend,  zeta += rc new        (leapfrog, Robert filter)
    zeta_prev = zeta,  zeta = new,  and u, v and the grid vorticity follow from the new zeta.
The quadratic product aliases unless 3 T + 1 <= nlon: choose T <= (nlon - 1) // 3 (T = nlon // 3 is the customary advice).

The leading dims of the state are independent runs.  A numpy state runs on the host in float64; a float32 device tensor runs on
the device -- per step dlwpcs_barotropic_flux, dlwpcs_sht_vector_analysis, dlwpcs_barotropic_update,
dlwpcs_sht_vector_synthesis and dlwpcs_sht_synthesis, one linear chain on the current stream with no host synchronisation and,
after one eager step, no allocation, so that a run of steps can be captured in a graph.  Neither path falls back to the other.
"""
import math
from datetime import timedelta

import numpy as np

from ..remap import spharm


def _is_device_tensor(z):
    try:
        import torch
    except ImportError:
        return False
    return isinstance(z, torch.Tensor)


class BarotropicModel(object):
    """
    :param z: (..., nlat, nlon) initial state: numpy (host, float64) or a float32 device tensor (device)
    :param truncation: the spectral truncation T (triangular)
    :param dt: time step in seconds
    :param start_time: datetime of the initial state
    :param robert_coefficient: the Robert time filter's coefficient rc
    :param damping_coefficient, damping_order: the scale-selective damping d_n
    :param lat: latitudes in degrees, any layout spharm recognises, either direction; None: Gaussian, north to south
    :param field: what `z` is: 'streamfunction' (zeta = lap z) or 'vorticity' (zeta = z)
    :param radius: the sphere's radius in metres;  omega: its rotation rate in 1 / s
    """

    def __init__(self, z, truncation, dt, start_time, robert_coefficient=0.04, damping_coefficient=1e-4, damping_order=4,
                 lat=None, field='streamfunction', radius=6371200., omega=7.29e-5):
        if field not in ('streamfunction', 'vorticity'):
            raise ValueError("BarotropicModel: field %r, 'streamfunction' or 'vorticity'" % (field,))
        if len(z.shape) < 2:
            raise ValueError('BarotropicModel: the state needs a latitude and a longitude axis')
        self.device = _is_device_tensor(z)
        if self.device:
            import torch
            from .. import ops
            ops.require_device(z, 'BarotropicModel')
            if z.dtype != torch.float32:
                raise TypeError('BarotropicModel: a device state must be float32, got %s' % z.dtype)
        self.nlat, self.nlon = int(z.shape[-2]), int(z.shape[-1])
        self.batch = tuple(int(e) for e in z.shape[:-2])
        if lat is None:
            lat = np.degrees(np.arcsin(spharm._nodes('gauss', self.nlat)[1]))
        self.transform = spharm.SphericalTransform(lat, self.nlon, int(truncation))
        if self.transform.nlat != self.nlat:
            raise ValueError('BarotropicModel: %d latitudes for a latitude axis of %d' % (self.transform.nlat, self.nlat))
        self.lat = self.transform.lat
        T = self.truncation = self.transform.truncation
        self.field = field
        self.radius, self.omega = float(radius), float(omega)
        self.dt = float(dt)
        self.robert_coefficient = float(robert_coefficient)
        n = np.arange(T + 1, dtype=np.float64)
        self.damping = float(damping_coefficient) * (n * (n + 1.0) / max(T * (T + 1.0), 1.0)) ** damping_order
        self.f = 2.0 * self.omega * np.sin(np.radians(self.lat))
        degree = np.concatenate([np.arange(m, T + 1) for m in range(T + 1)])
        self._damp_rows = self.damping[degree]
        self._r_tend = np.full(T + 1, -1.0 / self.radius)
        self._r_uv = spharm.uv_response(T, self.radius)
        self._r_z = spharm.laplacian_response(T, self.radius, inverse=True)
        self._r_vrt = spharm.laplacian_response(T, self.radius)
        self.start_time = start_time
        if self.device:
            self._device_setup(z.device)
        self.set_state(z)

    # ---- device plumbing ------------------------------------------------------------------------------------------ #

    def _device_setup(self, dev):
        import torch
        from .. import ops
        if torch.cuda.is_current_stream_capturing():
            raise ops.nat.NativeError('BarotropicModel: built inside a graph capture (build it and run one step eagerly first)')
        self._dev = dev
        up = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32))).to(dev)   # noqa: E731
        self._d_f, self._d_damp = up(self.f), up(self._damp_rows)
        self._d_r_tend, self._d_r_uv, self._d_r_z = up(self._r_tend), up(self._r_uv), up(self._r_z)
        self._d_r_vrt_rows = up(self._per_row(self._r_vrt))
        rows = spharm.packed_rows(self.truncation)
        grid = self.batch + (self.nlat, self.nlon)
        new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)        # noqa: E731
        self.vrt_spec, self.vrt_spec_prev = new(self.batch + (rows,), torch.complex64), new(self.batch + (rows,), torch.complex64)
        self._tend = new(self.batch + (rows,), torch.complex64)
        self.vrt_grid, self.u_grid, self.v_grid = new(grid, torch.float32), new(grid, torch.float32), new(grid, torch.float32)
        self._flux = (new(grid, torch.float32), new(grid, torch.float32))
        self._tables = self.transform.device_vector_tables(dev)
        self._stables = self.transform.device_synthesis_tables(dev)
        lead = self.batch
        strides = tuple(int(s) for s in self.vrt_grid.stride()[:-2])
        dims = ops.spectrum_dims(lead, [strides, strides], ())
        self._desc2 = ops.sht_desc(self.nlat, self.nlon, self.truncation, dims, (self.nlon, self.nlon))
        self._desc1 = ops.sht_synthesis_desc(self.nlat, self.nlon, self.truncation, ops.spectrum_dims(lead, [strides], ()), self.nlon)

    def _diagnose_device(self):
        """u, v and the grid vorticity of the spectral vorticity: the vector synthesis and the scalar synthesis"""
        import torch
        from .. import ops
        if not self.vrt_spec.numel():
            return
        zs = torch.view_as_real(self.vrt_spec)
        ops.sht_vector_synthesis_launch(self._desc2, zs, None, self._d_r_uv, None, self._tables, self.u_grid, self.v_grid)
        ops.sht_synthesis_launch(self._desc1, zs, None, self._stables[0], self._stables[1], self.vrt_grid)

    # ---- state ---------------------------------------------------------------------------------------------------- #

    def set_state(self, z):
        """Set the state from `z` (a streamfunction or a vorticity, as `field` says) and restart the time stepping: the spectral
        vorticity truncated to T, the grid vorticity and the wind consistent with it, zeta_prev = zeta, t = 0."""
        if tuple(int(e) for e in z.shape) != self.batch + (self.nlat, self.nlon):
            raise ValueError('BarotropicModel: a state of %s, the model holds %s' % (tuple(z.shape), self.batch + (self.nlat, self.nlon)))
        if _is_device_tensor(z) != self.device:
            raise TypeError('BarotropicModel: the state must stay on the %s' % ('device' if self.device else 'host'))
        tr = self.transform
        if self.device:
            import torch
            from .. import ops
            if z.dtype != torch.float32 or z.device != self._dev:
                raise TypeError('BarotropicModel: the state must be a float32 tensor on the device of the model')
            coef = ops.spherical_analysis(z, tr)
            if self.field == 'streamfunction':
                coef = coef * self._d_r_vrt_rows                # -n (n + 1) / radius^2 per packed row, as the host path
            self.vrt_spec.copy_(coef)
            self.vrt_spec_prev.copy_(coef)
            self._diagnose_device()
        else:
            coef = tr.coefficients(np.asarray(z, dtype=np.float64))
            if self.field == 'streamfunction':
                coef = coef * self._per_row(self._r_vrt)
            self.vrt_spec = coef
            self.vrt_spec_prev = coef.copy()
            self._diagnose_host()
        self.t = 0.0
        self.first_step = True

    def _per_row(self, r):
        T = self.truncation
        return np.asarray(r)[np.concatenate([np.arange(m, T + 1) for m in range(T + 1)])]

    def _diagnose_host(self):
        tr = self.transform
        self.u_grid, self.v_grid = tr.vector_synthesis(self.vrt_spec, None, self._r_uv, None)
        self.vrt_grid = tr.synthesis(self.vrt_spec)

    @property
    def valid_time(self):
        """the datetime of the current state"""
        return self.start_time + timedelta(seconds=self.t)

    @property
    def z_grid(self):
        """the streamfunction lap^-1 zeta of the current state (its mean is zero), synthesised on demand"""
        if self.device:
            from .. import ops
            return ops.spherical_synthesis(self.vrt_spec, self.transform, self._d_r_z)
        return self.transform.synthesis(self.vrt_spec, self._r_z)

    # ---- stepping ------------------------------------------------------------------------------------------------- #

    def step_forward(self):
        """one time step (the module's docstring states it)"""
        dt, rc = self.dt, self.robert_coefficient
        if self.device:
            import torch
            from .. import ops
            if self.vrt_spec.numel():
                ops.barotropic_flux(self.vrt_grid, self.u_grid, self.v_grid, self._d_f, self._flux[0], self._flux[1])
                ops.sht_vector_analysis_launch(self._desc2, self._flux[0], self._flux[1], self._d_r_tend, self._tables, None,
                                               torch.view_as_real(self._tend))
                ops.barotropic_update(self._tend, self.vrt_spec, self.vrt_spec_prev, self._d_damp, dt, rc, self.first_step)
                self._diagnose_device()
        else:
            s = self.f[:, None] + self.vrt_grid
            tend, = self.transform.vector_analysis(s * self.u_grid, s * self.v_grid, self._r_tend, want=('div',))
            d = self._damp_rows
            tend = (tend - d * self.vrt_spec_prev) / (1.0 + d * dt)
            z = self.vrt_spec
            if self.first_step:
                new = z + dt * tend
                z = z + rc * (new - z)
            else:
                z = z + rc * (self.vrt_spec_prev - 2.0 * z)
                new = self.vrt_spec_prev + 2.0 * dt * tend
                z = z + rc * new
            self.vrt_spec_prev, self.vrt_spec = z, new
            self._diagnose_host()
        self.first_step = False
        self.t += dt

    def run(self, steps):
        """`steps` time steps.  On the device, after one eager step, this allocates nothing and never synchronises: it can be
        captured in a graph and replayed.  `t`, `valid_time` and `first_step` live on the host: they advance while the steps are
        captured (the capture counts as having run them once the graph has been replayed), but a further replay moves the device
        state only -- call advance_time(steps) after each further replay."""
        for _ in range(int(steps)):
            self.step_forward()
        return self

    def advance_time(self, steps):
        """move the model time `t` (and with it `valid_time`) by `steps` time steps without touching the state: the host side of
        replaying a captured run(steps)"""
        steps = int(steps)
        if steps < 0:
            raise ValueError('BarotropicModel: advance_time(%d): the steps cannot be negative' % steps)
        if steps:
            self.first_step = False
        self.t += steps * self.dt
        return self

    def run_with_snapshots(self, run_time, snapshot_start=0, snapshot_interval=None):
        """A generator that advances the model by ceil(run_time / dt) steps and yields the model time `t` after every
        ceil(snapshot_interval / dt)-th of them (None: every step) once t > snapshot_start."""
        interval = max(float(snapshot_interval or self.dt), self.dt)
        steps = int(math.ceil(float(run_time) / self.dt - 1e-9))
        every = int(math.ceil(interval / self.dt - 1e-9))
        for n in range(1, steps + 1):
            self.step_forward()
            if self.t > snapshot_start and n % every == 0:
                yield self.t

    # ---- conversions ---------------------------------------------------------------------------------------------- #

    def get_z(self, vrt):
        """the streamfunction lap^-1 vrt of a grid vorticity (degree n divided by -n (n + 1) / radius^2, the mean set to 0)"""
        from .. import verify
        return verify.spherical_laplacian(vrt, lat=self.lat, truncation=self.truncation, radius=self.radius, inverse=True)

    def get_vrt(self, z):
        """the vorticity lap z of a grid streamfunction"""
        from .. import verify
        return verify.spherical_laplacian(z, lat=self.lat, truncation=self.truncation, radius=self.radius)
