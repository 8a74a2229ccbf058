"""
DLWP.barotropic.BarotropicModel on the host (float64): the analytic Rossby-Haurwitz wave, the time scheme against a literal
restatement, the snapshot generator's step counts, batches, the reference's attributes and the refusals.
"""
import datetime
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sht_ref as R             # noqa: E402
import sht_vector_ref as V      # noqa: E402

from DLWP.barotropic import BarotropicModel      # noqa: E402
from DLWP.remap import spharm   # noqa: E402

START = datetime.datetime(2000, 1, 1)


def test_rossby_haurwitz_wave_translates_at_the_analytic_speed():
    """wavenumber 4 on a 32 x 64 Gaussian grid at T = 21, dt = 600 s, 144 steps, no filter and no damping: the wave translated by
    nu t within 1e-4 (measured: 1.5e-5), and further than 0.5 from the untranslated wave (measured: 0.75)"""
    kind, nlat, L, T = 'gauss', 32, 64, 21
    m = BarotropicModel(V.rossby_haurwitz(kind, nlat, L), T, 600., START, robert_coefficient=0., damping_coefficient=0.,
                        field='vorticity')
    m.run(144)
    assert m.t == 86400. and m.valid_time == START + datetime.timedelta(days=1)
    exact = V.rossby_haurwitz(kind, nlat, L, shift=V.rossby_haurwitz_speed() * m.t)
    scale = np.abs(exact).max()
    err = np.abs(m.vrt_grid - exact).max() / scale
    still = np.abs(m.vrt_grid - V.rossby_haurwitz(kind, nlat, L)).max() / scale
    print('Rossby-Haurwitz after 24 h: %.3g from the translated wave, %.3g from the untranslated' % (err, still))
    assert err <= 1e-4
    assert still > 0.5


@pytest.mark.parametrize('kind,nlat,L,T', [('gauss', 16, 32, 10), ('clenshaw-curtis', 19, 36, 9), ('fejer', 20, 36, 9)])
def test_time_scheme_is_its_literal_restatement(kind, nlat, L, T):
    rng = np.random.default_rng(11)
    lat = R.latitudes(kind, nlat)
    z0 = np.stack([V.rossby_haurwitz(kind, nlat, L, shift=0.3 * b, K=V.RH['K'] * (1 + 0.2 * b)) for b in range(3)])
    z0 = z0 + 1e-6 * rng.standard_normal(z0.shape)
    dt, rc, dc, order, a, om = 900., 0.05, 2e-4, 3, 6371200., 7.29e-5
    m = BarotropicModel(z0, T, dt, START, robert_coefficient=rc, damping_coefficient=dc, damping_order=order, lat=lat,
                        field='vorticity')
    tr = spharm.SphericalTransform(lat, L, T)
    n = np.concatenate([np.arange(mm, T + 1) for mm in range(T + 1)]).astype(float)
    d = dc * (n * (n + 1) / (T * (T + 1))) ** order
    f = (2 * om * np.sin(np.radians(lat)))[:, None]
    zeta = prev = tr.coefficients(z0)
    assert np.array_equal(m.vrt_spec, zeta) and np.array_equal(m.vrt_spec_prev, zeta)
    for step in range(4):
        u, v = tr.uv_from_vrtdiv(zeta, None, a)
        g = tr.synthesis(zeta)
        assert np.array_equal(m.vrt_grid, g) and np.array_equal(m.u_grid, u) and np.array_equal(m.v_grid, v)
        tend = -tr.vrtdiv_from_uv((f + g) * u, (f + g) * v, a, want=('div',))[0]
        tend = (tend - d * prev) / (1 + d * dt)
        if step == 0:
            new = zeta + dt * tend
            zeta = zeta + rc * (new - zeta)
        else:
            zeta = zeta + rc * (prev - 2 * zeta)
            new = prev + 2 * dt * tend
            zeta = zeta + rc * new
        prev, zeta = zeta, new
        m.step_forward()
        scale = np.abs(zeta).max()
        assert np.abs(m.vrt_spec - zeta).max() <= 1e-13 * scale and np.abs(m.vrt_spec_prev - prev).max() <= 1e-13 * scale
        assert m.t == (step + 1) * dt
    # the runs of a batch are independent
    one = BarotropicModel(z0[1], T, dt, START, robert_coefficient=rc, damping_coefficient=dc, damping_order=order, lat=lat,
                          field='vorticity').run(4)
    assert np.abs(one.vrt_spec - m.vrt_spec[1]).max() <= 1e-13 * np.abs(one.vrt_spec).max()


def test_streamfunction_state_and_conversions():
    kind, nlat, L, T = 'gauss', 16, 32, 10
    a = 6371200.
    zeta = V.rossby_haurwitz(kind, nlat, L)
    m = BarotropicModel(zeta, T, 600., START, field='vorticity')
    psi = m.z_grid
    assert np.abs(m.get_vrt(psi) - zeta).max() <= 1e-12 * np.abs(zeta).max()
    assert np.abs(m.get_z(zeta) - psi).max() <= 1e-12 * np.abs(psi).max()
    # psi = -a^2 w mu + a^2 K mu cos^R cos(R lambda), whose mean is zero
    Rw, w, K = V.RH['R'], V.RH['w'], V.RH['K']
    mu = R.sin_lat(kind, nlat)[:, None]
    lam = 2 * np.pi * np.arange(L)[None, :] / L
    exact = -a * a * w * mu + a * a * K * mu * (1 - mu * mu) ** (Rw / 2) * np.cos(Rw * lam)
    assert np.abs(psi - exact).max() <= 1e-12 * np.abs(exact).max()
    m2 = BarotropicModel(psi, T, 600., START)                       # field='streamfunction'
    assert np.abs(m2.vrt_grid - zeta).max() <= 1e-12 * np.abs(zeta).max()
    assert np.abs(m2.u_grid - m.u_grid).max() <= 1e-11 * np.abs(m.u_grid).max()
    m2.run(3)
    m2.set_state(psi)
    assert m2.t == 0 and m2.first_step and np.abs(m2.vrt_grid - zeta).max() <= 1e-12 * np.abs(zeta).max()


def test_run_with_snapshots_counts_steps():
    kind, nlat, L, T = 'gauss', 8, 16, 5
    z = V.rossby_haurwitz(kind, nlat, L)
    m = BarotropicModel(z, T, 600., START, field='vorticity')
    assert list(m.run_with_snapshots(3600.)) == [600. * k for k in range(1, 7)]
    assert m.t == 3600.
    assert list(m.run_with_snapshots(3000., snapshot_start=4000., snapshot_interval=1200.)) == [4800., 6000.]
    assert m.t == 6600.                                               # ceil(3000 / 600) = 5 more steps
    assert list(m.run_with_snapshots(1000., snapshot_interval=1.)) == [7200., 7800.]      # an interval below dt is dt
    ref = BarotropicModel(z, T, 600., START, field='vorticity').run(13)
    assert np.array_equal(ref.vrt_spec, m.vrt_spec)


def test_refusals():
    z = np.zeros((8, 16))
    with pytest.raises(ValueError, match='field'):
        BarotropicModel(z, 5, 600., START, field='height')
    with pytest.raises(ValueError, match='longitudes'):
        BarotropicModel(z, 8, 600., START)
    with pytest.raises(ValueError, match='above'):
        BarotropicModel(np.zeros((8, 32)), 8, 600., START)
    with pytest.raises(ValueError, match='neither'):
        BarotropicModel(z, 3, 600., START, lat=np.linspace(-80., 80., 8))
    with pytest.raises(ValueError, match='latitudes'):
        BarotropicModel(z, 3, 600., START, lat=R.latitudes('gauss', 9))
    with pytest.raises(ValueError, match='axis'):
        BarotropicModel(np.zeros(16), 3, 600., START)
    m = BarotropicModel(z, 5, 600., START)
    with pytest.raises(ValueError, match='state'):
        m.set_state(np.zeros((2, 8, 16)))
    import torch
    from DLWP import _native as nat
    with pytest.raises(nat.NativeError):                                        # a host tensor: there is no fall-back
        BarotropicModel(torch.zeros((8, 16)), 5, 600., START)
