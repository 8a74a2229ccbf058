"""
DLWP.barotropic.BarotropicModel on the device against its float64 host twin.  The allowance for N steps is not taken from the
device: it is four times the distance of sht_vector_ref.emulate_model -- the same step in sequential float32 on the host -- from
the twin (the factor allows for the device's different but fixed summation order).  Both numbers are printed.
"""
import datetime
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sht_ref as R          # noqa: E402
import sht_vector_ref as V   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
START = datetime.datetime(2000, 1, 1)
SETUPS = {'gauss': ('gauss', 32, 64, 21, 600.), 'clenshaw-curtis': ('clenshaw-curtis', 19, 36, 9, 900.)}
STEPS = (1, 2, 24)
_REFERENCES = {}


def _state(kind, nlat, L, batch):
    return np.stack([V.rossby_haurwitz(kind, nlat, L, shift=0.3 * b, K=V.RH['K'] * (1 + 0.02 * b)) for b in range(batch)]
                    ).astype(np.float32)


def _references(name, batch, steps, rc=0.04, dc=1e-4):
    """{step: (twin grids, allowance (vorticity, wind))}, computed once per setup: the float64 twin and 4 x the distance of the
    sequential-float32 emulation from it"""
    from DLWP.barotropic import BarotropicModel
    key = (name, batch, steps, rc, dc)
    if key not in _REFERENCES:
        kind, nlat, L, T, dt = SETUPS[name]
        z0 = _state(kind, nlat, L, batch)
        twin = BarotropicModel(z0.astype(np.float64), T, dt, START, robert_coefficient=rc, damping_coefficient=dc,
                               lat=R.latitudes(kind, nlat), field='vorticity')
        p = V.model_params(T, dt, rc, dc, 4, 6371200., 7.29e-5, kind, nlat)
        emul = V.emulate_model(z0, kind, p, steps)
        out = {}
        for s in range(1, max(steps) + 1):
            twin.step_forward()
            if s in steps:
                grids = (twin.vrt_grid.copy(), twin.u_grid.copy(), twin.v_grid.copy())
                out[s] = (grids, tuple(4.0 * e for e in V.relative_errors(emul[s], grids)))
        _REFERENCES[key] = out
    return _REFERENCES[key]


def _bits(t):
    t = t.detach()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().view(torch.int32).cpu().numpy()


@pytest.mark.parametrize('batch', [1, 33])
@pytest.mark.parametrize('name', sorted(SETUPS))
def test_model_against_its_twin(name, batch):
    from DLWP.barotropic import BarotropicModel
    kind, nlat, L, T, dt = SETUPS[name]
    ref = _references(name, batch, STEPS)
    z0 = torch.from_numpy(_state(kind, nlat, L, batch)).to(DEV)
    m = BarotropicModel(z0, T, dt, START, lat=R.latitudes(kind, nlat), field='vorticity')
    assert m.vrt_spec.dtype == torch.complex64 and m.vrt_grid.shape == (batch, nlat, L)
    done = 0
    for s in STEPS:
        m.run(s - done)
        done = s
        grids, allow = ref[s]
        err = V.relative_errors([g.cpu().numpy() for g in (m.vrt_grid, m.u_grid, m.v_grid)], grids)
        print('%s batch %d, %d steps: device - twin = (%.3g, %.3g), allowance 4 x emulation = (%.3g, %.3g)'
              % (name, batch, s, err[0], err[1], allow[0], allow[1]))
        assert err[0] <= allow[0] and err[1] <= allow[1]
    assert m.t == 24 * dt and m.valid_time == START + datetime.timedelta(seconds=24 * dt)
    psi = m.z_grid
    assert psi.shape == (batch, nlat, L) and psi.dtype == torch.float32
    back = m.get_vrt(psi)
    assert float((back - m.vrt_grid).abs().max()) <= 1e-4 * float(m.vrt_grid.abs().max())


def test_rossby_haurwitz_on_the_device():
    """144 steps without filter and damping: within the allowance of the twin, which is itself 1.5e-5 from the analytic wave"""
    from DLWP.barotropic import BarotropicModel
    kind, nlat, L, T, dt = SETUPS['gauss']
    ref = _references('gauss', 1, (144,), rc=0.0, dc=0.0)
    m = BarotropicModel(torch.from_numpy(_state(kind, nlat, L, 1)).to(DEV), T, dt, START, robert_coefficient=0.,
                        damping_coefficient=0., field='vorticity')
    m.run(144)
    grids, allow = ref[144]
    err = V.relative_errors([g.cpu().numpy() for g in (m.vrt_grid, m.u_grid, m.v_grid)], grids)
    exact = V.rossby_haurwitz(kind, nlat, L, shift=V.rossby_haurwitz_speed() * m.t)
    wave = np.abs(m.vrt_grid.cpu().numpy()[0] - exact).max() / np.abs(exact).max()
    print('Rossby-Haurwitz, 144 steps: device - twin = (%.3g, %.3g), allowance = (%.3g, %.3g); device - analytic wave = %.3g'
          % (err[0], err[1], allow[0], allow[1], wave))
    assert err[0] <= allow[0] and err[1] <= allow[1]


def test_captured_run_replays_the_eager_run():
    from DLWP.barotropic import BarotropicModel
    kind, nlat, L, T, dt = SETUPS['clenshaw-curtis']
    z0 = torch.from_numpy(_state(kind, nlat, L, 5)).to(DEV)
    lat = R.latitudes(kind, nlat)
    eager = BarotropicModel(z0, T, dt, START, lat=lat, field='vorticity').run(5)
    m = BarotropicModel(z0, T, dt, START, lat=lat, field='vorticity')
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.run(1)                                                         # one eager step: every workspace has its size
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                        # one stream: a single chain of launches
        before = torch.cuda.memory_allocated()                           # (inside: beginning a capture allocates on its own)
        m.run(4)
        assert torch.cuda.memory_allocated() == before, 'a captured run allocated'
    assert m.t == 5 * dt                                                 # the captured steps count once: the first replay runs them
    graph.replay()
    torch.cuda.synchronize()
    for a, b in ((m.vrt_spec, eager.vrt_spec), (m.vrt_spec_prev, eager.vrt_spec_prev), (m.vrt_grid, eager.vrt_grid),
                 (m.u_grid, eager.u_grid), (m.v_grid, eager.v_grid)):
        assert np.array_equal(_bits(a), _bits(b))
    graph.replay()                                                       # four more steps from where the state stands
    torch.cuda.synchronize()
    eager.run(4)
    assert np.array_equal(_bits(m.vrt_spec), _bits(eager.vrt_spec))
    assert m.t == 5 * dt and m.advance_time(4) is m                      # the model time is host state: the caller moves it
    assert m.t == eager.t == 9 * dt and m.valid_time == eager.valid_time and not m.first_step
    with pytest.raises(ValueError, match='negative'):
        m.advance_time(-1)


def test_streamfunction_state_on_the_device():
    """zeta_n^m = -n (n + 1) / a^2 psi_n^m applied to the packed coefficients: within the scalar analysis' bound times the
    factor, plus the rounding of the factor and of the product (2 u of the value), of the float64 twin"""
    import sht_synth_ref as S
    from DLWP.barotropic import BarotropicModel
    from DLWP.remap import spharm
    kind, nlat, L, T, dt = SETUPS['gauss']
    twin0 = BarotropicModel(_state(kind, nlat, L, 3).astype(np.float64), T, dt, START, field='vorticity')
    psi = twin0.z_grid.astype(np.float32)
    twin = BarotropicModel(psi.astype(np.float64), T, dt, START)
    m = BarotropicModel(torch.from_numpy(psi).to(DEV), T, dt, START)
    factor = np.abs(np.concatenate([spharm.laplacian_response(T)[k:] for k in range(T + 1)]))
    lim = factor * S.analysis_bound(psi.astype(np.float64), kind)[..., None] + 2 * V.EPS * np.abs(twin.vrt_spec)
    err = np.abs(m.vrt_spec.cpu().numpy().astype(np.complex128) - twin.vrt_spec)
    print('streamfunction state: largest |error| / bound = %.4f' % float((err / np.maximum(lim, 1e-300)).max()))
    assert (err <= lim).all()
    assert np.array_equal(_bits(m.vrt_spec), _bits(m.vrt_spec_prev))
    rel = V.relative_errors([g.cpu().numpy() for g in (m.vrt_grid, m.u_grid, m.v_grid)], (twin.vrt_grid, twin.u_grid, twin.v_grid))
    print('streamfunction state: grids (%.3g, %.3g) from the twin' % rel)


def test_model_built_inside_a_capture_is_refused():
    from DLWP._native import NativeError
    from DLWP.barotropic import BarotropicModel
    z0 = torch.from_numpy(_state('gauss', 12, 24, 1)).to(DEV)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(NativeError, match='capture'):
        with torch.cuda.graph(graph):
            BarotropicModel(z0, 7, 600., START, field='vorticity')
    torch.cuda.synchronize()
    with pytest.raises(TypeError, match='float32'):
        BarotropicModel(z0.double(), 7, 600., START, field='vorticity')
    m = BarotropicModel(z0[:0], 7, 600., START, field='vorticity').run(2)      # no runs: nothing is launched
    assert m.vrt_spec.shape == (0, 36)
