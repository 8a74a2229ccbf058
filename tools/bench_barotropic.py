#!/usr/bin/env python3
"""
The batched barotropic model and the two vector transforms on the device: what they cost.  One JSON line.

`DLWP.barotropic.BarotropicModel` on a clenshaw-curtis 181 x 360 grid at T = 90 for --runs independent runs (default 32 and 512):
steps per second of the device model (device events around --steps steps after two warm-up steps), and of the same step written
with the torch expressions tools/bench_sht_synthesis.py uses -- torch.fft.rfft / irfft and one torch.einsum per order m with the
same fp32 tables -- with the largest difference of the two states after those steps relative to the largest value.  Then
`ops.spherical_vector_analysis` and `ops.spherical_vector_synthesis` alone against their torch expressions: milliseconds (median of
--reps calls after one warm-up call) and the largest relative difference.
"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'dlwp-cs_amd')]

import numpy as np   # noqa: E402
import torch         # noqa: E402

NLAT, L, T = 181, 360, 90


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def _rel(a, b):
    a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


class TorchStep(object):
    """the model's step with torch expressions on the tables of the transform"""

    def __init__(self, model, dev):
        from DLWP.remap import spharm
        tr = model.transform
        self.starts = [spharm.packed_row(m, m, T) for m in range(T + 1)]
        tabs = tr.device_vector_tables(dev)[1:]
        cut = lambda t: [t[s:s + T + 1 - m, :NLAT].contiguous().to(torch.complex64) for m, s in enumerate(self.starts)]      # noqa: E731
        self.D, self.Q, self.wD, self.wQ = (cut(t) for t in tabs)
        self.P = cut(tr.device_synthesis_tables(dev)[1])
        self.f = model._d_f[None, :, None]
        self.damp, self.r_tend, self.r_uv = model._d_damp, model._d_r_tend, model._d_r_uv
        self.dt, self.rc = model.dt, model.robert_coefficient

    def analysis(self, u, v, resp, want=('vrt', 'div')):
        U = torch.fft.rfft(u, dim=-1)[..., :T + 1] / L
        V = torch.fft.rfft(v, dim=-1)[..., :T + 1] / L
        out = {w: [] for w in want}
        for m in range(T + 1):
            r = resp[m:]
            if 'vrt' in out:
                out['vrt'].append(r * (1j * torch.einsum('ni,fi->fn', self.wQ[m], V[..., m]) + torch.einsum('ni,fi->fn', self.wD[m], U[..., m])))
            if 'div' in out:
                out['div'].append(r * (1j * torch.einsum('ni,fi->fn', self.wQ[m], U[..., m]) - torch.einsum('ni,fi->fn', self.wD[m], V[..., m])))
        return tuple(torch.cat(out[w], dim=-1) for w in want)

    def uv(self, psi, resp):
        U = torch.zeros((psi.shape[0], NLAT, L // 2 + 1), dtype=psi.dtype, device=psi.device)
        V = torch.zeros_like(U)
        for m, s in enumerate(self.starts):
            a = psi[:, s:s + T + 1 - m] * resp[m:]
            U[..., m] = -torch.einsum('ni,fn->fi', self.D[m], a)
            V[..., m] = 1j * torch.einsum('ni,fn->fi', self.Q[m], a)
        return torch.fft.irfft(U * L, n=L, dim=-1), torch.fft.irfft(V * L, n=L, dim=-1)

    def scalar(self, coef):
        G = torch.zeros((coef.shape[0], NLAT, L // 2 + 1), dtype=coef.dtype, device=coef.device)
        for m, s in enumerate(self.starts):
            G[..., m] = torch.einsum('ni,fn->fi', self.P[m], coef[:, s:s + T + 1 - m])
        return torch.fft.irfft(G * L, n=L, dim=-1)

    def step(self, state, first):
        z, zp, g, u, v = state
        s = self.f + g
        tend, = self.analysis(s * u, s * v, self.r_tend, want=('div',))
        tend = (tend - self.damp * zp) / (1.0 + self.damp * self.dt)
        if first:
            new = z + self.dt * tend
            z = z + self.rc * (new - z)
        else:
            z = z + self.rc * (zp - 2.0 * z)
            new = zp + 2.0 * self.dt * tend
            z = z + self.rc * new
        u, v = self.uv(new, self.r_uv)
        return new, z, self.scalar(new), u, v


def _model_case(runs, steps, torch_steps, dev):
    from DLWP.barotropic import BarotropicModel
    lat = np.linspace(90., -90., NLAT)
    gen = torch.Generator(device=dev).manual_seed(5)
    phi = torch.deg2rad(torch.from_numpy(lat).float().to(dev))[None, :, None]
    lam = (2 * np.pi / L) * torch.arange(L, device=dev)[None, None, :]
    shift = 6.28 * torch.rand((runs, 1, 1), device=dev, generator=gen)
    z0 = 2 * 7.848e-6 * torch.sin(phi) - 7.848e-6 * 30 * torch.sin(phi) * torch.cos(phi) ** 4 * torch.cos(4 * (lam - shift))
    start = datetime.datetime(2000, 1, 1)
    m = BarotropicModel(z0.contiguous(), T, 600., start, lat=lat, field='vorticity')
    ts = TorchStep(m, dev)
    state = (m.vrt_spec.clone(), m.vrt_spec_prev.clone(), m.vrt_grid.clone(), m.u_grid.clone(), m.v_grid.clone())
    m.run(2)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    m.run(steps)
    e1.record()
    e1.synchronize()
    ours = e0.elapsed_time(e1) / steps
    state = ts.step(ts.step(state, True), False)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(torch_steps):
        state = ts.step(state, False)
    e1.record()
    e1.synchronize()
    theirs = e0.elapsed_time(e1) / torch_steps
    # the two states after the same number of steps
    cmp_model = BarotropicModel(z0.contiguous(), T, 600., start, lat=lat, field='vorticity').run(2 + torch_steps)
    return {'runs': runs, 'steps': steps, 'ms_per_step': round(ours, 3), 'steps_per_s': round(1e3 / ours, 1),
            'run_steps_per_s': round(1e3 * runs / ours, 1), 'torch_ms_per_step': round(theirs, 3),
            'torch_over_ours': round(theirs / ours, 2), 'max_rel_diff_vorticity': _rel(cmp_model.vrt_grid, state[2])}


def _transform_case(fields, reps, dev):
    from DLWP import ops
    from DLWP.barotropic import BarotropicModel
    lat = np.linspace(90., -90., NLAT)
    m = BarotropicModel(torch.zeros((1, NLAT, L), device=dev), T, 600., datetime.datetime(2000, 1, 1), lat=lat, field='vorticity')
    ts, tr = TorchStep(m, dev), m.transform
    gen = torch.Generator(device=dev).manual_seed(3)
    u = torch.randn((fields, NLAT, L), dtype=torch.float32, device=dev, generator=gen)
    v = torch.randn((fields, NLAT, L), dtype=torch.float32, device=dev, generator=gen)
    ones = torch.ones(T + 1, device=dev)
    psi = ops.spherical_vector_analysis(u, v, tr, want=('vrt',))[0]
    ou, ov = torch.empty_like(u), torch.empty_like(v)
    res = {'fields': fields}
    routes = {'vector_analysis': (lambda: ops.spherical_vector_analysis(u, v, tr), lambda: ts.analysis(u, v, ones)),
              'vector_analysis_div_only': (lambda: ops.spherical_vector_analysis(u, v, tr, want=('div',)),
                                           lambda: ts.analysis(u, v, ones, want=('div',))),
              'vector_synthesis_psi': (lambda: ops.spherical_vector_synthesis(psi, None, tr, out_u=ou, out_v=ov), lambda: ts.uv(psi, ones))}
    for name, (ours, theirs) in routes.items():
        ms, t_ms = _time(ours, reps), _time(theirs, reps)
        res[name] = {'ms': round(ms, 3), 'us_per_field': round(1e3 * ms / fields, 3), 'torch_ms': round(t_ms, 3),
                     'torch_over_ours': round(t_ms / ms, 2), 'max_rel_diff': _rel(ours()[0].clone(), theirs()[0])}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, nargs='+', default=[32, 512])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--torch-steps', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_barotropic: no HIP device (times are measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    out = {'device': torch.cuda.get_device_name(0), 'grid': [NLAT, L], 'T': T, 'model': [], 'transforms': []}
    for runs in a.runs:
        out['model'].append(_model_case(runs, a.steps, a.torch_steps, dev))
        torch.cuda.empty_cache()
        out['transforms'].append(_transform_case(runs, a.reps, dev))
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
