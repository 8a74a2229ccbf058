"""
GPU tests of the streaming helper kernels (csrc/elementwise.hip), one case table per host entry point, called through the
C ABI (DLWP._native) so that forms DLWP/ops.py never produces are reachable: a null half of split2, a channel window inside a
wider row, a view that starts at an odd element offset.

Reference: tests/stream_ref.py (plain numpy, written from include/dlwpcs.h; checked against the fp64 oracle on the CPU by
tests/test_stream_ref.py).  The kernels are pure data movement or one fp32 expression with one rounding, so every comparison
is bitwise (np.array_equal on the raw element bits), as the convention in tests/test_gpu_bf16.py says.  Every output buffer
is pre-filled with a sentinel bit pattern, never left uninitialised, so an element a kernel skips cannot be right by accident.

Each case carries
  * `vec`: the storage vector the dispatcher picks for it ('H8' / 'H2' / 'bf16' / 'float4' / 'float' for arithmetic kernels,
    'u128' / 'u32' / 'u16' for movers).  The test recomputes it from the documented rule (stream_ref.vec_*) and asserts the
    field, and tests/test_stream_ref.py asserts on the CPU that each table names every reachable vector, so an edit of a
    table cannot silently lose a kernel instantiation;
  * `cls`: the size class, asserted from the work-item count (one work item = one storage vector of the tensor the kernel
    loops over): 'tiny' (less than one workgroup), 'ragged' (not a multiple of 256) and 'wrap' (more than two grid-stride
    sweeps plus a ragged third).

THE WRAP SIZES FOLLOW stream_grid()'s CAP of 2048 workgroups x 256 lanes = 524 288 work items per sweep (SWEEP below): they
have to grow with it if the cap is ever raised, or the wrap cases stop wrapping (the class assertion then fails).

The last section checks the bf16 activation-gradient mask against the PRE-activation (never against a device output), for
max_value that bf16 cannot represent.
"""
import numpy as np
import pytest
import torch

import stream_ref as R
from oracle import cs_oracle as orc

pytestmark = pytest.mark.gpu

SWEEP = 2048 * 256
DT = {'f32': torch.float32, 'bf16': torch.bfloat16}
IT = {'f32': torch.int32, 'bf16': torch.int16}
SENT = {'f32': -842150451, 'bf16': -12851}          # 0xCDCDCDCD / 0xCDCD: about -4.3e8 in either type
ALPHA, VMAX = 0.1, 10.0


def _dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch.device('cuda', 0)


def _nat():
    from DLWP import _native as nat
    return nat


def _tag(dt):
    nat = _nat()
    return nat.BF16 if dt == 'bf16' else nat.F32


def _call(name, *args):
    nat = _nat()
    nat.check(getattr(nat.lib(), 'dlwpcs_' + name)(*args, nat.stream_ptr()), name)
    torch.cuda.synchronize()


def _p(t):
    return 0 if t is None else t.data_ptr()


def _normal(rng, shape, dt, scale=1.0):
    """N(0, scale) rounded to the storage type; a large tensor repeats a block of prime length (the wrap cases are about where
    an element goes, and a prime period lines up with no row, face or sweep), which keeps the host's share of a case small"""
    n = int(np.prod(shape))
    block = R.store(rng.standard_normal(min(n, 1000003), dtype=np.float32) * np.float32(scale), dt)
    return np.resize(block, n).reshape(shape)


def _rand(rng, shape, dt, scale=1.0):
    """(stored values as float32 numpy, device tensor)"""
    a = _normal(rng, shape, dt, scale)
    return a, torch.from_numpy(a).to(DT[dt]).to(_dev())


def _to_dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DT[dt]).to(_dev())


def _out(shape, dt):
    t = torch.empty(shape, dtype=DT[dt], device=_dev())
    t.view(IT[dt]).fill_(SENT[dt])
    return t


def _bits(t):
    return t.contiguous().view(IT['bf16' if t.dtype == torch.bfloat16 else 'f32']).cpu().numpy()


def _ref_bits(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DT[dt]).view(IT[dt]).numpy()


def _same(out, ref, dt):
    return np.array_equal(_bits(out), _ref_bits(ref, dt).reshape(_bits(out).shape))


def _untouched(t):
    dt = 'bf16' if t.dtype == torch.bfloat16 else 'f32'
    return bool((t.view(IT[dt]) == SENT[dt]).all().item())


def _id(case):
    return '-'.join('%s' % (v,) for v in case.values())


# ------------------------------------------------------------------------------------------------------------------ #
# case tables.  Channel counts per (dtype, storage vector): three vectors per pixel, so that the wrap cases split rows.
# A spatial kernel loops over a grid of B * 6 * G * G pixels: tiny G = 2 (B = 1: 72 items), ragged G = 10 (B = 3: 5400 items),
# wrap G = 172 (B = 2: 1 065 024 items = two sweeps + 16 448).
# ------------------------------------------------------------------------------------------------------------------ #
ARITH_C = {('bf16', 'H8'): 24, ('bf16', 'H2'): 6, ('bf16', 'bf16'): 3, ('f32', 'float4'): 12, ('f32', 'float'): 3}
MOVER_C = {('bf16', 'u128'): 24, ('bf16', 'u32'): 6, ('bf16', 'u16'): 3, ('f32', 'u128'): 12, ('f32', 'u32'): 3}
GRIDS = (('tiny', 1, 2), ('ragged', 3, 10), ('wrap', 2, 172))


def _cls(items):
    """size class of a hand-written extra case (the three classes every kernel must see come from GRIDS, spelled out)"""
    assert items < 256 or items % 256 != 0, items
    return 'tiny' if items < 256 else 'ragged'


def _spatial(chan, n_of_grid, grid_of_n, extra=()):
    """GRIDS x every (dtype, vector) of `chan`, plus extra (dtype, vec, B, N, C) cases; n_of_grid / grid_of_n translate between
    the face size N of the call and the grid the kernel loops over"""
    out = []
    for (dt, vec), C in chan.items():
        for cls, B, G in GRIDS:
            out.append(dict(dt=dt, vec=vec, cls=cls, B=B, N=n_of_grid(G), C=C))
    for dt, vec, B, N, C in extra:
        w = R.vec_width(vec) if vec in ('H8', 'H2', 'bf16', 'float4', 'float') else {'u128': 16, 'u32': 4, 'u16': 2}[vec] // R.esize(dt)
        out.append(dict(dt=dt, vec=vec, cls=_cls(B * 6 * grid_of_n(N) ** 2 * C // w), B=B, N=N, C=C))
    return out


# the U-Net's own channel counts and the ones the older tests used, at a face size that is not a power of two: (.., B, N, C)
_ARITH_EXTRA = [('bf16', 'H8', 1, 6, 64), ('bf16', 'H8', 3, 6, 8), ('bf16', 'H8', 2, 6, 32), ('bf16', 'H2', 3, 6, 12),
                ('bf16', 'H2', 1, 6, 2), ('bf16', 'bf16', 3, 6, 1), ('bf16', 'bf16', 1, 6, 7), ('f32', 'float4', 3, 6, 4),
                ('f32', 'float4', 1, 6, 20), ('f32', 'float4', 2, 6, 8), ('f32', 'float', 3, 6, 1), ('f32', 'float', 1, 6, 6),
                ('f32', 'float', 3, 6, 5)]
_ODD = [(d, v, B, N - 1, C) for d, v, B, N, C in _ARITH_EXTRA]                  # N = 5: where odd faces are allowed

POOL_FWD = _spatial(ARITH_C, lambda g: 2 * g, lambda n: n // 2, _ARITH_EXTRA + [('bf16', 'H8', 1, 2, 8), ('f32', 'float', 1, 2, 3)])
POOL_BWD = _spatial(ARITH_C, lambda g: g, lambda n: n, _ARITH_EXTRA + [('bf16', 'H2', 1, 2, 2), ('f32', 'float4', 1, 2, 4)])
POOL_BWD_ADD = [dict(c, alias=a) for c in _spatial(ARITH_C, lambda g: g, lambda n: n, _ARITH_EXTRA)
                for a in ((False,) if c['cls'] == 'wrap' else (False, True))]          # alias: dx is dskip
UP_BWD = _spatial(ARITH_C, lambda g: g, lambda n: n, _ODD + [('bf16', 'H8', 1, 1, 8), ('f32', 'float', 1, 1, 3),
                                                            ('bf16', 'bf16', 2, 9, 3)])
UP_FWD = _spatial(MOVER_C, lambda g: g // 2, lambda n: 2 * n,
                  [('bf16', 'u32', 3, 5, 10), ('bf16', 'u16', 2, 7, 5), ('bf16', 'u128', 1, 3, 32), ('f32', 'u128', 3, 5, 8),
                   ('f32', 'u32', 2, 7, 7), ('f32', 'u32', 1, 1, 1), ('bf16', 'u16', 1, 1, 1)])
# p = 1: pad_fwd loops over the padded grid (N + 2), pad_bwd over the face
PAD_FWD = _spatial(MOVER_C, lambda g: max(g - 2, 1), lambda n: n + 2, [('bf16', 'u128', 2, 4, 64), ('f32', 'u32', 2, 5, 7)])
PAD_BWD = _spatial(ARITH_C, lambda g: g, lambda n: n, _ODD)
# masked pooling adjoint: skip = dskip given / null; C = 12 is float4 in fp32 and H2 in bf16
POOL_MASKED = [dict(c, skip=k) for c in _spatial(ARITH_C, lambda g: g, lambda n: n,
                                                 [('f32', 'float4', 3, 6, 12), ('bf16', 'H2', 3, 6, 12), ('bf16', 'H8', 1, 10, 64),
                                                  ('f32', 'float', 2, 6, 6), ('bf16', 'bf16', 2, 6, 5)])
               for k in ((True,) if c['cls'] == 'wrap' else (True, False))] + \
              [dict(dt='bf16', vec='H8', cls='wrap', B=2, N=172, C=24, skip=False),
               dict(dt='f32', vec='float4', cls='wrap', B=2, N=172, C=12, skip=False)]

# concat2 / split2: (dtype, vec, class, rows, Ca, Cb); `only` (split2): which halves are asked for
_CAT = [('bf16', 'u128', 'tiny', 5, 8, 16), ('bf16', 'u128', 'ragged', 601, 8, 16), ('bf16', 'u128', 'wrap', 355011, 8, 16),
        ('bf16', 'u32', 'tiny', 7, 8, 12), ('bf16', 'u32', 'ragged', 601, 8, 12), ('bf16', 'u32', 'wrap', 213011, 8, 12),
        ('bf16', 'u32', 'ragged', 333, 2, 6), ('bf16', 'u16', 'tiny', 9, 8, 3), ('bf16', 'u16', 'ragged', 601, 8, 3),
        ('bf16', 'u16', 'wrap', 97011, 8, 3), ('bf16', 'u16', 'ragged', 601, 3, 5), ('bf16', 'u16', 'ragged', 77, 1, 1),
        ('f32', 'u128', 'tiny', 5, 8, 12), ('f32', 'u128', 'ragged', 601, 8, 12), ('f32', 'u128', 'wrap', 213011, 8, 12),
        ('f32', 'u128', 'ragged', 333, 4, 4), ('f32', 'u32', 'tiny', 9, 8, 3), ('f32', 'u32', 'ragged', 601, 8, 3),
        ('f32', 'u32', 'wrap', 97011, 8, 3), ('f32', 'u32', 'ragged', 601, 3, 5), ('f32', 'u32', 'ragged', 77, 1, 1)]
CONCAT = [dict(dt=d, vec=v, cls=c, rows=r, Ca=a, Cb=b) for d, v, c, r, a, b in _CAT]
SPLIT = [dict(c, only=o) for c in CONCAT for o in (('ab',) if c['cls'] == 'wrap' else ('ab', 'a', 'b'))]

# raw-word kernels: (dtype, vec, class, rows, C, Cp)
_CHP = [(d, v, c, r, C, Cp) for d, v in (('bf16', 'u16'), ('f32', 'u32'))
        for c, r, C, Cp in (('tiny', 6, 3, 8), ('tiny', 3, 8, 8), ('ragged', 601, 7, 8), ('ragged', 600, 12, 16),
                            ('ragged', 101, 1, 32), ('wrap', 213011, 5, 8))]
CHAN_PAD = [dict(dt=d, vec=v, cls=c, rows=r, C=C, Cp=Cp) for d, v, c, r, C, Cp in _CHP]
# state_repack: (T, V, E) x (B, S)
REPACK = [dict(dt=d, vec=v, cls=c, B=B, S=S, T=T, V=V, E=E) for d, v in (('bf16', 'u16'), ('f32', 'u32'))
          for c, B, S, T, V, E in (('tiny', 1, 24, 1, 4, 1), ('ragged', 2, 150, 1, 4, 1), ('ragged', 2, 150, 2, 7, 1),
                                   ('tiny', 1, 6, 2, 7, 1), ('ragged', 3, 150, 2, 13, 3), ('tiny', 1, 7, 2, 13, 3),
                                   ('ragged', 2, 150, 3, 1, 2), ('tiny', 1, 24, 3, 1, 2), ('wrap', 2, 6 * 53 * 53, 2, 13, 3))]
# layout converters: C and S below, equal to and not a multiple of the 32 x 32 tile, and a full-size face
TRANSPOSE = [dict(dt=d, vec=v, B=B, C=C, S=S) for d, v in (('bf16', 'u16'), ('f32', 'u32'))
             for B, C, S in ((1, 3, 24), (2, 32, 32), (2, 32, 150), (3, 7, 32), (2, 33, 96), (1, 70, 600), (2, 31, 31),
                             (1, 64, 64), (2, 18, 6 * 96 * 96))]

# flat kernels: (dtype, vec, class, n, element offset of the view); n % 8 in {1, 7} (bf16) / n % 4 in {1, 3} (fp32) for the
# scalar tails, at a tiny and at a wrap size; offsets 1 and 3 start the view off a 16-B boundary (scalar instantiation)
_WV = 2 * SWEEP + 16448
FLAT = [dict(dt=d, vec=v, cls=c, n=n, off=o) for d, v, c, n, o in (
    ('bf16', 'H8', 'tiny', 1, 0), ('bf16', 'H8', 'tiny', 7, 0), ('bf16', 'H8', 'tiny', 8, 0), ('bf16', 'H8', 'tiny', 8 * 9 + 1, 0),
    ('bf16', 'H8', 'tiny', 8 * 30 + 7, 0), ('bf16', 'H8', 'ragged', 8 * 1001 + 5, 0), ('bf16', 'H8', 'ragged', 8 * 3000, 0),
    ('bf16', 'H8', 'wrap', 8 * _WV + 1, 0), ('bf16', 'H8', 'wrap', 8 * _WV + 7, 0), ('bf16', 'H8', 'tiny', 8 * 9 + 1, 8),
    ('bf16', 'bf16', 'tiny', 8 * 9 + 1, 1), ('bf16', 'bf16', 'tiny', 8 * 9 + 7, 3), ('bf16', 'bf16', 'ragged', 8 * 1001 + 5, 1),
    ('bf16', 'bf16', 'wrap', _WV, 3), ('bf16', 'bf16', 'ragged', 8 * 1001, 4),
    ('f32', 'float4', 'tiny', 1, 0), ('f32', 'float4', 'tiny', 3, 0), ('f32', 'float4', 'tiny', 4, 0), ('f32', 'float4', 'tiny', 4 * 9 + 1, 0),
    ('f32', 'float4', 'tiny', 4 * 30 + 3, 0), ('f32', 'float4', 'ragged', 4 * 1001 + 2, 0), ('f32', 'float4', 'ragged', 4 * 3000, 0),
    ('f32', 'float4', 'wrap', 4 * _WV + 1, 0), ('f32', 'float4', 'wrap', 4 * _WV + 3, 0), ('f32', 'float4', 'tiny', 4 * 9 + 1, 4),
    ('f32', 'float', 'tiny', 4 * 9 + 1, 1), ('f32', 'float', 'tiny', 4 * 9 + 3, 3), ('f32', 'float', 'ragged', 4 * 1001 + 2, 1),
    ('f32', 'float', 'wrap', _WV, 3), ('f32', 'float', 'ragged', 4 * 1001, 2))]

# batch gather: kern = the kernel the call is there for.  S: 96 (one partial tile), 6*48*48 (54 full 256-pixel tiles), 600
# (S % 4 == 0, ragged last tile of both sizes), 150 (S % 4 != 0: 64-pixel kernel, ragged).  win = (Ctot, c_off, c_stride) or None
# for "the gathered channels are the output row".
_G = []
for _dt in ('f32', 'bf16'):
    for _S in (96, 6 * 48 * 48, 600, 150):
        _rows = 'rows' if _S % 4 == 0 else 'tile'
        _G += [(_dt, _rows, _S, 4, 2, None, 1), (_dt, _rows if _dt == 'f32' else 'tile', _S, 3, 1, None, 1),
               (_dt, 'tile', _S, 3, 2, (11, 2, 4), 1), (_dt, 'cf', _S, 3, 2, (11, 2, 4), 0), (_dt, 'cf', _S, 4, 2, None, 0)]
    _G += [(_dt, 'rows', 600, 7, 2, None, 1), (_dt, 'rows', 600, 2, 3, (6, 0, 2), 1), (_dt, 'tile', 600, 2, 3, (7, 0, 2), 1),
           (_dt, 'tile', 600, 2, 3, (8, 1, 2), 1), (_dt, 'rows', 600, 1, 2, None, 1), (_dt, 'tile', 150, 1, 1, None, 1)]
GATHER = [dict(dt=d, kern=k, S=S, nv=nv, steps=st, win=w, cl=cl) for d, k, S, nv, st, w, cl in _G]

# the storage vectors each entry point can reach (tests/test_stream_ref.py: every table names all of them)
_ARITH_SET = {'H8', 'H2', 'bf16', 'float4', 'float'}
_MOVER_SET = {'u128', 'u32', 'u16'}
_FLAT_SET = {'H8', 'bf16', 'float4', 'float'}
_WORD_SET = {'u16', 'u32'}


def _arith(grid_of_n):
    return (lambda c: R.vec_arith(c['dt'], c['C']),
            lambda c: c['B'] * 6 * grid_of_n(c['N']) ** 2 * c['C'] // R.vec_width(c['vec']))


def _mover(grid_of_n):
    return (lambda c: R.vec_mover(c['dt'], c['C']),
            lambda c: R.mover_items(c['dt'], c['vec'], c['B'] * 6 * grid_of_n(c['N']) ** 2 * c['C']))


_CATR = (lambda c: R.vec_mover(c['dt'], c['Ca'], c['Cb']), lambda c: R.mover_items(c['dt'], c['vec'], c['rows'] * (c['Ca'] + c['Cb'])))
_FLATR = (lambda c: R.vec_flat(c['dt'], c['off'] * R.esize(c['dt'])), lambda c: max(c['n'] // R.vec_width(c['vec']), 1))
_WORD = lambda c: R.vec_word(c['dt'])                                                                     # noqa: E731
# entry point -> (case table, reachable vectors, documented rule for the vector, work items of a case or None: no sweep)
TABLES = {
    'pad_fwd': (PAD_FWD, _MOVER_SET) + _mover(lambda n: n + 2),
    'pad_bwd': (PAD_BWD, _ARITH_SET) + _arith(lambda n: n),
    'act_fwd': (FLAT, _FLAT_SET) + _FLATR, 'act_bwd': (FLAT, _FLAT_SET) + _FLATR, 'add': (FLAT, _FLAT_SET) + _FLATR,
    'avgpool2_fwd': (POOL_FWD, _ARITH_SET) + _arith(lambda n: n // 2),
    'avgpool2_bwd': (POOL_BWD, _ARITH_SET) + _arith(lambda n: n),
    'avgpool2_bwd_add': (POOL_BWD_ADD, _ARITH_SET) + _arith(lambda n: n),
    'avgpool2_bwd_masked': (POOL_MASKED, _ARITH_SET) + _arith(lambda n: n),
    'upsample2_fwd': (UP_FWD, _MOVER_SET) + _mover(lambda n: 2 * n),
    'upsample2_bwd': (UP_BWD, _ARITH_SET) + _arith(lambda n: n),
    'concat2': (CONCAT, _MOVER_SET) + _CATR, 'split2': (SPLIT, _MOVER_SET) + _CATR,
    'pad_channels': (CHAN_PAD, _WORD_SET, _WORD, lambda c: c['rows'] * c['Cp']),
    'slice_channels': (CHAN_PAD, _WORD_SET, _WORD, lambda c: c['rows'] * c['C']),
    'state_repack': (REPACK, _WORD_SET, _WORD, lambda c: c['B'] * c['S'] * c['T'] * (c['V'] + c['E'])),
    'cf_to_cl': (TRANSPOSE, _WORD_SET, _WORD, None), 'cl_to_cf': (TRANSPOSE, _WORD_SET, _WORD, None),
}
GATHER_KERNELS = {'rows', 'tile', 'cf'}


def check_case(entry, case):
    """the case's `vec` is what the documented rule gives and its `cls` is what the work-item count gives (no device needed)"""
    _, _, vec_rule, items = TABLES[entry]
    assert case['vec'] == vec_rule(case), (entry, case, vec_rule(case))
    if items is None:
        return
    n, cls = items(case), case['cls']
    if cls == 'tiny':
        assert n < 256, (entry, case, n)
    elif cls == 'ragged':
        assert n % 256 != 0, (entry, case, n)
    else:
        assert cls == 'wrap' and n > 2 * SWEEP and n % SWEEP != 0, (entry, case, n)


def gather_rule(case):
    nch = case['nv'] * case['steps']
    Ctot, c_off, c_stride = case['win'] if case['win'] else (nch, 0, case['nv'])
    return R.gather_kernel(case['dt'], case['S'], case['nv'], case['steps'], Ctot, c_off, c_stride, case['cl'])


# ------------------------------------------------------------------------------------------------------------------ #
# padding layer
# ------------------------------------------------------------------------------------------------------------------ #

def _tables(N, p, inverse=True):
    """oracle table and library inverse table on the host, both on the device"""
    nat = _nat()
    t_host = orc.halo_table(N, p)
    assert np.array_equal(nat.halo_table_host(N, p), t_host)
    inv_host = inv_dev = None
    if inverse:
        inv_host = nat.halo_inverse_table_host(N, p)
        assert np.array_equal(inv_host, R.inverse_table(t_host, N, p))
        inv_dev = torch.from_numpy(inv_host).to(_dev())
    return t_host, inv_host, torch.from_numpy(t_host).to(_dev()), inv_dev


def _pad_fwd(dt, B, N, C, p, rng):
    t_host, _, t_dev, _ = _tables(N, p, inverse=False)
    x, xd = _rand(rng, (B, 6, N, N, C), dt)
    y = _out((B, 6, N + 2 * p, N + 2 * p, C), dt)
    _call('pad_fwd', _p(xd), _p(y), B, N, C, p, _tag(dt), _p(t_dev))
    assert _same(y, R.pad_fwd(x, t_host), dt), (dt, B, N, C, p)


def _pad_bwd(dt, B, N, C, p, rng):
    t_host, inv_host, _, inv_dev = _tables(N, p)
    M = N + 2 * p
    dy, dyd = _rand(rng, (B, 6, M, M, C), dt)
    dx = _out((B, 6, N, N, C), dt)
    _call('pad_bwd', _p(dyd), _p(dx), B, N, C, p, _tag(dt), _p(inv_dev))
    assert _same(dx, R.pad_bwd(dy, N, p, inv_host, dt), dt), (dt, B, N, C, p)


@pytest.mark.parametrize('case', PAD_FWD, ids=_id)
def test_pad_fwd(case):
    check_case('pad_fwd', case)
    dt, B, N, C = case['dt'], case['B'], case['N'], case['C']
    _pad_fwd(dt, B, N, C, 1, np.random.default_rng(N + C))


@pytest.mark.parametrize('case', PAD_BWD, ids=_id)
def test_pad_bwd(case):
    check_case('pad_bwd', case)
    dt, B, N, C = case['dt'], case['B'], case['N'], case['C']
    _pad_bwd(dt, B, N, C, 1, np.random.default_rng(N + C + 1))


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('N', [1, 3, 9])
def test_pad_odd_faces_every_halo_width(N, dt):
    """every halo width 0..3 the table builders accept for an odd face (the inverse table refuses a fan-out above 5: the adjoint
    is run where it exists), all storage vectors"""
    nat = _nat()
    fwd, bwd = [], []
    for p in range(4):
        try:
            nat.halo_table_host(N, p)
        except ValueError:
            continue
        fwd.append(p)
        try:
            nat.halo_inverse_table_host(N, p)
            bwd.append(p)
        except ValueError:
            pass
        for C in sorted(set(c for (d, _), c in list(ARITH_C.items()) + list(MOVER_C.items()) if d == dt) | {1, 8, 5}):
            _pad_fwd(dt, 2, N, C, p, np.random.default_rng(100 * N + 10 * p + C))
            if p in bwd:
                _pad_bwd(dt, 2, N, C, p, np.random.default_rng(100 * N + 10 * p + C + 7))
    assert fwd == [p for p in range(4) if p <= N], fwd                    # the documented domain of dlwpcs_halo_table
    assert bwd == {1: [0], 3: [0, 1], 9: [0, 1, 2, 3]}[N], bwd


# ------------------------------------------------------------------------------------------------------------------ #
# flat kernels: activation, add
# ------------------------------------------------------------------------------------------------------------------ #
GUARD = 64


def _flat_buf(n, off, dt, values=None):
    """a sentinel-filled buffer of off + n + GUARD elements and its view [off, off + n) (filled with `values` if given)"""
    base = _out((off + n + GUARD,), dt)
    view = base[off:off + n]
    if values is not None:
        view.copy_(_to_dev(values, dt))
    return base, view


def _guard_ok(base, n, off):
    return _untouched(base[:off]) and _untouched(base[off + n:])


def _flat_check(entry, case):
    check_case(entry, case)
    assert _out((8,), case['dt']).data_ptr() % 16 == 0          # the allocator's alignment, which `off` is relative to


@pytest.mark.parametrize('case', FLAT, ids=_id)
def test_act_fwd(case):
    _flat_check('act_fwd', case)
    dt, n, off = case['dt'], case['n'], case['off']
    rng = np.random.default_rng(n)
    x = _normal(rng, n, dt, 6)
    xb, xv = _flat_buf(n, off, dt, x)
    yb, yv = _flat_buf(n, off, dt)
    _call('act_fwd', _p(xv), _p(yv), n, _nat().ACT_LEAKY_CLIP, ALPHA, VMAX, _tag(dt))
    assert _same(yv, R.act_fwd(x, ALPHA, VMAX, dt), dt), case
    assert _guard_ok(yb, n, off) and _guard_ok(xb, n, off), case


@pytest.mark.parametrize('inplace', [False, True])
@pytest.mark.parametrize('case', FLAT, ids=_id)
def test_act_bwd(case, inplace):
    """dx = dy * act'(.), the derivative taken from the PRE-activation x whose stored output y the kernel is given (max_value
    10 is a bf16 value: x < 10 <=> y < 10 exactly); in place (dx == dy) as _AvgPool2Skip.backward calls it"""
    _flat_check('act_bwd', case)
    dt, n, off = case['dt'], case['n'], case['off']
    rng = np.random.default_rng(n + 1)
    x = _normal(rng, n, dt, 6)
    dy = _normal(rng, n, dt)
    y = R.act_fwd(x, ALPHA, VMAX, dt)
    sl = R.act_slope(x, ALPHA, VMAX)
    if n > 1000:
        assert (sl == 0).any() and (sl == 1).any() and (sl == np.float32(ALPHA)).any()
    yb, yv = _flat_buf(n, off, dt, y)
    gb, gv = _flat_buf(n, off, dt, dy)
    ob, ov = (gb, gv) if inplace else _flat_buf(n, off, dt)
    _call('act_bwd', _p(gv), _p(yv), _p(ov), n, _nat().ACT_LEAKY_CLIP, ALPHA, VMAX, _tag(dt))
    assert _same(ov, R.act_bwd(dy, x, ALPHA, VMAX, dt), dt), case
    assert _guard_ok(ob, n, off) and _guard_ok(yb, n, off), case
    if not inplace:
        assert _same(gv, dy, dt)


@pytest.mark.parametrize('case', FLAT, ids=_id)
def test_add(case):
    _flat_check('add', case)
    dt, n, off = case['dt'], case['n'], case['off']
    rng = np.random.default_rng(n + 2)
    a = _normal(rng, n, dt)
    b = _normal(rng, n, dt, 3)
    ab, av = _flat_buf(n, off, dt, a)
    bb, bv = _flat_buf(n, off, dt, b)
    yb, yv = _flat_buf(n, off, dt)
    _call('add', _p(av), _p(bv), _p(yv), n, _tag(dt))
    assert _same(yv, R.add(a, b, dt), dt), case
    assert _guard_ok(yb, n, off), case


def test_flat_kernels_mixed_alignment():
    """one unaligned pointer among aligned ones is enough to need the scalar instantiation"""
    n = 8 * 41 + 3
    for dt in ('f32', 'bf16'):
        rng = np.random.default_rng(5)
        a = _normal(rng, n, dt)
        b = _normal(rng, n, dt)
        for offs in ((1, 0, 0), (0, 3, 0), (0, 0, 1)):
            (_, av), (_, bv), (yb, yv) = _flat_buf(n, offs[0], dt, a), _flat_buf(n, offs[1], dt, b), _flat_buf(n, offs[2], dt)
            _call('add', _p(av), _p(bv), _p(yv), n, _tag(dt))
            assert _same(yv, R.add(a, b, dt), dt) and _guard_ok(yb, n, offs[2]), (dt, offs)
            yb, yv = _flat_buf(n, offs[2], dt)
            _call('act_bwd', _p(av), _p(bv), _p(yv), n, _nat().ACT_LEAKY_CLIP, ALPHA, VMAX, _tag(dt))
            # (b plays the stored output; 10 is representable, so act' from the output is act' from the pre-activation)
            assert _same(yv, R.act_bwd(a, b, ALPHA, VMAX, dt), dt) and _guard_ok(yb, n, offs[2]), (dt, offs)


def _special_values(vmax, dt):
    v = [-0.0, 0.0, 1.0, -1.0, 3.0, -3.0, np.inf, -np.inf, np.nan, 2.0 ** -126, -2.0 ** -126, 1e-40, -1e-40, 65280.0, -65280.0]
    if np.isfinite(vmax):
        u = R.bf16_ulp(vmax) if vmax > 0 else 2.0 ** -133
        v += [vmax, vmax + u, vmax - u, vmax + 2 * u, vmax - 2 * u, vmax * (1 + 2.0 ** -23), vmax * (1 - 2.0 ** -24), -vmax]
    return R.store(np.array(v * 3, dtype=np.float32), dt)        # (3 copies: 8-element vectors and a scalar tail both see them)


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('alpha,vmax', [(0.1, 10.0), (0.0, np.inf), (1.5, 6.0), (0.1, 0.0)])
def test_act_special_values(alpha, vmax, dt):
    """signed zeros, max_value and its bf16 neighbours, infinities, NaN, denormals: the forward against the fp64 oracle
    (oracle.cs_oracle.relu_leaky_clip, cast), the backward against the slope at the pre-activation (every max_value here is a
    bf16 value, so the stored output decides the slope exactly)"""
    x = _special_values(vmax, dt)
    n = x.size
    with np.errstate(all='ignore'):
        ref = orc.relu_leaky_clip(torch.tensor(x, dtype=torch.float64), float(np.float32(alpha)), float(np.float32(vmax)))
    ref = R.store(ref.to(torch.float32).numpy(), dt)
    _, xv = _flat_buf(n, 0, dt, x)
    yb, yv = _flat_buf(n, 0, dt)
    _call('act_fwd', _p(xv), _p(yv), n, _nat().ACT_LEAKY_CLIP, alpha, vmax, _tag(dt))
    y = yv.float().cpu().numpy()
    assert np.array_equal(y, ref, equal_nan=True), (alpha, vmax, dt, x, y, ref)        # (by value: -0.0 == +0.0)
    assert _guard_ok(yb, n, 0)
    # backward: every finite pre-activation that is not max_value itself (there the derivative is a convention)
    dy = R.store(np.linspace(-2, 2, n, dtype=np.float32) + np.float32(0.3), dt)
    _, gv = _flat_buf(n, 0, dt, dy)
    ob, ov = _flat_buf(n, 0, dt)
    _call('act_bwd', _p(gv), _p(yv), _p(ov), n, _nat().ACT_LEAKY_CLIP, alpha, vmax, _tag(dt))
    dx = ov.float().cpu().numpy()
    # (and not the values so small that alpha * x underflows to a zero, which has lost x's sign)
    ok = np.isfinite(x) & (x != np.float32(vmax)) & ((x == 0) | (np.abs(x) > 2.0 ** -100))
    want = R.act_bwd(dy, x, alpha, vmax, dt)
    assert np.array_equal(dx[ok], want[ok]), (alpha, vmax, dt, x[ok], dx[ok], want[ok])
    assert ok.sum() >= 15 and (want[ok] != 0).any() and _guard_ok(ob, n, 0)


# ------------------------------------------------------------------------------------------------------------------ #
# pooling / upsampling
# ------------------------------------------------------------------------------------------------------------------ #

def _arith_case(entry, case):
    check_case(entry, case)
    return case['dt'], case['B'], case['N'], case['C']


@pytest.mark.parametrize('case', POOL_FWD, ids=_id)
def test_avgpool2_fwd(case):
    dt, B, N, C = _arith_case('avgpool2_fwd', case)
    x, xd = _rand(np.random.default_rng(N * C), (B, 6, N, N, C), dt)
    y = _out((B, 6, N // 2, N // 2, C), dt)
    _call('avgpool2_fwd', _p(xd), _p(y), B, N, C, _tag(dt))
    assert _same(y, R.avgpool2_fwd(x, dt), dt), case


@pytest.mark.parametrize('case', POOL_BWD, ids=_id)
def test_avgpool2_bwd(case):
    dt, B, N, C = _arith_case('avgpool2_bwd', case)
    dy, dyd = _rand(np.random.default_rng(N * C + 1), (B, 6, N // 2, N // 2, C), dt)
    dx = _out((B, 6, N, N, C), dt)
    _call('avgpool2_bwd', _p(dyd), _p(dx), B, N, C, _tag(dt))
    assert _same(dx, R.avgpool2_bwd(dy, dt), dt), case


@pytest.mark.parametrize('case', POOL_BWD_ADD, ids=_id)
def test_avgpool2_bwd_add(case):
    dt, B, N, C = _arith_case('avgpool2_bwd_add', case)
    alias = case['alias']
    rng = np.random.default_rng(N * C + 2)
    dy, dyd = _rand(rng, (B, 6, N // 2, N // 2, C), dt)
    sk, skd = _rand(rng, (B, 6, N, N, C), dt, 3.0)
    dx = skd if alias else _out((B, 6, N, N, C), dt)
    _call('avgpool2_bwd_add', _p(dyd), _p(skd), _p(dx), B, N, C, _tag(dt))
    assert _same(dx, R.avgpool2_bwd_add(dy, sk, dt), dt), case


@pytest.mark.parametrize('case', POOL_MASKED, ids=_id)
def test_avgpool2_bwd_masked(case):
    """m = the stored output of ReLU(0.1, 10) at a known pre-activation x; act' is taken from x"""
    dt, B, N, C = _arith_case('avgpool2_bwd_masked', case)
    rng = np.random.default_rng(N * C + 3)
    dy, dyd = _rand(rng, (B, 6, N // 2, N // 2, C), dt)
    sk, skd = _rand(rng, (B, 6, N, N, C), dt, 3.0) if case['skip'] else (None, None)
    x = _normal(rng, (B, 6, N, N, C), dt, 6)
    md = _to_dev(R.act_fwd(x, ALPHA, VMAX, dt), dt)
    dx = _out((B, 6, N, N, C), dt)
    _call('avgpool2_bwd_masked', _p(dyd), _p(skd), _p(md), _p(dx), B, N, C, ALPHA, VMAX, _tag(dt))
    assert _same(dx, R.avgpool2_bwd_masked(dy, sk, R.act_slope(x, ALPHA, VMAX), dt), dt), case


@pytest.mark.parametrize('case', UP_FWD, ids=_id)
def test_upsample2_fwd(case):
    dt, B, N, C = _arith_case('upsample2_fwd', case)
    x, xd = _rand(np.random.default_rng(N * C + 4), (B, 6, N, N, C), dt)
    y = _out((B, 6, 2 * N, 2 * N, C), dt)
    _call('upsample2_fwd', _p(xd), _p(y), B, N, C, _tag(dt))
    assert _same(y, R.upsample2_fwd(x), dt), case


@pytest.mark.parametrize('case', UP_BWD, ids=_id)
def test_upsample2_bwd(case):
    dt, B, N, C = _arith_case('upsample2_bwd', case)
    dy, dyd = _rand(np.random.default_rng(N * C + 5), (B, 6, 2 * N, 2 * N, C), dt)
    dx = _out((B, 6, N, N, C), dt)
    _call('upsample2_bwd', _p(dyd), _p(dx), B, N, C, _tag(dt))
    assert _same(dx, R.upsample2_bwd(dy, dt), dt), case


# ------------------------------------------------------------------------------------------------------------------ #
# channel movers
# ------------------------------------------------------------------------------------------------------------------ #

def _cat_case(entry, case):
    check_case(entry, case)
    return case['dt'], case['rows'], case['Ca'], case['Cb']


@pytest.mark.parametrize('case', CONCAT, ids=_id)
def test_concat2(case):
    dt, rows, Ca, Cb = _cat_case('concat2', case)
    rng = np.random.default_rng(rows + Ca)
    a, ad = _rand(rng, (rows, Ca), dt)
    b, bd = _rand(rng, (rows, Cb), dt)
    y = _out((rows, Ca + Cb), dt)
    _call('concat2', _p(ad), _p(bd), _p(y), rows, Ca, Cb, _tag(dt))
    assert _same(y, R.concat2(a, b), dt), case


@pytest.mark.parametrize('case', SPLIT, ids=_id)
def test_split2(case):
    """both halves, only `a` (b null), only `b` (a null)"""
    dt, rows, Ca, Cb = _cat_case('split2', case)
    y, yd = _rand(np.random.default_rng(rows + Cb), (rows, Ca + Cb), dt)
    a = _out((rows, Ca), dt)
    b = _out((rows, Cb), dt)
    only = case['only']
    _call('split2', _p(yd), _p(a) if 'a' in only else 0, _p(b) if 'b' in only else 0, rows, Ca, Cb, _tag(dt))
    ra, rb = R.split2(y, Ca)
    assert _same(a, ra, dt) if 'a' in only else _untouched(a), case
    assert _same(b, rb, dt) if 'b' in only else _untouched(b), case


@pytest.mark.parametrize('case', CHAN_PAD, ids=_id)
def test_pad_channels(case):
    dt, rows, C, Cp = case['dt'], case['rows'], case['C'], case['Cp']
    check_case('pad_channels', case)
    x, xd = _rand(np.random.default_rng(rows + C), (rows, C), dt)
    y = _out((rows, Cp), dt)
    _call('pad_channels', _p(xd), _p(y), rows, C, Cp, _tag(dt))
    assert _same(y, R.pad_channels(x, Cp), dt), case


@pytest.mark.parametrize('case', CHAN_PAD, ids=_id)
def test_slice_channels(case):
    dt, rows, C, Cp = case['dt'], case['rows'], case['C'], case['Cp']
    check_case('slice_channels', case)
    y, yd = _rand(np.random.default_rng(rows + Cp), (rows, Cp), dt)
    x = _out((rows, C), dt)
    _call('slice_channels', _p(yd), _p(x), rows, Cp, C, _tag(dt))
    assert _same(x, R.slice_channels(y, C), dt), case


@pytest.mark.parametrize('case', REPACK, ids=_id)
def test_state_repack(case):
    dt, B, S, T, V, E = (case[k] for k in ('dt', 'B', 'S', 'T', 'V', 'E'))
    check_case('state_repack', case)
    rng = np.random.default_rng(S + V)
    st, std = _rand(rng, (B, S, T * V), dt)
    ex, exd = _rand(rng, (B, T, S, E), dt, 5.0)
    out = _out((B, S, T * (V + E)), dt)
    _call('state_repack', _p(std), _p(exd), _p(out), B, S, T, V, E, _tag(dt))
    assert _same(out, R.state_repack(st, ex, T), dt), case


@pytest.mark.parametrize('case', TRANSPOSE, ids=_id)
def test_layout_converters(case):
    dt, B, C, S = case['dt'], case['B'], case['C'], case['S']
    check_case('cf_to_cl', case)
    x, xd = _rand(np.random.default_rng(C + S), (B, C, S), dt)
    y = _out((B, S, C), dt)
    _call('cf_to_cl', _p(xd), _p(y), B, C, S, _tag(dt))
    assert _same(y, R.cf_to_cl(x), dt), case
    back = _out((B, C, S), dt)
    _call('cl_to_cf', _p(y), _p(back), B, C, S, _tag(dt))
    assert _same(back, x, dt), case
    z, zd = _rand(np.random.default_rng(C + S + 1), (B, S, C), dt)
    w = _out((B, C, S), dt)
    _call('cl_to_cf', _p(zd), _p(w), B, C, S, _tag(dt))
    assert _same(w, R.cl_to_cf(z), dt), case


# ------------------------------------------------------------------------------------------------------------------ #
# batch gather
# ------------------------------------------------------------------------------------------------------------------ #

@pytest.mark.parametrize('case', GATHER, ids=_id)
def test_batch_gather(case):
    dt, S, nv, steps, win, cl = (case[k] for k in ('dt', 'S', 'nv', 'steps', 'win', 'cl'))
    nch = nv * steps
    Ctot, c_off, c_stride = win if win else (nch, 0, nv)
    assert case['kern'] == gather_rule(case), case
    T, V, B = 9, nv + 3, 5
    t_off, t_stride = (1, 2) if steps > 1 else (2, 1)
    rng = np.random.default_rng(S + nv)
    array = rng.standard_normal((T, V, S), dtype=np.float32)
    samples = np.array([3, 0, 3, 1, 2], dtype=np.int32)[:B]              # repeated and out of order
    var_idx = rng.permutation(V)[:nv].astype(np.int32)                    # a permuted subset
    assert int(samples.max()) + t_off + (steps - 1) * t_stride < T
    dev = _dev()
    ad = torch.from_numpy(array).to(dev)
    assert ad.data_ptr() % 16 == 0
    shape = (B, S, Ctot) if cl else (B, Ctot, S)
    out = _out(shape, dt)
    assert out.data_ptr() % 16 == 0
    before = out.float().cpu().numpy()
    sd, vd = torch.from_numpy(samples).to(dev), torch.from_numpy(var_idx).to(dev)
    _call('batch_gather', _p(ad), T, V, S, _p(sd), B, _p(vd), nv, steps, t_off, t_stride, _p(out), Ctot, c_off, c_stride, int(cl),
          _tag(dt))
    ref = R.batch_gather(array, samples, var_idx, steps, t_off, t_stride, before, c_off, c_stride, cl, dt)
    assert _same(out, ref, dt), case                # (the columns outside the window still hold the sentinel: `before`)
    keep = np.ones(Ctot, dtype=bool)
    for n in range(steps):
        keep[c_off + n * c_stride:c_off + n * c_stride + nv] = False
    if keep.any():
        outside = out[:, :, torch.from_numpy(keep).to(dev)] if cl else out[:, torch.from_numpy(keep).to(dev), :]
        assert _untouched(outside.contiguous()), case


def test_batch_gather_unaligned_output_takes_the_tile_kernel():
    """the 256-pixel kernel writes 16-B vectors: an output that starts off a 16-B boundary must be served by the 64-pixel one"""
    for dt in ('f32', 'bf16'):
        S, nv, steps, T, V, B = 600, 4, 2, 6, 5, 3
        rng = np.random.default_rng(11)
        array = rng.standard_normal((T, V, S), dtype=np.float32)
        samples = np.array([2, 0, 2], dtype=np.int32)
        var_idx = np.array([4, 0, 3, 1], dtype=np.int32)
        dev = _dev()
        base = _out((B * S * nv * steps + 2 + GUARD,), dt)
        view = base[2:2 + B * S * nv * steps]
        assert view.data_ptr() % 16 != 0
        ad, sd, vd = torch.from_numpy(array).to(dev), torch.from_numpy(samples).to(dev), torch.from_numpy(var_idx).to(dev)
        _call('batch_gather', _p(ad), T, V, S, _p(sd), B, _p(vd), nv, steps, 0, 3, _p(view), nv * steps, 0, nv, 1, _tag(dt))
        ref = R.batch_gather(array, samples, var_idx, steps, 0, 3, np.zeros((B, S, nv * steps), np.float32), 0, nv, True, dt)
        assert _same(view, ref, dt) and _guard_ok(base, B * S * nv * steps, 2), dt


# ------------------------------------------------------------------------------------------------------------------ #
# bf16: the activation-gradient mask against the PRE-activation, for max_value that bf16 cannot represent
# ------------------------------------------------------------------------------------------------------------------ #
# 0.7 -> 0.69921875 and 0.9 -> 0.8984375 round DOWN (every clipped output is stored below max_value), 5.3 and 10.1 round up,
# 10 is exact.  The band |x - max_value| <= ulp_bf16(max_value) holds the pre-activations whose stored output is one of the two
# bf16 neighbours of max_value although they are not clipped (or vice versa); it is a cap, checked to hold <= 1 % of the elements.
MASK_VMAX = [0.7, 0.9, 5.3, 10.1, 10.0]


def _band(x, vmax):
    return np.abs(x.astype(np.float64) - float(np.float32(vmax))) <= R.bf16_ulp(vmax)


def _report(what, got, want, use):
    bad = (got != want) & use
    share = bad.sum() / max(use.sum(), 1)
    print('%s: %d of %d elements outside the band differ (%.2f %%)' % (what, bad.sum(), use.sum(), 100 * share))
    return share


@pytest.mark.parametrize('alpha', [0.0, 0.1])
@pytest.mark.parametrize('vmax', MASK_VMAX)
def test_bf16_act_mask_follows_the_preactivation(vmax, alpha):
    dt, n = 'bf16', 200003
    rng = np.random.default_rng(int(vmax * 10) + int(alpha * 10))
    x = _normal(rng, n, dt)
    dy = _normal(rng, n, dt)
    _, xv = _flat_buf(n, 0, dt, x)
    _, yv = _flat_buf(n, 0, dt)
    _call('act_fwd', _p(xv), _p(yv), n, _nat().ACT_LEAKY_CLIP, alpha, vmax, _tag(dt))
    y = yv.float().cpu().numpy()
    clipped = x >= np.float32(vmax)
    assert np.all(np.abs(y[clipped].astype(np.float64) - float(np.float32(vmax))) <= R.bf16_ulp(vmax))
    assert np.array_equal(y[~clipped], R.act_fwd(x, alpha, vmax, dt)[~clipped])
    if vmax < 1:
        assert clipped.mean() > 0.1
    _, gv = _flat_buf(n, 0, dt, dy)
    ob, ov = _flat_buf(n, 0, dt)
    _call('act_bwd', _p(gv), _p(yv), _p(ov), n, _nat().ACT_LEAKY_CLIP, alpha, vmax, _tag(dt))
    band = _band(x, vmax)
    assert band.mean() <= 0.01, band.mean()
    share = _report('act_bwd max_value=%g alpha=%g' % (vmax, alpha), _bits(ov), _ref_bits(R.act_bwd(dy, x, alpha, vmax, dt), dt), ~band)
    assert share == 0.0, 'act_bwd(max_value=%g): %.2f %% of the elements outside the band got the wrong slope' % (vmax, 100 * share)
    assert _guard_ok(ob, n, 0)


@pytest.mark.parametrize('skip', [True, False])
@pytest.mark.parametrize('vmax', MASK_VMAX)
def test_bf16_pool_mask_follows_the_preactivation(vmax, skip):
    """avgpool2_bwd_masked with m = the forward kernel's own output of a known x"""
    dt, B, N, C, alpha = 'bf16', 2, 12, 24, 0.1
    rng = np.random.default_rng(int(vmax * 10) + 50)
    x, xd = _rand(rng, (B, 6, N, N, C), dt)
    dy, dyd = _rand(rng, (B, 6, N // 2, N // 2, C), dt)
    sk, skd = _rand(rng, (B, 6, N, N, C), dt) if skip else (None, None)
    m = _out(x.shape, dt)
    _call('act_fwd', _p(xd), _p(m), x.size, _nat().ACT_LEAKY_CLIP, alpha, vmax, _tag(dt))
    dx = _out(x.shape, dt)
    _call('avgpool2_bwd_masked', _p(dyd), _p(skd), _p(m), _p(dx), B, N, C, alpha, vmax, _tag(dt))
    band = _band(x, vmax)
    assert band.mean() <= 0.01, band.mean()
    want = _ref_bits(R.avgpool2_bwd_masked(dy, sk, R.act_slope(x, alpha, vmax), dt), dt).reshape(x.shape)
    share = _report('avgpool2_bwd_masked max_value=%g' % vmax, _bits(dx), want, ~band)
    assert share == 0.0, 'avgpool2_bwd_masked(max_value=%g): %.2f %% wrong outside the band' % (vmax, 100 * share)
