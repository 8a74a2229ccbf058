"""
numpy restatement of dlwpcs_solar_fill (include/dlwpcs.h, csrc/solar.hip) and the inputs the solar-forcing tests share.

`fill` is the kernel's arithmetic operation by operation: `hour` from two rounded fp32 operations, the fp32 cosine of it, the
combine in fp64 in the kernel's order, the clamp, the rounding to fp32.  The only thing it does not share with the kernel is the
cosine itself (numpy's here, the device's cosf there).
"""
import numpy as np

import remap_maps


def fill(row_tab, cell_tab, rows):
    """(len(rows), cells) float32: the value dlwpcs_solar_fill writes for row `rows[i]` and every cell"""
    row_tab, cell_tab = np.asarray(row_tab, dtype=np.float64), np.asarray(cell_tab, dtype=np.float64)
    r = row_tab[np.asarray(rows, dtype=np.int64)]
    sindec, cosdec, scale = r[:, 0:1], r[:, 1:2], r[:, 2:3]
    day = r[:, 3:4].astype(np.float32)
    sinphi, cosphi = cell_tab[None, :, 0], cell_tab[None, :, 1]
    lonfrac = cell_tab[None, :, 2].astype(np.float32)
    hour = np.float32(2 * np.pi) * (day + lonfrac)
    assert hour.dtype == np.float32
    c = np.cos(hour).astype(np.float64)
    a = sinphi * sindec
    b = (cosphi * cosdec) * c
    v = scale * (a - b)
    return np.maximum(v, 0.).astype(np.float32)


def cube_latlon(N):
    """(lat, lon), each (6, N, N) float64 degrees, lon in 0-360: cell centres of the equiangular cubed sphere"""
    lat, lon = remap_maps.Cube(N).centres()
    return lat.reshape(6, N, N), lon.reshape(6, N, N)


def dates_6h(start, n, hours=6):
    """n datetime64 stamps from `start` every `hours` hours"""
    return np.datetime64(start, 'ns') + np.arange(n) * np.timedelta64(hours, 'h')


#: (start, count): 6-hourly records that cross a year boundary, run through a leap day and over the end of a leap year
DATE_CASES = {
    'new_year': ('2014-12-29T00', 40),
    'leap_day': ('2016-02-26T18', 40),
    'leap_year_end': ('2016-12-28T06', 40),
    'summer': ('2015-06-19T03', 24),
}

#: generator settings the host and the device tests run: single-step and sequence mode, interval > 1, both channel layouts
GEN_CASES = {
    'single_cl': dict(input_time_steps=2, output_time_steps=2, channels_last=True),
    'single_cf': dict(input_time_steps=2, output_time_steps=2, channels_last=False),
    'single_interval2': dict(input_time_steps=3, output_time_steps=1, interval=2, channels_last=True),
    'sequence_cl': dict(input_time_steps=2, output_time_steps=2, sequence=3, channels_last=True),
    'sequence_cf_interval2': dict(input_time_steps=2, output_time_steps=2, sequence=2, interval=2, channels_last=False),
}


def gen_data(N=4, T=40, V=3, K=2, seed=5, start='2015-12-27T00'):
    """(data (T, V, 6, N, N), constants (K, 6, N, N), SolarForcing of the same T rows): one small cubed-sphere record"""
    from DLWP.util import SolarForcing
    rng = np.random.default_rng(seed)
    lat, lon = cube_latlon(N)
    arr = rng.standard_normal((T, V, 6, N, N)).astype(np.float32)
    const = rng.standard_normal((K, 6, N, N)).astype(np.float32)
    return arr, const, SolarForcing(dates_6h(start, T), lat, lon)
