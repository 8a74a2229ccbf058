"""
Seeded random sweep of the fused cubed-sphere convolution (forward + all gradients) against the fp64 oracle, in both
dtypes, over shapes the hand-picked cases do not cover: batch 1..5, face sizes 4..26 (odd and even), channel counts that
are odd / even-only / multiples of 8 / of 64, with and without the fused upsample + concat, halo or plain 'valid', 1x1 and
3x3, flip / independent north pole, with and without the activation.  The kernels pick different code paths by shape
(vector widths, matrix-core vs fallback weight gradient, dz hand-over, direct data-gradient writes, ring fix-up, LDS patch
or quad stores), so this is mostly a dispatch-consistency test.  Tolerances as in test_gpu_parity.py / test_gpu_bf16.py.
The runner is shared with test_gpu_conv_coverage.py (conv_check.py).
"""
import os

import numpy as np
import pytest

from conv_check import check as _run

pytestmark = pytest.mark.gpu


def _cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        k = int(rng.choice([1, 3, 3, 3]))
        halo = bool(k == 3 and rng.random() < 0.8)
        up0 = bool(halo and rng.random() < 0.35)
        # (faces >= 24 with channel counts in multiples of 8 take the round-5 default data gradient -- the gather form -- in bf16)
        N = int(rng.choice([4, 6, 8, 10, 12, 16, 20, 24, 26, 32] if up0 else [4, 5, 6, 7, 8, 9, 12, 13, 16, 20, 24, 25, 27, 32]))
        c0 = int(rng.choice([1, 2, 3, 6, 8, 14, 16, 24, 32, 64]))
        c1 = int(rng.choice([0, 0, 2, 8, 10, 32])) if halo else 0
        if c0 + c1 > 72:
            c1 = 0
        cout = int(rng.choice([1, 2, 7, 8, 14, 16, 24, 32, 40, 64]))
        B = int(rng.integers(1, 6))
        flip, indep, act = bool(rng.random() < 0.7), bool(rng.random() < 0.3), bool(rng.random() < 0.7)
        out.append((B, N, c0, c1, cout, k, halo, up0, flip, indep, act))
    return out


_N = int(os.environ.get('DLWPCS_FUZZ_N', '28'))                 # DLWPCS_FUZZ_N / DLWPCS_FUZZ_SEED widen or move the sweep
_S = int(os.environ.get('DLWPCS_FUZZ_SEED', '0'))


@pytest.mark.parametrize('case', _cases(_N, 101 + _S))
def test_conv_random_shapes_f32(case):
    _run(case, bf16=False)


@pytest.mark.parametrize('case', _cases(_N, 202 + _S))
def test_conv_random_shapes_bf16(case):
    _run(case, bf16=True)
