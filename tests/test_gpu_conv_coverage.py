"""
Case table of the fused cubed-sphere convolution that NAMES the kernel instantiations it runs: every case runs forward,
data gradient and weight gradient (or the passes it names) through ops.cs_conv with the library's per-launch profiler on,
asserts that each declared tag (dlwpcs_prof_known_tag) was launched, and compares forward, both source gradients, dW and db
of every weight group with the fp64 oracle (the runner of test_gpu_fuzz.py, conv_check.py).  test_conv_coverage_tags.py
(CPU) checks that the declared tags plus UNREACHABLE are exactly the registered ones.

The comments give what launch_conv_cfg (conv_launch.h) computes for the forward launch of the regime a case is there for:
pix (tile pixels), ncol (column strips), nblk (tiles per strip), ntiles, gx (workers), lds (bytes), patches (0: quad-store
epilogue), wstat (resident weight areas), pool / colsplit (pooled second output, half-row split).

Also the face-size surface (FACE_SIZES): the layer shapes of a U-Net whose finest level is N, each either matching the
oracle or refused with NotImplementedError -- never a wrong result.
"""
import json
import os
import subprocess
import sys
from collections import namedtuple

import pytest

import conv_check

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, F = True, False

# name, case = (B, N, C0, C1, Cout, k, halo, up0, flip, indep, act), bf16, runner options (conv_check.errors), declared tags
C = namedtuple('C', 'name case bf16 kw tags')

CASES = [
    C('f32_n96_32_32_b2', (2, 96, 32, 0, 32, 3, True, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_n96_64_64', (1, 96, 64, 0, 64, 3, True, False, True, True, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 2, 2, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_n96_128_64', (1, 96, 128, 0, 64, 3, True, False, False, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 2, 2, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 2, 2, 4, 2, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_n96_dec', (1, 96, 64, 32, 32, 3, True, True, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 2, 2, 4, 2, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_n96_odd', (1, 96, 7, 0, 9, 3, True, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 8, 3, 1, 4, 1, 1, 2, true, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_n96_even', (1, 96, 6, 0, 10, 3, True, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 8, 3, 1, 4, 1, 2, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 8, 3, 1, 4, 1, 2, 2, true, false, false, false>', 'wgrad_mfma_kernel<float, 3, 2, true>')),
    C('f32_n96_pool', (1, 96, 32, 0, 32, 3, True, False, True, False, True), False, {'want_pool': True},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_n96_pool64', (1, 96, 32, 0, 64, 3, True, False, True, False, True), False, {'want_pool': True},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 2, 2, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_n80_64_64', (1, 80, 64, 0, 64, 3, True, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 2, 2, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_n80_32_64', (1, 80, 32, 0, 64, 3, True, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 2, 2, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_n80_64_32', (1, 80, 64, 0, 32, 3, True, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('bf_n96_32_32_b2', (2, 96, 32, 0, 32, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, true>', 'wgrad_bf16_kernel<3, true, 8, 4, 1, 8>')),
    C('bf_n96_64_64', (1, 96, 64, 0, 64, 3, True, False, True, True, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, true>', 'wgrad_bf16_kernel<3, true, 8, 4, 2, 8>')),
    C('bf_n96_128_64', (1, 96, 128, 0, 64, 3, True, False, False, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 2, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 8, 4, 2, 8>')),
    C('bf_n96_dec', (1, 96, 64, 32, 32, 3, True, True, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 2, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 8, 4, 1, 8>')),
    C('bf_n96_dec_noact', (1, 96, 64, 32, 32, 3, True, True, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 2, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_bf16_kernel<3, false, 8, 4, 1, 8>')),
    C('bf_n96_odd', (1, 96, 7, 0, 9, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 1, 2, true, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 3, 8, true>')),
    C('bf_n96_even', (1, 96, 6, 0, 10, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 2, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 2, 2, true, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 3, 2, true>')),
    C('bf_n96_pool', (1, 96, 32, 0, 32, 3, True, False, True, False, True), True, {'want_pool': True},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, true>', 'wgrad_bf16_kernel<3, true, 8, 4, 1, 8>')),
    C('bf_n96_pool64', (1, 96, 32, 0, 64, 3, True, False, True, False, True), True, {'want_pool': True},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, true>', 'wgrad_bf16_kernel<3, true, 8, 4, 1, 8>')),
    C('bf_n80_64_64', (1, 80, 64, 0, 64, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 8, 4, 2, 8>')),
    C('f32_valid_48_small', (2, 18, 32, 0, 48, 3, False, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 2, 2, 4, 0, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_valid_96_small', (1, 18, 32, 0, 96, 3, False, False, True, True, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 8, 5, 1, 1, 4, 4, 0, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_valid_48_large', (1, 24, 16, 0, 48, 3, False, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 2, 2, 4, 0, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_valid_96_large', (1, 24, 16, 0, 96, 3, False, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 2, 2, 4, 0, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('bf_valid_48_small', (2, 18, 32, 0, 48, 3, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 0, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 8, 4, 1, 8>')),
    C('bf_valid_96_small', (1, 18, 32, 0, 96, 3, False, False, True, True, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 5, 1, 1, 4, 8, 0, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 8, 4, 1, 8>')),
    C('bf_valid_48_large', (1, 24, 16, 0, 48, 3, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 0, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 8, 4, 1, 8>')),
    C('bf_valid_96_large', (1, 24, 16, 0, 96, 3, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 0, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 8, 4, 1, 8>')),
    C('f32_valid_odd', (1, 12, 5, 0, 7, 3, False, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 0, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 8, 3, 1, 4, 1, 1, 2, true, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_valid_even', (1, 12, 6, 0, 10, 3, False, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 8, 3, 1, 4, 1, 2, 0, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 8, 3, 1, 4, 1, 2, 2, true, false, false, false>', 'wgrad_mfma_kernel<float, 3, 2, true>')),
    C('bf_valid_odd', (1, 12, 5, 0, 7, 3, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 1, 2, true, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 3, 8, true>')),
    C('bf_valid_even', (1, 12, 6, 0, 10, 3, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 2, 0, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 2, 2, true, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 3, 2, true>')),
    C('f32_halo_96out_small', (1, 16, 32, 0, 96, 3, True, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 8, 5, 1, 1, 4, 4, 1, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('bf_halo_96out_small', (1, 16, 32, 0, 96, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 5, 1, 1, 4, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 8, 4, 1, 8>')),
    C('f32_halo_96in', (1, 16, 96, 0, 32, 3, True, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 2, 2, 4, 2, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('bf_halo_96in', (1, 16, 64, 32, 32, 3, True, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 2, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_bf16_kernel<3, false, 8, 4, 1, 8>')),
    C('bf_halo_96in_n24', (1, 24, 64, 32, 32, 3, True, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 1, false, false, false, true>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_bf16_kernel<3, false, 8, 4, 1, 8>')),
    C('bf_halo_128_64_n24', (1, 24, 128, 0, 64, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 1, false, false, false, true>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 8, 4, 2, 8>')),
    C('f32_dx_only_32', (2, 12, 32, 0, 32, 3, True, False, True, False, True), False, {'wgrad': False},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, true, false, false, false>')),
    C('f32_dx_only_64', (1, 12, 64, 0, 32, 3, True, False, True, False, True), False, {'wgrad': False},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, true, false, false, false>')),
    C('f32_dx_only_96', (1, 12, 96, 0, 32, 3, True, False, True, False, True), False, {'wgrad': False},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 2, 2, 4, 2, true, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>')),
    C('bf_dx_only_32', (2, 12, 32, 0, 32, 3, True, False, True, False, True), True, {'wgrad': False},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, true, false, false, false>')),
    C('bf_dx_only_64', (1, 12, 64, 0, 32, 3, True, False, True, False, True), True, {'wgrad': False},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, true, false, false, false>')),
    C('bf_dx_only_96', (1, 12, 96, 0, 32, 3, True, False, True, False, True), True, {'wgrad': False},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 2, true, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>')),
    C('f32_dx_only_odd', (1, 8, 8, 0, 7, 3, True, False, True, False, True), False, {'wgrad': False},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 8, 3, 1, 4, 1, 1, 2, true, false, false, false>')),
    C('f32_dx_only_even', (1, 8, 8, 0, 6, 3, True, False, True, False, True), False, {'wgrad': False},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 8, 3, 1, 4, 1, 2, 2, true, false, false, false>')),
    C('bf_dx_only_odd', (1, 8, 8, 0, 7, 3, True, False, True, False, True), True, {'wgrad': False},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 1, 2, true, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>')),
    C('bf_dx_only_even', (1, 8, 8, 0, 6, 3, True, False, True, False, True), True, {'wgrad': False},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 2, 2, true, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>')),
    C('f32_dw_only', (2, 12, 32, 0, 32, 3, True, False, True, True, True), False, {'dgrad': False},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('bf_dw_only', (2, 12, 32, 0, 32, 3, True, False, True, True, True), True, {'dgrad': False},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 8, 4, 1, 8>')),
    C('bf_premask_grid_32', (2, 6, 16, 16, 16, 3, True, False, True, False, False), True, {'premask': True},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, true, false>', 'wgrad_bf16_kernel<3, false, 8, 4, 1, 8>')),
    C('bf_premask_grid_64', (1, 6, 32, 32, 16, 3, True, False, True, False, False), True, {'premask': True},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, true, false>', 'wgrad_bf16_kernel<3, false, 8, 4, 2, 8>')),
    C('bf_premask_grid_96', (1, 6, 64, 32, 16, 3, True, False, True, False, False), True, {'premask': True},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 2, false, false, true, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_bf16_kernel<3, false, 8, 4, 1, 8>')),
    C('bf_premask_grid_act', (2, 6, 16, 16, 16, 3, True, False, True, False, True), True, {'premask': True},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, true, false>', 'wgrad_bf16_kernel<3, false, 8, 4, 1, 8>')),
    C('bf_premask_gather_32', (2, 24, 16, 16, 32, 3, True, False, True, False, False), True, {'premask': True},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, true, true>', 'wgrad_bf16_kernel<3, false, 8, 4, 1, 8>')),
    C('bf_premask_gather_96', (1, 24, 64, 32, 32, 3, True, False, True, False, False), True, {'premask': True},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 1, false, false, true, true>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_bf16_kernel<3, false, 8, 4, 1, 8>')),
    C('bf_premask_gather_up', (1, 96, 64, 32, 32, 3, True, True, True, False, False), True, {'premask': True},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 2, false, false, true, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_bf16_kernel<3, false, 8, 4, 1, 8>')),
    C('bf_gather_32', (2, 24, 16, 16, 32, 3, True, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, true>', 'wgrad_bf16_kernel<3, false, 8, 4, 1, 8>')),
    C('bf_gather_64', (1, 24, 32, 32, 32, 3, True, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, true>', 'wgrad_bf16_kernel<3, false, 8, 4, 2, 8>')),
    C('bf_gather_up_n96', (1, 96, 64, 32, 32, 3, True, True, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 2, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_bf16_kernel<3, false, 8, 4, 1, 8>')),
    C('bf_tail8_14_32', (2, 16, 14, 0, 32, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 8, 1, false, true, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 2, 8, 1, 8>')),
    C('bf_tail8_14_64', (1, 16, 14, 0, 64, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 2, 2, 8, 1, false, true, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 2, 8, 1, 8>')),
    C('bf_tail8_26_32', (2, 16, 26, 0, 32, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, true, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 2, 16, 1, 8>')),
    C('bf_tail8_26_64', (1, 16, 26, 0, 64, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 2, 2, 8, 1, false, true, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 2, 16, 1, 8>')),
    C('f32_pw_v4', (2, 8, 8, 0, 8, 1, False, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 1, 8, 3, 1, 4, 1, 4, 0, false, false, false, false>', 'wgrad_mfma_kernel<float, 1, 4, true>')),
    C('f32_pw_v4_dx', (2, 8, 8, 0, 8, 1, False, False, True, False, True), False, {'wgrad': False},
      ('conv_mfma_ws_kernel<float, 1, 8, 3, 1, 4, 1, 4, 0, false, false, false, false>', 'conv_mfma_ws_kernel<float, 1, 8, 3, 1, 4, 1, 4, 0, true, false, false, false>')),
    C('f32_pw_v2', (2, 8, 6, 0, 10, 1, False, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 1, 8, 3, 1, 4, 1, 2, 0, false, false, false, false>', 'conv_mfma_ws_kernel<float, 1, 8, 3, 1, 4, 1, 2, 0, true, false, false, false>', 'wgrad_mfma_kernel<float, 1, 2, true>')),
    C('f32_pw_v1', (2, 8, 5, 0, 7, 1, False, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 1, 8, 3, 1, 4, 1, 1, 0, true, false, false, false>', 'conv_mfma_ws_kernel<float, 1, 8, 3, 1, 4, 1, 4, 0, false, false, false, false>', 'wgrad_mfma_kernel<float, 1, 4, true>')),
    C('f32_pw_v4_noact', (2, 8, 8, 0, 8, 1, False, False, True, True, False), False, {},
      ('conv_mfma_ws_kernel<float, 1, 8, 3, 1, 4, 1, 4, 0, false, false, false, false>', 'wgrad_mfma_kernel<float, 1, 4, false>')),
    C('f32_pw_v2_noact', (2, 8, 6, 0, 10, 1, False, False, True, False, False), False, {},
      ('conv_mfma_ws_kernel<float, 1, 8, 3, 1, 4, 1, 2, 0, false, false, false, false>', 'wgrad_mfma_kernel<float, 1, 2, false>')),
    C('f32_pw_v1_noact', (2, 8, 5, 0, 7, 1, False, False, True, False, False), False, {},
      ('conv_mfma_ws_kernel<float, 1, 8, 3, 1, 4, 1, 1, 0, false, false, false, false>', 'conv_mfma_ws_kernel<float, 1, 8, 3, 1, 4, 1, 4, 0, false, false, false, false>', 'wgrad_mfma_kernel<float, 1, 4, false>')),
    C('bf_pw_v8', (2, 8, 8, 0, 8, 1, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'wgrad_bf16_kernel<1, true, 8, 4, 1, 8>')),
    C('bf_pw_v8_dx', (2, 8, 8, 0, 8, 1, False, False, True, False, True), True, {'wgrad': False},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, true, false, false, false>')),
    C('bf_pw_v2', (2, 8, 6, 0, 10, 1, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 2, 0, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 2, 0, true, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 1, 2, true>')),
    C('bf_pw_v1', (2, 8, 5, 0, 7, 1, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 1, 0, true, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 1, 8, true>')),
    C('bf_pw_v8_noact', (2, 8, 8, 0, 8, 1, False, False, True, True, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'wgrad_bf16_kernel<1, false, 8, 4, 1, 8>')),
    C('bf_pw_v2_noact', (2, 8, 6, 0, 10, 1, False, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 2, 0, false, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 1, 2, false>')),
    C('bf_pw_v1_noact', (2, 8, 5, 0, 7, 1, False, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 1, 0, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 1, 8, false>')),
    C('bf_pw_head16', (2, 8, 32, 0, 16, 1, False, False, True, False, False), True, {},
      ('pw_dgrad_kernel<false>', 'pw_fwd_kernel<false, 1>', 'wgrad_bf16_kernel<1, false, 8, 4, 1, 8>')),
    C('bf_pw_head32', (2, 8, 32, 0, 32, 1, False, False, True, False, False), True, {},
      ('pw_dgrad_kernel<false>', 'pw_fwd_kernel<false, 2>', 'wgrad_bf16_kernel<1, false, 8, 4, 1, 8>')),
    C('bf_pw_head16_act', (2, 8, 32, 0, 16, 1, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'pw_fwd_kernel<true, 1>', 'wgrad_bf16_kernel<1, true, 8, 4, 1, 8>')),
    C('bf_pw_head32_act', (2, 8, 32, 0, 32, 1, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'pw_fwd_kernel<true, 2>', 'wgrad_bf16_kernel<1, true, 8, 4, 1, 8>')),
    C('bf_pw_head_premask', (2, 8, 32, 0, 16, 1, False, False, True, False, False), True, {'premask': True},
      ('pw_dgrad_kernel<true>', 'pw_fwd_kernel<false, 1>', 'wgrad_bf16_kernel<1, false, 8, 4, 1, 8>')),
    C('bf_pw_14', (2, 8, 8, 0, 14, 1, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 2, 0, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'wgrad_bf16_kernel<1, true, 8, 4, 1, 2>')),
    C('bf_pw_14_noact', (2, 8, 8, 0, 14, 1, False, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 2, 0, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'wgrad_bf16_kernel<1, false, 8, 4, 1, 2>')),
    C('f32_wg_v2', (2, 8, 6, 0, 8, 3, True, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 8, 3, 1, 4, 1, 2, 1, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 2, true>')),
    C('f32_wg_v1', (2, 8, 5, 0, 8, 3, True, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_wg_v2_noact', (2, 8, 6, 0, 8, 3, True, False, True, False, False), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 8, 3, 1, 4, 1, 2, 1, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 2, false>')),
    C('f32_wg_v1_noact', (2, 8, 5, 0, 8, 3, True, False, True, False, False), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, false>')),
    C('f32_wg_v4_noact', (2, 8, 8, 0, 8, 3, True, False, True, False, False), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, false>')),
    C('bf_wg_mfma_v8', (2, 8, 8, 8, 7, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 1, 2, true, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 3, 8, true>')),
    C('bf_wg_mfma_v8_noact', (2, 8, 8, 8, 7, 3, True, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 1, 2, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 3, 8, false>')),
    C('bf_wg_mfma_v2', (2, 8, 6, 0, 7, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 1, 2, true, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 2, 1, false, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 3, 2, true>')),
    C('bf_wg_mfma_v2_noact', (2, 8, 6, 0, 7, 3, True, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 1, 2, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 2, 1, false, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 3, 2, false>')),
    C('bf_wg_mfma_v1', (2, 8, 5, 0, 7, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 1, 2, true, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 3, 8, true>')),
    C('bf_wg_mfma_v1_noact', (2, 8, 5, 0, 7, 3, True, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 1, 2, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 3, 8, false>')),
    C('bf_wg_mfma1_v8', (2, 8, 8, 0, 7, 1, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 1, 0, true, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 1, 8, true>')),
    C('bf_wg_mfma1_v8_noact', (2, 8, 8, 0, 7, 1, False, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 1, 0, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 1, 8, false>')),
    C('bf_wg_mfma1_v2', (2, 8, 6, 0, 7, 1, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 1, 0, true, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 2, 0, false, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 1, 2, true>')),
    C('bf_wg_mfma1_v2_noact', (2, 8, 6, 0, 7, 1, False, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 1, 0, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 2, 0, false, false, false, false>', 'wgrad_mfma_kernel<unsigned short, 1, 2, false>')),
    C('bf_wg_ct2', (2, 12, 32, 32, 32, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 8, 4, 2, 8>')),
    C('bf_wg_ct2_noact', (2, 12, 32, 32, 32, 3, True, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, false, 8, 4, 2, 8>')),
    C('bf_wg_ct1', (2, 12, 16, 8, 16, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 8, 4, 1, 8>')),
    C('bf_wg_ct1_noact', (2, 12, 16, 8, 16, 3, True, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, false, 8, 4, 1, 8>')),
    C('bf_wg_qx8', (2, 12, 6, 0, 16, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 2, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 2, 8, 1, 8>')),
    C('bf_wg_qx8_noact', (2, 12, 6, 0, 16, 3, True, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 2, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, false, 2, 8, 1, 8>')),
    C('bf_wg_qx16', (2, 12, 22, 0, 16, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, true, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 2, 16, 1, 8>')),
    C('bf_wg_qx16_noact', (2, 12, 22, 0, 16, 3, True, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, true, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, false, 2, 16, 1, 8>')),
    C('bf_wg1_ct2', (2, 8, 64, 0, 16, 1, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'wgrad_bf16_kernel<1, true, 8, 4, 2, 8>')),
    C('bf_wg1_ct2_noact', (2, 8, 64, 0, 16, 1, False, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'wgrad_bf16_kernel<1, false, 8, 4, 2, 8>')),
    C('bf_wg1_ct1', (2, 8, 24, 0, 16, 1, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'wgrad_bf16_kernel<1, true, 8, 4, 1, 8>')),
    C('bf_wg1_ct1_noact', (2, 8, 24, 0, 16, 1, False, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'wgrad_bf16_kernel<1, false, 8, 4, 1, 8>')),
    C('bf_wg1_qx8', (2, 8, 6, 0, 16, 1, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 2, 0, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'wgrad_bf16_kernel<1, true, 2, 8, 1, 8>')),
    C('bf_wg1_qx8_noact', (2, 8, 6, 0, 16, 1, False, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 2, 0, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'wgrad_bf16_kernel<1, false, 2, 8, 1, 8>')),
    C('bf_wg1_qx16', (2, 8, 22, 0, 16, 1, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 2, 0, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'wgrad_bf16_kernel<1, true, 2, 16, 1, 8>')),
    C('bf_wg1_qx16_noact', (2, 8, 22, 0, 16, 1, False, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 2, 0, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 1, 16, 3, 1, 4, 1, 8, 0, false, false, false, false>', 'wgrad_bf16_kernel<1, false, 2, 16, 1, 8>')),
]

# Column strips (N = 96, fp32 / bf16, 32 -> 32, B = 2): pix 384 (8 rows of a 48-column strip), ncol 2, nblk 12,
#   ntiles 288 > gx 256 -- workers take a second tile; lds 135296 (fp32) / 127104 (bf16).
# N = 96, 64 -> 64 and 128 -> 64: 2 x 2 tiling, pix 192, ncol 2, nblk 24, ntiles 288, gx 256, lds 140160 (fp32) / 131968;
#   bf16 128 -> 64 takes the 4 x 1 tiling (3-4 chunks, face > 320 px): pix 384, ncol 2, ntiles 144, gx 128, lds 127104.
# Decoder N = 96 (48 -> 96 upsampled + 32 skip -> 32), bf16: pix 384, ncol 2, wstat 3 (three resident weight areas),
#   lds 145536.
# Quad-store epilogue (f32_n80_*_64): fp32 2 x 2 tiling at N = 80, pix 192, ncol 1, nblk 34, ntiles 204, gx 204:
#   2 x (in 39360 + w 36864) + patches 18432 = 170880 > 160 KiB -> patches 0, lds 152448 (bf16 at N = 80 keeps the patches:
#   lds 162688).
# Pooled second output (bf16 *_pool): 32 -> 32 pix 384, ncol 2, pool 1 (row pairs), lds 147584; 32 -> 64 pix 192, ncol 2,
#   pool 1, lds 152448.  fp32 at N = 96: the patches x MT do not fit, the caller pools (pool 0).  The half-row split
#   (colsplit 1) needs a 96-wide tile row and four consumer waves: NOSTRIP_CASES below.
# Gather-form data gradient at N = 96 with an upsampled source (bf_gather_up_n96_64: 32 up + 32 skip -> 32, 64 gradient
#   channels -> NTtot 2 -> the EDGE 4 x 1 tiling): pix 384 = 4 rows of 96, ncol 1, nblk 24, ntiles 144, gx 144; its 2 x 2
#   block sums would need 2 x (in 47040 + w 24576) + 3 x 10240 = 173952 > 160 KiB -> pool 0, lds 153472: the upsampled
#   source's gradient goes through the workspace and one window-sum launch.  bf_gather_up_n96 / bf_premask_gather_up (96
#   gradient channels, NTtot 3) take the EDGE 2 x 2 tiling, which loses its patches at N = 96 (no direct stores): they fall
#   back to the padded grid (MODE_ZERO 2 x 2, declared below).
# 'valid' 3x3 with 33-64 / > 64 output channels: faces of <= 320 px (N = 18 -> 16 x 16: 2 x 2 tiling, pix 192, ntiles 24 /
#   12; > 64: the 5 x 1 x 1 x 4 tiling) and > 320 px (N = 24 -> 22 x 22: split over output-channel groups, pix 176, ntiles 18).
# bf_n96_odd / bf_n96_vw1: 2-byte vectors on a wide face -- 48 input vectors per producer thread, slots >= 32 in use
#   (data gradient: 7 x 100 px tile; forward without strips: 6 x 98 px); the 32-bit validity mask lost their bits (fixed in
#   conv_ws.h: OkMask).
CASES += [
    C('bf_gather_up_n96_64', (1, 96, 32, 32, 32, 3, T, T, T, F, F), T, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, true>',)),
    C('bf_n96_vw1', (1, 96, 6, 5, 9, 3, T, F, T, F, T), T, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 1, 1, false, false, false, false>',
       'conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 1, 2, true, false, false, false>',
       'wgrad_mfma_kernel<unsigned short, 3, 1, true>')),
    C('f32_vw1', (2, 8, 6, 5, 8, 3, T, F, T, F, T), F, {},
      ('conv_mfma_ws_kernel<float, 3, 8, 3, 1, 4, 1, 1, 1, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 1, true>')),
    C('f32_vw1_noact', (2, 8, 6, 5, 8, 3, T, F, T, F, F), F, {}, ('wgrad_mfma_kernel<float, 3, 1, false>',)),
    C('bf_vw1', (2, 8, 6, 5, 8, 3, T, F, T, F, T), T, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 1, 1, false, false, false, false>',
       'wgrad_mfma_kernel<unsigned short, 3, 1, true>')),
    C('bf_vw1_noact', (2, 8, 6, 5, 8, 3, T, F, T, F, F), T, {}, ('wgrad_mfma_kernel<unsigned short, 3, 1, false>',)),
    C('f32_valid_vw1', (1, 10, 6, 5, 8, 3, F, F, T, F, T), F, {},
      ('conv_mfma_ws_kernel<float, 3, 8, 3, 1, 4, 1, 1, 0, false, false, false, false>',)),
    C('bf_valid_vw1', (1, 10, 6, 5, 8, 3, F, F, T, F, T), T, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 1, 0, false, false, false, false>',)),
    C('f32_pw_vw1', (2, 8, 6, 5, 8, 1, F, F, T, F, T), F, {}, ('wgrad_mfma_kernel<float, 1, 1, true>',)),
    C('f32_pw_vw1_noact', (2, 8, 6, 5, 8, 1, F, F, T, F, F), F, {}, ('wgrad_mfma_kernel<float, 1, 1, false>',)),
    C('bf_pw_vw1', (2, 8, 6, 5, 8, 1, F, F, T, F, T), T, {}, ('wgrad_mfma_kernel<unsigned short, 1, 1, true>',)),
    C('bf_pw_vw1_noact', (2, 8, 6, 5, 8, 1, F, F, T, F, F), T, {}, ('wgrad_mfma_kernel<unsigned short, 1, 1, false>',)),
    C('f32_dx_vw1_noact', (1, 8, 8, 0, 7, 3, T, F, T, F, F), F, {},
      ('conv_mfma_ws_kernel<float, 3, 8, 3, 1, 4, 1, 1, 2, false, false, false, false>',)),
    C('f32_dx_vw2_noact', (1, 8, 8, 0, 6, 3, T, F, T, F, F), F, {},
      ('conv_mfma_ws_kernel<float, 3, 8, 3, 1, 4, 1, 2, 2, false, false, false, false>',)),
    C('bf_dx_vw2_noact', (1, 8, 8, 0, 6, 3, T, F, T, F, F), T, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 4, 1, 2, 2, false, false, false, false>',)),
]

# DLWPCS_TUNE without TUNE_CONV_SPLIT_N (16): > 64 channels no longer split over output-channel groups -- the 3 x 1 x 1 x 4
# tilings (faces > 320 px) and, for the data gradient, the 5 x 1 x 1 x 4 ones (<= 320 px).  Run in a fresh process
# (tune_bits() is read once per process).
TUNE = 16247 & ~16
TUNE_CASES = [
    C('f32_halo_96out_large', (1, 24, 32, 0, 96, 3, True, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 8, 3, 1, 1, 4, 4, 1, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_valid_96out_large', (1, 26, 32, 0, 96, 3, False, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 8, 3, 1, 1, 4, 4, 0, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_halo_96in_large', (1, 24, 96, 0, 32, 3, True, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 8, 3, 1, 1, 4, 4, 2, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_halo_96in_small', (1, 16, 96, 0, 32, 3, True, False, True, False, True), False, {},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 8, 3, 1, 1, 4, 4, 2, false, false, false, false>', 'wgrad_mfma_kernel<float, 3, 4, true>')),
    C('f32_halo_96in_small_dx', (1, 16, 96, 0, 32, 3, True, False, True, False, True), False, {'wgrad': False},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 8, 3, 1, 1, 4, 4, 2, true, false, false, false>')),
    C('f32_halo_96in_large_dx', (1, 24, 96, 0, 32, 3, True, False, True, False, True), False, {'wgrad': False},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 8, 3, 1, 1, 4, 4, 2, true, false, false, false>')),
    C('bf_halo_96out_large', (1, 24, 32, 0, 96, 3, True, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 1, 4, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, true>', 'wgrad_bf16_kernel<3, true, 8, 4, 1, 8>')),
    C('bf_valid_96out_large', (1, 26, 32, 0, 96, 3, False, False, True, False, True), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 1, 4, 8, 0, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, false, false, false, false>', 'wgrad_bf16_kernel<3, true, 8, 4, 1, 8>')),
    C('bf_halo_96in_large', (1, 24, 64, 32, 32, 3, True, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 1, 4, 8, 1, false, false, false, true>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_bf16_kernel<3, false, 8, 4, 1, 8>')),
    C('bf_halo_96in_small', (1, 16, 64, 32, 32, 3, True, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 1, 4, 8, 2, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_bf16_kernel<3, false, 8, 4, 1, 8>')),
    C('bf_halo_96in_small_dx', (1, 16, 96, 0, 32, 3, True, False, True, False, True), True, {'wgrad': False},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 1, 4, 8, 2, true, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>')),
    C('bf_halo_96in_large_dx', (1, 24, 96, 0, 32, 3, True, False, True, False, True), True, {'wgrad': False},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 1, 4, 8, 2, true, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>')),
    C('bf_premask_grid_96_small', (1, 6, 64, 32, 16, 3, True, False, True, False, False), True, {'premask': True},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 5, 1, 1, 4, 8, 2, false, false, true, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_bf16_kernel<3, false, 8, 4, 1, 8>')),
    C('bf_premask_grid_96_large', (1, 20, 64, 32, 16, 3, True, False, True, False, False), True, {'premask': True},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 1, 4, 8, 1, false, false, true, true>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_bf16_kernel<3, false, 8, 4, 1, 8>')),
    C('bf_premask_gather_96', (1, 24, 64, 32, 32, 3, True, False, True, False, False), True, {'premask': True},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 1, 4, 8, 1, false, false, true, true>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'wgrad_bf16_kernel<3, false, 8, 4, 1, 8>')),
    C('bf_gather_64', (1, 24, 32, 32, 32, 3, True, False, True, False, False), True, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, true>', 'wgrad_bf16_kernel<3, false, 8, 4, 2, 8>')),
    C('bf_premask_gather_64', (1, 24, 32, 32, 32, 3, True, False, True, False, False), True, {'premask': True},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, true, true>', 'wgrad_bf16_kernel<3, false, 8, 4, 2, 8>')),
    C('f32_dx_only_64', (1, 12, 64, 0, 32, 3, True, False, True, False, True), False, {'wgrad': False},
      ('conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 1, false, false, false, false>', 'conv_mfma_ws_kernel<float, 3, 16, 3, 1, 4, 1, 4, 2, true, false, false, false>')),
    C('bf_dx_only_64', (1, 24, 64, 0, 32, 3, True, False, True, False, True), True, {'wgrad': False},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>', 'conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 2, true, false, false, false>')),
    C('f32_dx96_small', (1, 12, 96, 0, 32, 3, T, F, T, F, F), F, {},
      ('conv_mfma_ws_kernel<float, 3, 8, 5, 1, 1, 4, 4, 2, false, false, false, false>',)),
    C('f32_dx96_small_mask', (1, 12, 96, 0, 32, 3, T, F, T, F, T), F, {'wgrad': False},
      ('conv_mfma_ws_kernel<float, 3, 8, 5, 1, 1, 4, 4, 2, true, false, false, false>',)),
    C('bf_dx96_small', (1, 12, 96, 0, 32, 3, T, F, T, F, F), T, {},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 5, 1, 1, 4, 8, 2, false, false, false, false>',)),
    C('bf_dx96_small_mask', (1, 12, 96, 0, 32, 3, T, F, T, F, T), T, {'wgrad': False},
      ('conv_mfma_ws_kernel<unsigned short, 3, 16, 5, 1, 1, 4, 8, 2, true, false, false, false>',)),
]

# DLWPCS_TUNE without TUNE_CONV_STRIPS (1024): the pooled second output with the half-row split.  bf16 32 -> 32 at N = 96,
# one 96-wide strip: pix 384 = 4 rows of 96 (32 * MT = 96 = one row per consumer wave: no row pairs -> halfrows), ncol 1,
# nblk 24, ntiles 144, gx 144; 2 x (in 47040 + w 18432) + 3 patches x 10240 = 161664 <= 160 KiB -> pool 1, colsplit 1.
# (fp32: the three patches need 55296 bytes -> the caller pools; with strips on, 8-row bands of 48 columns pool by row pairs.)
NOSTRIP_TUNE = 16247 & ~1024
NOSTRIP_CASES = [
    C('bf_n96_pool_colsplit', (1, 96, 32, 0, 32, 3, T, F, T, F, T), T, {'want_pool': True},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>',)),
    C('bf_n96_pool_colsplit_b2', (2, 96, 32, 0, 32, 3, T, F, T, T, F), T, {'want_pool': True},
      ('conv_mfma_ws_kernel<unsigned short, 3, 32, 3, 1, 4, 1, 8, 1, false, false, false, false>',)),
]

_TL = 'conv_mfma_ws_kernel<unsigned short, 3, 16, 3, 1, 1, 4, 8, 2, false, false, true, false>'
UNREACHABLE = {
    _TL: 'pre-masked padded-grid data gradient, > 64 channels, face > 320 px, SPLIT_N off: the gather form takes such layers '
         '(conv_mfma.hip conv_bwd_data_impl, DLWPCS_CONV_DGRAD_GATHER branch) unless dgrad_gather=0 as well',
    'pw_head_train_kernel<1>': 'fused training tail dlwpcs_head_mse_step (conv_mfma.hip head_launch), not launched by cs_conv; '
                               'test_gpu_pointwise_head.py',
    'pw_head_train_kernel<2>': 'fused training tail dlwpcs_head_mse_step (conv_mfma.hip head_launch), not launched by cs_conv; '
                               'test_gpu_pointwise_head.py',
    'wgrad_batch_kernel': 'batched weight gradient of a whole backward pass (wgrad_batch.hip, ops.flush_wgrad_batch), '
                          'not per-layer cs_conv; test_gpu_wgrad_batch.py',
    'wb_reduce_kernel': 'reduction of the batched weight gradient (wgrad_batch.hip), not per-layer cs_conv; '
                        'test_gpu_wgrad_batch.py',
    'wb_reduce_kernel(apply)': 'reduction + optimizer of the batched weight gradient (wgrad_batch.hip, '
                               'dlwpcs_wgrad_batch_apply), not per-layer cs_conv; test_gpu_wgrad_batch.py',
    'wgrad_reduce_batch_kernel': 'deferred reduction of several layers (ops.py:105 dlwpcs_wgrad_reduce_batch, '
                                 'DEFER_WGRAD_REDUCE in Model), not per-layer cs_conv; test_gpu_wgrad_batch.py',
}


def _check(c):
    with conv_check.launched_tags() as tags:
        errs = conv_check.check(c.case, c.bf16, device_mask=True, **c.kw)
    missing = sorted(set(c.tags) - tags)
    assert not missing, 'not launched: %s (launched: %s)' % (missing, sorted(tags))
    return errs


@pytest.mark.parametrize('c', CASES, ids=lambda c: c.name)
def test_conv_case(c):
    _check(c)


_TUNE_CHILD = r"""
import sys
sys.path[:0] = sys.argv[2:5]
import test_gpu_conv_coverage as cov
for c in getattr(cov, sys.argv[1]):
    cov._check(c)                       # (the first failure ends the process: nothing more is launched after it)
    print('__OK__ ' + c.name, flush=True)
"""


def _run_child(tune, cases):
    env = dict(os.environ, DLWPCS_TUNE=str(tune))
    r = subprocess.run([sys.executable, '-c', _TUNE_CHILD, cases, ROOT, os.path.join(ROOT, 'dlwp-cs_amd'), os.path.join(ROOT, 'tests')],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    done = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith('__OK__ ')]
    assert done == [c.name for c in globals()[cases]], r.stdout[-2000:]


def test_conv_cases_without_output_channel_split():
    _run_child(TUNE, 'TUNE_CASES')


def test_conv_cases_without_column_strips():
    _run_child(NOSTRIP_TUNE, 'NOSTRIP_CASES')


# Face-size surface: per finest face size N, the layer shapes of a U-Net at that level (14 -> 32, 32 -> 32, 32 -> 64 3x3
# halo, and a decoder 64 (upsampled from N / 2) + 32 -> 32), fp32 and bf16, B = 1.  Each pass is run and checked on its own --
# forward alone, then data gradient alone (mask on load), then weight gradient alone -- and, where all three are served, the
# training combination (weight gradient first, dz handed over; bf16 takes the gather-form data gradient then).  Observed
# outcome, frozen as 'fwd/dgrad/wgrad/train' with 'ok' (matches the oracle), 'refused' (NotImplementedError,
# DLWPCS_E_UNSUPPORTED) or '-' (not run: no forward).
FACE_SHAPES = {'enc_14_32': (14, 0, 32, False), 'enc_32_32': (32, 0, 32, False), 'enc_32_64': (32, 0, 64, False),
               'dec_64_32_up': (64, 32, 32, True)}
FACE_SIZES = {
    64: {('dec_64_32_up', 'bf16'): 'ok/ok/ok/ok', ('dec_64_32_up', 'f32'): 'ok/ok/ok/ok',
         ('enc_14_32', 'bf16'): 'ok/ok/ok/ok', ('enc_14_32', 'f32'): 'ok/ok/ok/ok',
         ('enc_32_32', 'bf16'): 'ok/ok/ok/ok', ('enc_32_32', 'f32'): 'ok/ok/ok/ok',
         ('enc_32_64', 'bf16'): 'ok/ok/ok/ok', ('enc_32_64', 'f32'): 'ok/ok/ok/ok'},
    72: {('dec_64_32_up', 'bf16'): 'ok/ok/ok/ok', ('dec_64_32_up', 'f32'): 'ok/ok/ok/ok',
         ('enc_14_32', 'bf16'): 'ok/ok/ok/ok', ('enc_14_32', 'f32'): 'ok/ok/ok/ok',
         ('enc_32_32', 'bf16'): 'ok/ok/ok/ok', ('enc_32_32', 'f32'): 'ok/ok/ok/ok',
         ('enc_32_64', 'bf16'): 'ok/ok/ok/ok', ('enc_32_64', 'f32'): 'ok/ok/ok/ok'},
    80: {('dec_64_32_up', 'bf16'): 'ok/ok/ok/ok', ('dec_64_32_up', 'f32'): 'ok/ok/ok/ok',
         ('enc_14_32', 'bf16'): 'ok/ok/ok/ok', ('enc_14_32', 'f32'): 'ok/ok/ok/ok',
         ('enc_32_32', 'bf16'): 'ok/ok/ok/ok', ('enc_32_32', 'f32'): 'ok/ok/ok/ok',
         ('enc_32_64', 'bf16'): 'ok/ok/ok/ok', ('enc_32_64', 'f32'): 'ok/ok/ok/ok'},
    96: {('dec_64_32_up', 'bf16'): 'ok/ok/ok/ok', ('dec_64_32_up', 'f32'): 'ok/ok/ok/ok',
         ('enc_14_32', 'bf16'): 'ok/ok/ok/ok', ('enc_14_32', 'f32'): 'ok/ok/ok/ok',
         ('enc_32_32', 'bf16'): 'ok/ok/ok/ok', ('enc_32_32', 'f32'): 'ok/ok/ok/ok',
         ('enc_32_64', 'bf16'): 'ok/ok/ok/ok', ('enc_32_64', 'f32'): 'ok/ok/ok/ok'},
    112: {('dec_64_32_up', 'bf16'): 'refused/-/-/-', ('dec_64_32_up', 'f32'): 'refused/-/-/-',
         ('enc_14_32', 'bf16'): 'refused/-/-/-', ('enc_14_32', 'f32'): 'refused/-/-/-',
         ('enc_32_32', 'bf16'): 'refused/-/-/-', ('enc_32_32', 'f32'): 'refused/-/-/-',
         ('enc_32_64', 'bf16'): 'refused/-/-/-', ('enc_32_64', 'f32'): 'refused/-/-/-'},
    120: {('dec_64_32_up', 'bf16'): 'refused/-/-/-', ('dec_64_32_up', 'f32'): 'refused/-/-/-',
         ('enc_14_32', 'bf16'): 'refused/-/-/-', ('enc_14_32', 'f32'): 'refused/-/-/-',
         ('enc_32_32', 'bf16'): 'refused/-/-/-', ('enc_32_32', 'f32'): 'refused/-/-/-',
         ('enc_32_64', 'bf16'): 'refused/-/-/-', ('enc_32_64', 'f32'): 'refused/-/-/-'},
    128: {('dec_64_32_up', 'bf16'): 'ok/refused/ok/refused', ('dec_64_32_up', 'f32'): 'ok/refused/ok/refused',
         ('enc_14_32', 'bf16'): 'ok/refused/ok/refused', ('enc_14_32', 'f32'): 'ok/refused/ok/refused',
         ('enc_32_32', 'bf16'): 'ok/refused/ok/ok', ('enc_32_32', 'f32'): 'ok/refused/ok/refused',
         ('enc_32_64', 'bf16'): 'refused/-/-/-', ('enc_32_64', 'f32'): 'ok/refused/ok/refused'},
    144: {('dec_64_32_up', 'bf16'): 'refused/-/-/-', ('dec_64_32_up', 'f32'): 'ok/refused/ok/refused',
         ('enc_14_32', 'bf16'): 'refused/-/-/-', ('enc_14_32', 'f32'): 'ok/refused/ok/refused',
         ('enc_32_32', 'bf16'): 'refused/-/-/-', ('enc_32_32', 'f32'): 'ok/refused/ok/refused',
         ('enc_32_64', 'bf16'): 'refused/-/-/-', ('enc_32_64', 'f32'): 'refused/-/-/-'},
    160: {('dec_64_32_up', 'bf16'): 'refused/-/-/-', ('dec_64_32_up', 'f32'): 'refused/-/-/-',
         ('enc_14_32', 'bf16'): 'refused/-/-/-', ('enc_14_32', 'f32'): 'refused/-/-/-',
         ('enc_32_32', 'bf16'): 'refused/-/-/-', ('enc_32_32', 'f32'): 'refused/-/-/-',
         ('enc_32_64', 'bf16'): 'refused/-/-/-', ('enc_32_64', 'f32'): 'refused/-/-/-'},
    192: {('dec_64_32_up', 'bf16'): 'ok/refused/refused/refused', ('dec_64_32_up', 'f32'): 'ok/refused/refused/refused',
         ('enc_14_32', 'bf16'): 'ok/refused/refused/refused', ('enc_14_32', 'f32'): 'ok/refused/refused/refused',
         ('enc_32_32', 'bf16'): 'ok/refused/refused/refused', ('enc_32_32', 'f32'): 'ok/refused/refused/refused',
         ('enc_32_64', 'bf16'): 'ok/refused/refused/refused', ('enc_32_64', 'f32'): 'ok/refused/refused/refused'},
}


def _served(case, bf16, **kw):
    """True: the passes ran and matched the oracle (asserted); False: refused cleanly, and a supported call on the same stream
    is still right afterwards."""
    try:
        conv_check.check(case, bf16, device_mask=True, **kw)
        return True
    except NotImplementedError as e:
        assert 'internal' not in str(e), str(e)
        conv_check.check((1, 8, 16, 0, 16, 3, True, False, True, False, True), bf16)
        return False


def face_outcome(N, shape, dt):
    C0, C1, Cout, up0 = FACE_SHAPES[shape]
    case = (1, N, C0, C1, Cout, 3, True, up0, True, False, True)
    bf16 = dt == 'bf16'
    word = {True: 'ok', False: 'refused'}
    if not _served(case, bf16, dgrad=False, wgrad=False):
        return 'refused/-/-/-'
    dx, dw = _served(case, bf16, wgrad=False), _served(case, bf16, dgrad=False)
    return 'ok/%s/%s/%s' % (word[dx], word[dw], word[_served(case, bf16)])


@pytest.mark.parametrize('N', sorted(FACE_SIZES))
def test_face_size_surface(N):
    seen = {key: face_outcome(N, *key) for key in sorted(FACE_SIZES[N])}
    assert seen == FACE_SIZES[N]
