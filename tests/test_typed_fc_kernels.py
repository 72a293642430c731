"""csrc/typed_fc.hip (K19), launcher by launcher, against plain float64 torch with buffers of the test's own.

The scaffolding of tests/test_lstm_kernels.py and tests/test_lstm_f32_kernels.py: a synthetic ``flat`` with an odd
non-zero ``off`` and ``chunk = K*C + C + 5`` (the 5 gap words of every module and everything outside
``[off, off + M*chunk)`` hold the sentinel, in the parameters and in the gradient buffer), 64 NaN rows after every
input, 64 sentinel rows after every output, a ReLU buffer prefilled with a byte that is neither 0 nor 1, and masks of
exact 0.0 / 1.0 floats built by hand per case (``compose``) over type tables of the test's own.  The backward
launchers get a ReLU mask of random 0 / 1 bytes that no forward produced, inactive planes included, so they are
tested on their own and nothing in their comparison is undetermined.

The reference is the definition in the file header, in float64:

    out_j = x | relu(x W_j + b_j) | relu(x W_j + b_j) + x,   summed over the path's active modules
    dX    = sum_m (dY * relu'_m) W_m^T + nid * dY
    dW_m  = X^T (dY * relu'_m),  db_m = its column sums, over the rows of the paths that use m; zero for a skip
            module and for a module that no path uses

Bounds.  Both engines are k-ordered fp32 fmaf chains: the VALU kernels by construction, and
``v_mfma_f32_16x16x4_f32`` has exact products and one rounding per term (tests/test_lstm_f32_kernels.py).  A chain
of n roundings is within n * 2^-24 * sum|terms| of the exact sum to first order; with EPS = 2^-23 that leaves a factor
2, as in the LSTM suites:

    |hip - ref64| <= n * EPS * (|A| @ |B|)

with n the reduction length plus the extra adds each kernel makes:

  pre-activation  n_pre = K + ceil(K / 256) + 1: the K fmaf of the chain, the add of each 256-wide chunk's partial
                  into the accumulator (VALU; the MFMA kernel keeps one chain and makes none), the bias add;
                  |A| @ |B| = |x| @ |W_m| + |b_m|.
  out             n_pre + nact + 2: one add per active weighted module into the row's sum, and the identity's
                  multiply and add; |A| @ |B| = sum over the active weighted modules of (|x| @ |W_m| + |b_m|), plus
                  nid * |x|.  relu is 1-Lipschitz and relu(pre) <= |x| @ |W| + |b|, so this holds whichever way a
                  pre-activation near zero rounds: ``out`` has no exclusions.
  dx              nact * C + 1: the chain over the active modules' C columns and the identity term
                  (an unfused multiply and add is two roundings of 2^-24, inside the factor 2);
                  |A| @ |B| = sum_m |g_m| @ |W_m|^T + nid * |dy|.
  dW_m, db_m      the number of contributing rows (rpp times the number of paths that use m): one chain across the
                  row chunks in both engines.  No contributing row: bound 0, exact zero asked.

The forward ReLU mask is compared exactly: ``pre64 > 0`` in the planes of the path's active weighted modules, 0 in
every other plane (inactive modules, skip modules, all of [R][M][C] for an all-skip path), the prefill byte in the
rows past the end.  Elements with ``|pre64| <= `` the pre-activation bound are undetermined and left out; they must
be under 1 % of a case (tests/test_typed_fc_host.py asserts the actual maximum on the CPU) and still hold 0 or 1.

The worst measured ratio of every tensor to its bound is kept in tests/data/typed_fc_measured.json (written when
``PATHNET_RECORD_TYPED_FC=<file>`` is set): a record, not a budget.
"""
import json
import os

import pytest
import torch

from test_lstm_kernels import EPS, PAD, SENT, assert_sentinel, bits, gemm_bound, outbuf, padded
from test_lstm_f32_kernels import excess

gpu = pytest.mark.gpu
DEV = "cuda"
PREFILL = 7                          # ReLU buffer prefill: neither 0 nor 1
OFF, GAP, TAIL = 37, 5, 29           # odd offset of the layer, gap words after every module, words after the layer

# the constants of csrc/typed_fc.hip (tests/test_typed_fc_host.py reads them out of the file and compares)
TF_RT, TF_KC, TF_MAXM, TF_MAXC, TF_PPT = 16, 256, 16, 64, 4
WG_KT, WG_RC = 16, 64
TM_T, TM_KC = 64, 32

COMPS = ["allfc", "layer0", "allskip", "nid3", "shared", "unused", "skipactive"]

# ---------------------------------------------------------------------------------------------------------------
# The shapes.  (engine, K, C, rpp, P, M, composition, reach); every row runs fwd, dgrad and wgrad of its engine.
#
# A pairwise selection over the value sets below: every pair of values of (C, rpp), (C, P), (C, M), (C, composition),
# (rpp, P), (rpp, M), (rpp, composition), (P, M), (P, composition), (M, composition) that the constraints allow is in
# some row, and in the rows whose modules are all fc every pair of (K, C) and (K, P).  K is not paired with rpp or M:
# the K loop of every kernel is independent of its row tiling and of its module loop.  Constraints: identity types
# need K == C, so K varies in the all-fc rows only ("layer0" = K != C); compositions with three kinds of module need
# M >= 3.
#   VALU  C {1, 20, 33, 64}          K {1, 15, 16, 17, 255, 256, 257, 513}   rpp {1, 15, 16, 17, 33 | 63, 64, 65, 130}
#   MFMA  C {1, 20, 63, 64, 65, 130} K {1, 3, 31, 32, 33, 64, 65, 100}       rpp {1, 31, 32, 33, 63, 64, 65, 130}
#   both  P {1, 5}, M {1, 3, 10, 16}
# reach = what the row's sizes are against each tile, "tile:full+tail" (``reach`` below recomputes it):
#   VALU  k256 forward K chunks (TF_KC)   r16 forward / dgrad row tiles (TF_RT)   wk16 wgrad k tiles (KT)
#         wr64 wgrad row chunks (RC)      ppt (row, c) pairs per thread, ceil(16 C / 256) (4 = the launcher's last width)
#   MFMA  k32 forward staging chunks (TM_KC)   r64 row tiles (TM_T)   c64 column tiles   c32 dgrad staging chunks
#         k64 dgrad / wgrad k tiles            wr32 wgrad row chunks
# ---------------------------------------------------------------------------------------------------------------
CASES = [
    ("valu", 1, 1, 65, 5, 16, "allfc", "k256:0+1 r16:4+1 wk16:0+1 wr64:1+1 ppt:1"),
    ("valu", 15, 1, 16, 5, 1, "layer0", "k256:0+15 r16:1+0 wk16:0+15 wr64:0+16 ppt:1"),
    ("valu", 16, 1, 33, 5, 1, "layer0", "k256:0+16 r16:2+1 wk16:1+0 wr64:0+33 ppt:1"),
    ("valu", 17, 1, 16, 1, 1, "layer0", "k256:0+17 r16:1+0 wk16:1+1 wr64:0+16 ppt:1"),
    ("valu", 255, 1, 16, 1, 1, "layer0", "k256:0+255 r16:1+0 wk16:15+15 wr64:0+16 ppt:1"),
    ("valu", 256, 1, 63, 1, 16, "layer0", "k256:1+0 r16:3+15 wk16:16+0 wr64:0+63 ppt:1"),
    ("valu", 257, 1, 16, 5, 3, "layer0", "k256:1+1 r16:1+0 wk16:16+1 wr64:0+16 ppt:1"),
    ("valu", 513, 1, 63, 5, 10, "layer0", "k256:2+1 r16:3+15 wk16:32+1 wr64:0+63 ppt:1"),
    ("valu", 1, 20, 64, 1, 3, "layer0", "k256:0+1 r16:4+0 wk16:0+1 wr64:1+0 ppt:2"),
    ("valu", 15, 20, 63, 1, 1, "layer0", "k256:0+15 r16:3+15 wk16:0+15 wr64:0+63 ppt:2"),
    ("valu", 16, 20, 130, 5, 10, "layer0", "k256:0+16 r16:8+2 wk16:1+0 wr64:2+2 ppt:2"),
    ("valu", 17, 20, 130, 5, 16, "layer0", "k256:0+17 r16:8+2 wk16:1+1 wr64:2+2 ppt:2"),
    ("valu", 255, 20, 64, 1, 3, "layer0", "k256:0+255 r16:4+0 wk16:15+15 wr64:1+0 ppt:2"),
    ("valu", 256, 20, 16, 5, 16, "layer0", "k256:1+0 r16:1+0 wk16:16+0 wr64:0+16 ppt:2"),
    ("valu", 257, 20, 33, 5, 3, "layer0", "k256:1+1 r16:2+1 wk16:16+1 wr64:0+33 ppt:2"),
    ("valu", 513, 20, 130, 1, 3, "layer0", "k256:2+1 r16:8+2 wk16:32+1 wr64:2+2 ppt:2"),
    ("valu", 1, 33, 33, 5, 3, "layer0", "k256:0+1 r16:2+1 wk16:0+1 wr64:0+33 ppt:3"),
    ("valu", 15, 33, 1, 5, 1, "layer0", "k256:0+15 r16:0+1 wk16:0+15 wr64:0+1 ppt:3"),
    ("valu", 16, 33, 65, 1, 10, "layer0", "k256:0+16 r16:4+1 wk16:1+0 wr64:1+1 ppt:3"),
    ("valu", 17, 33, 64, 1, 1, "layer0", "k256:0+17 r16:4+0 wk16:1+1 wr64:1+0 ppt:3"),
    ("valu", 255, 33, 17, 5, 3, "layer0", "k256:0+255 r16:1+1 wk16:15+15 wr64:0+17 ppt:3"),
    ("valu", 256, 33, 16, 1, 10, "layer0", "k256:1+0 r16:1+0 wk16:16+0 wr64:0+16 ppt:3"),
    ("valu", 257, 33, 130, 1, 1, "layer0", "k256:1+1 r16:8+2 wk16:16+1 wr64:2+2 ppt:3"),
    ("valu", 513, 33, 15, 1, 1, "layer0", "k256:2+1 r16:0+15 wk16:32+1 wr64:0+15 ppt:3"),
    ("valu", 1, 64, 64, 1, 16, "layer0", "k256:0+1 r16:4+0 wk16:0+1 wr64:1+0 ppt:4"),
    ("valu", 15, 64, 1, 5, 1, "layer0", "k256:0+15 r16:0+1 wk16:0+15 wr64:0+1 ppt:4"),
    ("valu", 16, 64, 15, 1, 10, "layer0", "k256:0+16 r16:0+15 wk16:1+0 wr64:0+15 ppt:4"),
    ("valu", 17, 64, 64, 5, 1, "layer0", "k256:0+17 r16:4+0 wk16:1+1 wr64:1+0 ppt:4"),
    ("valu", 255, 64, 16, 5, 10, "layer0", "k256:0+255 r16:1+0 wk16:15+15 wr64:0+16 ppt:4"),
    ("valu", 256, 64, 65, 5, 1, "layer0", "k256:1+0 r16:4+1 wk16:16+0 wr64:1+1 ppt:4"),
    ("valu", 257, 64, 63, 1, 16, "layer0", "k256:1+1 r16:3+15 wk16:16+1 wr64:0+63 ppt:4"),
    ("valu", 513, 64, 65, 5, 1, "layer0", "k256:2+1 r16:4+1 wk16:32+1 wr64:1+1 ppt:4"),
    ("valu", 1, 1, 16, 5, 16, "allskip", "k256:0+1 r16:1+0 wk16:0+1 wr64:0+16 ppt:1"),
    ("valu", 1, 1, 17, 1, 1, "allskip", "k256:0+1 r16:1+1 wk16:0+1 wr64:0+17 ppt:1"),
    ("valu", 20, 20, 15, 1, 3, "allskip", "k256:0+20 r16:0+15 wk16:1+4 wr64:0+15 ppt:2"),
    ("valu", 20, 20, 65, 1, 1, "allskip", "k256:0+20 r16:4+1 wk16:1+4 wr64:1+1 ppt:2"),
    ("valu", 33, 33, 33, 1, 16, "allskip", "k256:0+33 r16:2+1 wk16:2+1 wr64:0+33 ppt:3"),
    ("valu", 33, 33, 63, 5, 16, "allskip", "k256:0+33 r16:3+15 wk16:2+1 wr64:0+63 ppt:3"),
    ("valu", 64, 64, 1, 5, 10, "allskip", "k256:0+64 r16:0+1 wk16:4+0 wr64:0+1 ppt:4"),
    ("valu", 64, 64, 64, 5, 16, "allskip", "k256:0+64 r16:4+0 wk16:4+0 wr64:1+0 ppt:4"),
    ("valu", 64, 64, 130, 1, 1, "allskip", "k256:0+64 r16:8+2 wk16:4+0 wr64:2+2 ppt:4"),
    ("valu", 1, 1, 1, 5, 16, "nid3", "k256:0+1 r16:0+1 wk16:0+1 wr64:0+1 ppt:1"),
    ("valu", 1, 1, 15, 1, 16, "nid3", "k256:0+1 r16:0+15 wk16:0+1 wr64:0+15 ppt:1"),
    ("valu", 20, 20, 17, 1, 10, "nid3", "k256:0+20 r16:1+1 wk16:1+4 wr64:0+17 ppt:2"),
    ("valu", 20, 20, 65, 1, 3, "nid3", "k256:0+20 r16:4+1 wk16:1+4 wr64:1+1 ppt:2"),
    ("valu", 33, 33, 33, 5, 10, "nid3", "k256:0+33 r16:2+1 wk16:2+1 wr64:0+33 ppt:3"),
    ("valu", 64, 64, 16, 5, 3, "nid3", "k256:0+64 r16:1+0 wk16:4+0 wr64:0+16 ppt:4"),
    ("valu", 64, 64, 63, 1, 16, "nid3", "k256:0+64 r16:3+15 wk16:4+0 wr64:0+63 ppt:4"),
    ("valu", 64, 64, 64, 5, 16, "nid3", "k256:0+64 r16:4+0 wk16:4+0 wr64:1+0 ppt:4"),
    ("valu", 64, 64, 130, 5, 10, "nid3", "k256:0+64 r16:8+2 wk16:4+0 wr64:2+2 ppt:4"),
    ("valu", 1, 1, 16, 5, 16, "shared", "k256:0+1 r16:1+0 wk16:0+1 wr64:0+16 ppt:1"),
    ("valu", 1, 1, 130, 5, 3, "shared", "k256:0+1 r16:8+2 wk16:0+1 wr64:2+2 ppt:1"),
    ("valu", 20, 20, 64, 1, 10, "shared", "k256:0+20 r16:4+0 wk16:1+4 wr64:1+0 ppt:2"),
    ("valu", 33, 33, 1, 5, 16, "shared", "k256:0+33 r16:0+1 wk16:2+1 wr64:0+1 ppt:3"),
    ("valu", 33, 33, 33, 1, 16, "shared", "k256:0+33 r16:2+1 wk16:2+1 wr64:0+33 ppt:3"),
    ("valu", 64, 64, 15, 1, 3, "shared", "k256:0+64 r16:0+15 wk16:4+0 wr64:0+15 ppt:4"),
    ("valu", 64, 64, 17, 1, 3, "shared", "k256:0+64 r16:1+1 wk16:4+0 wr64:0+17 ppt:4"),
    ("valu", 64, 64, 63, 5, 10, "shared", "k256:0+64 r16:3+15 wk16:4+0 wr64:0+63 ppt:4"),
    ("valu", 64, 64, 65, 5, 16, "shared", "k256:0+64 r16:4+1 wk16:4+0 wr64:1+1 ppt:4"),
    ("valu", 1, 1, 1, 5, 10, "unused", "k256:0+1 r16:0+1 wk16:0+1 wr64:0+1 ppt:1"),
    ("valu", 1, 1, 16, 1, 16, "unused", "k256:0+1 r16:1+0 wk16:0+1 wr64:0+16 ppt:1"),
    ("valu", 1, 1, 64, 5, 3, "unused", "k256:0+1 r16:4+0 wk16:0+1 wr64:1+0 ppt:1"),
    ("valu", 20, 20, 65, 1, 10, "unused", "k256:0+20 r16:4+1 wk16:1+4 wr64:1+1 ppt:2"),
    ("valu", 33, 33, 15, 5, 16, "unused", "k256:0+33 r16:0+15 wk16:2+1 wr64:0+15 ppt:3"),
    ("valu", 33, 33, 63, 1, 3, "unused", "k256:0+33 r16:3+15 wk16:2+1 wr64:0+63 ppt:3"),
    ("valu", 33, 33, 130, 5, 16, "unused", "k256:0+33 r16:8+2 wk16:2+1 wr64:2+2 ppt:3"),
    ("valu", 64, 64, 17, 5, 16, "unused", "k256:0+64 r16:1+1 wk16:4+0 wr64:0+17 ppt:4"),
    ("valu", 64, 64, 33, 5, 10, "unused", "k256:0+64 r16:2+1 wk16:4+0 wr64:0+33 ppt:4"),
    ("valu", 1, 1, 15, 5, 16, "skipactive", "k256:0+1 r16:0+15 wk16:0+1 wr64:0+15 ppt:1"),
    ("valu", 1, 1, 16, 1, 10, "skipactive", "k256:0+1 r16:1+0 wk16:0+1 wr64:0+16 ppt:1"),
    ("valu", 20, 20, 1, 1, 3, "skipactive", "k256:0+20 r16:0+1 wk16:1+4 wr64:0+1 ppt:2"),
    ("valu", 33, 33, 17, 1, 10, "skipactive", "k256:0+33 r16:1+1 wk16:2+1 wr64:0+17 ppt:3"),
    ("valu", 33, 33, 33, 1, 10, "skipactive", "k256:0+33 r16:2+1 wk16:2+1 wr64:0+33 ppt:3"),
    ("valu", 33, 33, 64, 1, 3, "skipactive", "k256:0+33 r16:4+0 wk16:2+1 wr64:1+0 ppt:3"),
    ("valu", 33, 33, 65, 5, 3, "skipactive", "k256:0+33 r16:4+1 wk16:2+1 wr64:1+1 ppt:3"),
    ("valu", 64, 64, 63, 5, 16, "skipactive", "k256:0+64 r16:3+15 wk16:4+0 wr64:0+63 ppt:4"),
    ("valu", 64, 64, 130, 1, 10, "skipactive", "k256:0+64 r16:8+2 wk16:4+0 wr64:2+2 ppt:4"),
    ("mfma", 1, 1, 31, 5, 10, "allfc", "k32:0+1 r64:0+31 c64:0+1 c32:0+1 k64:0+1 wr32:0+31"),
    ("mfma", 3, 1, 130, 1, 1, "layer0", "k32:0+3 r64:2+2 c64:0+1 c32:0+1 k64:0+3 wr32:4+2"),
    ("mfma", 31, 1, 33, 1, 1, "layer0", "k32:0+31 r64:0+33 c64:0+1 c32:0+1 k64:0+31 wr32:1+1"),
    ("mfma", 32, 1, 63, 1, 1, "layer0", "k32:1+0 r64:0+63 c64:0+1 c32:0+1 k64:0+32 wr32:1+31"),
    ("mfma", 33, 1, 32, 5, 10, "layer0", "k32:1+1 r64:0+32 c64:0+1 c32:0+1 k64:0+33 wr32:1+0"),
    ("mfma", 64, 1, 1, 5, 16, "layer0", "k32:2+0 r64:0+1 c64:0+1 c32:0+1 k64:1+0 wr32:0+1"),
    ("mfma", 65, 1, 1, 5, 3, "layer0", "k32:2+1 r64:0+1 c64:0+1 c32:0+1 k64:1+1 wr32:0+1"),
    ("mfma", 100, 1, 63, 5, 16, "layer0", "k32:3+4 r64:0+63 c64:0+1 c32:0+1 k64:1+36 wr32:1+31"),
    ("mfma", 1, 20, 64, 1, 16, "layer0", "k32:0+1 r64:1+0 c64:0+20 c32:0+20 k64:0+1 wr32:2+0"),
    ("mfma", 3, 20, 63, 5, 10, "layer0", "k32:0+3 r64:0+63 c64:0+20 c32:0+20 k64:0+3 wr32:1+31"),
    ("mfma", 31, 20, 65, 5, 10, "layer0", "k32:0+31 r64:1+1 c64:0+20 c32:0+20 k64:0+31 wr32:2+1"),
    ("mfma", 32, 20, 130, 5, 3, "layer0", "k32:1+0 r64:2+2 c64:0+20 c32:0+20 k64:0+32 wr32:4+2"),
    ("mfma", 33, 20, 63, 1, 10, "layer0", "k32:1+1 r64:0+63 c64:0+20 c32:0+20 k64:0+33 wr32:1+31"),
    ("mfma", 64, 20, 31, 5, 1, "layer0", "k32:2+0 r64:0+31 c64:0+20 c32:0+20 k64:1+0 wr32:0+31"),
    ("mfma", 65, 20, 63, 5, 3, "layer0", "k32:2+1 r64:0+63 c64:0+20 c32:0+20 k64:1+1 wr32:1+31"),
    ("mfma", 100, 20, 65, 5, 3, "layer0", "k32:3+4 r64:1+1 c64:0+20 c32:0+20 k64:1+36 wr32:2+1"),
    ("mfma", 1, 63, 31, 1, 3, "layer0", "k32:0+1 r64:0+31 c64:0+63 c32:1+31 k64:0+1 wr32:0+31"),
    ("mfma", 3, 63, 64, 5, 1, "layer0", "k32:0+3 r64:1+0 c64:0+63 c32:1+31 k64:0+3 wr32:2+0"),
    ("mfma", 31, 63, 65, 5, 1, "layer0", "k32:0+31 r64:1+1 c64:0+63 c32:1+31 k64:0+31 wr32:2+1"),
    ("mfma", 32, 63, 63, 5, 3, "layer0", "k32:1+0 r64:0+63 c64:0+63 c32:1+31 k64:0+32 wr32:1+31"),
    ("mfma", 33, 63, 31, 1, 3, "layer0", "k32:1+1 r64:0+31 c64:0+63 c32:1+31 k64:0+33 wr32:0+31"),
    ("mfma", 64, 63, 33, 5, 3, "layer0", "k32:2+0 r64:0+33 c64:0+63 c32:1+31 k64:1+0 wr32:1+1"),
    ("mfma", 65, 63, 65, 5, 3, "layer0", "k32:2+1 r64:1+1 c64:0+63 c32:1+31 k64:1+1 wr32:2+1"),
    ("mfma", 100, 63, 33, 1, 1, "layer0", "k32:3+4 r64:0+33 c64:0+63 c32:1+31 k64:1+36 wr32:1+1"),
    ("mfma", 1, 64, 63, 5, 16, "layer0", "k32:0+1 r64:0+63 c64:1+0 c32:2+0 k64:0+1 wr32:1+31"),
    ("mfma", 3, 64, 130, 1, 16, "layer0", "k32:0+3 r64:2+2 c64:1+0 c32:2+0 k64:0+3 wr32:4+2"),
    ("mfma", 31, 64, 65, 1, 16, "layer0", "k32:0+31 r64:1+1 c64:1+0 c32:2+0 k64:0+31 wr32:2+1"),
    ("mfma", 32, 64, 1, 5, 1, "layer0", "k32:1+0 r64:0+1 c64:1+0 c32:2+0 k64:0+32 wr32:0+1"),
    ("mfma", 33, 64, 32, 5, 10, "layer0", "k32:1+1 r64:0+32 c64:1+0 c32:2+0 k64:0+33 wr32:1+0"),
    ("mfma", 64, 64, 64, 5, 16, "allfc", "k32:2+0 r64:1+0 c64:1+0 c32:2+0 k64:1+0 wr32:2+0"),
    ("mfma", 65, 64, 65, 1, 16, "layer0", "k32:2+1 r64:1+1 c64:1+0 c32:2+0 k64:1+1 wr32:2+1"),
    ("mfma", 100, 64, 130, 5, 16, "layer0", "k32:3+4 r64:2+2 c64:1+0 c32:2+0 k64:1+36 wr32:4+2"),
    ("mfma", 1, 65, 130, 5, 3, "layer0", "k32:0+1 r64:2+2 c64:1+1 c32:2+1 k64:0+1 wr32:4+2"),
    ("mfma", 3, 65, 31, 5, 1, "layer0", "k32:0+3 r64:0+31 c64:1+1 c32:2+1 k64:0+3 wr32:0+31"),
    ("mfma", 31, 65, 33, 5, 16, "layer0", "k32:0+31 r64:0+33 c64:1+1 c32:2+1 k64:0+31 wr32:1+1"),
    ("mfma", 32, 65, 32, 1, 16, "layer0", "k32:1+0 r64:0+32 c64:1+1 c32:2+1 k64:0+32 wr32:1+0"),
    ("mfma", 33, 65, 33, 1, 3, "layer0", "k32:1+1 r64:0+33 c64:1+1 c32:2+1 k64:0+33 wr32:1+1"),
    ("mfma", 64, 65, 65, 1, 1, "layer0", "k32:2+0 r64:1+1 c64:1+1 c32:2+1 k64:1+0 wr32:2+1"),
    ("mfma", 65, 65, 65, 5, 16, "allfc", "k32:2+1 r64:1+1 c64:1+1 c32:2+1 k64:1+1 wr32:2+1"),
    ("mfma", 100, 65, 64, 1, 10, "layer0", "k32:3+4 r64:1+0 c64:1+1 c32:2+1 k64:1+36 wr32:2+0"),
    ("mfma", 1, 130, 1, 1, 3, "layer0", "k32:0+1 r64:0+1 c64:2+2 c32:4+2 k64:0+1 wr32:0+1"),
    ("mfma", 3, 130, 130, 1, 3, "layer0", "k32:0+3 r64:2+2 c64:2+2 c32:4+2 k64:0+3 wr32:4+2"),
    ("mfma", 31, 130, 65, 1, 10, "layer0", "k32:0+31 r64:1+1 c64:2+2 c32:4+2 k64:0+31 wr32:2+1"),
    ("mfma", 32, 130, 32, 1, 1, "layer0", "k32:1+0 r64:0+32 c64:2+2 c32:4+2 k64:0+32 wr32:1+0"),
    ("mfma", 33, 130, 32, 1, 1, "layer0", "k32:1+1 r64:0+32 c64:2+2 c32:4+2 k64:0+33 wr32:1+0"),
    ("mfma", 64, 130, 32, 5, 3, "layer0", "k32:2+0 r64:0+32 c64:2+2 c32:4+2 k64:1+0 wr32:1+0"),
    ("mfma", 65, 130, 32, 1, 1, "layer0", "k32:2+1 r64:0+32 c64:2+2 c32:4+2 k64:1+1 wr32:1+0"),
    ("mfma", 100, 130, 32, 1, 1, "layer0", "k32:3+4 r64:0+32 c64:2+2 c32:4+2 k64:1+36 wr32:1+0"),
    ("mfma", 1, 1, 65, 5, 16, "allskip", "k32:0+1 r64:1+1 c64:0+1 c32:0+1 k64:0+1 wr32:2+1"),
    ("mfma", 20, 20, 33, 1, 3, "allskip", "k32:0+20 r64:0+33 c64:0+20 c32:0+20 k64:0+20 wr32:1+1"),
    ("mfma", 63, 63, 1, 5, 16, "allskip", "k32:1+31 r64:0+1 c64:0+63 c32:1+31 k64:0+63 wr32:0+1"),
    ("mfma", 64, 64, 31, 1, 10, "allskip", "k32:2+0 r64:0+31 c64:1+0 c32:2+0 k64:1+0 wr32:0+31"),
    ("mfma", 64, 64, 64, 1, 16, "allskip", "k32:2+0 r64:1+0 c64:1+0 c32:2+0 k64:1+0 wr32:2+0"),
    ("mfma", 65, 65, 32, 1, 16, "allskip", "k32:2+1 r64:0+32 c64:1+1 c32:2+1 k64:1+1 wr32:1+0"),
    ("mfma", 65, 65, 130, 5, 1, "allskip", "k32:2+1 r64:2+2 c64:1+1 c32:2+1 k64:1+1 wr32:4+2"),
    ("mfma", 130, 130, 63, 5, 3, "allskip", "k32:4+2 r64:0+63 c64:2+2 c32:4+2 k64:2+2 wr32:1+31"),
    ("mfma", 1, 1, 33, 5, 16, "nid3", "k32:0+1 r64:0+33 c64:0+1 c32:0+1 k64:0+1 wr32:1+1"),
    ("mfma", 1, 1, 130, 1, 10, "nid3", "k32:0+1 r64:2+2 c64:0+1 c32:0+1 k64:0+1 wr32:4+2"),
    ("mfma", 20, 20, 1, 1, 10, "nid3", "k32:0+20 r64:0+1 c64:0+20 c32:0+20 k64:0+20 wr32:0+1"),
    ("mfma", 63, 63, 63, 5, 16, "nid3", "k32:1+31 r64:0+63 c64:0+63 c32:1+31 k64:0+63 wr32:1+31"),
    ("mfma", 64, 64, 32, 1, 3, "nid3", "k32:2+0 r64:0+32 c64:1+0 c32:2+0 k64:1+0 wr32:1+0"),
    ("mfma", 65, 65, 31, 1, 16, "nid3", "k32:2+1 r64:0+31 c64:1+1 c32:2+1 k64:1+1 wr32:0+31"),
    ("mfma", 65, 65, 65, 5, 16, "nid3", "k32:2+1 r64:1+1 c64:1+1 c32:2+1 k64:1+1 wr32:2+1"),
    ("mfma", 130, 130, 64, 5, 16, "nid3", "k32:4+2 r64:1+0 c64:2+2 c32:4+2 k64:2+2 wr32:2+0"),
    ("mfma", 1, 1, 64, 5, 10, "shared", "k32:0+1 r64:1+0 c64:0+1 c32:0+1 k64:0+1 wr32:2+0"),
    ("mfma", 20, 20, 65, 5, 10, "shared", "k32:0+20 r64:1+1 c64:0+20 c32:0+20 k64:0+20 wr32:2+1"),
    ("mfma", 20, 20, 130, 5, 16, "shared", "k32:0+20 r64:2+2 c64:0+20 c32:0+20 k64:0+20 wr32:4+2"),
    ("mfma", 63, 63, 1, 1, 3, "shared", "k32:1+31 r64:0+1 c64:0+63 c32:1+31 k64:0+63 wr32:0+1"),
    ("mfma", 64, 64, 31, 1, 3, "shared", "k32:2+0 r64:0+31 c64:1+0 c32:2+0 k64:1+0 wr32:0+31"),
    ("mfma", 64, 64, 32, 1, 10, "shared", "k32:2+0 r64:0+32 c64:1+0 c32:2+0 k64:1+0 wr32:1+0"),
    ("mfma", 65, 65, 63, 1, 3, "shared", "k32:2+1 r64:0+63 c64:1+1 c32:2+1 k64:1+1 wr32:1+31"),
    ("mfma", 130, 130, 33, 5, 10, "shared", "k32:4+2 r64:0+33 c64:2+2 c32:4+2 k64:2+2 wr32:1+1"),
    ("mfma", 1, 1, 31, 5, 3, "unused", "k32:0+1 r64:0+31 c64:0+1 c32:0+1 k64:0+1 wr32:0+31"),
    ("mfma", 20, 20, 63, 5, 10, "unused", "k32:0+20 r64:0+63 c64:0+20 c32:0+20 k64:0+20 wr32:1+31"),
    ("mfma", 20, 20, 64, 1, 10, "unused", "k32:0+20 r64:1+0 c64:0+20 c32:0+20 k64:0+20 wr32:2+0"),
    ("mfma", 63, 63, 32, 1, 16, "unused", "k32:1+31 r64:0+32 c64:0+63 c32:1+31 k64:0+63 wr32:1+0"),
    ("mfma", 64, 64, 65, 5, 10, "unused", "k32:2+0 r64:1+1 c64:1+0 c32:2+0 k64:1+0 wr32:2+1"),
    ("mfma", 65, 65, 1, 5, 3, "unused", "k32:2+1 r64:0+1 c64:1+1 c32:2+1 k64:1+1 wr32:0+1"),
    ("mfma", 130, 130, 33, 5, 16, "unused", "k32:4+2 r64:0+33 c64:2+2 c32:4+2 k64:2+2 wr32:1+1"),
    ("mfma", 130, 130, 130, 5, 16, "unused", "k32:4+2 r64:2+2 c64:2+2 c32:4+2 k64:2+2 wr32:4+2"),
    ("mfma", 1, 1, 65, 1, 16, "skipactive", "k32:0+1 r64:1+1 c64:0+1 c32:0+1 k64:0+1 wr32:2+1"),
    ("mfma", 20, 20, 32, 1, 16, "skipactive", "k32:0+20 r64:0+32 c64:0+20 c32:0+20 k64:0+20 wr32:1+0"),
    ("mfma", 20, 20, 63, 5, 16, "skipactive", "k32:0+20 r64:0+63 c64:0+20 c32:0+20 k64:0+20 wr32:1+31"),
    ("mfma", 63, 63, 130, 5, 10, "skipactive", "k32:1+31 r64:2+2 c64:0+63 c32:1+31 k64:0+63 wr32:4+2"),
    ("mfma", 64, 64, 33, 1, 16, "skipactive", "k32:2+0 r64:0+33 c64:1+0 c32:2+0 k64:1+0 wr32:1+1"),
    ("mfma", 64, 64, 64, 1, 3, "skipactive", "k32:2+0 r64:1+0 c64:1+0 c32:2+0 k64:1+0 wr32:2+0"),
    ("mfma", 65, 65, 1, 5, 16, "skipactive", "k32:2+1 r64:0+1 c64:1+1 c32:2+1 k64:1+1 wr32:0+1"),
    ("mfma", 130, 130, 31, 1, 16, "skipactive", "k32:4+2 r64:0+31 c64:2+2 c32:4+2 k64:2+2 wr32:0+31"),
]


def case_id(row):
    eng, K, C, rpp, P, M, comp = row[:7]
    return f"{eng}-K{K}-C{C}-r{rpp}-P{P}-M{M}-{comp}"


def reach(eng, K, C, rpp):
    """The "tile:full+tail" note of a row, from the kernels' constants."""
    d = lambda n, t: f"{n // t}+{n % t}"                                                              # noqa: E731
    if eng == "valu":
        return (f"k256:{d(K, TF_KC)} r16:{d(rpp, TF_RT)} wk16:{d(K, WG_KT)} wr64:{d(rpp, WG_RC)} "
                f"ppt:{-(-TF_RT * C // 256)}")
    return (f"k32:{d(K, TM_KC)} r64:{d(rpp, TM_T)} c64:{d(C, TM_T)} c32:{d(C, TM_KC)} k64:{d(K, TM_T)} "
            f"wr32:{d(rpp, TM_KC)}")


# ---------------------------------------------------------------------------------------------------------------
# path compositions and cases (CPU tensors; also run by tests/test_typed_fc_host.py)
# ---------------------------------------------------------------------------------------------------------------
def compose(comp, P, M):
    """-> (types [M], mask [P][M] of exact 0.0 / 1.0).  Path 0 carries the composition, the other paths take two or
    three neighbouring modules.
      allfc / layer0  every type 1; path 0 uses all M modules (nact = M, at M = 16 the kernels' whole act[] table)
      allskip         types 0, 1, 2, 0, ...; path 0 uses the skip modules only: nact = 0, nid = their number
      nid3            types 0, 2, 2, 1, ...; path 0 = {skip, residual, residual}: nid = 3, nact = 2
      shared          types 2, 1, 0, ...; module 0 (residual) is in every path
      unused          types 1, 2, 0, ...; module 1 (residual: it has weights) is in no path
      skipactive      types 1, 0, 1, 2, ...; every path holds module 0 (fc) and module 1 (a skip that is active)"""
    ring = lambda s, n: {(s + i) % M for i in range(min(n, M))}                                      # noqa: E731
    if comp in ("allfc", "layer0"):
        types = [1] * M
        paths = [set(range(M))] + [ring(2 * p, 3) for p in range(1, P)]
    elif comp == "allskip":
        types = [(0, 1, 2)[j % 3] for j in range(M)]
        paths = [{j for j in range(M) if types[j] == 0}] + [ring(p, 3) for p in range(1, P)]
    elif comp == "nid3":
        types = [(0, 2, 2, 1)[j % 4] for j in range(M)]
        paths = [{0, 1, 2}] + [ring(p, 3) for p in range(1, P)]
    elif comp == "shared":
        types = [(2, 1, 0)[j % 3] for j in range(M)]
        paths = [{0, 1 + p % (M - 1)} for p in range(P)]
    elif comp == "unused":
        types = [(1, 2, 0)[j % 3] for j in range(M)]
        paths = [{0, 2 + p % (M - 2)} for p in range(P)]
    elif comp == "skipactive":
        types = [(1, 0, 1, 2)[j % 4] for j in range(M)]
        paths = [{0, 1, 2 + p % (M - 2)} for p in range(P)]
    else:
        raise ValueError(comp)
    mask = torch.zeros(P, M)
    for p, s in enumerate(paths):
        mask[p, sorted(s)] = 1.0
    return types, mask


def make_case(eng, K, C, rpp, P, M, comp, note=None, seed=None):
    """One layer's parameters in a synthetic ``flat``, its inputs and a backward ReLU mask of the test's own."""
    if seed is None:
        seed = 7919 * K + 131 * C + 17 * rpp + 5 * P + M + 1000003 * COMPS.index(comp)
    g = torch.Generator().manual_seed(seed)
    types, mask = compose(comp, P, M)
    R, chunk = P * rpp, K * C + C + GAP
    W = torch.randn(M, K, C, generator=g) * 0.1
    b = torch.randn(M, C, generator=g) * 0.5
    flat = torch.full((OFF + M * chunk + TAIL,), SENT)
    owned = torch.zeros(flat.numel(), dtype=torch.bool)
    for j in range(M):
        s = OFF + j * chunk
        flat[s:s + K * C] = W[j].reshape(-1)
        flat[s + K * C:s + K * C + C] = b[j]
        owned[s:s + K * C + C] = True
    x = torch.randn(R, K, generator=g) * 0.5
    dy = torch.randn(R, C, generator=g) * 0.1
    relu = (torch.rand(R, M, C, generator=g) < 0.5).to(torch.uint8)
    return dict(eng=eng, K=K, C=C, rpp=rpp, P=P, M=M, R=R, comp=comp, off=OFF, chunk=chunk, types=types, mask=mask,
                W=W, b=b, flat=flat, owned=owned, x=x, dy=dy, relu=relu)


def path_terms(cs, types=None, drop_path=None):
    """Per row: the 0/1 module mask [R][M], its weighted part, nid and nact (float64)."""
    t = torch.tensor(cs["types"] if types is None else types)
    m = cs["mask"].clone()
    if drop_path is not None:
        m[drop_path] = 0.0
    rowmask = m.repeat_interleave(cs["rpp"], 0).double()
    wsel = rowmask * (t != 0).double()[None]
    nid = (rowmask * (t != 1).double()[None]).sum(1)
    return rowmask, wsel, nid, wsel.sum(1)


def ref_forward(cs, W=None, types=None, nid_delta=0):
    """float64 forward from the definition, the expected ReLU mask and the bounds of the module docstring.
    W / types / nid_delta: a deliberately wrong reference (the negative controls)."""
    K, M = cs["K"], cs["M"]
    t = cs["types"] if types is None else types
    x = cs["x"].double()
    W64, b = (cs["W"] if W is None else W).double(), cs["b"].double()
    rowmask, wsel, nid, nact = path_terms(cs, t)
    pre = torch.einsum("rk,mkc->rmc", x, W64) + b[None]
    apre = torch.einsum("rk,mkc->rmc", x.abs(), W64.abs()) + b.abs()[None]
    out = torch.zeros(cs["R"], cs["C"], dtype=torch.float64)
    for j in range(M):
        if not bool(rowmask[:, j].any()):
            continue
        if t[j] == 0:
            o = x
        elif t[j] == 1:
            o = torch.relu(pre[:, j])
        else:
            o = torch.relu(pre[:, j]) + x
        out = out + o * rowmask[:, j:j + 1]
    if nid_delta:
        out = out + nid_delta * x
    n_pre = K + -(-K // TF_KC) + 1
    T = (apre * wsel[:, :, None]).sum(1)
    if bool(nid.any()):
        T = T + nid[:, None] * x.abs()
    active = wsel[:, :, None] > 0
    pre_bound = n_pre * EPS * apre
    return dict(pre=pre, out=out, out_bound=(n_pre + nact + 2)[:, None] * EPS * T, pre_bound=pre_bound,
                relu=((pre > 0) & active).to(torch.uint8), undet=(pre.abs() <= pre_bound) & active)


def masked_grad(cs, wsel):
    return cs["dy"].double()[:, None, :] * cs["relu"].double() * wsel[:, :, None]         # [R][M][C]


def ref_dgrad(cs, W=None, types=None, nid_delta=0):
    """float64 dX of cs["dy"] under cs["relu"], and its bound."""
    W64 = (cs["W"] if W is None else W).double()
    _, wsel, nid, nact = path_terms(cs, types)
    g, dy = masked_grad(cs, wsel), cs["dy"].double()
    dx = torch.einsum("rmc,mkc->rk", g, W64)
    adx = torch.einsum("rmc,mkc->rk", g.abs(), W64.abs())
    if bool(nid.any()) or nid_delta:
        dx = dx + (nid + nid_delta)[:, None] * dy
        adx = adx + nid[:, None] * dy.abs()
    return dx, (nact * cs["C"] + 1)[:, None] * EPS * adx


def ref_wgrad(cs, drop_path=None):
    """float64 dW [M][K][C] and db [M][C] with their bounds; n = the rows that contribute to the module."""
    _, wsel, _, _ = path_terms(cs, drop_path=drop_path)
    g, x = masked_grad(cs, wsel), cs["x"].double()
    rows = wsel.sum(0)                                                                    # [M]
    dW = torch.einsum("rk,rmc->mkc", x, g)
    bW = torch.stack([gemm_bound(x.t(), g[:, m], float(rows[m])) for m in range(cs["M"])])
    return dW, bW, g.sum(0), rows[:, None] * EPS * g.abs().sum(0)


def unpack_grad(cs, gflat):
    """flat gradient -> dW [M][K][C], db [M][C] (copies)."""
    K, C, M, chunk = cs["K"], cs["C"], cs["M"], cs["chunk"]
    body = gflat[cs["off"]:cs["off"] + M * chunk].view(M, chunk)
    return body[:, :K * C].reshape(M, K, C).clone(), body[:, K * C:K * C + C].clone()


# ---------------------------------------------------------------------------------------------------------------
# the comparison code (GPU results and the CPU emulation of tests/test_typed_fc_host.py go through the same)
# ---------------------------------------------------------------------------------------------------------------
def record_ratio(name, value):
    """PATHNET_RECORD_TYPED_FC=<file>: keep the worst measured error / bound per tensor."""
    rec = os.environ.get("PATHNET_RECORD_TYPED_FC")
    if not rec:
        return
    d = {}
    if os.path.exists(rec):
        with open(rec) as f:
            d = json.load(f)
    t = d.setdefault("worst_err_over_bound", {})
    t[name] = max(float(value), float(t.get(name, 0.0)))
    os.makedirs(os.path.dirname(rec) or ".", exist_ok=True)
    with open(rec, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def within(name, got, ref, tol, record=True):
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    r = excess(got, ref, tol)
    worst = float(r.max())
    print(f"{name}: worst err / bound = {worst:.4f}")
    if record:
        record_ratio(name, worst)
    assert worst <= 1.0, (name, worst, int((r > 1).sum()), r.numel())
    return worst


def check_forward(tag, cs, fw, out, relu, record=True):
    """out [R][C] and relu [R][M][C] of a forward against ``fw``; -> the undetermined share of the case."""
    within(f"{tag}.out", out, fw["out"], fw["out_bound"], record)
    relu = relu.cpu()
    assert int(relu.max()) <= 1, f"{tag}: the relu mask holds a byte that is neither 0 nor 1"
    known = ~fw["undet"]
    wrong = int((relu[known] != fw["relu"][known]).sum())
    assert wrong == 0, f"{tag}: {wrong} relu mask bytes differ from pre64 > 0 (or an inactive plane is not zero)"
    share = float(fw["undet"].double().mean())
    assert share < 0.01, (tag, share)
    return share


def check_wgrad(tag, cs, rw, gflat, prefill, record=True):
    """The flat gradient buffer: owned words against float64, everything else still the prefill."""
    gflat = gflat.cpu()
    assert bool((gflat[~cs["owned"]] == prefill).all()), f"{tag}: a gap word or a word outside the layer was written"
    dWr, bW, dbr, bb = rw
    dW, db = unpack_grad(cs, gflat)
    within(f"{tag}.dW", dW, dWr, bW, record)
    within(f"{tag}.db", db, dbr, bb, record)
    _, wsel, _, _ = path_terms(cs)
    for m in range(cs["M"]):
        if float(wsel[:, m].sum()) == 0:               # a skip module or one that no path uses: exact zeros
            assert float(dW[m].abs().max()) == 0.0 and float(db[m].abs().max()) == 0.0, (tag, m)


# ---------------------------------------------------------------------------------------------------------------
# GPU plumbing
# ---------------------------------------------------------------------------------------------------------------
def launcher(kind, eng):
    return f"launch_typed_fc_{kind}" + ("_mfma" if eng == "mfma" else "")


def to_dev(cs):
    relu = torch.full((cs["R"] + PAD, cs["M"], cs["C"]), PREFILL, dtype=torch.uint8)
    relu[:cs["R"]] = cs["relu"]
    return dict(flat=cs["flat"].to(DEV), mask=cs["mask"].contiguous().to(DEV),
                types=torch.tensor(cs["types"], dtype=torch.int32, device=DEV), x=padded(cs["x"]),
                dy=padded(cs["dy"]), relu=relu.to(DEV))


def run_fwd(cs, d, eng, fill=None, relu_fill=PREFILL):
    from pathnet_gym_amd.ops import _lib
    R = cs["R"]
    out = outbuf(R, cs["C"])
    if fill is not None:
        out[:R] = fill
    relu = torch.full((R + PAD, cs["M"], cs["C"]), relu_fill, dtype=torch.uint8, device=DEV)
    relu[R:] = PREFILL
    _lib.call(launcher("fwd", eng), d["x"].data_ptr(), cs["K"], d["flat"].data_ptr(), cs["off"], cs["chunk"],
              cs["C"], cs["M"], d["mask"].data_ptr(), d["types"].data_ptr(), cs["P"], cs["rpp"], out.data_ptr(),
              relu.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert_sentinel(out, R, "out")
    assert bool((relu[R:] == PREFILL).all()), "relu: rows past the end were written"
    return out[:R], relu[:R]


def valu_dgrad_fits(C, M):
    """Whether the VALU input-gradient kernel's dynamic LDS request is inside the limit its launcher reads."""
    from pathnet_gym_amd.ops import _lib
    return M * TF_RT * C * 4 <= _lib.lib().typed_fc_dgrad_lds_limit()


def run_dgrad(cs, d, eng, fill=None):
    """-> (return code, dx [R][K]).  The VALU launcher refuses (-1) a shape whose LDS request does not fit."""
    from pathnet_gym_amd.ops import _lib
    R = cs["R"]
    dx = outbuf(R, cs["K"])
    if fill is not None:
        dx[:R] = fill
    rc = getattr(_lib.lib(), launcher("dgrad", eng))(
        d["dy"].data_ptr(), cs["K"], d["flat"].data_ptr(), cs["off"], cs["chunk"], cs["C"], cs["M"],
        d["mask"].data_ptr(), d["types"].data_ptr(), cs["P"], cs["rpp"], d["relu"].data_ptr(), dx.data_ptr(),
        _lib.stream())
    torch.cuda.synchronize()
    assert_sentinel(dx, R, "dx")
    return rc, dx[:R]


def run_wgrad(cs, d, eng, prefill=SENT):
    from pathnet_gym_amd.ops import _lib
    gflat = torch.full((cs["flat"].numel(),), prefill, device=DEV)
    _lib.call(launcher("wgrad", eng), d["x"].data_ptr(), d["dy"].data_ptr(), cs["K"], cs["off"], cs["chunk"],
              cs["C"], cs["M"], cs["P"], d["mask"].data_ptr(), d["types"].data_ptr(), cs["rpp"],
              d["relu"].data_ptr(), gflat.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    return gflat


def checked_dgrad(tag, cs, d, eng, rd, fill=None, record=True):
    """Run dgrad and hold it to ``rd``; a VALU shape over the LDS limit must be refused with dx untouched.
    -> dx, or None where the launcher refused."""
    rc, dx = run_dgrad(cs, d, eng, fill)
    if eng == "valu" and not valu_dgrad_fits(cs["C"], cs["M"]):
        assert rc == -1, rc
        assert bool((dx == (SENT if fill is None else fill)).all()), "a refused launch wrote dx"
        return None
    assert rc == 0, rc
    within(f"{tag}.dx", dx, rd[0], rd[1], record)
    return dx


# ---------------------------------------------------------------------------------------------------------------
# every launcher at every row of the table
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("row", CASES, ids=case_id)
def test_launchers_match_float64(hip_lib, row):
    """fwd (out, relu mask), dgrad and wgrad of the row's engine: float64 within the derived bounds, the ReLU mask
    exact, sentinels and gap words untouched, and a second run into differently prefilled outputs gives the bits."""
    eng = row[0]
    cs = make_case(*row)
    d = to_dev(cs)
    fw = ref_forward(cs)
    out, relu = run_fwd(cs, d, eng)
    share = check_forward(eng, cs, fw, out, relu)
    record_ratio("fwd.undetermined_share_over_1pct", share / 0.01)
    out2, relu2 = run_fwd(cs, d, eng, fill=11.0, relu_fill=9)
    assert torch.equal(bits(out2), bits(out)) and torch.equal(relu2, relu)
    # backward, under a ReLU mask that no forward made (random planes for the inactive modules too)
    rd = ref_dgrad(cs)
    dx = checked_dgrad(eng, cs, d, eng, rd)
    if dx is not None:
        dx2 = checked_dgrad(eng, cs, d, eng, rd, fill=11.0)
        assert torch.equal(bits(dx2), bits(dx))
    rw = ref_wgrad(cs)
    gflat = run_wgrad(cs, d, eng)
    check_wgrad(eng, cs, rw, gflat, SENT)
    gflat2 = run_wgrad(cs, d, eng, prefill=11.0)
    check_wgrad(eng, cs, rw, gflat2, 11.0)
    owned = cs["owned"].to(DEV)
    assert torch.equal(bits(gflat2[owned]), bits(gflat[owned]))


VALU_BOTH = [r for r in CASES if r[0] == "valu"][::3]


@gpu
@pytest.mark.parametrize("row", VALU_BOTH, ids=case_id)
def test_valu_and_mfma_agree(hip_lib, row):
    """At widths both engines admit: out, dx and the gradients within the sum of the two bounds (the same bound
    twice), and the ReLU masks equal outside the undetermined set."""
    cs = make_case(*row)
    d = to_dev(cs)
    fw, rd, rw = ref_forward(cs), ref_dgrad(cs), ref_wgrad(cs)
    ov, rv = run_fwd(cs, d, "valu")
    om, rm = run_fwd(cs, d, "mfma")
    assert bool(((ov.double() - om.double()).abs().cpu() <= 2 * fw["out_bound"]).all())
    known = ~fw["undet"]
    assert torch.equal(rv.cpu()[known], rm.cpu()[known])
    rcv, dv = run_dgrad(cs, d, "valu")
    rcm, dm = run_dgrad(cs, d, "mfma")
    assert rcm == 0 and rcv == (0 if valu_dgrad_fits(cs["C"], cs["M"]) else -1)
    if rcv == 0:
        assert bool(((dv.double() - dm.double()).abs().cpu() <= 2 * rd[1]).all())
    Wv, bv = unpack_grad(cs, run_wgrad(cs, d, "valu").cpu())
    Wm, bm = unpack_grad(cs, run_wgrad(cs, d, "mfma").cpu())
    assert bool(((Wv.double() - Wm.double()).abs() <= 2 * rw[1]).all())
    assert bool(((bv.double() - bm.double()).abs() <= 2 * rw[3]).all())


# ---------------------------------------------------------------------------------------------------------------
# negative controls: the same comparison, a reference that is wrong in one respect
# ---------------------------------------------------------------------------------------------------------------
def control_references(cs):
    """The wrong references of the negative controls of a ``nid3`` case (path 0 = modules 0 skip, 1 and 2 residual):
    -> {name: (forward reference, dgrad reference)} and the weight gradient with path 0 dropped."""
    assert cs["comp"] == "nid3" and cs["types"][:3] == [0, 2, 2]
    W = cs["W"].clone()
    W[1] *= 1.02
    as_fc = list(cs["types"])
    as_fc[1] = 1
    bad = {"weights of module 1 scaled by 1.02": dict(W=W), "residual module 1 typed as fc": dict(types=as_fc),
           "nid off by one": dict(nid_delta=1)}
    return {k: (ref_forward(cs, **kw), ref_dgrad(cs, **kw)) for k, kw in bad.items()}, ref_wgrad(cs, drop_path=0)


def control_margins(cs, out, dx, dW, db):
    """Worst err / bound of correct results against each wrong reference: all must be over 1."""
    refs, rw = control_references(cs)
    m = {}
    for name, (fw, rd) in refs.items():
        m[f"out | {name}"] = float(excess(out, fw["out"], fw["out_bound"]).max())
        m[f"dx | {name}"] = float(excess(dx, rd[0], rd[1]).max())
    m["dW | path 0 dropped"] = float(excess(dW, rw[0], rw[1]).max())
    m["db | path 0 dropped"] = float(excess(db, rw[2], rw[3]).max())
    return m


CONTROL_ROW = (20, 20, 17, 5, 10, "nid3")


@gpu
@pytest.mark.parametrize("eng", ["valu", "mfma"])
def test_negative_controls_fail_the_bounds(hip_lib, eng):
    cs = make_case(eng, *CONTROL_ROW)
    d = to_dev(cs)
    out, relu = run_fwd(cs, d, eng)
    check_forward(eng, cs, ref_forward(cs), out, relu, record=False)
    rc, dx = run_dgrad(cs, d, eng)
    assert rc == 0
    within("dx", dx, *ref_dgrad(cs), record=False)
    gflat = run_wgrad(cs, d, eng).cpu()
    check_wgrad(eng, cs, ref_wgrad(cs), gflat, SENT, record=False)
    dW, db = unpack_grad(cs, gflat)
    for name, worst in control_margins(cs, out, dx, dW, db).items():
        print(f"{eng} {name}: {worst:.1f}")
        assert worst > 1.0, (name, worst)


# ---------------------------------------------------------------------------------------------------------------
# launcher contract: a bad shape returns its code and launches nothing
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_launchers_reject_bad_arguments(hip_lib):
    from pathnet_gym_amd.ops import _lib
    lib, s = hip_lib, _lib.stream()
    buf = torch.zeros(1 << 20, device=DEV)
    p = buf.data_ptr() + (1 << 21)
    good = dict(K=8, off=3, chunk=77, C=8, M=2, P=1, rpp=4)

    def fwd(name, **kw):
        a = dict(good, **kw)
        return getattr(lib, name)(p, a["K"], p, a["off"], a["chunk"], a["C"], a["M"], p, p, a["P"], a["rpp"], p, p, s)

    def wgrad(name, **kw):
        a = dict(good, **kw)
        return getattr(lib, name)(p, p, a["K"], a["off"], a["chunk"], a["C"], a["M"], a["P"], p, p, a["rpp"], p, p, s)

    calls = [(fwd, launcher("fwd", e)) for e in ("valu", "mfma")] + \
            [(fwd, launcher("dgrad", e)) for e in ("valu", "mfma")] + \
            [(wgrad, launcher("wgrad", e)) for e in ("valu", "mfma")]           # dgrad has fwd's argument order
    for fn, name in calls:
        for key in ("K", "chunk", "C", "M", "P", "rpp"):
            for v in (0, -1):
                assert fn(name, **{key: v}) == -22, (name, key, v)
        assert fn(name, off=-1) == -22, name
        assert fn(name, M=TF_MAXM + 1) == -1, name
        if not name.endswith("_mfma"):
            assert fn(name, C=TF_MAXC + 1) == -1, name
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0            # nothing ran


# ---------------------------------------------------------------------------------------------------------------
# M = 16, C = 64: the VALU input gradient's largest dynamic LDS request (65 536 B beside 72 B of static)
# ---------------------------------------------------------------------------------------------------------------
LDS_ROW = ("valu", 64, 64, 17, 2, 16, "allfc")


@gpu
def test_valu_dgrad_at_its_largest_lds_request(hip_lib):
    """The raw VALU launcher either runs (0, dx correct) or refuses before launching (-1, dx untouched), by the
    limit its host side reads -- never another code."""
    cs = make_case(*LDS_ROW)
    assert cs["M"] == TF_MAXM and cs["C"] == TF_MAXC and float(cs["mask"][0].sum()) == TF_MAXM
    limit = hip_lib.typed_fc_dgrad_lds_limit()
    print("typed_fc_dgrad_lds_limit:", limit)
    assert limit > 0
    d = to_dev(cs)
    rc, dx = run_dgrad(cs, d, "valu")
    assert rc in (0, -1), rc
    assert rc == (0 if valu_dgrad_fits(cs["C"], cs["M"]) else -1)
    if rc == 0:
        within("valu.dx", dx, *ref_dgrad(cs))
    else:
        assert bool((dx == SENT).all()), "a refused launch wrote dx"
    rc, dx = run_dgrad(cs, d, "mfma")
    assert rc == 0
    within("mfma.dx", dx, *ref_dgrad(cs))


@gpu
@pytest.mark.parametrize("mode", ["never", "never-small-lds", "auto", "always"])
def test_op_dgrad_at_m16_c64_whichever_route(hip_lib, mode, monkeypatch):
    """ops/typed_fc.py at M = 16, C = 64: the input gradient is right whether the layer's dgrad runs on the VALU
    kernel or is sent to the MFMA kernel because the LDS request does not fit.  ``never-small-lds`` takes that second
    route on a device whose limit admits the shape: VALU forward and weight gradient, MFMA input gradient over the
    VALU forward's mask."""
    from pathnet_gym_amd.config import LayerSpec, PathNetConfig
    from pathnet_gym_amd.models.pathnet import ParamStore
    from pathnet_gym_amd.ops import typed_fc
    cs = make_case(*LDS_ROW, seed=3)
    K, C, M, P, rpp = cs["K"], cs["C"], cs["M"], cs["P"], cs["rpp"]
    fw = ref_forward(cs)
    assert int(fw["undet"].sum()) == 0              # this seed's forward mask is determined: dx has one right answer
    cs["relu"] = fw["relu"]
    cfg = PathNetConfig(L=1, M=M, N=3, input_shape=(K,), layers=[LayerSpec("fc", C)], trunk_scale="none",
                        num_actions=10)
    st = ParamStore(cfg, torch.device(DEV), seed=1)
    li = st.layout.layer_info[0]
    assert li["offset"] == 0 and li["chunk"] == K * C + C
    packed = torch.cat([cs["W"].reshape(M, -1), cs["b"]], 1).reshape(-1)
    flat = st.flat.detach().clone()
    flat[:packed.numel()] = packed.to(DEV)
    st.flat = flat.requires_grad_(True)
    x = cs["x"].to(DEV).requires_grad_(True)
    assert typed_fc._dgrad_use_mfma(C, M, False) == (not valu_dgrad_fits(C, M))
    assert typed_fc._dgrad_use_mfma(C, M, True)
    calls = []
    real_call = typed_fc._lib.call
    monkeypatch.setattr(typed_fc._lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    small = mode == "never-small-lds"
    if small:
        monkeypatch.setattr(typed_fc, "_dgrad_use_mfma", lambda C, M, mfma: True)
    typed_fc.set_mfma("never" if small else mode)
    try:
        y = typed_fc.typed_trunk_forward(st, x, cs["mask"][:, None, :].to(DEV), rpp)
        (y * cs["dy"].to(DEV)).sum().backward()
    finally:
        typed_fc.set_mfma("auto")
    torch.cuda.synchronize()
    sfx = "_mfma" if mode == "always" else ""
    dsfx = "_mfma" if small or mode == "always" or not valu_dgrad_fits(C, M) else ""
    assert sorted(calls) == sorted([f"launch_typed_fc_fwd{sfx}", f"launch_typed_fc_wgrad{sfx}",
                                    f"launch_typed_fc_dgrad{dsfx}"]), calls
    within(f"op[{mode}].out", y.detach(), fw["out"], fw["out_bound"], record=False)
    within(f"op[{mode}].dx", x.grad, *ref_dgrad(cs), record=False)
    dWr, bW, dbr, bb = ref_wgrad(cs)
    g = st.flat.grad[:packed.numel()].cpu().view(M, K * C + C)
    within(f"op[{mode}].dW", g[:, :K * C].reshape(M, K, C), dWr, bW, record=False)
    within(f"op[{mode}].db", g[:, K * C:], dbr, bb, record=False)
