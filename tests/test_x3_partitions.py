"""csrc/trunk_x3.hip at the work partitions the bench shape takes, on a small shape.

Most fp32x trunk launchers divide their P*T*E units by a target workgroup count, with a floor for small populations.
The other numerics tests of that file run at 3-5 paths x 16/32 envs x T <= 5, where every launcher sits on its
floor: the multi-sample unit walk of a workgroup, its tail, the staged first-valid table of a many-sample workgroup
(``fcs[]``), the env-major map over a long run, the ``MAXB`` segment loop of the band forward, several user paths per
workgroup in the fc weight gradients and their ``nsplit == 1`` store branch are then never run.  Here the setters
(``fast_conv_set_x3_*_target``, ``HipPathNet.fc_wgrad_gm_wgs_small``) force those partitions at 5 paths x 16 envs x
T = 9 (800 samples; T*E = 144 rows per path: two 128-row blocks, three 64-row blocks, 4.5 32-row blocks), episode
ends inside the rollout.  ``masks_with_edges`` gives an empty layer, an all-modules path (several slot groups and
passes) and a one-module layer.

The Python mirrors below restate each launcher's units-per-workgroup formula; ``test_settings_hit_their_regimes_cpu``
asserts that every setting still lands in the regime it is here for, and ``test_defaults_match_the_sources_cpu`` that
the defaults this file restores are the ones the sources start with.

Checks.  (1) Forwards are partition-invariant bit for bit: an output element's sum is formed inside one workgroup in
a fixed order.  (2) So are the conv input gradients and the amax slot they write: one workgroup computes a sample's dX
in slot-group order, the amax is a max.  (3) Weight gradients, per launcher and setting, against the same operation
in float64 on the stored operands (the activations' fp16 pairs upcast, the exact uint8 stacks x in_scale for the
first layer, the stored ReLU bits, the stored output gradient), one path at a time on the GPU, under the two criteria
of tests/test_lstm_x3_kernels.py: (a) elementwise ``|hip - ref| <= x3_bound(X^T, 1, G_masked, g16_scale(gamax), n)``,
n the rows summed, without the pair term of the exact uint8 operand, plus 2^-24 (|X|^T |G|) per workgroup that adds
into the element (deterministic mode: that file's quantisation term); (b) ``||hip - ref|| / ||ref|| < 2e-5`` per module,
weights and biases separately.  The bound is derived and 2e-5 is the mode's class; neither is tuned to the kernel.
(4) The same in the deterministic mode, and repeats are bit-identical.  (5) Negative controls: a unit dropped from,
or counted twice in, the reference, and a 1.02 scale of one module, must fail (b).

The worst err / bound and rel per (launcher, setting) are kept in tests/data/x3_partitions_measured.json (written
when ``PATHNET_RECORD_X3_PARTITIONS=<file>`` is set): a record, not a budget.
"""
import contextlib
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pathnet_gym_amd.config import preset
from test_lstm_kernels import EPS
from test_lstm_x3_kernels import g16_scale, x3_bound
from test_x3_engine import (X3_LAYER_TOL, _oracle_grad, _oracles, check_layers, masks_with_edges, pixel_cfg, rel)

gpu = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P_, E_, T_ = 5, 16, 9
NSAMP = T_ * E_                 # samples per path
NB1W = 20                       # Slab<C1, 2>::NB = ceil(39 / 2): slabs per sample, conv1 weight gradient
NB2W = 3                        # Slab<C2, 7>::NB = ceil(18 / 7)
NB1F = 5                        # BD1<C1>::NB = ceil(39 / 8): bands per sample, conv1 forward
X3_RING_FCS = 1024              # first-valid bytes a ring weight-gradient workgroup stages
X3_C1_FWD_FCS = 128             # ... and a ring band-forward workgroup
C1F_CAP = (X3_C1_FWD_FCS - 2) * NB1F        # x3_conv1_ring_fwd caps bands_per_wg here; the kernel's MAXB

# what the sources start with (test_defaults_match_the_sources_cpu); knobs() restores these
DEFAULTS = dict(wg_auto=1, wg_target=1536, wg2_target=512, wg3_target=256, dg_target=512, dg3_target=512,
                fcw_target=1024, c1f_target=512, c1f_minb=2, c23_target=512, c23_mins=1, c1_emaj=1, dg_bal=1,
                dg_gsplit=2, gm_wgs_small=256)
STATICS = dict(wg_auto="X3_WG_AUTO", wg_target="X3_WG_TARGET", wg2_target="X3_WG2_TARGET", wg3_target="X3_WG3_TARGET",
               dg_target="X3_DG_TARGET", dg3_target="X3_DG3_TARGET", fcw_target="X3_FCW_TARGET",
               c1f_target="X3_C1F_TARGET", c1f_minb="X3_C1F_MINB", c23_target="X3_C23_TARGET", c23_mins="X3_C23_MINS",
               c1_emaj="X3_C1_EMAJ", dg_bal="X3_DG_BAL", dg_gsplit="X3_DG_GSPLIT")


# ---------------------------------------------------------------------------------------------------------------
# the launchers' partition formulas (csrc/trunk_x3.hip, pathnet_gym_amd/ops/pathnet_ops.py), restated
# ---------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def ring_wgrad_upw(P, E, T, wg_target, wg_auto, ncu=256):
    """x3_conv1_ring_wgrad: slabs per workgroup."""
    units = T * E * NB1W
    wgs = wg_target
    if wg_auto and wgs > 0:
        cap = 3 * ncu
        r10 = units * P * 10 // (cap * 133)
        wgs = cap * (1 if r10 <= 15 else (2 if r10 <= 50 else 4))
    upw = cdiv(units * P, wgs) if wgs > 0 else (units + 23) // 24
    return max(upw, 8)


def slab_wgrad_upw(units, P, target):
    """x3_conv_wgrad, the slab lambda (packed conv1: X3_WG_TARGET, conv2: X3_WG2_TARGET)."""
    upw = cdiv(units * P, target) if target > 0 else (units + 23) // 24
    return max(upw, 8)


def tile_wgrad_spw(P, E, T, target):
    """x3_conv_wgrad, the C3 branch: samples per workgroup."""
    return max(cdiv(T * E * P, target), 4)


def dgrad_spw(P, E, T, target):
    """x3_conv_dgrad: samples per workgroup (X3_DG_TARGET for conv2, X3_DG3_TARGET for conv3)."""
    n = T * E
    return max(cdiv(n * P, target) if target > 0 else (n + 31) // 32, 2)


def ring_fwd_bpw(P, E, T, target, minb):
    """x3_conv1_ring_fwd: bands per workgroup."""
    return min(max(cdiv(T * E * NB1F * P, target), minb), C1F_CAP)


def conv23_fwd_spw(P, E, T, target, mins):
    """x3_conv23_fwd: samples per workgroup."""
    return max(cdiv(T * E * P, target), mins)


def packed_fwd_upw(units, P):
    """x3_conv_fwd: bands (C1) or samples (C2, C3) per workgroup; no knob."""
    return max(cdiv(units * P, 512), 2)


def fc2_nsplit(P, fcw_target, K=256, Cout=256, M=10):
    """x3_fc_wgrad: the path split of a module's users."""
    tiles = cdiv(K, 64) * cdiv(Cout, 64) * M
    return min(max(cdiv(fcw_target, tiles), 1), P)


def fc1_nsplit(P, wgs, K=1408, M=10):
    """HipPathNet._layer_bwd_x3 -> x3_fc_wgrad_gm (P <= 16: fc_wgrad_gm_wgs_small)."""
    return max(1, min(P, cdiv(wgs, cdiv(K, 128) * M)))


class S:
    """One setting: the knobs to set, the units per workgroup (or nsplit) they must yield at the fixture shape, and
    the regime it is here for: floor / aligned / straddle (not a multiple of the units per sample) / tail
    (units % units_per_wg != 0) / multi (more than 2 samples per workgroup) / whole (one workgroup per path)."""
    def __init__(self, expect, regime, **knobs):
        self.expect, self.regime, self.knobs = expect, set(regime.split()), knobs
        self.id = "-".join([str(expect)] + [f"{k}{v}" for k, v in knobs.items() if k in ("c1_emaj", "wg_auto", "dg_bal")])


def _emaj(rows):
    return [S(s.expect, " ".join(sorted(s.regime)), **s.knobs, c1_emaj=e) for s in rows for e in (0, 1)]


RING_WGRAD = _emaj([S(8, "floor", wg_auto=0, wg_target=4096),
                    S(120, "aligned multi", wg_auto=0, wg_target=0),
                    S(134, "straddle tail multi", wg_auto=0, wg_target=108),
                    S(267, "straddle tail multi", wg_auto=0, wg_target=54),
                    S(2880, "whole multi", wg_auto=0, wg_target=5)]) + [S(19, "straddle tail", wg_auto=1)]
PACKED_C1_WGRAD = [S(8, "floor", wg_target=4096), S(134, "straddle tail multi", wg_target=108),
                   S(2880, "whole multi", wg_target=5)]
C2_WGRAD = [S(8, "floor straddle", wg2_target=512), S(30, "aligned tail multi", wg2_target=72),
            S(240, "aligned tail multi", wg2_target=9), S(31, "straddle tail multi", wg2_target=70),
            S(432, "whole multi", wg2_target=5)]
C3_WGRAD = [S(4, "floor", wg3_target=256), S(20, "tail multi", wg3_target=36), S(103, "tail multi", wg3_target=7),
            S(144, "whole multi", wg3_target=5)]
DGRAD = [S(spw, reg, dg_target=t, dg3_target=t, dg_bal=bal, dg_gsplit=2)
         for spw, reg, t in ((2, "floor", 512), (10, "tail multi", 72), (80, "tail multi", 9), (144, "whole multi", 5))
         for bal in (1, 0)]
FC2_WGRAD = [S(5, "floor", fcw_target=1024), S(3, "uneven", fcw_target=480), S(2, "uneven", fcw_target=320),
             S(1, "whole", fcw_target=160)]
FC1_WGRAD = [S(3, "uneven", gm_wgs_small=256), S(5, "floor", gm_wgs_small=550), S(2, "uneven", gm_wgs_small=220),
             S(1, "whole", gm_wgs_small=110)]
RING_FWD_STEP = [S(2, "floor", c1f_target=512), S(3, "straddle tail", c1f_target=134),
                 S(20, "aligned multi", c1f_target=20), S(400, "whole multi", c1f_target=1)]
RING_FWD_ALL = [S(3, "straddle tail", c1f_target=1334), S(C1F_CAP, "cap tail multi", c1f_target=1)]
C23_FWD_STEP = [S(1, "floor", c23_target=512), S(3, "tail multi", c23_target=27), S(4, "multi", c23_target=20),
                S(16, "whole multi", c23_target=5)]
C23_FWD_ALL = [S(7, "tail multi", c23_target=115), S(160, "whole multi", c23_target=5)]
# the deterministic mode: the default, a straddling (fc: uneven) setting and the whole path / nsplit 1
DET = {"ring": [S(19, "straddle tail", wg_auto=1), RING_WGRAD[4], RING_WGRAD[8]],
       "packed1": PACKED_C1_WGRAD, "conv2": [C2_WGRAD[0], C2_WGRAD[3], C2_WGRAD[4]],
       "conv3": [C3_WGRAD[0], C3_WGRAD[2], C3_WGRAD[3]], "fc2": [FC2_WGRAD[0], FC2_WGRAD[1], FC2_WGRAD[3]],
       "fc1": [FC1_WGRAD[0], FC1_WGRAD[2], FC1_WGRAD[3]]}

# launcher -> (settings, units per path, units per sample, mirror(knobs merged over DEFAULTS))
TABLES = {
    "ring": (RING_WGRAD, NSAMP * NB1W, NB1W, lambda k: ring_wgrad_upw(P_, E_, T_, k["wg_target"], k["wg_auto"])),
    "packed1": (PACKED_C1_WGRAD, NSAMP * NB1W, NB1W, lambda k: slab_wgrad_upw(NSAMP * NB1W, P_, k["wg_target"])),
    "conv2": (C2_WGRAD, NSAMP * NB2W, NB2W, lambda k: slab_wgrad_upw(NSAMP * NB2W, P_, k["wg2_target"])),
    "conv3": (C3_WGRAD, NSAMP, 1, lambda k: tile_wgrad_spw(P_, E_, T_, k["wg3_target"])),
    "dgrad2": (DGRAD, NSAMP, 1, lambda k: dgrad_spw(P_, E_, T_, k["dg_target"])),
    "dgrad3": (DGRAD, NSAMP, 1, lambda k: dgrad_spw(P_, E_, T_, k["dg3_target"])),
    "ring_fwd_step": (RING_FWD_STEP, E_ * NB1F, NB1F, lambda k: ring_fwd_bpw(P_, E_, 1, k["c1f_target"], k["c1f_minb"])),
    "ring_fwd_all": (RING_FWD_ALL, (T_ + 1) * E_ * NB1F, NB1F,
                     lambda k: ring_fwd_bpw(P_, E_, T_ + 1, k["c1f_target"], k["c1f_minb"])),
    "c23_step": (C23_FWD_STEP, E_, 1, lambda k: conv23_fwd_spw(P_, E_, 1, k["c23_target"], k["c23_mins"])),
    "c23_all": (C23_FWD_ALL, (T_ + 1) * E_, 1, lambda k: conv23_fwd_spw(P_, E_, T_ + 1, k["c23_target"], k["c23_mins"])),
}


def _huge_targets(knobs):
    """The same knobs with every workgroup target a setting names made huge: the floor is what is left."""
    return {k: 1 << 20 for k in knobs if k.endswith("_target") or k == "gm_wgs_small"}


def test_defaults_match_the_sources_cpu():
    """DEFAULTS (what knobs() restores) are the values csrc/trunk_x3.hip and ops/pathnet_ops.py start with."""
    with open(os.path.join(ROOT, "csrc", "trunk_x3.hip")) as f:
        src = f.read()
    for k, name in STATICS.items():
        m = re.search(r"static int %s = (\w+);" % name, src)
        assert m, name
        v = m.group(1)
        if not v.isdigit():
            v = re.search(r"#define %s (\d+)" % v, src).group(1)
        assert int(v) == DEFAULTS[k], (name, v)
    for name, v in (("X3_RING_FCS", X3_RING_FCS), ("X3_C1_FWD_FCS", X3_C1_FWD_FCS)):
        assert int(re.search(r"#define %s (\d+)" % name, src).group(1)) == v
    with open(os.path.join(ROOT, "pathnet_gym_amd", "ops", "pathnet_ops.py")) as f:
        py = f.read()
    assert int(re.search(r'"PATHNET_X3_FC_WGRAD_WGS_SMALL", "(\d+)"', py).group(1)) == DEFAULTS["gm_wgs_small"]


def test_settings_hit_their_regimes_cpu():
    """Every setting, at the fixture shape and on 256 CUs, yields the units per workgroup it names and sits in the
    regime it is here for, so a change of defaults or of a launcher formula cannot quietly turn these cases back
    into the floor case."""
    for name, (table, units, per, mirror) in TABLES.items():
        for s in table:
            upw = mirror({**DEFAULTS, **s.knobs})
            assert upw == s.expect, (name, s.id, upw)
            r = s.regime
            if "floor" in r:
                assert mirror({**DEFAULTS, **s.knobs, **_huge_targets(s.knobs)}) == upw, (name, s.id)
            if "straddle" in r:
                assert upw % per != 0, (name, s.id)
            if "aligned" in r:
                assert upw % per == 0, (name, s.id)
            if "tail" in r:
                assert units % upw != 0, (name, s.id)
            if "multi" in r:
                assert upw > 2 * per, (name, s.id)
            if "whole" in r:
                assert upw >= units, (name, s.id)
            if "cap" in r:
                # the launcher's cap applies (what the balanced schedule makes of it: test_band_forward_schedules_cpu)
                assert upw == C1F_CAP < units, (name, s.id)
            if name == "ring":
                # the launcher answers -22 past this: the workgroup's first-valid bytes must fit its LDS table
                assert upw // NB1W + 2 <= X3_RING_FCS and cdiv(upw, NB1W) <= X3_RING_FCS - 2, (name, s.id)
            if name.startswith("ring_fwd"):
                assert cdiv(upw, NB1F) + 1 <= X3_C1_FWD_FCS, (name, s.id)
    assert RING_WGRAD[8].expect // NB1W + 2 == 146          # one workgroup per path: 146 staged first-valid bytes
    for s in FC2_WGRAD:
        assert fc2_nsplit(P_, s.knobs["fcw_target"]) == s.expect, s.id
    for s in FC1_WGRAD:
        assert fc1_nsplit(P_, s.knobs["gm_wgs_small"]) == s.expect, s.id
    assert fc2_nsplit(P_, DEFAULTS["fcw_target"]) == 5 and fc1_nsplit(P_, DEFAULTS["gm_wgs_small"]) == 3
    # uneven: 5 users do not divide over the split; whole: the store branch
    assert all(5 % s.expect for s in FC2_WGRAD + FC1_WGRAD if "uneven" in s.regime)
    # the packed forward has no knob: 3 bands per workgroup straddle the 5-band sample at T = 3; 3 samples, tail 1, at 13
    assert packed_fwd_upw(3 * E_ * NB1F, P_) == 3 and 3 % NB1F != 0
    assert packed_fwd_upw(13 * E_, P_) == 3 and (13 * E_) % 3 == 1
    # the bench shape (P = 64 / 32 / 16 / 8, E = 32, T = 20) on 256 CUs, as the settings above were chosen from
    assert [ring_wgrad_upw(p, 32, 20, 1536, 1) for p in (64, 32, 16, 8)] == [267, 267, 134, 134]
    assert [slab_wgrad_upw(20 * 32 * NB2W, p, 512) for p in (64, 32, 16, 8)] == [240, 120, 60, 30]
    assert [tile_wgrad_spw(p, 32, 20, 256) for p in (64, 32, 16, 8)] == [160, 80, 40, 20]
    assert [dgrad_spw(p, 32, 20, 512) for p in (64, 32, 16, 8)] == [80, 40, 20, 10]
    assert [ring_fwd_bpw(p, 32, 1, 512, 2) for p in (64, 32, 16, 8)] == [20, 10, 5, 3]
    assert [conv23_fwd_spw(p, 32, 1, 512, 1) for p in (64, 32, 16, 8)] == [4, 2, 1, 1]
    assert fc2_nsplit(64, 1024) == 7 and fc1_nsplit(64, 768) == 7 and fc1_nsplit(16, 256) == 3


def c1_npass(cnt):
    """csrc/trunk_x3.hip c1_npass: what a band of a path with cnt active first-layer modules costs."""
    nct = (cnt + 1) >> 1
    return (nct + 1) // 2 if nct > 2 else 1


def bal_runs(costs, n, grid):
    """csrc/trunk_x3.hip bal_schedule: workgroup b of ``grid`` takes the b-th equal share of the total cost of P paths
    x n units (a unit of path p costing costs[p]), rounded down to unit boundaries.  -> per workgroup, the (path,
    first unit, end unit) runs it walks."""
    incl = np.cumsum([c * n for c in costs])
    U = int(incl[-1])

    def at(c):
        if c >= U:
            return len(costs) - 1, n
        p = int(np.searchsorted(incl, c, side="right"))
        return p, (c - (int(incl[p]) - costs[p] * n)) // costs[p]

    out = []
    for b in range(grid):
        (p0, u0), (p1, u1) = at(U * b // grid), at(U * (b + 1) // grid)
        out.append([(p, u0 if p == p0 else 0, u1 if p == p1 else n) for p in range(p0, p1 + 1)])
    return out


def maxb_masks():
    """Four all-modules paths (3 passes per band) behind one single-module path: the balanced schedule's equal shares
    of the cost then give the cheap path's whole run of bands to one workgroup."""
    cfg = pixel_cfg()
    m = masks_with_edges(P_, cfg.L, cfg.M, cfg.N, seed=6)
    m[:, 0, :] = 1
    m[0, 0, :] = 0
    m[0, 0, 3] = 1
    return m


def test_band_forward_schedules_cpu():
    """What the balanced schedule of the ring band forward does with one launch of all T + 1 steps (800 bands per
    path) under the launcher's cap of 630 bands.  With the fixture's paths (costs 1, 3, 1, 1, 1) the ten workgroups'
    shares are 560 cost units, so no run of bands within one path exceeds the kernel's MAXB = 630 and the segment loop
    takes no second segment there; with maxb_masks() (costs 1, 3, 3, 3, 3) a workgroup walks all 800 bands of the
    cheap path, in two segments.  The tiling is checked too: the runs cover every (path, band) once."""
    cfg = pixel_cfg()
    n = (T_ + 1) * E_ * NB1F
    grid = cdiv(n, C1F_CAP) * P_
    longest = {}
    for name, m in (("fixture", masks_with_edges(P_, cfg.L, cfg.M, cfg.N, seed=2)), ("maxb", maxb_masks())):
        costs = [c1_npass(int(m[p, 0].sum())) for p in range(P_)]
        runs = bal_runs(costs, n, grid)
        seen = np.zeros((P_, n), dtype=int)
        for wg in runs:
            for p, u0, u1 in wg:
                seen[p, u0:u1] += 1
        assert (seen == 1).all(), name
        longest[name] = max(u1 - u0 for wg in runs for _, u0, u1 in wg)
    assert longest["fixture"] <= C1F_CAP < longest["maxb"] == n, longest


def pair_bound(A, Bm, sb, n, exact_a):
    """Criterion (a) of X^T G from the row-major operands A [n, k] (scale 1) and Bm [n, q] (scale sb): x3_bound(A^T, 1,
    Bm, sb, n)[1], with the A side's |.| and d(.) hoisted out (a path's slots share A); exact_a: A is exact in fp16
    (the uint8 first layer), so its pair term d(A) is dropped.  -> (bound, |A|^T |Bm|)"""
    absA, absB = A.double().abs(), Bm.double().abs()
    dB = 2.0 ** -22 * absB + 2.0 ** -25 / sb
    AB = absA.t() @ absB
    if exact_a:
        pair_part = absA.t() @ dB
    else:
        dA = 2.0 ** -22 * absA + 2.0 ** -25
        pair_part = dA.t() @ absB + (absA + dA).t() @ dB + 2.0 ** -22 * AB
    return pair_part + 3 * n * EPS * AB, AB


def test_pair_bound_is_x3_bound_cpu():
    g = torch.Generator().manual_seed(3)
    A, Bm = torch.randn(37, 12, generator=g), torch.randn(37, 9, generator=g) * 1e-3
    sb = g16_scale(float(Bm.abs().max()))
    got, AB = pair_bound(A, Bm, sb, 37, False)
    assert torch.allclose(got, x3_bound(A.t(), 1.0, Bm, sb, 37)[1], rtol=1e-12, atol=0)
    assert torch.allclose(AB, A.double().abs().t() @ Bm.double().abs(), rtol=1e-12, atol=0)
    exact, _ = pair_bound(A, Bm, sb, 37, True)
    assert bool((exact < got).all())


# ---------------------------------------------------------------------------------------------------------------
# GPU plumbing
# ---------------------------------------------------------------------------------------------------------------
def record(kind, name, value):
    """PATHNET_RECORD_X3_PARTITIONS=<file>: keep the worst measured figure per (launcher, setting)."""
    rec = os.environ.get("PATHNET_RECORD_X3_PARTITIONS")
    if not rec:
        return
    d = {}
    if os.path.exists(rec):
        with open(rec) as f:
            d = json.load(f)
    t = d.setdefault(kind, {})
    t[name] = max(float(value), float(t.get(name, 0.0)))
    os.makedirs(os.path.dirname(rec) or ".", exist_ok=True)
    with open(rec, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def _set(hp, key, v):
    from pathnet_gym_amd.ops import _lib
    if key == "gm_wgs_small":
        hp.fc_wgrad_gm_wgs_small = v
    else:
        getattr(_lib.lib(), "fast_conv_set_x3_" + key)(v)


@contextlib.contextmanager
def knobs(hp, **kw):
    """Set partition knobs; the committed defaults come back whatever happens inside."""
    try:
        for k, v in kw.items():
            _set(hp, k, v)
        yield
    finally:
        for k in kw:
            _set(hp, k, DEFAULTS[k])


class Ctx:
    """One stored rollout + backward at the fixture shape, and what the tests share: the engine's operands (left as
    they are), its gradient, the amaxes its backward left, and the float64 truths of the weight gradients (computed
    on first use, one per layer)."""

    def __init__(self, deterministic, oracle):
        from pathnet_gym_amd.algo.trainer import PathNetTrainer
        cfg = preset("pong")
        cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = P_, E_, T_
        cfg.use_graph = False
        cfg.compute_dtype = "fp32x"
        cfg.frame_ring = True
        cfg.deterministic = deterministic
        tr = PathNetTrainer(cfg, device=DEV)
        eng = tr.engine
        assert tr.compute_dtype == "fp32x" and eng.ring and tr.model.hip.fx_det == deterministic
        tr.env.max_episode_steps = 5
        tr.update()
        tr.model.set_paths(masks_with_edges(P_, cfg.net.L, cfg.net.M, cfg.net.N, seed=2))
        eng._rollout_backward_body()
        torch.cuda.synchronize()
        assert eng.dones.any() and (eng.T, eng.E, eng.P, eng.B) == (T_, E_, P_, P_ * E_)
        self.tr, self.eng, self.hp, self.det = tr, eng, tr.model.hip, deterministic
        hp = self.hp
        self.L, self.M = hp.L, hp.M
        self.gamax = hp.gamax.clone()
        self.g_hip = eng.grad_flat.clone()
        self.rbase = eng.rbase
        self.stacks = eng.obs_stacks(T_ + 1).contiguous()
        self.cnt = tr.model.act_cnt.view(P_, self.L).cpu().numpy()
        self.idx = tr.model.act_idx.view(P_, self.L, self.M).cpu().numpy()
        self.users = [[sum(int(j in self.idx[p, l, :self.cnt[p, l]]) for p in range(P_)) for j in range(self.M)]
                      for l in range(self.L)]
        self.oracles = None
        if oracle:
            # (float64 truth, plain fp32 oracle) of the whole chain.  The fp32 one on torch's own im2col + GEMM
            # convolution, as the float64 one always is: the library convolution spends ~10 s choosing kernels for a
            # batch size it has not seen, and either is plain fp32
            with torch.backends.cudnn.flags(enabled=False):
                self.oracles = _oracles(_oracle_grad, tr, eng)
        self.ncu = torch.cuda.get_device_properties(0).multi_processor_count
        self._vals, self._truth, self._fwd = {}, {}, None
        hp.check_x3_status()

    # -- operands ------------------------------------------------------------------------------------------------
    def value(self, l):
        """fp32 value of the stored fp16-pair activations of layer l, [T + 1, B, features]."""
        from pathnet_gym_amd.ops.pathnet_ops import x2_value
        if l not in self._vals:
            self._vals[l] = x2_value(self.eng.acts[l])
        return self._vals[l]

    def operand(self, l, p):
        """float64 X of layer l's weight gradient for path p, steps 0..T-1: [n, K], rows in (step, env, position)
        order, k = (kh, kw, ci) -- the im2col matrix of a conv layer, the activation rows of an fc layer."""
        g = self.hp.geoms[l]
        rows = slice(p * E_, (p + 1) * E_)
        if l == 0:
            x = self.stacks[:T_, rows].double() * float(np.float32(g.in_scale))      # exact pixels x the fp32 scale
        else:
            x = self.value(l - 1)[:T_, rows].double()
        if g.kind == "fc":
            return x.reshape(NSAMP, g.K)
        x = x.reshape(NSAMP, g.Hin, g.Win, g.Cin).permute(0, 3, 1, 2)
        cols = F.unfold(x, (g.KH, g.KW), stride=g.S)                                 # [N, (ci, kh, kw), positions]
        return cols.view(NSAMP, g.Cin, g.KH, g.KW, g.HWo).permute(0, 4, 2, 3, 1).reshape(NSAMP * g.HWo, g.K)

    def masked_g(self, l, p, a):
        """float64 output gradient of path p, x the scale layer_bwd passes (fp32, as the kernel multiplies), where
        slot a's stored ReLU bit is set, else 0: [n, Cout]."""
        eng, g = self.eng, self.hp.geoms[l]
        rows = slice(p * E_, (p + 1) * E_)
        G = eng.grads[l].view(T_, P_ * E_, -1)[:, rows]
        if l == self.L - 1:
            G = G * torch.tensor(self.hp.out_scale_last, dtype=torch.float32, device=DEV)
        if g.kind == "conv":
            b = eng.bits[l][a].view(T_ + 1, P_ * E_, g.HWo)[:T_, rows].reshape(-1).to(torch.int32)
            on = ((b[:, None] >> torch.arange(8, device=DEV)) & 1).bool()
        else:
            w = eng.bits[l][a].view(T_ + 1, P_ * E_, g.Cout // 16)[:T_, rows].reshape(NSAMP, -1).to(torch.int32) & 0xFFFF
            on = ((w[:, :, None] >> torch.arange(16, device=DEV)) & 1).bool().reshape(NSAMP, g.Cout)
        G = G.reshape(-1, g.Cout).double()
        return torch.where(on, G, torch.zeros_like(G))

    def slots(self, l, p):
        """(slot, module) pairs of path p in layer l."""
        return [(a, int(self.idx[p, l, a])) for a in range(int(self.cnt[p, l]))]

    def truth(self, l):
        """Per module j of layer l, summed over the (path, slot) pairs that use it: float64 dW [K, Cout] and db
        [Cout], their criterion-(a) bounds without the adds, and |X|^T |G|, sum |G| for the adds."""
        if l in self._truth:
            return self._truth[l]
        g = self.hp.geoms[l]
        z = lambda *s: torch.zeros(self.M, *s, dtype=torch.float64, device=DEV)       # noqa: E731
        t = dict(dW=z(g.K, g.Cout), bW=z(g.K, g.Cout), absW=z(g.K, g.Cout), db=z(g.Cout), bb=z(g.Cout), absb=z(g.Cout))
        sb = g16_scale(float(self.gamax[l]))
        for p in range(P_):
            if not self.cnt[p, l]:
                continue
            A = self.operand(l, p)
            n = A.shape[0]
            for a, j in self.slots(l, p):
                Gm = self.masked_g(l, p, a)
                bound, AB = pair_bound(A, Gm, sb, n, exact_a=(l == 0))
                t["dW"][j] += A.t() @ Gm
                t["bW"][j] += bound
                t["absW"][j] += AB
                absg = Gm.abs().sum(0)
                t["db"][j] += Gm.sum(0)
                # the bias sums the fp32 gradient (or, fc1, its fp16 pair read back: d(G)) in fp32, n terms
                t["bb"][j] += n * EPS * absg + 2.0 ** -22 * absg + n * 2.0 ** -25 / sb
                t["absb"][j] += absg
            del A
        self._truth[l] = t
        return t

    # -- launches ------------------------------------------------------------------------------------------------
    def zero_grad(self):
        return torch.zeros_like(self.eng.grad_flat)

    def wgrad(self, launcher, grad):
        """One weight-gradient launcher into ``grad`` (zeroed by the caller: the nsplit == 1 fc kernels store), after
        the part="d" call that fills Gm (fc) -- with the amaxes of the stored backward in place."""
        eng, hp = self.eng, self.hp
        l = {"ring": 0, "packed1": 0, "conv2": 1, "conv3": 2, "fc1": 3, "fc2": 4}[launcher]
        scratch = None
        if hp.geoms[l].kind == "fc":
            scratch = torch.empty_like(eng.grads[l - 1])
            hp.layer_bwd(l, eng.acts[l - 1], eng.grads[l], eng.bits[l], grad, scratch, P_, E_, T_, eng.bits_rows[l],
                         part="d")                         # (the last layer's resets every amax slot)
        hp.gamax.copy_(self.gamax)
        hp.fx_begin()
        try:
            if launcher == "ring":
                hp.ring_wgrad(eng.frames, eng.fc, eng.grads[0], eng.bits[0], grad, P_, E_, T_, eng.bits_rows[0],
                              rbase=self.rbase)
            else:
                X = self.stacks[:T_] if l == 0 else eng.acts[l - 1]
                hp.layer_bwd(l, X, eng.grads[l], eng.bits[l], grad, scratch, P_, E_, T_, eng.bits_rows[l], part="w")
        finally:
            hp.fx_end(grad)
        torch.cuda.synchronize()
        if self.det:
            assert int(hp._fxbuf.abs().sum()) == 0
        return l

    def adds(self, launcher, s):
        """Per module: how many workgroups add into an element of its gradient under setting s."""
        l = {"ring": 0, "packed1": 0, "conv2": 1, "conv3": 2, "fc1": 3, "fc2": 4}[launcher]
        if launcher in ("fc1", "fc2"):
            return [min(s.expect, u) for u in self.users[l]]
        _, units, _, mirror = TABLES[launcher]
        k = {**DEFAULTS, **s.knobs}
        upw = ring_wgrad_upw(P_, E_, T_, k["wg_target"], k["wg_auto"], self.ncu) if launcher == "ring" else mirror(k)
        return [u * cdiv(units, upw) for u in self.users[l]]

    def check_wgrad(self, name, l, grad, adds, scale_control=False):
        """Criteria (a) and (b) per module, weights and biases; exact zeros outside the layer's range and in every
        module nobody uses.  -> {module: (hip dW, hip db)}"""
        g, t = self.hp.geoms[l], self.truth(l)
        assert bool(torch.isfinite(grad).all()), name
        expect_nz = torch.zeros_like(grad, dtype=torch.bool)
        worst_a = worst_b = 0.0
        out, rels = {}, {}
        for j in range(self.M):
            if not self.users[l][j]:
                continue
            w0, b0 = g.w_off + j * g.chunk, g.b_off + j * g.chunk
            expect_nz[w0:w0 + g.K * g.Cout] = True
            expect_nz[b0:b0 + g.Cout] = True
            w = grad[w0:w0 + g.K * g.Cout].view(g.K, g.Cout).double()
            b = grad[b0:b0 + g.Cout].double()
            if self.det:       # every contribution quantised to 2^-34 once (a bias partial: <= 512 threads of a
                               # workgroup), the flush converts (one rounding) and adds once
                f, qw, qb = 2 * 2.0 ** -24 * 1.001, adds[j] * 2.0 ** -35, adds[j] * 512 * 2.0 ** -35
            else:              # one atomic add per workgroup
                f, qw, qb = adds[j] * 2.0 ** -24 * 1.001, 0.0, 0.0
            tolw = t["bW"][j] + f * t["absW"][j] + qw
            tolb = t["bb"][j] + f * t["absb"][j] + qb
            worst_a = max(worst_a, float(((w - t["dW"][j]).abs() / tolw.clamp_min(1e-300)).max()),
                          float(((b - t["db"][j]).abs() / tolb.clamp_min(1e-300)).max()))
            assert float(t["dW"][j].norm()) > 0 and float(t["db"][j].norm()) > 0, (name, j)
            rels[j] = (rel(w, t["dW"][j]), rel(b, t["db"][j]))
            worst_b = max(worst_b, *rels[j])
            if scale_control:
                assert rel(w, 1.02 * t["dW"][j]) > X3_LAYER_TOL and rel(b, 1.02 * t["db"][j]) > X3_LAYER_TOL, (name, j)
            out[j] = (w, b)
        print(f"{name}: worst err / bound = {worst_a:.4f}, worst rel = {worst_b:.3e}")
        record("worst_err_over_bound", name, worst_a)
        record("worst_rel", name, worst_b)
        assert worst_a <= 1.0, (name, worst_a)
        assert worst_b < X3_LAYER_TOL, (name, {j: (f"{ew:.2e}", f"{eb:.2e}") for j, (ew, eb) in rels.items()})
        assert int(grad[~expect_nz].count_nonzero()) == 0, f"{name}: non-zero outside the modules in use"
        return out

    def run_wgrad(self, launcher, s, tag="", scale_control=False):
        grad = self.zero_grad()
        with knobs(self.hp, **s.knobs):
            l = self.wgrad(launcher, grad)
        name = f"{launcher}{tag}.{s.id}"
        return grad, self.check_wgrad(name, l, grad, self.adds(launcher, s), scale_control)

    # -- forwards ------------------------------------------------------------------------------------------------
    def alloc_fwd(self, layers):
        hp = self.hp
        out = {}
        for l in layers:
            b, rows = hp.alloc_bits(l, T_ + 1, P_ * E_)
            out[l] = (hp.alloc_act(l, (T_ + 1, P_ * E_, hp.geoms[l].out_feat)), b, rows)
        return out

    def ring_fwd(self, buf, T, t0):
        eng = self.eng
        Y, b, rows = buf[0]
        self.hp.ring_fwd(eng.frames, eng.fc, Y, b, P_, E_, T, t0, rows, rbase=self.rbase)

    def c23_fwd(self, X0, buf, T, t0):
        (Y1, b1, r1), (Y2, b2, r2) = buf[1], buf[2]
        assert self.hp.conv23_fwd(1, X0, Y1, b1, r1, Y2, b2, r2, P_, E_, T, t0)

    def fwd_ref(self):
        """conv1 (ring) and the fused conv2 + conv3 forward at the default partition, launched one step at a time."""
        if self._fwd is None:
            buf = self.alloc_fwd((0, 1, 2))
            for t in range(T_ + 1):
                self.ring_fwd(buf, 1, t)
                self.c23_fwd(buf[0][0], buf, 1, t)
            torch.cuda.synchronize()
            self._fwd = buf
        return self._fwd

    def assert_fwd_equal(self, l, got, ref, steps):
        """Both fp16 planes and their value bit for bit on ``steps``; ReLU bits of the slots below each path's active
        count (the rest is never written)."""
        from pathnet_gym_amd.ops.pathnet_ops import _plane, x2_value
        (Y, b, _), (Yr, br, _) = got, ref
        hw = self.hp.geoms[l].HWo
        B = P_ * E_
        for t in steps:
            assert torch.equal(Y[t], Yr[t]), (l, t, "hi")
            assert torch.equal(_plane(Y, 1, torch.float16)[t], _plane(Yr, 1, torch.float16)[t]), (l, t, "lo")
            assert torch.equal(x2_value(Y[t]), x2_value(Yr[t])), (l, t)
            for p in range(P_):
                k = int(self.cnt[p, l])
                r0 = (t * B + p * E_) * hw
                assert torch.equal(b[:k, r0:r0 + E_ * hw], br[:k, r0:r0 + E_ * hw]), (l, t, p)
        assert float(Y[list(steps)].float().abs().sum()) > 0


@pytest.fixture(scope="module")
def part(hip_lib):
    return Ctx(deterministic=False, oracle=True)


@pytest.fixture(scope="module")
def part_det(hip_lib):
    return Ctx(deterministic=True, oracle=False)


def ids(table):
    return [s.id for s in table]


# ---------------------------------------------------------------------------------------------------------------
# the engine at this shape
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_engine_gradient_at_the_partition_shape(part):
    """At defaults the engine's whole gradient passes the per-layer budget against the float64 and fp32 autograd
    oracles at this shape too: T*E = 144 puts two 128-row blocks (the second a 16-row tail) in fc_dgrad_gemm_x3 and
    4.5 32-row blocks in the fc weight gradients."""
    g64, g32 = part.oracles
    check_layers("fp32x frame-ring engine, 5 x 16 x 9", part.tr, part.g_hip, g64, g32)


# ---------------------------------------------------------------------------------------------------------------
# (1) forwards: bit-identical under every partition
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_forward_default_partition_is_the_engines(part):
    ref = part.fwd_ref()
    for l in (0, 1, 2):
        part.assert_fwd_equal(l, (part.eng.acts[l], part.eng.bits[l], 0), ref[l], range(T_ + 1))


@gpu
@pytest.mark.parametrize("s", RING_FWD_STEP, ids=ids(RING_FWD_STEP))
def test_ring_forward_one_step_partitions_bit_equal(part, s):
    """conv1_fwd_band_x2 on the ring, one step (steps 0 and T), at 2 / 3 (straddling, tail) / 20 / 400 (one workgroup's
    share spans every path) bands per workgroup == the default partition."""
    ref = part.fwd_ref()
    buf = part.alloc_fwd((0,))
    with knobs(part.hp, **s.knobs):
        for t in (0, T_):
            part.ring_fwd(buf, 1, t)
    torch.cuda.synchronize()
    part.assert_fwd_equal(0, buf[0], ref[0], (0, T_))


@gpu
@pytest.mark.parametrize("s", RING_FWD_ALL, ids=ids(RING_FWD_ALL))
def test_ring_forward_all_steps_partitions_bit_equal(part, s):
    """One launch of all T + 1 steps: 3 bands per workgroup, and a target of 1, where the launcher's cap of 630 bands
    applies (ten workgroups whose shares of 560 cost units span paths; the MAXB segment loop's second segment needs
    the paths of test_ring_forward_maxb_second_segment_bit_equal)."""
    ref = part.fwd_ref()
    buf = part.alloc_fwd((0,))
    with knobs(part.hp, **s.knobs):
        part.ring_fwd(buf, T_ + 1, 0)
    torch.cuda.synchronize()
    part.assert_fwd_equal(0, buf[0], ref[0], range(T_ + 1))


@gpu
def test_ring_forward_maxb_second_segment_bit_equal(hip_lib):
    """The MAXB segment loop of conv1_fwd_band_x2: one launch of 10 steps under a workgroup target of 1 with
    maxb_masks() (test_band_forward_schedules_cpu: one workgroup walks the cheap path's 800 bands, 630 + 170, restaging
    the first-valid bytes for the second segment) == the default partition one step at a time, on a synthetic modular
    ring (random frames, first-valid channels 0..3, base slot 9 of 18: the slots wrap)."""
    from pathnet_gym_amd.models.acnet import ACPathNet
    from pathnet_gym_amd.ops.pathnet_ops import _plane
    cfg = pixel_cfg()
    m = ACPathNet(cfg, P_, DEV, "hip", seed=11, compute_dtype="fp32x")
    masks = maxb_masks()
    m.set_paths(masks)
    hp = m.hip
    hp.enable_ring()
    B, steps, nslots, rbase = P_ * E_, T_ + 1, 2 * T_, T_
    gen = torch.Generator(device="cpu").manual_seed(9)
    frames = torch.randint(0, 256, (B, nslots, 160 * 120), generator=gen, dtype=torch.uint8).to(DEV)
    fc = torch.randint(0, 4, (steps, B), generator=gen, dtype=torch.uint8).to(DEV)
    outs = []
    for at_once in (False, True):
        Y = hp.alloc_act(0, (steps, B, hp.geoms[0].out_feat))
        b, rows = hp.alloc_bits(0, steps, B)
        if at_once:
            with knobs(hp, c1f_target=1):
                hp.ring_fwd(frames, fc, Y, b, P_, E_, steps, 0, rows, rbase=rbase)
        else:
            for t in range(steps):
                hp.ring_fwd(frames, fc, Y, b, P_, E_, 1, t, rows, rbase=rbase)
        torch.cuda.synchronize()
        outs.append((Y, b))
    (Ya, ba), (Yb, bb) = outs
    assert float(Ya.float().abs().sum()) > 0
    assert torch.equal(Ya, Yb) and torch.equal(_plane(Ya, 1, torch.float16), _plane(Yb, 1, torch.float16))
    hw = hp.geoms[0].HWo
    for p in range(P_):
        k = int(masks[p, 0].sum())
        for t in range(steps):
            r0 = (t * B + p * E_) * hw
            assert torch.equal(ba[:k, r0:r0 + E_ * hw], bb[:k, r0:r0 + E_ * hw]), (p, t)
    hp.check_x3_status()


@gpu
@pytest.mark.parametrize("s", C23_FWD_STEP + C23_FWD_ALL, ids=ids(C23_FWD_STEP) + ["all-" + i for i in ids(C23_FWD_ALL)])
def test_fused_conv23_forward_partitions_bit_equal(part, s):
    """conv23_fwd_tile_x3 at 1 / 3 (tail) / 4 / 16 samples per workgroup for one step (steps 0 and T), 7 and 160 for
    one launch of all T + 1 steps == the default partition one step at a time."""
    ref = part.fwd_ref()
    buf = part.alloc_fwd((1, 2))
    steps = range(T_ + 1) if s in C23_FWD_ALL else (0, T_)
    with knobs(part.hp, **s.knobs):
        if s in C23_FWD_ALL:
            part.c23_fwd(ref[0][0], buf, T_ + 1, 0)
        else:
            for t in steps:
                part.c23_fwd(ref[0][0], buf, 1, t)
    torch.cuda.synchronize()
    for l in (1, 2):
        part.assert_fwd_equal(l, buf[l], ref[l], steps)


@gpu
def test_forward_forced_partition_matches_plain_fp32_oracle(part):
    """The anchor of the bit-equality tests: the trunk forward with 20 bands and 4 samples per workgroup (the 64-path
    bench partition) meets the plain fp32 oracle per path, as test_x3_trunk_forward_matches_plain_fp32_oracle does at
    its own shape."""
    from pathnet_gym_amd.models.pathnet import trunk_forward_ref
    hp, tr = part.hp, part.tr
    B = P_ * E_
    buf = part.alloc_fwd(range(part.L))
    with knobs(hp, c1f_target=20, c23_target=20):
        assert ring_fwd_bpw(P_, E_, 1, 20, 2) == 20 and conv23_fwd_spw(P_, E_, 1, 20, 1) == 4
        for t in range(T_ + 1):
            part.ring_fwd(buf, 1, t)
            part.c23_fwd(buf[0][0], buf, 1, t)
            for l in range(3, part.L):
                hp.layer_fwd(l, buf[l - 1][0], buf[l][0], buf[l][1], P_, E_, 1, t, buf[l][2])
    torch.cuda.synchronize()
    feat = buf[part.L - 1][0].view(T_ + 1, P_, E_, -1)
    with torch.no_grad():
        x = part.stacks.reshape((T_ + 1) * B, 160, 120, 4).float() / 255.0
        ref = trunk_forward_ref(tr.model.store, x, tr.model.mask.repeat_interleave(E_, 0).repeat(T_ + 1, 1, 1))
    ref = ref.view(T_ + 1, P_, E_, -1)
    errs = []
    for p in range(P_):
        if ref[:, p].norm() == 0:
            assert feat[:, p].norm() == 0, p
            continue
        errs.append(rel(feat[:, p], ref[:, p]))
    print("fp32x forward at the forced partition vs fp32 oracle, per path:", [f"{e:.2e}" for e in errs])
    assert max(errs) < X3_LAYER_TOL, errs
    hp.check_x3_status()


@gpu
def test_packed_conv_forward_multi_step_partitions_bit_equal(hip_lib):
    """x3_conv_fwd has no knob (max(2, units * P / 512) per workgroup): at P = 5, E = 16 one launch of T = 3 steps of
    the first layer takes 3 bands per workgroup (straddling the 5-band samples), one launch of T = 13 steps of conv2 /
    conv3 3 samples per workgroup with a tail of 1 == one launch per step (2 per workgroup), planes and ReLU bits."""
    from pathnet_gym_amd.models.acnet import ACPathNet
    from pathnet_gym_amd.ops.pathnet_ops import _plane
    cfg = pixel_cfg()
    m = ACPathNet(cfg, P_, DEV, "hip", seed=11, compute_dtype="fp32x")
    m.set_paths(masks_with_edges(P_, cfg.L, cfg.M, cfg.N, seed=6))
    hp = m.hip
    cnt = m.act_cnt.view(P_, -1).cpu()
    B = P_ * E_
    gen = torch.Generator(device="cpu").manual_seed(5)
    obs = torch.randint(0, 256, (13 * B, 160, 120, 4), generator=gen, dtype=torch.uint8).to(DEV)

    def run(l, X, T, at_once):
        Y = hp.alloc_act(l, (T, B, hp.geoms[l].out_feat))
        b, rows = hp.alloc_bits(l, T, B)
        if at_once:
            hp.layer_fwd(l, X, Y, b, P_, E_, T, 0, rows)
        else:
            for t in range(T):
                hp.layer_fwd(l, X, Y, b, P_, E_, 1, t, rows)
        torch.cuda.synchronize()
        return Y, b

    X = obs
    for l, T in ((0, 3), (0, 13), (1, 13), (2, 13)):
        if (l, T) == (0, 13):
            X = run(0, obs, 13, True)[0]                 # the input of the conv2 / conv3 runs
            continue
        (Ya, ba), (Yb, bb) = run(l, X, T, True), run(l, X, T, False)
        assert float(Ya.float().abs().sum()) > 0
        assert torch.equal(Ya, Yb) and torch.equal(_plane(Ya, 1, torch.float16), _plane(Yb, 1, torch.float16)), l
        hw = hp.geoms[l].HWo
        for p in range(P_):
            k = int(cnt[p, l])
            for t in range(T):
                r0 = (t * B + p * E_) * hw
                assert torch.equal(ba[:k, r0:r0 + E_ * hw], bb[:k, r0:r0 + E_ * hw]), (l, p, t)
        if l > 0:
            X = Ya
    hp.check_x3_status()


# ---------------------------------------------------------------------------------------------------------------
# (2) conv input gradients: bit-identical under every partition
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("l", [1, 2])
def test_conv_dgrad_partitions_bit_equal(part, l):
    """conv_dgrad_x3 at 2 / 10 / 80 / 144 samples per workgroup, on the cost-balanced 1-D schedule whose workgroups
    span paths (BAL, the default) and on the per-path grid with the sample split of paths of > 4 slots (gridDim.z = 2)
    == the default partition, and == the gradient the engine's own backward stored: one workgroup computes a sample's
    dX in slot-group order and the amax it writes is a max.  dX is pre-filled with NaN: every row of the T*B samples
    comes back finite, the rows of a path whose layer is empty exactly zero, the rows past T*B stay NaN."""
    eng, hp = part.eng, part.hp
    R = T_ * P_ * E_
    outs = []
    for s in DGRAD:
        dX = torch.full((R + 64, hp.geoms[l - 1].out_feat), float("nan"), device=DEV)
        hp.gamax.copy_(part.gamax)
        hp.gamax[l - 1] = 0.0
        with knobs(hp, **s.knobs):
            hp.layer_bwd(l, eng.acts[l - 1], eng.grads[l], eng.bits[l], part.zero_grad(), dX, P_, E_, T_,
                         eng.bits_rows[l], part="d")
        torch.cuda.synchronize()
        outs.append((dX, hp.gamax.clone()))
        hp.gamax.copy_(part.gamax)
        assert bool(torch.isfinite(dX[:R]).all()), s.id
        assert bool(torch.isnan(dX[R:]).all()), s.id
    d0, am0 = outs[0]
    assert float(d0[:R].norm()) > 0
    empty = [p for p in range(P_) if part.cnt[p, l] == 0]
    assert empty or l == 2
    for p in empty:
        assert int(d0[:R].view(T_, P_, E_, -1)[:, p].count_nonzero()) == 0, p
    assert torch.equal(d0[:R], eng.grads[l - 1]) and torch.equal(am0, part.gamax)
    for s, (d, am) in zip(DGRAD[1:], outs[1:]):
        assert torch.equal(d[:R], d0[:R]) and torch.equal(am, am0), (l, s.id)


# ---------------------------------------------------------------------------------------------------------------
# (3) weight gradients against float64, per launcher and setting
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("s", RING_WGRAD, ids=ids(RING_WGRAD))
def test_conv1_ring_wgrad_partitions_vs_float64(part, s):
    """conv_wgrad_slab_x3 on the frame ring at 8 (the floor), 120 (the fixed per-path size, sample-aligned), 134 and 267
    (the bench values: workgroups begin and end mid-sample and cross env and step boundaries, with a tail) and 2880
    slabs per workgroup (one per path: 146 staged first-valid bytes), step-major and env-major, and once as the
    launcher sizes it itself (X3_WG_AUTO)."""
    part.run_wgrad("ring", s)


@gpu
@pytest.mark.parametrize("s", PACKED_C1_WGRAD, ids=ids(PACKED_C1_WGRAD))
def test_conv1_packed_wgrad_partitions_vs_float64(part, s):
    part.run_wgrad("packed1", s)


@gpu
@pytest.mark.parametrize("s", C2_WGRAD, ids=ids(C2_WGRAD))
def test_conv2_wgrad_partitions_vs_float64(part, s):
    """conv_wgrad_slab_x3, 4x4/s2: 8, 30 and 240 (bench, sample-aligned), 31 (straddling) and 432 (the whole path)
    slabs per workgroup; a 1.02 scale of any module's reference fails criterion (b) at every one."""
    part.run_wgrad("conv2", s, scale_control=True)


@gpu
@pytest.mark.parametrize("s", C3_WGRAD, ids=ids(C3_WGRAD))
def test_conv3_wgrad_partitions_vs_float64(part, s):
    part.run_wgrad("conv3", s)


@gpu
@pytest.mark.parametrize("s", FC2_WGRAD, ids=ids(FC2_WGRAD))
def test_fc2_wgrad_partitions_vs_float64(part, s):
    """fc_wgrad_x3 with a module's users split 5 ways (at most one path per workgroup), 3 and 2 ways (several paths per
    workgroup, unevenly) and not at all (nsplit == 1: the kernel stores instead of adding); a 1.02 scale of any
    module's reference fails criterion (b) at every one."""
    part.run_wgrad("fc2", s, scale_control=True)


@gpu
@pytest.mark.parametrize("s", FC1_WGRAD, ids=ids(FC1_WGRAD))
def test_fc1_wgrad_gm_partitions_vs_float64(part, s):
    part.run_wgrad("fc1", s)


# ---------------------------------------------------------------------------------------------------------------
# (4) the deterministic mode
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("launcher", list(DET))
def test_deterministic_wgrad_partitions_vs_float64_and_repeat(part_det, launcher):
    """The int64 fixed-point accumulation at the default, a straddling (fc: uneven) and the whole-path partition of
    every weight-gradient launcher: criteria (a) (with the quantisation term) and (b), the accumulator left zero, and a
    repeat under the same setting bit-identical."""
    for s in DET[launcher]:
        grad, _ = part_det.run_wgrad(launcher, s, tag=".det")
        again = part_det.zero_grad()
        with knobs(part_det.hp, **s.knobs):
            part_det.wgrad(launcher, again)
        assert torch.equal(again, grad), (launcher, s.id)
    part_det.hp.check_x3_status()


# ---------------------------------------------------------------------------------------------------------------
# (5) negative controls: a condition on the test, not on the kernel
# ---------------------------------------------------------------------------------------------------------------
def _unit_controls(ctx, launcher, s, l, rows_of, what):
    """Of every (path, slot) pair, the row set of ``rows_of`` with the largest masked gradient; of those units, the one
    that is the largest share of its module's gradient (a unit that is 1e-5 of the norm cannot move criterion (b),
    whatever the check).  The reference without it, and with it twice, must fail (b); the reference as it is passes."""
    _, got = ctx.run_wgrad(launcher, s, tag=".control")
    truth = ctx.truth(l)["dW"]
    best = None
    for p in range(P_):
        if not ctx.cnt[p, l]:
            continue
        A = ctx.operand(l, p)
        for a, j in ctx.slots(l, p):
            Gm = ctx.masked_g(l, p, a)
            mass = torch.stack([Gm[r].abs().sum() for r in rows_of])
            rows = rows_of[int(mass.argmax())]
            unit = A[rows].t() @ Gm[rows]
            share = float(unit.norm() / truth[j].norm())
            if best is None or share > best[0]:
                best = (share, j, p, a, unit)
    share, j, p, a, unit = best
    assert share > 0
    w = got[j][0]
    e0, e_drop, e_twice = rel(w, truth[j]), rel(w, truth[j] - unit), rel(w, truth[j] + unit)
    print(f"{launcher}.{s.id}, module {j} (path {p}, slot {a}), {what} ({share:.2e} of the module's gradient): rel "
          f"{e0:.2e}; dropped from the reference {e_drop:.2e}; counted twice {e_twice:.2e}")
    assert e0 < X3_LAYER_TOL < min(e_drop, e_twice), (e0, e_drop, e_twice)


@gpu
def test_negative_control_conv2_slab_unit(part):
    """conv2 at 31 slabs per workgroup (straddling): one sample's last slab (output rows 14..17) dropped from, or
    counted twice in, the reference of a module whose masked gradient is non-zero there fails criterion (b)."""
    g = part.hp.geoms[1]
    last = range(2 * 7 * g.Wo, g.HWo)                       # the positions of slab 2 of Slab<C2, 7>
    rows_of = [slice(smp * g.HWo + last.start, (smp + 1) * g.HWo) for smp in range(NSAMP)]
    _unit_controls(part, "conv2", C2_WGRAD[3], 1, rows_of, "one sample's last slab")


@gpu
def test_negative_control_fc2_row_block(part):
    """fc2 with its users split 3 ways (unevenly): one 32-row block of one user path dropped from, or counted twice
    in, the reference fails criterion (b)."""
    rows_of = [slice(r, min(r + 32, NSAMP)) for r in range(0, NSAMP, 32)]
    _unit_controls(part, "fc2", FC2_WGRAD[1], 4, rows_of, "one 32-row block of one user path")
