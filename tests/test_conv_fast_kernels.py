"""The compile-time-geometry bf16 conv kernels (csrc/conv_fast.hip) launcher by launcher against plain float64.

C1 160x120x4 uint8 k8 s4 (K 256, 39x29 outputs), C2 39x29x8 k4 s2 (K 128, 18x13), C3 18x13x8 k3 s1 (K 72 padded to 96,
16x11): the hot path of ``compute_dtype="bf16"``.  The method is that of tests/test_trunk_geometry.py, whose float64
reference and comparison code this file imports: every launcher runs alone, through ``_lib.call_fast`` / ``_lib.call``,
on a one-layer parameter buffer of the test's own (LEAD floats in front, GAP floats after every module, TAILW after the
layer); the reference is fed what the kernel read -- the operand copy read back from the device and widened, the uint8
pixels or a bf16 activation of the test's own, ReLU bits of the test's own for the backward launchers.  Every assertion
is element by element; outputs carry 64 sentinel rows, float inputs 64 rows of NaN (uint8: 255), dX is pre-filled with
NaN, bit planes of slots a path does not have keep their sentinel, a module on no path has an exactly zero gradient.

Rounding models, read from csrc/conv_fast.hip:

conv_fwd_fast<.., F16>   fp16 MFMA on (1024 + pixel) (`u8x8_to_f16off`, common.h) times the fp16 copy, fp32 accumulation;
          `bv -= 1024.f * in_scale * hcorr[mods[tid >> 3] * 8 + (tid & 7)]`, then `v = acc * in_scale + bb`,
          `pos = v > 0.f`, `Y = f2bf(sum[r] * out_scale)`.  The reference is in_scale ((1024 + x) @ W16) + b', b' the
          corrected bias in float64 from the hcorr read back.  Products are exact in fp32, so the slot bound is
          K 2^-23 in_scale ((1024 + x) @ |W16|) + 2^-23 |pre| + 4 * 2^-23 (|1024 in_scale hcorr| + |b|) (three roundings
          form b').  hcorr itself: fp32 sum of K fp16 values against the float64 column sum, K 2^-24 sum |w|.
conv_fwd_fast (no F16), conv_fwd_slab, conv_fwd_img   bf16 MFMA on the bf16 copy; the bound of ``forward_ref`` with the
          2^-8 |y| of the bf16 store.
conv_wgrad_fast / conv_wgrad_slab   the masked G goes to bf16 unscaled (`v = f32x8_to_bf16(gg)` / `f32x8_to_bf16(m)`),
          the accumulator is scaled once (`acc[mi][nt][r] * (in_scale * g_scale)`), the bias gradient sums the unrounded
          masked G (`bpart[c] += gg[c]`, `acc_b[k][c] += m[c]`) and is scaled at the end (`* g_scale`): ``backward_ref``
          with round_w and scale_after.  GT = bf16_t reads a G that is bf16 already.  Atomics add in any order: the
          bound n 2^-23 (|A|^T |G|) holds for every order.
conv_dgrad_fast   fp32 VALU on the fp32 master (`wt = flat + w_off + ...`), `gv = g * g_scale` unrounded.
conv_dgrad_mfma   master rounded at staging (`Bs[...] = f32x8_to_bf16(v)`), masked G * g_scale rounded
          (`f32x8_to_bf16(m)`); bf16 G at g_scale == 1 masks the raw words; dX fp32 or `f2bf(acc[nt][r])`: + 2^-8 |dX|.

Two kinds of case per launcher.  EXACT: dyadic operands (weights multiples of 2^-4 in +-0.25, biases of 2^-3, pixels
0..255, bf16 inputs multiples of 2^-3 below 8, G in {-1, 0, 1}, power-of-two scales) for which every product and every
partial sum in any order is exact in fp32 -- tests/test_conv_fast_host.py proves that per case -- so Y, every ReLU bit
(``v > 0`` at pre == 0 included: one all-zero sample meets a zero bias), every gradient and dX must equal the reference
bit for bit, nothing excluded.  RANDOM: the model's init, uniform pixels, G ~ N(0, 1), in_scale = fp32(1/255),
out_scale = g_scale = fp32(1/M), inside the derived bound; ReLU bits must equal pre64 > 0 wherever |pre64| exceeds the
slot bound and at most 1 % of a layer's decisions may lie inside it.

The worst measured |hip - ref| / bound per launcher and setting is kept in tests/data/conv_fast_measured.json (written
when ``PATHNET_RECORD_CONV_FAST=<file>`` is set): a record, not a budget.
"""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pathnet_gym_amd.config import LayerSpec, PathNetConfig
from pathnet_gym_amd.models.pathnet import ParamStore
from test_trunk_geometry import (BITS_SENT8, EPS, IN_SCALE, PAD, SENT, Layer, act_lists, as_input, backward_ref,
                                 col2im, compare, forward_ref, im2col, padded, path_rows, unpack_bits, within)

gpu = pytest.mark.gpu
DEV = "cuda"
P = 4
LEAD, GAP, TAILW = 40, 8, 24
GEOM = {"C1": ((160, 120, 4), 8, 4, True), "C2": ((39, 29, 8), 4, 2, False), "C3": ((18, 13, 8), 3, 1, False)}
# every launcher of the extern "C" block of csrc/conv_fast.hip; launch() / setter() refuse any other name
LAUNCHERS = ("fast_conv_fwd", "fast_conv_wgrad", "fast_conv_dgrad", "fast_conv_dgrad_bf16", "fast_conv_wgrad_bf16g",
             "fast_conv1_ring_fwd", "fast_conv1_ring_wgrad")
# setter -> the default written in csrc/conv_fast.hip
SETTERS = {"fast_conv_set_slab": 1, "fast_conv_set_slab_fwd": 0, "fast_conv_set_dgrad_mfma": 1,
           "fast_conv_set_img_fwd": 0, "fast_conv_set_wgrad_ob": 2, "fast_conv_set_fwd_nt": 4,
           "fast_conv_set_wgrad_pf": 2, "fast_conv_set_f16_fwd": 1}
EXACT_SCALES = {"C1": (2.0 ** -8, 2.0 ** -3, 2.0 ** -3), "C2": (2.0 ** -2, 2.0 ** -3, 2.0 ** -3),
                "C3": (2.0 ** -2, 2.0 ** -3, 2.0 ** -3)}

# (geometry, E, T, M, t0, cnts): cnts = active modules per path; None = the edges of random_masks (an empty layer, a
# path with all M modules, a single last module, N = 4 random ones)
C1_CASES = [("C1", 16, 1, 10, 0, None), ("C1", 16, 2, 10, 0, None), ("C1", 16, 3, 10, 0, None),
            ("C1", 16, 1, 10, 1, None), ("C1", 16, 1, 3, 0, None)]
C2_CASES = [("C2", 8, 1, 10, 0, None), ("C2", 8, 3, 10, 0, None), ("C2", 16, 1, 10, 0, None), ("C2", 8, 1, 3, 0, None)]
C3_CASES = [("C3", E, T, 10, 0, None) for E in (1, 3, 5, 16) for T in (1, 2)] + \
           [("C3", 3, 1, 3, 0, None), ("C3", 5, 1, 10, 0, (5, 7, 3, 6)), ("C3", 1, 1, 10, 1, None)]
M16_CASE = ("C3", 3, 1, 16, 0, (0, 16, 1, 4))
RING_CASES = [("C1", 16, 2, 10, 0, None), ("C1", 16, 1, 10, 1, None)]
KINDS = ("exact", "random")


def case_id(c):
    name, E, T, M, t0, cnts = c
    return f"{name}-E{E}-T{T}-M{M}" + (f"-t{t0}" if t0 else "") + ("-mixed" if cnts and M <= 10 else "")


# ---------------------------------------------------------------------------------------------------------------
# cases (CPU tensors only: tests/test_conv_fast_host.py builds the same ones)
# ---------------------------------------------------------------------------------------------------------------
def make_layer(name, M, in_scale, out_scale):
    inp, k, s, _ = GEOM[name]
    cfg = PathNetConfig(L=1, M=M, N=min(4, M), input_shape=inp, layers=[LayerSpec("conv", 8, k, s)], trunk_scale="M",
                        num_actions=2)
    ly = Layer(cfg, 0)
    ly.in_scale, ly.out_scale = float(in_scale), float(out_scale)
    return ly, cfg


def path_masks(M, cnts, rng):
    """[P, 1, M] expressed-module masks.  cnts None: path 0 none, path 1 all M, path 2 the last module alone, path 3
    min(4, M - 1) random ones (M = 3: two, so that cnt 1, 2 and 3 occur)."""
    m = np.zeros((P, 1, M), np.float32)
    if cnts is None:
        m[1] = 1
        m[2, 0, M - 1] = 1
        m[3, 0, rng.permutation(M)[:min(4, M - 1)]] = 1
    else:
        for p, c in enumerate(cnts):
            m[p, 0, rng.permutation(M)[:c]] = 1
    return m


_CASES = {}


def make_case(spec, kind, ring=False):
    key = (spec, kind, ring)
    if key in _CASES:
        return _CASES[key]
    name, E, T, M, t0, cnts = spec
    exact = kind == "exact"
    seed = 1000 * (1 + list(GEOM).index(name)) + 97 * E + 13 * T + M + 7 * t0 + (500 if ring else 0)
    g = torch.Generator().manual_seed(seed)
    rng = np.random.RandomState(seed)
    i_s, o_s, g_s = EXACT_SCALES[name] if exact else ((IN_SCALE if name == "C1" else 1.0),
                                                     float(np.float32(1.0 / M)), float(np.float32(1.0 / M)))
    ly, cfg = make_layer(name, M, i_s, o_s)
    cs = SimpleNamespace(spec=spec, name=name, kind=kind, exact=exact, ring=ring, ly=ly, E=E, T=T, M=M, t0=t0,
                         steps=t0 + T, B=P * E, in_scale=i_s, out_scale=o_s, g_scale=g_s, u8=GEOM[name][3], refs={})
    mask = path_masks(M, cnts, rng)
    cs.acts = [a[0] for a in act_lists(mask)]
    cs.idx = torch.zeros(P, 1, M, dtype=torch.int32)
    cs.cnt = torch.zeros(P, 1, dtype=torch.int32)
    for p in range(P):
        cs.cnt[p, 0] = len(cs.acts[p])
        cs.idx[p, 0, :len(cs.acts[p])] = torch.tensor([int(j) for j in cs.acts[p]], dtype=torch.int32)
    K = ly.K
    if exact:
        W = torch.randint(-4, 5, (M, K, 8), generator=g).float() / 16.0
        b = torch.randint(-4, 5, (M, 8), generator=g).float() / 8.0
        b[:, 0] = 0.0                                  # meets the all-zero sample below: pre == 0 exactly
    else:
        st = ParamStore(cfg, "cpu", seed=seed)
        W, b = st.W(0).clone(), st.b(0).clone()
    cs.W, cs.b = W, b
    cs.chunk = K * 8 + 8 + GAP
    cs.w_off, cs.b_off = LEAD, LEAD + K * 8
    cs.numel = LEAD + M * cs.chunk + TAILW
    flat = torch.zeros(cs.numel)
    seg = flat[LEAD:LEAD + M * cs.chunk].view(M, cs.chunk)
    seg[:, :K * 8] = W.reshape(M, K * 8)
    seg[:, K * 8:K * 8 + 8] = b
    seg[:, K * 8 + 8:] = float("nan")                  # the gap after a module is never read
    flat[:LEAD] = float("nan")
    flat[LEAD + M * cs.chunk:] = float("nan")
    cs.flat = flat
    S, B = cs.steps, cs.B
    if cs.u8:
        if ring:
            cs.nslots = S + 3 + 2
            cs.frames = torch.randint(0, 256, (B, cs.nslots, 160 * 120), generator=g, dtype=torch.uint8)
            fc = torch.randint(0, 4, (S + 1, B), generator=g, dtype=torch.uint8)
            fc[:, :4] = torch.tensor([0, 1, 2, 3], dtype=torch.uint8)          # every value in every step ...
            fc[-2, :4] = torch.tensor([3, 0, 1, 2], dtype=torch.uint8)         # ... and a change between steps
            if exact:
                for p in range(P):
                    cs.frames[p * E + E - 1, :4] = 0
            cs.fc = fc
            x = torch.zeros(S, B, 160 * 120, 4, dtype=torch.uint8)
            for t in range(S):
                for c in range(4):
                    slot = t + torch.clamp(fc[t].long(), min=c)                # t + max(c, fc[t][b])
                    x[t, :, :, c] = cs.frames[torch.arange(B), slot]
            x = x.reshape(S, P, E, ly.in_feat)
        else:
            x = torch.randint(0, 256, (S, P, E, ly.in_feat), generator=g, dtype=torch.uint8)
    elif exact:
        x = (torch.randint(0, 64, (S, P, E, ly.in_feat), generator=g).float() / 8.0).to(torch.bfloat16)
    else:
        x = (torch.randn(S, P, E, ly.in_feat, generator=g).abs() * 0.5).to(torch.bfloat16)
    if exact and not ring:
        x[t0, :, E - 1] = 0
    cs.x = x
    R = T * E * ly.HWo
    if exact:
        dens = 0.125 if name == "C1" else 0.5          # C1: keeps every weight-gradient sum below 2^24 units
        cs.G = (torch.randint(0, 2, (T, P, E, ly.out_feat), generator=g) * 2 - 1).float() * \
            (torch.rand(T, P, E, ly.out_feat, generator=g) < dens).float()
    else:
        cs.G = torch.randn(T, P, E, ly.out_feat, generator=g)
    cs.bits = [torch.rand(len(cs.acts[p]), R, 8, generator=g) < 0.5 for p in range(P)]
    _CASES[key] = cs
    return cs


def pack_planes(cs, bits, t0=0, steps=None):
    """ReLU bits[p] [cnt, T*E*HWo, 8] (bool) -> the kernels' bit planes [M, steps*B*HWo + PAD] uint8: byte of a row =
    its 8 maps, rows (t, p, e, pos); everything else (inactive slots, other steps, the PAD rows) the sentinel."""
    ly, T, E = cs.ly, cs.T, cs.E
    steps = T if steps is None else steps
    planes = torch.full((cs.M, steps, P, E * ly.HWo), BITS_SENT8, dtype=torch.uint8)
    wts = (2 ** torch.arange(8)).to(torch.int32)
    for p in range(P):
        c = len(cs.acts[p])
        if c:
            by = (bits[p].to(torch.int32) * wts).sum(-1).to(torch.uint8)            # [cnt, R]
            planes[:c, t0:t0 + T, p] = by.reshape(c, T, E * ly.HWo)
    out = torch.full((cs.M, steps * cs.B * ly.HWo + PAD), BITS_SENT8, dtype=torch.uint8)
    out[:, :steps * cs.B * ly.HWo] = planes.reshape(cs.M, -1)
    return out


def cmajor(W):
    """[M, K, 8] in the master's (kh, kw, ci) order -> the frame ring's channel-major [M, 8, K], k' = (ci*8 + kh)*8 + kw."""
    M = W.shape[0]
    return W.reshape(M, 8, 8, 4, 8).permute(0, 4, 3, 1, 2).reshape(M, 8, 256).contiguous()


def from_cmajor(Wr):
    """Inverse of cmajor: [M, 8, 256] -> [M, K, 8] in the master's order."""
    M = Wr.shape[0]
    return Wr.reshape(M, 8, 4, 8, 8).permute(0, 3, 4, 2, 1).reshape(M, 256, 8).contiguous()


# ---------------------------------------------------------------------------------------------------------------
# float64 references (cached per case) and the checks every result goes through, from the GPU or from the emulation
# ---------------------------------------------------------------------------------------------------------------
def fwd_reference(cs, W64, hcorr=None):
    """-> (y, bound, pres, slot bounds) of steps t0 .. t0+T-1; hcorr (fp32, as read back): the fp16-offset path."""
    key = ("fwd_f16", hcorr.numpy().tobytes()) if hcorr is not None else "fwd_bf16"
    if key not in cs.refs:
        x = cs.x[cs.t0:cs.t0 + cs.T]
        b64 = cs.b.double()
        if hcorr is None:
            cs.refs[key] = forward_ref(cs.ly, x, W64, b64, cs.acts, True)
        else:
            corr = 1024.0 * cs.in_scale * hcorr.double().reshape(cs.M, 8)
            slack = None if cs.exact else 4 * EPS * (corr.abs() + b64.abs())
            cs.refs[key] = forward_ref(cs.ly, x, W64, b64 - corr, cs.acts, True, offset=1024.0, bias_slack=slack)
    return cs.refs[key]


def wgrad_reference(cs, g_bf16=False):
    key = "wgrad_bf16g" if g_bf16 else "wgrad"
    if key not in cs.refs:
        G = cs.G.to(torch.bfloat16).float() if g_bf16 else cs.G
        cs.refs[key] = backward_ref(cs.ly, cs.x[:cs.T], G, cs.bits, None, cs.acts, cs.M, cs.g_scale, round_w=True,
                                    want_dx=False, scale_after=True)
    return cs.refs[key]


def dgrad_reference(cs, mfma, g_bf16=False, dx_bf16=False, g_scale=None):
    g_scale = cs.g_scale if g_scale is None else g_scale
    key = ("dgrad", mfma, g_bf16, dx_bf16, g_scale)
    if key not in cs.refs:
        G = cs.G.to(torch.bfloat16).float() if g_bf16 else cs.G
        Wd = (cs.W.to(torch.bfloat16) if mfma else cs.W).double()
        r = backward_ref(cs.ly, cs.x[:cs.T], G, cs.bits, Wd, cs.acts, cs.M, g_scale, round_d=mfma, want_dx=True)
        bX = r["bX"] + (2.0 ** -8 * r["dX"].abs() if dx_bf16 else 0.0)
        cs.refs[key] = (r["dX"], bX)
    return cs.refs[key]


RATIOS = {}


def record(key, value):
    """PATHNET_RECORD_CONV_FAST=<file>: keep the worst measured error / bound per launcher and setting."""
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(value))
    rec = os.environ.get("PATHNET_RECORD_CONV_FAST")
    if not rec:
        return
    d = {}
    if os.path.exists(rec):
        with open(rec) as f:
            d = json.load(f)
    t = d.setdefault("worst_err_over_bound", {})
    t[key] = max(float(value), float(t.get(key, 0.0)))
    os.makedirs(os.path.dirname(rec) or ".", exist_ok=True)
    with open(rec, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def bf16_bits(t):
    return t.contiguous().view(torch.int16)


def check_forward(cs, ref, Y, planes, key, rec=True):
    """Y [steps*B + PAD, out_feat] bf16 and bit planes [M, steps*B*HWo + PAD] (CPU) against the reference."""
    ly, T, E, B, t0 = cs.ly, cs.T, cs.E, cs.B, cs.t0
    y, yb, pres, bnds = ref
    r0, r1 = t0 * B, (t0 + T) * B
    got = Y[r0:r1].reshape(T, P, E, -1)
    if cs.exact:
        want = (y.float()).to(torch.bfloat16)
        nbad = int((bf16_bits(got) != bf16_bits(want)).sum())
        assert nbad == 0, f"{key}: {nbad} of {want.numel()} Y elements differ from the exact reference"
    else:
        ratios = {}
        within(f"{key} Y", got, y, yb, ratios, "r")
        if rec:
            record(key + ".Y", ratios["r"])
    assert bool((Y[:r0].float() == SENT).all()) and bool((Y[r1:].float() == SENT).all()), f"{key}: Y rows outside written"
    rows0, rows = t0 * B * ly.HWo, T * B * ly.HWo
    assert bool((planes[:, :rows0] == BITS_SENT8).all()) and bool((planes[:, rows0 + rows:] == BITS_SENT8).all()), \
        f"{key}: ReLU bits outside the steps written"
    hb = planes[:, rows0:rows0 + rows]
    left_out = total = 0
    for p in range(P):
        c = len(cs.acts[p])
        got = unpack_bits(ly, hb, rows, c, p, T, P, E)
        want = pres[p] > 0
        if cs.exact:
            nbad = int((got != want).sum())
            assert nbad == 0, f"{key} path {p}: {nbad} ReLU bits differ from pre64 > 0 (exact case)"
        else:
            sure = pres[p].abs() > bnds[p]
            nbad = int((got != want)[sure].sum())
            assert nbad == 0, f"{key} path {p}: {nbad} ReLU bits differ from pre64 > 0 outside the slot bound"
            left_out += int((~sure).sum())
            total += sure.numel()
        if c < cs.M:
            un = hb[c:].reshape(cs.M - c, T, P, -1)[:, :, p]
            assert bool((un == BITS_SENT8).all()), f"{key} path {p}: bits of inactive slots written"
    if not cs.exact:
        print(f"{key}: {left_out}/{total} ReLU decisions inside the slot bound")
        assert left_out <= 0.01 * max(total, 1), f"{key}: {left_out}/{total} ReLU decisions inside the bound"
    return left_out, total


def check_wgrad(cs, r, grad, key, rec=True):
    """grad [numel + 8*PAD] fp32 (CPU): the layer's segment against dW / db, zeros everywhere else."""
    ly, M, K = cs.ly, cs.M, cs.ly.K
    lo, hi = LEAD, LEAD + M * cs.chunk
    seg = grad[lo:hi].reshape(M, cs.chunk)
    dW, db = seg[:, :K * 8].reshape(M, K, 8), seg[:, K * 8:K * 8 + 8]
    if cs.exact:
        for nm, got, want in (("dW", dW, r["dW"]), ("db", db, r["db"])):
            nbad = int((got.double() != want).sum())
            assert nbad == 0, f"{key}: {nbad} of {want.numel()} {nm} elements differ from the exact reference"
    else:
        ratios = {}
        within(f"{key} dW", dW, r["dW"], r["bW"], ratios, "w")
        within(f"{key} db", db, r["db"], r["bb"], ratios, "b")
        if rec:
            record(key + ".dW", ratios["w"])
            record(key + ".db", ratios["b"])
    for j in range(M):
        if r["users"][j] == 0:
            assert not seg[j].any(), f"{key}: module {j} is on no path but has a gradient"
    assert not seg[:, K * 8 + 8:].any(), f"{key}: gradient written between two modules"
    assert not grad[:lo].any() and not grad[hi:cs.numel].any(), f"{key}: gradient outside the layer"
    assert bool((grad[cs.numel:] == SENT).all()), f"{key}: gradient sentinel overwritten"


def check_dgrad(cs, ref, dX, key, rec=True):
    """dX [T*B + PAD, in_feat] fp32 or bf16 (CPU)."""
    T, E, B = cs.T, cs.E, cs.B
    want, bound = ref
    got = dX[:T * B].reshape(T, P, E, -1)
    if cs.exact:
        w = want.float().to(dX.dtype)
        nbad = int(((got.double() != w.double()) | ~torch.isfinite(got.double())).sum())
        assert nbad == 0, f"{key}: {nbad} of {w.numel()} dX elements differ from the exact reference"
    else:
        ratios = {}
        within(f"{key} dX", got, want, bound, ratios, "r")
        if rec:
            record(key + ".dX", ratios["r"])
    assert bool((dX[T * B:].float() == SENT).all()), f"{key}: dX sentinel rows overwritten"


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
def _L():
    from pathnet_gym_amd.ops import _lib
    return _lib


def launch(name, *args):
    assert name in LAUNCHERS, name
    _lib = _L()
    if name.startswith("fast_conv1_ring"):
        _lib.call(name, *args, _lib.stream())             # 0 on success
        return True
    return _lib.call_fast(name, *args, _lib.stream())


def setter(name, value):
    assert name in SETTERS, name
    getattr(_L().lib(), name)(int(value))


class settings:
    """with settings(fast_conv_set_slab=0, ...): every setter back at its default on exit."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            setter(k, v)

    def __exit__(self, *exc):
        for k in SETTERS:
            setter(k, SETTERS[k])


def geo_args(cs):
    ly = cs.ly
    return (ly.Hin, ly.Win, ly.Cin, ly.KH, ly.KW, ly.S)


def device_setup(cs):
    """The parameter buffer, module tables and operand copies on the device (made by the project's own refresh
    launchers), each copy checked bit for bit against the cast of the master; -> namespace with the copies widened."""
    if getattr(cs, "dv", None) is not None:
        return cs.dv
    _lib = _L()
    ly, M, K = cs.ly, cs.M, cs.ly.K
    KP = (K + 31) // 32 * 32
    dv = SimpleNamespace(flat=cs.flat.to(DEV), idx=cs.idx.to(DEV), cnt=cs.cnt.to(DEV), KP=KP)
    dv.Wc = torch.full((M, 8, KP), float("nan"), dtype=torch.bfloat16, device=DEV)
    _lib.call("launch_refresh_weights", dv.flat.data_ptr(), cs.w_off, cs.chunk, K, KP, 8, M, dv.Wc.data_ptr(), None,
              _lib.stream())
    want = torch.zeros(M, 8, KP, dtype=torch.bfloat16)
    want[:, :, :K] = cs.W.to(torch.bfloat16).permute(0, 2, 1)
    assert torch.equal(bf16_bits(dv.Wc.cpu()), bf16_bits(want)), "bf16 operand copy"
    dv.W64 = dv.Wc[:, :, :K].permute(0, 2, 1).double().cpu()
    if cs.u8:
        dv.Wh = torch.full((M, 8, KP), float("nan"), dtype=torch.float16, device=DEV)
        dv.hcorr = torch.full((M * 8,), float("nan"), dtype=torch.float32, device=DEV)
        _lib.call("launch_refresh_weights_f16", dv.flat.data_ptr(), cs.w_off, cs.chunk, K, KP, 8, M, dv.Wh.data_ptr(),
                  dv.hcorr.data_ptr(), _lib.stream())
        wanth = cs.W.to(torch.float16).permute(0, 2, 1).contiguous()
        assert torch.equal(dv.Wh.cpu().view(torch.int16), wanth.view(torch.int16)), "fp16 operand copy"
        dv.Wh64 = dv.Wh.permute(0, 2, 1).double().cpu()
        dv.hc = dv.hcorr.cpu()
        colsum = dv.Wh64.sum(1)                                                     # [M, 8]
        hb = K * 2.0 ** -24 * dv.Wh64.abs().sum(1)
        nbad, worst = compare(dv.hc.reshape(M, 8), colsum, hb)
        assert nbad == 0, f"hcorr: {nbad} column sums outside K 2^-24 sum |w| (worst {worst:.3g})"
        if cs.exact:
            assert torch.equal(dv.hc.reshape(M, 8).double(), colsum)
        if cs.ring:
            dv.Wc_ring = torch.full((M, 8, KP), float("nan"), dtype=torch.bfloat16, device=DEV)
            dv.Wh_ring = torch.full((M, 8, KP), float("nan"), dtype=torch.float16, device=DEV)
            for buf, f16 in ((dv.Wc_ring, 0), (dv.Wh_ring, 1)):
                _lib.call("launch_refresh_weights_cmajor", dv.flat.data_ptr(), cs.w_off, cs.chunk, 8, 8, 4, 8, M,
                          buf.data_ptr(), f16, _lib.stream())
            assert torch.equal(bf16_bits(dv.Wc_ring.cpu()), bf16_bits(cmajor(cs.W.to(torch.bfloat16)))), "Wc_ring"
            assert torch.equal(dv.Wh_ring.cpu().view(torch.int16), cmajor(cs.W.to(torch.float16)).view(torch.int16)), \
                "Wh_ring"
            dv.Wr64 = from_cmajor(dv.Wc_ring.cpu()).double()
            dv.Whr64 = from_cmajor(dv.Wh_ring.cpu()).double()
    cs.dv = dv
    return dv


def fwd_buffers(cs):
    ly, S, B = cs.ly, cs.steps, cs.B
    Y = padded(S * B, ly.out_feat, torch.bfloat16, SENT, SENT)
    Y[cs.t0 * B:S * B] = float("nan")
    planes = torch.full((cs.M, S * B * ly.HWo + PAD), BITS_SENT8, dtype=torch.uint8, device=DEV)
    return Y, planes


def run_fwd(cs, f16):
    dv, ly = device_setup(cs), cs.ly
    X = as_input(cs.x.reshape(cs.steps * cs.B, -1).to(DEV), torch.uint8 if cs.u8 else torch.bfloat16)
    Y, planes = fwd_buffers(cs)
    wop = dv.Wh if (cs.u8 and f16) else dv.Wc
    ok = launch("fast_conv_fwd", X.data_ptr(), int(cs.u8), Y.data_ptr(), planes.data_ptr(), wop.data_ptr(),
                dv.flat.data_ptr(), cs.b_off, cs.chunk, dv.idx.data_ptr(), dv.cnt.data_ptr(), 0, 1, cs.M, *geo_args(cs),
                P, cs.E, cs.T, cs.t0, planes.shape[1], cs.in_scale, cs.out_scale,
                dv.hcorr.data_ptr() if (cs.u8 and f16) else None, dv.Wc.data_ptr())
    assert ok, "fast_conv_fwd did not take the specialised shape"
    torch.cuda.synchronize()
    return Y.cpu(), planes.cpu()


def fwd_ref_for(cs, f16):
    dv = device_setup(cs)
    return fwd_reference(cs, dv.Wh64, dv.hc) if (cs.u8 and f16) else fwd_reference(cs, dv.W64)


def bwd_inputs(cs, g_bf16=False):
    T, B = cs.T, cs.B
    X = as_input(cs.x[:T].reshape(T * B, -1).to(DEV), torch.uint8 if cs.u8 else torch.bfloat16)
    G = cs.G.reshape(T * B, -1)
    G = as_input(G.to(torch.bfloat16).to(DEV), torch.bfloat16) if g_bf16 else as_input(G.to(DEV), torch.float32)
    return X, G, pack_planes(cs, cs.bits).to(DEV)


def grad_buffer(cs):
    grad = torch.zeros(cs.numel + 8 * PAD, dtype=torch.float32, device=DEV)
    grad[cs.numel:] = SENT
    return grad


def run_wgrad(cs, name="fast_conv_wgrad"):
    dv = device_setup(cs)
    X, G, planes = bwd_inputs(cs, g_bf16=name.endswith("bf16g"))
    grad = grad_buffer(cs)
    ok = launch(name, X.data_ptr(), int(cs.u8), G.data_ptr(), planes.data_ptr(), grad.data_ptr(), cs.w_off, cs.b_off,
                cs.chunk, dv.idx.data_ptr(), dv.cnt.data_ptr(), 0, 1, cs.M, *geo_args(cs), P, cs.E, cs.T,
                planes.shape[1], cs.in_scale, cs.g_scale)
    assert ok, f"{name} did not take the specialised shape"
    torch.cuda.synchronize()
    return grad.cpu()


def run_dgrad(cs, name="fast_conv_dgrad", g_bf16=False, dx_bf16=False, g_scale=None):
    dv, ly = device_setup(cs), cs.ly
    g_scale = cs.g_scale if g_scale is None else g_scale
    _, G, planes = bwd_inputs(cs, g_bf16)
    dX = padded(cs.T * cs.B, ly.in_feat, torch.bfloat16 if dx_bf16 else torch.float32, float("nan"), SENT)
    common = (planes.data_ptr(), dv.flat.data_ptr(), cs.w_off, cs.chunk, dv.idx.data_ptr(), dv.cnt.data_ptr(), 0, 1,
              cs.M, *geo_args(cs), P, cs.E, cs.T, planes.shape[1], g_scale, dX.data_ptr())
    if name == "fast_conv_dgrad":
        ok = launch(name, G.data_ptr(), *common)
    else:
        ok = launch(name, G.data_ptr(), int(g_bf16), *common, int(dx_bf16))
    assert ok, f"{name} did not take the specialised shape"
    torch.cuda.synchronize()
    return dX.cpu()


def _fwd_variants(cs, variants):
    """[(label, f16, settings)] on one case: the reference is computed once per operand type."""
    for label, f16, kw in variants:
        with settings(**kw):
            Y, planes = run_fwd(cs, f16)
        check_forward(cs, fwd_ref_for(cs, f16), Y, planes, f"fast_conv_fwd[{cs.name},{label}]")


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("spec", C1_CASES, ids=case_id)
def test_conv1_forward(hip_lib, spec, kind):
    """conv_fwd_fast<C1> on packed uint8 stacks: the fp16-offset operands (default) and the bf16 ones
    (fast_conv_set_f16_fwd(0)), at 512-, 1024- and 2048-row workgroups (fast_conv_set_fwd_nt 2, 4, 8 -> NT 4, 8, 16).
    T*16*1131 rows leave tails of 688 / 352 / 16 rows of a 1024-row workgroup: a tile whose second 16-row half is past
    the end, a last workgroup of a single half.  T = 1 takes the linear row path, T > 1 the iterator; t0 = 1 writes
    the second step of a two-step buffer."""
    cs = make_case(spec, kind)
    _fwd_variants(cs, [("f16,nt4", True, {}), ("f16,nt2", True, {"fast_conv_set_fwd_nt": 2}),
                       ("f16,nt8", True, {"fast_conv_set_fwd_nt": 8}),
                       ("bf16,nt4", False, {"fast_conv_set_f16_fwd": 0}),
                       ("bf16,nt2", False, {"fast_conv_set_f16_fwd": 0, "fast_conv_set_fwd_nt": 2}),
                       ("bf16,nt8", False, {"fast_conv_set_f16_fwd": 0, "fast_conv_set_fwd_nt": 8})])


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_conv1_forward_experiments(hip_lib, kind):
    """conv_fwd_slab<C1, 2> (fast_conv_set_slab_fwd(1)) and conv_fwd_img<C1> (fast_conv_set_img_fwd(1)) at E = 16,
    T = 2: both take the bf16 copy whatever fast_conv_set_f16_fwd says."""
    cs = make_case(C1_CASES[1], kind)
    _fwd_variants(cs, [("slab_fwd", False, {"fast_conv_set_slab_fwd": 1}), ("img_fwd", False, {"fast_conv_set_img_fwd": 1})])


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("spec", C2_CASES + C3_CASES, ids=case_id)
def test_conv23_forward(hip_lib, spec, kind):
    """conv_fwd_fast<C2> / <C3> on a bf16 activation of the test's own, at 256-, 512- and 1024-row workgroups; C3 at
    E = 1 has 176 rows per path: one workgroup larger than the path."""
    cs = make_case(spec, kind)
    _fwd_variants(cs, [("nt4", False, {}), ("nt2", False, {"fast_conv_set_fwd_nt": 2}),
                       ("nt8", False, {"fast_conv_set_fwd_nt": 8})])


WG_SETTINGS = [("slab,ob2,pf2", {}), ("slab,ob3,pf2", {"fast_conv_set_wgrad_ob": 3}),
               ("slab,ob2,pf1", {"fast_conv_set_wgrad_pf": 1}),
               ("slab,ob3,pf1", {"fast_conv_set_wgrad_ob": 3, "fast_conv_set_wgrad_pf": 1}),
               ("fast", {"fast_conv_set_slab": 0})]


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("spec", [c for c in C1_CASES + C2_CASES + C3_CASES if c[4] == 0], ids=case_id)
def test_conv_wgrad(hip_lib, spec, kind):
    """fast_conv_wgrad on an fp32 G: conv_wgrad_slab (C1 at 2 and 3 output rows per stage, C2 at 7; one and two
    register sets in flight) and conv_wgrad_fast (fast_conv_set_slab(0); always for C3); fast_conv_wgrad_bf16g on the
    bf16 G for C1 and C2."""
    cs = make_case(spec, kind)
    r = wgrad_reference(cs)
    for label, kw in WG_SETTINGS:
        if cs.name == "C3" and label != "fast" or cs.name == "C2" and "ob3" in label:
            continue
        with settings(**kw):
            grad = run_wgrad(cs)
        check_wgrad(cs, r, grad, f"fast_conv_wgrad[{cs.name},{label}]")
    if cs.name != "C3":
        rb = wgrad_reference(cs, g_bf16=True)
        for label, kw in WG_SETTINGS[:2 if cs.name == "C1" else 1] + WG_SETTINGS[2:3]:
            with settings(**kw):
                grad = run_wgrad(cs, "fast_conv_wgrad_bf16g")
            check_wgrad(cs, rb, grad, f"fast_conv_wgrad_bf16g[{cs.name},{label}]")


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("spec", [c for c in C2_CASES + C3_CASES if c[4] == 0], ids=case_id)
def test_conv_dgrad(hip_lib, spec, kind):
    """fast_conv_dgrad: conv_dgrad_mfma (default) and conv_dgrad_fast (fast_conv_set_dgrad_mfma(0));
    fast_conv_dgrad_bf16 at the four combinations of a bf16 G and a bf16 dX, the bf16 G also at g_scale = 1 (raw words
    masked)."""
    cs = make_case(spec, kind)
    dX = run_dgrad(cs)
    check_dgrad(cs, dgrad_reference(cs, True), dX, f"fast_conv_dgrad[{cs.name},mfma]")
    with settings(fast_conv_set_dgrad_mfma=0):
        dX = run_dgrad(cs)
    check_dgrad(cs, dgrad_reference(cs, False), dX, f"fast_conv_dgrad[{cs.name},valu]")
    for g_bf16 in (0, 1):
        for dx_bf16 in (0, 1):
            for gs in ((cs.g_scale, 1.0) if g_bf16 else (cs.g_scale,)):
                dX = run_dgrad(cs, "fast_conv_dgrad_bf16", bool(g_bf16), bool(dx_bf16), gs)
                check_dgrad(cs, dgrad_reference(cs, True, bool(g_bf16), bool(dx_bf16), gs), dX,
                            f"fast_conv_dgrad_bf16[{cs.name},g{'bf16' if g_bf16 else 'f32'},dx{'bf16' if dx_bf16 else 'f32'}"
                            f"{',unit' if gs == 1.0 and cs.g_scale != 1.0 else ''}]")


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_conv_dgrad_sixteen_modules_take_the_valu_kernel(hip_lib, kind):
    """M = 16 (one path with all 16): fast_conv_dgrad must run conv_dgrad_fast, whose rounding model is the tighter
    one (fp32 master, unrounded G); fast_conv_dgrad_bf16, the forward and the weight gradient decline (0)."""
    cs = make_case(M16_CASE, kind)
    dv = device_setup(cs)
    dX = run_dgrad(cs)
    check_dgrad(cs, dgrad_reference(cs, False), dX, "fast_conv_dgrad[C3,M16]")
    _, G, planes = bwd_inputs(cs)
    dX = padded(cs.T * cs.B, cs.ly.in_feat, torch.float32, float("nan"), SENT)
    ok = launch("fast_conv_dgrad_bf16", G.data_ptr(), 0, planes.data_ptr(), dv.flat.data_ptr(), cs.w_off, cs.chunk,
                dv.idx.data_ptr(), dv.cnt.data_ptr(), 0, 1, cs.M, *geo_args(cs), P, cs.E, cs.T, planes.shape[1],
                cs.g_scale, dX.data_ptr(), 0)
    torch.cuda.synchronize()
    assert ok is False and bool(torch.isnan(dX[:cs.T * cs.B]).all())


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("spec", RING_CASES, ids=case_id)
def test_conv1_frame_ring(hip_lib, spec, kind):
    """fast_conv1_ring_fwd (fp16-offset and bf16 operands, NT 4 and 8) and fast_conv1_ring_wgrad (2 and 3 output rows
    per stage) on a frame ring [P*E][nslots][160*120] with nslots > t0 + T + 3, against the same reference on the
    stacks rebuilt by the kernel's rule: channel c of sample (t, b) is slot t + max(c, fc[t][b])."""
    cs = make_case(spec, kind, ring=True)
    dv = device_setup(cs)
    frames = torch.cat([cs.frames.reshape(-1), torch.full((PAD * 160 * 120,), 255, dtype=torch.uint8)]).to(DEV)
    fc = cs.fc.to(DEV)
    for label, f16, kw in (("f16,nt4", True, {}), ("f16,nt8", True, {"fast_conv_set_fwd_nt": 8}),
                           ("bf16,nt4", False, {"fast_conv_set_f16_fwd": 0})):
        Y, planes = fwd_buffers(cs)
        with settings(**kw):
            launch("fast_conv1_ring_fwd", frames.data_ptr(), fc.data_ptr(), Y.data_ptr(), planes.data_ptr(),
                   dv.Wh_ring.data_ptr(), dv.flat.data_ptr(), cs.b_off, cs.chunk, dv.idx.data_ptr(), dv.cnt.data_ptr(),
                   0, 1, cs.M, P, cs.E, cs.T, cs.t0, cs.nslots, planes.shape[1], cs.in_scale, cs.out_scale,
                   dv.hcorr.data_ptr(), dv.Wc_ring.data_ptr())
            torch.cuda.synchronize()
        ref = fwd_reference(cs, dv.Whr64, dv.hc) if f16 else fwd_reference(cs, dv.Wr64)
        check_forward(cs, ref, Y.cpu(), planes.cpu(), f"fast_conv1_ring_fwd[{label}]")
    if cs.t0:
        return                                     # the ring weight gradient always starts at step 0
    r = wgrad_reference(cs)
    _, G, planes = bwd_inputs(cs)
    for label, kw in (("ob2", {}), ("ob3", {"fast_conv_set_wgrad_ob": 3}), ("ob2,pf1", {"fast_conv_set_wgrad_pf": 1})):
        grad = grad_buffer(cs)
        with settings(**kw):
            launch("fast_conv1_ring_wgrad", frames.data_ptr(), fc.data_ptr(), G.data_ptr(), planes.data_ptr(),
                   grad.data_ptr(), cs.w_off, cs.b_off, cs.chunk, dv.idx.data_ptr(), dv.cnt.data_ptr(), 0, 1, cs.M, P,
                   cs.E, cs.T, cs.nslots, planes.shape[1], cs.in_scale, cs.g_scale)
            torch.cuda.synchronize()
        check_wgrad(cs, r, grad.cpu(), f"fast_conv1_ring_wgrad[{label}]")


@gpu
def test_launcher_contract(hip_lib):
    """Return codes, and nothing written on refusal: -22 for every non-positive / negative argument class, 0 for a
    shape that is not specialised and for M > 10 in the forward and the weight gradients, -2 for E * Ho*Wo % 16 != 0,
    -33 for a ring that is too short, -34 for T * E / 24 + 3 > 1024 (arguments alone: nothing is launched)."""
    _lib = _L()
    lib = _lib.lib()
    buf = torch.full((4096,), SENT, dtype=torch.float32, device=DEV)
    z = buf.data_ptr()
    st = _lib.stream()
    C1g, C3g = (160, 120, 4, 8, 8, 4), (18, 13, 8, 3, 3, 1)

    def fwd(u8=1, chunk=2064, layer=0, L=1, M=10, geo=C1g, Pn=4, E=16, T=1, t0=0, br=4096, boff=0):
        return lib.fast_conv_fwd(z, u8, z, z, z, z, boff, chunk, z, z, layer, L, M, *geo, Pn, E, T, t0, br, 1.0, 1.0, z,
                                 z, st)

    def wg(fn="fast_conv_wgrad", u8=1, chunk=2064, layer=0, L=1, M=10, geo=C1g, Pn=4, E=16, T=1, br=4096, woff=0,
           boff=0):
        return getattr(lib, fn)(z, u8, z, z, z, woff, boff, chunk, z, z, layer, L, M, *geo, Pn, E, T, br, 1.0, 1.0, st)

    def dg(chunk=584, layer=0, L=1, M=10, geo=C3g, Pn=4, E=16, T=1, br=4096, woff=0):
        return lib.fast_conv_dgrad(z, z, z, woff, chunk, z, z, layer, L, M, *geo, Pn, E, T, br, 1.0, z, st)

    def dgb(gb=0, db=0, chunk=584, layer=0, L=1, M=10, geo=C3g, Pn=4, E=16, T=1, br=4096, woff=0):
        return lib.fast_conv_dgrad_bf16(z, gb, z, z, woff, chunk, z, z, layer, L, M, *geo, Pn, E, T, br, 1.0, z, db, st)

    def rf(chunk=2064, layer=0, L=1, M=10, Pn=4, E=16, T=1, t0=0, ns=8, br=4096, boff=0):
        return lib.fast_conv1_ring_fwd(z, z, z, z, z, z, boff, chunk, z, z, layer, L, M, Pn, E, T, t0, ns, br, 1.0, 1.0,
                                       z, z, st)

    def rw(chunk=2064, layer=0, L=1, M=10, Pn=4, E=16, T=1, ns=8, br=4096, woff=0, boff=0):
        return lib.fast_conv1_ring_wgrad(z, z, z, z, z, woff, boff, chunk, z, z, layer, L, M, Pn, E, T, ns, br, 1.0,
                                         1.0, st)

    bad_geo = [tuple(0 if i == j else v for i, v in enumerate(C1g)) for j in range(6)]
    common = [dict(chunk=0), dict(L=0), dict(M=0), dict(Pn=0), dict(E=0), dict(T=0), dict(br=0), dict(layer=-1),
              dict(chunk=-5), dict(E=-16)]
    for kw in common + [dict(geo=g) for g in bad_geo] + [dict(u8=-1), dict(boff=-1), dict(t0=-1)]:
        assert fwd(**kw) == -22, ("fast_conv_fwd", kw)
    for fn in ("fast_conv_wgrad", "fast_conv_wgrad_bf16g"):
        for kw in common + [dict(geo=g) for g in bad_geo] + [dict(u8=-1), dict(boff=-1), dict(woff=-1)]:
            assert wg(fn, **kw) == -22, (fn, kw)
    bad3 = [tuple(0 if i == j else v for i, v in enumerate(C3g)) for j in range(6)]
    for kw in common + [dict(geo=g) for g in bad3] + [dict(woff=-1)]:
        assert dg(**kw) == -22, ("fast_conv_dgrad", kw)
        assert dgb(**kw) == -22, ("fast_conv_dgrad_bf16", kw)
    assert dgb(gb=-1) == -22 and dgb(db=-1) == -22
    for kw in common + [dict(ns=0), dict(boff=-1), dict(t0=-1), dict(M=11)]:
        assert rf(**kw) == -22, ("fast_conv1_ring_fwd", kw)
    for kw in common + [dict(ns=0), dict(boff=-1), dict(woff=-1), dict(M=11)]:
        assert rw(**kw) == -22, ("fast_conv1_ring_wgrad", kw)
    # not specialised: another geometry, a uint8 flag that does not fit the shape, more modules than the kernels hold
    other = (36, 28, 4, 4, 4, 2)
    assert fwd(geo=other) == 0 and wg(geo=other) == 0 and wg("fast_conv_wgrad_bf16g", geo=other) == 0
    assert dg(geo=other) == 0 and dgb(geo=other) == 0 and dg(geo=C1g) == 0
    assert fwd(u8=0) == 0 and wg(u8=0) == 0 and fwd(u8=1, geo=C3g) == 0
    assert fwd(M=11) == 0 and wg(M=11) == 0 and wg("fast_conv_wgrad_bf16g", M=11) == 0 and dgb(M=11) == 0
    assert wg("fast_conv_wgrad_bf16g", u8=0, geo=C3g) == 0                 # C3 has no slab kernel
    with settings(fast_conv_set_slab=0):
        assert wg("fast_conv_wgrad_bf16g") == 0
    with settings(fast_conv_set_dgrad_mfma=0):
        assert dgb() == 0
    # E * Ho*Wo % 16: 8 * 1131 and 4 * 234
    assert fwd(E=8) == -2 and fwd(u8=0, geo=(39, 29, 8, 4, 4, 2), E=4) == -2 and rf(E=8) == -2
    # the ring: nslots >= t0 + T + 3, and the first-channel table of the weight gradient
    assert rf(T=2, t0=1, ns=5) == -33 and rf(T=5, ns=7) == -33 and rw(T=6, ns=8) == -33
    assert rw(E=16, T=1533, ns=1536) == -34 and rw(E=24, T=1022, ns=1025) == -34          # 24528 / 24 + 3 = 1025
    torch.cuda.synchronize()
    assert bool((buf == SENT).all()), "a refused launch wrote to its buffers"
