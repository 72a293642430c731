"""csrc/conv_fast.hip on any machine: what tests/test_conv_fast_kernels.py relies on, checked without a GPU.

* the launcher and setter names of that file are the ``fast_conv*`` entries of ops/_lib.py, each is reached by name in
  a test, and the setter defaults are the ones written in csrc/conv_fast.hip;
* the shapes reach the workgroup tails they claim;
* EXACT cases: every operand lies on its dyadic grid and, for every output element, the sum of the absolute terms stays
  under 2^24 units -- so every product and every partial sum in any order is exact in fp32 -- and a plain torch fp32
  evaluation of the kernels' formulas then equals the float64 reference bit for bit;
* RANDOM cases: that fp32 emulation sits inside every derived bound at every shape of the GPU file, and the share of
  ReLU decisions inside the slot bound is under 1 % for the seeds in use;
* negative controls, through the same checks: a shifted im2col, one dropped tap on one output column, the hcorr of one
  module zeroed, the bit bytes of rows r and r + 1 swapped, one module's weights off by 2 % -- each falls outside the
  bound, and breaks equality in the exact cases.  The scale applied before instead of after the bf16 rounding of G at
  g_scale = 1/M is separated by the weight-gradient bound where rows x users x 2^-23 < 2^-9 (the small shapes) and
  not at the largest one; the exact cases cannot see it (a power-of-two scale commutes with the rounding):
  test_scale_before_rounding_against_the_wgrad_bound.
"""
import math
import os
import re

import pytest
import torch

from pathnet_gym_amd.ops import _lib
import test_conv_fast_kernels as tk
from test_conv_fast_kernels import (C1_CASES, C2_CASES, C3_CASES, KINDS, M16_CASE, P, PAD, RING_CASES, SENT, case_id,
                                    check_dgrad, check_forward, check_wgrad, dgrad_reference, fwd_reference, make_case,
                                    pack_planes, wgrad_reference)
from test_trunk_geometry import BITS_SENT8, EPS, col2im, path_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_CASES = C1_CASES + C2_CASES + C3_CASES + [M16_CASE]
F32 = torch.float32


# ---------------------------------------------------------------------------------------------------------------
# names, defaults, shapes
# ---------------------------------------------------------------------------------------------------------------
def test_every_launcher_and_setter_is_reached_by_name():
    names = {n for n in _lib._SIGS if n.startswith("fast_conv") and not n.startswith("fast_conv_set_x3_")}
    assert names == set(tk.LAUNCHERS) | set(tk.SETTERS)
    src = open(os.path.join(ROOT, "tests", "test_conv_fast_kernels.py")).read()
    body = src[src.index("# GPU\n"):]
    for n in tk.LAUNCHERS:
        assert f'"{n}"' in body[:body.index("def test_launcher_contract")], n          # run through launch() ...
        assert f"lib.{n}(" in body or f'"{n}"' in body[body.index("def test_launcher_contract"):], n   # ... and refused
    for n in tk.SETTERS:
        assert re.search(rf'"{n}": \d|{n}=\d', body), n
    hip = open(os.path.join(ROOT, "csrc", "conv_fast.hip")).read()
    ext = hip[hip.index('extern "C" {'):]
    assert set(re.findall(r"^(?:int|void) (fast_conv\w+)\(", ext, re.M)) == names
    for n, default in tk.SETTERS.items():
        var = re.search(rf"void {n}\(int \w+\) {{ (\w+) = \w+; }}", hip).group(1)
        assert int(re.search(rf"static int {var} = (\d+);", hip).group(1)) == default, n


def test_shapes_reach_the_tails_they_claim():
    ly1, ly2, ly3 = (tk.make_layer(n, 10, 1.0, 1.0)[0] for n in ("C1", "C2", "C3"))
    assert (ly1.HWo, ly1.K, ly2.HWo, ly2.K, ly3.HWo, ly3.K) == (1131, 256, 234, 128, 176, 72)
    assert [T * 16 * 1131 % 1024 for T in (1, 2, 3)] == [688, 352, 16]        # NT 8: 1024-row workgroups
    assert 688 % 32 == 16 and 352 % 32 == 0 and 16 % 32 == 16                 # a 32-row tile with one 16-row half
    assert {c[2] for c in C1_CASES} == {1, 2, 3} and any(c[4] == 1 for c in C1_CASES)
    assert 1 * 176 < 256 and {c[1] for c in C3_CASES} >= {1, 3, 5, 16}        # NT 2: a workgroup larger than the path
    for name, E, T, M, t0, cnts in ALL_CASES:
        assert (E * {"C1": 1131, "C2": 234, "C3": 176}[name]) % 16 == 0
    cnts = set()
    for spec in ALL_CASES:
        cnts |= {len(a) for a in make_case(spec, "exact").acts}
    assert {0, 1, 2, 3, 4, 5, 6, 7, 10, 16} <= cnts                           # column tiles 1..5, DG slot groups 1..3
    for spec in RING_CASES:
        cs = make_case(spec, "exact", ring=True)
        assert cs.nslots > cs.t0 + cs.T + 3 and set(cs.fc.unique().tolist()) == {0, 1, 2, 3}
        assert bool((cs.fc[-2] != cs.fc[-1]).any())


# ---------------------------------------------------------------------------------------------------------------
# the kernels' formulas in plain torch fp32 (any summation order)
# ---------------------------------------------------------------------------------------------------------------
def operands(cs, f16):
    Wop = (cs.W.to(torch.float16) if f16 else cs.W.to(torch.bfloat16)).float()
    return Wop, Wop.sum(1).reshape(-1)                  # hcorr: fp32 column sums


def emulate_forward(cs, f16, fault=None):
    ly, T, E, B, t0 = cs.ly, cs.T, cs.E, cs.B, cs.t0
    Wop, hc = operands(cs, f16)
    j0 = cs.M - 1                                       # the last module: on paths 1 and 2
    Wk = Wop.clone()
    hk = hc.clone().reshape(cs.M, 8)
    if fault == "tap":
        Wk[j0, 5 * ly.Cin:6 * ly.Cin, 3] = 0            # tap (kh 0, kw 5 % KW ...) of output map 3
    if fault == "w2":
        Wk[j0] = Wk[j0] * 1.02
    if fault == "hcorr":
        hk[j0] = 0
    i_s = torch.tensor(cs.in_scale, dtype=F32)
    x = cs.x[t0:t0 + T]
    Y = torch.full((cs.steps * B + PAD, ly.out_feat), SENT, dtype=torch.bfloat16)
    bits = []
    for p in range(P):
        A = path_rows(x, ly, p, shifted=fault == "shifted").float()
        if f16:
            A = A + 1024.0
        tot = torch.zeros(A.shape[0], 8)
        bp = []
        for j in cs.acts[p]:
            bb = cs.b[j] - (1024.0 * i_s) * hk[j] if f16 else cs.b[j]
            v = (A @ Wk[j]) * i_s + bb
            bp.append(v > 0)
            tot = tot + torch.relu(v)
        bits.append(torch.stack(bp) if bp else torch.zeros(0, A.shape[0], 8, dtype=torch.bool))
        yp = (tot * torch.tensor(cs.out_scale, dtype=F32)).to(torch.bfloat16)
        Y[t0 * B:(t0 + T) * B].view(T, P, E, -1)[:, p] = yp.reshape(T, E, -1)
    planes = pack_planes(cs, bits, t0, cs.steps)
    if fault == "swap":
        r0 = t0 * B * ly.HWo + E * ly.HWo               # path 1, slot 0, its first 64 rows
        sw = planes[0, r0:r0 + 64].clone().reshape(32, 2).flip(1).reshape(64)
        planes[0, r0:r0 + 64] = sw
    return Y, planes


def emulate_wgrad(cs, g_bf16=False, scale_before=False):
    ly, T, K = cs.ly, cs.T, cs.ly.K
    G = cs.G.to(torch.bfloat16).float() if g_bf16 else cs.G
    i_s, g_s = torch.tensor(cs.in_scale, dtype=F32), torch.tensor(cs.g_scale, dtype=F32)
    grad = torch.zeros(cs.numel + 8 * PAD)
    grad[cs.numel:] = SENT
    seg = grad[tk.LEAD:tk.LEAD + cs.M * cs.chunk].view(cs.M, cs.chunk)
    for p in range(P):
        if not cs.acts[p]:
            continue
        A = path_rows(cs.x[:T], ly, p).float()
        gp = G[:, p].reshape(A.shape[0], 8)
        for a, j in enumerate(cs.acts[p]):
            gm = torch.where(cs.bits[p][a], gp, torch.zeros_like(gp))
            if scale_before:
                dW = (A.t() @ (gm * g_s).to(torch.bfloat16).float()) * i_s
            else:
                dW = (A.t() @ gm.to(torch.bfloat16).float()) * (i_s * g_s)
            seg[j, :K * 8] += dW.reshape(-1)
            seg[j, K * 8:K * 8 + 8] += gm.sum(0) * g_s
    return grad


def emulate_dgrad(cs, mfma, g_bf16=False, dx_bf16=False, g_scale=None, fault=None):
    ly, T, E, B = cs.ly, cs.T, cs.E, cs.B
    g_s = torch.tensor(cs.g_scale if g_scale is None else g_scale, dtype=F32)
    G = cs.G.to(torch.bfloat16).float() if g_bf16 else cs.G
    W = (cs.W.to(torch.bfloat16).float() if mfma else cs.W).clone()
    if fault == "w2":
        W[cs.M - 1] = W[cs.M - 1] * 1.02
    if fault == "tap":
        W[cs.M - 1, 2 * ly.Cin:3 * ly.Cin, 3] = 0
    dX = torch.full((T * B + PAD, ly.in_feat), SENT, dtype=torch.bfloat16 if dx_bf16 else F32)
    R = T * E * ly.HWo
    for p in range(P):
        dcol = torch.zeros(R, ly.K)
        gp = (G[:, p] * g_s).reshape(R, 8)
        for a, j in enumerate(cs.acts[p]):
            gm = torch.where(cs.bits[p][a], gp, torch.zeros_like(gp))
            if mfma:
                gm = gm.to(torch.bfloat16).float()
            dcol = dcol + gm @ W[j].t()
        d = col2im(dcol.reshape(T * E, ly.HWo, ly.K), ly).reshape(T, E, ly.in_feat)
        dX[:T * B].view(T, P, E, -1)[:, p] = d.to(dX.dtype)
    return dX


def host_fwd_ref(cs, f16):
    Wop, hc = operands(cs, f16)
    return fwd_reference(cs, Wop.double(), hc) if f16 else fwd_reference(cs, Wop.double())


# ---------------------------------------------------------------------------------------------------------------
# exactness proofs
# ---------------------------------------------------------------------------------------------------------------
def on_grid(t, unit):
    v = t.double() / unit
    return bool((v == v.round()).all())


def pow2(v):
    return math.frexp(v)[0] == 0.5


def prove_exact(cs):
    """Every operand on its grid; per output element sum |terms| / unit < 2^24, so any order of fp32 sums is exact."""
    ly, LIM = cs.ly, 2.0 ** 24
    ux, uw, ub = (1.0 if cs.u8 else 2.0 ** -3), 2.0 ** -4, 2.0 ** -3
    assert on_grid(cs.W, uw) and float(cs.W.abs().max()) <= 0.25 and on_grid(cs.b, ub)
    assert on_grid(cs.x, ux) and on_grid(cs.G, 1.0) and float(cs.G.abs().max()) <= 1.0
    assert pow2(cs.in_scale) and pow2(cs.out_scale) and pow2(cs.g_scale)
    # the dyadic weights survive both operand casts, and fp16(1024 + pixel) is exact
    assert torch.equal(cs.W.to(torch.bfloat16).float(), cs.W) and torch.equal(cs.W.to(torch.float16).float(), cs.W)
    worst = {}
    for f16 in ((True, False) if cs.u8 else (False,)):
        y, yb, pres, bnds = host_fwd_ref(cs, f16)                 # exact cases: no bias slack in the bound
        corr = 1024.0 * cs.in_scale * operands(cs, f16)[1].double().reshape(cs.M, 8).abs() if f16 else \
            torch.zeros(cs.M, 8, dtype=torch.float64)
        uv = min(cs.in_scale * ux * uw, ub, (1024.0 * cs.in_scale * uw) if f16 else ub)
        for p in range(P):
            if not cs.acts[p]:
                continue
            S = (bnds[p] - EPS * pres[p].abs()) / (ly.K * EPS * cs.in_scale)     # (offset + |x|) @ |W|
            assert float(S.max()) / (ux * uw) < LIM
            for a, j in enumerate(cs.acts[p]):                                   # v = acc * in_scale + b'
                assert float((cs.in_scale * S[a] + cs.b[j].double().abs() + corr[j]).max()) / uv < LIM
            assert int((pres[p] == 0).sum()) >= ly.HWo                           # the zero sample: v > 0 at pre == 0
            tot = pres[p].abs().sum(0)                                           # the sum over the slots
            assert float(tot.max()) / uv < LIM
            worst["fwd"] = max(worst.get("fwd", 0.0), float(S.max()) / (ux * uw), float(tot.max()) / uv)
    r = wgrad_reference(cs)
    n_w = (cs.T * cs.E * ly.HWo * r["users"]).clamp_min(1.0)[:, None, None]
    Sw = r["bW"] / (n_w * EPS * cs.in_scale * cs.g_scale)
    Sb = r["bb"] / (n_w[:, 0] * EPS * cs.g_scale)
    assert float(Sw.max()) / ux < LIM and float(Sb.max()) < LIM
    worst["wgrad"] = float(Sw.max()) / ux
    if not cs.u8:
        _, bX = dgrad_reference(cs, False)
        for p in range(P):
            if cs.acts[p]:
                n = len(cs.acts[p]) * -(-ly.KH // ly.S) * -(-ly.KW // ly.S) * 8
                assert float(bX[:, p].max()) / (n * EPS) / (cs.g_scale * uw) < LIM
    return worst


# ---------------------------------------------------------------------------------------------------------------
# the emulation against every check of the GPU file, at every shape of the GPU file
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("spec", ALL_CASES, ids=case_id)
def test_emulation_passes_every_check(spec, kind):
    """EXACT: the proof, then bit equality of the fp32 emulation.  RANDOM: the emulation inside every bound, and the
    ReLU decisions left out by the slot bound under 1 % (asserted inside check_forward) for the seeds in use."""
    cs = make_case(spec, kind)
    if cs.exact:
        print("units of the largest sum:", prove_exact(cs))
    if cs.M <= 10:
        for f16 in ((True, False) if cs.u8 else (False,)):
            Y, planes = emulate_forward(cs, f16)
            left, total = check_forward(cs, host_fwd_ref(cs, f16), Y, planes, f"emu fwd {'f16' if f16 else 'bf16'}",
                                        rec=False)
            if not cs.exact:
                print(f"ReLU decisions left out: {100.0 * left / max(total, 1):.3f} %")
        if cs.t0 == 0:
            check_wgrad(cs, wgrad_reference(cs), emulate_wgrad(cs), "emu wgrad", rec=False)
            if cs.name != "C3":
                check_wgrad(cs, wgrad_reference(cs, True), emulate_wgrad(cs, True), "emu wgrad bf16g", rec=False)
    if not cs.u8 and cs.t0 == 0:
        check_dgrad(cs, dgrad_reference(cs, False), emulate_dgrad(cs, False), "emu dgrad valu", rec=False)
        if cs.M <= 10:
            for gb, db, gs in ((False, False, None), (True, False, None), (False, True, None), (True, True, None),
                               (True, True, 1.0)):
                check_dgrad(cs, dgrad_reference(cs, True, gb, db, gs), emulate_dgrad(cs, True, gb, db, gs),
                            f"emu dgrad mfma g_bf16={gb} dx_bf16={db} gs={gs}", rec=False)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("spec", RING_CASES, ids=case_id)
def test_ring_stacks_follow_the_kernel_rule(spec, kind):
    """The stacks of the ring cases: channel c of sample (t, b) is frame slot t + max(c, fc[t][b]) -- spelled out
    element by element on a few samples -- and the channel-major permutation inverts."""
    cs = make_case(spec, kind, ring=True)
    x = cs.x.reshape(cs.steps, cs.B, 160 * 120, 4)
    for t in range(cs.steps):
        for b in (0, 1, 2, 3, cs.B - 1):
            for c in range(4):
                assert torch.equal(x[t, b, :, c], cs.frames[b, t + max(c, int(cs.fc[t, b]))])
    W = cs.W
    assert torch.equal(tk.from_cmajor(tk.cmajor(W)), W)
    kh, kw, ci, c, j = 3, 5, 2, 6, 1
    assert tk.cmajor(W)[j, c, (ci * 8 + kh) * 8 + kw] == W[j, (kh * 8 + kw) * 4 + ci, c]
    Y, planes = emulate_forward(cs, True)
    check_forward(cs, host_fwd_ref(cs, True), Y, planes, "emu ring fwd", rec=False)


# ---------------------------------------------------------------------------------------------------------------
# negative controls
# ---------------------------------------------------------------------------------------------------------------
CONTROL_SPECS = [C1_CASES[0], C2_CASES[0], C3_CASES[2]]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fault", ["shifted", "tap", "hcorr", "swap", "w2"])
@pytest.mark.parametrize("spec", CONTROL_SPECS, ids=case_id)
def test_forward_faults_fall_outside(spec, fault, kind):
    cs = make_case(spec, kind)
    for f16 in ((True, False) if cs.u8 else (False,)):
        if fault == "hcorr" and not f16:
            continue
        Y, planes = emulate_forward(cs, f16, fault)
        with pytest.raises(AssertionError):
            check_forward(cs, host_fwd_ref(cs, f16), Y, planes, f"control {fault}", rec=False)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fault", ["tap", "w2"])
@pytest.mark.parametrize("spec", CONTROL_SPECS[1:], ids=case_id)
def test_dgrad_faults_fall_outside(spec, fault, kind):
    cs = make_case(spec, kind)
    for mfma in (False, True):
        with pytest.raises(AssertionError):
            check_dgrad(cs, dgrad_reference(cs, mfma), emulate_dgrad(cs, mfma, fault=fault), f"control {fault}",
                        rec=False)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("spec", CONTROL_SPECS, ids=case_id)
def test_wgrad_faults_fall_outside(spec, kind):
    """One ReLU byte of one row taken from the row after it, and a gradient row dropped: outside the bound."""
    cs = make_case(spec, kind)
    good = emulate_wgrad(cs)
    keep = [b.clone() for b in cs.bits]
    try:
        cs.bits[1][0, :-1] = keep[1][0, 1:]                  # path 1, slot 0: every row reads the next row's byte
        bad = emulate_wgrad(cs)
    finally:
        for p in range(P):
            cs.bits[p] = keep[p]
    assert not torch.equal(good, bad)
    with pytest.raises(AssertionError):
        check_wgrad(cs, wgrad_reference(cs), bad, "control shifted bits", rec=False)
    leak = good.clone()
    leak[tk.LEAD + cs.ly.K * 8 + 8] = 2.0 ** -20             # one word between two modules
    with pytest.raises(AssertionError):
        check_wgrad(cs, wgrad_reference(cs), leak, "control gap", rec=False)


def test_scale_before_rounding_against_the_wgrad_bound():
    """g_scale = 1/M applied before the bf16 rounding of G (what the runtime-geometry kernel does) instead of after
    the sum.  Each term then carries another rounding of 2^-9 relative; the bound is n 2^-23 |A|^T |G| with
    n = rows x users.  Result: at C2, E = 8, T = 1 (n = 1872 per user, n 2^-23 = 2^-12.1 < 2^-9) the bound separates
    the two -- scale-before falls outside (worst ratio 1.7 here) -- while at C1, E = 16, T = 3 (n = 54288 per user,
    n 2^-23 = 2^-7.3 > 2^-9) it cannot, and does not.  The exact cases cannot see it at any shape: a power-of-two
    scale commutes with the rounding."""
    cs = make_case(C2_CASES[0], "random")
    after, before = emulate_wgrad(cs), emulate_wgrad(cs, scale_before=True)
    r = wgrad_reference(cs)
    check_wgrad(cs, r, after, "scale after", rec=False)
    with pytest.raises(AssertionError, match="outside the derived bound"):
        check_wgrad(cs, r, before, "scale before", rec=False)
    assert cs.T * cs.E * cs.ly.HWo * EPS < 2.0 ** -9
    big = make_case(C1_CASES[2], "random")
    assert big.T * big.E * big.ly.HWo * EPS > 2.0 ** -9
    check_wgrad(big, wgrad_reference(big), emulate_wgrad(big, scale_before=True), "scale before, C1 T=3", rec=False)
    ex = make_case(C2_CASES[0], "exact")
    assert torch.equal(emulate_wgrad(ex), emulate_wgrad(ex, scale_before=True))
