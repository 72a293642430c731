"""csrc/heads.hip, launcher by launcher, against plain float64 torch with buffers of the test's own.

The kernels are called through ``ops/_lib.call`` on a synthetic ``flat`` buffer (no model): the policy / value
weights and biases sit at odd offsets and everything between them is NaN.  The float64 reference is fed ``x`` as the
kernel reads it (bf16 widened, or fp32) and the fp32 weights widened, so all that separates a kernel output from
float64 is the fp32 arithmetic, and its tolerance is derived, not measured:

    forward    |hip - ref64| <= (F + 2) 2^-23 (|x| @ |W| + |b|)                    F products, F adds
    dfeat      |hip - ref64| <= (A + 3) 2^-23 (|dz| @ |Wp|^T + |dv| |wv|)
    dW, db     |g   - ref64| <= (N + 8) 2^-23 (|x|^T @ |dz|)      (biases: sum |dz|)

(2^-23 and not 2^-24: the bounds then hold for any summation order, with or without fused multiply-adds).  The head
gradients are ACCUMULATED: grad = fl(grad0 + g).  From grad0 = 0 the bound on g is asserted as it stands.  From a
random non-zero grad0 even an exact g leaves fl(grad0 + g) one fp32 rounding of |grad0 + g| away from grad0 + g, so
each add into the entry (one for the partials + ordered reduction of ``_det`` / the 32-row split, one per 128-row
chunk for the atomic kernels) contributes 2^-24 (|grad0| + |x|^T |dz|) on top, as in test_lstm_kernels.py.

Sampling is Gumbel-max on a counter-based hash: action = argmax_j lg_j - log(-log u_j).  The uniforms are integer
arithmetic, shared bit for bit with ``a2c_math.sampling_u01``; what differs from any other evaluation is ``__logf``.
The kernel's action must equal the float64 argmax (fed the kernel's own fp32 logits) on every row whose float64
top-two gap is at least g_tol = 8 e32, e32 = the max abs error of a torch fp32 evaluation of the same scores; at most
0.2 % of the rows may sit below g_tol at all.  The distribution of the draws is tested against softmax(logits) with
the 5-sigma binomial bound of test_ga_modes.py, on the kernel and on the torch mirror.

Every output buffer carries 64 extra rows of a sentinel that must survive; every input carries 64 extra rows of NaN.
Measured figures are recorded under ``heads_kernels_f64`` in tests/data/numerics_measured.json
(``PATHNET_RECORD_NUMERICS``).
"""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import numerics_budget as budget
from pathnet_gym_amd.algo.a2c_math import hash_to_u01, sample_actions_keyed, sampling_u01
from pathnet_gym_amd.envs.base import wang_hash

gpu = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -23
PAD = 64                           # sentinel rows after every buffer
SENT = -3.0                        # exact in bf16, fp32 and int32
NAN = float("nan")
M32 = 0xFFFFFFFF
BATCHES = [1, 15, 16, 17, 63, 64, 65, 130]          # the 16-sample and 64-sample workgroup edges, 4 samples per wave
SAMPLER_N = 16384
SAMPLER_A = [2, 6, 18, 32]
SAMPLER_KEYS = [(99, 0), (12345, 4096)]             # (seed, row_base)
CTR, T_ROLL = 3, 5                                  # stepkey = ctr * T + t


# ---------------------------------------------------------------------------------------------------------------
# float64 references and bounds (CPU tensors; also run by the CPU tests below)
# ---------------------------------------------------------------------------------------------------------------
def make_heads(A, F, seed, wscale=0.1, zero_w=False, bias=None):
    """A synthetic ``flat`` (CPU fp32): policy weight [F, A], policy bias [A], value weight [F], value bias at odd
    offsets, NaN everywhere else.  For A >= 2 two policy biases are equal and above all others (the planted tie)."""
    g = torch.Generator().manual_seed(seed)
    pw = 37
    pb = (pw + F * A + 11) | 1
    vw = (pb + A + 7) | 1
    vb = (vw + F + 5) | 1
    flat = torch.full((vb + 1 + 29,), NAN)
    Wp = torch.randn(F, A, generator=g) * wscale
    wv = torch.randn(F, generator=g) * wscale
    bp = (torch.randn(A, generator=g) * 0.3).clamp(-0.7, 0.7)
    tie = None
    if A >= 2:
        tie = (A // 3, A - 1)
        bp[tie[0]] = bp[tie[1]] = 0.75
    if zero_w:
        Wp, wv = torch.zeros(F, A), torch.zeros(F)
    if bias is not None:
        bp, tie = bias.float().clone(), None
    flat[pw:pw + F * A] = Wp.reshape(-1)
    flat[pb:pb + A] = bp
    flat[vw:vw + F] = wv
    flat[vb] = torch.randn(1, generator=g).item()
    return dict(A=A, F=F, pw=pw, pb=pb, vw=vw, vb=vb, flat=flat, tie=tie, Wp=flat[pw:pw + F * A].view(F, A),
                bp=flat[pb:pb + A], wv=flat[vw:vw + F], bv=flat[vb:vb + 1])


def make_feat(B, F, seed, f32, scale=0.5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, F, generator=g) * scale
    return x if f32 else x.to(torch.bfloat16)


def ref_forward(hd, x):
    """float64 logits [B, A] and value [B] of features ``x`` (bf16 or fp32, as the kernel reads them) and their
    elementwise bounds."""
    F = hd["F"]
    x64, Wp, wv = x.double(), hd["Wp"].double(), hd["wv"].double()
    bp, bv = hd["bp"].double(), hd["bv"].double()
    return dict(logits=x64 @ Wp + bp, value=x64 @ wv + bv,
                logits_bound=(F + 2) * EPS * (x64.abs() @ Wp.abs() + bp.abs()),
                value_bound=(F + 2) * EPS * (x64.abs() @ wv.abs() + bv.abs()))


def ref_backward(hd, x, dz, dv):
    """float64 head gradients of N rows (x as the kernel reads it, dz [N, A] / dv [N] fp32) and their bounds."""
    A, N = hd["A"], x.shape[0]
    x64, dz64, dv64 = x.double(), dz.double(), dv.double()
    Wp, wv = hd["Wp"].double(), hd["wv"].double()
    nb = (N + 8) * EPS
    return dict(dfeat=dz64 @ Wp.t() + dv64[:, None] * wv[None, :],
                dfeat_bound=(A + 3) * EPS * (dz64.abs() @ Wp.abs().t() + dv64.abs()[:, None] * wv.abs()[None, :]),
                dWp=x64.t() @ dz64, dWp_bound=nb * (x64.abs().t() @ dz64.abs()),
                dwv=x64.t() @ dv64, dwv_bound=nb * (x64.abs().t() @ dv64.abs()),
                dbp=dz64.sum(0), dbp_bound=nb * dz64.abs().sum(0),
                dbv=dv64.sum().reshape(1), dbv_bound=nb * dv64.abs().sum().reshape(1))


def first_argmax(logits):
    """argmax with the FIRST maximum on exact ties (numpy's rule; the kernels scan j upwards with a strict >)."""
    return torch.from_numpy(np.argmax(logits.numpy(), axis=1))


def dispatch(A, F, s16=1):
    """The forward kernel launch_heads_fwd_sample reaches (heads.hip heads_fwd_lanes_launch), mirrored."""
    if F % 32 != 0 or A > 18:
        return "wave"
    if s16 and F % 128 == 0 and A <= 8 and (F * 9 + 16 * 9 * 16) * 4 <= 64 * 1024:
        return "s16<8>"
    if s16 and F % 128 == 0 and (F * 19 + 16 * 19 * 16) * 4 <= 64 * 1024:
        return "s16<18>"
    AM = 8 if A <= 8 else 18
    if (F * (AM + 1) + 3 * (AM + 1) * 64) * 4 > 64 * 1024:
        return "wave"
    return f"lanes<{AM}>"


def gumbel_reference(lg32, seed, stepkey, row_base):
    """float64 Gumbel-max scores of fp32 logits [N, A] on the kernel's key, their argmax and top-two gap, and e32 =
    the max abs error of the fp32 torch evaluation of the same scores.  -> u, ref action, gap, e32."""
    rows = torch.arange(lg32.shape[0], dtype=torch.int64) + int(row_base)
    u = sampling_u01(int(seed), int(stepkey), rows, lg32.shape[1])
    s64 = lg32.double() - torch.log(-torch.log(u.double()))
    s32 = lg32 - torch.log(-torch.log(u))
    e32 = float((s32.double() - s64).abs().max())
    top = s64.topk(2, dim=1)
    return u, top.indices[:, 0], top.values[:, 0] - top.values[:, 1], e32


def check_sampler_agreement(lg32, actions, seed, stepkey, row_base, tag, record=True):
    """The rule of the module docstring.  Prints the figures before it asserts; -> dict of them."""
    _, ref, gap, e32 = gumbel_reference(lg32.cpu().float(), seed, stepkey, row_base)
    g_tol = 8.0 * e32
    near = gap < g_tol
    dis = actions.cpu().long() != ref
    worst = float(gap[dis].max()) if bool(dis.any()) else 0.0
    out = dict(e32=e32, g_tol=g_tol, near_frac=float(near.double().mean()), disagree=int(dis.sum()),
               worst_gap=worst, worst_gap_over_e32=worst / e32, rows_below_1e3=float((gap < 1e-3).double().mean()))
    print(f"{tag}: " + ", ".join(f"{k} = {v:.4g}" for k, v in out.items()))
    if record:
        record_measured({"sampler.worst_disagreeing_gap": worst, "sampler.worst_disagreeing_gap_over_e32": worst / e32})
    assert 0 < e32 < 1e-5, (tag, e32)
    assert out["near_frac"] <= 0.002, (tag, out)
    assert not bool((dis & ~near).any()), (tag, out)
    return out


def cell_z(counts, p, n):
    """z of every cell with n p >= 25 and of the pooled rest, (count - n p) / sqrt(n p (1 - p))."""
    counts, p = counts.double(), p.double()
    big = n * p >= 25
    c, q = counts[big], p[big]
    if bool((~big).any()):
        c, q = torch.cat([c, counts[~big].sum()[None]]), torch.cat([q, p[~big].sum()[None]])
    return (c - n * q) / torch.sqrt(n * q * (1 - q))


def dist_logits(A, scale):
    return torch.randn(A, generator=torch.Generator().manual_seed(7 * A + 1)) * scale


def wang(x):
    x &= M32
    x = (x ^ 61) ^ (x >> 16)
    x = (x * 9) & M32
    x ^= x >> 4
    x = (x * 0x27D4EB2D) & M32
    return x ^ (x >> 15)


def wang_inv(y):
    """The hash is a bijection: two invertible xorshifts, two odd multipliers and (x ^ 61) ^ (x >> 16), whose upper
    half is x's own."""
    y &= M32
    y ^= y >> 15
    y ^= y >> 30
    y = (y * pow(0x27D4EB2D, -1, 1 << 32)) & M32
    y ^= y >> 4
    y ^= y >> 8
    y ^= y >> 16
    y = (y * pow(9, -1, 1 << 32)) & M32
    return y ^ 61 ^ (y >> 16)


U1 = dict(stepkey=17, row=37, j0=4, A=6)


def u1_seed():
    """The seed for which the draw of (stepkey 17, row 37, action 4) hashes to 0xFFFFFF00: k = 2^24 - 1."""
    return wang_inv(0xFFFFFF00) ^ wang(wang(U1["stepkey"] * 64 + U1["j0"]) ^ U1["row"])


def u1_logits():
    lg = torch.zeros(U1["A"])
    lg[U1["j0"]] = -30.0
    return lg


def record_measured(vals):
    """PATHNET_RECORD_NUMERICS=<file>: keep the max per key under heads_kernels_f64."""
    rec = os.environ.get("PATHNET_RECORD_NUMERICS")
    if not rec:
        return
    d = budget._load(rec)
    t = d.setdefault("heads_kernels_f64", {})
    for k, v in vals.items():
        t[k] = max(float(v), float(t.get(k, 0.0)))
    os.makedirs(os.path.dirname(rec) or ".", exist_ok=True)
    with open(rec, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def within(name, got, ref, bound):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    err = (got - ref).abs()
    ok = err <= bound
    ratio = float((err / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0
    print(f"{name}: worst err / bound = {ratio:.4f}")
    record_measured({name: ratio})
    assert bool(ok.all()), (name, ratio, int((~ok).sum()), err.numel())


# ---------------------------------------------------------------------------------------------------------------
# CPU: the references, the bounds, the mirror's distribution and the u < 1 draw, checked on any machine
# ---------------------------------------------------------------------------------------------------------------
def test_reference_and_bounds_cpu():
    for A, F, N, f32 in ((6, 256, 213, False), (18, 96, 33, True), (32, 320, 129, False), (1, 32, 1, True)):
        hd = make_heads(A, F, seed=A + F)
        x = make_feat(N, F, seed=N, f32=f32)
        g = torch.Generator().manual_seed(3 + N)
        dz, dv = torch.randn(N, A, generator=g) * 0.1, torch.randn(N, generator=g) * 0.1
        fw, bw = ref_forward(hd, x), ref_backward(hd, x, dz, dv)
        # the closed forms are the float64 autograd of the heads
        leaves = [t.double().clone().requires_grad_(True) for t in (x, hd["Wp"], hd["bp"], hd["wv"], hd["bv"])]
        x64, Wp, bp, wv, bv = leaves
        lg, v = x64 @ Wp + bp, x64 @ wv + bv
        assert torch.equal(lg.detach(), fw["logits"]) and torch.equal(v.detach(), fw["value"])
        ((lg * dz.double()).sum() + (v * dv.double()).sum()).backward()
        for got, name in zip(leaves, ("dfeat", "dWp", "dbp", "dwv", "dbv")):
            assert torch.allclose(got.grad, bw[name], rtol=0, atol=1e-12), name
        # the derived bounds hold, with room, for an fp32 torch evaluation of the same operands ...
        xf = x.float()
        for got, name in ((xf @ hd["Wp"] + hd["bp"], "logits"), (xf @ hd["wv"] + hd["bv"], "value")):
            err = (got.double() - fw[name]).abs()
            assert bool((err <= fw[name + "_bound"]).all()) and float((err / fw[name + "_bound"]).max()) < 0.5
        for got, name in ((dz @ hd["Wp"].t() + dv[:, None] * hd["wv"][None, :], "dfeat"), (xf.t() @ dz, "dWp"),
                          (xf.t() @ dv, "dwv"), (dz.sum(0), "dbp"), (dv.sum().reshape(1), "dbv")):
            assert bool(((got.double() - bw[name]).abs() <= bw[name + "_bound"]).all()), name
        assert hd["pw"] % 2 == hd["pb"] % 2 == hd["vw"] % 2 == hd["vb"] % 2 == 1
        if hd["tie"]:
            j1, j2 = hd["tie"]
            z = ref_forward(hd, torch.zeros(1, F))["logits"]
            assert z[0, j1] == z[0, j2] == z.max() and int(first_argmax(z)) == j1 < j2
    # ... and are tight enough to see one policy-weight column off by 2 % (the project's single-module control),
    hd = make_heads(6, 256, seed=1)
    x = make_feat(37, 256, seed=2, f32=False)
    fw = ref_forward(hd, x)
    off = dict(hd, Wp=hd["Wp"].clone())
    off["Wp"][:, 2] *= 1.02
    bad = (ref_forward(off, x)["logits"] - fw["logits"]).abs() > fw["logits_bound"]
    assert bool(bad[:, 2].double().mean() > 0.9) and not bool(bad[:, [0, 1, 3, 4, 5]].any())
    # one row of N = 213 missing from the weight and bias gradients, one action missing from dfeat
    g = torch.Generator().manual_seed(5)
    dz, dv = torch.randn(37, 6, generator=g) * 0.1, torch.randn(37, generator=g) * 0.1
    bw, short = ref_backward(hd, x, dz, dv), ref_backward(hd, x[:-1], dz[:-1], dv[:-1])
    for name in ("dWp", "dwv", "dbp", "dbv"):
        assert float(((short[name] - bw[name]).abs() > bw[name + "_bound"]).double().mean()) > 0.9, name
    dz5 = dz.clone()
    dz5[:, 5] = 0
    off5 = (ref_backward(hd, x, dz5, dv)["dfeat"] - bw["dfeat"]).abs() > bw["dfeat_bound"]
    assert float(off5.double().mean()) > 0.9


def test_dispatch_table_names_every_forward_kernel():
    for label, s16, A, F in FWD_TABLE:
        assert dispatch(A, F, s16) == label, (label, s16, A, F)
    assert {k for k, _, _, _ in FWD_TABLE} == {"s16<8>", "s16<18>", "lanes<8>", "lanes<18>", "wave"}
    assert {dispatch(A, F) for _, A, F in SWEEP_SHAPES} == {"s16<8>", "s16<18>", "lanes<8>", "lanes<18>", "wave"}


def test_wang_inverse_and_u_strictly_inside_unit_interval_cpu():
    for x in (0, 1, 61, 0xFFFFFF00, 0xFFFFFFFF, 0x12345678, 1295160987):
        assert wang(wang_inv(x)) == x and wang_inv(wang(x)) == x
        assert int(wang_hash(torch.tensor([x], dtype=torch.int64))) == wang(x)
    # the formula at the ends of the hash range, and at the first k whose k + 0.5 has no fp32
    u = hash_to_u01(torch.tensor([0, 0xFF, 0xFFFFFF00, 0xFFFFFFFF, 0xFFFFFE00, 1 << 31], dtype=torch.int64))
    assert u.dtype == torch.float32 and bool((u > 0).all()) and bool((u < 1).all())
    assert u[0] == u[1] == 2.0 ** -25 and u[2] == u[3] == 1.0 - 2.0 ** -24 and u[4] == 1.0 - 2.0 ** -23
    assert u[5] == 0.5                                             # k = 2^23: k + 0.5 rounds to even, k
    assert bool(torch.isfinite(-torch.log(-torch.log(u))).all())
    # the crafted key: this draw hashes to k = 2^24 - 1, where fp32(k + 0.5) * 2^-24 == 1 without the clamp
    seed = u1_seed()
    assert seed == 1295160987
    rows = torch.arange(64, dtype=torch.int64)
    uu = sampling_u01(seed, U1["stepkey"], rows, U1["A"])
    assert float(uu[U1["row"], U1["j0"]]) == 1.0 - 2.0 ** -24 and bool((uu > 0).all()) and bool((uu < 1).all())
    # the same draw turns up by itself in the inputs of the agreement test below: seed 12345, row 4096 + 9390, A = 32
    un = sampling_u01(12345, U1["stepkey"], torch.tensor([4096 + 9390]), 32)
    assert float(un[0, 26]) == 1.0 - 2.0 ** -24 and bool((un < 1).all())
    a = sample_actions_keyed(u1_logits()[None].expand(64, -1), seed, U1["stepkey"])
    assert int(a[U1["row"]]) != U1["j0"] and not bool((a == U1["j0"]).any())       # p(j0) ~ e^-30
    # row_base shifts the key: the same draw lands on row 37 - row_base
    a5 = sample_actions_keyed(u1_logits()[None].expand(59, -1), seed, U1["stepkey"], row_base=5)
    assert torch.equal(a5, a[5:])


def test_mirror_sampler_follows_softmax_cpu():
    """a2c_math.sample_actions_keyed on constant logits: every cell within 5 sigma (measured max |z| 3.5), and the
    gap rule is not vacuous on these inputs: no row of the float64 reference lies below 8 e32."""
    worst = 0.0
    for A in SAMPLER_A:
        for scale in (0.0, 1.0, 2.0):
            lg = dist_logits(A, scale)
            p = torch.softmax(lg.double(), 0)
            for seed, rb in SAMPLER_KEYS:
                counts = torch.zeros(A, dtype=torch.int64)
                for stepkey in range(15, 23):
                    a = sample_actions_keyed(lg[None].expand(SAMPLER_N, -1), seed, stepkey, rb)
                    counts += torch.bincount(a, minlength=A)
                z = cell_z(counts, p, 8 * SAMPLER_N)
                worst = max(worst, float(z.abs().max()))
                assert float(z.abs().max()) <= 5.0, (A, scale, seed, rb, z)
    z = contingency_z(lambda stepkey: sample_actions_keyed(torch.zeros(65536, 4), 99, stepkey, 0))
    print(f"mirror: max |z| = {worst:.3f}, contingency max |z| = {float(z.abs().max()):.3f}")
    assert float(z.abs().max()) <= 5.0, z
    g = torch.Generator().manual_seed(11)
    for A in SAMPLER_A:
        lg = torch.randn(SAMPLER_N, A, generator=g) * 2.0
        a = sample_actions_keyed(lg, 99, 17, 0)
        out = check_sampler_agreement(lg, a, 99, 17, 0, f"mirror A={A}", record=False)
        assert out["near_frac"] == 0.0 and out["disagree"] == 0 and out["rows_below_1e3"] <= 0.002


def contingency_z(draw):
    """4 x 4 table of (action at step 17, action at step 18) of the same 65536 rows, equal logits: p = 1/16."""
    a1, a2 = draw(17).long().cpu(), draw(18).long().cpu()
    counts = torch.bincount(a1 * 4 + a2, minlength=16)
    return cell_z(counts, torch.full((16,), 1.0 / 16, dtype=torch.float64), a1.numel())


# ---------------------------------------------------------------------------------------------------------------
# GPU plumbing
# ---------------------------------------------------------------------------------------------------------------
def padded(t, fill=NAN):
    """[B, ...] CPU input -> [B + PAD, ...] on the GPU; the extra rows hold ``fill``."""
    out = torch.full((t.shape[0] + PAD,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    out[:t.shape[0]] = t
    return out.to(DEV)


def outbuf(rows, cols=None, dtype=torch.float32, fill=SENT):
    shape = (rows + PAD,) if cols is None else (rows + PAD, cols)
    return torch.full(shape, fill, dtype=dtype, device=DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def run_forward(hd, feat_d, B, f32, greedy, seed=7, ctr=0, t=0, T=1, b0=0, row_base=0, flat_d=None):
    """One launch on device features [>= B rows]; -> logits [B + PAD, A], value, actions with their sentinel rows."""
    from pathnet_gym_amd.ops import _lib
    A, F = hd["A"], hd["F"]
    flat_d = hd["flat"].to(DEV) if flat_d is None else flat_d
    logits, value, actions = outbuf(B, A), outbuf(B), outbuf(B, dtype=torch.int32, fill=int(SENT))
    ctr_d = torch.full((1,), ctr, dtype=torch.int64, device=DEV)
    _lib.call("launch_heads_fwd_sample_f32" if f32 else "launch_heads_fwd_sample", feat_d.data_ptr(), F,
              flat_d.data_ptr(), hd["pw"], hd["pb"], hd["vw"], hd["vb"], A, B, logits.data_ptr(), value.data_ptr(),
              actions.data_ptr(), seed, ctr_d.data_ptr(), t, T, int(greedy), b0, row_base, _lib.stream())
    torch.cuda.synchronize()
    return logits, value, actions


def check_forward_case(A, F, B, s16, seed):
    from pathnet_gym_amd.ops import _lib
    kernel = dispatch(A, F, s16)
    hd = make_heads(A, F, seed)
    _lib.lib().heads_set_s16(s16)
    try:
        for f32 in (False, True):
            x = make_feat(B, F, seed + 1, f32)
            if B > 1:
                x[B - 1] = 0                                 # logits == bias there: the planted tie
            fw = ref_forward(hd, x)
            feat_d = padded(x)
            for b0 in (0, 5) if B > 5 else (0,):
                tag = f"{kernel} A={A} F={F} B={B} {'f32' if f32 else 'bf16'} b0={b0}"
                logits, value, actions = run_forward(hd, feat_d, B, f32, greedy=True, b0=b0)
                for buf, name in ((logits, "logits"), (value, "value"), (actions, "actions")):
                    assert bool((buf[:b0] == SENT).all()) and bool((buf[B:] == SENT).all()), f"{tag}: {name} rows"
                within("fwd.logits", logits[b0:B], fw["logits"][b0:], fw["logits_bound"][b0:])
                within("fwd.value", value[b0:B], fw["value"][b0:], fw["value_bound"][b0:])
                lg = logits[b0:B].cpu()
                assert torch.equal(actions[b0:B].cpu().long(), first_argmax(lg)), tag
                if hd["tie"] and B > 1:
                    j1, j2 = hd["tie"]
                    assert lg[-1, j1] == lg[-1, j2] == lg[-1].max() == 0.75 and int(actions[B - 1]) == j1, tag
                if kernel != "wave":                         # fixed summation order: the same bits again
                    again = run_forward(hd, feat_d, B, f32, greedy=True, b0=b0)
                    assert all(torch.equal(bits(p), bits(q)) for p, q in zip((logits, value, actions), again)), tag
    finally:
        _lib.lib().heads_set_s16(1)


# (kernel reached, heads_set_s16, A, F): every branch of heads_fwd_lanes_launch
FWD_TABLE = [
    ("s16<8>", 1, 1, 128), ("s16<8>", 1, 8, 128), ("s16<8>", 1, 6, 256), ("s16<8>", 1, 3, 1024),   # A <= 8, F % 128 = 0
    ("s16<18>", 1, 9, 128), ("s16<18>", 1, 18, 512),                     # 9 <= A <= 18, F % 128 == 0, fits LDS
    ("lanes<8>", 1, 3, 32), ("lanes<8>", 1, 8, 96), ("lanes<8>", 1, 6, 160),   # A <= 8, F % 32 == 0, F % 128 != 0
    ("lanes<8>", 0, 6, 256),                                             # heads_set_s16(0)
    ("lanes<18>", 1, 9, 32), ("lanes<18>", 1, 18, 96),                   # F % 128 != 0
    ("lanes<18>", 1, 18, 640),                                           # s16 LDS 68 096 B > 64 KB, lanes 63 232 B
    ("lanes<18>", 0, 18, 256),                                           # heads_set_s16(0)
    ("wave", 1, 6, 40), ("wave", 1, 18, 100), ("wave", 1, 2, 1),         # F % 32 != 0
    ("wave", 1, 19, 128), ("wave", 1, 32, 256),                          # 19 <= A <= 32
    ("wave", 1, 18, 768), ("wave", 1, 8, 1664),                          # both LDS sizes over 64 KB
]
SWEEP_SHAPES = [(1, 6, 256), (1, 9, 128), (1, 8, 96), (1, 18, 96), (1, 6, 40)]      # one per kernel, every B


# ---------------------------------------------------------------------------------------------------------------
# A1 forward
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kernel,s16,A,F", FWD_TABLE)
def test_forward_every_dispatch_branch_matches_float64(hip_lib, kernel, s16, A, F):
    """B = 37: a ragged last workgroup in every kernel (16 / 64 samples per workgroup, 4 per workgroup of waves);
    bf16 and fp32 features, b0 in {0, 5}, greedy actions == first argmax of the kernel's own logits."""
    assert dispatch(A, F, s16) == kernel
    check_forward_case(A, F, 37, s16, seed=100 * A + F)


@gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("s16,A,F", SWEEP_SHAPES)
def test_forward_batch_edges(hip_lib, s16, A, F, B):
    check_forward_case(A, F, B, s16, seed=1000 * B + 10 * A + F)


@gpu
def test_forward_launcher_rejects_bad_arguments(hip_lib):
    hd = make_heads(6, 128, seed=1)
    flat_d = hd["flat"].to(DEV)
    ctr = torch.zeros(1, dtype=torch.int64, device=DEV)
    from pathnet_gym_amd.ops import _lib
    for f32 in (False, True):
        feat = padded(make_feat(16, 128, 2, f32))
        logits, value, actions = outbuf(16, 33), outbuf(16), outbuf(16, dtype=torch.int32, fill=int(SENT))
        fn = getattr(hip_lib, "launch_heads_fwd_sample_f32" if f32 else "launch_heads_fwd_sample")

        def call(F=128, A=6, B=16, T=1, b0=0):
            return fn(feat.data_ptr(), F, flat_d.data_ptr(), hd["pw"], hd["pb"], hd["vw"], hd["vb"], A, B,
                      logits.data_ptr(), value.data_ptr(), actions.data_ptr(), 7, ctr.data_ptr(), 0, T, 1, b0, 0,
                      _lib.stream())
        assert call(A=33) == -1 and call(b0=16) == -1 and call(b0=17) == -1
        assert call(F=0) == -22 and call(F=-128) == -22 and call(B=0) == -22 and call(T=0) == -22
        assert call(A=0) == -22 and call(b0=-1) == -22
        torch.cuda.synchronize()
        for buf in (logits, value, actions):
            assert bool((buf == SENT).all())                # nothing ran


# ---------------------------------------------------------------------------------------------------------------
# A2 - A4 sampler
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sampler_feat(N, F=128):
    return padded(make_feat(N, F, seed=21, f32=False, scale=1.0))


@gpu
@pytest.mark.parametrize("seed,row_base", SAMPLER_KEYS)
@pytest.mark.parametrize("A", SAMPLER_A)
def test_sampled_actions_equal_float64_gumbel_argmax_outside_near_ties(hip_lib, A, seed, row_base):
    """16384 rows, logits of standard deviation ~2 (s16<8>, s16<18> and the wave kernel), stepkey 3 * 5 + 2.  (The
    case A = 32, seed 12345 holds one draw with k = 2^24 - 1: global row 13486, action 26.)"""
    hd = make_heads(A, 128, seed=31 + A, wscale=2.0 / math.sqrt(128))
    logits, _, actions = run_forward(hd, sampler_feat(SAMPLER_N), SAMPLER_N, False, greedy=False, seed=seed, ctr=CTR,
                                     t=2, T=T_ROLL, row_base=row_base)
    assert bool((actions[SAMPLER_N:] == SENT).all())
    lg, a = logits[:SAMPLER_N].cpu(), actions[:SAMPLER_N].cpu()
    assert 1.5 < float(lg.std()) < 2.5 and int(a.min()) >= 0 and int(a.max()) < A
    check_sampler_agreement(lg, a, seed, CTR * T_ROLL + 2, row_base, f"A={A} seed={seed} row_base={row_base}")


def gpu_draws(hd, flat_d, N, seed, stepkey, row_base):
    ctr, t = divmod(stepkey, T_ROLL)
    logits, _, actions = run_forward(hd, sampler_feat(N), N, False, greedy=False, seed=seed, ctr=ctr, t=t, T=T_ROLL,
                                     row_base=row_base, flat_d=flat_d)
    return logits[:N], actions[:N]


@gpu
@pytest.mark.parametrize("scale", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("A", SAMPLER_A)
def test_sampled_actions_follow_softmax(hip_lib, A, scale):
    """Constant logits (zero policy weights, bias = lg) over 16384 rows, stepkeys 15 .. 22 pooled: every action's
    count within 5 sigma of n softmax(lg) (actions with n p < 25 pooled into one cell).  Both sides of the count are
    bounded; a draw that is TOO uniform is not tested for: the hash is no i.i.d. source."""
    lg = dist_logits(A, scale)
    hd = make_heads(A, 128, seed=A, zero_w=True, bias=lg)
    flat_d = hd["flat"].to(DEV)
    p = torch.softmax(lg.double(), 0)
    for seed, rb in SAMPLER_KEYS:
        counts = torch.zeros(A, dtype=torch.int64)
        for stepkey in range(15, 23):
            logits, a = gpu_draws(hd, flat_d, SAMPLER_N, seed, stepkey, rb)
            if stepkey == 15:
                assert torch.equal(logits.cpu(), lg[None].expand(SAMPLER_N, -1))    # zero weights: the bias itself
            counts += torch.bincount(a.cpu().long(), minlength=A)
        z = cell_z(counts, p, 8 * SAMPLER_N)
        print(f"A={A} scale={scale} seed={seed} row_base={rb}: max |z| = {float(z.abs().max()):.3f}")
        record_measured({"sampler.max_abs_z": float(z.abs().max())})
        assert int(counts.sum()) == 8 * SAMPLER_N and float(z.abs().max()) <= 5.0, (seed, rb, z)


@gpu
def test_consecutive_steps_are_independent(hip_lib):
    """A = 4, equal logits, 65536 rows: the 4 x 4 table of (action at step 17, action at step 18), p = 1/16 a cell."""
    hd = make_heads(4, 128, seed=4, zero_w=True, bias=torch.zeros(4))
    flat_d = hd["flat"].to(DEV)
    z = contingency_z(lambda stepkey: gpu_draws(hd, flat_d, 65536, 99, stepkey, 0)[1])
    print(f"contingency: max |z| = {float(z.abs().max()):.3f}")
    record_measured({"sampler.contingency_max_abs_z": float(z.abs().max())})
    assert float(z.abs().max()) <= 5.0, z


@gpu
@pytest.mark.parametrize("F", [128, 96, 40])
def test_draw_with_every_hash_bit_set_does_not_force_its_action(hip_lib, F):
    """The crafted key of test_wang_inverse_and_u_strictly_inside_unit_interval_cpu through the s16 (F = 128), lanes
    (96) and wave-per-sample (40) kernels: logits 0 except -30 on action 4, and the draw of (row 37, action 4) has
    k = 2^24 - 1.  With u == 1 its Gumbel noise is +inf and row 37 draws the action of probability e^-30."""
    A, j0 = U1["A"], U1["j0"]
    assert dispatch(A, F) == {128: "s16<8>", 96: "lanes<8>", 40: "wave"}[F]
    hd = make_heads(A, F, seed=F, zero_w=True, bias=u1_logits())
    B, row_base = 40, 5
    feat_d = padded(make_feat(B, F, seed=3, f32=False))
    seed = u1_seed()
    logits, _, actions = run_forward(hd, feat_d, B, False, greedy=False, seed=seed, ctr=CTR, t=2, T=T_ROLL,
                                     row_base=row_base)
    lg, a = logits[:B].cpu(), actions[:B].cpu().long()
    assert torch.equal(lg, u1_logits()[None].expand(B, -1))
    assert int(a[U1["row"] - row_base]) != j0 and not bool((a == j0).any()), a
    out = check_sampler_agreement(lg, a, seed, U1["stepkey"], row_base, f"u=1 F={F}", record=False)
    assert out["near_frac"] == 0.0 and out["disagree"] == 0
    assert torch.equal(a, sample_actions_keyed(lg, seed, U1["stepkey"], row_base))


# ---------------------------------------------------------------------------------------------------------------
# A5 backward
# ---------------------------------------------------------------------------------------------------------------
BWD_MODES = ["atomic", "det", "split32", "split128"]


def part_numel(mode, N, F, A):
    from pathnet_gym_amd.ops import _lib
    PS = F * A + F + A + 1
    if mode == "det":
        n = _lib.lib().heads_bwd_part_numel(N, F, A)
        assert n == -(-N // 128) * PS
    else:
        n = _lib.lib().heads_bwd_split_numel(N, F, A)
        assert n == -(-N // 32) * PS
    return n


def run_backward(hd, x, dz, dv, mode, g0):
    """One launch of ``mode``; -> grad (CPU, flat-sized), dfeat [N + PAD, F] (CPU)."""
    from pathnet_gym_amd.ops import _lib
    A, F, N = hd["A"], hd["F"], x.shape[0]
    f32 = int(x.dtype == torch.float32)
    flat_d, grad = hd["flat"].to(DEV), g0.to(DEV)
    feat_d, dz_d, dv_d = padded(x), padded(dz), padded(dv)
    dfeat = outbuf(N, F)
    dfeat[:N] = NAN                                          # overwritten, never accumulated into
    offs = (hd["pw"], hd["pb"], hd["vw"], hd["vb"])
    part = None
    if mode == "atomic":
        _lib.call("launch_heads_bwd_f32" if f32 else "launch_heads_bwd", feat_d.data_ptr(), F, dz_d.data_ptr(),
                  dv_d.data_ptr(), N, A, flat_d.data_ptr(), *offs, grad.data_ptr(), dfeat.data_ptr(), _lib.stream())
    else:
        n = part_numel(mode, N, F, A)
        part = torch.full((n + PAD,), SENT, device=DEV)
        if mode != "det":
            _lib.lib().heads_set_bwd_rows(32 if mode == "split32" else 128)
        try:
            _lib.call("launch_heads_bwd_det" if mode == "det" else "launch_heads_bwd_split", feat_d.data_ptr(), f32, F,
                      dz_d.data_ptr(), dv_d.data_ptr(), N, A, flat_d.data_ptr(), *offs, grad.data_ptr(),
                      dfeat.data_ptr(), part.data_ptr(), _lib.stream())
        finally:
            _lib.lib().heads_set_bwd_rows(32)                # the default
    torch.cuda.synchronize()
    if part is not None:
        assert bool((part[n:] == SENT).all()), f"{mode}: the partials ran past {n} floats"
        if mode == "split128":
            assert bool((part == SENT).all())                # the 128-row atomic kernel takes no partials
    return grad.cpu(), dfeat.cpu()


def check_backward_case(A, F, N, mode, f32, seed):
    hd = make_heads(A, F, seed)
    x = make_feat(N, F, seed + 1, f32)
    g = torch.Generator().manual_seed(seed + 2)
    dz, dv = torch.randn(N, A, generator=g) * 0.1, torch.randn(N, generator=g) * 0.1
    bw = ref_backward(hd, x, dz, dv)
    numel = hd["flat"].numel()
    segs = {"dWp": slice(hd["pw"], hd["pw"] + F * A), "dbp": slice(hd["pb"], hd["pb"] + A),
            "dwv": slice(hd["vw"], hd["vw"] + F), "dbv": slice(hd["vb"], hd["vb"] + 1)}
    outside = torch.ones(numel, dtype=torch.bool)
    for s in segs.values():
        outside[s] = False
    adds = 1 if mode in ("det", "split32") else -(-N // 128)         # fp32 adds into a grad entry (module docstring)
    tag = f"bwd.{mode}"
    for g0 in (torch.zeros(numel), torch.randn(numel, generator=g) * 0.05):
        grad, dfeat = run_backward(hd, x, dz, dv, mode, g0)
        assert bool((dfeat[N:] == SENT).all()), "dfeat: rows >= N were written"
        assert torch.equal(bits(grad)[outside], bits(g0)[outside]), "grad was written outside the head parameters"
        within(f"{tag}.dfeat", dfeat[:N], bw["dfeat"], bw["dfeat_bound"])
        for name, s in segs.items():
            ref, bound = bw[name].reshape(-1), bw[name + "_bound"].reshape(-1)
            key = f"{tag}.{name}"
            if bool((g0 != 0).any()):                        # recorded apart: the bound carries the accumulate term
                bound = bound + adds * 2.0 ** -24 * 1.001 * (g0[s].abs().double() + bound / ((N + 8) * EPS))
                key += ".accumulate"
            within(key, grad[s].double() - g0[s].double(), ref, bound)
        if mode in ("det", "split32"):                       # fixed order: the same bits from the same state
            grad2, dfeat2 = run_backward(hd, x, dz, dv, mode, g0)
            assert torch.equal(bits(grad2), bits(grad)) and torch.equal(bits(dfeat2), bits(dfeat)), tag


def bwd_cases():
    out = [(A, F, N) for A, F in ((8, 320), (18, 320)) for N in (1, 31, 32, 33, 127, 128, 129, 213)]
    # the reduced cross: every A and every F twice or more, at a ragged N of two 128-row / five 32-row chunks
    out += [(1, 32, 129), (1, 256, 129), (8, 32, 129), (8, 96, 129), (8, 256, 129), (9, 32, 129), (9, 96, 129),
            (9, 320, 129), (18, 96, 129), (18, 256, 129), (32, 32, 129), (32, 96, 129), (32, 256, 129),
            (32, 320, 129), (1, 320, 213), (9, 256, 213)]
    return out


@gpu
@pytest.mark.parametrize("mode", BWD_MODES)
@pytest.mark.parametrize("A,F,N", bwd_cases())
def test_backward_every_launcher_matches_float64(hip_lib, A, F, N, mode):
    """AM = 8 (A <= 8) and AM = 32 templates, F under and over the 256 threads of a workgroup, N at the 32- and
    128-row chunk edges; bf16 and fp32 features; grad from zero and from a random vector (+= contract)."""
    for f32 in (False, True):
        check_backward_case(A, F, N, mode, f32, seed=10000 * A + 10 * F + N)


@gpu
def test_backward_launchers_reject_bad_arguments(hip_lib):
    from pathnet_gym_amd.ops import _lib
    lib, s = hip_lib, _lib.stream()
    A, F, N = 6, 64, 40
    hd = make_heads(A, F, seed=1)
    flat_d = hd["flat"].to(DEV)
    offs = (hd["pw"], hd["pb"], hd["vw"], hd["vb"])
    x, dz, dv = padded(make_feat(N, F, 2, False)), outbuf(N, 33, fill=0.5), outbuf(N, fill=0.5)
    grad, dfeat, part = outbuf(hd["flat"].numel()), outbuf(N, F), outbuf(8 * (F * 33 + F + 34))
    for fn in (lib.launch_heads_bwd, lib.launch_heads_bwd_f32):
        call = lambda F=F, N=N, A=A, pw=offs[0]: fn(x.data_ptr(), F, dz.data_ptr(), dv.data_ptr(), N, A,      # noqa
                                                     flat_d.data_ptr(), pw, *offs[1:], grad.data_ptr(),
                                                     dfeat.data_ptr(), s)
        assert call(F=0) == -22 and call(N=0) == -22 and call(A=0) == -22 and call(N=-5) == -22 and call(pw=-1) == -22
        assert call(A=33) == -1
    for fn, null_part in ((lib.launch_heads_bwd_det, -1), (lib.launch_heads_bwd_split, -22)):
        for f32 in (0, 1):
            call = lambda F=F, N=N, A=A, f32=f32, part=part.data_ptr(): fn(                                    # noqa
                x.data_ptr(), f32, F, dz.data_ptr(), dv.data_ptr(), N, A, flat_d.data_ptr(), *offs, grad.data_ptr(),
                dfeat.data_ptr(), part, s)
            assert call(F=0) == -22 and call(N=0) == -22 and call(A=0) == -22 and call(f32=-1) == -22
            assert call(A=33) == -1 and call(part=None) == null_part
    assert lib.heads_bwd_part_numel(0, F, A) == -1 and lib.heads_bwd_split_numel(N, 0, A) == -1
    assert lib.heads_bwd_part_numel(N, F, 0) == -1 and lib.heads_bwd_split_numel(-1, F, A) == -1
    assert lib.heads_bwd_part_numel(129, F, A) == 2 * (F * A + F + A + 1)
    assert lib.heads_bwd_split_numel(129, F, A) == 5 * (F * A + F + A + 1)
    torch.cuda.synchronize()
    for buf in (grad, dfeat, part):
        assert bool((buf == SENT).all())                     # nothing ran
