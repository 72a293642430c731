"""csrc/lstm_x3.hip, launcher by launcher, against plain float64 torch with buffers of the test's own.

The method and scaffolding of tests/test_lstm_kernels.py (synthetic ``flat`` with odd ``k_off`` / ``b_off``, 64
sentinel rows after every output, 64 NaN rows after every input, NaN in h / c where ``prev_done`` is set).  The
operands are plain fp32 and enter the float64 reference as they are: splitting them into fp16 pairs is the kernel's
business.  Every GEMM output (dx, dh_prev, dK; for the forward gates, cout, hout) meets two criteria.

(a) An elementwise bound, derived.  An operand a, multiplied by the power of two s the kernel applies before the split
(1 for the forward's [x | h], 2^8 for K, the G16 scale 2^(13 - e) of an amax in [2^e, 2^(e+1)) for dz and for the
weight gradient's xh), becomes hi = rn16(a s), lo = rn16(a s - hi).  hi is within half an ulp, 2^-11 |a s|, and lo
rounds that remainder to 11 bits again unless it is subnormal in fp16, where the spacing is 2^-24:

    |a - (hi + lo) / s| <= 2^-22 |a| + 2^-25 / s                                   =: d(a)

The kernel forms hi*hi + hi*lo + lo*hi and drops lo*lo, |lo_a lo_k| / (s_a s_k) <= 2^-22 |a| |k|.  So, against the
exact product sum, with |A|, |K| the elementwise absolute values,

    pair  = d(A) @ |K| + (|A| + d(A)) @ d(K) + 2^-22 |A| @ |K|

and the fp32 accumulation of the three MFMAs per k-step adds n * 2^-23 * (|A| @ |K|), n = 3 x the reduction length
(2^-24 per term would be the first-order bound of a chain of n terms; 2^-23 covers whatever rounding the f16 MFMA
uses inside, and the one rounding of the final power-of-two rescale or chain subtraction).  The forward's z = acc + b
gets 2^-23 |z| for the bias add, and gates / cout / hout carry the bound of z through the cell with the Lipschitz
constants of tests/test_lstm_f32_kernels.py ``ref_forward`` (1/4 sigmoid, 1 tanh) plus ``8 * e32``, e32 = the max abs
error of a torch fp32 evaluation of the same formulas against float64 (``__expf`` is not torch's ``exp``).  The atomic
weight gradient adds once per row chunk into a running fp32 value: 2^-24 (|grad0| + |xh|^T |dz|) per add, as in the
bf16 suite; the deterministic one quantises each chunk's contribution to 2^-34 (2^-35 per chunk and entry) and the
flush converts and adds once.

(b) The accuracy class of the mode.  With n in the hundreds, (a) is far looser than the 2^-12 a lost cross term
(hi*lo or lo*hi) or a lo plane read at the wrong offset costs, so each of these outputs must also satisfy

    ||hip - ref64||_F / ||ref64||_F < X3_LAYER_TOL = 2e-5         over the valid rows

the per-layer figure of tests/test_x3_engine.py.  ``test_pair_emulation_separates_the_mutants_cpu`` emulates the
split in torch on the inputs used here and shows that the full three-product form and a plain fp32 matmul stay
below it at every shape and scale, and that each mutant (a cross term dropped, the lo plane shifted by one 32-wide
k-step, no G16 scale at a small scale) exceeds it at least twice over: a condition on the inputs, not a tolerance
on the kernel.  The worst measured ``rel`` and ``err / bound`` per tensor are kept in
tests/data/lstm_x3_measured.json (written when ``PATHNET_RECORD_LSTM_X3=<file>`` is set): a record, not a budget.
"""
import json
import math
import os

import pytest
import torch

from test_lstm_kernels import (BATCHES, EPS, NAN, SENT, SMALL_FH, assert_sentinel, bits, cell_from_z, gemm_bound,
                               outbuf, padded, ptr, ref_backward_point, select_rows)
from test_x3_engine import X3_LAYER_TOL

gpu = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")
ALL_FH = SMALL_FH + [(256, 256)]
FWD_SHAPES = [(F, H, B) for F, H in SMALL_FH for B in BATCHES] + [(256, 256, 17), (256, 256, 130)]
K_SCALE = 256.0                                    # LX3_SHIFT
DZ_SCALES = [1.0, 2.0 ** -30, 3e-7, 2.0 ** 10]     # what the backward GEMM's dz is multiplied by
STALE = [1.0, 8.0]                                 # the amax slot: exact, or a stale larger one
STEP_SCALES = [2.0 ** -10, 1.0, 2.0 ** -20]        # T = 3: the rows of step t are scaled by STEP_SCALES[t]
assert len(FWD_SHAPES) == 3 * len(BATCHES) + 2


# ---------------------------------------------------------------------------------------------------------------
# the split, its bound, and the float64 reference (CPU tensors)
# ---------------------------------------------------------------------------------------------------------------
def f32(v):
    """A Python float rounded to fp32 (what an amax slot holds)."""
    return float(torch.tensor(v, dtype=torch.float32))


def g16_scale(amax):
    """csrc/lstm_x3.hip g16_scale_of: the power of two that puts amax into [2^13, 2^14); 1 for 0, non-finite or
    subnormal-range amaxes."""
    if not (amax > 0.0) or math.isinf(amax):
        return 1.0
    e = math.frexp(amax)[1] - 1
    if e < -110 or e >= 128:
        return 1.0
    return 2.0 ** min(13 - e, 126)


def pair(v, s):
    """fp16 pair of v * s, round to nearest even like ``(_Float16)``: hi, lo as float64."""
    t = v.float() * s
    hi = t.half()
    lo = (t - hi.float()).half()
    return hi.double(), lo.double()


def x3_bound(A, sa, Bm, sb, n):
    """Criterion (a) for A [m, k] @ Bm [k, q], split at scales sa / sb, reduction length n: (pair part, whole bound)."""
    A, Bm = A.double().abs(), Bm.double().abs()
    dA, dB = 2.0 ** -22 * A + 2.0 ** -25 / sa, 2.0 ** -22 * Bm + 2.0 ** -25 / sb
    pair_part = dA @ Bm + (A + dA) @ dB + 2.0 ** -22 * (A @ Bm)
    return pair_part, pair_part + gemm_bound(A, Bm, 3 * n)


def rel(got, ref):
    got, ref = got.double().cpu(), ref.double()
    return float((got - ref).norm() / ref.norm())


def rand_xh(g, R, F, H):
    return torch.cat([torch.randn(R, F, generator=g) * 0.5, torch.tanh(torch.randn(R, H, generator=g)) * 0.5], 1)


def rand_dz(g, R, G4):
    """0.05 randn, every other column another 1e-3 smaller."""
    dz = torch.randn(R, G4, generator=g) * 0.05
    dz[:, 1::2] *= 1e-3
    return dz


def make_case(F, H, B, seed, prev="rand", sat=False):
    """Synthetic weights + one step's inputs (CPU), all plain fp32.  k_off / b_off are non-zero and odd; rows whose
    prev_done is set hold NaN in h and c: the cell must see zeros there without ever touching them."""
    g = torch.Generator().manual_seed(seed)
    KK, G4 = F + H, 4 * H
    k_off = 37
    b_off = k_off + KK * G4 + 12
    flat = torch.randn(b_off + G4 + 29, generator=g) * 0.1
    bias = torch.randn(G4, generator=g) * 0.5
    if sat:   # pre-activations around +-30: every gate saturated, either way
        bias = torch.where(torch.rand(G4, generator=g) < 0.5, -30.0, 30.0) + torch.randn(G4, generator=g)
    flat[b_off:b_off + G4] = bias
    xh = rand_xh(g, B, F, H)
    x, h = xh[:, :F].clone(), xh[:, F:].clone()
    c = torch.randn(B, H, generator=g)
    if prev is None:
        pd = None
    elif prev == "rand":
        pd = (torch.rand(B, generator=g) < 0.4).to(torch.uint8)
        pd[0] = 0
        if B > 1:
            pd[B - 1] = 1
    else:
        pd = torch.full((B,), 1 if prev == "ones" else 0, dtype=torch.uint8)
    if pd is not None:
        h[pd.bool()] = NAN
        c[pd.bool()] = NAN
    return dict(F=F, H=H, B=B, k_off=k_off, b_off=b_off, flat=flat, x=x, h=h, c=c, prev_done=pd,
                K=flat[k_off:k_off + KK * G4].view(KK, G4), b=flat[b_off:b_off + G4])


def forward_from_acc(cs, xh, ck, acc, zb):
    """float64 cell outputs of pre-activations acc + b and the tolerances that a bound zb of z gives them."""
    z = acc + cs["b"].double()
    zb = zb + EPS * z.abs()
    gates, c, h = cell_from_z(z, ck.double())
    g32, c32, h32 = cell_from_z(acc.float() + cs["b"], ck)             # torch fp32 on the same inputs
    e32 = {"gates": float((g32 - gates).abs().max()), "cout": float((c32 - c).abs().max()),
           "hout": float((h32 - h).abs().max())}
    di, dj, df, do = zb.chunk(4, 1)
    dg = torch.cat([di / 4, dj, df / 4, do / 4], 1)                    # |sig'| <= 1/4, |tanh'| <= 1
    dc = ck.double().abs() * df / 4 + di / 4 + dj                      # c = c0 sig(f) + sig(i) tanh(j), |.| <= 1
    dh = dc + do / 4                                                   # h = tanh(c) sig(o)
    tol = {"gates": dg + 8 * e32["gates"], "cout": dc + 8 * e32["cout"], "hout": dh + 8 * e32["hout"]}
    return dict(xh=xh, acc=acc, z=z, ck=ck, gates=gates, c=c, h=h, e32=e32, tol=tol)


def ref_forward(cs, K=None):
    """float64 forward of a case + the tolerances of every forward output (module docstring).  K: another kernel
    matrix in place of the case's (the negative control)."""
    F, H = cs["F"], cs["H"]
    keep = None if cs["prev_done"] is None else cs["prev_done"] == 0
    hk, ck = select_rows(keep, cs["h"]), select_rows(keep, cs["c"])
    xh = torch.cat([cs["x"], hk], 1)
    K = cs["K"] if K is None else K
    return forward_from_acc(cs, xh, ck, xh.double() @ K.double(), x3_bound(xh, 1.0, K, K_SCALE, F + H)[1])


def ref_backward_gemm(cs, dz, amax):
    """float64 [dx | dh_prev] = dz K^T, the pair part and the whole bound (n = 4H) for a dz amax slot ``amax``."""
    Kt = cs["K"].t()
    return (dz.double() @ Kt.double(),) + x3_bound(dz, g16_scale(amax), Kt, K_SCALE, 4 * cs["H"])


def ref_wgrad(xh, dz, amax_xh, amax_dz):
    """float64 weight / bias gradient of R rows: dK, its pair part and whole bound (n = R), db and its bound (the
    bias gradient sums the unrounded fp32 dz)."""
    R = xh.shape[0]
    pair_part, bound = x3_bound(xh.t(), g16_scale(amax_xh), dz, g16_scale(amax_dz), R)
    return xh.double().t() @ dz.double(), pair_part, bound, dz.double().sum(0), R * EPS * dz.double().abs().sum(0)


def amax_of(t):
    t = t[torch.isfinite(t)]
    return float(t.abs().max()) if t.numel() else 0.0


def step_of_rows(R, T):
    return torch.arange(R) * T // R


# ---------------------------------------------------------------------------------------------------------------
# CPU: criterion (b) separates the mutants on these inputs
# ---------------------------------------------------------------------------------------------------------------
def emulate(A, sa, Bm, sb, mutant=None):
    """The kernel's three products of the fp16 pairs of A * sa [m, k] and Bm * sb [k, q], formed in float64.
    Mutants: "no_hi_lo" / "no_lo_hi" drop a cross term, "lo_shift" reads Bm's lo plane one 32-wide k-step off."""
    ah, al = pair(A, sa)
    bh, bl = pair(Bm, sb)
    if mutant == "lo_shift":
        bl = torch.roll(bl, 32, dims=0)
    out = ah @ bh
    if mutant != "no_hi_lo":
        out = out + ah @ bl
    if mutant != "no_lo_hi":
        out = out + al @ bh
    return out / (sa * sb)


def check_emulation(name, A, sa, Bm, sb, small_scale=False, unscaled=None, through=None):
    """The full pair form is within the pair part of (a) and below the tolerance, like plain fp32; every mutant is
    at least twice over it.  ``through``: maps the GEMM output to further tensors that must show the same."""
    ref = A.double() @ Bm.double()
    views = {"": lambda t: t}
    views.update(through or {})
    full = emulate(A, sa, Bm, sb)
    assert bool(((full - ref).abs() <= x3_bound(A, sa, Bm, sb, 1)[0]).all()), name
    plain = (A.float() @ Bm.float()).double()
    muts = {m: emulate(A, sa, Bm, sb, m) for m in ("no_hi_lo", "no_lo_hi", "lo_shift")}
    if small_scale:
        muts["no_g16"] = emulate(A, *unscaled)
    for vn, view in views.items():
        r0 = view(ref)
        e_full, e_plain = rel(view(full), r0), rel(view(plain), r0)
        assert e_full < X3_LAYER_TOL and e_plain < X3_LAYER_TOL, (name, vn, e_full, e_plain)
        for m, out in muts.items():
            e = rel(view(out), r0)
            assert e > 2 * X3_LAYER_TOL, (name, vn, m, e)


def test_pair_emulation_separates_the_mutants_cpu():
    for F, H in ALL_FH:
        B = R = 130
        cs = make_case(F, H, B, seed=3 * F + H, prev=None)
        fw = ref_forward(cs)
        gates_of = lambda acc: cell_from_z(acc + cs["b"].double(), fw["ck"].double())[0]     # noqa: E731
        check_emulation(f"fwd {F} {H}", fw["xh"], 1.0, cs["K"], K_SCALE, through={"gates": gates_of})
        g = torch.Generator().manual_seed(F + 7 * H)
        dz0, xh = rand_dz(g, R, 4 * H), rand_xh(g, R, F, H)
        sx = g16_scale(amax_of(xh))
        for scale in DZ_SCALES:
            dz = dz0 * scale
            small = scale < 1e-3
            for stale in STALE:
                sg = g16_scale(f32(amax_of(dz) * stale))
                check_emulation(f"bwd {F} {H} {scale} {stale}", dz, sg, cs["K"].t(), K_SCALE, small,
                                (1.0, cs["K"].t(), K_SCALE))
                check_emulation(f"wgrad {F} {H} {scale} {stale}", xh.t(), sx, dz, sg, small, (sx, dz, 1.0))
        dz = dz0 * torch.tensor(STEP_SCALES)[step_of_rows(R, 3)][:, None]
        check_emulation(f"wgrad {F} {H} T=3", xh.t(), sx, dz, g16_scale(amax_of(dz)))
    # the twin of g16_scale_of
    assert g16_scale(0.0) == 1.0 and g16_scale(INF) == 1.0 and g16_scale(NAN) == 1.0
    assert g16_scale(1.0) == 2.0 ** 13 and g16_scale(1.999) == 2.0 ** 13 and g16_scale(2.0) == 2.0 ** 12
    assert g16_scale(2.0 ** -120) == 1.0 and g16_scale(2.0 ** -110) == 2.0 ** 123 and g16_scale(2.0 ** -113.5) == 1.0


# ---------------------------------------------------------------------------------------------------------------
# GPU plumbing
# ---------------------------------------------------------------------------------------------------------------
def record(kind, name, value):
    """PATHNET_RECORD_LSTM_X3=<file>: keep the worst measured figure per tensor."""
    rec = os.environ.get("PATHNET_RECORD_LSTM_X3")
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


def excess(got, ref, tol):
    """Elementwise err / tol of a finite output."""
    return (got.double().cpu() - ref).abs() / tol.clamp_min(1e-300)


def within(name, got, ref, tol):
    """Criterion (a)."""
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    r = excess(got, ref, tol)
    worst = float(r.max())
    print(f"{name}: worst err / bound = {worst:.4f}")
    record("worst_err_over_bound", name, worst)
    assert worst <= 1.0, (name, worst, int((r > 1).sum()), r.numel())


def accurate(name, got, ref):
    """Criterion (b)."""
    e = rel(got, ref)
    print(f"{name}: rel = {e:.3e}")
    record("worst_rel", name, e)
    assert e < X3_LAYER_TOL, (name, e)


def both(name, got, ref, tol):
    within(name, got, ref, tol)
    accurate(name, got, ref)


def halfbuf(n):
    return torch.full((n + 4096,), SENT, dtype=torch.float16, device=DEV)


def refresh(cs, status=None):
    from pathnet_gym_amd.ops import _lib
    F, H = cs["F"], cs["H"]
    flat = cs["flat"].to(DEV)
    n2 = 2 * (F + H) * 4 * H
    KpT2, Kb2 = halfbuf(n2), halfbuf(n2)
    _lib.call("launch_lstm_refresh_x3", flat.data_ptr(), cs["k_off"], F, H, KpT2.data_ptr(), Kb2.data_ptr(),
              ptr(status), _lib.stream())
    return flat, KpT2, Kb2


def run_forward(cs, want_gates=True, want_xh=True, ldx=None, amax0=0.0, x=None):
    from pathnet_gym_amd.ops import _lib
    F, H, B = cs["F"], cs["H"], cs["B"]
    flat, KpT2, _ = refresh(cs)
    X = padded(cs["x"] if x is None else x, cols=ldx)                 # ldx > F: the pad columns hold NaN
    hp, cp = padded(cs["h"]), padded(cs["c"])
    pd = None if cs["prev_done"] is None else padded(cs["prev_done"][:, None], fill=1).view(-1)
    hout, cout = outbuf(B, H), outbuf(B, H)
    gates = outbuf(B, 4 * H) if want_gates else None
    xh = outbuf(B, F + H) if want_xh else None
    status = torch.tensor([0, 12345], dtype=torch.int32, device=DEV)
    amax = torch.tensor([SENT, amax0, SENT], device=DEV)
    _lib.call("launch_lstm_fwd_x3", X.data_ptr(), X.shape[1], hp.data_ptr(), cp.data_ptr(), ptr(pd),
              KpT2.data_ptr(), flat.data_ptr(), cs["b_off"], hout.data_ptr(), cout.data_ptr(), ptr(gates), ptr(xh),
              status.data_ptr(), amax.data_ptr() + 4, F, H, B, _lib.stream())
    torch.cuda.synchronize()
    assert int(status[1]) == 12345 and float(amax[0]) == SENT and float(amax[2]) == SENT
    return dict(hout=hout, cout=cout, gates=gates, xh=xh, status=int(status[0]), amax=amax[1:2].cpu(), amax0=amax0)


def check_forward(cs, out, fw, tag="fwd"):
    B = cs["B"]
    for name in ("hout", "cout", "gates", "xh"):
        if out[name] is not None:
            assert_sentinel(out[name], B, name)
    assert out["status"] == 0                       # the NaN of the pad rows and of the reset rows was never read
    want_amax = out["amax0"]
    if out["xh"] is not None:     # [x | h * keep], bit for bit, and its amax over the B valid rows
        assert torch.equal(bits(out["xh"][:B].cpu()), bits(fw["xh"]))
        want_amax = max(want_amax, float(fw["xh"].abs().max()))
    assert torch.equal(bits(out["amax"]), bits(torch.tensor([want_amax])))
    if out["gates"] is not None:
        both(f"{tag}.gates", out["gates"][:B], fw["gates"], fw["tol"]["gates"])
    both(f"{tag}.cout", out["cout"][:B], fw["c"], fw["tol"]["cout"])
    both(f"{tag}.hout", out["hout"][:B], fw["h"], fw["tol"]["hout"])


def assert_scaled_column_fails(cs, out):
    """Negative control (tests/test_lstm_f32_kernels.py): against a reference whose kernel column H + 3 (unit 3 of
    the j gate) is scaled by 1.02, the same outputs leave the same kind of bound."""
    B, H = cs["B"], cs["H"]
    K = cs["K"].clone()
    K[:, H + 3] *= 1.02
    bad = ref_forward(cs, K=K)
    assert float(excess(out["gates"][:B], bad["gates"], bad["tol"]["gates"]).max()) > 1.0
    assert float(excess(out["cout"][:B], bad["c"], bad["tol"]["cout"]).max()) > 1.0
    assert float(excess(out["hout"][:B], bad["h"], bad["tol"]["hout"]).max()) > 1.0


# ---------------------------------------------------------------------------------------------------------------
# refresh / carry
# ---------------------------------------------------------------------------------------------------------------
def h16(t):
    return t.contiguous().view(torch.int16)


@gpu
@pytest.mark.parametrize("F,H", ALL_FH)
def test_refresh_pairs_and_permutation_are_bit_exact(hip_lib, F, H):
    """Kb2 = [hi | lo] of K * 2^8 in TF layout; KpT2[plane][(u/16)*64 + g*16 + u%16][n] = plane of K[n][g*H + u]."""
    cs = make_case(F, H, 1, seed=F + 3 * H)
    KK, G4 = F + H, 4 * H
    n = KK * G4
    status = torch.tensor([0, 12345], dtype=torch.int32, device=DEV)
    _, KpT2, Kb2 = refresh(cs, status)
    torch.cuda.synchronize()
    assert status.tolist() == [0, 12345]
    assert bool((KpT2[2 * n:] == SENT).all()) and bool((Kb2[2 * n:] == SENT).all()), "written past 2 * KK * 4H halves"
    k256 = cs["K"] * K_SCALE
    hi = k256.half()
    lo = (k256 - hi.float()).half()
    assert bool((lo != 0).any())
    col = torch.arange(G4)
    g_, u = col // H, col % H
    p = (u >> 4) * 64 + g_ * 16 + (u & 15)
    assert sorted(p.tolist()) == list(range(G4))
    for i, plane in enumerate((hi, lo)):
        assert torch.equal(h16(Kb2[i * n:(i + 1) * n].cpu()), h16(plane).view(-1)), ("Kb2", i)
        want = torch.empty(G4, KK, dtype=torch.float16)
        want[p] = plane.t()
        assert torch.equal(h16(KpT2[i * n:(i + 1) * n].cpu()), h16(want).view(-1)), ("KpT2", i)


@gpu
@pytest.mark.parametrize("value,flag", [(127.99999, 0), (-127.99999, 0), (128.0, 1), (-128.0, 1), (INF, 1), (NAN, 1)])
def test_refresh_status_word(hip_lib, value, flag):
    """Bit 0 is set when a kernel weight times 2^8 reaches 32768, and for inf and NaN; a null status is accepted."""
    F, H = 64, 128
    cs = make_case(F, H, 1, seed=5)
    cs["K"][F + 2, 3 * H + 17] = value               # (a view of flat)
    assert abs(f32(value)) < 128.0 or flag
    status = torch.tensor([0, 12345], dtype=torch.int32, device=DEV)
    _, KpT2, Kb2 = refresh(cs, status)
    _, KpT2n, Kb2n = refresh(cs, None)
    torch.cuda.synchronize()
    assert status.tolist() == [flag, 12345]
    assert torch.equal(h16(KpT2), h16(KpT2n)) and torch.equal(h16(Kb2), h16(Kb2n))


@gpu
@pytest.mark.parametrize("H,B", [(64, 1), (128, 17), (64, 65)])
def test_carry_f32_zeroes_done_rows_and_copies_the_rest(hip_lib, H, B):
    """An exact select; done rows hold NaN that must not survive."""
    from pathnet_gym_amd.ops import _lib
    g = torch.Generator().manual_seed(H + B)
    hT, cT = torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)
    done = (torch.rand(B, generator=g) < 0.4).to(torch.uint8)
    done[0], done[B - 1] = 0, 1
    hT[done.bool()] = NAN
    cT[done.bool()] = NAN
    h0, c0 = outbuf(B, H), outbuf(B, H)
    hT_d, cT_d, done_d = padded(hT), padded(cT), padded(done[:, None], fill=0)
    _lib.call("launch_lstm_carry_f32", hT_d.data_ptr(), cT_d.data_ptr(), done_d.data_ptr(), h0.data_ptr(),
              c0.data_ptr(), H, B, _lib.stream())
    torch.cuda.synchronize()
    assert_sentinel(h0, B, "h0")
    assert_sentinel(c0, B, "c0")
    keep = done == 0
    assert torch.equal(bits(h0[:B].cpu()), bits(select_rows(keep, hT)))          # +0 bits in the done rows
    assert torch.equal(bits(c0[:B].cpu()), bits(select_rows(keep, cT)))


# ---------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("F,H,B", FWD_SHAPES)
def test_forward_matches_float64(hip_lib, F, H, B):
    """Random prev_done per row (NaN state in the reset rows), gates and xh saved, every batch edge."""
    cs = make_case(F, H, B, seed=1000 * F + 10 * H + B)
    out = run_forward(cs)
    check_forward(cs, out, ref_forward(cs))
    assert_scaled_column_fails(cs, out)


@gpu
@pytest.mark.parametrize("prev", [None, "zeros", "ones"])
@pytest.mark.parametrize("F,H,B", [(64, 128, 65), (128, 64, 17)])
def test_forward_prev_done_none_all_kept_all_reset(hip_lib, F, H, B, prev):
    cs = make_case(F, H, B, seed=7 + B, prev=prev)
    fw = ref_forward(cs)
    if prev == "ones":            # every row starts from a zero state: c = sig(i) tanh(j) whatever c held
        assert bool(torch.isnan(cs["c"]).all()) and bool((fw["ck"] == 0).all())
    out = run_forward(cs)
    check_forward(cs, out, fw)
    assert_scaled_column_fails(cs, out)


@gpu
@pytest.mark.parametrize("F,H,B", [(64, 128, 65), (128, 64, 17)])
def test_forward_without_gates_and_xh_and_with_padded_x(hip_lib, F, H, B):
    """The bootstrap step's launch (gates = xh = None: the amax slot stays untouched) and an x whose row stride is
    F + 8 (pad columns NaN) give the bits of the plain launch."""
    cs = make_case(F, H, B, seed=11 + B)
    fw = ref_forward(cs)
    full = run_forward(cs)
    check_forward(cs, full, fw)
    for kw in (dict(want_gates=False, want_xh=False), dict(ldx=F + 8), dict(ldx=F + 8, want_gates=False, want_xh=False)):
        out = run_forward(cs, **kw)
        check_forward(cs, out, fw)
        for name in ("hout", "cout", "gates", "xh"):
            if out[name] is not None:
                assert torch.equal(bits(out[name]), bits(full[name])), (kw, name)


@gpu
def test_forward_amax_keeps_a_larger_seed(hip_lib):
    """atomicMax: an amax slot holding more than max|xh| keeps its bits, with and without xh."""
    cs = make_case(64, 128, 65, seed=12)
    fw = ref_forward(cs)
    seed = f32(float(fw["xh"].abs().max()) * 1.0000002 + 1e-6)
    assert seed > float(fw["xh"].abs().max())
    for kw in (dict(), dict(want_gates=False, want_xh=False)):
        check_forward(cs, run_forward(cs, amax0=seed, **kw), fw)


@gpu
@pytest.mark.parametrize("F,H,B", [(64, 128, 65)])
def test_forward_saturated_gates_stay_finite(hip_lib, F, H, B):
    cs = make_case(F, H, B, seed=13 + B, sat=True)
    fw = ref_forward(cs)
    assert float(fw["z"].abs().min()) > 20 and float(fw["z"].abs().max()) < 45
    check_forward(cs, run_forward(cs), fw, tag="fwd_sat")


@gpu
@pytest.mark.parametrize("value,flag", [(65503.996, 0), (65504.0, 2), (-65504.0, 2), (INF, 2), (NAN, 2)])
def test_forward_status_word(hip_lib, value, flag):
    """Bit 1 (value 2): one x element at or beyond fp16's 65504, inf or NaN; the largest fp32 below 65504 passes."""
    F, H, B = 64, 64, 17
    cs = make_case(F, H, B, seed=14)
    assert (abs(f32(value)) < 65504.0) == (flag == 0)
    x = cs["x"].clone()
    x[B - 1, F - 3] = value
    assert run_forward(cs, x=x)["status"] == flag
    assert run_forward(cs, x=x, want_gates=False, want_xh=False)["status"] == flag


# ---------------------------------------------------------------------------------------------------------------
# backward, pointwise
# ---------------------------------------------------------------------------------------------------------------
def run_backward_point(cs, fw, mode, seed, plant=NAN, amax0=0.0):
    """mode "scan": dh_rec / dc_rec / done_t / prev_done all present (an interior step of the reverse scan);
    "last": no recurrent gradient and no done_t; "last_done": no recurrent gradient, done_t present (what the engine
    passes at step T-1); "first": recurrent gradient, prev_done = None (step 0).  ``plant`` fills dh_rec / dc_rec of
    the rows whose done_t is set."""
    from pathnet_gym_amd.ops import _lib
    H, B = cs["H"], cs["B"]
    g = torch.Generator().manual_seed(seed)
    dh_heads = torch.randn(B, H, generator=g)
    dh_rec = dc_rec = done_t = None
    if mode != "last":
        done_t = (torch.rand(B, generator=g) < 0.4).to(torch.uint8)
        done_t[0] = 0
        if B > 1:
            done_t[1] = 1
    if mode in ("scan", "first"):
        dh_rec, dc_rec = torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)
        dh_rec[done_t.bool()] = plant        # an ended episode's row never reads its recurrent gradient
        dc_rec[done_t.bool()] = -plant
    assert (cs["prev_done"] is None) == (mode == "first")
    dz_ref, dck_ref, e32 = ref_backward_point(cs, fw, dh_heads, dh_rec, dc_rec, done_t)
    # the kernel reads the activations the forward saved: here the float64 reference's, rounded to fp32
    dz, dc_out = outbuf(B, 4 * H), outbuf(B, H)
    args = [padded(t) if t is not None else None for t in (dh_heads, dh_rec, dc_rec)]
    dn = None if done_t is None else padded(done_t[:, None], fill=0).view(-1)
    pd = None if cs["prev_done"] is None else padded(cs["prev_done"][:, None], fill=1).view(-1)
    gates, c_t, c_prev = padded(fw["gates"].float()), padded(fw["c"].float()), padded(cs["c"])
    amax = torch.tensor([SENT, amax0, SENT], device=DEV)
    _lib.call("launch_lstm_bwd_point_x3", ptr(args[0]), ptr(args[1]), ptr(args[2]), ptr(dn), gates.data_ptr(),
              c_t.data_ptr(), c_prev.data_ptr(), ptr(pd), dz.data_ptr(), dc_out.data_ptr(), amax.data_ptr() + 4,
              H, B, _lib.stream())
    torch.cuda.synchronize()
    assert_sentinel(dz, B, "dz")
    assert_sentinel(dc_out, B, "dc_out")
    assert float(amax[0]) == SENT and float(amax[2]) == SENT
    # the slot is the amax of what was written, bit for bit, or the larger value it held
    assert bool(torch.isfinite(dz[:B]).all()), "bwd.dz: non-finite output"
    want = torch.maximum(dz[:B].abs().max(), torch.tensor(amax0, device=DEV)).reshape(1)
    assert torch.equal(bits(amax[1:2]), bits(want))
    return dz, dc_out, dz_ref, dck_ref, e32


@gpu
@pytest.mark.parametrize("mode,plant", [("scan", NAN), ("scan", INF), ("first", NAN), ("first", INF), ("last", NAN),
                                        ("last_done", NAN)],
                         ids=["scan-nan", "scan-inf", "first-nan", "first-inf", "last", "last_done"])
@pytest.mark.parametrize("F,H,B", [(64, 64, 15), (64, 128, 65), (128, 64, 130), (256, 256, 17)])
def test_backward_pointwise_matches_float64_autograd(hip_lib, F, H, B, mode, plant):
    """The rows whose done_t is set hold NaN, or +-inf, in dh_rec / dc_rec: a select never reads them (a product
    with 0 turns them into NaN in dz and dc_out, and from there in dx, dh_prev and the whole weight gradient)."""
    cs = make_case(F, H, B, seed=17 + B, prev=None if mode == "first" else "rand")
    dz, dc_out, dz_ref, dck_ref, e32 = run_backward_point(cs, ref_forward(cs), mode, seed=B, plant=plant)
    within("bwd.dz", dz[:B], dz_ref, torch.full_like(dz_ref, 8 * e32["dz"]))
    within("bwd.dc_out", dc_out[:B], dck_ref, torch.full_like(dck_ref, 8 * e32["dc_out"]))


@gpu
def test_backward_pointwise_amax_keeps_a_larger_seed(hip_lib):
    cs = make_case(64, 128, 65, seed=43)
    dz, _, dz_ref, _, e32 = run_backward_point(cs, ref_forward(cs), "scan", seed=3, plant=1.0, amax0=1000.0)
    assert float(dz[:65].abs().max()) < 1000.0
    within("bwd.dz", dz[:65], dz_ref, torch.full_like(dz_ref, 8 * e32["dz"]))


@gpu
def test_backward_pointwise_grid_stride_trip(hip_lib):
    """H = 64, B = 2049: one row more than the 512 x 256 threads of the launch; that row is written by a second trip
    of the grid-stride loop.  dz only."""
    H, B = 64, 2049
    cs = make_case(64, H, B, seed=47)
    dz, _, dz_ref, _, e32 = run_backward_point(cs, ref_forward(cs), "scan", seed=5, plant=1.0)
    assert B * H == 512 * 256 + H
    within("bwd.dz", dz[:B], dz_ref, torch.full_like(dz_ref, 8 * e32["dz"]))


# ---------------------------------------------------------------------------------------------------------------
# backward GEMM
# ---------------------------------------------------------------------------------------------------------------
def run_backward_gemm(cs, dz, amax):
    from pathnet_gym_amd.ops import _lib
    F, H, B = cs["F"], cs["H"], cs["B"]
    _, _, Kb2 = refresh(cs)
    lddx = F + 8
    dx, dh_prev = outbuf(B, lddx), outbuf(B, H)
    dz_d = padded(dz)
    am = torch.tensor([SENT, amax, SENT], device=DEV)
    assert float(am[1]) == amax
    _lib.call("launch_lstm_bwd_gemm_x3", dz_d.data_ptr(), Kb2.data_ptr(), dx.data_ptr(), lddx, dh_prev.data_ptr(),
              am.data_ptr() + 4, F, H, B, _lib.stream())
    torch.cuda.synchronize()
    assert_sentinel(dx, B, "dx")
    assert_sentinel(dh_prev, B, "dh_prev")
    assert bool((dx[:, F:] == SENT).all()), "dx pad columns were written"
    assert am.tolist() == [SENT, amax, SENT]
    return dx[:B, :F], dh_prev[:B]


def check_backward_gemm(cs, dz, amax, dx, dh_prev, rows=None, tag=""):
    F = cs["F"]
    ref, _, bound = ref_backward_gemm(cs, dz, amax)
    rows = slice(None) if rows is None else rows
    both(f"dx{tag}", dx[rows], ref[rows, :F], bound[rows, :F])
    both(f"dh_prev{tag}", dh_prev[rows], ref[rows, F:], bound[rows, F:])


@gpu
@pytest.mark.parametrize("F,H,B", FWD_SHAPES)
def test_backward_gemm_matches_float64(hip_lib, F, H, B):
    cs = make_case(F, H, B, seed=19 + B)
    dz = rand_dz(torch.Generator().manual_seed(23 + B), B, 4 * H)
    amax = amax_of(dz)
    dx, dh_prev = run_backward_gemm(cs, dz, amax)
    check_backward_gemm(cs, dz, amax, dx, dh_prev)
    # negative controls: the whole kernel of the reference scaled by 1.02, then (B > 1: a single entry may be near
    # zero) only its row 5 (a dx column) and row F + 5 (a dh_prev column)
    ref, _, bound = ref_backward_gemm(dict(cs, K=cs["K"] * 1.02), dz, amax)
    assert float(excess(dx, ref[:, :F], bound[:, :F]).max()) > 1.0
    assert float(excess(dh_prev, ref[:, F:], bound[:, F:]).max()) > 1.0
    assert rel(dx, ref[:, :F]) > X3_LAYER_TOL and rel(dh_prev, ref[:, F:]) > X3_LAYER_TOL
    if B > 1:
        K = cs["K"].clone()
        K[5] *= 1.02
        K[F + 5] *= 1.02
        ref, _, bound = ref_backward_gemm(dict(cs, K=K), dz, amax)
        assert float(excess(dx[:, 5], ref[:, 5], bound[:, 5]).mean()) > 1.0
        assert float(excess(dh_prev[:, 5], ref[:, F + 5], bound[:, F + 5]).mean()) > 1.0
        assert rel(dx, ref[:, :F]) > X3_LAYER_TOL and rel(dh_prev, ref[:, F:]) > X3_LAYER_TOL


@gpu
@pytest.mark.parametrize("stale", STALE)
@pytest.mark.parametrize("scale", DZ_SCALES)
@pytest.mark.parametrize("F,H,B", [(64, 128, 65), (128, 64, 17)])
def test_backward_gemm_g16_scales(hip_lib, F, H, B, scale, stale):
    """dz at 2^-30 ... 2^10 of its usual magnitude, the amax slot exact or 8 x too large (a stale larger slot is
    allowed): the accuracy class holds at every scale."""
    cs = make_case(F, H, B, seed=53 + B)
    dz = rand_dz(torch.Generator().manual_seed(59 + B), B, 4 * H) * scale
    amax = f32(amax_of(dz) * stale)
    dx, dh_prev = run_backward_gemm(cs, dz, amax)
    check_backward_gemm(cs, dz, amax, dx, dh_prev, tag=".scaled")


@gpu
def test_backward_gemm_of_zero_dz_is_exactly_zero(hip_lib):
    F, H, B = 64, 128, 65
    cs = make_case(F, H, B, seed=61)
    dx, dh_prev = run_backward_gemm(cs, torch.zeros(B, 4 * H), 0.0)
    assert bool((dx == 0).all()) and bool((dh_prev == 0).all())


@gpu
def test_backward_gemm_non_finite_dz_stays_in_its_row(hip_lib):
    """One NaN and one inf in dz make dx / dh_prev of their rows non-finite (the optimizer's skip relies on it) and
    leave every other row within the bound."""
    F, H, B = 64, 128, 65
    cs = make_case(F, H, B, seed=67)
    dz = rand_dz(torch.Generator().manual_seed(71), B, 4 * H)
    amax = amax_of(dz)
    dz[3, 2 * H + 5] = NAN
    dz[B - 1, 77] = INF
    dx, dh_prev = run_backward_gemm(cs, dz, amax)
    for r in (3, B - 1):
        assert not bool(torch.isfinite(dx[r]).any()) and not bool(torch.isfinite(dh_prev[r]).any()), r
    rows = torch.tensor([r for r in range(B) if r not in (3, B - 1)])
    check_backward_gemm(cs, dz, amax, dx.cpu(), dh_prev.cpu(), rows=rows, tag=".nonfinite")


# ---------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------
def wgrad_cases():
    out = []
    for rpc in (32, 64):
        F, H = (128, 64) if rpc == 64 else (64, 128)
        for R in (1, 31, 33, rpc, rpc + 1, 2 * rpc + 7):
            out.append((F, H, R, rpc))
    return out + [(64, 128, 130, 2048), (256, 256, 130, 2048)]


def wgrad_inputs(cs, R, T, seed, start="random"):
    """R rows of xh and dz, grad0 (zero or random), and the amax slots: one for xh, one per step for dz.  T = 3: the rows
    of step t are scaled by STEP_SCALES[t] and slot t holds that step's own amax (0 for a step without rows)."""
    F, H = cs["F"], cs["H"]
    g = torch.Generator().manual_seed(seed)
    xh, dz = rand_xh(g, R, F, H), rand_dz(g, R, 4 * H)
    g0 = torch.randn(cs["flat"].numel(), generator=g) * 0.05
    if start == "zero":
        ks, bs, _ = segments(cs)
        g0[ks] = 0.0
        g0[bs] = 0.0
    step = step_of_rows(R, T)
    if T > 1:
        dz = dz * torch.tensor(STEP_SCALES)[step][:, None]
    slots = [amax_of(dz[step == t]) for t in range(T)]
    return xh, dz, g0, amax_of(xh), slots


def run_wgrad(cs, xh, dz, g0, R, rpc, amax_xh, slots, det=False):
    """Atomic mode, or (det) the int64 fixed-point route: x3_set_fx -> launch -> x3_fx_flush.  -> grad (CPU) and,
    det, the guard word fx[-1] read after the launch (and cleared before the flush)."""
    from pathnet_gym_amd.ops import _lib
    F, H = cs["F"], cs["H"]
    xh_d, dz_d = padded(xh), padded(dz)              # NaN rows after R
    grad = g0.to(DEV)
    am = torch.tensor([SENT, amax_xh] + slots + [SENT], device=DEV)
    T = len(slots)
    args = (xh_d.data_ptr(), dz_d.data_ptr(), grad.data_ptr(), cs["k_off"], cs["b_off"], F, H, R, rpc,
            am.data_ptr() + 8, T, am.data_ptr() + 4, _lib.stream())
    guard = None
    if det:
        fx = torch.zeros(g0.numel() + 1, dtype=torch.int64, device=DEV)
        _lib.call("x3_set_fx", fx.data_ptr() + 8)
        try:
            _lib.call("launch_lstm_wgrad_x3", *args)
        finally:
            _lib.call("x3_set_fx", None)
        torch.cuda.synchronize()
        guard = int(fx[0])
        fx[0] = 0                                    # (a set guard word would raise the process-wide range flag)
        _lib.call("x3_fx_flush", fx.data_ptr() + 8, grad.data_ptr(), 0, g0.numel(), _lib.stream())
        torch.cuda.synchronize()
        assert int(fx.abs().sum()) == 0, "the flush left accumulator entries behind"
    else:
        _lib.call("launch_lstm_wgrad_x3", *args)
        torch.cuda.synchronize()
    assert am.tolist() == [SENT, f32(amax_xh)] + [f32(s) for s in slots] + [SENT]
    return grad.cpu(), guard


def segments(cs):
    KK, G4 = cs["F"] + cs["H"], 4 * cs["H"]
    ks, bs = slice(cs["k_off"], cs["k_off"] + KK * G4), slice(cs["b_off"], cs["b_off"] + G4)
    outside = torch.ones(cs["flat"].numel(), dtype=torch.bool)
    outside[ks] = False
    outside[bs] = False
    return ks, bs, outside


def check_wgrad(cs, xh, dz, g0, grad, amax_xh, slots, rpc, det, skip_cols=(), control=True):
    """The increment against float64 with bound (a) + the adds into the running value, the bits outside the two
    segments, and the 2 % negative control on column 6.  Criterion (b) on dK where grad0 is zero in the segment: the
    rounding of an fp32 add into a grad0 of 0.05 is no part of the GEMM's accuracy, and at the small step scales it
    alone exceeds 2e-5 of the increment."""
    KK, G4 = cs["F"] + cs["H"], 4 * cs["H"]
    R = xh.shape[0]
    nchunks = -(-R // rpc)
    ks, bs, outside = segments(cs)
    assert torch.equal(bits(grad)[outside], bits(g0)[outside])
    dK, _, bK, db, bb = ref_wgrad(xh, dz, amax_xh, max(slots))
    absK = xh.double().abs().t() @ dz.double().abs()
    if det:     # per chunk one quantisation to 2^-34; the flush converts (one rounding) and adds once
        adds, quant = 2 * 2.0 ** -24 * 1.001, nchunks * 2.0 ** -35
    else:       # one atomic add per chunk
        adds, quant = nchunks * 2.0 ** -24 * 1.001, 0.0
    bK = bK + adds * (g0[ks].view(KK, G4).abs().double() + absK) + quant
    bb = bb + adds * (g0[bs].abs().double() + dz.double().abs().sum(0)) + quant
    keep = torch.ones(G4, dtype=torch.bool)
    for c in skip_cols:
        keep[c] = False
    incK = (grad[ks].double() - g0[ks].double()).view(KK, G4)
    incb = grad[bs].double() - g0[bs].double()
    tag = ".det" if det else ""
    within(f"dK{tag}", incK[:, keep], dK[:, keep], bK[:, keep])
    zero_start = not bool(g0[ks].any())
    if zero_start:
        accurate(f"dK{tag}", incK[:, keep], dK[:, keep])
    within(f"db{tag}", incb[keep], db[keep], bb[keep])
    if control and R > 1:
        dz2 = dz.clone()
        dz2[:, 6] *= 1.02
        dK2, _, _, db2, _ = ref_wgrad(xh, dz2, amax_xh, max(slots))
        assert float(excess(incK[:, 6], dK2[:, 6], bK[:, 6]).max()) > 1.0
        assert float(excess(incb[6], db2[6], bb[6])) > 1.0
        assert not zero_start or rel(incK, dK2) > X3_LAYER_TOL


@gpu
@pytest.mark.parametrize("start", ["zero", "random"])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("F,H,R,rpc", wgrad_cases())
def test_wgrad_atomic_increment_matches_float64(hip_lib, F, H, R, rpc, T, start):
    """The kernel accumulates into grad, zero or not, in its two segments: the increment is compared.  Chunks whose last 32-row
    block is partial, R < 32, one chunk and several; one amax slot, or three that differ by 2^10 from step to step."""
    cs = make_case(F, H, 1, seed=37 + R + rpc)
    xh, dz, g0, amax_xh, slots = wgrad_inputs(cs, R, T, seed=41 + R, start=start)
    grad, _ = run_wgrad(cs, xh, dz, g0, R, rpc, amax_xh, slots)
    check_wgrad(cs, xh, dz, g0, grad, amax_xh, slots, rpc, det=False)


@gpu
@pytest.mark.parametrize("start", ["zero", "random"])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("F,H,R,rpc", wgrad_cases())
def test_wgrad_deterministic_matches_float64_and_repeats_bit_for_bit(hip_lib, F, H, R, rpc, T, start):
    """The int64 fixed-point route: the same bound plus the quantisation, the guard word clear, three runs one set of
    bits."""
    cs = make_case(F, H, 1, seed=37 + R + rpc)
    xh, dz, g0, amax_xh, slots = wgrad_inputs(cs, R, T, seed=41 + R, start=start)
    grad, guard = run_wgrad(cs, xh, dz, g0, R, rpc, amax_xh, slots, det=True)
    assert guard == 0
    check_wgrad(cs, xh, dz, g0, grad, amax_xh, slots, rpc, det=True)
    for _ in range(2):
        again, guard = run_wgrad(cs, xh, dz, g0, R, rpc, amax_xh, slots, det=True)
        assert guard == 0 and torch.equal(bits(again), bits(grad))


@gpu
def test_wgrad_deterministic_nan_stays_in_the_entries_it_feeds(hip_lib):
    """One NaN in dz[r][p]: column p of dK and db[p] are NaN (a non-finite update, not a range error), every other
    entry is within its bound."""
    F, H, R, rpc = 64, 128, 71, 32
    cs = make_case(F, H, 1, seed=73)
    xh, dz, g0, amax_xh, slots = wgrad_inputs(cs, R, 1, seed=79, start="zero")
    p = 2 * H + 9
    dz[40, p] = NAN
    grad, guard = run_wgrad(cs, xh, dz, g0, R, rpc, amax_xh, slots, det=True)
    assert guard == 0
    ks, bs, _ = segments(cs)
    assert bool(torch.isnan(grad[ks].view(F + H, 4 * H)[:, p]).all()) and bool(torch.isnan(grad[bs][p]))
    check_wgrad(cs, xh, dz, g0, grad, amax_xh, slots, rpc, det=True, skip_cols=(p,), control=False)


@gpu
def test_wgrad_deterministic_range_guard(hip_lib):
    """A finite contribution of magnitude >= 65536 (300 x 300) cannot be quantised: bit 0 of the guard word fx[-1] is
    set and the entry becomes NaN; without it the word stays clear."""
    F, H, R, rpc = 64, 64, 1, 32
    cs = make_case(F, H, 1, seed=83)
    xh, dz, g0, _, _ = wgrad_inputs(cs, R, 1, seed=89)
    xh[0, 5], dz[0, 9] = 300.0, 300.0
    grad, guard = run_wgrad(cs, xh, dz, g0, R, rpc, amax_of(xh), [amax_of(dz)], det=True)
    assert guard & 1
    ks, _, _ = segments(cs)
    gk = grad[ks].view(F + H, 4 * H)
    assert bool(torch.isnan(gk[5, 9])) and int(torch.isnan(grad).sum()) == 1
    xh[0, 5] = 200.0                                 # 60000: in range
    grad, guard = run_wgrad(cs, xh, dz, g0, R, rpc, amax_of(xh), [amax_of(dz)], det=True)
    assert guard == 0 and bool(torch.isfinite(grad).all())


# ---------------------------------------------------------------------------------------------------------------
# launcher contract: a bad argument returns its code and launches nothing
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_launchers_reject_bad_arguments(hip_lib):
    from pathnet_gym_amd.ops import _lib
    lib = hip_lib
    s = _lib.stream()
    # real, zero-filled buffers larger than any shape below, entered in the middle (negative offsets stay inside)
    buf = torch.zeros(1 << 20, device=DEV)
    p = buf.data_ptr() + (1 << 21)
    fwd = lambda ldx, F, H, B, b_off=0: lib.launch_lstm_fwd_x3(p, ldx, p, p, None, p, p, b_off, p, p, p, p, p, p,  # noqa
                                                              F, H, B, s)
    assert fwd(64, 64, 96, 16) == -1 and fwd(96, 96, 64, 16) == -1 and fwd(68, 64, 64, 16) == -1
    assert fwd(64, 128, 64, 16) == -1                                  # a row stride below F
    assert fwd(0, 64, 64, 16) == -22 and fwd(64, 0, 64, 16) == -22 and fwd(64, 64, -64, 16) == -22
    assert fwd(64, 64, 64, 0) == -22 and fwd(64, 64, 64, 16, b_off=-1) == -22
    point = lambda H, B, am=p: lib.launch_lstm_bwd_point_x3(p, p, p, None, p, p, p, None, p, p, am, H, B, s)     # noqa
    assert point(0, 16) == -22 and point(64, -3) == -22 and point(64, 16, am=None) == -22
    gemm = lambda lddx, F, H, B, am=p: lib.launch_lstm_bwd_gemm_x3(p, p, p, lddx, p, am, F, H, B, s)             # noqa
    assert gemm(64, 64, 32, 16) == -1 and gemm(160, 160, 64, 16) == -1 and gemm(64, 128, 64, 16) == -1
    assert gemm(0, 64, 64, 16) == -22 and gemm(64, 64, 64, -1) == -22 and gemm(64, -64, 64, 16) == -22
    assert gemm(64, 64, 0, 16) == -22 and gemm(64, 64, 64, 16, am=None) == -22
    wg = lambda F, H, R, rpc, k_off=0, b_off=0, T=1, am=p, ax=p: lib.launch_lstm_wgrad_x3(                       # noqa
        p, p, p, k_off, b_off, F, H, R, rpc, am, T, ax, s)
    assert wg(64, 64, 32, 48) == -1 and wg(64, 65, 32, 32) == -1 and wg(32, 64, 32, 32) == -1
    assert wg(64, 64, 0, 32) == -22 and wg(64, 64, 32, 0) == -22 and wg(64, 64, 32, 32, k_off=-1) == -22
    assert wg(64, 64, 32, 32, b_off=-5) == -22 and wg(0, 64, 32, 32) == -22 and wg(64, -64, 32, 32) == -22
    assert wg(64, 64, 32, 32, T=0) == -22 and wg(64, 64, 32, 32, am=None) == -22
    assert wg(64, 64, 32, 32, ax=None) == -22
    ref = lambda k_off, F, H: lib.launch_lstm_refresh_x3(p, k_off, F, H, p, p, p, s)                              # noqa
    assert ref(0, 64, 72) == -1 and ref(0, 96, 64) == -1      # H % 16 != 0 would permute past KpT2's 4H rows
    assert ref(-1, 64, 64) == -22 and ref(0, 0, 64) == -22 and ref(0, 64, 0) == -22
    carry = lambda H, B: lib.launch_lstm_carry_f32(p, p, p, p, p, H, B, s)                                        # noqa
    assert carry(0, 16) == -22 and carry(64, 0) == -22 and carry(-64, 16) == -22
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0            # nothing ran
