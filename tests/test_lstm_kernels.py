"""csrc/lstm.hip, launcher by launcher, against plain float64 torch with buffers of the test's own.

The kernels are called through ``ops/_lib.call`` on a synthetic ``flat`` buffer (no model), so F != H and odd
``k_off`` / ``b_off`` are covered.  The float64 reference is fed the operands the kernel multiplies: ``K``, ``x``,
``h`` and, in the two backward GEMMs, ``dz`` are rounded to bf16 (round to nearest even, what ``(__bf16)`` compiles
to) and widened to float64.  A bf16 x bf16 product is exact in fp32, so all that separates a GEMM output from
float64 is the fp32 summation, and its tolerance is derived, not measured:

    |hip - ref64| <= n * 2^-23 * (|A| @ |B|)          n = reduction length

(2^-23 and not 2^-24: the bound then holds whatever rounding the MFMA uses inside its accumulation).  The bias
gradient sums the UNROUNDED fp32 dz, in the kernel and here.

Pointwise outputs (gates, cout, dz, dc_out) go through ``__expf``, which is not torch's ``exp``: their tolerance is
``L * dz_bound + 8 * e32``, e32 = the max abs error of a torch fp32 evaluation of the same formulas against float64
on the same inputs, L the Lipschitz constant that carries the pre-activation bound through the gate (1/4 sigmoid,
1 tanh).  The measured ratios max|hip - ref64| / e32 are recorded under ``lstm_kernels_f64`` in
tests/data/numerics_measured.json (``PATHNET_RECORD_NUMERICS``).  hout (bf16) adds 2^-8 |h64|: one rounding flip.

Every output buffer carries 64 extra rows of a sentinel that must survive; every input carries 64 extra rows of NaN.
"""
import json
import os

import pytest
import torch

import numerics_budget as budget
from pathnet_gym_amd.models.pathnet import lstm_cell_ref

gpu = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -23
TINY = 2.0 ** -126                 # smallest normal fp32
PAD = 64                           # sentinel rows after every buffer
SENT = -3.0                        # exact in bf16 and fp32
NAN = float("nan")
SMALL_FH = [(64, 64), (64, 128), (128, 64)]
ALL_FH = SMALL_FH + [(256, 256)]
BATCHES = [1, 15, 16, 17, 63, 64, 65, 130]          # the 16-row wave and 64-row workgroup edges
FWD_SHAPES = [(F, H, B) for F, H in SMALL_FH for B in BATCHES] + [(256, 256, 17), (256, 256, 130)]


# ---------------------------------------------------------------------------------------------------------------
# float64 reference (CPU tensors; also run by the CPU test below)
# ---------------------------------------------------------------------------------------------------------------
def bf(x):
    return x.to(torch.bfloat16)


def gemm_bound(A, B, n):
    """The derived elementwise bound of an fp32-accumulated GEMM of exactly representable products."""
    return n * EPS * (A.abs().double() @ B.abs().double())


def select_rows(keep, v):
    """v where keep, else 0 -- a select, so whatever the dropped rows hold (NaN here) never enters the arithmetic."""
    return v if keep is None else torch.where(keep[:, None], v, torch.zeros_like(v))


def cell_from_z(z, c0):
    """TF BasicLSTMCell pointwise part (gate order i, j, f, o; forget_bias 1) in the dtype of ``z``:
    -> gates [B, 4H] (sig i, tanh j, sig(f + 1), sig o), c, h."""
    i, j, f, o = z.chunk(4, 1)
    si, tj, sf, so = torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + 1.0), torch.sigmoid(o)
    c = c0 * sf + si * tj
    h = torch.tanh(c) * so
    return torch.cat([si, tj, sf, so], 1), c, h


def bwd_pointwise(dh_heads, dh_rec, dc_rec, keep_t, gates, c_t, c0):
    """The closed-form gate gradients of one cell step from its saved activations, in the dtype of the inputs:
    upstream dh_heads + keep_t * dh_rec on h and keep_t * dc_rec on c  ->  dz [B, 4H], d(c0)."""
    si, tj, sf, so = gates.chunk(4, 1)
    dh = dh_heads if dh_rec is None else dh_heads + select_rows(keep_t, dh_rec)
    tc = torch.tanh(c_t)
    dc = dh * so * (1.0 - tc * tc)
    if dc_rec is not None:
        dc = select_rows(keep_t, dc_rec) + dc
    dz = torch.cat([dc * tj * si * (1.0 - si), dc * si * (1.0 - tj * tj), dc * c0 * sf * (1.0 - sf),
                    dh * tc * so * (1.0 - so)], 1)
    return dz, dc * sf


def make_case(F, H, B, seed, prev="rand", sat=False):
    """Synthetic weights + one step's inputs (CPU).  k_off / b_off are non-zero and odd; rows whose prev_done is set
    hold NaN in h and c: the cell must see zeros there without ever touching them."""
    g = torch.Generator().manual_seed(seed)
    KK, G4 = F + H, 4 * H
    k_off = 37
    b_off = k_off + KK * G4 + 11
    flat = torch.randn(b_off + G4 + 29, generator=g) * 0.1
    bias = torch.randn(G4, generator=g) * 0.5
    if sat:   # pre-activations around +-30: every gate saturated, either way
        bias = torch.where(torch.rand(G4, generator=g) < 0.5, -30.0, 30.0) + torch.randn(G4, generator=g)
    flat[b_off:b_off + G4] = bias
    x = bf(torch.randn(B, F, generator=g) * 0.5)
    h = bf(torch.randn(B, H, generator=g) * 0.5)
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


def ref_forward(cs):
    """float64 forward of a case + the tolerances of every forward output (module docstring)."""
    F, H = cs["F"], cs["H"]
    keep = None if cs["prev_done"] is None else cs["prev_done"] == 0
    hk, ck = select_rows(keep, cs["h"]), select_rows(keep, cs["c"])
    xh = torch.cat([cs["x"], hk], 1)
    A, Kq = xh.double(), bf(cs["K"]).double()
    acc = A @ Kq
    dz = gemm_bound(A, Kq, F + H)
    gates, c, h = cell_from_z(acc + cs["b"].double(), ck.double())
    g32, c32, h32 = cell_from_z(acc.float() + cs["b"], ck)             # torch fp32 on the same inputs
    e32 = {"gates": float((g32 - gates).abs().max()), "cout": float((c32 - c).abs().max()),
           "hout": float((h32 - h).abs().max())}
    di, dj, df, do = dz.chunk(4, 1)
    dg = torch.cat([di / 4, dj, df / 4, do / 4], 1)                    # |sig'| <= 1/4, |tanh'| <= 1
    dc = ck.double().abs() * df / 4 + di / 4 + dj                      # c = c0 sig(f) + sig(i) tanh(j), |.| <= 1
    dh = dc + do / 4                                                   # h = tanh(c) sig(o)
    tol = {"gates": dg + 8 * e32["gates"], "cout": dc + 8 * e32["cout"],
           "hout": 2.0 ** -8 * h.abs() + dh + 8 * e32["hout"]}
    return dict(xh=xh, acc=acc, z=acc + cs["b"].double(), ck=ck, gates=gates, c=c, h=h, e32=e32, tol=tol)


def ref_backward_point(cs, fw, dh_heads, dh_rec, dc_rec, done_t):
    """float64 autograd of one cell step (upstream dh_heads + keep_t dh_rec on h, keep_t dc_rec on c) -> dz, the
    gradient of the (masked) previous cell state, and e32 of the closed form evaluated in fp32 on the saved
    fp32 activations the kernel is given."""
    keep_t = None if done_t is None else done_t == 0
    z = fw["z"].clone().requires_grad_(True)
    ck = fw["ck"].double().clone().requires_grad_(True)
    _, c, h = cell_from_z(z, ck)
    gh = dh_heads.double() if dh_rec is None else dh_heads.double() + select_rows(keep_t, dh_rec).double()
    loss = (h * gh).sum()
    if dc_rec is not None:
        loss = loss + (c * select_rows(keep_t, dc_rec).double()).sum()
    loss.backward()
    dz32, dc32 = bwd_pointwise(dh_heads, dh_rec, dc_rec, keep_t, fw["gates"].float(), fw["c"].float(), fw["ck"])
    e32 = {"dz": float((dz32 - z.grad).abs().max()), "dc_out": float((dc32 - ck.grad).abs().max())}
    return z.grad, ck.grad, e32


def ref_wgrad(xh, dz):
    """float64 weight / bias gradient of R rows and their summation bounds (n = R); dz enters the GEMM rounded to
    bf16 and the bias sum unrounded, as in the kernel."""
    R = xh.shape[0]
    A, Bq = xh.double().t(), bf(dz).double()
    return A @ Bq, gemm_bound(A, Bq, R), dz.double().sum(0), R * EPS * dz.double().abs().sum(0)


# ---------------------------------------------------------------------------------------------------------------
# CPU: the reference and the bound, checked on any machine
# ---------------------------------------------------------------------------------------------------------------
def test_reference_helpers_and_gemm_bound_cpu():
    for (F, H, B), prev in (((64, 128, 70), "rand"), ((128, 64, 17), None), ((256, 256, 96), "rand")):
        cs = make_case(F, H, B, seed=F + B, prev=prev)
        fw = ref_forward(cs)
        keep = None if cs["prev_done"] is None else cs["prev_done"] == 0
        Kq = bf(cs["K"]).double().requires_grad_(True)
        bb = cs["b"].double().requires_grad_(True)
        x = cs["x"].double().requires_grad_(True)
        hk = select_rows(keep, cs["h"]).double().requires_grad_(True)
        ck = fw["ck"].double().requires_grad_(True)
        h2, c2 = lstm_cell_ref(x, hk, ck, Kq, bb)
        assert torch.allclose(h2, fw["h"], rtol=0, atol=1e-13) and torch.allclose(c2, fw["c"], rtol=0, atol=1e-13)
        assert torch.isfinite(fw["h"]).all() and torch.isfinite(fw["c"]).all()       # the planted NaN never got in
        # backward: autograd through the reference helper == the closed form in float64 == autograd of lstm_cell_ref
        g = torch.Generator().manual_seed(5)
        dh_heads, dh_rec, dc_rec = (torch.randn(B, H, generator=g) for _ in range(3))
        done_t = (torch.rand(B, generator=g) < 0.4).to(torch.uint8)
        dh_rec[done_t.bool()] = NAN
        dc_rec[done_t.bool()] = NAN
        dz, dck, e32 = ref_backward_point(cs, fw, dh_heads, dh_rec, dc_rec, done_t)
        keep_t = done_t == 0
        dz_cf, dck_cf = bwd_pointwise(dh_heads.double(), dh_rec.double(), dc_rec.double(), keep_t, fw["gates"],
                                      fw["c"], fw["ck"].double())
        assert torch.allclose(dz, dz_cf, rtol=0, atol=1e-13) and torch.allclose(dck, dck_cf, rtol=0, atol=1e-13)
        gh = dh_heads.double() + select_rows(keep_t, dh_rec).double()
        ((h2 * gh).sum() + (c2 * select_rows(keep_t, dc_rec).double()).sum()).backward()
        assert torch.allclose(ck.grad, dck, rtol=0, atol=1e-13)
        assert torch.allclose(bb.grad, dz.sum(0), rtol=0, atol=1e-11)
        assert torch.allclose(Kq.grad, torch.cat([x, hk], 1).detach().t() @ dz, rtol=0, atol=1e-11)
        assert torch.allclose(torch.cat([x.grad, hk.grad], 1), dz @ Kq.detach().t(), rtol=0, atol=1e-12)
        assert 0 < e32["dz"] < 1e-5 and 0 < e32["dc_out"] < 1e-5
        for k in ("gates", "cout", "hout"):
            assert 0 < fw["e32"][k] < 1e-5
        # the derived bound holds, with room, for an fp32 matmul of the same bf16 operands
        A, Kq = fw["xh"].double(), Kq.detach()
        err = (fw["xh"].float() @ bf(cs["K"]).float()).double() - A @ Kq
        bound = gemm_bound(A, Kq, F + H)
        assert (err.abs() <= bound).all() and float((err.abs() / bound).max()) < 0.05
    # ... and it is tight enough to see one row of R = 357 missing from a weight gradient
    g = torch.Generator().manual_seed(9)
    xh, dz = bf(torch.randn(357, 192, generator=g) * 0.5), torch.randn(357, 512, generator=g) * 0.1
    dK, bK, db, bb_ = ref_wgrad(xh, dz)
    dK32 = (xh.float().t() @ bf(dz).float()).double()
    assert ((dK32 - dK).abs() <= bK).all() and ((dz.sum(0).double() - db).abs() <= bb_).all()
    short = (xh[:-1].float().t() @ bf(dz[:-1]).float()).double()
    assert float(((short - dK).abs() > bK).double().mean()) > 0.9
    assert float(((dz[:-1].sum(0).double() - db).abs() > bb_).double().mean()) > 0.9


# ---------------------------------------------------------------------------------------------------------------
# GPU plumbing
# ---------------------------------------------------------------------------------------------------------------
def padded(t, fill=NAN, cols=None):
    """[B, C] CPU input -> [B + PAD, cols or C] on the GPU; the extra rows and columns hold ``fill``."""
    out = torch.full((t.shape[0] + PAD, cols or t.shape[1]), fill, dtype=t.dtype)
    out[:t.shape[0], :t.shape[1]] = t
    return out.to(DEV)


def outbuf(rows, cols, dtype=torch.float32):
    return torch.full((rows + PAD, cols), SENT, dtype=dtype, device=DEV)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def assert_sentinel(buf, rows, name):
    assert bool((buf[rows:] == SENT).all()), f"{name}: rows >= {rows} were written"


def ptr(t):
    return None if t is None else t.data_ptr()


def record_ratios(ratios):
    """PATHNET_RECORD_NUMERICS=<file>: keep the max of max|hip - ref64| / e32 per tensor under lstm_kernels_f64."""
    rec = os.environ.get("PATHNET_RECORD_NUMERICS")
    if not rec:
        return
    d = budget._load(rec)
    t = d.setdefault("lstm_kernels_f64", {})
    for k, v in ratios.items():
        t[k] = max(float(v), float(t.get(k, 0.0)))
    os.makedirs(os.path.dirname(rec) or ".", exist_ok=True)
    with open(rec, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def within(name, got, ref, tol, e32=None):
    err = (got.double().cpu() - ref).abs()
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    worst = float((err / tol.clamp_min(1e-300)).max())
    if e32 is not None:
        print(f"{name}: max|hip - ref64| / e32 = {float(err.max()) / e32:.3f}, worst err / tol = {worst:.3f}")
        record_ratios({name: float(err.max()) / e32})
    else:
        print(f"{name}: worst err / bound = {worst:.4f}")
    assert bool((err <= tol).all()), (name, worst, int((err > tol).sum()), err.numel())


def refresh(cs):
    from pathnet_gym_amd.ops import _lib
    F, H = cs["F"], cs["H"]
    flat = cs["flat"].to(DEV)
    KpT, Kb = outbuf(4 * H, F + H, torch.bfloat16), outbuf(F + H, 4 * H, torch.bfloat16)
    _lib.call("launch_lstm_refresh", flat.data_ptr(), cs["k_off"], F, H, KpT.data_ptr(), Kb.data_ptr(), _lib.stream())
    return flat, KpT, Kb


def run_forward(cs, want_gates=True, want_xh=True, ldx=None):
    from pathnet_gym_amd.ops import _lib
    F, H, B = cs["F"], cs["H"], cs["B"]
    flat, KpT, _ = refresh(cs)
    X = padded(cs["x"], cols=ldx)                                     # ldx > F: the pad columns hold NaN
    hp, cp = padded(cs["h"]), padded(cs["c"])
    pd = None if cs["prev_done"] is None else padded(cs["prev_done"][:, None], fill=1).view(-1)
    hout, cout = outbuf(B, H, torch.bfloat16), outbuf(B, H)
    gates = outbuf(B, 4 * H) if want_gates else None
    xh = outbuf(B, F + H, torch.bfloat16) if want_xh else None
    _lib.call("launch_lstm_fwd", X.data_ptr(), X.shape[1], hp.data_ptr(), cp.data_ptr(), ptr(pd), KpT.data_ptr(),
              flat.data_ptr(), cs["b_off"], hout.data_ptr(), cout.data_ptr(), ptr(gates), ptr(xh), F, H, B,
              _lib.stream())
    torch.cuda.synchronize()
    return dict(hout=hout, cout=cout, gates=gates, xh=xh)


def check_forward(cs, out, fw, tag="fwd"):
    B = cs["B"]
    for name in ("hout", "cout", "gates", "xh"):
        if out[name] is not None:
            assert_sentinel(out[name], B, name)
    if out["xh"] is not None:     # [x | h * keep], bit for bit
        assert torch.equal(bits(out["xh"][:B].cpu()), bits(fw["xh"]))
    if out["gates"] is not None:
        within(f"{tag}.gates", out["gates"][:B], fw["gates"], fw["tol"]["gates"], fw["e32"]["gates"])
    within(f"{tag}.cout", out["cout"][:B], fw["c"], fw["tol"]["cout"], fw["e32"]["cout"])
    within(f"{tag}.hout", out["hout"][:B], fw["h"], fw["tol"]["hout"])


# ---------------------------------------------------------------------------------------------------------------
# refresh / carry
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("F,H", ALL_FH)
def test_refresh_permutation_is_bit_exact(hip_lib, F, H):
    """Kb == bf16(K); KpT[(u/16)*64 + g*16 + u%16][n] == bf16(K[n][g*H + u])."""
    cs = make_case(F, H, 1, seed=F + 3 * H)
    _, KpT, Kb = refresh(cs)
    torch.cuda.synchronize()
    Kq = bf(cs["K"])
    assert_sentinel(KpT, 4 * H, "KpT")
    assert_sentinel(Kb, F + H, "Kb")
    assert torch.equal(bits(Kb[:F + H].cpu()), bits(Kq))
    want = torch.full((4 * H, F + H), SENT, dtype=torch.bfloat16)
    for gate in range(4):
        for u in range(H):
            want[(u // 16) * 64 + gate * 16 + u % 16] = Kq[:, gate * H + u]
    assert torch.equal(bits(KpT[:4 * H].cpu()), bits(want))


@gpu
@pytest.mark.parametrize("H,B", [(64, 15), (128, 17), (256, 130)])
def test_carry_zeroes_done_rows_and_copies_the_rest(hip_lib, H, B):
    """B is no multiple of the 256 / H rows a block covers; done rows hold NaN that must not survive."""
    from pathnet_gym_amd.ops import _lib
    g = torch.Generator().manual_seed(H + B)
    hT, cT = bf(torch.randn(B, H, generator=g)), torch.randn(B, H, generator=g)
    done = (torch.rand(B, generator=g) < 0.4).to(torch.uint8)
    done[0], done[B - 1] = 0, 1
    hT[done.bool()] = NAN
    cT[done.bool()] = NAN
    h0, c0 = outbuf(B, H, torch.bfloat16), outbuf(B, H)
    hT_d, cT_d, done_d = padded(hT), padded(cT), padded(done[:, None], fill=0)
    _lib.call("launch_lstm_carry", hT_d.data_ptr(), cT_d.data_ptr(), done_d.data_ptr(), h0.data_ptr(), c0.data_ptr(),
              H, B, _lib.stream())
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
    check_forward(cs, run_forward(cs), ref_forward(cs))


@gpu
@pytest.mark.parametrize("prev", [None, "zeros", "ones"])
@pytest.mark.parametrize("F,H,B", [(64, 128, 65), (128, 64, 17)])
def test_forward_prev_done_none_all_kept_all_reset(hip_lib, F, H, B, prev):
    cs = make_case(F, H, B, seed=7 + B, prev=prev)
    fw = ref_forward(cs)
    if prev == "ones":            # every row starts from a zero state: c = sig(i) tanh(j) whatever c held
        assert bool(torch.isnan(cs["c"]).all()) and bool((fw["ck"] == 0).all())
    check_forward(cs, run_forward(cs), fw)


@gpu
@pytest.mark.parametrize("F,H,B", [(64, 128, 65), (128, 64, 17)])
def test_forward_without_gates_and_xh_and_with_padded_x(hip_lib, F, H, B):
    """The bootstrap step's launch (gates = xh = None) and an x whose row stride is F + 8 (pad columns NaN) give the
    bits of the plain launch."""
    cs = make_case(F, H, B, seed=11 + B)
    fw = ref_forward(cs)
    full = run_forward(cs)
    for kw in (dict(want_gates=False, want_xh=False), dict(ldx=F + 8), dict(want_gates=False), dict(want_xh=False)):
        out = run_forward(cs, **kw)
        check_forward(cs, out, fw)
        for name in ("hout", "cout", "gates", "xh"):
            if out[name] is not None:
                assert torch.equal(bits(out[name]), bits(full[name])), (kw, name)


@gpu
@pytest.mark.parametrize("F,H,B", [(64, 128, 65), (256, 256, 17)])
def test_forward_saturated_gates_stay_finite(hip_lib, F, H, B):
    cs = make_case(F, H, B, seed=13 + B, sat=True)
    fw = ref_forward(cs)
    assert float(fw["z"].abs().min()) > 20 and float(fw["z"].abs().max()) < 45
    check_forward(cs, run_forward(cs), fw, tag="fwd_sat")


# ---------------------------------------------------------------------------------------------------------------
# backward, pointwise
# ---------------------------------------------------------------------------------------------------------------
def run_backward_point(cs, fw, mode, seed):
    """mode "scan": dh_rec / dc_rec / done_t / prev_done all present (an interior step of the reverse scan);
    "last": no recurrent gradient and no done_t; "last_done": no recurrent gradient, done_t present (what the engine
    passes at step T-1); "first": recurrent gradient, prev_done = None (step 0)."""
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
        dh_rec[done_t.bool()] = NAN          # an ended episode's row never reads its recurrent gradient
        dc_rec[done_t.bool()] = NAN
    assert (cs["prev_done"] is None) == (mode == "first")
    dz_ref, dck_ref, e32 = ref_backward_point(cs, fw, dh_heads, dh_rec, dc_rec, done_t)
    # the kernel reads the activations the forward saved: here the float64 reference's, rounded to fp32
    dz, dc_out = outbuf(B, 4 * H), outbuf(B, H)
    args = [padded(t) if t is not None else None for t in (dh_heads, dh_rec, dc_rec)]
    dn = None if done_t is None else padded(done_t[:, None], fill=0).view(-1)
    pd = None if cs["prev_done"] is None else padded(cs["prev_done"][:, None], fill=1).view(-1)
    gates, c_t, c_prev = padded(fw["gates"].float()), padded(fw["c"].float()), padded(cs["c"])
    # launch_lstm_bwd_point(dh_heads, dh_rec, dc_rec, done_t, gates, c_t, c_prev, prev_done, dz, dc_out, H, B)
    _lib.call("launch_lstm_bwd_point", ptr(args[0]), ptr(args[1]), ptr(args[2]), ptr(dn), gates.data_ptr(),
              c_t.data_ptr(), c_prev.data_ptr(), ptr(pd), dz.data_ptr(), dc_out.data_ptr(), H, B, _lib.stream())
    torch.cuda.synchronize()
    assert_sentinel(dz, B, "dz")
    assert_sentinel(dc_out, B, "dc_out")
    return dz, dc_out, dz_ref, dck_ref, e32


@gpu
@pytest.mark.parametrize("mode", ["scan", "last", "last_done", "first"])
@pytest.mark.parametrize("F,H,B", [(64, 64, 15), (64, 128, 65), (128, 64, 130), (256, 256, 17)])
def test_backward_pointwise_matches_float64_autograd(hip_lib, F, H, B, mode):
    cs = make_case(F, H, B, seed=17 + B, prev=None if mode == "first" else "rand")
    dz, dc_out, dz_ref, dck_ref, e32 = run_backward_point(cs, ref_forward(cs), mode, seed=B)
    within("bwd.dz", dz[:B], dz_ref, torch.full_like(dz_ref, 8 * e32["dz"]), e32["dz"])
    within("bwd.dc_out", dc_out[:B], dck_ref, torch.full_like(dck_ref, 8 * e32["dc_out"]), e32["dc_out"])


# ---------------------------------------------------------------------------------------------------------------
# backward GEMM
# ---------------------------------------------------------------------------------------------------------------
def run_backward_gemm(cs, dz, abs_term=0.0):
    from pathnet_gym_amd.ops import _lib
    F, H, B = cs["F"], cs["H"], cs["B"]
    _, _, Kb = refresh(cs)
    lddx = F + 8
    dx, dh_prev = outbuf(B, lddx), outbuf(B, H)
    dz_d = padded(dz)
    _lib.call("launch_lstm_bwd_gemm", dz_d.data_ptr(), Kb.data_ptr(), dx.data_ptr(), lddx, dh_prev.data_ptr(),
              F, H, B, _lib.stream())
    torch.cuda.synchronize()
    assert_sentinel(dx, B, "dx")
    assert_sentinel(dh_prev, B, "dh_prev")
    assert bool((dx[:, F:] == SENT).all()), "dx pad columns were written"
    A, Kq = bf(dz).double(), bf(cs["K"]).double()
    ref, bound = A @ Kq.t(), gemm_bound(A, Kq.t(), 4 * H) + abs_term
    within("dx", dx[:B, :F], ref[:, :F], bound[:, :F])
    within("dh_prev", dh_prev[:B], ref[:, F:], bound[:, F:])


@gpu
@pytest.mark.parametrize("F,H,B", FWD_SHAPES)
def test_backward_gemm_matches_float64(hip_lib, F, H, B):
    cs = make_case(F, H, B, seed=19 + B)
    g = torch.Generator().manual_seed(23 + B)
    run_backward_gemm(cs, torch.randn(B, 4 * H, generator=g) * 0.1)


@gpu
def test_backward_gemm_of_saturated_gate_gradients(hip_lib):
    """dz of saturated gates spans many orders of magnitude and is mostly zero.  Should any entry be subnormal, the
    MFMA (and the bf16 conversion) may flush it where float64 keeps it: 4H times the smallest normal fp32 is then
    added to the bound as an absolute term."""
    F, H, B = 64, 128, 65
    cs = make_case(F, H, B, seed=29, sat=True)
    fw = ref_forward(cs)
    g = torch.Generator().manual_seed(31)
    dz, _, _ = ref_backward_point(cs, fw, torch.randn(B, H, generator=g), None, None, None)
    dz = dz.float()
    assert bool(torch.isfinite(dz).all()) and float(dz.abs().max()) > 0
    subnormal = bool(((dz != 0) & (dz.abs() < TINY)).any())
    run_backward_gemm(cs, dz, abs_term=4 * H * TINY if subnormal else 0.0)


# ---------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------
def wgrad_cases():
    out = []
    for rpc in (32, 64, 2048):
        F, H = (128, 64) if rpc == 64 else (64, 128)
        for R in (1, 31, 32, 33, 95, rpc, rpc + 1):
            out.append((F, H, R, rpc))
    return out + [(256, 256, 95, 32), (256, 256, 130, 2048)]


@gpu
@pytest.mark.parametrize("F,H,R,rpc", wgrad_cases())
def test_wgrad_increment_matches_float64(hip_lib, F, H, R, rpc):
    """grad starts non-zero and the kernel accumulates into it: the increment is compared.  On top of the GEMM bound
    (n = R) each of the ceil(R / rows_per_chunk) atomic adds into an entry rounds the running value once, an fp32
    round-to-nearest of at most |g0| + |xh|^T |dz|: that term is added.  Everything outside the kernel and bias
    ranges keeps its bits."""
    from pathnet_gym_amd.ops import _lib
    KK, G4 = F + H, 4 * H
    cs = make_case(F, H, 1, seed=37 + R + rpc)
    g = torch.Generator().manual_seed(41 + R)
    xh, dz = bf(torch.randn(R, KK, generator=g) * 0.5), torch.randn(R, G4, generator=g) * 0.1
    g0 = torch.randn(cs["flat"].numel(), generator=g) * 0.05
    grad, xh_d, dz_d = g0.to(DEV), padded(xh), padded(dz)
    _lib.call("launch_lstm_wgrad", xh_d.data_ptr(), dz_d.data_ptr(), grad.data_ptr(), cs["k_off"], cs["b_off"],
              F, H, R, rpc, _lib.stream())
    torch.cuda.synchronize()
    grad = grad.cpu()
    ks, bs = slice(cs["k_off"], cs["k_off"] + KK * G4), slice(cs["b_off"], cs["b_off"] + G4)
    outside = torch.ones(g0.numel(), dtype=torch.bool)
    outside[ks] = False
    outside[bs] = False
    assert torch.equal(bits(grad)[outside], bits(g0)[outside])
    dK, bK, db, bb = ref_wgrad(xh, dz)
    adds = -(-R // rpc) * 2.0 ** -24 * 1.001
    bK = bK + adds * (g0[ks].view(KK, G4).abs().double() + xh.double().abs().t() @ bf(dz).double().abs())
    bb = bb + adds * (g0[bs].abs().double() + dz.double().abs().sum(0))
    within("dK", grad[ks].view(KK, G4).double() - g0[ks].view(KK, G4).double(), dK, bK)
    within("db", grad[bs].double() - g0[bs].double(), db, bb)


# ---------------------------------------------------------------------------------------------------------------
# launcher contract: a bad shape returns its code and launches nothing
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_launchers_reject_bad_arguments(hip_lib):
    from pathnet_gym_amd.ops import _lib
    lib = hip_lib
    s = _lib.stream()
    # real, zero-filled buffers larger than any shape below, entered in the middle (negative offsets stay inside)
    buf = torch.zeros(1 << 20, device=DEV)
    p = buf.data_ptr() + (1 << 21)
    fwd = lambda ldx, F, H, B, b_off=0: lib.launch_lstm_fwd(p, ldx, p, p, None, p, p, b_off, p, p, None, None,   # noqa
                                                           F, H, B, s)
    assert fwd(64, 64, 96, 16) == -1 and fwd(96, 96, 64, 16) == -1 and fwd(68, 64, 64, 16) == -1
    assert fwd(0, 64, 64, 16) == -22 and fwd(64, 0, 64, 16) == -22 and fwd(64, 64, -64, 16) == -22
    assert fwd(64, 64, 64, 0) == -22 and fwd(64, 64, 64, 16, b_off=-1) == -22
    gemm = lambda lddx, F, H, B: lib.launch_lstm_bwd_gemm(p, p, p, lddx, p, F, H, B, s)                          # noqa
    assert gemm(64, 64, 32, 16) == -1 and gemm(160, 160, 64, 16) == -1
    assert gemm(0, 64, 64, 16) == -22 and gemm(64, 64, 64, -1) == -22 and gemm(64, -64, 64, 16) == -22
    wg = lambda F, H, R, rpc, k_off=0, b_off=0: lib.launch_lstm_wgrad(p, p, p, k_off, b_off, F, H, R, rpc, s)    # noqa
    assert wg(64, 64, 32, 48) == -1 and wg(64, 65, 32, 32) == -1 and wg(32, 64, 32, 32) == -1
    assert wg(64, 64, 0, 32) == -22 and wg(64, 64, 32, 0) == -22 and wg(64, 64, 32, 32, k_off=-1) == -22
    assert wg(64, 64, 32, 32, b_off=-5) == -22 and wg(0, 64, 32, 32) == -22
    assert lib.launch_lstm_bwd_point(p, None, None, None, p, p, p, None, p, p, 0, 16, s) == -22
    assert lib.launch_lstm_bwd_point(p, None, None, None, p, p, p, None, p, p, 64, -3, s) == -22
    assert lib.launch_lstm_refresh(p, 0, 64, 72, p, p, s) == -1 and lib.launch_lstm_refresh(p, 0, 96, 64, p, p, s) == -1
    assert lib.launch_lstm_refresh(p, -1, 64, 64, p, p, s) == -22 and lib.launch_lstm_refresh(p, 0, 0, 64, p, p, s) == -22
    assert lib.launch_lstm_carry(p, p, p, p, p, 0, 16, s) == -22 and lib.launch_lstm_carry(p, p, p, p, p, 64, 0, s) == -22
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0            # nothing ran
