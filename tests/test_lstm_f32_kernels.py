"""csrc/lstm_f32.hip, launcher by launcher, against plain float64 torch with buffers of the test's own.

The method and scaffolding of tests/test_lstm_kernels.py (synthetic ``flat`` with odd ``k_off`` / ``b_off``, 64
sentinel rows after every output, 64 NaN rows after every input, NaN in h / c where ``prev_done`` is set), with one
difference: the operands are plain fp32 and enter the float64 reference as they are, with no rounding step.  The
fp32 MFMA is a k-ordered fmaf chain with one rounding per product, so all that separates a GEMM output from float64
is that chain, and its tolerance is derived, not measured:

    |hip - ref64| <= n * 2^-23 * (|A| @ |B|)          n = reduction length

(2^-24 per term would be the first-order bound of the chain; 2^-23 leaves a factor 2).  The pre-activation
z = acc + b gets one more term 2^-23 |z| for the bias add.  The weight gradient sums its rows in chunks of
``lstm_wgrad_f32_chunk_rows()`` and then the chunk partials in chunk order: at most (chunk + number of chunks - 1)
roundings of at most 2^-24 sum|terms| each, which n = R covers; the one add into a non-zero ``grad`` rounds the
result once more, 2^-24 (|grad0| + sum|terms|).

Pointwise outputs (gates, cout, hout) go through ``__expf``, which is not torch's ``exp``: their tolerance is
``L * z_bound + 8 * e32``, e32 = the max abs error of a torch fp32 evaluation of the same formulas against float64
on the same inputs, L the Lipschitz constant that carries the pre-activation bound through the gate (1/4 sigmoid,
1 tanh).  The worst measured ratio of every tensor to its bound is kept in tests/data/lstm_f32_measured.json
(written when ``PATHNET_RECORD_LSTM_F32=<file>`` is set): a record, not a budget.
"""
import json
import os

import pytest
import torch

from test_lstm_kernels import (BATCHES, EPS, FWD_SHAPES, NAN, SENT, TINY, assert_sentinel, bits, bwd_pointwise,
                               cell_from_z, gemm_bound, outbuf, padded, ptr, select_rows)

gpu = pytest.mark.gpu
DEV = "cuda"
WGRAD_ROWS = ["1", "31", "33", "chunk", "chunk+1", "2chunk+7"]
assert len(FWD_SHAPES) == 3 * len(BATCHES) + 2


# ---------------------------------------------------------------------------------------------------------------
# float64 reference (CPU tensors; also run by tests/test_lstm_f32_host.py)
# ---------------------------------------------------------------------------------------------------------------
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
    x = torch.randn(B, F, generator=g) * 0.5
    h = torch.randn(B, H, generator=g) * 0.5
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


def ref_forward(cs, K=None):
    """float64 forward of a case + the tolerances of every forward output (module docstring).  K: another kernel
    matrix in place of the case's (the negative control)."""
    F, H = cs["F"], cs["H"]
    keep = None if cs["prev_done"] is None else cs["prev_done"] == 0
    hk, ck = select_rows(keep, cs["h"]), select_rows(keep, cs["c"])
    xh = torch.cat([cs["x"], hk], 1)
    A, K64 = xh.double(), (cs["K"] if K is None else K).double()
    acc = A @ K64
    z = acc + cs["b"].double()
    dz = gemm_bound(A, K64, F + H) + EPS * z.abs()
    gates, c, h = cell_from_z(z, ck.double())
    g32, c32, h32 = cell_from_z(acc.float() + cs["b"], ck)             # torch fp32 on the same inputs
    e32 = {"gates": float((g32 - gates).abs().max()), "cout": float((c32 - c).abs().max()),
           "hout": float((h32 - h).abs().max())}
    di, dj, df, do = dz.chunk(4, 1)
    dg = torch.cat([di / 4, dj, df / 4, do / 4], 1)                    # |sig'| <= 1/4, |tanh'| <= 1
    dc = ck.double().abs() * df / 4 + di / 4 + dj                      # c = c0 sig(f) + sig(i) tanh(j), |.| <= 1
    dh = dc + do / 4                                                   # h = tanh(c) sig(o)
    tol = {"gates": dg + 8 * e32["gates"], "cout": dc + 8 * e32["cout"], "hout": dh + 8 * e32["hout"]}
    return dict(xh=xh, acc=acc, z=z, ck=ck, gates=gates, c=c, h=h, e32=e32, tol=tol)


def ref_backward_gemm(cs, dz):
    """float64 [dx | dh_prev] = dz K^T and its bound (n = 4H)."""
    A, Kt = dz.double(), cs["K"].double().t()
    return A @ Kt, gemm_bound(A, Kt, 4 * cs["H"])


def ref_wgrad(xh, dz):
    """float64 weight / bias gradient of R rows and their summation bounds (n = R)."""
    R = xh.shape[0]
    A, Bm = xh.double().t(), dz.double()
    return A @ Bm, gemm_bound(A, Bm, R), Bm.sum(0), R * EPS * Bm.abs().sum(0)


# ---------------------------------------------------------------------------------------------------------------
# GPU plumbing
# ---------------------------------------------------------------------------------------------------------------
def record_ratio(name, ratio):
    """PATHNET_RECORD_LSTM_F32=<file>: keep the worst measured error / bound per tensor."""
    rec = os.environ.get("PATHNET_RECORD_LSTM_F32")
    if not rec:
        return
    d = {}
    if os.path.exists(rec):
        with open(rec) as f:
            d = json.load(f)
    t = d.setdefault("worst_err_over_bound", {})
    t[name] = max(float(ratio), float(t.get(name, 0.0)))
    os.makedirs(os.path.dirname(rec) or ".", exist_ok=True)
    with open(rec, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def excess(got, ref, tol):
    """Elementwise err / tol of a finite output."""
    return (got.double().cpu() - ref).abs() / tol.clamp_min(1e-300)


def within(name, got, ref, tol):
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    r = excess(got, ref, tol)
    worst = float(r.max())
    print(f"{name}: worst err / bound = {worst:.4f}")
    record_ratio(name, worst)
    assert worst <= 1.0, (name, worst, int((r > 1).sum()), r.numel())


def run_forward(cs, want_gates=True, want_xh=True, ldx=None):
    from pathnet_gym_amd.ops import _lib
    F, H, B = cs["F"], cs["H"], cs["B"]
    flat = cs["flat"].to(DEV)
    X = padded(cs["x"], cols=ldx)                                     # ldx > F: the pad columns hold NaN
    hp, cp = padded(cs["h"]), padded(cs["c"])
    pd = None if cs["prev_done"] is None else padded(cs["prev_done"][:, None], fill=1).view(-1)
    hout, cout = outbuf(B, H), outbuf(B, H)
    gates = outbuf(B, 4 * H) if want_gates else None
    xh = outbuf(B, F + H) if want_xh else None
    _lib.call("launch_lstm_fwd_f32", X.data_ptr(), X.shape[1], hp.data_ptr(), cp.data_ptr(), ptr(pd),
              flat.data_ptr(), cs["k_off"], cs["b_off"], hout.data_ptr(), cout.data_ptr(), ptr(gates), ptr(xh),
              F, H, B, _lib.stream())
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
        within(f"{tag}.gates", out["gates"][:B], fw["gates"], fw["tol"]["gates"])
    within(f"{tag}.cout", out["cout"][:B], fw["c"], fw["tol"]["cout"])
    within(f"{tag}.hout", out["hout"][:B], fw["h"], fw["tol"]["hout"])


def assert_scaled_column_fails(cs, out):
    """Negative control: against a reference whose kernel column H + 3 (unit 3 of the j gate) is scaled by 1.02, the
    same outputs leave the same kind of bound."""
    B, H = cs["B"], cs["H"]
    K = cs["K"].clone()
    K[:, H + 3] *= 1.02
    bad = ref_forward(cs, K=K)
    assert float(excess(out["gates"][:B], bad["gates"], bad["tol"]["gates"]).max()) > 1.0
    assert float(excess(out["cout"][:B], bad["c"], bad["tol"]["cout"]).max()) > 1.0
    assert float(excess(out["hout"][:B], bad["h"], bad["tol"]["hout"]).max()) > 1.0


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
    """The bootstrap step's launch (gates = xh = None) and an x whose row stride is F + 4 (pad columns NaN) give the
    bits of the plain launch."""
    cs = make_case(F, H, B, seed=11 + B)
    fw = ref_forward(cs)
    full = run_forward(cs)
    for kw in (dict(want_gates=False, want_xh=False), dict(ldx=F + 4), dict(want_gates=False), dict(want_xh=False)):
        out = run_forward(cs, **kw)
        check_forward(cs, out, fw)
        for name in ("hout", "cout", "gates", "xh"):
            if out[name] is not None:
                assert torch.equal(bits(out[name]), bits(full[name])), (kw, name)


@gpu
@pytest.mark.parametrize("F,H,B", [(64, 128, 65)])
def test_forward_saturated_gates_stay_finite(hip_lib, F, H, B):
    cs = make_case(F, H, B, seed=13 + B, sat=True)
    fw = ref_forward(cs)
    assert float(fw["z"].abs().min()) > 20 and float(fw["z"].abs().max()) < 45
    check_forward(cs, run_forward(cs), fw, tag="fwd_sat")


# ---------------------------------------------------------------------------------------------------------------
# backward GEMM
# ---------------------------------------------------------------------------------------------------------------
def run_backward_gemm(cs, dz, abs_term=0.0):
    from pathnet_gym_amd.ops import _lib
    F, H, B = cs["F"], cs["H"], cs["B"]
    flat = cs["flat"].to(DEV)
    lddx = F + 8
    dx, dh_prev = outbuf(B, lddx), outbuf(B, H)
    dz_d = padded(dz)
    _lib.call("launch_lstm_bwd_gemm_f32", dz_d.data_ptr(), flat.data_ptr(), cs["k_off"], dx.data_ptr(), lddx,
              dh_prev.data_ptr(), F, H, B, _lib.stream())
    torch.cuda.synchronize()
    assert_sentinel(dx, B, "dx")
    assert_sentinel(dh_prev, B, "dh_prev")
    assert bool((dx[:, F:] == SENT).all()), "dx pad columns were written"
    ref, bound = ref_backward_gemm(cs, dz)
    within("dx", dx[:B, :F], ref[:, :F], bound[:, :F] + abs_term)
    within("dh_prev", dh_prev[:B], ref[:, F:], bound[:, F:] + abs_term)
    return dx, dh_prev


@gpu
@pytest.mark.parametrize("F,H,B", FWD_SHAPES)
def test_backward_gemm_matches_float64(hip_lib, F, H, B):
    cs = make_case(F, H, B, seed=19 + B)
    g = torch.Generator().manual_seed(23 + B)
    dz = torch.randn(B, 4 * H, generator=g) * 0.1
    dx, dh_prev = run_backward_gemm(cs, dz)
    # negative control: kernel row 5 (a dx column) and row F + 5 (a dh_prev column) of the reference scaled by 1.02
    K = cs["K"].clone()
    K[5] *= 1.02
    K[F + 5] *= 1.02
    ref, bound = ref_backward_gemm(dict(cs, K=K), dz)
    assert float(excess(dx[:B, :F], ref[:, :F], bound[:, :F]).max()) > 1.0
    assert float(excess(dh_prev[:B], ref[:, F:], bound[:, F:]).max()) > 1.0


@gpu
def test_backward_gemm_of_saturated_gate_gradients(hip_lib):
    """dz of saturated gates spans many orders of magnitude and is mostly zero.  Should any entry be subnormal, the
    MFMA may flush it where float64 keeps it: 4H times the smallest normal fp32 is then added to the bound as an
    absolute term."""
    F, H, B = 64, 128, 65
    cs = make_case(F, H, B, seed=29, sat=True)
    fw = ref_forward(cs)
    g = torch.Generator().manual_seed(31)
    dh = torch.randn(B, H, generator=g).double()
    dz, _ = bwd_pointwise(dh, None, None, None, fw["gates"], fw["c"], fw["ck"].double())
    dz = dz.float()
    assert bool(torch.isfinite(dz).all()) and float(dz.abs().max()) > 0
    subnormal = bool(((dz != 0) & (dz.abs() < TINY)).any())
    run_backward_gemm(cs, dz, abs_term=4 * H * TINY if subnormal else 0.0)


# ---------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------
def wgrad_rows(lib, label):
    ch = lib.lstm_wgrad_f32_chunk_rows()
    return {"chunk": ch, "chunk+1": ch + 1, "2chunk+7": 2 * ch + 7}.get(label) or int(label)


def run_wgrad(cs, xh_d, dz_d, g0, R):
    from pathnet_gym_amd.ops import _lib
    F, H = cs["F"], cs["H"]
    n = _lib.lib().lstm_wgrad_f32_part_numel(F, H, R)
    part = torch.full((n + 4096,), SENT, device=DEV)
    grad = g0.to(DEV)
    _lib.call("launch_lstm_wgrad_f32", xh_d.data_ptr(), dz_d.data_ptr(), grad.data_ptr(), part.data_ptr(),
              cs["k_off"], cs["b_off"], F, H, R, _lib.stream())
    torch.cuda.synchronize()
    assert bool((part[n:] == SENT).all()), "the scratch buffer was written past its slabs"
    return grad.cpu()


@gpu
@pytest.mark.parametrize("start", ["zero", "random"])
@pytest.mark.parametrize("F,H,rows", [(64, 128, r) for r in WGRAD_ROWS] + [(128, 64, "33"), (256, 256, "33")])
def test_wgrad_matches_float64_and_repeats_bit_for_bit(hip_lib, F, H, rows, start):
    """grad starts at zero, or at a random grad0 into which the kernel adds once.  Everything outside the kernel and
    bias ranges keeps its bits, and a second call on the same inputs gives the same bits."""
    R = wgrad_rows(hip_lib, rows)
    KK, G4 = F + H, 4 * H
    ch = hip_lib.lstm_wgrad_f32_chunk_rows()
    assert hip_lib.lstm_wgrad_f32_part_numel(F, H, R) == -(-R // ch) * (KK * G4 + G4)
    cs = make_case(F, H, 1, seed=37 + R)
    g = torch.Generator().manual_seed(41 + R)
    xh, dz = torch.randn(R, KK, generator=g) * 0.5, torch.randn(R, G4, generator=g) * 0.1
    g0 = torch.randn(cs["flat"].numel(), generator=g) * 0.05
    if start == "zero":
        g0.zero_()
    xh_d, dz_d = padded(xh), padded(dz)
    grad = run_wgrad(cs, xh_d, dz_d, g0, R)
    assert torch.equal(bits(run_wgrad(cs, xh_d, dz_d, g0, R)), bits(grad))
    ks, bs = slice(cs["k_off"], cs["k_off"] + KK * G4), slice(cs["b_off"], cs["b_off"] + G4)
    outside = torch.ones(g0.numel(), dtype=torch.bool)
    outside[ks] = False
    outside[bs] = False
    assert torch.equal(bits(grad)[outside], bits(g0)[outside])
    dK, bK, db, bb = ref_wgrad(xh, dz)
    if start == "random":          # the one add into grad0
        add = 2.0 ** -24 * 1.001
        bK = bK + add * (g0[ks].view(KK, G4).abs().double() + xh.double().abs().t() @ dz.double().abs())
        bb = bb + add * (g0[bs].abs().double() + dz.double().abs().sum(0))
    within("dK", grad[ks].view(KK, G4).double() - g0[ks].view(KK, G4).double(), dK, bK)
    within("db", grad[bs].double() - g0[bs].double(), db, bb)
    # negative control: one row fewer leaves the bound almost everywhere (the bound grows with R^2 and a single row
    # does not: at the chunk-sized R it is wider than one row's share)
    if 1 < R <= 64:
        dKs, _, dbs, _ = ref_wgrad(xh[:-1], dz[:-1])
        assert float((excess(grad[ks].view(KK, G4).double() - g0[ks].view(KK, G4).double(), dKs, bK) > 1)
                     .double().mean()) > 0.5


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
    fwd = lambda ldx, F, H, B, k_off=0, b_off=0: lib.launch_lstm_fwd_f32(p, ldx, p, p, None, p, k_off, b_off, p,   # noqa
                                                                       p, None, None, F, H, B, s)
    assert fwd(64, 64, 96, 16) == -1 and fwd(96, 96, 64, 16) == -1 and fwd(66, 64, 64, 16) == -1
    assert fwd(64, 128, 64, 16) == -1                                  # a row stride below F
    assert fwd(0, 64, 64, 16) == -22 and fwd(64, 0, 64, 16) == -22 and fwd(64, 64, -64, 16) == -22
    assert fwd(64, 64, 64, 0) == -22 and fwd(64, 64, 64, 16, b_off=-1) == -22
    assert fwd(64, 64, 64, 16, k_off=-1) == -22
    gemm = lambda lddx, F, H, B, k_off=0: lib.launch_lstm_bwd_gemm_f32(p, p, k_off, p, lddx, p, F, H, B, s)       # noqa
    assert gemm(64, 64, 32, 16) == -1 and gemm(160, 160, 64, 16) == -1 and gemm(64, 128, 64, 16) == -1
    assert gemm(0, 64, 64, 16) == -22 and gemm(64, 64, 64, -1) == -22 and gemm(64, -64, 64, 16) == -22
    assert gemm(64, 64, 64, 16, k_off=-3) == -22
    wg = lambda F, H, R, k_off=0, b_off=0, part=p: lib.launch_lstm_wgrad_f32(p, p, p, part, k_off, b_off, F, H,  # noqa
                                                                             R, s)
    assert wg(64, 65, 32) == -1 and wg(32, 64, 32) == -1
    assert wg(64, 64, 0) == -22 and wg(64, 64, 32, k_off=-1) == -22 and wg(64, 64, 32, b_off=-5) == -22
    assert wg(0, 64, 32) == -22 and wg(64, 64, 32, part=None) == -22
    assert lib.lstm_wgrad_f32_part_numel(0, 64, 32) == 0 and lib.lstm_wgrad_f32_part_numel(64, 64, -1) == 0
    assert lib.lstm_wgrad_f32_chunk_rows() % 32 == 0
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0            # nothing ran
