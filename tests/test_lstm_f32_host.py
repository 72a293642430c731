"""csrc/lstm_f32.hip on any machine: the ctypes table holds its launchers, and the float64 reference functions of
tests/test_lstm_f32_kernels.py agree with ``models/pathnet.py:lstm_cell_ref`` in float64."""
import ast
import os

import torch

from pathnet_gym_amd.models.pathnet import lstm_cell_ref
from pathnet_gym_amd.ops import _lib
from test_lstm_kernels import EPS, bwd_pointwise, gemm_bound, select_rows
from test_lstm_f32_kernels import make_case, ref_backward_gemm, ref_forward, ref_wgrad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ctypes_table_holds_the_fp32_lstm_launchers():
    from ctypes import c_int, c_long, c_void_p
    P = c_void_p
    want = {
        "launch_lstm_fwd_f32": [P, c_int, P, P, P, P, c_long, c_long, P, P, P, P, c_int, c_int, c_int, P],
        "launch_lstm_bwd_gemm_f32": [P, P, c_long, P, c_int, P, c_int, c_int, c_int, P],
        "launch_lstm_wgrad_f32": [P, P, P, P, c_long, c_long, c_int, c_int, c_long, P],
        "lstm_wgrad_f32_part_numel": [c_int, c_int, c_long],
        "lstm_wgrad_f32_chunk_rows": [],
    }
    for name, sig in want.items():
        assert _lib._SIGS.get(name) == sig, name
    # the shared fp32 kernels the fused fp32 cell reuses
    assert "launch_lstm_bwd_point" in _lib._SIGS and "launch_lstm_carry_f32" in _lib._SIGS


def test_every_fp32_lstm_launcher_has_a_call_site():
    """ops/pathnet_ops.py dispatches to each launcher (a name in the table that nothing calls is dead)."""
    src = open(os.path.join(ROOT, "pathnet_gym_amd", "ops", "pathnet_ops.py")).read()
    called = {n.args[0].value for n in ast.walk(ast.parse(src))
              if isinstance(n, ast.Call) and getattr(n.func, "attr", None) == "call" and n.args
              and isinstance(n.args[0], ast.Constant)}
    assert {"launch_lstm_fwd_f32", "launch_lstm_bwd_gemm_f32", "launch_lstm_wgrad_f32"} <= called
    assert "lstm_wgrad_f32_part_numel" in src


def test_reference_helpers_agree_with_lstm_cell_ref_in_float64():
    for (F, H, B), prev in (((64, 128, 70), "rand"), ((128, 64, 17), None), ((256, 256, 96), "rand")):
        cs = make_case(F, H, B, seed=F + B, prev=prev)
        assert cs["k_off"] % 2 == 1 and cs["b_off"] % 2 == 1
        fw = ref_forward(cs)
        keep = None if cs["prev_done"] is None else cs["prev_done"] == 0
        K = cs["K"].double().requires_grad_(True)
        bb = cs["b"].double().requires_grad_(True)
        x = cs["x"].double().requires_grad_(True)
        hk = select_rows(keep, cs["h"]).double().requires_grad_(True)
        ck = fw["ck"].double().requires_grad_(True)
        h2, c2 = lstm_cell_ref(x, hk, ck, K, bb)
        assert torch.allclose(h2, fw["h"], rtol=0, atol=1e-13) and torch.allclose(c2, fw["c"], rtol=0, atol=1e-13)
        assert torch.isfinite(fw["h"]).all() and torch.isfinite(fw["c"]).all()       # the planted NaN never got in
        if keep is not None:
            assert bool(torch.isnan(cs["h"][~keep]).all()) and bool((fw["xh"][~keep][:, F:] == 0).all())
        # the backward GEMM and weight-gradient references == autograd of lstm_cell_ref
        g = torch.Generator().manual_seed(5)
        gh, gc = torch.randn(B, H, generator=g).double(), torch.randn(B, H, generator=g).double()
        ((h2 * gh).sum() + (c2 * gc).sum()).backward()
        dz, dck = bwd_pointwise(gh, None, gc, None, fw["gates"], fw["c"], fw["ck"].double())
        assert torch.allclose(ck.grad, dck, rtol=0, atol=1e-13)
        dxh, _ = ref_backward_gemm(dict(cs, K=cs["K"].double()), dz)
        assert torch.allclose(torch.cat([x.grad, hk.grad], 1), dxh, rtol=0, atol=1e-12)
        dK, _, db, _ = ref_wgrad(fw["xh"].double(), dz)
        assert torch.allclose(K.grad, dK, rtol=0, atol=1e-11) and torch.allclose(bb.grad, db, rtol=0, atol=1e-11)
        for k in ("gates", "cout", "hout"):
            assert 0 < fw["e32"][k] < 1e-5
        # the derived bound holds, with room, for an fp32 matmul of the same fp32 operands
        A = fw["xh"].double()
        err = (fw["xh"] @ cs["K"]).double() - A @ cs["K"].double()
        bound = gemm_bound(A, cs["K"].double(), F + H)
        assert (err.abs() <= bound).all() and float((err.abs() / bound).max()) < 0.25
    # ... and it is tight enough to see one row of R = 33 missing from a weight gradient
    g = torch.Generator().manual_seed(9)
    xh, dz = torch.randn(33, 192, generator=g) * 0.5, torch.randn(33, 512, generator=g) * 0.1
    dK, bK, db, bb_ = ref_wgrad(xh, dz)
    assert ((xh.t() @ dz).double() - dK).abs().le(bK).all() and (dz.sum(0).double() - db).abs().le(bb_).all()
    short = (xh[:-1].t() @ dz[:-1]).double()
    assert float(((short - dK).abs() > bK).double().mean()) > 0.9
    assert float(((dz[:-1].sum(0).double() - db).abs() > bb_).double().mean()) > 0.9
    assert bb_.shape == (512,) and float(bb_.min()) > 0 and EPS == 2.0 ** -23
