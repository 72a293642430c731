"""csrc/typed_fc.hip on any machine: the float64 reference of tests/test_typed_fc_kernels.py is pinned to
``models.pathnet.trunk_forward_ref``, a plain torch fp32 evaluation of every formula passes every derived bound at
every shape of the table (and each negative control fails its bound by a wide margin on that same emulation), the
shape table reaches the tile and chunk edges it claims, and ``im2col_nhwc`` has the (kh, kw, cin) order the conv
modules rely on."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from pathnet_gym_amd.config import LayerSpec, PathNetConfig
from pathnet_gym_amd.models.pathnet import ParamStore, trunk_forward_ref
from pathnet_gym_amd.ops import _lib
from test_lstm_kernels import SENT
import test_typed_fc_kernels as tk
from test_typed_fc_kernels import (CASES, CONTROL_ROW, case_id, check_forward, check_wgrad, compose, control_margins,
                                   make_case, path_terms, reach, ref_dgrad, ref_forward, ref_wgrad, unpack_grad, within)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def emulate_fp32(cs):
    """Every formula of the kernels in plain torch fp32 (any summation order; the bounds hold for all of them):
    -> out, forward relu mask, dx and the flat gradient buffer under cs["relu"]."""
    K, C, M = cs["K"], cs["C"], cs["M"]
    x, W, b, dy = cs["x"], cs["W"], cs["b"], cs["dy"]
    rowmask, wsel, nid, _ = (t.float() for t in path_terms(cs))
    pre = torch.einsum("rk,mkc->rmc", x, W) + b[None]
    out = (torch.relu(pre) * wsel[:, :, None]).sum(1)
    g = dy[:, None, :] * cs["relu"].float() * wsel[:, :, None]
    dx = torch.einsum("rmc,mkc->rk", g, W)
    if bool(nid.any()):
        out = out + nid[:, None] * x
        dx = dx + nid[:, None] * dy
    relu = ((pre > 0) & (wsel[:, :, None] > 0)).to(torch.uint8)
    gflat = torch.full((cs["flat"].numel(),), SENT)
    body = torch.cat([torch.einsum("rk,rmc->mkc", x, g).reshape(M, K * C), g.sum(0)], 1)        # [M][K*C + C]
    for m in range(M):
        s = cs["off"] + m * cs["chunk"]
        gflat[s:s + K * C + C] = body[m]
    return out, relu, dx, gflat


# ---------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------
def test_table_constants_are_those_of_the_kernels():
    src = open(os.path.join(ROOT, "csrc", "typed_fc.hip")).read()
    define = lambda n: int(re.search(rf"#define {n} (\d+)", src).group(1))                           # noqa: E731
    for name in ("TF_RT", "TF_KC", "TF_MAXM", "TF_MAXC", "TF_PPT", "TM_T", "TM_KC"):
        assert define(name) == getattr(tk, name), name
    m = re.search(r"constexpr int KT = (\d+), RC = (\d+);", src)
    assert (int(m.group(1)), int(m.group(2))) == (tk.WG_KT, tk.WG_RC)
    assert "(K + 15) / 16" in src and tk.WG_KT == 16                  # the wgrad launcher's grid is in k tiles of KT
    for name in ("fwd", "dgrad", "wgrad"):
        assert f"launch_typed_fc_{name}" in _lib._SIGS and f"launch_typed_fc_{name}_mfma" in _lib._SIGS
    assert _lib._SIGS["typed_fc_dgrad_lds_limit"] == []


def test_table_reaches_the_edges_it_claims():
    """Each row's note is the arithmetic of its sizes on the kernels' constants, and between them the rows hold the
    value sets, the pairs and the edges the table's header states."""
    assert len({case_id(r) for r in CASES}) == len(CASES) and 140 <= len(CASES) <= 180
    for eng, K, C, rpp, P, M, comp, note in CASES:
        assert note == reach(eng, K, C, rpp), case_id((eng, K, C, rpp, P, M, comp))
        assert M <= tk.TF_MAXM and (eng == "mfma" or (C <= tk.TF_MAXC and tk.TF_RT * C <= 256 * tk.TF_PPT))
        assert (comp == "layer0") == (K != C)
    want = {"valu": dict(C={1, 20, 33, 64}, K={1, 15, 16, 17, 255, 256, 257, 513},
                         rpp={1, 15, 16, 17, 33, 63, 64, 65, 130}),
            "mfma": dict(C={1, 20, 63, 64, 65, 130}, K={1, 3, 31, 32, 33, 64, 65, 100},
                         rpp={1, 31, 32, 33, 63, 64, 65, 130})}
    for eng, w in want.items():
        rows = [r for r in CASES if r[0] == eng]
        fc = [r for r in rows if r[6] in ("allfc", "layer0")]
        assert {r[2] for r in rows} == w["C"] and {r[3] for r in rows} == w["rpp"]
        assert {r[1] for r in fc} >= w["K"] and {r[1] for r in rows} == w["K"] | w["C"]
        assert {r[4] for r in rows} == {1, 5} and {r[5] for r in rows} == {1, 3, 10, 16}
        assert {r[6] for r in rows} == set(tk.COMPS)
        # the pairs
        assert {(r[1], r[2]) for r in fc} >= {(k, c) for k in w["K"] for c in w["C"]}
        assert {(r[2], r[3]) for r in rows} == {(c, r) for c in w["C"] for r in w["rpp"]}
        assert {(r[3], r[4]) for r in rows} == {(r, p) for r in w["rpp"] for p in (1, 5)}
        assert {(r[3], r[5]) for r in rows} == {(r, m) for r in w["rpp"] for m in (1, 3, 10, 16)}
        assert {(r[2], r[5]) for r in rows} == {(c, m) for c in w["C"] for m in (1, 3, 10, 16)}
        assert {(r[4], r[5]) for r in rows} == {(p, m) for p in (1, 5) for m in (1, 3, 10, 16)}
        assert {(r[2], r[6]) for r in rows if r[6] not in ("allfc", "layer0")} == \
            {(c, k) for c in w["C"] for k in tk.COMPS[2:]}
    ceil = lambda n, t: -(-n // t)                                                                   # noqa: E731
    v = [r for r in CASES if r[0] == "valu"]
    m = [r for r in CASES if r[0] == "mfma"]
    # VALU forward: one chunk short / exact / one over / three chunks with a tail of 1; the 16-row tile likewise
    assert {(ceil(r[1], 256), r[1] % 256) for r in v} >= {(1, 255), (1, 0), (2, 1), (3, 1), (1, 1)}
    assert {(ceil(r[3], 16), r[3] % 16) for r in v} >= {(1, 1), (1, 15), (1, 0), (2, 1), (3, 1)}
    # VALU wgrad: the 64-row chunk and the 16-wide k tile short, exact, over, and three chunks
    assert {(ceil(r[3], 64), r[3] % 64) for r in v} >= {(1, 63), (1, 0), (2, 1), (3, 2)}
    assert {r[1] % 16 for r in v} >= {0, 1, 4, 15} and max(ceil(r[1], 16) for r in v) == 33
    # VALU widths: 1 .. 4 (row, c) pairs per thread; C = 64 is the last width the launcher admits
    assert {ceil(16 * r[2], 256) for r in v} == {1, 2, 3, 4} and 16 * 64 == 256 * tk.TF_PPT
    # MFMA: the 64 tile in rows and columns short / exact / over / three tiles, the 32-deep chunks of the forward
    # (K), of dgrad (C) and of wgrad (rows) likewise, and K < 32
    for dim in (2, 3):
        assert {(ceil(r[dim], 64), r[dim] % 64) for r in m} >= {(1, 1), (1, 63), (1, 0), (2, 1), (3, 2)}
    assert {(ceil(r[1], 32), r[1] % 32) for r in m} >= {(1, 1), (1, 3), (1, 31), (1, 0), (2, 1), (2, 0), (3, 1), (4, 4)}
    assert {(ceil(r[2], 32), r[2] % 32) for r in m} >= {(1, 1), (1, 20), (2, 31), (2, 0), (3, 1), (5, 2)}
    assert {(ceil(r[3], 32), r[3] % 32) for r in m} >= {(1, 1), (1, 31), (1, 0), (2, 1), (2, 31), (2, 0), (3, 1), (5, 2)}
    assert {(ceil(r[1], 64), r[1] % 64) for r in m} >= {(1, 1), (1, 0), (2, 1), (2, 36), (3, 2)}   # dgrad / wgrad k tiles


def test_compositions_are_what_their_names_say():
    for P in (1, 5):
        for M in (1, 3, 10, 16):
            for comp in tk.COMPS:
                if M < 3 and comp not in ("allfc", "layer0", "allskip"):
                    continue
                types, mask = compose(comp, P, M)
                t = torch.tensor(types)
                assert set(mask.unique().tolist()) <= {0.0, 1.0} and mask.shape == (P, M)
                nact = (mask * (t != 0)).sum(1)
                nid = (mask * (t != 1)).sum(1)
                assert bool((mask.sum(1) >= 1).all())
                if comp in ("allfc", "layer0"):
                    assert types == [1] * M and int(nact[0]) == M and float(nid.sum()) == 0
                elif comp == "allskip":
                    assert int(nact[0]) == 0 and int(nid[0]) >= 1
                elif comp == "nid3":
                    assert int(nid[0]) == 3 and int(nact[0]) == 2
                elif comp == "shared":
                    assert bool((mask[:, 0] == 1).all()) and types[0] == 2
                elif comp == "unused":
                    assert float(mask[:, 1].sum()) == 0 and types[1] == 2
                elif comp == "skipactive":
                    assert types[1] == 0 and bool((mask[:, 1] == 1).all()) and bool((nact >= 1).all())
    # over the table: an identity coefficient of 2 and of 3 both occur, and so does a module that several paths share
    nids = set()
    for row in CASES:
        types, mask = compose(row[6], row[4], row[5])
        nids |= set((mask * (torch.tensor(types) != 1)).sum(1).int().tolist())
    assert {0, 1, 2, 3} <= nids


# ---------------------------------------------------------------------------------------------------------------
# the reference is the project's oracle
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mtype,K,C", [(0, 20, 20), (1, 20, 20), (1, 37, 20), (2, 20, 20)])
def test_reference_equals_trunk_forward_ref_in_float64(mtype, K, C):
    """One layer whose modules all have the type: forward, input gradient and parameter gradient of the float64
    reference == trunk_forward_ref and its autograd (the backward references get the forward's own ReLU mask)."""
    P, M, rpp = 3, 4, 5
    cs = make_case("valu", K, C, rpp, P, M, "allfc" if K == C else "layer0", seed=11 + mtype)
    cs["types"] = [mtype] * M
    cs["mask"] = torch.tensor([[1., 1., 0., 0.], [0., 1., 1., 0.], [1., 0., 1., 0.]])
    cfg = PathNetConfig(L=1, M=M, N=2, input_shape=(K,), layers=[LayerSpec("fc", C, module_types=[mtype])],
                        trunk_scale="none", num_actions=10)
    st = ParamStore(cfg, "cpu", seed=1)
    li = st.layout.layer_info[0]
    assert li["offset"] == 0 and li["chunk"] == K * C + C
    flat = st.flat.double()
    flat[:M * li["chunk"]] = torch.cat([cs["W"].reshape(M, -1), cs["b"]], 1).reshape(-1).double()
    st.flat = flat.requires_grad_(True)
    x = cs["x"].double().requires_grad_(True)
    y = trunk_forward_ref(st, x, cs["mask"].double().repeat_interleave(rpp, 0)[:, None, :])
    fw = ref_forward(cs)
    assert torch.allclose(y, fw["out"], rtol=0, atol=1e-13)
    (y * cs["dy"].double()).sum().backward()
    assert int(fw["undet"].sum()) == 0
    cs["relu"] = (fw["pre"] > 0).to(torch.uint8)        # every plane: the references must mask the inactive ones
    dx, _ = ref_dgrad(cs)
    assert torch.allclose(x.grad, dx, rtol=0, atol=1e-13)
    dW, _, db, _ = ref_wgrad(cs)
    grad = torch.zeros_like(flat) if st.flat.grad is None else st.flat.grad        # all-skip: the weights are unused
    g = grad[:M * li["chunk"]].view(M, -1)
    assert torch.allclose(g[:, :K * C].reshape(M, K, C), dW, rtol=0, atol=1e-12)
    assert torch.allclose(g[:, K * C:], db, rtol=0, atol=1e-12)
    if mtype == 0:
        assert float(dW.abs().max()) == 0 and float(db.abs().max()) == 0 and bool((fw["relu"] == 0).all())


# ---------------------------------------------------------------------------------------------------------------
# the bounds, on a CPU emulation
# ---------------------------------------------------------------------------------------------------------------
def test_fp32_emulation_passes_every_bound_at_every_shape():
    """... and the undetermined share of every forward case is far under 1 %."""
    worst_share, worst = 0.0, {}
    for row in CASES:
        cs = make_case(*row)
        out, relu, dx, gflat = emulate_fp32(cs)
        tag = case_id(row)
        share = check_forward(tag, cs, ref_forward(cs), out, relu, record=False)
        worst_share = max(worst_share, share)
        rd = ref_dgrad(cs)
        worst["dx"] = max(worst.get("dx", 0.0), within(f"{tag}.dx", dx, rd[0], rd[1], record=False))
        check_wgrad(tag, cs, ref_wgrad(cs), gflat, SENT, record=False)
    print("largest undetermined share of a case:", worst_share)
    assert worst_share < 0.002


@pytest.mark.parametrize("eng", ["valu", "mfma"])
def test_negative_controls_fail_by_a_wide_margin_on_the_emulation(eng):
    cs = make_case(eng, *CONTROL_ROW)
    out, relu, dx, gflat = emulate_fp32(cs)
    check_forward("control", cs, ref_forward(cs), out, relu, record=False)
    dW, db = unpack_grad(cs, gflat)
    margins = control_margins(cs, out, dx, dW, db)
    assert len(margins) == 8
    for name, worst in margins.items():
        assert worst > 100.0, (name, worst)


# ---------------------------------------------------------------------------------------------------------------
# dgrad routing by the LDS limit
# ---------------------------------------------------------------------------------------------------------------
def test_dgrad_goes_to_mfma_where_the_lds_request_does_not_fit(monkeypatch):
    from pathnet_gym_amd.ops import typed_fc

    class Lib:
        limit = 0

        def typed_fc_dgrad_lds_limit(self):
            return self.limit

    lib = Lib()
    monkeypatch.setattr(typed_fc._lib, "lib", lambda: lib)
    lib.limit = 163840 - 72                               # what the MI355X reports: every admitted shape fits
    assert not typed_fc._dgrad_use_mfma(64, 16, False) and typed_fc._dgrad_use_mfma(64, 16, True)
    lib.limit = 65536 - 72                                # a 64 KiB device: M = 16, C = 64 asks for 65 536 B
    assert typed_fc._dgrad_use_mfma(64, 16, False) and not typed_fc._dgrad_use_mfma(64, 15, False)
    assert not typed_fc._dgrad_use_mfma(63, 16, False) and not typed_fc._dgrad_use_mfma(20, 10, False)
    lib.limit = -1                                        # no limit could be read: the launcher would refuse
    assert typed_fc._dgrad_use_mfma(1, 1, False)


# ---------------------------------------------------------------------------------------------------------------
# im2col
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,stride", [(5, 2), (3, 2), (3, 1)])
def test_im2col_nhwc_times_the_tf_kernel_matrix_is_conv2d(k, stride):
    """A non-square input, so that a (kw, kh) or (cin, kh, kw) order cannot pass."""
    from pathnet_gym_amd.ops.typed_fc import im2col_nhwc
    g = torch.Generator().manual_seed(3 + k + stride)
    B, H, Wd, cin, cout = 2, 11, 14, 3, 4
    h = torch.randn(B, H, Wd, cin, generator=g, dtype=torch.float64)
    Wt = torch.randn(k, k, cin, cout, generator=g, dtype=torch.float64)               # TF layout [kh, kw, cin, cout]
    cols, Ho, Wo = im2col_nhwc(h, k, stride)
    assert (Ho, Wo) == ((H - k) // stride + 1, (Wd - k) // stride + 1) and Ho != Wo
    assert cols.shape == (B * Ho * Wo, k * k * cin)
    y = (cols @ Wt.reshape(k * k * cin, cout)).reshape(B, Ho, Wo, cout)
    ref = F.conv2d(h.permute(0, 3, 1, 2), Wt.permute(3, 2, 0, 1), stride=stride).permute(0, 2, 3, 1)
    assert torch.allclose(y, ref, rtol=0, atol=1e-12)
