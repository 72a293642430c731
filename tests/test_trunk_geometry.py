"""The runtime-geometry trunk kernels (csrc/trunk_fwd.hip, trunk_bwd.hip, trunk_f32.hip) off the reference geometry,
layer by layer against plain float64.

Every other GPU test runs these kernels at the reference's 160x120x4 k8 s4 / 39x29x8 k4 s2 / 18x13x8 k3 s1 trunk.
``HipPathNet.layer_fwd`` / ``layer_bwd`` fall through to them for every other trunk, so here they get odd Ho / Wo,
stride 3, K == KP, zero-padded K, row counts that end inside a workgroup, E not a multiple of 16, M = 16, and every
row-count / width branch of the fc launchers.

Method (that of tests/test_lstm_kernels.py).  The reference of layer l is fed what the kernel read: the previous
layer's HIP output, read back (the uint8 pixels for layer 0), and the operand copy ``hp.Wc[l]`` / ``hp.WcT[l]`` the
kernel multiplies, widened to float64 -- errors do not compound and every tolerance is derived, not measured:

forward   pre = in_scale * (x @ W) + b per active slot;  slot bound = K 2^-23 in_scale (|x| @ |W|) + 2^-23 |pre|
          (fp32 accumulation of exact, or once-rounded, products; 2^-23 and not 2^-24 so that it holds whatever
          rounding the MFMA uses inside).  y = out_scale * sum_slots relu(pre); ReLU is 1-Lipschitz, so its bound is
          out_scale * sum of the slot bounds, plus 2^-8 |y| for a bf16 store (one rounding flip), nothing for fp32.
bits      the ReLU bit planes must equal pre64 > 0 wherever |pre64| exceeds the slot bound; at most 1 % of a layer's
          elements may lie inside it (the reference alone leaves out 0.3 % at K = 1408).
backward  ``layer_bwd`` on a random fp32 G with the X and ReLU bits the forward kernels produced.  The reference
          rounds its operands as the kernel does:
          * conv_wgrad_kernel (bf16): masked G * g_scale -> bf16 (trunk_bwd.hip `v[c] = (short)f2bf(x)`), bias
            gradient from the unrounded x (`atomicAdd(&dbias[a * 8 + c], x)`);
          * conv_dgrad_kernel: fp32 VALU on the fp32 master weights (`Wl[i] = flat[...]`), G * g_scale unrounded;
          * fc_wgrad_kernel: masked G * g_scale -> bf16 (`gv8[c] = (short)f2bf(x)`), bias from the unrounded x
            (`bpart[c] += x`);
          * fc_dgrad_kernel / fc_dgrad_lds_kernel: masked G * g_scale -> bf16 (`af[i][c] = (short)f2bf(...)`,
            `f32x8_to_bf16(m)`) times the bf16 WcT;
          * fc_wgrad_gm_kernel: reads that bf16 Gm, and sums the bias gradient from the ROUNDED values
            (`bsum[jj] += bf2f((uint16_t)bf[e])`);
          * trunk_f32.hip: nothing is rounded.
          G * g_scale is one fp32 multiply in the kernels and here.  Bound: n 2^-23 (|A|^T @ |B|), n the full
          reduction length (weight gradients: T*E*Ho*Wo times the paths expressing the module -- any order of the
          atomics; input gradients: active slots x contributing taps x Cout).  Modules no path expresses: exactly 0.

Every output buffer carries 64 extra rows of a sentinel that must survive, every float input 64 extra rows of NaN
(uint8 frames: 255), and dX is pre-filled with NaN: the kernels must write all of it.  The measured
max |hip - ref| / bound per launcher is recorded under ``trunk_geometry_f64`` in tests/data/numerics_measured.json
(``PATHNET_RECORD_NUMERICS``) -- for the record only, the assertion is the derived bound, element by element.
"""
import math
import os

import numpy as np
import pytest
import torch

import numerics_budget as budget
from pathnet_gym_amd.algo.ga import get_geopath
from pathnet_gym_amd.config import LayerSpec, PathNetConfig, preset
from pathnet_gym_amd.models.pathnet import ParamStore, trunk_forward_ref
from pathnet_gym_amd.ops.pathnet_ops import geometry_unsupported_reason

gpu = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -23
PAD = 64                      # sentinel rows after every buffer
SENT = -3.0                   # exact in bf16 and fp32
BITS_SENT8, BITS_SENT16 = 0xA5, 0x5A5A
IN_SCALE = float(np.float32(1.0 / 255.0))          # what the launchers receive as a C float

# id -> (input shape, [(kind, kernel, stride) | (kind, width)], E)
GEOMS = {
    "G1": ((36, 28, 4), [("conv", 4, 2), ("conv", 3, 1), ("conv", 3, 2), ("fc", 256), ("fc", 64)], 16),
    "G2": ((45, 33, 4), [("conv", 6, 3), ("conv", 2, 1), ("conv", 5, 2), ("fc", 96), ("fc", 32)], 16),
    "G3": ((24, 24, 4), [("conv", 4, 4), ("conv", 3, 1), ("fc", 64)], 4),
    "G4": ((20, 16, 8), [("conv", 3, 1), ("conv", 3, 2), ("fc", 64)], 4),
    "G5": ((30, 22, 4), [("conv", 5, 2), ("conv", 3, 1), ("fc", 64)], 16),
}
FC_WIDTHS = (64, 256, 256, 96, 32)                  # section "fc dispatch": vector input of 4 -> these


def random_masks(P, L, M, N, seed=0, with_edge=True):
    """tests/test_hip_kernels.py random_masks: an empty layer, a path with all modules, a single (last) module."""
    rng = np.random.RandomState(seed)
    m = np.stack([get_geopath(L, M, N, rng) for _ in range(P)])
    if with_edge and P >= 3:
        m[0, 1, :] = 0
        m[1, :, :] = 1
        m[2, 0, :] = 0
        m[2, 0, M - 1] = 1
    return m


def geom_cfg(name, M=10, N=4):
    inp, layers, _ = GEOMS[name]
    specs = [LayerSpec("conv", 8, l[1], l[2]) if l[0] == "conv" else LayerSpec("fc", l[1]) for l in layers]
    return PathNetConfig(L=len(specs), M=M, N=N, input_shape=inp, layers=specs, trunk_scale="M", num_actions=6)


def fc_cfg(M=10, N=4):
    return PathNetConfig(L=len(FC_WIDTHS), M=M, N=N, input_shape=(4,), layers=[LayerSpec("fc", w) for w in FC_WIDTHS],
                         trunk_scale="M", num_actions=2)


# ---------------------------------------------------------------------------------------------------------------
# float64 reference (CPU tensors; also run by the CPU tests below)
# ---------------------------------------------------------------------------------------------------------------
class Layer:
    """Geometry of one trunk layer, from PathNetConfig.layer_shapes()."""

    def __init__(self, cfg, l):
        spec = cfg.layers[l]
        ins, outs, K, cin = cfg.layer_shapes()[l]
        self.l, self.kind, self.K, self.Cout = l, spec.kind, K, spec.out
        self.in_feat = int(math.prod(ins))
        self.last = l == cfg.L - 1
        self.out_scale = float(np.float32(1.0 / cfg.M)) if (self.last and cfg.trunk_scale == "M") else 1.0
        if spec.kind == "conv":
            self.Hin, self.Win, self.Cin = ins
            self.KH = self.KW = spec.kernel
            self.S = spec.stride
            self.Ho, self.Wo = outs[0], outs[1]
            self.HWo = self.Ho * self.Wo
            self.in_scale = IN_SCALE if l == 0 else 1.0
        else:
            self.HWo, self.in_scale = 1, 1.0
        self.out_feat = self.HWo * self.Cout


def im2col(x, ly, shifted=False):
    """x [R, Hin, Win, Cin] -> [R, Ho*Wo, K], k = (kh*KW + kw)*Cin + ci.  ``shifted`` (negative control): the last 4 k
    of every kernel row come from kernel row kh + 1 -- what one 8-wide load does to a row of KW*Cin % 8 == 4 values."""
    R = x.shape[0]
    cols = x.new_zeros(R, ly.Ho, ly.Wo, ly.KH, ly.KW, ly.Cin)
    for kh in range(ly.KH):
        for kw in range(ly.KW):
            cols[:, :, :, kh, kw] = x[:, kh:kh + ly.S * (ly.Ho - 1) + 1:ly.S, kw:kw + ly.S * (ly.Wo - 1) + 1:ly.S]
    cols = cols.reshape(R, ly.HWo, ly.KH, ly.KW * ly.Cin)
    if shifted:
        bad = cols.clone()
        bad[:, :, :-1, -4:] = cols[:, :, 1:, -4:]
        cols = bad
    return cols.reshape(R, ly.HWo, ly.K)


def col2im(dcol, ly):
    """Transpose of im2col: dcol [R, Ho*Wo, K] -> [R, Hin, Win, Cin]."""
    R = dcol.shape[0]
    d = dcol.reshape(R, ly.Ho, ly.Wo, ly.KH, ly.KW, ly.Cin)
    dx = dcol.new_zeros(R, ly.Hin, ly.Win, ly.Cin)
    for kh in range(ly.KH):
        for kw in range(ly.KW):
            dx[:, kh:kh + ly.S * (ly.Ho - 1) + 1:ly.S, kw:kw + ly.S * (ly.Wo - 1) + 1:ly.S] += d[:, :, :, kh, kw]
    return dx


def path_rows(x, ly, p, shifted=False):
    """GEMM rows of path p: x [T, P, E, in_feat] -> [T*E*HWo, K] float64, row = (s, pos) with s = t*E + e."""
    T, _, E, _ = x.shape
    xp = x[:, p].double().reshape(T * E, -1)
    if ly.kind == "conv":
        return im2col(xp.reshape(T * E, ly.Hin, ly.Win, ly.Cin), ly, shifted).reshape(T * E * ly.HWo, ly.K)
    return xp[:, :ly.K]


def forward_ref(ly, x, W, b, acts, bf16_store, shifted=False, offset=0.0, bias_slack=None):
    """x [T, P, E, in_feat] (raw: uint8 pixels for layer 0), W [M, K, Cout], b [M, Cout] float64, acts[p] = module of
    every active slot  ->  y, its bound [T, P, E, out_feat], and per path pre / slot bound [cnt, T*E*HWo, Cout].
    ``offset`` (fp16-offset operands, csrc/conv_fast.hip F16): every operand enters the GEMM as offset + x, so
    pre = in_scale * ((offset + x) @ W) + b with ``b`` the corrected bias and the bound on (offset + |x|) @ |W|;
    ``bias_slack`` [M, Cout] is added to the slot bound (the rounding of that corrected bias)."""
    T, P, E, _ = x.shape
    y = torch.zeros(T, P, E, ly.out_feat, dtype=torch.float64)
    yb = torch.zeros_like(y)
    pres, bounds = [], []
    for p in range(P):
        A = path_rows(x, ly, p, shifted)
        if offset:
            A = A + offset
        pre = torch.stack([ly.in_scale * (A @ W[j]) + b[j] for j in acts[p]]) if len(acts[p]) else \
            torch.zeros(0, A.shape[0], ly.Cout, dtype=torch.float64)
        bnd = torch.stack([ly.K * EPS * ly.in_scale * (A.abs() @ W[j].abs()) for j in acts[p]]) + EPS * pre.abs() \
            if len(acts[p]) else torch.zeros_like(pre)
        if bias_slack is not None and len(acts[p]):
            bnd = bnd + torch.stack([bias_slack[j] for j in acts[p]])[:, None, :]
        yp = ly.out_scale * torch.relu(pre).sum(0)
        ybp = ly.out_scale * bnd.sum(0)
        if bf16_store:
            ybp = ybp + 2.0 ** -8 * yp.abs()
        y[:, p] = yp.reshape(T, E, ly.out_feat)
        yb[:, p] = ybp.reshape(T, E, ly.out_feat)
        pres.append(pre)
        bounds.append(bnd)
    return y, yb, pres, bounds


def backward_ref(ly, x, G, bits, Wd, acts, M, g_scale, round_w=False, round_d=False, bias_rounded=False,
                 want_dx=True, scale_after=False):
    """Gradients of one layer from G [T, P, E, out_feat] and the ReLU bits[p] [cnt, R, Cout] (bool): dW [M, K, Cout],
    db [M, Cout], dX [T, P, E, in_feat] (None unless want_dx) and their elementwise bounds.  x and the masked
    G * g_scale (one multiply in the dtype of G: fp32 as in the kernels, float64 in the CPU oracle test) enter the
    weight gradient, ``Wd`` [M, K, Cout] the input gradient.  round_w / round_d: the masked gradient is rounded to
    bf16 before the weight / input gradient GEMM; bias_rounded: the bias gradient sums those rounded values.
    scale_after (weight gradient only): the masked G is rounded unscaled and g_scale multiplies the sums."""
    assert not (scale_after and want_dx)
    post = float(g_scale) if scale_after else 1.0
    if scale_after:
        g_scale = 1.0
    T, P, E, _ = x.shape
    dW = torch.zeros(M, ly.K, ly.Cout, dtype=torch.float64)
    bW = torch.zeros_like(dW)
    db = torch.zeros(M, ly.Cout, dtype=torch.float64)
    bb = torch.zeros_like(db)
    users = torch.zeros(M, dtype=torch.float64)
    dX = bX = None
    if want_dx:
        dX = torch.zeros(T, P, E, ly.in_feat, dtype=torch.float64)
        bX = torch.zeros_like(dX)
    gs = G * torch.tensor(g_scale, dtype=G.dtype)
    for p in range(P):
        if not len(acts[p]):
            continue
        A = path_rows(x, ly, p)
        R = A.shape[0]
        gp = gs[:, p].reshape(R, ly.Cout)
        dcol = torch.zeros(R, ly.K, dtype=torch.float64)
        bcol = torch.zeros_like(dcol)
        for a, j in enumerate(acts[p]):
            gm = torch.where(bits[p][a], gp, torch.zeros_like(gp))
            gr = gm.to(torch.bfloat16).double() if (round_w or round_d or bias_rounded) else None
            gw = gr if round_w else gm.double()
            dW[j] += post * ly.in_scale * (A.t() @ gw)
            bW[j] += post * ly.in_scale * (A.abs().t() @ gw.abs())
            gb = gr if bias_rounded else gm.double()
            db[j] += post * gb.sum(0)
            bb[j] += post * gb.abs().sum(0)
            users[j] += 1
            if want_dx:
                gd = gr if round_d else gm.double()
                dcol += gd @ Wd[j].t()
                bcol += gd.abs() @ Wd[j].abs().t()
        if want_dx:
            if ly.kind == "conv":
                n = len(acts[p]) * -(-ly.KH // ly.S) * -(-ly.KW // ly.S) * ly.Cout
                dX[:, p] = col2im(dcol.reshape(T * E, ly.HWo, ly.K), ly).reshape(T, E, ly.in_feat)
                bX[:, p] = n * EPS * col2im(bcol.reshape(T * E, ly.HWo, ly.K), ly).reshape(T, E, ly.in_feat)
            else:
                n = len(acts[p]) * ly.Cout
                dX[:, p, :, :ly.K] = dcol.reshape(T, E, ly.K)
                bX[:, p, :, :ly.K] = n * EPS * bcol.reshape(T, E, ly.K)
    n_w = (T * E * ly.HWo * users)[:, None, None]
    return dict(dW=dW, bW=n_w * EPS * bW, db=db, bb=n_w[:, 0] * EPS * bb, dX=dX, bX=bX, users=users)


def compare(got, ref, bound):
    """The comparison every assertion goes through: element by element |got - ref| <= bound, never a norm.
    -> (violations, max |got - ref| / bound); a non-finite element is a violation."""
    got = got.double().cpu()
    err = (got - ref).abs()
    bad = ~(err <= bound)                   # NaN compares false: counted
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    return int(bad.sum()), float(ratio.max()) if ratio.numel() else 0.0


def within(name, got, ref, bound, ratios=None, key=None):
    nbad, worst = compare(got, ref, bound)
    print(f"{name}: max |hip - ref64| / bound = {worst:.3f} over {ref.numel()} elements")
    if ratios is not None:
        ratios[key] = max(ratios.get(key, 0.0), worst)
    assert nbad == 0, f"{name}: {nbad} of {ref.numel()} elements outside the derived bound (worst ratio {worst:.3g})"


def act_lists(mask):
    """[P][L] lists of active modules (ascending, the order of algo/ga.py compact_active)."""
    return [[list(np.nonzero(mask[p, l] > 0.5)[0]) for l in range(mask.shape[1])] for p in range(mask.shape[0])]


# ---------------------------------------------------------------------------------------------------------------
# CPU: the reference against the dense float64 oracle with autograd, and the comparison's negative controls
# ---------------------------------------------------------------------------------------------------------------
def _chain_ref(cfg, P, E, T, seed):
    """The float64 reference chained over the whole trunk (its own outputs as inputs, no rounding anywhere)."""
    g = torch.Generator().manual_seed(seed)
    mask = random_masks(P, cfg.L, cfg.M, cfg.N, seed=seed)
    acts = act_lists(mask)
    flat = (ParamStore(cfg, "cpu", seed=seed + 1).flat.double()).requires_grad_(True)
    st = ParamStore(cfg, "cpu", flat=flat)
    pixels = cfg.layers[0].kind == "conv"
    if pixels:
        x0 = torch.randint(0, 256, (T, P, E, int(math.prod(cfg.input_shape))), generator=g).double()
    else:
        x0 = torch.randn(T, P, E, cfg.input_shape[0], generator=g, dtype=torch.float64)
    layers = [Layer(cfg, l) for l in range(cfg.L)]
    if layers[-1].out_scale != 1.0:
        layers[-1].out_scale = 1.0 / cfg.M           # the dense oracle divides by M in float64, not by fp32(1 / M)
    xs, outs = [x0], []
    for ly in layers:
        y, _, pres, _ = forward_ref(ly, xs[-1], st.W(ly.l).detach(), st.b(ly.l).detach(),
                                    [a[ly.l] for a in acts], False)
        outs.append(pres)
        xs.append(y)
    return dict(mask=mask, acts=acts, flat=flat, st=st, layers=layers, xs=xs, pres=outs, g=g, pixels=pixels)


@pytest.mark.parametrize("name,E,T,M", [("G1", 2, 2, 10), ("G2", 2, 1, 10), ("G3", 3, 2, 16), ("G4", 2, 1, 10),
                                        ("G5", 2, 1, 10), ("fc", 5, 2, 10)])
def test_reference_matches_dense_float64_oracle(name, E, T, M):
    """forward_ref / backward_ref on the geometries of this file == trunk_forward_ref in float64 + autograd."""
    cfg = fc_cfg(M) if name == "fc" else geom_cfg(name, M)
    P = 4
    c = _chain_ref(cfg, P, E, T, seed=3)
    xin = c["xs"][0].reshape(T * P * E, *cfg.input_shape)
    if c["pixels"]:
        xin = xin * IN_SCALE
    m = torch.from_numpy(c["mask"]).double()
    mask = m.repeat_interleave(E, 0).repeat(T, 1, 1)
    feat = trunk_forward_ref(c["st"], xin, mask)
    ref = c["xs"][-1].reshape(T * P * E, -1)
    assert feat.shape == ref.shape
    assert float((feat.detach() - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    G = torch.randn(T, P, E, feat.shape[1], generator=c["g"], dtype=torch.float64)
    (feat * G.reshape(feat.shape)).sum().backward()
    gref = c["flat"].grad
    lay = c["st"].layout
    Gl = G
    for ly in reversed(c["layers"]):
        W = c["st"].W(ly.l).detach()
        bits = [pre > 0 for pre in c["pres"][ly.l]]
        r = backward_ref(ly, c["xs"][ly.l], Gl, bits, W, [a[ly.l] for a in c["acts"]], cfg.M, ly.out_scale,
                         want_dx=ly.l > 0)
        for j in range(cfg.M):
            sw, sb = lay.by_name[f"layer{ly.l}.module{j}.weight"], lay.by_name[f"layer{ly.l}.module{j}.bias"]
            gw = gref[sw.offset:sw.offset + sw.numel].view(ly.K, ly.Cout)
            gb = gref[sb.offset:sb.offset + sb.numel]
            scale = max(float(gw.abs().max()), 1e-30)
            assert float((r["dW"][j] - gw).abs().max()) <= 1e-10 * scale, (ly.l, j)
            assert float((r["db"][j] - gb).abs().max()) <= 1e-10 * max(float(gb.abs().max()), 1e-30), (ly.l, j)
            if r["users"][j] == 0:
                assert not gw.any() and not gb.any()
        Gl = r["dX"]


def test_comparison_reports_scaled_element_and_shifted_im2col():
    """Negative controls of compare(): one output element off by 2^-6, and the im2col of the 8-wide load that
    crosses a kernel row (KW*Cin = 20), must both be reported against the derived forward bound."""
    cfg = geom_cfg("G5")
    P, E, T = 3, 2, 1
    c = _chain_ref(cfg, P, E, T, seed=5)
    ly = c["layers"][0]
    W, b = c["st"].W(0).detach(), c["st"].b(0).detach()
    # the operands of the bf16 kernel: bf16 weights, bf16 store
    Wq = W.float().to(torch.bfloat16).double()
    acts = [a[0] for a in c["acts"]]
    y, yb, _, _ = forward_ref(ly, c["xs"][0], Wq, b, acts, True)
    assert compare(y.clone(), y, yb)[0] == 0
    off = y.clone().reshape(-1)
    i = int(off.abs().argmax())
    off[i] *= 1.0 + 2.0 ** -6
    nbad, worst = compare(off.reshape(y.shape), y, yb)
    assert nbad == 1 and worst > 1.0, (nbad, worst)
    ybad, _, _, _ = forward_ref(ly, c["xs"][0], Wq, b, acts, True, shifted=True)
    nbad, worst = compare(ybad, y, yb)
    assert nbad > 0.5 * y.numel() and worst > 1.0, (nbad, worst)
    # ... and in fp32 (no store rounding), where the bound is ~2^-15 of the value
    y32, yb32, _, _ = forward_ref(ly, c["xs"][0], W, b, acts, False)
    off = y32.clone().reshape(-1)
    off[int(off.abs().argmax())] *= 1.0 + 2.0 ** -6
    assert compare(off.reshape(y32.shape), y32, yb32)[0] == 1


@pytest.mark.parametrize("dtype", ["bf16", "fp32", "fp32x"])
def test_envelope_refuses_by_layer_and_reason(dtype):
    """A first layer with Cin = 4 and an odd kernel (--kernel_num 5,4,3), a fan-in past the weight gradient's 16
    k-tiles, and more modules than the kernels hold are refused at construction -- by layer and reason, in every
    precision, before any GPU is needed; the geometries this file runs are accepted."""
    from pathnet_gym_amd.models.acnet import ACPathNet
    for name in ("G1", "G2", "G3", "G4"):
        assert geometry_unsupported_reason(geom_cfg(name), dtype) is None
    assert geometry_unsupported_reason(geom_cfg("G3", M=16), dtype) is None
    assert geometry_unsupported_reason(fc_cfg(), dtype) is None
    assert geometry_unsupported_reason(preset("pong").net, dtype) is None
    assert geometry_unsupported_reason(preset("reference").net, dtype) is None
    why = geometry_unsupported_reason(geom_cfg("G5"), dtype)
    assert "conv layer 0" in why and "KW*Cin = 5*4 = 20" in why and "multiple of 8" in why
    odd = PathNetConfig(L=5, M=10, N=4, layers=[LayerSpec("conv", 8, 5, 4), LayerSpec("conv", 8, 4, 2),
                                                LayerSpec("conv", 8, 3, 1), LayerSpec("fc", 256), LayerSpec("fc", 256)])
    assert "conv layer 0" in geometry_unsupported_reason(odd, dtype)
    wide = PathNetConfig(L=3, M=10, N=4, input_shape=(40, 40, 4),
                         layers=[LayerSpec("conv", 8, 4, 2), LayerSpec("conv", 8, 6, 1), LayerSpec("fc", 64)])
    why = geometry_unsupported_reason(wide, dtype)           # K = 6*6*8 = 288 -> KP 288 > 256
    assert "conv layer 1" in why and "weight gradient" in why
    huge = PathNetConfig(L=3, M=10, N=4, input_shape=(40, 40, 4),
                         layers=[LayerSpec("conv", 8, 4, 2), LayerSpec("conv", 8, 9, 1), LayerSpec("fc", 64)])
    why = geometry_unsupported_reason(huge, dtype)           # K = 9*9*8 = 648 -> KP 672 > 512
    assert "conv layer 1" in why and "forward" in why
    assert "M=17" in geometry_unsupported_reason(fc_cfg(M=17), dtype)
    # the constructor raises that reason (the trainer builds the model first: it fails there, in every precision;
    # fp32x has no kernel for such a trunk either and falls back to fp32 before it)
    with pytest.raises(NotImplementedError, match=r"conv layer 0.*KW\*Cin = 5\*4 = 20"):
        ACPathNet(geom_cfg("G5"), 2, "cpu", "hip", compute_dtype="fp32" if dtype == "fp32x" else dtype)


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
RATIOS = {}


def _record(ratios):
    """PATHNET_RECORD_NUMERICS=<file>: keep the max ratio to the derived bound per launcher (trunk_geometry_f64)."""
    for k, v in ratios.items():
        RATIOS[k] = max(RATIOS.get(k, 0.0), v)
    rec = os.environ.get("PATHNET_RECORD_NUMERICS")
    if not rec:
        return
    import json
    d = budget._load(rec)
    t = d.setdefault("trunk_geometry_f64", {})
    for k, v in ratios.items():
        t[k] = max(float(v), float(t.get(k, 0.0)))
    os.makedirs(os.path.dirname(rec) or ".", exist_ok=True)
    with open(rec, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def fwd_branch(hp, l, rows):
    """The launcher (and branch) layer_fwd takes for layer l at ``rows`` = T*E rows per path."""
    g = hp.geoms[l]
    if hp.f32:
        return "launch_conv_fwd_f32" if g.kind == "conv" else f"launch_fc_fwd_f32.t{32 if rows <= 32 else 64}"
    if g.kind == "conv":
        return "launch_conv_fwd"
    if rows <= 32 and g.Cout % 64 == 0:
        return "launch_fc_fwd." + ("mw1" if rows <= 16 else "mw2_k1408" if g.KP == 1408 else
                                   "mw2_k256" if g.KP == 256 else "mw2")
    return f"launch_fc_fwd.t{32 if rows <= 32 else 64}"


def make_model(cfg, P, mask, dtype, seed=3):
    from pathnet_gym_amd.models.acnet import ACPathNet
    m = ACPathNet(cfg, P, DEV, "hip", seed=seed, compute_dtype=dtype)
    m.set_paths(mask)
    return m


def padded(rows, feat, dtype, fill, tail):
    """[rows + PAD, feat] buffer: ``fill`` in the rows, ``tail`` in the PAD rows after them."""
    t = torch.full((rows + PAD, feat), fill, dtype=dtype, device=DEV)
    t[rows:] = tail
    return t


def as_input(y_rows, dtype):
    """A layer input holding ``y_rows`` [rows, feat] followed by PAD rows of NaN (uint8: 255)."""
    t = padded(y_rows.shape[0], y_rows.shape[1], dtype, 0, 255 if dtype == torch.uint8 else float("nan"))
    t[:y_rows.shape[0]] = y_rows
    return t


def check_operand_copies(m, layers):
    """hp.Wc[l] == cast(W) in [M][Cout][KP], zero for K <= k < KP; hp.WcT[l] (fc, l > 0) its transpose -- bit for bit
    (launch_refresh_weights / launch_refresh_weights_f32)."""
    hp = m.hip
    for ly in layers:
        g = hp.geoms[ly.l]
        assert g.KP % 32 == 0 and g.KP >= ly.K and g.K == ly.K
        W = m.store.W(ly.l).detach()                                     # [M, K, Cout] fp32 master
        want = torch.zeros(m.cfg.M, ly.Cout, g.KP, dtype=hp.act_dtype, device=DEV)
        want[:, :, :ly.K] = W.to(hp.act_dtype).permute(0, 2, 1)
        bits_of = (lambda t: t.view(torch.int16)) if hp.act_dtype == torch.bfloat16 else (lambda t: t.view(torch.int32))
        assert torch.equal(bits_of(hp.Wc[ly.l]), bits_of(want)), f"Wc[{ly.l}]"
        assert not hp.Wc[ly.l][:, :, ly.K:].any(), f"Wc[{ly.l}] K padding"
        if ly.kind == "fc" and ly.l > 0:
            assert torch.equal(bits_of(hp.WcT[ly.l]), bits_of(want.permute(0, 2, 1).contiguous())), f"WcT[{ly.l}]"
        else:
            assert hp.WcT[ly.l] is None


def unpack_bits(ly, bits, rows, cnt, p, T, P, E):
    """ReLU bits of path p's slots [cnt, T*E*HWo, Cout] (bool) from a read-back bit-plane buffer."""
    if ly.kind == "conv":
        b = bits[:cnt, :rows].reshape(cnt, T, P, E * ly.HWo)[:, :, p].reshape(cnt, T * E * ly.HWo).to(torch.int32)
        return ((b[:, :, None] >> torch.arange(8, dtype=torch.int32)) & 1).bool()
    w = bits[:cnt, :rows].reshape(cnt, T, P, E, ly.Cout // 16)[:, :, p].reshape(cnt, T * E, ly.Cout // 16)
    w = w.to(torch.int32) & 0xFFFF
    return ((w[:, :, :, None] >> torch.arange(16, dtype=torch.int32)) & 1).bool().reshape(cnt, T * E, ly.Cout)


def run_trunk(cfg, P, E, T, dtype, seed, ratios, layers_to_run=None, x0=None, gm_min_k=None, backward=True):
    """Forward then backward of every layer through HipPathNet.layer_fwd / layer_bwd on padded buffers of the
    test's own, each against the float64 reference on what the kernel read.  -> {launcher branch names}."""
    mask = random_masks(P, cfg.L, cfg.M, cfg.N, seed=seed)
    m = make_model(cfg, P, mask, dtype, seed=seed + 1)
    hp = m.hip
    if gm_min_k is not None:
        hp.fc_wgrad_gm_min_k = gm_min_k
    f32 = dtype == "fp32"
    adt = torch.float32 if f32 else torch.bfloat16
    layers = [Layer(cfg, l) for l in range(cfg.L)]
    check_operand_copies(m, layers)
    acts_all = act_lists(mask)
    idx, cnt = m.act_idx.cpu().numpy(), m.act_cnt.cpu().numpy()
    for p in range(P):
        for l in range(cfg.L):
            assert list(idx[p, l, :cnt[p, l]]) == acts_all[p][l]       # what the kernels read == the reference's slots
    B = P * E
    g = torch.Generator().manual_seed(seed)
    pixels = cfg.layers[0].kind == "conv"
    if x0 is not None:
        X = x0
    elif pixels:
        X = as_input(torch.randint(0, 256, (T * B, layers[0].in_feat), generator=g, dtype=torch.uint8).to(DEV),
                     torch.uint8)
    elif f32:
        X = as_input(torch.randn(T * B, cfg.input_shape[0], generator=g).to(DEV), torch.float32)
    else:
        from pathnet_gym_amd.ops.envs import obs_to_bf16_padded
        X = as_input(obs_to_bf16_padded(torch.randn(T * B, cfg.input_shape[0], generator=g).to(DEV)), torch.bfloat16)
    branches = set()
    saved = {}
    for ly in layers:
        if layers_to_run is not None and ly.l not in layers_to_run:
            continue
        l = ly.l
        gl = hp.geoms[l]
        Y = padded(T * B, ly.out_feat, adt, float("nan"), SENT)
        rows = T * B * ly.HWo
        if ly.kind == "conv":
            bits = torch.full((cfg.M, rows + PAD), BITS_SENT8, dtype=torch.uint8, device=DEV)
        else:
            bits = torch.full((cfg.M, rows + PAD, ly.Cout // 16), BITS_SENT16, dtype=torch.int16, device=DEV)
        hp.layer_fwd(l, X, Y, bits, P, E, T, 0, rows + PAD)
        torch.cuda.synchronize()
        name = fwd_branch(hp, l, T * E)
        branches.add(name)
        # ---- reference on what the kernel read ----
        xin = X[:T * B].cpu()
        xin = xin.double().reshape(T, P, E, -1) if xin.dtype != torch.uint8 else xin.reshape(T, P, E, -1)
        W64 = hp.Wc[l][:, :, :ly.K].permute(0, 2, 1).double().cpu()
        b64 = m.store.b(l).detach().double().cpu()
        acts = [a[l] for a in acts_all]
        y, yb, pres, bnds = forward_ref(ly, xin, W64, b64, acts, not f32)
        within(f"{dtype} layer {l} {name} Y", Y[:T * B].reshape(T, P, E, -1), y, yb, ratios, name)
        assert bool((Y[T * B:] == SENT).all()), f"layer {l}: Y sentinel rows overwritten"
        hb = bits.cpu()
        sent = BITS_SENT8 if ly.kind == "conv" else BITS_SENT16
        assert bool((hb[:, rows:] == sent).all()), f"layer {l}: ReLU-bit sentinel rows overwritten"
        relu_bits, left_out, total = [], 0, 0
        for p in range(P):
            c = len(acts[p])
            got = unpack_bits(ly, hb, rows, c, p, T, P, E)
            sure = pres[p].abs() > bnds[p]
            assert bool((got == (pres[p] > 0))[sure].all()), f"layer {l} path {p}: ReLU bits differ from pre64 > 0"
            left_out += int((~sure).sum())
            total += sure.numel()
            relu_bits.append(got)
            if c < cfg.M:             # slots the path does not have: untouched
                un = hb[c:, :rows].reshape(cfg.M - c, T, P, -1)[:, :, p]
                assert bool((un == sent).all()), f"layer {l} path {p}: bits of inactive slots written"
        assert left_out <= 0.01 * max(total, 1), f"layer {l}: {left_out}/{total} ReLU bits inside the bound"
        saved[l] = dict(X=X, xin=xin, bits=bits, relu=relu_bits, acts=acts, rows=rows)
        X = as_input(Y[:T * B], Y.dtype)
    if not backward:
        return branches
    # ---- backward, layer by layer, each on a random G of its own ----
    numel = m.store.flat.numel()
    for ly in layers:
        l = ly.l
        if l not in saved:
            continue
        s = saved[l]
        gl = hp.geoms[l]
        G = as_input(torch.randn(T * B, ly.out_feat, generator=g).to(DEV), torch.float32)
        grad = torch.zeros(numel + PAD * 8, dtype=torch.float32, device=DEV)
        grad[numel:] = SENT
        dX = padded(T * B, ly.in_feat, torch.float32, float("nan"), SENT) if l > 0 else None
        gm = (not f32 and ly.kind == "fc" and dX is not None and gl.Cout == 256 and gl.K >= hp.fc_wgrad_gm_min_k
              and hp.fc_wgrad_gm)
        hp.layer_bwd(l, s["X"], G, s["bits"], grad, dX, P, E, T, s["rows"] + PAD)
        torch.cuda.synchronize()
        g_scale = ly.out_scale
        Wd = None                          # the input gradient's weights: fp32 master (conv) / the WcT copy (fc)
        if l > 0:
            Wd = (m.store.W(l).detach() if ly.kind == "conv" else hp.WcT[l][:, :ly.K, :]).double().cpu()
        r = backward_ref(ly, s["xin"], G[:T * B].cpu().reshape(T, P, E, -1), s["relu"], Wd, s["acts"], cfg.M,
                         g_scale, round_w=not f32, round_d=(not f32 and ly.kind == "fc"), bias_rounded=gm,
                         want_dx=l > 0)
        sfx = "_f32" if f32 else ""
        wname = (f"launch_conv_wgrad{sfx}" if ly.kind == "conv" else
                 "launch_fc_wgrad_gm" if gm else f"launch_fc_wgrad{sfx}")
        branches.add(wname)
        lo, ch = gl.w_off, gl.chunk
        gh = grad[lo:lo + cfg.M * ch].reshape(cfg.M, ch).cpu()
        within(f"{dtype} layer {l} {wname} dW", gh[:, :ly.K * ly.Cout].reshape(cfg.M, ly.K, ly.Cout), r["dW"], r["bW"],
               ratios, wname + ".dW")
        within(f"{dtype} layer {l} {wname} db", gh[:, ly.K * ly.Cout:], r["db"], r["bb"], ratios, wname + ".db")
        for j in range(cfg.M):
            if r["users"][j] == 0:
                assert not gh[j].any(), f"layer {l}: module {j} is on no path but has a gradient"
        # nothing outside this layer's segment, and the sentinel after the buffer
        assert not grad[:lo].any() and not grad[lo + cfg.M * ch:numel].any(), f"layer {l}: gradient outside the layer"
        assert bool((grad[numel:] == SENT).all()), f"layer {l}: gradient sentinel overwritten"
        if l > 0:
            dname = (f"launch_conv_dgrad{sfx}" if ly.kind == "conv" else "launch_fc_dgrad_f32" if f32 else
                     "launch_fc_dgrad." + ("lds" if gl.Cout == 256 else "generic"))
            branches.add(dname)
            within(f"{dtype} layer {l} {dname} dX", dX[:T * B].reshape(T, P, E, -1), r["dX"], r["bX"], ratios, dname)
            assert bool((dX[T * B:] == SENT).all()), f"layer {l}: dX sentinel rows overwritten"
    return branches


def _geometry_case(name, dtype, T, E=None, M=10, seed=11):
    cfg = geom_cfg(name, M=M)
    E = GEOMS[name][2] if E is None else E
    ratios = {}
    br = run_trunk(cfg, 4, E, T, dtype, seed, ratios)
    print("launcher branches:", sorted(br))
    _record(ratios)
    return br


@gpu
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_g1_odd_output_padded_k_lds_dgrad(hip_lib, dtype, T):
    """36x28x4: 17x13 / 15x11 / 7x5 outputs, K = 72 padded to 96, K = 280 to 288, 16*221 rows end inside a 64-row
    workgroup, the LDS fc dgrad (256 wide) on the last-but-one layer."""
    br = _geometry_case("G1", dtype, T)
    if dtype == "bf16":
        assert {"launch_conv_fwd", "launch_conv_wgrad", "launch_conv_dgrad", "launch_fc_dgrad.lds"} <= br


@gpu
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_g2_stride3_k_equals_kp_narrow_fc(hip_lib, dtype, T):
    """45x33x4: stride 3, a 2x2 kernel with K == KP == 32, K = 200, fc widths 96 and 32 (Cout % 64 != 0: the tile
    kernels and the generic fc dgrad)."""
    br = _geometry_case("G2", dtype, T)
    if dtype == "bf16":
        assert {"launch_fc_dgrad.generic", "launch_fc_fwd.t32" if T == 1 else "launch_fc_fwd.t64"} <= br


@gpu
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("E,M", [(4, 10), (12, 10), (4, 16)], ids=["E4", "E12", "E4-M16"])
def test_g3_small_e_and_sixteen_modules(hip_lib, dtype, T, E, M):
    """24x24x4, kernel == stride: E = 4 and 12 (not multiples of 16); M = 16 with one path expressing all 16
    modules of every layer, the kernels' MAXM."""
    _geometry_case("G3", dtype, T, E=E, M=M)


@gpu
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_g4_uint8_first_layer_with_eight_channels(hip_lib, dtype, T):
    """20x16x8 uint8: a first layer with Cin = 8 and KW*Cin = 24."""
    _geometry_case("G4", dtype, T)


@gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp32", "fp32x"])
def test_g5_kernel_row_not_a_multiple_of_8_is_refused(hip_lib, dtype):
    """30x22x4 k5: KW*Cin = 20.  conv_fwd_kernel / conv_wgrad_kernel load 8 consecutive k with one vector load from
    koff[k/8]; k = (kh*KW + kw)*Cin + ci is contiguous only inside a kernel row, so k = 20..23 would be read from
    kernel row 0 (test_comparison_reports_scaled_element_and_shifted_im2col shows what that computes).  The model
    and the trainer refuse it at construction, by layer and reason, and so do the launchers themselves."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    from pathnet_gym_amd.ops import _lib
    cfg = geom_cfg("G5")
    if dtype != "fp32x":
        with pytest.raises(NotImplementedError, match=r"conv layer 0.*KW\*Cin = 5\*4 = 20"):
            make_model(cfg, 4, random_masks(4, cfg.L, cfg.M, cfg.N), dtype)
    tc = preset("pong")
    tc.net, tc.paths, tc.envs_per_path, tc.compute_dtype = cfg, 4, 16, dtype
    tc.a2c.t_max = 2
    with pytest.raises(NotImplementedError, match=r"conv layer 0.*KW\*Cin = 5\*4 = 20"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            PathNetTrainer(tc, device=DEV)
    # the launchers: argument checks only, nothing is launched (null pointers never reach a kernel)
    z = torch.zeros(64, dtype=torch.int32, device=DEV)
    for fn, extra in (("launch_conv_fwd", (0, 1, 1.0, 1.0)), ("launch_conv_fwd_f32", (0, 1, 1.0, 1.0))):
        with pytest.raises(RuntimeError, match="code -1"):
            _lib.call(fn, z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 0, 808,
                      z.data_ptr(), z.data_ptr(), 0, 3, 10, 30, 22, 4, 5, 5, 2, 13, 9, 100, 128, 4, 16, 1, *extra[:1],
                      16 * 4 * 117, extra[2], extra[3], _lib.stream())
    with pytest.raises(RuntimeError, match="code -1"):
        _lib.call("launch_conv_wgrad", z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), 0, 800, 808,
                  z.data_ptr(), z.data_ptr(), 0, 3, 10, 30, 22, 4, 5, 5, 2, 13, 9, 100, 128, 4, 16, 1, 16 * 4 * 117,
                  32, 1.0, 1.0, _lib.stream())


# -- fc dispatch and row edges ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("E", [1, 15, 16, 17, 31, 32, 33, 64, 65, 130])
def test_fc_dispatch_and_row_edges(hip_lib, dtype, E):
    """Vector trunk 4 -> 64 -> 256 -> 256 -> 96 -> 32, P = 3, T = 1: every row-count branch of launch_fc_fwd
    (module-per-wave with 1 and 2 row tiles, KP == 256 unrolled or not, the 32- and 64-row tile kernels), both fc
    dgrad kernels, and both fc weight-gradient kernels on the 256-wide layers -- against the same reference."""
    cfg = fc_cfg()
    ratios = {}
    br = run_trunk(cfg, 3, E, 1, dtype, 20 + E, ratios)
    if dtype == "bf16":
        want = {"launch_fc_fwd.mw1", "launch_fc_fwd.t32"} if E <= 16 else \
            {"launch_fc_fwd.mw2", "launch_fc_fwd.mw2_k256", "launch_fc_fwd.t32"} if E <= 32 else {"launch_fc_fwd.t64"}
        assert want | {"launch_fc_dgrad.lds", "launch_fc_dgrad.generic", "launch_fc_wgrad"} <= br, br
        assert "launch_fc_wgrad_gm" not in br
        br2 = run_trunk(cfg, 3, E, 1, dtype, 20 + E, ratios, gm_min_k=64)
        assert "launch_fc_wgrad_gm" in br2, br2
        br |= br2
    print("launcher branches:", sorted(br))
    _record(ratios)


@gpu
def test_fc_fwd_k1408_two_row_tiles(hip_lib):
    """FC_MW(2, 44): the reference pixel trunk's fc1 (KP == 1408) at 17..32 rows per path -- forward of layer 3 only,
    on a random bf16 activation buffer of the test's own."""
    cfg = preset("pong").net
    cfg.trunk_scale = "M"
    P, E, T = 2, 32, 1
    g = torch.Generator().manual_seed(5)
    x = as_input((torch.randn(T * P * E, 1408, generator=g).abs() * 0.5).to(torch.bfloat16).to(DEV), torch.bfloat16)
    ratios = {}
    br = run_trunk(cfg, P, E, T, "bf16", 31, ratios, layers_to_run=[3], x0=x, backward=False)
    assert br == {"launch_fc_fwd.mw2_k1408"}, br
    _record(ratios)


# -- one end-to-end update per precision on G1 ---------------------------------------------------------------------
class SyntheticFrames:
    """A device-resident env of G1's frame shape for the engine (envs/base.py VecEnv surface + step_into): the new
    frame is a hash of the env index, the step counter and the action; an episode ends every 5 steps.  In-place
    torch ops only, so a step is capturable in the rollout hipGraph."""
    graph_safe = True
    supports_ring = False
    reward_threshold = float("inf")
    max_episode_steps = 0
    id = "SyntheticFrames"
    id_base = 0

    def __init__(self, num_envs, shape, num_actions, device):
        self.num_envs, self.num_actions, self.device = num_envs, num_actions, device
        self.obs_shape, self.obs_dtype = tuple(shape), torch.uint8
        H, W, C = shape
        self.obs = torch.zeros(num_envs, H, W, C, dtype=torch.uint8, device=device)
        self.t = torch.zeros(num_envs, dtype=torch.int64, device=device)
        self.ret = torch.zeros(num_envs, device=device)
        self.pix = (torch.arange(H * W, device=device).view(1, H, W) * 7
                    + torch.arange(num_envs, device=device).view(-1, 1, 1) * 13)

    def set_id_base(self, base):
        self.id_base = int(base)

    def seed(self, seed):
        pass

    def close(self):
        pass

    def _frame(self, actions):
        return ((self.pix + (self.t * 31 + actions.long() * 57).view(-1, 1, 1)) % 256).to(torch.uint8)

    def reset(self):
        self.t.zero_()
        self.ret.zero_()
        f = self._frame(torch.zeros(self.num_envs, dtype=torch.int64, device=self.device))
        self.obs.copy_(f[..., None].expand_as(self.obs))
        return self.obs.clone()

    def step_into(self, actions, obs_in, obs_out, reward, done, epret):
        self.t.add_(1)
        f = self._frame(actions.view(-1))
        oi = obs_in.view(self.obs.shape)
        oo = obs_out.view(self.obs.shape)
        oo[..., :-1].copy_(oi[..., 1:])
        oo[..., -1].copy_(f)
        r = (actions.view(-1) % 2).float()
        d = (self.t % 5) == 0
        self.ret.add_(r)
        reward.copy_(r.view(reward.shape))
        done.copy_(d.view(done.shape).to(done.dtype))
        epret.copy_(torch.where(d, self.ret, torch.zeros_like(self.ret)).view(epret.shape))
        self.ret.mul_((~d).float())
        self.obs = oo


@gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp32x"])
def test_trainer_updates_on_g1(hip_lib, monkeypatch, dtype):
    """PathNetTrainer on a G1 trunk: two updates (eager, then from the captured graph) with finite weights, in bf16
    and -- asked for fp32x, which has no kernel for this trunk -- on the fp32 engine, with the fallback noted."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    tc = preset("pong")
    tc.net = geom_cfg("G1")
    tc.paths, tc.envs_per_path, tc.compute_dtype, tc.use_graph = 4, 16, dtype, True
    tc.a2c.t_max = 2
    monkeypatch.setattr(PathNetTrainer, "_make_env",
                        lambda self, task_idx: SyntheticFrames(self.P * self.E, tc.net.input_shape, tc.net.num_actions,
                                                               self.device))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tr = PathNetTrainer(tc, device=DEV)
    if dtype == "fp32x":
        assert tr.precision_note and "fp32x -> fp32" in tr.precision_note and "conv layer 0" in tr.precision_note
        assert tr.model.hip.f32 and not tr.model.hip.x3
    else:
        assert tr.precision_note is None and not tr.model.hip.f32
    assert tr.engine.use_graph and not tr.engine.ring
    w0 = tr.model.store.flat.detach().clone()
    for _ in range(2):
        tr.update()
    tr.flush()
    torch.cuda.synchronize()
    assert tr.engine.g_rollout is not None
    assert torch.isfinite(tr.model.store.flat).all()
    assert not torch.equal(w0, tr.model.store.flat.detach())
