"""The ordered bf16 LSTM weight gradient of csrc/lstm.hip (``launch_lstm_wgrad_ord``: per-chunk partial slabs added
in chunk order, no atomics) against plain float64 torch, with buffers of the test's own.

Operands and rounding are ``launch_lstm_wgrad``'s (tests/test_lstm_kernels.py): xh is bf16, dz enters the MFMA rounded
to bf16 and the bias sum unrounded, the products are exact in fp32.  The tolerance is derived, not measured:
``ref_wgrad``'s bound covers ANY summation tree of the R products (n = R, unit 2^-23), and the MFMA chain of a chunk
followed by the chunk-ordered slab sum is one such tree.  On top comes the one fp32 rounding of the final
``grad += sum`` of a value of at most |g0| + |xh|^T |bf(dz)|:

    |hip - ref64| <= R * 2^-23 * (|xh|^T |bf(dz)|)  +  2^-24 * 1.001 * (|g0| + |xh|^T |bf(dz)|)

which is the atomic kernel's test formula with ``adds = 1``; the bias likewise, R * 2^-23 * sum|dz| plus one add.
"""
import functools

import pytest
import torch

from test_lstm_kernels import DEV, SENT, bf, bits, gemm_bound, make_case, padded, ref_wgrad, within

gpu = pytest.mark.gpu
CHUNK = 4096                       # LORD_CHUNK of csrc/lstm.hip; run_ord asserts lstm_wgrad_ord_chunk_rows() == CHUNK
ONE_ADD = 2.0 ** -24 * 1.001
TAIL = 4096                        # sentinel floats after part[:part_numel]
R_EDGES = [1, 31, 32, 33, 95, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
SHAPES = [(F, H, R) for F, H in ((64, 128), (128, 64)) for R in R_EDGES] + [(256, 256, 95), (256, 256, 130)]


@functools.lru_cache(maxsize=None)
def case(F, H, R):
    """Inputs (CPU), the float64 reference and the derived bounds of one shape; computed once and never modified."""
    KK, G4 = F + H, 4 * H
    cs = make_case(F, H, 1, seed=53 + R + F)
    g = torch.Generator().manual_seed(59 + R + H)
    xh, dz = bf(torch.randn(R, KK, generator=g) * 0.5), torch.randn(R, G4, generator=g) * 0.1
    g0 = torch.randn(cs["flat"].numel(), generator=g) * 0.05
    ks, bs = slice(cs["k_off"], cs["k_off"] + KK * G4), slice(cs["b_off"], cs["b_off"] + G4)
    dK, bK, db, bb = ref_wgrad(xh, dz)
    absK = g0[ks].view(KK, G4).abs().double() + xh.double().abs().t() @ bf(dz).double().abs()
    absb = g0[bs].abs().double() + dz.double().abs().sum(0)
    return dict(F=F, H=H, R=R, KK=KK, G4=G4, k_off=cs["k_off"], b_off=cs["b_off"], xh=xh, dz=dz, g0=g0, ks=ks, bs=bs,
                dK=dK, db=db, gemmK=bK, gemmb=bb, absK=absK, absb=absb,
                tolK=bK + ONE_ADD * absK, tolb=bb + ONE_ADD * absb)


def increments(c, grad):
    """(dK, db) a launch added to grad (CPU fp32), in float64."""
    KK, G4 = c["KK"], c["G4"]
    return (grad[c["ks"]].view(KK, G4).double() - c["g0"][c["ks"]].view(KK, G4).double(),
            grad[c["bs"]].double() - c["g0"][c["bs"]].double())


# ---------------------------------------------------------------------------------------------------------------
# CPU: the slab scheme itself stays inside the derived bound
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 33, CHUNK + 1, 2 * CHUNK + 1])
def test_slab_scheme_emulated_in_fp32_is_inside_the_derived_bound_cpu(R):
    """An fp32 GEMM per chunk, the slabs added in chunk order in fp32, then + g0 in fp32: against float64 the
    increment is inside the bound, so the reference alone leaves the kernel its room."""
    c = case(64, 128, R)
    KK, G4 = c["KK"], c["G4"]
    sK, sb = torch.zeros(KK, G4), torch.zeros(G4)
    for r0 in range(0, R, CHUNK):
        xs, ds = c["xh"][r0:r0 + CHUNK], c["dz"][r0:r0 + CHUNK]
        sK = sK + xs.float().t() @ bf(ds).float()
        sb = sb + ds.sum(0)
    grad = c["g0"].clone()
    grad[c["ks"]] += sK.reshape(-1)
    grad[c["bs"]] += sb
    iK, ib = increments(c, grad)
    eK, eb = (iK - c["dK"]).abs(), (ib - c["db"]).abs()
    print(f"R={R}: worst err / bound  dK {float((eK / c['tolK']).max()):.4f}  db {float((eb / c['tolb']).max()):.4f}")
    assert bool((eK <= c["tolK"]).all()) and bool((eb <= c["tolb"]).all())
    assert bool((c["tolK"] > 0).all()) and bool((c["tolb"] > 0).all())


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
def part_buffer(lib, c, fill=SENT):
    n = lib.lstm_wgrad_ord_part_numel(c["F"], c["H"], c["R"])
    return torch.full((n + TAIL,), fill, dtype=torch.float32, device=DEV), n


def run_ord(c, part_fill=SENT):
    """One launch on fresh copies of the case's buffers -> grad (CPU).  NaN sentinel rows follow xh and dz, a
    sentinel tail follows part[:part_numel]; the tail must survive."""
    from pathnet_gym_amd.ops import _lib
    lib = _lib.lib()
    assert lib.lstm_wgrad_ord_chunk_rows() == CHUNK
    grad, xh_d, dz_d = c["g0"].to(DEV), padded(c["xh"]), padded(c["dz"])
    part, n = part_buffer(lib, c, part_fill)
    part[n:] = SENT
    _lib.call("launch_lstm_wgrad_ord", xh_d.data_ptr(), dz_d.data_ptr(), grad.data_ptr(), part.data_ptr(),
              c["k_off"], c["b_off"], c["F"], c["H"], c["R"], _lib.stream())
    torch.cuda.synchronize()
    assert bool((part[n:] == SENT).all()), "the tail after part[:part_numel] was written"
    assert bool(torch.isfinite(part[:n]).all()), "a slab entry was left unwritten"
    return grad.cpu()


@functools.lru_cache(maxsize=None)
def ord_result(F, H, R):
    return run_ord(case(F, H, R))


@gpu
@pytest.mark.parametrize("F,H,R", SHAPES)
def test_ord_wgrad_increment_matches_float64(hip_lib, F, H, R):
    """grad starts non-zero and the launch accumulates into it: the increment is compared, and every entry outside
    the kernel and bias ranges keeps its bits."""
    c = case(F, H, R)
    grad = ord_result(F, H, R)
    outside = torch.ones(c["g0"].numel(), dtype=torch.bool)
    outside[c["ks"]] = False
    outside[c["bs"]] = False
    assert torch.equal(bits(grad)[outside], bits(c["g0"])[outside])
    iK, ib = increments(c, grad)
    within("ord.dK", iK, c["dK"], c["tolK"])
    within("ord.db", ib, c["db"], c["tolb"])


@gpu
@pytest.mark.parametrize("F,H,R", [(64, 128, 95), (128, 64, CHUNK + 1), (64, 128, 2 * CHUNK + 1), (256, 256, 130)])
def test_ord_wgrad_is_bit_identical_run_to_run_and_ignores_stale_slabs(hip_lib, F, H, R):
    """The same inputs twice, then once more with part filled with NaN: the slabs are fully overwritten and nothing
    is summed with atomics, so all three gradients have the same bits."""
    c = case(F, H, R)
    a, b, n = ord_result(F, H, R), run_ord(c), run_ord(c, part_fill=float("nan"))
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(n))


@gpu
@pytest.mark.parametrize("F,H,R", [(64, 128, 33), (128, 64, CHUNK + 1), (64, 128, 2 * CHUNK + 1), (256, 256, 130)])
def test_ord_wgrad_agrees_with_the_atomic_kernel(hip_lib, F, H, R):
    """launch_lstm_wgrad (rows_per_chunk 2048, ceil(R / 2048) atomic adds per entry) on the same inputs: the two
    increments differ by at most the sum of the two derived bounds, elementwise."""
    from pathnet_gym_amd.ops import _lib
    c = case(F, H, R)
    rpc = 2048
    grad, xh_d, dz_d = c["g0"].to(DEV), padded(c["xh"]), padded(c["dz"])
    _lib.call("launch_lstm_wgrad", xh_d.data_ptr(), dz_d.data_ptr(), grad.data_ptr(), c["k_off"], c["b_off"], F, H, R,
              rpc, _lib.stream())
    torch.cuda.synchronize()
    aK, ab = increments(c, grad.cpu())
    oK, ob = increments(c, ord_result(F, H, R))
    adds = -(-R // rpc) * ONE_ADD
    atomK = gemm_bound(c["xh"].double().t(), bf(c["dz"]).double(), R) + adds * c["absK"]
    within("ord.dK vs atomic", oK, aK, c["tolK"] + atomK)
    within("ord.db vs atomic", ob, ab, c["tolb"] + c["gemmb"] + adds * c["absb"])


@gpu
@pytest.mark.parametrize("F,H,R", [(64, 128, 95), (128, 64, CHUNK + 1)])
def test_ord_wgrad_check_detects_a_two_percent_error(hip_lib, F, H, R):
    """Negative control: the kernel's own result scaled by 1.02 leaves the bound, in dK and in db."""
    c = case(F, H, R)
    iK, ib = increments(c, ord_result(F, H, R))
    with pytest.raises(AssertionError):
        within("ord.dK x 1.02", iK * 1.02, c["dK"], c["tolK"])
    with pytest.raises(AssertionError):
        within("ord.db x 1.02", ib * 1.02, c["db"], c["tolb"])


@gpu
def test_ord_launcher_rejects_bad_arguments_and_sizes_its_scratch(hip_lib):
    from pathnet_gym_amd.ops import _lib
    lib = hip_lib
    s = _lib.stream()
    # real, zero-filled buffers larger than any shape below, entered in the middle (negative offsets stay inside)
    buf = torch.zeros(1 << 20, device=DEV)
    p = buf.data_ptr() + (1 << 21)

    def wg(F, H, R, k_off=0, b_off=0, part=p):
        return lib.launch_lstm_wgrad_ord(p, p, p, part, k_off, b_off, F, H, R, s)

    assert wg(64, 65, 32) == -1 and wg(32, 64, 32) == -1 and wg(96, 64, 32) == -1 and wg(64, 96, 32) == -1
    assert wg(64, 64, 0) == -22 and wg(64, 64, -5) == -22 and wg(0, 64, 32) == -22 and wg(64, -64, 32) == -22
    assert wg(64, 64, 32, k_off=-1) == -22 and wg(64, 64, 32, b_off=-5) == -22 and wg(64, 64, 32, part=None) == -22
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0            # nothing ran
    C = lib.lstm_wgrad_ord_chunk_rows()
    assert C == CHUNK and C % 32 == 0 and 5 <= -(-20 * 2048 // C) <= 20       # ~10 slabs at the bench shape
    for F, H in ((64, 128), (256, 256)):
        slab = (F + H) * 4 * H + 4 * H
        prev = 0
        for R in (1, 32, C - 1, C, C + 1, 2 * C, 2 * C + 1, 20 * 2048):
            n = lib.lstm_wgrad_ord_part_numel(F, H, R)
            assert n == -(-R // C) * slab and n >= prev
            prev = n
    assert lib.lstm_wgrad_ord_part_numel(64, 64, 0) == 0 and lib.lstm_wgrad_ord_part_numel(0, 64, 32) == 0
