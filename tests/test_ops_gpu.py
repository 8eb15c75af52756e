"""Per-kernel parity tests, called through the C ABI (audiossl_amd.hip -> libatst_hip.so) on a real MI355X.

Each HIP kernel is compared with a plain fp32 formulation of the same op on the same (bf16-representable) inputs.
Tolerances: products of bf16 inputs are exact in fp32, so fp32 outputs differ only by accumulation order (<=2e-5 rel);
bf16 outputs carry one rounding (2^-9 = 2e-3 rel); integer / index work is bit-exact.
"""
import math
import os
import sys

import numpy as np
import pytest
import ctypes as C_
import torch

pytestmark = pytest.mark.gpu

from audiossl_amd import hip  # noqa: E402
from oracle import atst_oracle as O  # noqa: E402

DEV = "cuda"


def bf(x):
    return x.to(torch.bfloat16)


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    hip.load()
    yield
    torch.cuda.synchronize()


def gemm_nt(A, B, epi, out_dtype, **kw):
    M, K = A.shape
    N = B.shape[0]
    Cout = torch.empty(M, N, dtype=out_dtype, device=DEV)
    C2 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV) if epi == hip.EPI_BIAS_GELU else None
    hip.call("atst_gemm_nt_bf16", hip.ptr(A), hip.ptr(B), M, N, K, K, K, epi, None if kw.get("no_primary") else hip.ptr(Cout), N, hip.ptr(C2),
             hip.ptr(kw.get("bias")), hip.ptr(kw.get("resid")), hip.ptr(kw.get("row_scale")), kw.get("rps", 1),
             hip.ptr(kw.get("U")), hip.ptr(kw.get("table")), hip.ptr(kw.get("rowflag")), hip.ptr(kw.get("alt")), hip.ptr(kw.get("colsum")),
             hip.stream())
    return Cout, C2


@pytest.mark.parametrize("M,N,K", [(300, 384, 256), (128, 128, 64), (1027, 1152, 384), (512, 256, 4096),
                                   (8192 + 77, 1152, 384), (8192, 384, 1536),           # 256 x 384 tiles, ragged last tile
                                   (16384 + 40, 256, 768)])                             # fp32 output at >= 16 k rows: 256 x 128 tile (Frame heads)
def test_gemm_nt_plain(M, N, K):
    A, B = bf(rnd(M, K, seed=1)), bf(rnd(N, K, seed=2))       # asymmetric operands: catches transposed fragments
    ref = A.float() @ B.float().t()
    out, _ = gemm_nt(A, B, hip.EPI_F32, torch.float32)
    assert relerr(out, ref) < 2e-5
    bias = rnd(N, seed=3)
    outb, _ = gemm_nt(A, B, hip.EPI_BF16, torch.bfloat16, bias=bias)
    assert relerr(outb.float(), ref + bias) < 4e-3


@pytest.mark.parametrize("M,N,K", [(8192 + 77, 1152, 384), (8192, 384, 1536), (16384 + 256, 384, 128)])
def test_gemm_nt_row384_whole_line_main_loop_same_bits(M, N, K):
    """Hook 398 (round 6): the phased main loop of the 256 x 384 tile on 64-deep k-tiles of whole 128-B rows (two 80-KB slots) instead of 32-deep ones of
    64-B rows.  Every accumulator sees its k-steps in the same ascending order, so the fp32 output is BIT-identical to hook 397; ragged last row tile,
    K = 128 (two k-tiles: all prologue and tail), plain and fused epilogues."""
    lib = hip.load()
    A, B = bf(rnd(M, K, seed=1, scale=0.5)), bf(rnd(N, K, seed=2, scale=0.5))
    bias, resid = rnd(N, seed=3), rnd(M, N, seed=4)
    res = {}
    try:
        lib.atst_tune_gemm_variant(360)                                   # (keep the 8-wave tile for every shape)
        for hook in (397, 398):
            lib.atst_tune_gemm_variant(hook)
            f32, _ = gemm_nt(A, B, hip.EPI_F32, torch.float32, bias=bias)
            b16, _ = gemm_nt(A, B, hip.EPI_BF16, torch.bfloat16, bias=bias)
            x, _ = gemm_nt(A, B, hip.EPI_RESID, torch.float32, bias=bias, resid=resid)
            res[hook] = (f32, b16, x)
    finally:
        lib.atst_tune_gemm_variant(397); lib.atst_tune_gemm_variant(361)
    assert relerr(res[398][0], A.float() @ B.float().t() + bias) < 2e-5
    for a, b in zip(res[397], res[398]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("M,N,K", [(1536, 256, 12288), (512, 256, 12288), (1536, 384, 4096), (200, 128, 2048 + 32)])
def test_gemm_nt_f32_split_k(M, N, K):
    """fp32-output GEMMs with a handful of output tiles and a long K (the second head Linear: 24 tiles x 384 k-tiles) split K over the idle CUs;
    the last block of a tile sums the partial tiles in a fixed order: same result as the single-block-per-tile path (hook 380) to fp32
    summation order, bit-identical from run to run, bias added exactly once, ragged last K chunk, rows beyond M untouched."""
    A, B = bf(rnd(M, K, seed=1, scale=0.3)), bf(rnd(N, K, seed=2, scale=0.3))
    bias = rnd(N, seed=3)
    ref = A.double() @ B.double().t() + bias.double()
    outs = []
    try:
        for hook in (380, 381):
            hip.load().atst_tune_gemm_variant(hook)
            pad = torch.full((M + 3, N), 7.0, device=DEV)                          # rows beyond M must stay as they are
            hip.call("atst_gemm_nt_bf16", hip.ptr(A), hip.ptr(B), M, N, K, K, K, hip.EPI_F32, hip.ptr(pad), N, None, hip.ptr(bias), None, None, 1,
                     None, None, None, None, None, hip.stream())
            assert float((pad[M:] - 7.0).abs().max()) == 0.0
            outs.append(pad[:M].clone())
    finally:
        hip.load().atst_tune_gemm_variant(381)
    assert relerr(outs[0].double(), ref) < 2e-6 and relerr(outs[1].double(), ref) < 2e-6
    assert relerr(outs[1], outs[0]) < 1e-6
    again = torch.empty(M, N, device=DEV)
    for _ in range(3):                                                              # fixed summation order: the same bits every time
        hip.call("atst_gemm_nt_bf16", hip.ptr(A), hip.ptr(B), M, N, K, K, K, hip.EPI_F32, hip.ptr(again), N, None, hip.ptr(bias), None, None, 1,
                 None, None, None, None, None, hip.stream())
        assert torch.equal(again, outs[1])


@pytest.mark.parametrize("M,N,K", [(300, 384, 256), (1027, 1152, 384), (8192 + 77, 1152, 384), (8192, 384, 1536), (16384 + 130, 2304, 768)])
@pytest.mark.parametrize("has_bias", [True, False])
def test_gemm_nt_bf16_transposed_epilogue_same_bits(M, N, K, has_bias):
    """The store-only bf16 epilogue from transposed accumulators (hook 371) writes exactly what the staged fp32 epilogue (370, default) writes:
    same MFMA sums, same bias add, same rounding -- on 128- and 256-row tiles, ragged last tiles, with and without a bias."""
    A, B = bf(rnd(M, K, seed=1)), bf(rnd(N, K, seed=2))
    bias = rnd(N, seed=3) if has_bias else None
    outs = []
    try:
        for hook in (370, 371):
            hip.load().atst_tune_gemm_variant(hook)
            o, _ = gemm_nt(A, B, hip.EPI_BF16, torch.bfloat16, bias=bias)
            outs.append(o)
    finally:
        hip.load().atst_tune_gemm_variant(370)
    ref = A.float() @ B.float().t() + (bias if has_bias else 0.0)
    assert relerr(outs[1].float(), ref) < 4e-3
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("M", [640, 8192 + 64])                     # 128-row tiles / 256-row tiles with a ragged last tile
def test_gemm_nt_epilogues(M):
    N, K, rps = 384, 128, 64
    A, B = bf(rnd(M, K, seed=1, scale=0.5)), bf(rnd(N, K, seed=2, scale=0.5))
    bias = rnd(N, seed=3)
    ref = A.float() @ B.float().t()
    # bias + GELU (u, a)
    u, a = gemm_nt(A, B, hip.EPI_BIAS_GELU, torch.bfloat16, bias=bias)
    assert relerr(u.float(), ref + bias) < 4e-3
    assert relerr(a.float(), torch.nn.functional.gelu(ref + bias)) < 5e-3
    # residual with per-sequence DropPath scale
    resid = rnd(M, N, seed=4)
    scale = torch.tensor([1.0, 0.0, 1.25, 1.0, 1.25, 0.0, 1.0, 1.0, 1.0, 1.25], device=DEV).repeat(M // (10 * rps) + 1)[:M // rps].contiguous()
    x, _ = gemm_nt(A, B, hip.EPI_RESID, torch.float32, bias=bias, resid=resid, row_scale=scale, rps=rps)
    want = resid + scale.repeat_interleave(rps)[:, None] * (ref + bias)
    assert relerr(x, want) < 2e-5
    # dgelu
    U = bf(rnd(M, N, seed=5))
    cs = torch.full((N,), 0.25, device=DEV)
    d, _ = gemm_nt(A, B, hip.EPI_DGELU, torch.bfloat16, U=U, colsum=cs)
    uf = U.float().requires_grad_(True)
    torch.nn.functional.gelu(uf).backward(ref)
    assert relerr(d.float(), uf.grad) < 5e-3
    assert relerr(cs, uf.grad.sum(0) + 0.25) < 2e-3                  # fused fc1-bias gradient (column sums of du)
    # patch epilogue: per-token table + mask-token substitution
    table = rnd(rps, N, seed=6)
    flag = (torch.arange(M, device=DEV) % 5 == 0).to(torch.uint8)
    alt = rnd(N, seed=7)
    t, _ = gemm_nt(A, B, hip.EPI_PATCH, torch.float32, bias=bias, table=table, rowflag=flag, alt=alt, rps=rps)
    tab = table.repeat(M // rps, 1)
    want = torch.where(flag.bool()[:, None], tab - bias + alt, ref + tab)
    assert relerr(t, want) < 2e-5


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (512, 768, 768), (1024, 2304, 768), (8192, 768, 3072), (8192 + 256, 3072, 768), (768, 1536, 384)])
def test_gemm_nt_p8_phased_kernel(M, N, K):
    """The 256 x 256 phased kernel (csrc/gemm_p8.h; N % 256 == 0, K % 128 == 0, M % 256 == 0; hook 391 on / 390 off; hook 351 admits it below
    8192 rows): every epilogue it carries against the fp32 formula, and against the kernels it replaces.  Asymmetric operands catch a
    transposed fragment; K = 128 (two k-tiles) is all prologue + tail, K = 3072 runs 22 steady iterations."""
    lib = hip.load()
    A, B = bf(rnd(M, K, seed=1, scale=0.5)), bf(rnd(N, K, seed=2, scale=0.5))
    bias = rnd(N, seed=3)
    ref = A.float() @ B.float().t()
    rps = 64
    resid = rnd(M, N, seed=4)
    scale = torch.tensor([1.0, 0.0, 1.25, 1.0, 1.25, 0.0, 1.0, 1.0, 1.0, 1.25], device=DEV).repeat(M // (10 * rps) + 1)[:M // rps].contiguous()
    U = bf(rnd(M, N, seed=5))
    res = {}
    try:
        lib.atst_tune_gemm_variant(351)
        for hook in (390, 391):
            lib.atst_tune_gemm_variant(hook)
            f32, _ = gemm_nt(A, B, hip.EPI_F32, torch.float32, bias=bias)
            b16, _ = gemm_nt(A, B, hip.EPI_BF16, torch.bfloat16, bias=bias)
            b16nb, _ = gemm_nt(A, B, hip.EPI_BF16, torch.bfloat16)
            u, a = gemm_nt(A, B, hip.EPI_BIAS_GELU, torch.bfloat16, bias=bias)
            x, _ = gemm_nt(A, B, hip.EPI_RESID, torch.float32, bias=bias, resid=resid, row_scale=scale, rps=rps)
            cs = torch.full((N,), 0.25, device=DEV)
            d, _ = gemm_nt(A, B, hip.EPI_DGELU, torch.bfloat16, U=U, colsum=cs)
            res[hook] = (f32, b16, b16nb, u, a, x, d, cs)
    finally:
        lib.atst_tune_gemm_variant(393); lib.atst_tune_gemm_variant(350)
    f32, b16, b16nb, u, a, x, d, cs = res[391]
    assert relerr(f32, ref + bias) < 2e-5
    assert relerr(b16.float(), ref + bias) < 4e-3 and relerr(b16nb.float(), ref) < 4e-3
    assert relerr(u.float(), ref + bias) < 4e-3 and relerr(a.float(), torch.nn.functional.gelu(ref + bias)) < 5e-3
    assert relerr(x, resid + scale.repeat_interleave(rps)[:, None] * (ref + bias)) < 2e-5
    uf = U.float().requires_grad_(True)
    torch.nn.functional.gelu(uf).backward(ref)
    assert relerr(d.float(), uf.grad) < 5e-3 and relerr(cs, uf.grad.sum(0) + 0.25) < 2e-3
    for got, other in zip(res[391], res[390]):                            # the kernels it replaces: same sums up to the fp32 accumulation order
        assert relerr(got.float(), other.float()) < 4e-3


@pytest.mark.parametrize("M,N,K", [(768, 128, 384), (8192, 1152, 384), (16384, 1536, 384), (2048, 384, 1536), (256, 256, 448), (65536 + 256, 128, 384),
                                   (4096, 768, 768)])
def test_gemm_nt_two_team_kernel(M, N, K):
    """The persistent two-team kernel (csrc/gemm_tt.h; hook 2001 on / 2000 off; hook 351 admits it below 8192 rows): the epilogue of tile i is stored by
    one team of four waves while the other team multiplies tile i + 1.  Tile counts of 3 (253 of 256 blocks idle), 24, 96, 257 (one block with two
    rounds, the others one), 288, 768 (three rounds per block: both teams in both roles) ; K = 384 (6 stages of 64),
    448 (seven stages of 64), 768, 1536.  Against the fp32 formulas and against the kernels it replaces."""
    lib = hip.load()
    A, B = bf(rnd(M, K, seed=1, scale=0.5)), bf(rnd(N, K, seed=2, scale=0.5))
    bias = rnd(N, seed=3)
    ref = A.float() @ B.float().t()
    res = {}
    try:
        lib.atst_tune_gemm_variant(351)
        for hook in (2000, 2001, 2002):                                  # 2002: the same overlap as ONE instruction stream (4 waves x 512 registers, two accumulator sets)
            lib.atst_tune_gemm_variant(hook)
            b16, _ = gemm_nt(A, B, hip.EPI_BF16, torch.bfloat16, bias=bias)
            b16nb, _ = gemm_nt(A, B, hip.EPI_BF16, torch.bfloat16)
            u, a = gemm_nt(A, B, hip.EPI_BIAS_GELU, torch.bfloat16, bias=bias)
            _, a2 = gemm_nt(A, B, hip.EPI_BIAS_GELU, torch.bfloat16, bias=bias, no_primary=True)      # teacher / inference: u is not saved
            res[hook] = (b16, b16nb, u, a, a2)
    finally:
        lib.atst_tune_gemm_variant(2000); lib.atst_tune_gemm_variant(350)
    for hook in (2001, 2002):
        b16, b16nb, u, a, a2 = res[hook]
        assert relerr(b16.float(), ref + bias) < 4e-3 and relerr(b16nb.float(), ref) < 4e-3, hook
        assert relerr(u.float(), ref + bias) < 4e-3 and relerr(a.float(), torch.nn.functional.gelu(ref + bias)) < 5e-3, hook
        assert torch.equal(a, a2), hook
        for got, other in zip(res[hook], res[2000]):                      # the kernels it replaces: same sums up to the fp32 accumulation order
            assert relerr(got.float(), other.float()) < 4e-3, hook
        assert float((b16.float() - res[2000][0].float()).abs().max()) <= 0.07 * float(ref.abs().max()), hook      # no misplaced row / column anywhere


@pytest.mark.parametrize("M,N,K,split", [(1000, 256, 384, 0), (64, 128, 128, 0), (4099, 384, 256, 512), (777, 1152, 384, 0),
                                         (8192, 384, 384, 0), (16384 + 64, 1152, 384, 0), (8192 + 128, 384, 1536, 0)])   # last three: 192x384 LDS-DMA tile
def test_gemm_tn(M, N, K, split):
    dY, X = bf(rnd(M, N, seed=1)), bf(rnd(M, K, seed=2))
    dW = torch.full((N, K), 0.5, device=DEV)
    hip.call("atst_gemm_tn_bf16", hip.ptr(dY), hip.ptr(X), M, N, K, N, K, hip.ptr(dW), K, split, hip.stream())
    ref = dY.float().t() @ X.float() + 0.5
    assert relerr(dW, ref) < 2e-5


@pytest.mark.parametrize("hook", [121, 120, 122, 130])    # wgrad schedules: staggered issue (default) / all waves behind the hand-off / 32-row stages in a 4-deep ring ; 130: round-3 block order (no XCD group map)
@pytest.mark.parametrize("M", [8192, 8192 + 192, 32768 + 64, 1000])   # 192x384 LDS-DMA tiles in one launch (whole / ragged last split) / per-problem fallback
def test_gemm_tn_group(M, hook):
    import ctypes as C
    hip.load().atst_tune_gemm_variant(hook)
    shapes = [(1536, 384), (384, 1536), (1152, 384), (384, 384)]
    items = (hip.Wgrad * 4)()
    keep, want = [], []
    for i, (N, K) in enumerate(shapes):
        dY, X = bf(rnd(M, N, seed=10 + i)), bf(rnd(M, K, seed=20 + i))
        dW = torch.full((N, K), 0.25, device=DEV)
        keep.append((dY, X, dW))
        want.append(dY.float().t() @ X.float() + 0.25)
        items[i] = hip.Wgrad(hip.ptr(dY), hip.ptr(X), hip.ptr(dW), M, N, K, N, K, K)
    hip.call("atst_gemm_tn_group_bf16", C.cast(items, C.c_void_p), 4, hip.stream())
    torch.cuda.synchronize()
    hip.load().atst_tune_gemm_variant(121)
    hip.load().atst_tune_gemm_variant(131)
    for (dY, X, dW), ref in zip(keep, want):
        assert relerr(dW, ref) < 2e-5


@pytest.mark.parametrize("C", [384, 768])
def test_layernorm(C):
    M, rps = 517, 11
    x = rnd(M, C, seed=1) * 2 + 0.3
    gamma, beta = 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
    y = torch.empty(M, C, dtype=torch.bfloat16, device=DEV)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    hip.call("atst_layernorm_fwd", hip.ptr(x), hip.ptr(gamma), hip.ptr(beta), hip.ptr(y), hip.ptr(mean), hip.ptr(rstd), M, C, hip.stream())
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xr, (C,), gr, br, 1e-6)
    assert relerr(y.float(), ref) < 4e-3
    assert relerr(mean, x.mean(1)) < 1e-5
    dy = bf(rnd(M, C, seed=4))
    dres = rnd(M, C, seed=5)
    scale = (torch.arange((M + rps - 1) // rps, device=DEV) % 3).float() * 0.5
    ref.backward(dy.float())
    dx = torch.empty(M, C, device=DEV)
    g = torch.empty(M, C, dtype=torch.bfloat16, device=DEV)
    dgamma, dbeta, dbu = (torch.zeros(C, device=DEV) for _ in range(3))
    hip.call("atst_layernorm_bwd", hip.ptr(dy), hip.ptr(x), hip.ptr(mean), hip.ptr(rstd), hip.ptr(gamma), hip.ptr(dres),
             hip.ptr(dx), hip.ptr(g), hip.ptr(scale), rps, hip.ptr(dgamma), hip.ptr(dbeta), hip.ptr(dbu), M, C, hip.stream())
    want_dx = dres + xr.grad
    assert relerr(dx, want_dx) < 2e-5
    assert relerr(dgamma, gr.grad) < 2e-5 and relerr(dbeta, br.grad) < 2e-5
    want_g = want_dx * scale.repeat_interleave(rps)[:M, None]
    assert relerr(g.float(), want_g) < 4e-3
    assert relerr(dbu, want_g.sum(0)) < 2e-3


@pytest.mark.parametrize("M,K,hook,with_up", [(640, 128, None, True),          # 128-row tile, 8 waves
                                              (2048 + 40, 1152, None, True),  # <= 1.5 rounds: 128x384 tile on 4 waves, ragged
                                              (8192 + 64, 1536, 360, True),   # 256-row tile, 8 waves (4-wave auto-selection off)
                                              (8192 + 64, 1152, (360, 398), True),   # ... with the 64-deep whole-line main loop (hook 398, round 6)
                                              (700, 384, None, False)])       # block 0: no upstream operand / bias gradient
def test_gemm_lnbwd_epilogue(M, K, hook, with_up):
    """dgrad GEMM whose epilogue is the LayerNorm backward (EPI_LNBWD) vs autograd of layer_norm on the fp32 product."""
    C, rps = 384, 32
    lib = hip.load()
    dY, Wt = bf(rnd(M, K, seed=1, scale=0.5)), bf(rnd(C, K, seed=2, scale=0.5))
    x = rnd(M, C, seed=3) * 2 + 0.3
    gamma, beta = 1 + 0.1 * rnd(C, seed=4), 0.1 * rnd(C, seed=5)
    mean, var = x.mean(1), x.var(1, unbiased=False)
    rstd = torch.rsqrt(var + 1e-6)
    dres = rnd(M, C, seed=6)
    scale = ((torch.arange((M + rps - 1) // rps, device=DEV) % 3).float() * 0.625).contiguous()
    dx = torch.empty(M, C, device=DEV)
    g = torch.empty(M, C, dtype=torch.bfloat16, device=DEV) if with_up else None
    dgamma, dbeta, dbu = (torch.full((C,), 0.125, device=DEV) for _ in range(3))
    for hk in (() if hook is None else ((hook,) if isinstance(hook, int) else hook)):
        lib.atst_tune_gemm_variant(hk)
    try:
        hip.call("atst_gemm_nt_lnbwd_bf16", hip.ptr(dY), hip.ptr(Wt), M, K, hip.ptr(x), hip.ptr(mean.contiguous()), hip.ptr(rstd.contiguous()),
                 hip.ptr(gamma), hip.ptr(dres), hip.ptr(dx), hip.ptr(g), hip.ptr(scale), rps, hip.ptr(dgamma), hip.ptr(dbeta),
                 hip.ptr(dbu) if with_up else None, hip.stream())
    finally:
        if hook is not None:
            lib.atst_tune_gemm_variant(361); lib.atst_tune_gemm_variant(397)
    dy = dY.float() @ Wt.float().t()
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (C,), gr, br, 1e-6).backward(dy)
    want_dx = dres + xr.grad
    assert relerr(dx, want_dx) < 3e-5
    assert relerr(dgamma, gr.grad + 0.125) < 3e-5 and relerr(dbeta, br.grad + 0.125) < 3e-5
    if with_up:
        want_g = want_dx * scale.repeat_interleave(rps)[:M, None]
        assert relerr(g.float(), want_g) < 4e-3
        assert relerr(dbu, want_g.sum(0) + 0.125) < 3e-5
    else:
        assert float((dbu - 0.125).abs().max()) == 0.0


@pytest.mark.parametrize("M,K,hook", [(640, 128, None), (2048 + 40, 384, None), (8192 + 64, 1536, 360), (8192 + 64, 384, (360, 398))])   # 128-row tile / 4-wave 128x384 / 256-row tile / the same with the 64-deep whole-line main loop
def test_gemm_resid_layernorm_epilogue(M, K, hook):
    """residual GEMM whose epilogue also emits LayerNorm(new row) + its statistics vs the fp32 formulation."""
    C, rps = 384, 32
    lib = hip.load()
    A, B = bf(rnd(M, K, seed=1, scale=0.5)), bf(rnd(C, K, seed=2, scale=0.5))
    bias, resid = rnd(C, seed=3), rnd(M, C, seed=4) * 2 + 0.2
    gamma, beta = 1 + 0.1 * rnd(C, seed=5), 0.1 * rnd(C, seed=6)
    scale = ((torch.arange((M + rps - 1) // rps, device=DEV) % 3).float() * 0.625).contiguous()
    x = torch.empty(M, C, device=DEV)
    h = torch.empty(M, C, dtype=torch.bfloat16, device=DEV)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    for hk in (() if hook is None else ((hook,) if isinstance(hook, int) else hook)):
        lib.atst_tune_gemm_variant(hk)
    try:
        hip.call("atst_gemm_nt_resid_ln_bf16", hip.ptr(A), hip.ptr(B), M, K, hip.ptr(bias), hip.ptr(resid), hip.ptr(scale), rps, hip.ptr(x),
                 hip.ptr(gamma), hip.ptr(beta), hip.ptr(h), hip.ptr(mean), hip.ptr(rstd), hip.stream())
    finally:
        if hook is not None:
            lib.atst_tune_gemm_variant(361); lib.atst_tune_gemm_variant(397)
    want = resid + scale.repeat_interleave(rps)[:M, None] * (A.float() @ B.float().t() + bias)
    assert relerr(x, want) < 2e-5
    assert relerr(mean, want.mean(1)) < 2e-5
    assert relerr(rstd, torch.rsqrt(want.var(1, unbiased=False) + 1e-6)) < 2e-5
    assert relerr(h.float(), torch.nn.functional.layer_norm(want, (C,), gamma, beta, 1e-6)) < 4e-3


def _e4m3(x, scale):
    return (x.float() * scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


def _codes_close(got_u8, want_f8, frac=2e-3):
    """e4m3 bytes of a value that went through a different (but equivalent) fp32 summation order: equal, except that a value sitting on a rounding
    boundary may land on the neighbouring code -- at most `frac` of the elements, and never further than one code apart."""
    g, w = got_u8.view(torch.float8_e4m3fn).float(), want_f8.float()
    diff = g != w
    if float(diff.float().mean()) > frac:
        return False
    gi, wi = got_u8.view(torch.uint8).int(), want_f8.view(torch.uint8).int()
    mag = lambda c: torch.where(c >= 128, -(c - 128), c)                       # sign-magnitude byte -> ordered integer
    return int((mag(gi) - mag(wi)).abs().max()) <= 1


@pytest.mark.parametrize("M,K,both", [(700, 384, True), (8192 + 64, 1536, False), (2048 + 40, 384, False)])
def test_gemm_resid_layernorm_epilogue_fp8(M, K, both):
    """Round 6: the residual GEMM on e4m3 operands whose epilogue is also the LayerNorm of the new row, written as the e4m3 operand of the next GEMM
    (+ its amax and clip count) and, optionally, as bf16 -- against the fp32 formulation on the dequantised operands."""
    C, rps = 384, 32
    A, B = rnd(M, K, seed=1, scale=0.5), rnd(C, K, seed=2, scale=0.5)
    sa, sb = 8.0, 64.0
    A8, B8 = _e4m3(A, sa).view(torch.uint8).contiguous(), _e4m3(B, sb).view(torch.uint8).contiguous()
    dq, asc = torch.tensor([1.0 / sb], device=DEV), torch.tensor([sa], device=DEV)
    bias, resid = rnd(C, seed=3), rnd(M, C, seed=4) * 2 + 0.2
    gamma, beta = 1 + 0.1 * rnd(C, seed=5), 0.1 * rnd(C, seed=6)
    scale = ((torch.arange((M + rps - 1) // rps, device=DEV) % 3).float() * 0.625).contiguous()
    x = torch.empty(M, C, device=DEV)
    h = torch.empty(M, C, dtype=torch.bfloat16, device=DEV) if both else None
    h8 = torch.empty(M, C, dtype=torch.uint8, device=DEV)
    s8 = torch.tensor([96.0], device=DEV)                                       # large enough that a few elements clip at +-448
    site, sat = torch.zeros(hip.AMAX_SITE_STRIDE, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    hip.call("atst_gemm_nt_resid_ln_fp8", hip.ptr(A8), hip.ptr(B8), M, K, hip.ptr(dq), hip.ptr(asc), hip.ptr(bias), hip.ptr(resid), hip.ptr(scale), rps, hip.ptr(x),
             hip.ptr(gamma), hip.ptr(beta), hip.ptr(h), hip.ptr(h8), hip.ptr(s8), hip.ptr(site), hip.ptr(sat), hip.ptr(mean), hip.ptr(rstd), hip.stream())
    acc = (A8.view(torch.float8_e4m3fn).double() @ B8.view(torch.float8_e4m3fn).double().t()).float() / (sa * sb)
    want = resid + scale.repeat_interleave(rps)[:M, None] * (acc + bias)
    assert relerr(x, want) < 2e-5
    assert relerr(mean, want.mean(1)) < 2e-5
    assert relerr(rstd, torch.rsqrt(want.var(1, unbiased=False) + 1e-6)) < 2e-5
    ln = torch.nn.functional.layer_norm(x, (C,), gamma, beta, 1e-6)             # of the kernel's own x: isolates the LayerNorm + quantisation
    lnb = ln.bfloat16()
    if both:
        assert relerr(h.float(), ln) < 4e-3
        lnb = h                                                                # the e4m3 copy is the copy of THESE bf16 values
        assert torch.equal(h8.view(torch.float8_e4m3fn).float(), _e4m3(h, 96.0).float())
    else:
        assert _codes_close(h8, _e4m3(lnb, 96.0), frac=2e-2)                   # bf16 rounding boundaries of LN(x) move a code now and then
    assert abs(float(site.max()) - float(lnb.float().abs().max())) <= 0.02 * float(lnb.float().abs().max())
    nclip = int(((lnb.float() * 96.0).abs() > 448.0).sum())
    assert nclip > 0 and abs(int(sat) - nclip) <= max(2, nclip // 50)


@pytest.mark.parametrize("M,K,f8,g16,hook", [(700, 384, True, True, None), (8192 + 64, 1536, True, False, None), (2048 + 40, 1152, False, False, None),
                                             (8192 + 64, 1152, False, True, 360),      # bf16 operands on the 8-wave 256-row tile (4-wave auto-selection off)
                                             (640, 1152, True, False, None)])
def test_gemm_lnbwd_epilogue_q8(M, K, f8, g16, hook):
    """Round 6: the LayerNorm-backward dgrad epilogue that also writes the e4m3 copy of g and its amax, on e4m3 or bf16 operands."""
    C, rps = 384, 32
    dYf, Wtf = rnd(M, K, seed=1, scale=0.5), rnd(C, K, seed=2, scale=0.5)
    sy, sw = 16.0, 64.0
    if f8:
        dY, Wt = _e4m3(dYf, sy).view(torch.uint8).contiguous(), _e4m3(Wtf, sw).view(torch.uint8).contiguous()
        dy = (dY.view(torch.float8_e4m3fn).double() @ Wt.view(torch.float8_e4m3fn).double().t()).float() / (sy * sw)
    else:
        dY, Wt = bf(dYf), bf(Wtf)
        dy = dY.float() @ Wt.float().t()
    dq, dsc = torch.tensor([1.0 / sw], device=DEV), torch.tensor([sy], device=DEV)
    x = rnd(M, C, seed=3) * 2 + 0.3
    gamma, beta = 1 + 0.1 * rnd(C, seed=4), 0.1 * rnd(C, seed=5)
    mean, var = x.mean(1), x.var(1, unbiased=False)
    rstd = torch.rsqrt(var + 1e-6)
    dres = rnd(M, C, seed=6)
    scale = ((torch.arange((M + rps - 1) // rps, device=DEV) % 3).float() * 0.625).contiguous()
    dx = torch.empty(M, C, device=DEV)
    g = torch.empty(M, C, dtype=torch.bfloat16, device=DEV) if g16 else None
    g8 = torch.empty(M, C, dtype=torch.uint8, device=DEV)
    s8 = torch.tensor([24.0], device=DEV)
    site = torch.zeros(hip.AMAX_SITE_STRIDE, device=DEV)
    dgamma, dbeta, dbu = (torch.full((C,), 0.125, device=DEV) for _ in range(3))
    lib = hip.load()
    if hook is not None:
        lib.atst_tune_gemm_variant(hook)
    try:
        hip.call("atst_gemm_nt_lnbwd_q8", hip.ptr(dY), hip.ptr(Wt), 1 if f8 else 0, M, K, hip.ptr(dq), hip.ptr(dsc), hip.ptr(x), hip.ptr(mean.contiguous()),
                 hip.ptr(rstd.contiguous()), hip.ptr(gamma), hip.ptr(dres), hip.ptr(dx), hip.ptr(g), hip.ptr(g8), hip.ptr(s8), hip.ptr(site), hip.ptr(scale), rps,
                 hip.ptr(dgamma), hip.ptr(dbeta), hip.ptr(dbu), hip.stream())
    finally:
        if hook is not None:
            lib.atst_tune_gemm_variant(361)
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (C,), gr, br, 1e-6).backward(dy)
    want_dx = dres + xr.grad
    assert relerr(dx, want_dx) < 3e-5
    assert relerr(dgamma, gr.grad + 0.125) < 3e-5 and relerr(dbeta, br.grad + 0.125) < 3e-5
    gs = dx * scale.repeat_interleave(rps)[:M, None]                            # of the kernel's own dx
    assert relerr(dbu, gs.sum(0) + 0.125) < 3e-5
    if g16:
        assert torch.equal(g.float(), gs.bfloat16().float())
    assert torch.equal(g8.view(torch.float8_e4m3fn).float(), _e4m3(gs.bfloat16(), 24.0).float())
    assert float(site.max()) == float(gs.abs().max())


def attn_ref(qkv, valid, S, H, NP):
    C = H * 64
    q, k, v = qkv.float().reshape(S, NP, 3, H, 64).permute(2, 0, 3, 1, 4)
    att = (q @ k.transpose(-2, -1)) * 0.125
    mask = (torch.arange(NP, device=qkv.device)[None, :] >= valid[:, None]).float() * -10000.0
    att = (att + mask[:, None, None, :]).softmax(-1)
    return (att @ v).transpose(1, 2).reshape(S * NP, C)


@pytest.mark.parametrize("NP,valid", [(256, [251, 100, 33]), (256, [256, 1, 32, 224, 225, 2]), (32, [26, 26, 20, 1, 7]), (64, [64, 40, 3]), (128, [128, 97])])
def test_attention(NP, valid):
    S, H = len(valid), 6
    C = H * 64
    qkv = bf(rnd(S * NP, 3 * C, seed=1))
    vt = torch.tensor(valid, dtype=torch.int32, device=DEV)
    o = torch.empty(S * NP, C, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(S, H, NP, device=DEV)
    hip.call("atst_attention_fwd", hip.ptr(qkv), hip.ptr(vt), hip.ptr(o), hip.ptr(lse), S, H, NP, hip.stream())
    qr = qkv.float().requires_grad_(True)
    ref = attn_ref(qr, vt, S, H, NP)
    assert relerr(o.float(), ref) < 6e-3
    # backward: upstream gradient is zero on rows that are not valid tokens (as in the encoder)
    rowvalid = (torch.arange(NP, device=DEV)[None, :] < vt[:, None]).reshape(-1, 1).float()
    d_o = bf(rnd(S * NP, C, seed=2) * rowvalid)
    ref.backward(d_o.float())
    for scratch in (None, torch.empty(S, H, NP, device=DEV)):          # two-kernel path / merged per-sequence kernel (NP = 256)
        dqkv = torch.full_like(qkv, float("nan"))
        hip.call("atst_attention_bwd", hip.ptr(qkv), hip.ptr(vt), hip.ptr(o), hip.ptr(lse), hip.ptr(d_o), hip.ptr(dqkv), hip.ptr(scratch),
                 S, H, NP, hip.stream())
        got, want = dqkv.float().reshape(S * NP, 3, C), qr.grad.reshape(S * NP, 3, C)
        for i, name in enumerate("qkv"):
            assert relerr(got[:, i], want[:, i]) < 1.5e-2, (name, scratch is not None)
        # keys beyond `valid` receive exactly zero gradient
        inval = (rowvalid == 0).reshape(-1)
        assert float(got[inval][:, 1:].abs().max()) == 0.0 if inval.any() else True
    if NP in (256, 32):                                                 # (NP = 32, round 6: the 1 s local views take part in the e4m3 step)
        # fp8 forward: the e4m3 copy of the output written by the kernel itself, next to the bf16 output (training) or instead of it (inference):
        # the codes of the SAME bf16 values, their max |.| in the amax site, the clipped elements counted
        o_amax = float(o.float().abs().max())
        for sc, clips in ((torch.tensor([448.0 / (1.5 * o_amax)], device=DEV), False), (torch.tensor([448.0 / (0.25 * o_amax)], device=DEV), True)):
            want8 = (o.float() * sc).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
            n_clip = int(((o.float() * sc).abs() > 448.0).sum())
            assert (n_clip > 0) == clips
            for with_o in (True, False):
                o2 = torch.full_like(o, float("nan")) if with_o else None
                o8 = torch.full((S * NP, C), 0x7F, dtype=torch.uint8, device=DEV)
                site, sat, lse2 = torch.zeros(hip.AMAX_SITE_STRIDE, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), torch.empty_like(lse)
                hip.call("atst_attention_fwd_fp8", hip.ptr(qkv), hip.ptr(vt), hip.ptr(o2), hip.ptr(o8), hip.ptr(sc), hip.ptr(site), hip.ptr(sat), hip.ptr(lse2),
                         S, H, NP, hip.stream())
                assert torch.equal(o8.view(torch.float8_e4m3fn).float(), want8.float()) and torch.equal(lse2, lse)
                assert (o2 is None or torch.equal(o2, o)) and float(site.max()) == o_amax and int(sat) == n_clip
        # the e4m3-only output of the merged kernel (fp8 qkv gradient path): the SAME bf16 values times the scale, as e4m3 codes -- bit for bit -- and
        # their max |.| in the amax site; any other NP is refused
        amax_true = float(dqkv.float().abs().max())
        scale = torch.tensor([448.0 / (1.5 * amax_true)], device=DEV)              # margin 1.5: nothing clips ; a second scale that does clip
        for sc in (scale, scale * 4.0):
            d8 = torch.full((S * NP, 3 * C), 0x7F, dtype=torch.uint8, device=DEV)
            site = torch.zeros(hip.AMAX_SITE_STRIDE, device=DEV)
            hip.call("atst_attention_bwd_fp8", hip.ptr(qkv), hip.ptr(vt), hip.ptr(o), hip.ptr(lse), hip.ptr(d_o), hip.ptr(d8), hip.ptr(sc), hip.ptr(site),
                     hip.ptr(scratch), S, H, NP, hip.stream())
            want8 = (dqkv.float() * sc).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
            # -0 and +0 are distinct codes: compare the decoded values, and the codes wherever the value is not zero
            assert torch.equal(d8.view(torch.float8_e4m3fn).float(), want8.view(torch.float8_e4m3fn).float())
            assert float(site.max()) == amax_true
    else:
        rc = hip.load().atst_attention_bwd_fp8(hip.ptr(qkv), hip.ptr(vt), hip.ptr(o), hip.ptr(lse), hip.ptr(d_o), hip.ptr(qkv), hip.ptr(lse), hip.ptr(lse),
                                               hip.ptr(scratch), S, H, NP, hip.stream())
        assert rc != 0
    if NP == 32:                                                        # fused one-wave-per-pair backward (default, hook 409) against the two-kernel path (408)
        try:
            hip.load().atst_tune_gemm_variant(408)
            two = torch.full_like(qkv, float("nan"))
            hip.call("atst_attention_bwd", hip.ptr(qkv), hip.ptr(vt), hip.ptr(o), hip.ptr(lse), hip.ptr(d_o), hip.ptr(two), None, S, H, NP, hip.stream())
        finally:
            hip.load().atst_tune_gemm_variant(409)
        assert relerr(dqkv.float(), two.float()) < 2e-3                 # same math, D summed in a different order


def test_patchify_bit_exact():
    S, width, NP = 3, 1001, 256
    mel = ((torch.arange(S)[:, None, None, None] * 7 + torch.arange(64)[None, None, :, None] * 3
            + torch.arange(width)[None, None, None, :]) % 251).float()
    want = O.patchify(mel)                                            # [S,250,256]
    out = torch.empty(S * NP, 256, dtype=torch.bfloat16, device=DEV)
    hip.call("atst_patchify_bf16", hip.ptr(mel.to(DEV)), S, width, NP, 1, hip.ptr(out), hip.stream())
    got = out.float().cpu().reshape(S, NP, 256)
    assert torch.equal(got[:, 1:251], want) and float(got[:, 0].abs().max()) == 0 and float(got[:, 251:].abs().max()) == 0
    hip.call("atst_patchify_bf16", hip.ptr(mel.to(DEV)), S, width, NP, 0, hip.ptr(out), hip.stream())
    got = out.float().cpu().reshape(S, NP, 256)
    assert torch.equal(got[:, :250], want) and float(got[:, 250:].abs().max()) == 0
    # short local view: 101 frames -> 25 patches, NP = 32
    mel2 = mel[:, :, :, :101].contiguous()
    out2 = torch.empty(S * 32, 256, dtype=torch.bfloat16, device=DEV)
    hip.call("atst_patchify_bf16", hip.ptr(mel2.to(DEV)), S, 101, 32, 1, hip.ptr(out2), hip.stream())
    got2 = out2.float().cpu().reshape(S, 32, 256)
    assert torch.equal(got2[:, 1:26], O.patchify(mel2)) and float(got2[:, 26:].abs().max()) == 0


def test_rows_colsum_transpose():
    M, Cc = 700, 384
    src = bf(rnd(M, Cc, seed=1))
    rows = torch.tensor([0, 5, 699, 256, 3], dtype=torch.int32, device=DEV)
    dst = torch.empty(5, Cc, device=DEV)
    hip.call("atst_gather_rows_bf16", hip.ptr(src), hip.ptr(rows), 5, Cc, hip.ptr(dst), hip.stream())
    assert torch.equal(dst, src.float()[rows.long()])
    back = torch.zeros(M, Cc, dtype=torch.bfloat16, device=DEV)
    hip.call("atst_scatter_rows_bf16", hip.ptr(dst), hip.ptr(rows), 5, Cc, hip.ptr(back), hip.stream())
    want = torch.zeros(M, Cc, device=DEV); want[rows.long()] = dst
    assert torch.equal(back.float(), want)
    cs = torch.zeros(Cc, device=DEV)
    hip.call("atst_colsum_bf16_f32", hip.ptr(src), M, Cc, Cc, hip.ptr(cs), hip.stream())
    assert relerr(cs, src.float().sum(0)) < 1e-5
    t = torch.empty(Cc, M, dtype=torch.bfloat16, device=DEV)
    hip.call("atst_transpose_bf16_2d", hip.ptr(src), M, Cc, hip.ptr(t), hip.stream())
    assert torch.equal(t, src.t().contiguous())


def test_bn_finish_matches_torch_batchnorm():
    """atst_bn_finish_f32 = what nn.BatchNorm1d(train) does with the batch statistics besides normalising (rstd, running_mean / running_var with
    the unbiased variance, num_batches_tracked), with the row count as a host float and as a device scalar (cross-rank count)."""
    R, N = 300, 4096
    h = rnd(R, N, seed=1) * 2 + 0.5
    bn = torch.nn.BatchNorm1d(N).to(DEV).train()
    with torch.no_grad():
        bn.running_mean.copy_(rnd(N, seed=2)); bn.running_var.copy_(rnd(N, seed=3).abs() + 0.5)
    rm, rv, nb = bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()
    bn(h)
    mean, m2 = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    scratch = torch.empty(32 * N, device=DEV)
    hip.call("atst_bn_stats_f32", hip.ptr(h), R, N, hip.ptr(mean), hip.ptr(m2), hip.ptr(scratch), hip.stream())
    for count_dev in (None, torch.tensor(float(R), device=DEV)):
        rm2, rv2, nb2, rstd = rm.clone(), rv.clone(), nb.clone(), torch.empty(N, device=DEV)
        hip.call("atst_bn_finish_f32", hip.ptr(mean), hip.ptr(m2), float(R) if count_dev is None else 0.0, hip.ptr(count_dev), 0.1, 1e-5,
                 hip.ptr(rm2), hip.ptr(rv2), hip.ptr(nb2), hip.ptr(rstd), N, hip.stream())
        assert relerr(rstd, torch.rsqrt(h.var(0, unbiased=False) + 1e-5)) < 1e-6
        assert relerr(rm2, bn.running_mean) < 1e-6 and relerr(rv2, bn.running_var) < 1e-6
        assert int(nb2) == int(bn.num_batches_tracked) == int(nb) + 1
    # statistics only (inference-style use): running buffers untouched
    rstd = torch.empty(N, device=DEV)
    hip.call("atst_bn_finish_f32", hip.ptr(mean), hip.ptr(m2), float(R), None, 0.1, 1e-5, None, None, None, hip.ptr(rstd), N, hip.stream())
    assert relerr(rstd, torch.rsqrt(h.var(0, unbiased=False) + 1e-5)) < 1e-6


def test_bn_relu_head():
    R, N = 300, 4096
    h = rnd(R, N, seed=1) * 2 + 0.5
    gamma, beta = 1 + 0.1 * rnd(N, seed=2), 0.1 * rnd(N, seed=3)
    mean, m2 = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    scratch = torch.empty(32 * N, device=DEV)
    hip.call("atst_bn_stats_f32", hip.ptr(h), R, N, hip.ptr(mean), hip.ptr(m2), hip.ptr(scratch), hip.stream())
    assert relerr(mean, h.mean(0)) < 1e-5 and relerr(m2 / R, h.var(0, unbiased=False)) < 1e-5
    rstd = torch.rsqrt(m2 / R + 1e-5)
    y = torch.empty(R, N, dtype=torch.bfloat16, device=DEV)
    hip.call("atst_bn_apply_relu_bf16", hip.ptr(h), hip.ptr(mean), hip.ptr(rstd), hip.ptr(gamma), hip.ptr(beta), R, N, hip.ptr(y), hip.stream())
    hr, gr, br = h.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ref = torch.relu(torch.nn.functional.batch_norm(hr, None, None, gr, br, True, 0.1, 1e-5))
    assert relerr(y.float(), ref) < 4e-3
    dy = rnd(R, N, seed=4)
    ref.backward(dy)
    s1, s2 = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    scratch2 = torch.empty(2 * 32 * N, device=DEV)
    hip.call("atst_bn_relu_bwd_sums", hip.ptr(dy), hip.ptr(h), hip.ptr(mean), hip.ptr(rstd), hip.ptr(gamma), hip.ptr(beta), R, N,
             hip.ptr(s1), hip.ptr(s2), hip.ptr(scratch2), hip.stream())
    assert relerr(s1, br.grad) < 1e-4 and relerr(s2, gr.grad) < 1e-4
    dh = torch.empty(R, N, dtype=torch.bfloat16, device=DEV)
    hip.call("atst_bn_bwd_dx_bf16", hip.ptr(dy), hip.ptr(h), hip.ptr(mean), hip.ptr(rstd), hip.ptr(gamma), hip.ptr(beta),
             hip.ptr(s1), hip.ptr(s2), 1.0 / R, R, N, hip.ptr(dh), hip.stream())
    assert relerr(dh.float(), hr.grad) < 4e-3


@pytest.mark.parametrize("B,ncrops", [(2, 2), (7, 6), (64, 2)])
def test_byol_loss(B, ncrops):
    s = rnd(ncrops * B, 256, seed=1)
    t = rnd(2 * B, 256, seed=2)
    acc = torch.empty(1, device=DEV)
    ds = torch.empty_like(s)
    stats = torch.empty(4, 256, device=DEV)
    hip.call("atst_byol_loss_f32", hip.ptr(s), hip.ptr(t), B, ncrops, 256, hip.ptr(acc), hip.ptr(ds), hip.ptr(stats), hip.stream())
    sc = s.cpu().clone().requires_grad_(True)
    loss, std_s, std_t = O.byol_loss(sc, t.cpu(), ncrops)
    loss.backward()
    got = 2.0 - 2.0 * acc.item() / ((2 * ncrops - 2) * B)
    assert abs(got - loss.item()) < 1e-5
    assert relerr(ds, sc.grad) < 1e-5

    def std_from(sums, sq, n):
        var = sq / (n - 1) - sums ** 2 / (n * (n - 1))
        return torch.sqrt(var + 1e-6).mean().item()
    assert abs(std_from(stats[0], stats[1], ncrops * B) - std_s.item()) < 1e-5
    assert abs(std_from(stats[2], stats[3], 2 * B) - std_t.item()) < 1e-5


def test_adamw_ema_vs_oracle():
    n, nt = 256 * 40, 256 * 24
    p, g = rnd(n, seed=1), rnd(n, seed=2) * 0.1
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    t = rnd(nt, seed=3)
    flags = torch.zeros(n // 256, dtype=torch.uint8, device=DEV)
    flags[:10] = 1 | 2 | 4        # decay + update + ema
    flags[10:20] = 2 | 4          # no decay
    flags[20:24] = 4              # frozen (grad None in the reference) but still EMA'd
    flags[24:] = 1 | 2            # student-only (predictor)
    p16 = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    t16 = torch.empty(nt, dtype=torch.bfloat16, device=DEV)
    P, M_, V_, T = p.cpu().clone(), m.cpu().clone(), v.cpu().clone(), t.cpu().clone()
    lr, wd, ema = 3e-4, 0.05, 0.99
    for step in (1, 2, 3):
        ss = lr * math.sqrt(1 - 0.999 ** step) / (1 - 0.9 ** step)
        hip.call("atst_adamw_ema_step", hip.ptr(p), hip.ptr(g), hip.ptr(m), hip.ptr(v), hip.ptr(t), hip.ptr(p16), hip.ptr(t16),
                 hip.ptr(flags), n, nt, lr, wd, 0.9, 0.999, 1e-6, ss, ema, 1.0, hip.stream())
        G = g.cpu()
        for lo, hi_, decay, upd in ((0, 2560, True, True), (2560, 5120, False, True), (5120, 6144, False, False), (6144, n, True, True)):
            if upd:
                O.hf_adamw_step(P[lo:hi_], G[lo:hi_], M_[lo:hi_], V_[lo:hi_], step, lr, wd if decay else 0.0)
        T.mul_(ema).add_((1 - ema) * P[:nt])
    assert relerr(p, P) < 1e-6 and relerr(t, T) < 1e-6 and relerr(m, M_) < 1e-6 and relerr(v, V_) < 1e-6
    assert torch.equal(p16, p.to(torch.bfloat16)) and torch.equal(t16, t.to(torch.bfloat16))


# ---- fp8 (OCP e4m3) forward GEMMs: BASELINE.json configs[4] -------------------------------------------------------------
def _q8_ref(x, scale):
    return (x.float() * scale).clamp(-448, 448).to(torch.float8_e4m3fn).float()


@pytest.mark.parametrize("M,N,K", [(512, 768, 768), (300, 384, 3072), (256, 2304, 768)])
def test_gemm_fp8_vs_e4m3_emulation(M, N, K):
    """Quantisation kernels bit-exact against torch's e4m3 conversion; the MX-scaled MFMA GEMM against an fp32 matmul of the
    SAME e4m3 values (only the summation order differs): 5e-5."""
    g = torch.Generator().manual_seed(M + N)
    A = (torch.randn(M, K, generator=g) * 1.5).to(DEV).bfloat16()
    n_pad = (N * K + 255) // 256 * 256
    flat = torch.zeros(2 * n_pad, device=DEV)
    W0 = (torch.randn(N, K, generator=g) * 0.02).to(DEV); W1 = (torch.randn(N, K, generator=g) * 0.3).to(DEV)
    flat[:N * K] = W0.reshape(-1); flat[n_pad:n_pad + N * K] = W1.reshape(-1)
    table = torch.tensor([[0, N * K], [n_pad, N * K]], dtype=torch.int32, device=DEV)
    p8 = torch.zeros(2 * n_pad, dtype=torch.uint8, device=DEV); dq = torch.zeros(2, device=DEV); amax = torch.zeros(2, device=DEV)
    hip.call("atst_quant_weights_fp8", hip.ptr(flat), hip.ptr(table), 2, hip.ptr(p8), hip.ptr(dq), hip.ptr(amax), hip.stream())
    A8 = torch.empty(M, K, dtype=torch.uint8, device=DEV)
    hip.call("atst_quant_fp8_bf16", hip.ptr(A), M * K, 8.0, hip.ptr(A8), hip.stream())
    assert torch.equal(A8.view(torch.float8_e4m3fn).float(), _q8_ref(A, 8.0))                        # bit-exact quantisation
    for t, W in enumerate((W0, W1)):
        s = 448.0 / W.abs().max()
        w8 = p8[t * n_pad:t * n_pad + N * K].view(N, K)
        wq = w8.view(torch.float8_e4m3fn).float()
        # the device computes 448 / amax with its own division: an ulp of difference in the scale moves values sitting on an
        # e4m3 rounding tie by one code -> allow < 0.1 % of the elements to differ, each by one step (<= 1/8 relative)
        mism = wq != _q8_ref(W, s)
        assert float(mism.float().mean()) < 1e-3 and relerr(wq, _q8_ref(W, s)) < 2e-3 and abs(float(dq[t]) * float(s) - 1) < 1e-6
        bias = torch.randn(N, device=DEV)
        out = torch.empty(M, N, device=DEV)
        hip.call("atst_gemm_nt_fp8", hip.ptr(A8), hip.ptr(w8.contiguous()), M, N, K, K, K, hip.EPI_F32, hip.ptr(out), N, None, hip.ptr(bias), None, None, 1,
                 hip.ptr(dq[t:t + 1]), 1.0 / 8.0, hip.stream())
        ref = (_q8_ref(A, 8.0).double() @ wq.double().t()).float() / (8.0 * s) + bias
        assert relerr(out, ref) < 5e-5, relerr(out, ref)                                              # fp32 accumulation order over K (measured 1.5e-5 at K = 3072)
        assert relerr(out, A.float() @ W.t() + bias) < 6e-2                                           # e4m3: 3 mantissa bits per operand


def test_fp8_encoder_forward_and_step_base():
    """ATST-base geometry, fp8 forward: CLS features against the oracle's fp8 emulation (same rounding points) and against the
    fp32 oracle (the stated cost of e4m3 operands: 7 % after two blocks), then a full training step."""
    from audiossl_amd.engine import AtstEngine
    from oracle import atst_oracle as O
    depth, S = 2, 6
    W = O.recipe_weights("base", depth=depth, seed=7)
    eng = AtstEngine("base", depth=depth, drop_path_rate=0.0, fp8=True)
    eng.load_weights(W)
    mel = O.recipe_mel(S, 1001, seed=9); length = torch.tensor([1001, 900, 1001, 640, 1001, 333])
    ep = eng._pass("student", S, 1001, True, 0)
    cls = ep.forward(mel.to(DEV), eng._valid(length, 1), None, None).float().view(S, 256, 768)[:, 0].cpu()
    with torch.no_grad():
        ref32 = O.encoder_forward(W, "student.encoder.", mel, length, "base", depth=depth, drop_path_rate=0.0)
        with O.emulate_bf16(), O.emulate_fp8():
            ref8 = O.encoder_forward(W, "student.encoder.", mel, length, "base", depth=depth, drop_path_rate=0.0)
    e8, e32 = relerr(cls, ref8), relerr(cls, ref32)
    print(f"\\n[fp8 base depth {depth}] CLS rel-L2 vs fp8-emulating oracle {e8:.3e}, vs fp32 oracle {e32:.3e}")
    # measured 3.6e-2 / 7.3e-2 (x1.5).  e4m3 quantisation is a coarse staircase (steps of 6-12 %): a 2e-3 difference between two
    # bf16 realisations of a GEMM input moves ~2 % of its elements to the neighbouring code, i.e. perturbs the operand by ~1.3 %
    # per GEMM -- the GEMM itself is exact given identical bytes (test_gemm_fp8_vs_e4m3_emulation: 1.5e-5).
    assert e8 < 5.5e-2 and e32 < 1.1e-1, (e8, e32)
    mels = [O.recipe_mel(4, 1001, seed=1).to(DEV), O.recipe_mel(4, 1001, seed=2).to(DEV)]
    lens = [torch.full((4,), 1001)] * 2
    ref = AtstEngine("base", depth=depth, drop_path_rate=0.0)
    ref.load_weights(W)
    l16 = float(ref.forward(mels, lens)[0]); l8 = float(eng.forward(mels, lens)[0])
    eng.backward(); eng.optimizer_step(1e-3, 0.04, 0.99)
    assert abs(l8 - l16) < 5e-2 and torch.isfinite(eng.g32).all() and torch.isfinite(eng.p32).all()
    assert float(eng.dq_s.min()) > 0 and not torch.equal(eng.p8[:1 << 20], torch.zeros(1 << 20, dtype=torch.uint8, device=DEV))


def test_fp8_dynamic_quantiser_and_scale_update():
    """Gradient-operand quantiser of the fp8 dgrad path: y = e4m3(clamp(x * scale)), amax recorded by atomicMax, scale update."""
    n = 8 * 4099
    x = bf(rnd(n, scale=3e-4, seed=3))
    scale = torch.tensor([448.0 / (2.0 * 1.2e-3)], device=DEV)
    amax = torch.zeros(hip.AMAX_SITE_STRIDE, device=DEV)                 # one amax SITE: 16 slots, 256 B apart (include/atst_hip.h)
    y = torch.empty(n, dtype=torch.uint8, device=DEV)
    hip.call("atst_quant_fp8_dyn_bf16", hip.ptr(x), n, hip.ptr(scale), hip.ptr(y), hip.ptr(amax), hip.stream())
    assert float(amax.max()) == float(x.float().abs().max())
    assert int((amax.view(hip.AMAX_SLOTS, hip.AMAX_SLOT_STRIDE)[:, 1:] != 0).sum()) == 0 and int((amax != 0).sum()) > 1   # spread over the slots, nothing between them
    want = torch.clamp(x.float() * scale, -448, 448).to(torch.float8_e4m3fn)
    assert torch.equal(y.view(torch.float8_e4m3fn).float(), want.float())
    # record-only mode leaves no output and still tracks amax; the update turns amax into the next scale and clears it
    sites = torch.zeros(2, hip.AMAX_SITE_STRIDE, device=DEV); sc2 = torch.ones(2, device=DEV)
    hip.call("atst_quant_fp8_dyn_bf16", hip.ptr(x), n, None, None, hip.ptr(sites), hip.stream())
    amax2 = sites.amax(dim=-1).contiguous()                             # the reduced value of every site is what the scale update consumes
    hip.call("atst_fp8_update_scales", hip.ptr(amax2), hip.ptr(sc2), 2, 2.0, hip.stream())
    assert abs(float(sc2[0]) - 448.0 / (2.0 * float(x.float().abs().max()))) < 1e-3 * float(sc2[0])
    assert float(sc2[1]) == 1.0 and float(amax2.abs().max()) == 0.0          # nothing observed at site 1: scale unchanged


def _act_scales(eng):
    """{weight key: running activation scale of that Linear's input} for both networks, as the NEXT forward of `eng` will use them."""
    names = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")
    sc = eng.f8a_scale.cpu()
    return {f"{net}.encoder.blocks.{i}.{nm}": float(sc[k, 4 * i + j]) for k, net in enumerate(("student", "teacher")) for i in range(eng.depth)
            for j, nm in enumerate(names)}


@pytest.mark.parametrize("arch", ["base", "small"])
def test_fp8_dgrad_step_base(arch):
    """(arch = "small", round 6: the same scheme at d = 384, where the LayerNorm forward / backward of the e4m3 step run inside the GEMM epilogues -- parts 1-3.)
    BASELINE.json configs[4]: ATST-base with e4m3 forward AND e4m3 dgrad / weight-gradient GEMMs of all four Linears of a block (round 5: the
    qkv pair reads the e4m3 dqkv the NP = 256 attention backward writes).  Delayed scaling: the first backward records the amax of every gradient operand and runs in bf16, every later one
    quantises with the previous step's scale.  Checked against the ORACLE's emulation of the same scheme (oracle.emulate_fp8_dgrad:
    e4m3 rounding of the bf16 gradient operand with the delayed scale, e4m3 copy of the bf16 weight shadow), with the HIP run's ReLU
    gates injected as in tests/test_step_gpu.py:
      1. recording step: HIP's next-step scales = 448 / (2 amax) agree with the oracle's at all 4 x depth sites;
      2. fp8-dgrad step: per-tensor gradients HIP vs oracle (the oracle quantises on HIP's grid: the recorded scales are injected);
      3. the fp8-dgrad gradients stay within the e4m3 staircase of the bf16-dgrad gradients of the same engine state."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from parity_helpers import oracle_grads
    from audiossl_amd.engine import AtstEngine
    from oracle import atst_oracle as O
    depth, B = 2, 8
    W = O.recipe_weights(arch, depth=depth, seed=7)
    mels_c = [O.recipe_mel(B, 1001, seed=1), O.recipe_mel(B, 1001, seed=2)]
    mels = [m.to(DEV) for m in mels_c]
    lens = [torch.full((B,), 1001)] * 2
    eng = AtstEngine(arch, depth=depth, drop_path_rate=0.0, fp8=True)
    eng.load_weights(W)
    assert eng.fp8_bwd_state == 1 and eng.fp8_qkv_state == 1 and eng.fp8_wgrad_mode() == 3
    eng.forward(mels, lens)
    gates = {f"student.{w}.": (eng.heads[f"student.{w}"].saved[4][:, :4096].float() > 0).cpu() for w in ("projector", "predictor")}
    eng.backward()                                                # step 1: bf16 dgrad, amax recorded
    g_first = eng.g32.clone()
    sc = eng.g8_scale.view(depth, 4).clone()
    act2, act2_dev = _act_scales(eng), eng.f8a_scale.clone()      # forward activation scales of step 2 (running amax of step 1)
    assert all(v > 1.0 for v in act2.values()) and any(abs(v - 8.0) > 1e-3 for v in act2.values())
    assert eng.fp8_bwd_state == 2 and float(sc.min()) > 1.0 and float(eng.g8_amax.abs().max()) == 0.0   # sites g, du, g2, dqkv
    assert eng.fp8_qkv_state == 2 and eng.fp8_wgrad_mode() == 2
    fwd = lambda Wl: O.atst_forward(Wl, mels_c, lens, arch, 2, depth=depth, drop_path_rate=0.0)
    rec = O.emulate_fp8_dgrad(None, qkv=True)
    _, o_first = oracle_grads(W, fwd, True, gates, ctxs=(O.emulate_fp8(), rec))
    site = {0: "mlp.fc2.weight", 1: "mlp.fc1.weight", 2: "attn.proj.weight", 3: "attn.qkv.weight"}
    nxt, inject = rec.next_scales(), {}
    for i in range(depth):
        for k, nm in site.items():
            key = f"student.encoder.blocks.{i}.{nm}"
            ratio = float(sc[i, k]) / nxt[key]
            print(f"  scale site block {i} {nm}: HIP {float(sc[i, k]):.4e} oracle {nxt[key]:.4e} ratio {ratio:.4f}")
            assert abs(ratio - 1.0) < 0.1, (key, ratio)           # an amax (one element decides): measured within 3 %
            inject[key] = float(sc[i, k])
    eng.forward(mels, lens)                                       # same weights, same inputs: now e4m3 dgrad operands (and the adapted forward grid)
    gates2 = {f"student.{w}.": (eng.heads[f"student.{w}"].saved[4][:, :4096].float() > 0).cpu() for w in ("projector", "predictor")}
    eng.backward()
    g_fp8 = eng.g32.clone()
    assert torch.isfinite(g_fp8).all()
    _, o_fp8 = oracle_grads(W, fwd, True, gates2, ctxs=(O.emulate_fp8(act_scales=act2), O.emulate_fp8_dgrad(inject, wgrad=eng.fp8_wgrad, qkv=True)))   # e4m3 weight gradients emulated too
    # the same forward once more (activation scales put back to what step 2 used: bit-identical forward, same gates) with the dgrad on bf16
    # operands (recording mode): isolates what the e4m3 gradient operands change
    eng.f8a_scale.copy_(act2_dev); eng.fp8_bwd_state = 1
    eng.forward(mels, lens); eng.backward()
    g_bf = eng.g32.clone()
    _, o_bf = oracle_grads(W, fwd, True, gates2, ctxs=(O.emulate_fp8(act_scales=act2), O.emulate_fp8_dgrad(None, qkv=True)))

    def table(get_a, get_b):
        worst, num, den = ("", 0.0), 0.0, 0.0
        for name, (off, shape) in eng.layout.entries.items():
            n = math.prod(shape)
            a, b = get_a(name, off, n), get_b(name, off, n)
            if b is None or float(b.norm()) == 0.0 or name in ("encoder.pos_embed", "encoder.norm.bias"):
                continue
            r = relerr(a, b)
            num += r * n; den += n
            if r > worst[1]:
                worst = (name, r)
        return num / den, worst
    hip_of = lambda g: (lambda name, off, n: g[off:off + n].cpu())
    or_of = lambda o: (lambda name, off, n: o[name].reshape(-1) if name in o else None)
    m1, w1 = table(hip_of(g_first), or_of(o_first))
    m2, w2 = table(hip_of(g_fp8), or_of(o_fp8))
    m3, w3 = table(hip_of(g_fp8), hip_of(g_bf))
    mo, wo = table(lambda name, off, n: o_fp8[name].reshape(-1) if name in o_fp8 else torch.zeros(n), or_of(o_bf))
    print(f"\n[fp8 {arch} depth {depth}] HIP vs oracle, bf16 dgrad (fp8 forward): mean {m1:.3e} worst {w1[0]} {w1[1]:.3e}")
    print(f"[fp8 {arch} depth {depth}] HIP vs oracle, e4m3 dgrad:               mean {m2:.3e} worst {w2[0]} {w2[1]:.3e}")
    print(f"[fp8 {arch} depth {depth}] HIP e4m3 dgrad vs HIP bf16 dgrad (same fwd): mean {m3:.3e} worst {w3[0]} {w3[1]:.3e}   (oracle's own: mean {mo:.3e} worst {wo[1]:.3e})")
    # e4m3 is a 6-12 % staircase: a 2e-3 difference between two realisations of an operand moves ~2 % of its elements to the neighbouring code
    # (forward: test_fp8_encoder_forward_and_step_base measures 3.6e-2 on the features), and the gradient inherits the forward's difference
    assert m1 < 9e-2 and m2 < 9e-2 and w2[1] < 0.2, (m1, m2, w2)
    assert m2 < 1.5 * m1 + 2e-2                                   # quantising the gradient operands adds little on top of the fp8-forward gap
    assert m3 < 8e-2 and w3[1] < 0.2
    assert abs(m3 - mo) < 0.6 * max(m3, mo)                       # HIP moves by about as much as the oracle predicts when the dgrad goes e4m3
    # predictor / projector weight gradients do not pass through any encoder dgrad GEMM: unchanged up to atomics order
    off, shape = eng.layout.entries["predictor.3.weight"]
    assert relerr(g_fp8[off:off + math.prod(shape)], g_bf[off:off + math.prod(shape)]) < 1e-5
    if arch == "small":
        return
    # e4m3 WEIGHT gradients (csrc/gemm_tn8.hip, all four Linears of every block) + the e4m3 qkv dgrad against the same step with bf16 weight gradients and
    # a bf16 qkv gradient path (e4m3 fc2 / fc1 / proj dgrad in both): the operands are 2^-4-relative copies, the sums run over M = 4096 rows -- a few per
    # cent per tensor, and what the oracle's emulation predicts
    assert eng.fp8_wgrad
    inject3 = {k: v for k, v in inject.items() if not k.endswith("attn.qkv.weight")}
    eng.f8a_scale.copy_(act2_dev); eng.fp8_bwd_state = 2; eng.g8_scale.view(depth, 4).copy_(sc); eng.fp8_wgrad = False
    assert eng.fp8_wgrad_mode() == 0
    eng.forward(mels, lens); eng.backward()
    g_w16 = eng.g32.clone()
    eng.fp8_wgrad = True
    _, o_w16 = oracle_grads(W, fwd, True, gates2, ctxs=(O.emulate_fp8(act_scales=act2), O.emulate_fp8_dgrad(inject3, wgrad=False)))
    # ... and the intermediate mode (ATST_FP8_QKV=0: e4m3 fc1 / fc2 / proj weight gradients, bf16 qkv pair) against ITS emulation
    eng.f8a_scale.copy_(act2_dev); eng.fp8_bwd_state = 2; eng.g8_scale.view(depth, 4).copy_(sc); eng.fp8_qkv_state = 0
    assert eng.fp8_wgrad_mode() == 1
    eng.forward(mels, lens); eng.backward()
    g_q16 = eng.g32.clone()
    eng.fp8_qkv_state = 2
    _, o_q16 = oracle_grads(W, fwd, True, gates2, ctxs=(O.emulate_fp8(act_scales=act2), O.emulate_fp8_dgrad(inject3, wgrad=True)))
    m4, w4 = table(hip_of(g_q16), or_of(o_q16))
    print(f"[fp8 base depth {depth}] HIP vs oracle, e4m3 dgrad + weight gradients without the qkv pair: mean {m4:.3e} worst {w4[0]} {w4[1]:.3e}")
    assert m4 < 9e-2 and w4[1] < 0.2
    for i in range(depth):
        for nm in ("mlp.fc1.weight", "mlp.fc2.weight", "attn.proj.weight", "attn.qkv.weight"):
            off, shape = eng.layout.entries[f"encoder.blocks.{i}.{nm}"]
            n = math.prod(shape)
            r_hip = relerr(g_fp8[off:off + n], g_w16[off:off + n])
            r_or = relerr(o_fp8[f"encoder.blocks.{i}.{nm}"].reshape(-1), o_w16[f"encoder.blocks.{i}.{nm}"].reshape(-1))
            print(f"  e4m3 vs bf16 weight gradient, block {i} {nm}: HIP {r_hip:.3e}  oracle {r_or:.3e}")
            assert 1e-4 < r_hip < 6e-2 and abs(r_hip - r_or) < 0.6 * max(r_hip, r_or), (nm, r_hip, r_or)
        off, shape = eng.layout.entries[f"encoder.blocks.{i}.attn.qkv.weight"]
        assert relerr(g_q16[off:off + math.prod(shape)], g_w16[off:off + math.prod(shape)]) < 1e-5   # mode 1: the bf16 qkv weight gradient of the same dqkv (the weight-gradient mode does not touch the data gradients)
    eng.optimizer_step(1e-3, 0.04, 0.99)
    l1 = float(eng.forward(mels, lens)[0]); eng.backward()
    assert math.isfinite(l1) and torch.isfinite(eng.p32).all()


def test_configs4_base_fp8_hires_as_one_thing():
    """BASELINE.json configs[4] with every piece switched on TOGETHER: ATST-base (d = 768, depth 2 here), 10 s @ 32 kHz through the HIP
    front end with 128 mel bands, one patch row of 128 x 8 (the reference parameterises n_mels / patch_h / patch_w together:
    methods/atstframe/train.py:15,50-51, transform.py:14-17), e4m3 forward GEMMs and e4m3 fc2 / fc1 / proj dgrad GEMMs with delayed
    scaling -- against the oracle evaluated the same way (log_mel(sample_rate=32000, n_mels=128), emulate_bf16 + emulate_fp8 +
    emulate_fp8_dgrad on HIP's quantisation grid, HIP's ReLU gates).  Tolerances: those of the separate tests of each piece."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from parity_helpers import oracle_grads
    from audiossl_amd.engine import AtstEngine
    from audiossl_amd.frontend import LogMelFrontend
    depth, B, sr = 2, 6, 32000
    W = O.recipe_weights("base", depth=depth, seed=17, patch_h=128, patch_w=8)
    eng = AtstEngine("base", depth=depth, drop_path_rate=0.0, fp8=True, patch_h=128, patch_w=8)
    eng.load_weights(W)
    # white noise has a flat spectrum: every patch of its log-mel is the same up to noise, the 12 head rows become nearly identical and
    # their BatchNorm turns any forward difference into an O(1) gradient difference (measured: 1.1).  Clips with structure instead:
    # six amplitude-modulated tones per clip on top of the recipe noise, all drawn from a seeded generator.
    gen = torch.Generator().manual_seed(11)
    t = torch.arange(11 * sr, dtype=torch.float64) / sr
    wave = 0.02 * O.recipe_wave(B, 11 * sr, seed=5).double()
    for b in range(B):
        for _ in range(6):
            f, fm, ph, amp = (float(v) for v in torch.rand(4, generator=gen))
            wave[b] += (0.05 + 0.15 * amp) * torch.sin(2 * math.pi * (100.0 + 6000.0 * f * f) * t + 6.28 * ph) * (0.55 + 0.45 * torch.sin(2 * math.pi * (0.3 + 2.5 * fm) * t))
    wave = wave.clamp(-1.0, 1.0).float()
    views = [wave[:, :10 * sr].contiguous(), wave[:, sr // 2:sr // 2 + 10 * sr].contiguous()]
    fe = LogMelFrontend(1024, sr=sr, n_mels=128)
    mels = [fe(v.to(DEV)) for v in views]
    mels_c = [O.log_mel(v, 1024, n_mels=128, sample_rate=sr) for v in views]
    assert mels[0].shape == (B, 1, 128, 2001)
    dmel = max(float((a.cpu() - b).abs().max()) for a, b in zip(mels, mels_c))
    assert dmel < 2e-3, dmel                                               # the front-end tolerance of tests/test_frontend_gpu.py
    lens = [torch.full((B,), 2001), torch.tensor([2001, 1801, 1283, 2001, 999, 2001])]
    ep = eng._pass("student", 2 * B, 2001, True, 0)
    assert ep.n_tok == 250 and ep.NP == 256 and eng.fp8_bwd_state == 1
    fwd = lambda Wl: O.atst_forward(Wl, mels_c, lens, "base", 2, depth=depth, drop_path_rate=0.0)
    loss1 = float(eng.forward(mels, lens)[0])
    gates = {f"student.{w}.": (eng.heads[f"student.{w}"].saved[4][:, :4096].float() > 0).cpu() for w in ("projector", "predictor")}
    cls = eng._student_groups[0][0].out.float().view(2 * B, 256, 768)[:, 0].cpu()
    with torch.no_grad(), O.emulate_bf16(), O.emulate_fp8():
        cls_o = O.encoder_forward(W, "student.encoder.", torch.cat(mels_c), torch.cat(lens), "base", depth=depth, drop_path_rate=0.0)
    e_cls = relerr(cls, cls_o)
    eng.backward()                                                         # recording step (bf16 dgrad)
    sc = eng.g8_scale.view(depth, 4).clone()
    site = {0: "mlp.fc2.weight", 1: "mlp.fc1.weight", 2: "attn.proj.weight", 3: "attn.qkv.weight"}
    inject = {f"student.encoder.blocks.{i}.{nm}": float(sc[i, k]) for i in range(depth) for k, nm in site.items()}
    assert eng.fp8_bwd_state == 2 and min(inject.values()) > 1.0 and eng.fp8_wgrad_mode() == 2      # all 12 GEMMs of a block on e4m3 operands
    act2 = _act_scales(eng)                                                # the running forward scales step 2 quantises with
    loss2 = float(eng.forward(mels, lens)[0])                              # e4m3 dgrad step, same weights and inputs
    gates = {f"student.{w}.": (eng.heads[f"student.{w}"].saved[4][:, :4096].float() > 0).cpu() for w in ("projector", "predictor")}
    eng.backward()
    g = eng.g32.clone()
    lo, go = oracle_grads(W, fwd, True, gates, ctxs=(O.emulate_fp8(act_scales=act2), O.emulate_fp8_dgrad(inject, wgrad=eng.fp8_wgrad, qkv=True)))
    num = den = 0.0
    worst = ("", 0.0)
    for name, (off, shape) in eng.layout.entries.items():
        n = math.prod(shape)
        if name not in go or float(go[name].norm()) == 0.0 or name in ("encoder.pos_embed", "encoder.norm.bias"):
            continue
        r = relerr(g[off:off + n].cpu(), go[name].reshape(-1))
        num += r * n; den += n
        if r > worst[1]:
            worst = (name, r)
    print(f"\n[configs[4] base fp8 hires depth {depth}] mel max|d| {dmel:.1e}; CLS vs fp8-emulating oracle {e_cls:.3e}; loss {loss2:.5f} (oracle {lo:.5f}); "
          f"gradients mean {num / den:.3e} worst {worst[0]} {worst[1]:.3e}")
    assert abs(loss1 - loss2) < 2e-2 and abs(loss2 - lo) < 5e-2            # step 2 quantises its activations on the adapted grid
    assert e_cls < 5.5e-2                                                  # test_fp8_encoder_forward_and_step_base
    assert num / den < 1.3e-1 and worst[1] < 0.25                          # measured 8.8e-2 / 0.16 (x1.5): 12 head rows (test_fp8_dgrad_step_base: 16 rows, 7.6e-2 / 0.17)
    eng.optimizer_step(1e-3, 0.04, 0.99)
    assert torch.isfinite(eng.p32).all() and torch.isfinite(eng.g32).all()


@pytest.mark.parametrize("arch", ["base", "small"])
def test_fp8_multi_step_loss_curve_tracks_bf16(arch):
    """a multi-step comparison before trusting the e4m3 dgrad by default.  16 optimizer steps (fwd + bwd + HF-AdamW + EMA) of
    ATST-base (depth 2) from the same weights on the same stream of batches, three ways: bf16 | e4m3 forward, bf16 dgrad | e4m3 forward +
    fc2 / fc1 / proj dgrad (running activation scales, delayed gradient scales, 16-step windows).  The loss curves must stay together -- measured
    (tools/debug/fp8_curve.py, 24 steps): max |loss - bf16| 0.011, mean 0.0035 for both fp8 runs, the two fp8 runs within 0.003 of each other --
    and nothing may be clipped on the way.  arch "small" (round 6): the same at d = 384, where the fp8 backward became available this round."""
    from audiossl_amd.engine import AtstEngine
    N, depth, B = 16, 2, 16
    W = O.recipe_weights(arch, depth=depth, seed=7)

    def data(step):
        g = torch.Generator().manual_seed(1000 + step)
        mels = []
        for v in range(2):                                        # noise + per-clip ridges with a slow drift: the head rows must differ
            m = O.recipe_mel(B, 1001, seed=10 * step + v)
            f = torch.rand(B, 1, 64, 1, generator=g); tt = torch.linspace(0, 1, 1001).view(1, 1, 1, -1)
            mels.append((m * 0.3 + 0.7 * torch.sin(6.28 * (3 * f + 2 * tt * torch.rand(B, 1, 1, 1, generator=g)))).contiguous())
        return mels

    def run(kind):
        eng = AtstEngine(arch, depth=depth, drop_path_rate=0.0, fp8=kind != "bf16")
        eng.load_weights(W)
        if kind == "fp8_fwd":
            eng.fp8_bwd_state = 0
        losses = []
        for step in range(N):
            loss = eng.forward([m.to(DEV) for m in data(step)], [torch.full((B,), 1001)] * 2)[0]
            eng.backward()
            eng.optimizer_step(5e-4, 0.04, 0.99)
            losses.append(float(loss))
        assert kind == "bf16" or (kind == "fp8") == (eng.fp8_bwd_state == 2)
        return losses, (eng.fp8_saturation() if kind != "bf16" else {"student": 0, "teacher": 0})

    ref, _ = run("bf16")
    assert ref[-1] < 0.6 * ref[0]                                 # the run learns something (1.97 -> 0.93)
    curves = {}
    for kind in ("fp8_fwd", "fp8"):
        curves[kind], sat = run(kind)
        d = [abs(a - b) for a, b in zip(curves[kind], ref)]
        print(f"\n[fp8 curve {arch}] {kind}: max |loss - bf16| {max(d):.4f} mean {sum(d) / N:.4f}; last loss {curves[kind][-1]:.4f} (bf16 {ref[-1]:.4f}); clipped {sat}")
        assert all(math.isfinite(v) for v in curves[kind]) and max(d) < 3e-2 and sum(d) / N < 1e-2
        assert sat == {"student": 0, "teacher": 0}
    assert max(abs(a - b) for a, b in zip(curves["fp8"], curves["fp8_fwd"])) < 1e-2


@pytest.mark.parametrize("arch", ["base", "small"])
def test_fp8_inference_pass_bf16_residual_stream(arch):
    """fp8 inference / teacher passes keep their residual stream in bf16 (round 6; csrc/engine.hip `xb16`, tuning hook 2100 = off): the features of a
    teacher-style pass (no gradient, e4m3 GEMMs) against the oracle's fp8 emulation WITH the same rounding site (emulate_fp8(resid_bf16=True)) and, with the
    hook off, against the emulation without it -- both within the bound of the fp8 forward tests; the two engine modes differ from each other by bf16
    rounding of a 12-add residual stream (~1e-2 of an e4m3-staircase feature), far inside the 7.9e-2 the fp8 features are from fp32."""
    from audiossl_amd.engine import AtstEngine
    lib = hip.load()
    depth, S, d = 3, 6, 768 if arch == "base" else 384
    W = O.recipe_weights(arch, depth=depth, seed=91)
    eng = AtstEngine(arch, depth=depth, fp8=True)
    eng.load_weights(W)
    mel = O.recipe_mel(S, 1001, seed=93)
    length = torch.tensor([1001, 1001, 702, 1001, 523, 941])
    feats = {}
    try:
        lib.atst_tune_gemm_variant(2110)                                # d = 384: the fused LayerNorm epilogues (fp32 stream) would take precedence over the bf16 stream
        for hook in (2101, 2100):
            lib.atst_tune_gemm_variant(hook)
            ep = eng._pass("teacher", S, 1001, False, 0)
            out = ep.forward(mel.cuda(), eng._valid(length, 1), None, None)
            feats[hook] = out.float().view(S, 256, d)[:, 0].cpu()
        lib.atst_tune_gemm_variant(2111); lib.atst_tune_gemm_variant(2101)   # the shipped configuration
        out = eng._pass("teacher", S, 1001, False, 0).forward(mel.cuda(), eng._valid(length, 1), None, None)
        feats["shipped"] = out.float().view(S, 256, d)[:, 0].cpu()
    finally:
        lib.atst_tune_gemm_variant(2101); lib.atst_tune_gemm_variant(2111)
    errs = {}
    for hook, r16 in ((2101, True), (2100, False)):
        with torch.no_grad(), O.emulate_bf16(), O.emulate_fp8(resid_bf16=r16):
            cls_o = O.encoder_forward(W, "teacher.encoder.", mel, length, arch, depth=depth, drop_path_rate=0.0)
        errs[hook] = relerr(feats[hook], cls_o)
    with torch.no_grad():
        cls32 = O.encoder_forward(W, "teacher.encoder.", mel, length, arch, depth=depth, drop_path_rate=0.0)
    d_modes = relerr(feats[2101], feats[2100])
    print(f"\n[fp8 inference, bf16 residual stream, {arch}] CLS vs emulation: bf16 stream {errs[2101]:.3e}, fp32 stream {errs[2100]:.3e}; the two modes {d_modes:.3e}; "
          f"vs fp32 oracle {relerr(feats[2101], cls32):.3e} / {relerr(feats[2100], cls32):.3e}")
    assert errs[2101] < 5.5e-2 and errs[2100] < 5.5e-2                  # the bound of test_fp8_encoder_forward_and_step_base
    assert d_modes < 6e-2                                               # measured 4.1e-2 (small) : a 2^-9 perturbation of the stream moves a few per cent of the e4m3 codes behind it
    assert relerr(feats[2101], cls32) < 1.2 * relerr(feats[2100], cls32) + 1e-2
    # the shipped inference pass: base = the bf16 stream (bit for bit the 2101 run); small = fp32 stream with the LayerNorms in the GEMM epilogues
    if arch == "base":
        assert torch.equal(feats["shipped"], feats[2101])
    else:
        with torch.no_grad(), O.emulate_bf16(), O.emulate_fp8(resid_bf16=False):
            cls_f = O.encoder_forward(W, "teacher.encoder.", mel, length, arch, depth=depth, drop_path_rate=0.0)
        print(f"[fp8 inference, small, fused LayerNorm epilogues] CLS vs emulation {relerr(feats['shipped'], cls_f):.3e}; vs the separate-pass fp32-stream run {relerr(feats['shipped'], feats[2100]):.3e}")
        assert relerr(feats["shipped"], cls_f) < 5.5e-2
        assert relerr(feats["shipped"], feats[2100]) < 1e-3                # measured 0 on these CLS rows: the two LayerNorm forms differ in a few
                                                                           # elements by one bf16 step (next test), none of them feeds CLS at depth 3


def test_fp8_inference_small_fused_layernorm_epilogues_vs_separate_passes():
    """The shipped d = 384 fp8 inference pass (LayerNorms inside the residual GEMM epilogues, fp32 stream) against the separate-pass fp32-stream run
    (hooks 2110 + 2100), over EVERY token.  They are not bit-identical: the fused LayerNorm and ln_fwd_kernel reduce the row statistics in different
    orders, so a LayerNorm output next to a bf16 rounding boundary lands on the other side now and then -- measured at depth 1: 7 of 589,824 elements,
    each one bf16 step.  Through the e4m3 staircase that grows with depth: measured 4.1e-3 at depth 6, 1.7e-2 at depth 12 (24 residual adds)."""
    from audiossl_amd.engine import AtstEngine
    lib = hip.load()
    S = 6
    for depth, bound in ((1, None), (12, 2.5e-2)):
        W = O.recipe_weights("small", depth=depth, seed=95)
        eng = AtstEngine("small", depth=depth, fp8=True)
        eng.load_weights(W)
        mel = O.recipe_mel(S, 1001, seed=97).cuda()
        valid = eng._valid(torch.tensor([1001, 640, 1001, 1001, 333, 999]), 1)
        try:
            shipped = eng._pass("teacher", S, 1001, False, 0).forward(mel, valid, None, None).float().clone()
            lib.atst_tune_gemm_variant(2110); lib.atst_tune_gemm_variant(2100)
            separate = eng._pass("teacher", S, 1001, False, 0).forward(mel, valid, None, None).float().clone()
        finally:
            lib.atst_tune_gemm_variant(2101); lib.atst_tune_gemm_variant(2111)
        assert torch.isfinite(shipped).all()
        if bound is None:                                                  # one LayerNorm pair: a few elements, one bf16 step each
            d = shipped != separate
            step = (shipped - separate).abs() / separate.abs().clamp_min(1e-30)
            assert int(d.sum()) <= 1e-4 * d.numel() and float(step.max()) <= 2.0 ** -7, (int(d.sum()), float(step.max()))
        else:
            assert relerr(shipped, separate) < bound, relerr(shipped, separate)


def test_fp8_forward_saturation_counter_and_running_scales():
    """The e4m3 forward starts from the activation scales of rounds 2 / 3 (8; 4 behind GELU: |x| > 56 / 112 clips at +-448) and adapts them:
    every site records its amax, the next step quantises with 448 / (2 * max over the window) (atst_encoder_t.f8_act_scale / f8_act_amax).
    Every quantising kernel counts what it clipped (f8_sat, AtstEngine.fp8_saturation()).  Zero on the recipe weights; with a student
    LayerNorm gain of 40 the FIRST forward clips (student only) and the second -- on the adapted scales -- does not."""
    from audiossl_amd.engine import AtstEngine
    depth, B = 1, 2
    W = O.recipe_weights("base", depth=depth, seed=7)
    mels = [O.recipe_mel(B, 1001, seed=1).to(DEV), O.recipe_mel(B, 1001, seed=2).to(DEV)]
    lens = [torch.full((B,), 1001)] * 2
    eng = AtstEngine("base", depth=depth, drop_path_rate=0.0, fp8=True)
    eng.load_weights(W)
    assert torch.equal(eng.f8a_scale.cpu(), torch.tensor([8.0, 8.0, 8.0, 4.0]).repeat(2, depth))
    eng.forward(mels, lens)
    assert eng.fp8_saturation() == {"student": 0, "teacher": 0}
    sc1 = eng.f8a_scale.clone()
    assert float(eng.f8a_amax.abs().max()) == 0.0 and bool((sc1 > 1.0).all()) and not torch.equal(sc1.cpu(), torch.tensor([8.0, 8.0, 8.0, 4.0]).repeat(2, depth))
    W2 = {k: v.clone() for k, v in W.items()}
    W2["student.encoder.blocks.0.norm1.weight"] *= 40.0                      # LayerNorm output ~ N(0, 40^2): far beyond the range of any scale seen so far
    eng.load_weights(W2)
    loss = eng.forward(mels, lens)[0]
    sat = eng.fp8_saturation(reset=True)
    print(f"\n[fp8 saturation] clipped elements: {sat}; loss {float(loss):.4f}; LN1 site scale {float(sc1[0, 0]):.2f} -> {float(eng.f8a_scale[0, 0]):.3f}")
    assert sat["student"] > 1000 and sat["teacher"] == 0 and math.isfinite(float(loss))
    assert float(eng.f8a_scale[0, 0]) < 0.2 * float(sc1[0, 0])                # the window max now holds the large amax
    # the sites downstream of the clipped one saw clipped inputs in that forward, i.e. recorded too small an amax: one more step settles them
    eng.forward(mels, lens); eng.fp8_saturation(reset=True)
    eng.forward(mels, lens)
    assert eng.fp8_saturation() == {"student": 0, "teacher": 0}               # adapted: nothing clips any more


def test_fp8_forward_only_state_is_saved_and_restored(monkeypatch):
    """the forward activation scales, their 16-step amax window and its cursor are live for EVERY fp8 engine, also when the e4m3
    dgrad is off (ATST_FP8_BWD=0; until round 6 also every ATST-small engine) -- fp8_state() / load_fp8_state() must carry them, or a resumed run
    restarts from the constants 8 / 8 / 8 / 4 with an empty window."""
    from audiossl_amd.engine import AtstEngine
    monkeypatch.setenv("ATST_FP8_BWD", "0")
    depth, B = 1, 2
    W = O.recipe_weights("small", depth=depth, seed=7)
    mels = [O.recipe_mel(B, 1001, seed=1).to(DEV), O.recipe_mel(B, 1001, seed=2).to(DEV)]
    lens = [torch.full((B,), 1001)] * 2
    eng = AtstEngine("small", depth=depth, drop_path_rate=0.0, fp8=True)
    assert eng.fp8_bwd_state == 0                                              # forward-only fp8 (ATST_FP8_BWD=0)
    eng.load_weights(W)
    for _ in range(3):
        eng.forward(mels, lens)
    st = eng.fp8_state()
    assert st is not None and "f8a_scale" in st and "g8_scale" not in st and st["f8a_hist_k"] == 3
    assert not torch.equal(st["f8a_scale"], torch.tensor([8.0, 8.0, 8.0, 4.0]).repeat(2, depth))
    eng2 = AtstEngine("small", depth=depth, drop_path_rate=0.0, fp8=True)
    eng2.load_weights(W)
    eng2.load_fp8_state(st)
    assert torch.equal(eng2.f8a_scale.cpu(), st["f8a_scale"]) and torch.equal(eng2.f8a_hist.cpu(), st["f8a_hist"]) and eng2._f8a_hist_k == 3
    l1, l2 = eng.forward(mels, lens)[0], eng2.forward(mels, lens)[0]           # the resumed engine quantises as the saved one does
    assert float(l1) == float(l2)


def test_fp8_base_state_machine_checkpoint_and_lean_contract():
    """Host-side contracts of the all-e4m3 base step (round 5):
      * the delayed-scaling state incl. the qkv site (fp8_qkv_state) survives fp8_state() / load_fp8_state(), and the resumed engine takes the same step;
      * a checkpoint written BEFORE the qkv path existed (no "qkv_state" key, site-3 scale never observed) makes the engine record one step first --
        bf16 qkv pair, wgrad mode 3 -- instead of quantising dqkv with the placeholder scale 1;
      * a forward that left out bf16 activation copies (fp8_lean) refuses a backward whose mode changed in between (it would read copies never written)."""
    from audiossl_amd.engine import AtstEngine
    depth, B = 1, 2
    W = O.recipe_weights("base", depth=depth, seed=7)
    mels = [O.recipe_mel(B, 1001, seed=1).to(DEV), O.recipe_mel(B, 1001, seed=2).to(DEV)]
    lens = [torch.full((B,), 1001)] * 2
    eng = AtstEngine("base", depth=depth, drop_path_rate=0.0, fp8=True)
    eng.load_weights(W)
    for _ in range(2):
        eng.forward(mels, lens); eng.backward()
    assert eng.fp8_bwd_state == 2 and eng.fp8_qkv_state == 2 and eng.fp8_wgrad_mode() == 2
    st = eng.fp8_state()
    assert st["state"] == 2 and st["qkv_state"] == 2 and float(st["g8_scale"].view(depth, 4)[:, 3].min()) > 1.0
    eng2 = AtstEngine("base", depth=depth, drop_path_rate=0.0, fp8=True)
    eng2.load_weights(W); eng2.load_fp8_state(st)
    assert eng2.fp8_bwd_state == 2 and eng2.fp8_qkv_state == 2
    la = float(eng.forward(mels, lens)[0]); eng.backward(); ga = eng.g32.clone()
    lb = float(eng2.forward(mels, lens)[0]); eng2.backward()
    assert la == lb and relerr(eng2.g32, ga) < 1e-5                             # same scales, same codes: only the order of the fp32 atomics differs
    assert eng2._student_groups[0][0].e.fp8_lean == 2
    # an old checkpoint: no qkv_state, site 3 never observed
    old = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items() if k != "qkv_state"}
    old["g8_scale"].view(depth, 4)[:, 3] = 1.0; old["g8_hist"].view(-1, depth, 4)[:, :, 3] = 0.0
    eng3 = AtstEngine("base", depth=depth, drop_path_rate=0.0, fp8=True)
    eng3.load_weights(W); eng3.load_fp8_state(old)
    assert eng3.fp8_bwd_state == 2 and eng3.fp8_qkv_state == 1 and eng3.fp8_wgrad_mode() == 3
    eng3.forward(mels, lens)
    assert eng3._student_groups[0][0].e.fp8_lean == 1                           # fc1 / fc2 / proj weight gradients in e4m3, the qkv pair still bf16
    eng3.backward()
    assert eng3.fp8_qkv_state == 2 and float(eng3.g8_scale.view(depth, 4)[:, 3].min()) > 1.0 and torch.isfinite(eng3.g32).all()
    ratio = float(eng3.g8_scale.view(depth, 4)[0, 3]) / float(st["g8_scale"].view(depth, 4)[0, 3])
    assert 0.5 < ratio < 2.0, ratio                                            # one observation vs the other engine's window of two (measured 1.21)
    # the lean contract
    eng3.forward(mels, lens)
    eng3.fp8_wgrad = False                                                        # would need the bf16 h2 / a this forward did not write
    with pytest.raises(RuntimeError, match="fp8_lean"):
        eng3.backward()
    eng3.fp8_wgrad = True                                                         # refused before anything was consumed: the same backward goes through now
    eng3.backward()
    assert torch.isfinite(eng3.g32).all()


@pytest.mark.parametrize("M,N,K", [(512, 768, 768), (1024, 2304, 768), (8192, 768, 3072), (8192 + 256, 3072, 768)])
def test_gemm_fp8_phased_kernel(M, N, K):
    """The e4m3 form of the 256 x 256 phased kernel (csrc/gemm_p8.h, F8 = true: one v_mfma_scale_f32_32x32x64_f8f6f4 per 64-byte k-step) through
    atst_gemm_nt_fp8: every epilogue of the C ABI against an fp32 matmul of the SAME e4m3 values, and against the kernel it replaces (hook 390)."""
    lib = hip.load()
    g = torch.Generator().manual_seed(M + N)
    A = (torch.randn(M, K, generator=g) * 1.5).to(DEV).bfloat16()
    W = (torch.randn(N, K, generator=g) * 0.05).to(DEV).bfloat16()
    A8 = torch.empty(M, K, dtype=torch.uint8, device=DEV); W8 = torch.empty(N, K, dtype=torch.uint8, device=DEV)
    hip.call("atst_quant_fp8_bf16", hip.ptr(A), M * K, 8.0, hip.ptr(A8), hip.stream())
    hip.call("atst_quant_fp8_bf16", hip.ptr(W), N * K, 64.0, hip.ptr(W8), hip.stream())
    dq = torch.tensor([1.0 / 64.0], device=DEV)
    ref = (A8.view(torch.float8_e4m3fn).double() @ W8.view(torch.float8_e4m3fn).double().t()).float() / (8.0 * 64.0)
    bias = torch.randn(N, device=DEV)
    rps = 64
    resid = rnd(M, N, seed=4)
    scale = torch.tensor([1.0, 0.0, 1.25, 1.0], device=DEV).repeat(M // (4 * rps) + 1)[:M // rps].contiguous()
    res = {}
    try:
        lib.atst_tune_gemm_variant(351)
        for hook in (390, 393):                                               # 393 (default): the phased kernel for every e4m3 GEMM (392: all but fc1 + GELU)
            lib.atst_tune_gemm_variant(hook)
            outs = []
            for epi, dt in ((hip.EPI_F32, torch.float32), (hip.EPI_BF16, torch.bfloat16), (hip.EPI_BIAS_GELU, torch.bfloat16), (hip.EPI_RESID, torch.float32)):
                out = torch.empty(M, N, device=DEV, dtype=dt)
                c2 = torch.empty(M, N, device=DEV, dtype=torch.bfloat16) if epi == hip.EPI_BIAS_GELU else None
                hip.call("atst_gemm_nt_fp8", hip.ptr(A8), hip.ptr(W8), M, N, K, K, K, epi, hip.ptr(out), N, hip.ptr(c2), hip.ptr(bias),
                         hip.ptr(resid) if epi == hip.EPI_RESID else None, hip.ptr(scale) if epi == hip.EPI_RESID else None, rps, hip.ptr(dq), 1.0 / 8.0, hip.stream())
                outs += [out] + ([c2] if c2 is not None else [])
            res[hook] = outs
    finally:
        lib.atst_tune_gemm_variant(393); lib.atst_tune_gemm_variant(350)
    f32, b16, u, a, x = res[393]
    assert relerr(f32, ref + bias) < 5e-5
    assert relerr(b16.float(), ref + bias) < 4e-3 and relerr(u.float(), ref + bias) < 4e-3
    assert relerr(a.float(), torch.nn.functional.gelu(ref + bias)) < 5e-3
    assert relerr(x, resid + scale.repeat_interleave(rps)[:, None] * (ref + bias)) < 5e-5
    for got, other in zip(res[393], res[390]):
        assert relerr(got.float(), other.float()) < 4e-3


@pytest.mark.parametrize("M,N,K", [(2048 + 40, 1152, 384), (4096, 384, 384), (26624, 384, 1536)])
def test_gemm_fp8_small_grid_four_wave_kernel(M, N, K):
    """Round 6: e4m3 GEMMs whose grid is at most 1.5 rounds of 256 x 384 tiles (the 1 s local views of the e4m3 step at d = 384) run on the 4-wave
    kernels, two blocks per CU (hook 2121; 2120 = the 8-wave 256-row tile, the default: the 4-wave form measured -0.5 % in the step).  Every accumulator sees the same k-tiles in the same order:
    the plain-bf16 epilogue is bit-identical between the two, and both match the fp64 product of the same e4m3 values."""
    lib = hip.load()
    g = torch.Generator().manual_seed(M + N)
    A = (torch.randn(M, K, generator=g) * 1.5).to(DEV).bfloat16()
    W = (torch.randn(N, K, generator=g) * 0.05).to(DEV).bfloat16()
    A8 = torch.empty(M, K, dtype=torch.uint8, device=DEV); W8 = torch.empty(N, K, dtype=torch.uint8, device=DEV)
    hip.call("atst_quant_fp8_bf16", hip.ptr(A), M * K, 8.0, hip.ptr(A8), hip.stream())
    hip.call("atst_quant_fp8_bf16", hip.ptr(W), N * K, 64.0, hip.ptr(W8), hip.stream())
    dq = torch.tensor([1.0 / 64.0], device=DEV)
    ref = (A8.view(torch.float8_e4m3fn).double() @ W8.view(torch.float8_e4m3fn).double().t()).float() / (8.0 * 64.0)
    outs = {}
    try:
        for hook in (2120, 2121):
            lib.atst_tune_gemm_variant(hook)
            out = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
            hip.call("atst_gemm_nt_fp8", hip.ptr(A8), hip.ptr(W8), M, N, K, K, K, hip.EPI_BF16, hip.ptr(out), N, None, None, None, None, 1, hip.ptr(dq), 1.0 / 8.0, hip.stream())
            outs[hook] = out
    finally:
        lib.atst_tune_gemm_variant(2120)
    assert relerr(outs[2121].float(), ref) < 4e-3
    assert torch.equal(outs[2120], outs[2121])


@pytest.mark.parametrize("M,N,K", [(256, 256, 256), (1024, 768, 768), (8192 + 64, 768, 3072), (4096, 3072, 768),
                                   (1024, 384, 384), (2048 + 64, 1152, 384), (4096, 384, 1536), (512, 128, 128)])   # multiples of 128: half-valid edge tiles (d = 384)
def test_gemm_tn_fp8_weight_gradient(M, N, K):
    """e4m3 weight gradient (csrc/gemm_tn8.hip: transposed LDS reads ds_read_b64_tr_b8 + MX-scaled MFMA): dW += dY8^T X8 / (sy sx) against an fp64
    matmul of the SAME e4m3 values (only the summation order differs), accumulation into a non-zero dW, asymmetric operands (a transposed or
    permuted fragment would show), ragged last M-split."""
    g = torch.Generator().manual_seed(M + N + K)
    dY = (torch.randn(M, N, generator=g) * 0.02).to(DEV).bfloat16(); X = (torch.randn(M, K, generator=g) * 1.5).to(DEV).bfloat16()
    X[:, 0] = 3.0; dY[0] = 0.05                                                     # structure along both axes
    sy, sx = torch.tensor([2048.0], device=DEV), torch.tensor([8.0], device=DEV)
    dY8 = torch.empty(M, N, dtype=torch.uint8, device=DEV); X8 = torch.empty(M, K, dtype=torch.uint8, device=DEV)
    hip.call("atst_quant_fp8_bf16", hip.ptr(dY), M * N, 2048.0, hip.ptr(dY8), hip.stream())
    hip.call("atst_quant_fp8_bf16", hip.ptr(X), M * K, 8.0, hip.ptr(X8), hip.stream())
    dW = torch.full((N, K), 0.5, device=DEV)
    hip.call("atst_gemm_tn_fp8", hip.ptr(dY8), hip.ptr(X8), M, N, K, N, K, hip.ptr(dW), K, hip.ptr(sy), hip.ptr(sx), hip.stream())
    ref = (dY8.view(torch.float8_e4m3fn).double().t() @ X8.view(torch.float8_e4m3fn).double()) / (2048.0 * 8.0) + 0.5
    assert relerr(dW, ref.float()) < 2e-5
    # and close to the bf16 weight gradient of the unquantised operands (e4m3: 2^-4 relative per element, averaged over M)
    ref16 = dY.float().t() @ X.float() + 0.5
    assert relerr(dW, ref16) < 8e-2


@pytest.mark.parametrize("C", [768, 384])
@pytest.mark.parametrize("M", [4096, 8192 + 192])
def test_gemm_tn_group_fp8_matches_single_launches(M, C):
    """The four e4m3 weight gradients of an ATST-base block in ONE launch (atst_gemm_tn_group_fp8: shared M, shared M-splits, a fraction of the fp32
    atomics) against the same four problems launched one by one, and against the fp64 product of the e4m3 values; 3- and 4-problem groups, own scales.
    C = 384 (round 6): every dimension is a multiple of 128 but not of 256 -- 38 tiles with half-valid edges."""
    shapes = [(4 * C, C), (C, 4 * C), (C, C), (3 * C, C)]                          # fc1, fc2, proj, qkv: (N, K)
    g = torch.Generator().manual_seed(M)
    ops = []
    for i, (N, K) in enumerate(shapes):
        dY = (torch.randn(M, N, generator=g) * 0.02).to(DEV).bfloat16(); X = (torch.randn(M, K, generator=g) * 1.5).to(DEV).bfloat16()
        X[:, 0] = 3.0; dY[0] = 0.05
        sy, sx = torch.tensor([1024.0 * (i + 1)], device=DEV), torch.tensor([8.0 / (i + 1)], device=DEV)
        dY8 = torch.empty(M, N, dtype=torch.uint8, device=DEV); X8 = torch.empty(M, K, dtype=torch.uint8, device=DEV)
        hip.call("atst_quant_fp8_bf16", hip.ptr(dY), M * N, float(sy), hip.ptr(dY8), hip.stream())
        hip.call("atst_quant_fp8_bf16", hip.ptr(X), M * K, float(sx), hip.ptr(X8), hip.stream())
        ops.append((dY8, X8, N, K, sy, sx))
    for n in (3, 4):
        one = [torch.full((N, K), 0.25, device=DEV) for _, _, N, K, _, _ in ops[:n]]
        grp = [torch.full((N, K), 0.25, device=DEV) for _, _, N, K, _, _ in ops[:n]]
        items = (hip.Wgrad8 * n)()
        for i, (dY8, X8, N, K, sy, sx) in enumerate(ops[:n]):
            hip.call("atst_gemm_tn_fp8", hip.ptr(dY8), hip.ptr(X8), M, N, K, N, K, hip.ptr(one[i]), K, hip.ptr(sy), hip.ptr(sx), hip.stream())
            items[i].dY8, items[i].X8, items[i].dW = dY8.data_ptr(), X8.data_ptr(), grp[i].data_ptr()
            items[i].N, items[i].K, items[i].ldy, items[i].ldx, items[i].ldw = N, K, N, K, K
            items[i].scale_y, items[i].scale_x = sy.data_ptr(), sx.data_ptr()
        hip.call("atst_gemm_tn_group_fp8", C_.byref(items), n, M, hip.stream())
        for i, (dY8, X8, N, K, sy, sx) in enumerate(ops[:n]):
            ref = (dY8.view(torch.float8_e4m3fn).double().t() @ X8.view(torch.float8_e4m3fn).double()) / (float(sy) * float(sx)) + 0.25
            assert relerr(grp[i], ref.float()) < 2e-5 and relerr(grp[i], one[i]) < 2e-5, (n, i)
