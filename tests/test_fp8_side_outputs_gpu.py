"""Kernel-level tests of the outputs the fused epilogues write BESIDE their main result in the e4m3 step: the e4m3 copy of the activation they
produce (the A operand of the next e4m3 GEMM), its amax site (the next step's delayed scale), the clipped-element counter, and the bf16 residual
stream of the fp8 inference / teacher passes -- called through the test entry points atst_gemm_nt_q8 / atst_layernorm_fwd_q8 / atst_layernorm_bwd_q8,
which fill GemmArgs / LnBwdArgs exactly as csrc/engine.hip does (gemm8, gemm8_bwd, the bf16 dGELU of the recording step, the unfused LayerNorms).

References: fp64 products of the same e4m3 / bf16 values, torch.float8_e4m3fn conversion, autograd for GELU, GELU' and LayerNorm.
  * main outputs: fp32 within 5e-5 of the fp64 reference, bf16 within 4e-3 (the bounds of test_ops_gpu.py);
  * e4m3 copies: BIT-exact against e4m3(clamp(bf16_out * s, +-448)) of the kernel's OWN bf16 output from the same launch; with the bf16 output left out
    (lean / inference) the bytes equal those of the launch that wrote it; a device scale equal to the host scale gives the same bytes;
  * amax sites: posts only into the 16 slot heads; a larger pre-filled value survives, a smaller one is replaced; rows beyond M (filled with huge
    operand values) never post.  EXACT where the kernel takes the max of the values it rounds to bf16 (LayerNorm forward: max |bf16 y|) or of an fp32
    value the reference can reproduce (LayerNorm backward: max |row_scale dx| of the kernel's own dx); within ONE bf16 rounding (2^-8 relative) where it
    takes the fp32 value before rounding (fc1 + GELU: max |gelu| ; dGELU: max |du|, csrc/gemm.hip epilogue8);
  * clip counters: start value + count(|bf16(v) s| > 448), exactly, with data that clips several elements;
  * dq_div (device scale the accumulators are divided by) against dq_mul = 1 / scale: within 1e-6;
  * bf16 residual stream: bf16 out == bf16 rounding of the fp32-out run; bf16 in == the fp32-in run fed the same values upcast; in place (resid == C,
    as the engine runs it) == out of place; all within 4e-3 of fp64;
  * sentinels past M * ldc of every q8 / C buffer stay untouched.

Which launcher branch carries each side output (csrc/gemm.hip launch_nt / launch_nt_row384; row counts and hooks choose it, defaults restored in `finally`):

  side output                          | branch (kernel, as rocprofv3 names it)                 | test id
  -------------------------------------+--------------------------------------------------------+----------------------------------------------------------
  fc1+GELU e4m3: q8, amax, sat, lean   | p8 phased 256x256: gemm_nt_p8_kernel<2, true>           | test_bias_gelu_q8[8192-3072-768-None], [4096-3072-768-351]
                                       | row-384: gemm_nt_row384_kernel<2, 4, .., true (F8)>     | test_bias_gelu_q8[640|700|2088|8256|32832|26624|8192-..-None] (e4m3 K = 384:
                                       |                                                         | K / 2 % 128 != 0, never p8), [8192-1536-384-392]
  dGELU e4m3: du8, amax, colsum, lean  | p8 phased: gemm_nt_p8_kernel<4, true>                   | test_dgelu_e4m3_q8[8192-3072-768-None], [4096-3072-768-351]
                                       | row-384: gemm_nt_row384_kernel<4, 4, .., true>          | test_dgelu_e4m3_q8[640|2088|4096|8256|8192-..-None], [8192-1536-384-390]
  dGELU bf16: amax only (recording)    | 128x128 2-stage: gemm_nt_kernel<4, 128, 2, 64>          | test_dgelu_bf16_amax[640|2088|4096|8256-1536-384-None] (fcdef88: < 8192 rows,
                                       |                                                         | K = 384), [700-1536-384-4] (K < 768 overrides variant 4), [8192-1536-384-390]
                                       | 128x128 3-stage: gemm_nt_kernel<4, 128, 3, 64>          | test_dgelu_bf16_amax[2088-3072-768-306], [700-1536-384-1]
                                       | 256x128: gemm_nt_kernel<4, 256, 3, 128>                 | test_dgelu_bf16_amax[2088-1536-384-3]
                                       | row-384 128-row: gemm_nt_row384_kernel<4, 2, ..>        | test_dgelu_bf16_amax[2088-3072-768-None], [640-1536-384-307]
                                       | row-384 256-row: gemm_nt_row384_kernel<4, 4, .., PH=1>  | test_dgelu_bf16_amax[8256-3072-768-None]
                                       | p8 phased bf16: gemm_nt_p8_kernel<4, false>             | test_dgelu_bf16_amax[8192-1536-384-None], [26624-1536-384-None]
  resid_bf16 / out_bf16 (xb16)         | p8 phased: gemm_nt_p8_kernel<3, true>                   | test_resid_bf16_stream[8192-768-3072-None]
                                       | row-384: gemm_nt_row384_kernel<3, 4, .., true>          | test_resid_bf16_stream[700|2088|4096|8256|8192|26624-..-None], [8192-384-1536-390]
  dq_div vs dq_mul                     | p8: gemm_nt_p8_kernel<1, true>                          | test_dq_div_matches_dq_mul[8192-768-3072-1-None]
                                       | row-384: gemm_nt_row384_kernel<0|1, 4, .., true>        | test_dq_div_matches_dq_mul[700-..], [8192-1536-384-1-390], [26624-..], [8256-..]
                                       | 4-wave e4m3: gemm_nt_w4_kernel<0, 2, .., true>          | test_dq_div_matches_dq_mul[2088-1152-384-0-2121], [4096-384-384-0-2121]
  LayerNorm fwd y8, amax, sat, lean    | ln_fwd_kernel<6|12, bf16, float|bf16>                   | test_layernorm_fwd_q8[*]
  LayerNorm bwd g8, g_amax, g = null   | ln_bwd_kernel<6|12>                                     | test_layernorm_bwd_q8[*]
  weight-shadow prep                   | cast_kernel, transpose_batch_kernel, quant_bf16_table_kernel | test_cast_bf16_rne, test_transpose_bf16_batch_*, test_quant_bf16_table_fp8
  (launch counts per kernel: profiles/r07_side_outputs_kernel_stats.txt)

Row counts: besides the ragged edges (640, 700, 2048 + 40, 8192 + 64, 32768 + 64) they include what the multi-rank tests run per rank --
tests/test_dist_gpu.py: 2 ranks x 8 clips x 2 views x 256 rows = 4096 (the 1-rank reference: 8192), 8 ranks x 4 clips = 2048 -- and what bench.py runs
per GPU on ANY rank count (256 clips per GPU: the 4 local 1 s views 26624 rows, 4096 rows per 16 clips of a global view).  fcdef88 (the 128x128 dGELU kernel
never posted the du amax) lived below 8192 rows at K = 384: test_dgelu_bf16_amax[640 | 2088 | 4096-1536-384-None].
"""
import contextlib
import ctypes as C_

import pytest
import torch

pytestmark = pytest.mark.gpu

from audiossl_amd import hip  # noqa: E402

DEV = "cuda"
F8 = torch.float8_e4m3fn
SENT = 0xA5                                     # sentinel byte past M * ldc of every output buffer
PAD = 4096                                      # sentinel bytes
HUGE = 2.0 ** 100                               # pre-filled amax site value that must survive (exact in fp32)
BIG = 200.0                                     # operand value of the rows beyond M: they would dominate every amax if they were posted
# defaults of the tuning hooks these tests move (include/atst_hip.h): variant auto, row-384 auto, tall tiles everywhere, dGELU row-384 from K = 768,
# 4-wave auto for small grids, tall / 4-wave from M = 8192, phased kernel for every e4m3 GEMM, 8-wave e4m3 small grids
DEFAULT_HOOKS = (-1, 301, 304, 308, 361, 350, 393, 2120)


def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _e4m3(x, scale):
    return (x.float() * scale).clamp(-448.0, 448.0).to(F8)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    hip.load()
    yield
    torch.cuda.synchronize()


@contextlib.contextmanager
def hooks(*hs):
    lib = hip.load()
    try:
        for h in hs:
            if h is not None:
                lib.atst_tune_gemm_variant(h)
        yield
    finally:
        for h in DEFAULT_HOOKS:
            lib.atst_tune_gemm_variant(h)


class Guarded:
    """An output buffer [rows, cols] followed by PAD sentinel bytes: `t` is the tensor the kernel sees, `intact()` checks the tail."""

    def __init__(self, rows, cols, dtype):
        n = rows * cols * torch.tensor([], dtype=dtype).element_size()
        self.raw = torch.full((n + PAD,), SENT, dtype=torch.uint8, device=DEV)
        self.t = self.raw[:n].view(dtype).view(rows, cols)
        self.n = n

    def intact(self):
        return bool((self.raw[self.n:] == SENT).all())


def site(fill=0.0):
    s = torch.zeros(hip.AMAX_SITE_STRIDE, device=DEV)
    s.view(hip.AMAX_SLOTS, hip.AMAX_SLOT_STRIDE)[:, 0] = fill
    return s


def heads_only(s):
    """posts go to the 16 slot heads, nothing between them"""
    return int((s.view(hip.AMAX_SLOTS, hip.AMAX_SLOT_STRIDE)[:, 1:] != 0).sum()) == 0


def counter(start):
    return torch.tensor([start], dtype=torch.int32, device=DEV)


def e4m3_operand(M, K, scale, seed, std=0.5, pad_rows=256):
    """e4m3 bytes [M + pad_rows, K] of a random [M, K] (scale `scale`); the rows beyond M hold BIG: a kernel that read them into an amax, a store or
    a clip count would show it.  Returns (bytes, decoded [M, K] fp64 / scale)."""
    x = rnd(M + pad_rows, K, scale=std, seed=seed)
    x[M:] = BIG / scale
    x8 = _e4m3(x, scale).view(torch.uint8).contiguous()
    return x8, x8[:M].view(F8).double() / scale


def gemm_q8(A, B, f8, M, N, K, epi, C=None, ldc=None, C2=None, bias=None, resid=None, row_scale=None, rps=1, U=None, colsum=None, dq=None, dq_mul=1.0,
            q8=None, q8_scale=0.0, q8_scale_dev=None, q8_amax=None, q8_sat=None, a_scale_dev=None, resid_bf16=0, out_bf16=0, rc=0):
    x = hip.GemmQ8(hip.ptr(q8), q8_scale, hip.ptr(q8_scale_dev), hip.ptr(q8_amax), hip.ptr(q8_sat), hip.ptr(a_scale_dev), resid_bf16, out_bf16)
    got = hip.load().atst_gemm_nt_q8(hip.ptr(A), hip.ptr(B), 1 if f8 else 0, M, N, K, K, K, epi, hip.ptr(C), ldc or N, hip.ptr(C2), hip.ptr(bias),
                                     hip.ptr(resid), hip.ptr(row_scale), rps, hip.ptr(U), hip.ptr(colsum), hip.ptr(dq), dq_mul, C_.byref(x), hip.stream())
    assert got == rc, f"atst_gemm_nt_q8 returned {got}, expected {rc}"


def check_amax(s, want, exact):
    """site value against the max |v| of the kernel's bf16 output: equal (exact) or within one bf16 rounding (the kernel took it before rounding)"""
    got = float(s.max())
    assert heads_only(s)
    if exact:
        assert got == want, (got, want)
    else:
        assert abs(got - want) <= 2.0 ** -8 * want, (got, want)


# ---- fc1 + GELU on e4m3 operands: the e4m3 activation copy (fc2's A operand), its amax and clip count ------------------------------------------------
@pytest.mark.parametrize("M,N,K,hook", [(640, 1536, 384, None), (700, 3072, 768, None), (2048 + 40, 1536, 384, None), (8192 + 64, 1536, 384, None),
                                        (32768 + 64, 1536, 384, None), (8192, 1536, 384, 392), (8192, 1536, 384, None), (26624, 1536, 384, None), (8192, 3072, 768, None),
                                        (4096, 3072, 768, 351)])
def test_bias_gelu_q8(M, N, K, hook):
    """gemm8(EPI_BIAS_GELU, q8, running scales) of the fp8 forward (engine.hip fc1): u and the GELU activation (bf16) against fp64; the e4m3 copy bit-exact
    against the kernel's own activation; amax within one bf16 rounding (taken before rounding); clip count exact; lean (u and a left out) = same bytes;
    device scale == host scale; dq_div == dq_mul = 1 / scale."""
    sa, sb, s8 = 12.0, 64.0, 96.0                                         # 448 / 96 = 4.67: the tail of the GELU output clips
    A8, Ad = e4m3_operand(M, K, sa, seed=M + 1, std=0.5)
    B8, Bd = e4m3_operand(N, K, sb, seed=N + 2, std=0.25, pad_rows=0)
    bias = rnd(N, seed=3, scale=0.5)
    dq, asc, s8d = torch.tensor([1.0 / sb], device=DEV), torch.tensor([sa], device=DEV), torch.tensor([s8], device=DEV)
    u = Ad @ Bd.t() + bias.double()
    a = torch.nn.functional.gelu(u)
    C, C2, q8 = Guarded(M, N, torch.bfloat16), Guarded(M, N, torch.bfloat16), Guarded(M, N, torch.uint8)
    s, sat = site(), counter(7)
    with hooks(hook):
        gemm_q8(A8, B8, True, M, N, K, hip.EPI_BIAS_GELU, C=C.t, C2=C2.t, bias=bias, dq=dq, q8=q8.t, q8_scale_dev=s8d, q8_amax=s, q8_sat=sat, a_scale_dev=asc)
        lean8, s_lean, sat_lean = Guarded(M, N, torch.uint8), site(), counter(0)
        gemm_q8(A8, B8, True, M, N, K, hip.EPI_BIAS_GELU, bias=bias, dq=dq, q8=lean8.t, q8_scale_dev=s8d, q8_amax=s_lean, q8_sat=sat_lean, a_scale_dev=asc)
        host8 = Guarded(M, N, torch.uint8)
        C2m = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        gemm_q8(A8, B8, True, M, N, K, hip.EPI_BIAS_GELU, C2=C2m, bias=bias, dq=dq, dq_mul=1.0 / sa, q8=host8.t, q8_scale=s8)
        big, small = site(HUGE), site(1e-3)
        gemm_q8(A8, B8, True, M, N, K, hip.EPI_BIAS_GELU, C2=C2m, bias=bias, dq=dq, q8=host8.t, q8_scale=s8, q8_amax=big, a_scale_dev=asc)
        gemm_q8(A8, B8, True, M, N, K, hip.EPI_BIAS_GELU, C2=C2m, bias=bias, dq=dq, q8=host8.t, q8_scale=s8, q8_amax=small, a_scale_dev=asc)
    torch.cuda.synchronize()
    assert relerr(C.t, u) < 4e-3 and relerr(C2.t, a) < 4e-3
    act = C2.t.float()
    assert torch.equal(q8.t.view(F8).float(), _e4m3(act, s8).float())
    nclip = int((act.abs() * s8 > 448.0).sum())
    assert nclip >= 4 and int(sat) == 7 + nclip, (int(sat), nclip)
    amax = float(act.abs().max())
    ghost = torch.nn.functional.gelu(A8[M:].view(F8).double() / sa @ Bd.t() + bias.double())
    assert float(ghost.abs().max()) > 2 * amax                            # the rows beyond M would have shown in the site
    check_amax(s, amax, exact=False)
    assert torch.equal(lean8.t, q8.t) and float(s_lean.max()) == float(s.max()) and int(sat_lean) == nclip
    assert torch.equal(host8.t, q8.t)                                     # host scale == device scale ; dq_mul = 1 / sa == dq_div = sa (same bytes here)
    assert relerr(C2m, C2.t.double()) < 1e-6
    assert heads_only(big) and float(big.view(hip.AMAX_SLOTS, -1)[:, 0].min()) == HUGE
    assert heads_only(small) and float(small.max()) == float(s.max()) and float(small.view(hip.AMAX_SLOTS, -1)[:, 0].min()) >= 1e-3
    assert all(g.intact() for g in (C, C2, q8, lean8, host8))


# ---- dGELU dgrad on e4m3 operands: the e4m3 du (fc1 dgrad operand), its amax, the bias gradient -----------------------------------------------------
@pytest.mark.parametrize("M,N,K,hook", [(640, 1536, 384, None), (2048 + 40, 3072, 768, None), (4096, 1536, 384, None), (8192 + 64, 1536, 384, None),
                                        (8192, 1536, 384, None), (8192, 1536, 384, 390), (4096, 3072, 768, 351), (8192, 3072, 768, None)])
def test_dgelu_e4m3_q8(M, N, K, hook):
    """gemm8_bwd(EPI_DGELU, du8, gradient scales) (engine.hip:399): du (bf16) and the bias gradient against fp64 autograd of GELU; du8 bit-exact against
    the kernel's own du; amax within one bf16 rounding (taken before rounding); du left out = same bytes, same amax."""
    sy, sw, s8 = 20.0, 64.0, 24.0
    dY8, dYd = e4m3_operand(M, K, sy, seed=M + 5, std=0.5)
    W8, Wd = e4m3_operand(N, K, sw, seed=N + 6, std=0.25, pad_rows=0)
    Uf = rnd(M + 256, N, seed=7, scale=1.5)
    Uf[M:] = BIG
    U = Uf.bfloat16().contiguous()
    dq, dsc, s8d = torch.tensor([1.0 / sw], device=DEV), torch.tensor([sy], device=DEV), torch.tensor([s8], device=DEV)
    acc = dYd @ Wd.t()
    ur = U[:M].double().requires_grad_(True)
    torch.nn.functional.gelu(ur).backward(acc)
    du = ur.grad
    C, q8 = Guarded(M, N, torch.bfloat16), Guarded(M, N, torch.uint8)
    colsum = torch.full((N,), 0.25, device=DEV)
    s = site()
    with hooks(hook):
        gemm_q8(dY8, W8, True, M, N, K, hip.EPI_DGELU, C=C.t, U=U, colsum=colsum, dq=dq, q8=q8.t, q8_scale_dev=s8d, q8_amax=s, a_scale_dev=dsc)
        lean8, s_lean = Guarded(M, N, torch.uint8), site()
        gemm_q8(dY8, W8, True, M, N, K, hip.EPI_DGELU, U=U, dq=dq, q8=lean8.t, q8_scale_dev=s8d, q8_amax=s_lean, a_scale_dev=dsc)
    torch.cuda.synchronize()
    assert relerr(C.t, du) < 4e-3
    assert relerr(colsum - 0.25, du.sum(0)) < 4e-3
    dub = C.t.float()
    assert torch.equal(q8.t.view(F8).float(), _e4m3(dub, s8).float())
    check_amax(s, float(dub.abs().max()), exact=False)
    assert torch.equal(lean8.t, q8.t) and float(s_lean.max()) == float(s.max())
    assert all(g.intact() for g in (C, q8, lean8))


# ---- dGELU dgrad on bf16 operands with an amax post only: the recording step of the fp8 backward (engine.hip:404) --------------------------------------
@pytest.mark.parametrize("M,N,K,hook", [(640, 1536, 384, None), (2048 + 40, 1536, 384, None), (4096, 1536, 384, None), (8192 + 64, 1536, 384, None),
                                        (2048 + 40, 3072, 768, 306), (700, 1536, 384, 1), (2048 + 40, 1536, 384, 3),
                                        (2048 + 40, 3072, 768, None), (640, 1536, 384, 307), (700, 1536, 384, 4), (8192 + 64, 3072, 768, None),
                                        (8192, 1536, 384, None), (26624, 1536, 384, None), (8192, 1536, 384, 390)])
def test_dgelu_bf16_amax(M, N, K, hook):
    """The bf16 dGELU GEMM of the recording step posts max |du| into the du site (fcdef88: the 128x128 kernel never did, below 8192 rows at K = 384).
    du against fp64 autograd; the site within one bf16 rounding of max |du| (taken before rounding); rows beyond M never post."""
    A = rnd(M + 256, K, seed=M + 8, scale=0.5)
    A[M:] = BIG
    A = A.bfloat16().contiguous()
    B = rnd(N, K, seed=9, scale=0.05).bfloat16().contiguous()
    U = rnd(M + 256, N, seed=10, scale=1.5).bfloat16().contiguous()
    acc = A[:M].double() @ B.double().t()
    ur = U[:M].double().requires_grad_(True)
    torch.nn.functional.gelu(ur).backward(acc)
    C = Guarded(M, N, torch.bfloat16)
    colsum = torch.zeros(N, device=DEV)
    s = site(1e-6)
    with hooks(hook):
        gemm_q8(A, B, False, M, N, K, hip.EPI_DGELU, C=C.t, U=U, colsum=colsum, q8_amax=s)
    torch.cuda.synchronize()
    assert relerr(C.t, ur.grad) < 4e-3 and relerr(colsum, ur.grad.sum(0)) < 4e-3
    check_amax(s, float(C.t.float().abs().max()), exact=False)
    assert float(s.max()) < BIG
    assert C.intact()


# ---- EPI_RESID on e4m3 operands with the bf16 residual stream (xb16: fp8 inference / teacher passes, engine.hip:262,274) ---------------------------
@pytest.mark.parametrize("M,N,K,hook", [(700, 384, 384, None), (2048 + 40, 768, 3072, None), (4096, 384, 384, None), (8192 + 64, 384, 1536, None),
                                        (8192, 384, 384, None), (8192, 768, 3072, None), (26624, 384, 1536, None), (8192, 384, 1536, 390)])
def test_resid_bf16_stream(M, N, K, hook):
    """x_out = resid + row_scale (acc + bias) with the stream read and / or written as bf16: bf16 out == bf16(fp32-out run) and bf16 in == the fp32-in run on
    the same values upcast, bit for bit; in place (resid == C, how engine.hip runs it) == out of place; fp32 out within 5e-5, the rest 4e-3 of fp64."""
    sa, sb, rps = 8.0, 64.0, 256
    A8, Ad = e4m3_operand(M, K, sa, seed=M + 11)
    B8, Bd = e4m3_operand(N, K, sb, seed=N + 12, std=0.25, pad_rows=0)
    bias = rnd(N, seed=13)
    resid = rnd(M, N, seed=14) * 2 + 0.3
    R16 = resid.bfloat16().contiguous()
    scale = ((torch.arange((M + rps - 1) // rps, device=DEV) % 3).float() * 0.625 + 0.5).contiguous()
    dq, asc = torch.tensor([1.0 / sb], device=DEV), torch.tensor([sa], device=DEV)
    kw = dict(bias=bias, row_scale=scale, rps=rps, dq=dq, a_scale_dev=asc)
    x32, x32b = Guarded(M, N, torch.float32), Guarded(M, N, torch.float32)
    o16, io16, i16o16 = Guarded(M, N, torch.bfloat16), Guarded(M, N, torch.bfloat16), Guarded(M, N, torch.bfloat16)
    i16 = Guarded(M, N, torch.float32)
    with hooks(hook):
        gemm_q8(A8, B8, True, M, N, K, hip.EPI_RESID, C=x32.t, resid=resid, **kw)
        gemm_q8(A8, B8, True, M, N, K, hip.EPI_RESID, C=o16.t, resid=resid, out_bf16=1, **kw)
        r_up = R16.float().contiguous()
        gemm_q8(A8, B8, True, M, N, K, hip.EPI_RESID, C=x32b.t, resid=r_up, **kw)
        gemm_q8(A8, B8, True, M, N, K, hip.EPI_RESID, C=i16.t, resid=R16, resid_bf16=1, **kw)
        gemm_q8(A8, B8, True, M, N, K, hip.EPI_RESID, C=i16o16.t, resid=R16, resid_bf16=1, out_bf16=1, **kw)
        io16.t.copy_(R16)
        gemm_q8(A8, B8, True, M, N, K, hip.EPI_RESID, C=io16.t, resid=io16.t, resid_bf16=1, out_bf16=1, **kw)
    torch.cuda.synchronize()
    srow = scale.double().repeat_interleave(rps)[:M, None]
    want = resid.double() + srow * (Ad @ Bd.t() + bias.double())
    want16 = r_up.double() + srow * (Ad @ Bd.t() + bias.double())
    assert relerr(x32.t, want) < 5e-5 and relerr(x32b.t, want16) < 5e-5
    assert torch.equal(o16.t, x32.t.bfloat16())
    assert torch.equal(i16.t, x32b.t)
    assert torch.equal(i16o16.t, x32b.t.bfloat16())
    assert torch.equal(io16.t, i16o16.t)
    assert relerr(o16.t, want) < 4e-3 and relerr(i16.t, want) < 4e-3 and relerr(i16o16.t, want) < 4e-3
    assert all(g.intact() for g in (x32, x32b, o16, io16, i16o16, i16))


def test_gemm_q8_refuses_what_the_launcher_refuses():
    """The test entry point does not widen the launcher's contract: bf16 residual stream on bf16 operands, an e4m3 copy of a bf16-operand GELU / dGELU,
    ragged K on e4m3 operands and the row-wise epilogues are refused."""
    A = torch.zeros(256, 384, dtype=torch.bfloat16, device=DEV); B = torch.zeros(384, 384, dtype=torch.bfloat16, device=DEV)
    C = torch.zeros(256, 384, device=DEV); U = torch.zeros(256, 384, dtype=torch.bfloat16, device=DEV)
    q8 = torch.zeros(256, 384, dtype=torch.uint8, device=DEV); bias = torch.zeros(384, device=DEV)
    E = 1001
    gemm_q8(A, B, False, 256, 384, 384, hip.EPI_RESID, C=C, resid=C, bias=bias, out_bf16=1, rc=E)
    gemm_q8(A, B, False, 256, 384, 384, hip.EPI_BIAS_GELU, C2=C, bias=bias, q8=q8, q8_scale=1.0, rc=E)
    gemm_q8(A, B, False, 256, 384, 384, hip.EPI_DGELU, C=C, U=U, q8=q8, q8_scale=1.0, rc=E)
    gemm_q8(A, B, True, 256, 384, 384, hip.EPI_DGELU, U=U, rc=E)                                    # neither du nor its e4m3 copy
    gemm_q8(A, B, True, 256, 384, 352, hip.EPI_F32, C=C, rc=E)                                      # K % 64
    gemm_q8(A, B, True, 256, 384, 384, hip.EPI_LNBWD, C=C, rc=E)
    gemm_q8(A, B, True, 256, 384, 384, hip.EPI_PATCH, C=C, rc=E)
    gemm_q8(A, B, True, 256, 384, 384, hip.EPI_BF16, C=C, resid_bf16=1, rc=E)


# ---- dq_div: the device scale of the A operand the accumulators are divided by, on the plain e4m3 GEMMs --------------------------------------------------
@pytest.mark.parametrize("M,N,K,epi,hook", [(700, 1152, 384, hip.EPI_F32, None), (8192, 768, 3072, hip.EPI_F32, None), (8192, 1536, 384, hip.EPI_F32, 390),
                                            (2048 + 40, 1152, 384, hip.EPI_BF16, 2121), (4096, 384, 384, hip.EPI_BF16, 2121),
                                            (26624, 384, 1536, hip.EPI_BF16, None), (8192 + 64, 1152, 768, hip.EPI_BF16, None)])
def test_dq_div_matches_dq_mul(M, N, K, epi, hook):
    """Every gemm8 with running scales divides by *dq_div; the constant-scale form multiplies by dq_mul = 1 / scale: the same result within 1e-6 (one
    rounding of the scale), and against fp64 within the main-output bounds."""
    sa, sb = 12.0, 64.0
    A8, Ad = e4m3_operand(M, K, sa, seed=M + 15)
    B8, Bd = e4m3_operand(N, K, sb, seed=N + 16, std=0.25, pad_rows=0)
    dq, asc = torch.tensor([1.0 / sb], device=DEV), torch.tensor([sa], device=DEV)
    dt = torch.float32 if epi == hip.EPI_F32 else torch.bfloat16
    X, Y = Guarded(M, N, dt), Guarded(M, N, dt)
    with hooks(hook):
        gemm_q8(A8, B8, True, M, N, K, epi, C=X.t, dq=dq, a_scale_dev=asc)
        gemm_q8(A8, B8, True, M, N, K, epi, C=Y.t, dq=dq, dq_mul=1.0 / sa)
    torch.cuda.synchronize()
    ref = Ad @ Bd.t()
    assert relerr(X.t, ref) < (5e-5 if epi == hip.EPI_F32 else 4e-3)
    if epi == hip.EPI_F32:
        assert relerr(X.t, Y.t.double()) < 1e-6
    else:                                                                  # one fp32 rounding of the scale may move a bf16 rounding boundary: an ulp, rarely
        d = (X.t.float() - Y.t.float()).abs() / Y.t.float().abs().clamp_min(1e-30)
        assert float((X.t != Y.t).float().mean()) < 1e-3 and float(d.max()) <= 2.0 ** -7
    assert X.intact() and Y.intact()


# ---- LayerNorm forward with the e4m3 copy of its output (the qkv / fc1 operand), fp32 or bf16 (xb16) input -------------------------------------------
def ln_fwd_q8(x, bf16_in, gamma, beta, y, mean, rstd, M, C, y8, s8=0.0, s8_dev=None, amax=None, sat=None):
    hip.call("atst_layernorm_fwd_q8", hip.ptr(x), 1 if bf16_in else 0, hip.ptr(gamma), hip.ptr(beta), hip.ptr(y), hip.ptr(mean), hip.ptr(rstd), M, C,
             hip.ptr(y8), s8, hip.ptr(s8_dev), hip.ptr(amax), hip.ptr(sat), hip.stream())


@pytest.mark.parametrize("C", [384, 768])
@pytest.mark.parametrize("M,bf16_in", [(700, False), (2048 + 40, True), (4096, False), (8192 + 64, True), (26624, False)])
def test_layernorm_fwd_q8(M, C, bf16_in):
    """atst_ln_fwd / atst_ln_fwd_b16in with y8: y within 4e-3 of fp64 LayerNorm; y8 bit-exact against e4m3(y s) of the kernel's own y; amax EXACTLY
    max |y| (the kernel takes it from the bf16 values); clip count exact; y left out = same bytes; device scale == host scale; rows beyond M untouched."""
    s8 = 96.0
    x = rnd(M + 64, C, seed=M + C, scale=2.0) + 0.5
    x[M:] = 0.0
    x[M:, 0] = 1e4                                                         # rows beyond M: LayerNorm output gamma[0] sqrt(C - 1) = 59 / 83 at column 0
    if bf16_in:
        x = x.bfloat16().contiguous()
    gamma, beta = 1.5 + 0.5 * rnd(C, seed=17), 0.2 * rnd(C, seed=18)
    gamma[0] = 3.0
    y, y8, lean8, host8 = Guarded(M, C, torch.bfloat16), Guarded(M, C, torch.uint8), Guarded(M, C, torch.uint8), Guarded(M, C, torch.uint8)
    mean, rstd = Guarded(M, 1, torch.float32), Guarded(M, 1, torch.float32)
    s8d = torch.tensor([s8], device=DEV)
    s, sat = site(), counter(11)
    ln_fwd_q8(x, bf16_in, gamma, beta, y.t, mean.t, rstd.t, M, C, y8.t, s8_dev=s8d, amax=s, sat=sat)
    s_lean, sat_lean = site(), counter(0)
    ln_fwd_q8(x, bf16_in, gamma, beta, None, mean.t, rstd.t, M, C, lean8.t, s8_dev=s8d, amax=s_lean, sat=sat_lean)
    big, small = site(HUGE), site(1e-3)
    ln_fwd_q8(x, bf16_in, gamma, beta, None, mean.t, rstd.t, M, C, host8.t, s8=s8, amax=big)
    ln_fwd_q8(x, bf16_in, gamma, beta, None, mean.t, rstd.t, M, C, host8.t, s8=s8, amax=small)
    torch.cuda.synchronize()
    xd = x[:M].double()
    want = torch.nn.functional.layer_norm(xd, (C,), gamma.double(), beta.double(), 1e-6)
    assert relerr(y.t, want) < 4e-3
    assert relerr(mean.t.view(-1), xd.mean(1)) < 5e-5 and relerr(rstd.t.view(-1), torch.rsqrt(xd.var(1, unbiased=False) + 1e-6)) < 5e-5
    yb = y.t.float()
    assert torch.equal(y8.t.view(F8).float(), _e4m3(yb, s8).float())
    nclip = int((yb.abs() * s8 > 448.0).sum())
    assert nclip >= 4 and int(sat) == 11 + nclip, (int(sat), nclip)
    check_amax(s, float(yb.abs().max()), exact=True)
    assert float(s.max()) < 0.5 * 3.0 * (C - 1) ** 0.5                       # the rows beyond M were not read into it
    assert torch.equal(lean8.t, y8.t) and float(s_lean.max()) == float(s.max()) and int(sat_lean) == nclip
    assert torch.equal(host8.t, y8.t)
    assert heads_only(big) and float(big.view(hip.AMAX_SLOTS, -1)[:, 0].min()) == HUGE
    assert heads_only(small) and float(small.max()) == float(s.max())
    assert all(g.intact() for g in (y, y8, lean8, host8, mean, rstd))


# ---- LayerNorm backward with the e4m3 copy of g (the proj / fc2 dgrad operand) and its amax, g left out -----------------------------------------------
@pytest.mark.parametrize("C", [384, 768])
@pytest.mark.parametrize("M", [700, 2048 + 40, 8192 + 64])
def test_layernorm_bwd_q8(M, C):
    """atst_ln_bwd with g8 / g8_scale / g_amax: dx, dgamma, dbeta, the bias gradient against autograd; g == bf16(row_scale dx) and g8 == e4m3 of those
    bf16 values bit for bit; g_amax EXACTLY max |row_scale dx| of the kernel's own dx; g left out = same bytes, same amax."""
    rps, s8 = 32, 24.0
    dy = rnd(M, C, seed=M + 19).bfloat16().contiguous()
    x = rnd(M, C, seed=20) * 2 + 0.3
    gamma = 1 + 0.1 * rnd(C, seed=21)
    mean, rstd = x.mean(1).contiguous(), torch.rsqrt(x.var(1, unbiased=False) + 1e-6).contiguous()
    dres = rnd(M, C, seed=22)
    scale = ((torch.arange((M + rps - 1) // rps, device=DEV) % 3).float() * 0.625 + 0.25).contiguous()
    s8d = torch.tensor([s8], device=DEV)

    def run(with_g):
        dx, g, g8 = Guarded(M, C, torch.float32), Guarded(M, C, torch.bfloat16), Guarded(M, C, torch.uint8)
        dgamma, dbeta, dbu = (torch.full((C,), 0.125, device=DEV) for _ in range(3))
        s = site()
        hip.call("atst_layernorm_bwd_q8", hip.ptr(dy), hip.ptr(x), hip.ptr(mean), hip.ptr(rstd), hip.ptr(gamma), hip.ptr(dres), hip.ptr(dx.t),
                 hip.ptr(g.t) if with_g else None, hip.ptr(scale), rps, hip.ptr(dgamma), hip.ptr(dbeta), hip.ptr(dbu), M, C, hip.ptr(g8.t), hip.ptr(s8d),
                 hip.ptr(s), hip.stream())
        return dx, g, g8, dgamma, dbeta, dbu, s

    dx, g, g8, dgamma, dbeta, dbu, s = run(True)
    dx2, g_unused, g82, _, _, _, s2 = run(False)
    torch.cuda.synchronize()
    xr, gr = x.double().requires_grad_(True), gamma.double().requires_grad_(True)
    br = torch.zeros(C, dtype=torch.float64, device=DEV, requires_grad=True)
    torch.nn.functional.layer_norm(xr, (C,), gr, br, 1e-6).backward(dy.double())
    assert relerr(dx.t, dres.double() + xr.grad) < 5e-5
    assert relerr(dgamma - 0.125, gr.grad) < 5e-5 and relerr(dbeta - 0.125, br.grad) < 5e-5
    gs = dx.t * scale.repeat_interleave(rps)[:M, None]                     # of the kernel's own dx
    assert relerr(dbu - 0.125, gs.double().sum(0)) < 5e-5
    assert torch.equal(g.t, gs.bfloat16())
    assert torch.equal(g8.t.view(F8).float(), _e4m3(gs.bfloat16(), s8).float())
    check_amax(s, float(gs.abs().max()), exact=True)
    assert torch.equal(dx2.t, dx.t) and torch.equal(g82.t, g8.t) and float(s2.max()) == float(s.max())
    assert (g_unused.raw == SENT).all()                                    # g left out: not written
    assert all(t.intact() for t in (dx, g, g8, dx2, g82))


# ---- weight-shadow prep through the existing ABI (engine.py sync_shadows / _refresh_transposes, every step) ---------------------------------------------
def test_cast_bf16_rne():
    """atst_cast_bf16 (fp32 master -> bf16 shadow): torch's round-to-nearest-even bit for bit, including ties (low half 0x8000 on even and odd
    mantissas), values next to the bf16 maximum (rounding to it or overflowing to inf), subnormals, signed zeros and infinities."""
    g = torch.Generator().manual_seed(23)
    hi = torch.randint(0, 1 << 16, (40000,), generator=g, dtype=torch.int64)
    hi = torch.where(((hi >> 7) & 0xFF) == 0xFF, hi ^ (1 << 7), hi)       # no NaN patterns (their payload is not part of the contract)
    ties = (hi << 16) | 0x8000                                             # exact ties: even / odd bf16 mantissa
    near = (hi << 16) | torch.randint(0, 1 << 16, (40000,), generator=g)
    edge = torch.tensor([0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0x7F7E8000, 0xFF7F8000, 0xFF7F7FFF, 0x7F800000, 0xFF800000,
                         0x00000000, 0x80000000, 0x00000001, 0x00008000, 0x00018000, 0x807FFFFF, 0x00800000, 0x3F808000, 0x3F818000], dtype=torch.int64)
    bits = torch.cat([ties, near, edge, (torch.randn(20003, generator=g).view(torch.int32).to(torch.int64) & 0xFFFFFFFF)])
    x = torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32).view(torch.float32).to(DEV)
    y = torch.full((x.numel() + 64,), -1, dtype=torch.int16, device=DEV)
    hip.call("atst_cast_bf16", hip.ptr(x), x.numel(), hip.ptr(y), hip.stream())
    torch.cuda.synchronize()
    assert torch.equal(y[:x.numel()], x.to(torch.bfloat16).view(torch.int16))
    assert bool((y[x.numel():] == -1).all())


def test_transpose_bf16_batch_engine_table():
    """atst_transpose_bf16_batch on the engine's own table (every 2-D parameter of the flat buffer): p16t is p16 transposed per tensor, bit for bit."""
    from audiossl_amd.engine import AtstEngine
    eng = AtstEngine("small", depth=2, drop_path_rate=0.0)
    with torch.no_grad():
        eng.p32.copy_(torch.randn(eng.p32.numel(), generator=torch.Generator().manual_seed(24)).to(DEV))
    eng.sync_shadows(force=True)
    torch.cuda.synchronize()
    n2 = 0
    for name, (off, shape) in eng.layout.entries.items():
        if len(shape) == 2:
            r, c = shape
            src = eng.p16[off:off + r * c].view(r, c)
            assert torch.equal(eng.p16t[off:off + r * c].view(c, r), src.t()), name
            n2 += 1
    assert n2 >= 8 and torch.equal(eng.p16[:eng.p32.numel()], eng.p32.to(torch.bfloat16))


def test_transpose_bf16_batch_ragged_shapes_keep_gaps():
    """Shapes that are not multiples of 64 (last tiles partial in one or both dimensions), with gaps between the tensors: every tensor transposed bit
    for bit, the gaps and the tail of the destination untouched."""
    shapes = [(384, 1152), (100, 70), (65, 130), (1, 64), (63, 1), (129, 257), (1536, 384)]
    rows, off, tiles = [], 0, 0
    for r, c in shapes:
        off += 96                                                          # gap before every tensor
        rows.append((off, r, c, tiles))
        off += r * c
        tiles += -(-r // 64) * -(-c // 64)
    n = off + 200
    src = torch.randn(n, generator=torch.Generator().manual_seed(25)).to(DEV).bfloat16()
    dst = torch.full((n,), -7.0, dtype=torch.bfloat16, device=DEV)
    table = torch.tensor(rows, dtype=torch.int32, device=DEV).contiguous()
    hip.call("atst_transpose_bf16_batch", hip.ptr(src), hip.ptr(dst), hip.ptr(table), len(rows), tiles, hip.stream())
    torch.cuda.synchronize()
    touched = torch.zeros(n, dtype=torch.bool, device=DEV)
    for (o, r, c, _) in rows:
        assert torch.equal(dst[o:o + r * c].view(c, r), src[o:o + r * c].view(r, c).t()), (r, c)
        touched[o:o + r * c] = True
    assert bool((dst[~touched] == -7.0).all())


def test_quant_bf16_table_fp8():
    """atst_quant_bf16_table_fp8 (e4m3 copy of the transposed bf16 shadows, the dgrad B operands): e4m3(clamp(p16 (1 / dq))) per tensor.  The device
    takes 1 / dq with its own division: at most 1e-3 of the codes one step off (as test_gemm_fp8_vs_e4m3_emulation allows); gaps untouched; dq = 0
    gives zeros."""
    sizes, offs, off = [384 * 1152, 1536 * 384, 70 * 100, 4096], [], 0
    for n in sizes:
        off += 256
        offs.append(off)
        off += n
    total = off + 256
    p16 = (torch.randn(total, generator=torch.Generator().manual_seed(26)) * 0.05).to(DEV).bfloat16()
    dq = torch.tensor([float(p16[o:o + n].float().abs().max()) / 448.0 for o, n in zip(offs, sizes)], device=DEV)
    dq[3] = 0.0
    table = torch.tensor([[o, n] for o, n in zip(offs, sizes)], dtype=torch.int32, device=DEV).contiguous()
    p8 = torch.full((total,), SENT, dtype=torch.uint8, device=DEV)
    hip.call("atst_quant_bf16_table_fp8", hip.ptr(p16), hip.ptr(table), len(sizes), hip.ptr(dq), hip.ptr(p8), hip.stream())
    torch.cuda.synchronize()
    touched = torch.zeros(total, dtype=torch.bool, device=DEV)
    for t, (o, n) in enumerate(zip(offs, sizes)):
        got = p8[o:o + n]
        touched[o:o + n] = True
        if t == 3:
            assert int(got.view(F8).float().abs().max()) == 0
            continue
        want = _e4m3(p16[o:o + n], (1.0 / dq[t:t + 1]).float())
        gi, wi = got.int(), want.view(torch.uint8).int()
        mag = lambda c: torch.where(c >= 128, -(c - 128), c)               # sign-magnitude byte -> ordered integer
        diff = (mag(gi) - mag(wi)).abs()
        assert float((diff != 0).float().mean()) <= 1e-3 and int(diff.max()) <= 1, t
    assert bool((p8[~touched] == SENT).all())
