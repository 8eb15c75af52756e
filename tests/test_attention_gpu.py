"""Kernel-level tests of csrc/attention.hip: every launcher branch of atst_attn_fwd / atst_attn_bwd against an fp64 reference of the same operation,
per (sequence, head) pair, at H = 3, 6, 12, ragged `valid`, and the packed row layout of the short views (AttnArgs::stride, reached through the test
entry points atst_attention_fwd_rs / atst_attention_bwd_rs, which fill AttnArgs as csrc/engine.hip does).

Reference: fp64 attention on the SAME bf16 inputs, on the GPU, chunked over sequences -- q k^T * 0.125 + the reference's additive key mask
(-10000 on keys >= valid, audiossl/modules/transformer.py:152-159), softmax, * v ; lse = logsumexp of the masked logits ; fp64 autograd for the
backward with d_o zero on rows >= valid (as in the encoder).

Metrics, never pooled over pairs: per (sequence, head, tensor) the relative L2 error and the max-abs error relative to the pair's max |ref|.  Where a
pair's reference is exactly or nearly zero (dq, dk of a valid = 1 sequence: a one-key softmax has zero gradient) the denominators are floored at
FLOOR x the tensor's RMS pair norm / mean pair max, i.e. an absolute bound at the tensor's scale.  lse: absolute error of every query row, pad rows
included (the kernels write all NP rows).  Input regimes: plain randn ; peaky (q, k x4: near one-hot softmax, exercises the online / two-pass
rescaling) ; shifted (one vector added to every key of a head: the logits of a query shift by a constant of up to ~+-150, which softmax cannot see but a
missing max-subtraction overflows).

Branch (hook / argument; kernel as rocprofv3 names it)                     | tests
---------------------------------------------------------------------------+--------------------------------------------------------------------------
fwd NP=256  404 two-pass, default: attn_fwd256v2_kernel<0>                  | test_fwd_vs_fp64[fwd256v2-*], test_branches_agree, test_mask_exact,
            401 online softmax: attn_fwd256_kernel                          |   test_deterministic (all fwd branches) ; [fwd256_online-*], [fwd256_generic-*]
            400 per-(sequence, head): attn_fwd_kernel<256, 0>               |
            e4m3 copy: attn_fwd256v2_kernel<1> / <2>                        | test_fwd_vs_fp64[fwd256v2_m1|m2-*], test_q8_base, test_product_base512
fwd NP=128/64/32  attn_fwd_kernel<NP, 0>                                    | test_fwd_vs_fp64[fwd128|fwd64|fwd32-*], test_packed
fwd NP=32 e4m3  attn_fwd_kernel<32, 1> / <32, 2>                            | test_fwd_vs_fp64[fwd32_m1|m2-*], test_packed[32-26-*], test_q8_packed_np32
bwd NP=256  403 + dscratch, default: attn_rowdot_kernel + attn_bwd256_kernel<0> | test_bwd_vs_fp64[bwd256-*], test_branches_agree, test_mask_exact,
            403 + 406 row-per-lane dK/dV stores: attn_bwd256_kernel<0>      |   test_deterministic (all bwd branches) ; [bwd256_rowst-*]
            402 + dscratch / dscratch NULL: attn_bwd_dkv_kernel<256> + attn_bwd_dq_kernel<256> | [bwd256_generic_scr-*], [bwd256_generic-*]
            e4m3: attn_bwd256_kernel<2>                                     | test_q8_base, test_product_base512
bwd NP=32   409 fused, default: attn_bwd32_kernel<0> ; 408 two-kernel       | test_bwd_vs_fp64[bwd32-*], [bwd32_two-*], test_packed
            e4m3: attn_bwd32_kernel<2>                                      | test_q8_packed_np32, test_packed[32-26-*]
bwd NP=128/64  attn_bwd_dkv_kernel<NP> + attn_bwd_dq_kernel<NP>             | test_bwd_vs_fp64[bwd128|bwd64-*], test_packed
attn_rowdot_kernel grid cap (65536 blocks, S*H > 8192: grid-stride loop)    | test_product_rowdot_cap (S = 768, H = 12)
(launch counts per kernel: profiles/r07_attention_kernel_stats.txt)

Contract claims:
  * odd H (the NP = 256 head loops double-buffer on h & 1): H = 3 runs through every branch in tests 1-3 ;
  * inactive pairs (S*H not a multiple of Geo<NP>::G: 4 pairs per block at NP = 32, 2 at 64): S = 5 / 7 with H = 3 and 6 ;
  * the -10000 mask is exact (exp underflows to 0 in fp32 and fp64): test_mask_exact -- rows >= valid rewritten with large values change no bit of
    the outputs of rows < valid ;
  * packed rows (stride < NP: rows >= stride of a last tile read as zeros, never written): test_packed -- bit-identical to a padded run whose rows
    [stride, NP) are zero, NaN input tails never read, output tails keep their sentinel bytes ; test_packed_refusals ;
  * the e4m3 copies: codes bit-exact against the kernel's own bf16 output ; amax site == max |bf16| over LIVE rows exactly ; clip count exact:
    test_q8_base (NP = 256, H = 12), test_q8_packed_np32, and test_q8_absent_rows_excluded, an input on which the absent rows of a packed tile would
    dominate both the amax and the clip count ; refusals under hooks 410 / 412 / 402 / 408: test_q8_refusals ;
  * the *_rs entry points at stride 0 give the bits of the existing ones: test_rs_entry_points_match ;
  * every branch is deterministic (byte-identical relaunch; the clip counter is an integer atomic): test_deterministic.

Measured worst values of one MI355X run and the bounds derived from them: TOL below.  One finding, shared by every backward branch: the kernels round
P and dS to bf16 (MFMA operands), so dq / dk carry an error relative to the magnitude of their terms, not of the result.  Where the terms cancel --
valid = 2 (dq = dS_01 (k0 - k1)), near one-hot softmax, and above all keys with a common offset (sum_k dS = 0 removes it exactly in fp64, not after the
rounding of dS) -- the reference-relative error of a pair reaches 2.6 (dq, shifted).  The gradients are therefore bounded relative to their terms
(reference()'s dq_s / dk_s / dv_s), at 3-4e-4 measured.
"""
import contextlib
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from audiossl_amd import hip  # noqa: E402

DEV = "cuda"
F8 = torch.float8_e4m3fn
HD = 64
SENT = 0xA5                                      # sentinel byte of output rows that must not be written
DEFAULT_HOOKS = (404, 403, 407, 409, 411, 413)   # two-pass NP = 256 fwd, merged NP = 256 bwd, full-line dK/dV stores, fused NP = 32 bwd, e4m3 copies on
FLOOR = 0.05                                     # denominator floor of near-zero pairs, as a fraction of the tensor's typical pair (see pair_err)

# Bounds: about 2x the worst value measured on one MI355X run over every branch, H and regime (and the product sizes of tests 8), never above the global
# bounds of test_ops_gpu.py::test_attention (6e-3 for o, 1.5e-2 for the gradients).  rel: per-pair relative L2 ; max: per-pair max-abs relative ;
# lse: absolute ; steps: elementwise branch disagreement in units of 2^-8 max(|x|, pair scale) (about one bf16 step).  Gradients are measured against the
# magnitude of their terms (check_pairs); their reference-relative worst values, recorded for information: dq 2.8e-2 plain / 0.10 peaky / 2.6 shifted,
# dk 2.7e-2 / 0.10 / 5.0e-2, dv 3.7e-3 -- the worst pairs are the valid = 2 sequences and the shifted keys, on every branch alike (the bf16 rounding of
# dS that all of them share), so no branch falls short of a bound its siblings meet.
TOL = dict(
    o_rel=5e-3, o_max=1.1e-2,                  # measured 2.35e-3 (S = 768 product run ; 2.28e-3 in tests 1) / 5.4e-3
    lse=3e-5,                                  # measured 1.53e-5 (shifted: |lse| up to ~150 ; plain 1.1e-6)
    dq_rel=8e-4, dq_max=2e-3,                  # measured 3.7e-4 / 1.04e-3
    dk_rel=8e-4, dk_max=2e-3,                  # measured 3.6e-4 / 9.4e-4
    dv_rel=6e-3, dv_max=1.2e-2,                # measured 2.8e-3 / 5.7e-3
    steps_fwd=6.0, lse_agree=3e-5,             # measured 2.9 (online / per-pair NP = 256 forwards vs the two-pass one) / 1.53e-5
    steps_bwd=5.0,                             # measured 2.2 (generic NP = 256 backward vs the merged one ; row-per-lane stores, 408 vs 409: 0 / < 3e-3)
)

WORST = {}


def note(key, v):
    v = float(v)
    WORST[key] = v if math.isnan(v) else max(WORST.get(key, 0.0), v)
    return v


@pytest.fixture(scope="module", autouse=True)
def _lib():
    hip.load()
    yield
    torch.cuda.synchronize()
    _CASES.clear()
    print("\n[attention per-pair worst]\n" + "\n".join(f"  {k:48s} {v:.3e}" for k, v in sorted(WORST.items())))


@contextlib.contextmanager
def hooks(*hs):
    """Tuning hooks are process-global knobs read at launch time: set them for one launch, restore every default afterwards."""
    lib = hip.load()
    try:
        for h in hs:
            lib.atst_tune_gemm_variant(h)
        yield lib
    finally:
        for h in DEFAULT_HOOKS:
            lib.atst_tune_gemm_variant(h)


# name: (NP, hooks, mode) -- mode 0 bf16 o ; 1 bf16 o + e4m3 copy ; 2 e4m3 copy only
FWD = {
    "fwd256v2": (256, (404,), 0), "fwd256_online": (256, (401,), 0), "fwd256_generic": (256, (400,), 0),
    "fwd256v2_m1": (256, (), 1), "fwd256v2_m2": (256, (), 2),
    "fwd128": (128, (), 0), "fwd64": (64, (), 0),
    "fwd32": (32, (), 0), "fwd32_m1": (32, (), 1), "fwd32_m2": (32, (), 2),
}
# name: (NP, hooks, dscratch, e4m3)
BWD = {
    "bwd256": (256, (403,), True, False), "bwd256_rowst": (256, (403, 406), True, False), "bwd256_generic_scr": (256, (402,), True, False),
    "bwd256_generic": (256, (), False, False), "bwd256_q8": (256, (), True, True),
    "bwd128": (128, (), False, False), "bwd64": (64, (), False, False),
    "bwd32": (32, (409,), False, False), "bwd32_two": (32, (408,), False, False), "bwd32_q8": (32, (), False, True),
}
DEF_FWD = {256: "fwd256v2", 128: "fwd128", 64: "fwd64", 32: "fwd32"}
DEF_BWD = {256: "bwd256", 128: "bwd128", 64: "bwd64", 32: "bwd32"}
# valid sets: 1, 2, 31, 32, 33, NP - 1, NP (33 does not exist at NP = 32) ; S = 5 / 7 leave inactive pairs at NP = 32 (G = 4) and, with H = 3, NP = 64 (G = 2)
VALID = {256: [256, 1, 33, 255, 32, 2, 31, 129], 128: [128, 1, 33, 127, 32, 2, 31], 64: [64, 1, 33, 63, 32, 2, 31], 32: [32, 1, 31, 2, 26]}
REGIMES = ("plain", "peaky", "shifted")


def make_inputs(S, H, NP, regime, valid, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(S, NP, 3, H, HD, generator=g, device=DEV)
    if regime == "peaky":
        x[:, :, :2] *= 4.0
    elif regime == "shifted":                                        # q . c * 0.125 ~ N(0, 40^2): up to ~+-150 over the queries of a test
        x[:, :, 1] += torch.randn(H, HD, generator=g, device=DEV) * 40.0
    vt = torch.tensor(valid, dtype=torch.int32, device=DEV)
    live = (torch.arange(NP, device=DEV)[None, :] < vt[:, None]).reshape(S * NP, 1)
    d_o = (torch.randn(S * NP, H * HD, generator=g, device=DEV) * live).bfloat16()
    return x.reshape(S * NP, 3 * H * HD).bfloat16(), vt, d_o


def reference(qkv, vt, S, H, NP, d_o=None, s0=0, s1=None):
    """fp64 attention of sequences [s0, s1) of a padded [S*NP, 3C] bf16 qkv: o, lse (and dq, dk, dv with d_o) as [s, H, NP, 64] / [s, H, NP]."""
    s1 = S if s1 is None else s1
    x = qkv.view(S, NP, 3, H, HD)[s0:s1].double().permute(2, 0, 3, 1, 4)
    q, k, v = (t.detach().requires_grad_(d_o is not None) for t in x)
    mask = (torch.arange(NP, device=DEV)[None, :] >= vt[s0:s1, None]).double() * -10000.0
    with torch.enable_grad():
        att = q @ k.transpose(-1, -2) * 0.125 + mask[:, None, None, :]
        o = att.softmax(-1) @ v
        r = dict(o=o.detach(), lse=torch.logsumexp(att.detach(), -1))
        if d_o is not None:
            gr = d_o.view(S, NP, H, HD)[s0:s1].double().transpose(1, 2)
            r["dq"], r["dk"], r["dv"] = torch.autograd.grad(o, (q, k, v), gr)
    if d_o is not None:      # magnitudes of the summed terms: dS = P (dP - D) with dP = dO V^T, D = rowsum(dO O) -> |dS| <= P (|dO| |V|^T + rowsum |dO O|) ;
        p = att.detach().softmax(-1)                                 # dq: that |K| ; dk: that^T |Q| ; dv: P^T |dO|
        ga = gr.abs()
        ds = p * (ga @ v.detach().abs().transpose(-1, -2) + (ga * r["o"].abs()).sum(-1, keepdim=True)) * 0.125
        r["dq_s"], r["dk_s"], r["dv_s"] = ds @ k.detach().abs(), ds.transpose(-1, -2) @ q.detach().abs(), p.transpose(-1, -2) @ gr.abs()
    return r


def heads(t, S, RS, H, part=None, s0=0, s1=None):
    """[S*RS, C] (part None) or [S*RS, 3C] kernel tensor -> [s, H, RS, 64] view of sequences [s0, s1)."""
    s1 = S if s1 is None else s1
    if part is None:
        return t[: S * RS].view(S, RS, H, HD)[s0:s1].transpose(1, 2)
    return t[: S * RS].view(S, RS, 3, H, HD)[s0:s1, :, part].transpose(1, 2)


def buf(shape, dtype, fill):
    """output buffer pre-filled with NaN (fill None: bf16 / fp32 NaN, e4m3 code 0x7F) or with the byte `fill`"""
    if fill is None:
        return torch.full(shape, 0x7F, dtype=torch.uint8, device=DEV) if dtype == torch.uint8 else torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    n = shape[-1] * torch.empty(0, dtype=dtype).element_size()
    return torch.full((*shape[:-1], n), fill, dtype=torch.uint8, device=DEV).view(dtype)


def fwd(qkv, vt, S, H, NP, hk=(), mode=0, scale=1.0, stride=0, fill=None):
    R, C = qkv.shape[0], H * HD
    r = SimpleNamespace(o=buf((R, C), torch.bfloat16, fill) if mode != 2 else None, o8=None, site=None, sat=None,
                        lse=torch.full((S, H, NP), float("nan"), device=DEV))
    sc = None
    if mode:
        r.o8 = buf((R, C), torch.uint8, fill)
        r.site, r.sat = torch.zeros(hip.AMAX_SITE_STRIDE, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        sc = torch.tensor([scale], device=DEV)
    with hooks(*hk) as lib:
        rc = lib.atst_attention_fwd_rs(hip.ptr(qkv), hip.ptr(vt), hip.ptr(r.o), hip.ptr(r.o8), hip.ptr(sc), hip.ptr(r.site), hip.ptr(r.sat), hip.ptr(r.lse),
                                       S, H, NP, stride, hip.stream())
    hip.check(rc, "atst_attention_fwd_rs")
    return r


def bwd(qkv, vt, o, lse, d_o, S, H, NP, hk=(), scratch=False, q8=False, scale=1.0, stride=0, fill=None):
    R, C = qkv.shape[0], H * HD
    r = SimpleNamespace(dqkv=None, d8=None, site=None)
    sc = None
    if q8:
        r.d8, r.site, sc = buf((R, 3 * C), torch.uint8, fill), torch.zeros(hip.AMAX_SITE_STRIDE, device=DEV), torch.tensor([scale], device=DEV)
    else:
        r.dqkv = buf((R, 3 * C), torch.bfloat16, fill)
    dscr = torch.full((S, H, NP), float("nan"), device=DEV) if scratch else None
    with hooks(*hk) as lib:
        rc = lib.atst_attention_bwd_rs(hip.ptr(qkv), hip.ptr(vt), hip.ptr(o), hip.ptr(lse), hip.ptr(d_o), hip.ptr(r.dqkv), hip.ptr(r.d8), hip.ptr(sc),
                                       hip.ptr(r.site), hip.ptr(dscr), S, H, NP, stride, hip.stream())
    hip.check(rc, "atst_attention_bwd_rs")
    return r


def run_fwd(name, qkv, vt, S, H, **kw):
    NP, hk, mode = FWD[name]
    return fwd(qkv, vt, S, H, NP, hk=hk, mode=mode, **kw)


def run_bwd(name, qkv, vt, o, lse, d_o, S, H, **kw):
    NP, hk, scr, q8 = BWD[name]
    return bwd(qkv, vt, o, lse, d_o, S, H, NP, hk=hk, scratch=scr, q8=q8, **kw)


def pair_err(got, ref, scale=None):
    """per-pair (relative L2, max-abs relative) of [S, H, N, 64] tensors, relative to the reference -- or, with `scale`, to the magnitude of the
    terms the result is summed from.  A pair whose yardstick is (nearly) zero cannot be its own measure (dq, dk of a valid = 1 sequence are exactly 0
    in fp64 and ~1e-7 x |k| in fp32): both denominators are floored at FLOOR x the tensor's RMS pair norm / mean pair max -- for such a pair the test
    is an absolute bound at the scale of the tensor."""
    g, r = got.double().flatten(2), ref.double().flatten(2)
    m = r if scale is None else scale.double().flatten(2)
    d = g - r
    nr, mr = m.norm(dim=-1), m.abs().amax(-1)
    fn, fm = FLOOR * float(m.norm()) / math.sqrt(nr.numel()), FLOOR * float(mr.mean())
    return d.norm(dim=-1) / nr.clamp_min(fn), d.abs().amax(-1) / mr.clamp_min(fm)


def check_pairs(tag, name, got, ref, scale=None):
    """o: relative to the reference.  Gradients (scale = the magnitudes of their terms, from reference()): the kernels round P and dS to bf16 as MFMA
    operands, an error relative to the TERMS; where the terms cancel the reference-relative error grows without the kernel being wrong -- valid = 2
    (dq = dS_01 (k0 - k1)) and shifted keys (sum_k dS = 0 cancels the common key vector exactly in fp64, not after bf16 rounding of dS).  The
    reference-relative values are recorded as well (ref_rel), for the record."""
    rel, mx = pair_err(got, ref, scale)
    wr, wm = note(f"{tag}_rel {name}", rel.max()), note(f"{tag}_max {name}", mx.max())
    if scale is not None:
        note(f"{tag}_ref_rel {name}", pair_err(got, ref)[0].max())
    if not (wr < TOL[f"{tag}_rel"] and wm < TOL[f"{tag}_max"]):
        bad = torch.nonzero((rel >= TOL[f"{tag}_rel"]) | (mx >= TOL[f"{tag}_max"]) | rel.isnan())[:8].tolist()
        raise AssertionError(f"{tag} {name}: worst pair rel {wr:.3e} max {wm:.3e}; (sequence, head) pairs {bad}")


def check_lse(name, got, ref):
    err = (got.double() - ref).abs()
    w = note(f"lse {name}", err.max())
    assert w < TOL["lse"], (name, w, torch.nonzero((err >= TOL["lse"]) | err.isnan())[:8].tolist())


def steps(a, b, scale=None):
    """elementwise |a - b| in units of 2^-8 max(|b|, RMS of b's pair) (~ bf16 steps at the larger of the element and its pair's scale) ; gradients:
    2^-8 max(|b|, the magnitude of the element's terms) -- see check_pairs"""
    a, b = a.double().flatten(2), b.double().flatten(2)
    m = b if scale is None else scale.double().flatten(2)
    rms = m.pow(2).mean(-1, keepdim=True).sqrt().clamp_min(FLOOR * float(m.pow(2).mean().sqrt()))   # near-zero pairs: floored as in pair_err
    den = torch.maximum(b.abs(), rms) if scale is None else torch.maximum(b.abs(), torch.maximum(m, FLOOR * rms))
    return float(((a - b).abs() / (2.0 ** -8 * den)).max())


def e4m3(x, sc):
    """the values the kernels' e4m3 copies encode: e4m3(clamp(bf16 value * scale, +-448)), decoded (+0 / -0 are distinct codes of one value)"""
    return (x.float() * sc).clamp(-448.0, 448.0).to(F8).float()


def nclip(x, sc):
    return int(((x.float() * sc).abs() > 448.0).sum())


_CASES = {}


def case(NP, H, regime):
    """inputs + fp64 reference of one (NP, H, regime), shared by the tests that use them"""
    key = (NP, H, regime)
    if key not in _CASES:
        S = len(VALID[NP])
        qkv, vt, d_o = make_inputs(S, H, NP, regime, VALID[NP], seed=NP + H)
        _CASES[key] = (S, qkv, vt, d_o, reference(qkv, vt, S, H, NP, d_o))
    return _CASES[key]


HS = (3, 6, 12)


# ---------------------------------------------------------------------------------------------------------------------------- 1. forward vs fp64
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("name", list(FWD))
def test_fwd_vs_fp64(name, H, regime):
    NP, _, mode = FWD[name]
    S, qkv, vt, _, ref = case(NP, H, regime)
    r = run_fwd(name, qkv, vt, S, H)
    if mode != 2:
        check_pairs("o", f"{name} H{H} {regime}", heads(r.o, S, NP, H), ref["o"])
    check_lse(f"{name} H{H} {regime}", r.lse, ref["lse"])


# ---------------------------------------------------------------------------------------------------------------------------- 2. backward vs fp64
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("name", [n for n, b in BWD.items() if not b[3]])
def test_bwd_vs_fp64(name, H, regime):
    NP = BWD[name][0]
    S, qkv, vt, d_o, ref = case(NP, H, regime)
    f = run_fwd(DEF_FWD[NP], qkv, vt, S, H)
    r = run_bwd(name, qkv, vt, f.o, f.lse, d_o, S, H)
    for i, t in enumerate(("dq", "dk", "dv")):
        check_pairs(t, f"{name} H{H} {regime}", heads(r.dqkv, S, NP, H, i), ref[t], ref[t + "_s"])
    dead = (torch.arange(NP, device=DEV)[None, :] >= vt[:, None]).reshape(-1)      # keys >= valid: exactly zero dk and dv
    assert float(r.dqkv.view(S * NP, 3, -1)[dead][:, 1:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------- 3. branch agreement
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("NP", [256, 32])
def test_branches_agree(NP, H, regime):
    """every branch against the default on identical inputs, elementwise: same math, different summation order / softmax form"""
    S, qkv, vt, d_o, ref = case(NP, H, regime)
    f0 = run_fwd(DEF_FWD[NP], qkv, vt, S, H)
    for name in (n for n, b in FWD.items() if b[0] == NP and n != DEF_FWD[NP]):
        f = run_fwd(name, qkv, vt, S, H)
        if f.o is not None:
            st = note(f"steps_fwd {name}", steps(heads(f.o, S, NP, H), heads(f0.o, S, NP, H)))
            assert st < TOL["steps_fwd"], (name, st)
        d = note(f"lse_agree {name}", (f.lse - f0.lse).abs().max())
        assert d < TOL["lse_agree"], (name, d)
        if FWD[name][2] == 1:                                     # the e4m3 forwards run the bf16 arithmetic of the default unchanged
            assert torch.equal(f.o, f0.o) and torch.equal(f.lse, f0.lse), name
    b0 = run_bwd(DEF_BWD[NP], qkv, vt, f0.o, f0.lse, d_o, S, H)
    for name in (n for n, b in BWD.items() if b[0] == NP and n != DEF_BWD[NP] and not b[3]):
        b = run_bwd(name, qkv, vt, f0.o, f0.lse, d_o, S, H)
        for i, t in enumerate(("dq", "dk", "dv")):
            st = note(f"steps_bwd {t} {name}", steps(heads(b.dqkv, S, NP, H, i), heads(b0.dqkv, S, NP, H, i), ref[t + "_s"]))
            assert st < TOL["steps_bwd"], (name, t, st)


# ---------------------------------------------------------------------------------------------------------------------------- 4. mask exactness
@pytest.mark.parametrize("name", [n for n, b in BWD.items() if not b[3]])
def test_mask_exact(name):
    """Rows >= valid of q, k, v rewritten with values 12x larger (|q k| * 0.125 stays far below 10000, so the mask still wins in the reference):
    the outputs of rows < valid -- o, lse, dq, dk, dv -- do not change by one bit.  -10000 underflows exp to exactly 0 in fp32 as in fp64."""
    NP, H = BWD[name][0], 6
    S, qkv, vt, d_o, _ = case(NP, H, "plain")
    live = (torch.arange(NP, device=DEV)[None, :] < vt[:, None]).reshape(-1)
    g = torch.Generator(device=DEV).manual_seed(99)
    qkv2 = qkv.clone()
    qkv2[~live] = (torch.randn(int((~live).sum()), qkv.shape[1], generator=g, device=DEV) * 12.0).bfloat16()
    fwd_names = [DEF_FWD[NP]] + ([n for n, b in FWD.items() if b[0] == NP and n != DEF_FWD[NP] and b[2] != 2])
    rows = live.view(S, NP)
    for fname in fwd_names:
        a, b = run_fwd(fname, qkv, vt, S, H), run_fwd(fname, qkv2, vt, S, H)
        assert torch.equal(a.o[live], b.o[live]), fname
        assert torch.equal(a.lse.transpose(1, 2)[rows], b.lse.transpose(1, 2)[rows]), fname
    a, b = run_fwd(DEF_FWD[NP], qkv, vt, S, H), run_fwd(DEF_FWD[NP], qkv2, vt, S, H)
    da, db = run_bwd(name, qkv, vt, a.o, a.lse, d_o, S, H), run_bwd(name, qkv2, vt, b.o, b.lse, d_o, S, H)
    assert not da.dqkv[live].isnan().any() and torch.equal(da.dqkv[live], db.dqkv[live]), name


# ---------------------------------------------------------------------------------------------------------------------------- 5. packed layout
# (NP, stride): the engine's 1 s / 2 s / 4 s views (26 / 51 / 101 tokens with the CLS row), the ATST-Frame short crop of
# test_step_gpu.py::test_frame_short_crop_packed_vs_oracle (width 401: 100 tokens, no CLS, NP = 128), and a stride that is no token count
PACKED = [(32, 26), (64, 51), (128, 101), (128, 100), (64, 40)]


def pack(t, S, NP, stride, tail=float("nan")):
    """rows [0, stride) of every sequence of a padded tensor, followed by NP rows of `tail` (never to be read)"""
    v = t.view(S, NP, -1)[:, :stride].reshape(S * stride, -1)
    return torch.cat([v, torch.full((NP, t.shape[1]), tail, dtype=t.dtype, device=DEV)]).contiguous()


def packed_valid(S, stride):
    return ([stride, 1, 2, stride - 1, (stride + 1) // 2] * S)[:S]


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("NP,stride", PACKED)
def test_packed(NP, stride, S):
    """(a) packed == padded bit for bit (padded rows [stride, NP) zero: what stage_rows says the packed kernels see) for every row < stride of o,
    dqkv and the e4m3 codes, and for all NP rows of lse ; (b) the NaN rows past S * stride of qkv, o and d_o are never read: nothing comes out NaN ;
    (c) the rows past S * stride of every output keep their sentinel bytes (S = 1: rows [stride, NP) of a one-sequence buffer)."""
    H = 6
    vl = packed_valid(S, stride)
    qkv, vt, d_o = make_inputs(S, H, NP, "plain", vl, seed=stride)
    keep = (torch.arange(NP, device=DEV) < stride).repeat(S)[:, None]
    qkv = (qkv * keep).contiguous()                                 # padded layout of the same sequences
    qkv_p, d_o_p = pack(qkv, S, NP, stride), pack(d_o, S, NP, stride)
    n = S * stride

    def same(packed, padded):                                       # rows < stride of every sequence
        return torch.equal(packed[:n].view(S, stride, -1), padded.view(S, NP, -1)[:, :stride])

    def tail_kept(t):
        return bool((t[n:].contiguous().view(torch.uint8) == SENT).all())

    a0 = fwd(qkv, vt, S, H, NP)
    p0 = fwd(qkv_p, vt, S, H, NP, stride=stride, fill=SENT)
    assert torch.equal(p0.lse, a0.lse) and not p0.o[:n].isnan().any() and same(p0.o, a0.o) and tail_kept(p0.o)
    if NP == 32:                                                    # the e4m3 forwards, at a scale that clips the top half of the live range
        live = p0.o[:n]
        sc = 448.0 / (0.5 * float(live.float().abs().max()))
        for mode in (1, 2):
            a = fwd(qkv, vt, S, H, NP, mode=mode, scale=sc)
            p = fwd(qkv_p, vt, S, H, NP, mode=mode, scale=sc, stride=stride, fill=SENT)
            assert torch.equal(p.lse, a0.lse) and same(p.o8, a.o8) and tail_kept(p.o8), mode
            assert p.o is None or (same(p.o, a0.o) and tail_kept(p.o)), mode
            assert torch.equal(p.o8[:n].view(F8).float(), e4m3(live, sc)), mode
            assert float(p.site.max()) == float(live.float().abs().max()), mode                 # max over live rows only
            assert int(p.sat) == nclip(live, sc) > 0, mode
    o_p = p0.o.clone()
    o_p[n:] = float("nan")
    for name in [n_ for n_, b in BWD.items() if b[0] == NP and not b[3]]:
        a = run_bwd(name, qkv, vt, a0.o, a0.lse, d_o, S, H)
        p = run_bwd(name, qkv_p, vt, o_p, p0.lse, d_o_p, S, H, stride=stride, fill=SENT)
        assert not p.dqkv[:n].isnan().any() and same(p.dqkv, a.dqkv) and tail_kept(p.dqkv), name
    if NP == 32:
        b16 = run_bwd("bwd32", qkv_p, vt, o_p, p0.lse, d_o_p, S, H, stride=stride).dqkv[:n]
        sc = 448.0 / (0.5 * float(b16.float().abs().max()))
        a = run_bwd("bwd32_q8", qkv, vt, a0.o, a0.lse, d_o, S, H, scale=sc)
        p = run_bwd("bwd32_q8", qkv_p, vt, o_p, p0.lse, d_o_p, S, H, scale=sc, stride=stride, fill=SENT)
        assert same(p.d8, a.d8) and tail_kept(p.d8)
        assert torch.equal(p.d8[:n].view(F8).float(), e4m3(b16, sc))
        assert float(p.site.max()) == float(b16.float().abs().max())


def test_packed_refusals():
    """stride < 0, stride > NP and a packed NP = 256 are refused before any launch (buffers are sized for the largest stride tried anyway)"""
    lib = hip.load()
    H, S = 6, 2
    for NP, stride in ((32, -1), (32, 33), (64, 65), (128, 129), (256, 255), (256, 100), (256, 257)):
        R = S * (NP + 1) + NP
        qkv = torch.zeros(R, 3 * H * HD, dtype=torch.bfloat16, device=DEV)
        vt = torch.full((S,), 1, dtype=torch.int32, device=DEV)
        o, d_o, dqkv = torch.zeros(R, H * HD, dtype=torch.bfloat16, device=DEV), torch.zeros(R, H * HD, dtype=torch.bfloat16, device=DEV), torch.zeros_like(qkv)
        lse, scr = torch.zeros(S, H, NP, device=DEV), torch.zeros(S, H, NP, device=DEV)
        assert lib.atst_attention_fwd_rs(hip.ptr(qkv), hip.ptr(vt), hip.ptr(o), None, None, None, None, hip.ptr(lse), S, H, NP, stride, hip.stream()) != 0
        assert lib.atst_attention_bwd_rs(hip.ptr(qkv), hip.ptr(vt), hip.ptr(o), hip.ptr(lse), hip.ptr(d_o), hip.ptr(dqkv), None, None, None, hip.ptr(scr),
                                         S, H, NP, stride, hip.stream()) != 0
    # the backward writes exactly one of dqkv / dqkv8
    NP = 32
    qkv = torch.zeros(S * NP, 3 * H * HD, dtype=torch.bfloat16, device=DEV)
    o = torch.zeros(S * NP, H * HD, dtype=torch.bfloat16, device=DEV)
    vt, lse = torch.full((S,), 1, dtype=torch.int32, device=DEV), torch.zeros(S, H, NP, device=DEV)
    d8, sc, site = torch.zeros(S * NP, 3 * H * HD, dtype=torch.uint8, device=DEV), torch.ones(1, device=DEV), torch.zeros(hip.AMAX_SITE_STRIDE, device=DEV)
    for dq, dq8 in ((None, None), (qkv.clone(), d8)):
        assert lib.atst_attention_bwd_rs(hip.ptr(qkv), hip.ptr(vt), hip.ptr(o), hip.ptr(lse), hip.ptr(o), hip.ptr(dq), hip.ptr(dq8), hip.ptr(sc), hip.ptr(site),
                                         None, S, H, NP, 0, hip.stream()) == 1001
    torch.cuda.synchronize()
    assert not d8.any()


def test_rs_entry_points_match():
    """stride 0 through the *_rs entry points: the bits of atst_attention_fwd / _bwd / _fwd_fp8 / _bwd_fp8"""
    for NP in (256, 32):
        H = 6
        S, qkv, vt, d_o, _ = case(NP, H, "plain")
        C = H * HD
        o, lse = torch.empty(S * NP, C, dtype=torch.bfloat16, device=DEV), torch.empty(S, H, NP, device=DEV)
        hip.call("atst_attention_fwd", hip.ptr(qkv), hip.ptr(vt), hip.ptr(o), hip.ptr(lse), S, H, NP, hip.stream())
        r = fwd(qkv, vt, S, H, NP)
        assert torch.equal(r.o, o) and torch.equal(r.lse, lse), NP
        sc = torch.tensor([300.0], device=DEV)                      # clips some elements
        o8, site, sat = torch.empty(S * NP, C, dtype=torch.uint8, device=DEV), torch.zeros(hip.AMAX_SITE_STRIDE, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        hip.call("atst_attention_fwd_fp8", hip.ptr(qkv), hip.ptr(vt), hip.ptr(o), hip.ptr(o8), hip.ptr(sc), hip.ptr(site), hip.ptr(sat), hip.ptr(lse), S, H, NP, hip.stream())
        r = fwd(qkv, vt, S, H, NP, mode=1, scale=300.0)
        assert torch.equal(r.o8, o8) and torch.equal(r.site, site) and int(r.sat) == int(sat) > 0, NP
        scr = torch.empty(S, H, NP, device=DEV)
        dqkv = torch.empty_like(qkv)
        hip.call("atst_attention_bwd", hip.ptr(qkv), hip.ptr(vt), hip.ptr(o), hip.ptr(lse), hip.ptr(d_o), hip.ptr(dqkv), hip.ptr(scr), S, H, NP, hip.stream())
        r = bwd(qkv, vt, o, lse, d_o, S, H, NP, scratch=True)
        assert torch.equal(r.dqkv, dqkv), NP
        d8, site = torch.empty(S * NP, 3 * C, dtype=torch.uint8, device=DEV), torch.zeros(hip.AMAX_SITE_STRIDE, device=DEV)
        hip.call("atst_attention_bwd_fp8", hip.ptr(qkv), hip.ptr(vt), hip.ptr(o), hip.ptr(lse), hip.ptr(d_o), hip.ptr(d8), hip.ptr(sc), hip.ptr(site), hip.ptr(scr),
                 S, H, NP, hip.stream())
        r = bwd(qkv, vt, o, lse, d_o, S, H, NP, scratch=True, q8=True, scale=300.0)
        assert torch.equal(r.d8, d8) and torch.equal(r.site, site), NP


# ---------------------------------------------------------------------------------------------------------------------------- 6. e4m3 side outputs
def check_fwd_q8(qkv, vt, S, H, NP, stride=0):
    """MODE 1 / 2 against the kernel's own bf16 output at a scale that clips nothing and one that clips: codes bit-exact, amax over live rows exact,
    clip count exact ; MODE 1's bf16 output and lse are those of the bf16 forward"""
    n = S * (stride or NP)
    f0 = fwd(qkv, vt, S, H, NP, stride=stride)
    live = f0.o[:n].float()
    amax = float(live.abs().max())
    for sc in (448.0 / (1.5 * amax), 448.0 / (0.25 * amax)):
        m1 = fwd(qkv, vt, S, H, NP, mode=1, scale=sc, stride=stride)
        m2 = fwd(qkv, vt, S, H, NP, mode=2, scale=sc, stride=stride)
        assert torch.equal(m1.o[:n], f0.o[:n]) and torch.equal(m1.lse, f0.lse) and torch.equal(m2.lse, f0.lse)
        assert torch.equal(m1.o8[:n].view(F8).float(), e4m3(live, sc)) and torch.equal(m2.o8[:n], m1.o8[:n])
        for m in (m1, m2):
            assert float(m.site.max()) == amax and int(m.sat) == nclip(live, sc)
    return f0


def check_bwd_q8(qkv, vt, f0, d_o, S, H, NP, bname, b8name, stride=0):
    n = S * (stride or NP)
    b16 = run_bwd(bname, qkv, vt, f0.o, f0.lse, d_o, S, H, stride=stride).dqkv[:n]
    amax = float(b16.float().abs().max())
    for sc in (448.0 / (1.5 * amax), 448.0 / (0.25 * amax)):
        r = run_bwd(b8name, qkv, vt, f0.o, f0.lse, d_o, S, H, scale=sc, stride=stride)
        assert torch.equal(r.d8[:n].view(F8).float(), e4m3(b16, sc))
        assert float(r.site.max()) == amax


@pytest.mark.parametrize("regime", REGIMES)
def test_q8_base(regime):
    """ATST-base geometry: NP = 256, H = 12 -- attn_fwd256v2_kernel<1> / <2>, attn_bwd256_kernel<2>"""
    S, qkv, vt, d_o, _ = case(256, 12, regime)
    f0 = check_fwd_q8(qkv, vt, S, 12, 256)
    check_bwd_q8(qkv, vt, f0, d_o, S, 12, 256, "bwd256", "bwd256_q8")


@pytest.mark.parametrize("S", [1, 5])
def test_q8_packed_np32(S):
    """the 1 s local views: packed NP = 32 (stride 26) -- attn_fwd_kernel<32, 1> / <32, 2>, attn_bwd32_kernel<2>, amax / clips over live rows"""
    NP, stride, H = 32, 26, 6
    vl = packed_valid(S, stride)
    qkv, vt, d_o = make_inputs(S, H, NP, "plain", vl, seed=7)
    qkv_p, d_o_p = pack(qkv, S, NP, stride), pack(d_o, S, NP, stride)
    f0 = check_fwd_q8(qkv_p, vt, S, H, NP, stride=stride)
    o_p = f0.o.clone()
    o_p[S * stride:] = float("nan")
    f0.o = o_p
    check_bwd_q8(qkv_p, vt, f0, d_o_p, S, H, NP, "bwd32", "bwd32_q8", stride=stride)


def test_q8_absent_rows_excluded():
    """Packed NP = 32, valid = 2: key 0 carries V = 200, every live query row (all rows < stride) is steered away from it (q . k0 * 0.125 = -8), so live
    outputs stay ~N(0, 1).  The absent rows [stride, 32) of a tile are zero queries: they average keys 0 and 1 (~100) and would dominate the amax and
    every clip -- the padded run, where those rows are real, shows it.  The packed kernels must exclude them from both."""
    NP, stride, H, S = 32, 26, 6, 5
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(S, NP, 3, H, HD, generator=g, device=DEV)
    x[:, :, 0] = -1.0 + 0.05 * x[:, :, 0]                           # q of every row ~ -u
    x[:, 0, 1] = 1.0                                                # k0 = u: q . k0 * 0.125 ~ -8
    x[:, 1:, 1] *= 0.1
    x[:, 0, 2] = 200.0                                              # V of key 0
    x[:, stride:] = 0.0                                             # padded twin: absent rows are zero
    qkv = x.reshape(S * NP, -1).bfloat16()
    vt = torch.full((S,), 2, dtype=torch.int32, device=DEV)
    qkv_p = pack(qkv, S, NP, stride)
    p0 = fwd(qkv_p, vt, S, H, NP, stride=stride)
    live = p0.o[: S * stride].float()
    amax = float(live.abs().max())
    sc = 448.0 / (2.0 * amax)                                        # nothing live clips
    pad = fwd(qkv, vt, S, H, NP, mode=1, scale=sc)
    assert float(pad.site.max()) > 10.0 * amax and int(pad.sat) > 0   # the absent rows would dominate
    for mode in (1, 2):
        p = fwd(qkv_p, vt, S, H, NP, mode=mode, scale=sc, stride=stride)
        assert float(p.site.max()) == amax and int(p.sat) == 0, mode
        assert torch.equal(p.o8[: S * stride].view(F8).float(), e4m3(live, sc)), mode


def test_q8_refusals():
    """the e4m3 outputs exist only where atst_attention_fp8_ok says so: refused under hooks 410 (fp8 forward quantised by a separate pass), 412 (NP = 32
    kernels out of the e4m3 step), 402 (generic NP = 256 backward), 408 (two-kernel NP = 32 backward) -- before any launch"""
    lib = hip.load()
    H, S = 6, 2
    assert all(lib.atst_attention_fp8_ok(NP, H, b) == 1 for NP in (256, 32) for b in (0, 1))
    refused = {410: [(256, 0), (32, 0)], 412: [(32, 0), (32, 1)], 402: [(256, 1)], 408: [(32, 1)]}
    for hook, cases_ in refused.items():
        for NP, b in cases_:
            R = S * NP
            qkv = torch.zeros(R, 3 * H * HD, dtype=torch.bfloat16, device=DEV)
            vt = torch.full((S,), NP, dtype=torch.int32, device=DEV)
            o = torch.zeros(R, H * HD, dtype=torch.bfloat16, device=DEV)
            q8 = torch.full((R, 3 * H * HD), SENT, dtype=torch.uint8, device=DEV)
            lse, scr = torch.zeros(S, H, NP, device=DEV), torch.zeros(S, H, NP, device=DEV)
            sc, site = torch.ones(1, device=DEV), torch.zeros(hip.AMAX_SITE_STRIDE, device=DEV)
            with hooks(hook) as lib_:
                assert lib_.atst_attention_fp8_ok(NP, H, b) == 0, (hook, NP, b)
                if b:
                    rc = lib_.atst_attention_bwd_rs(hip.ptr(qkv), hip.ptr(vt), hip.ptr(o), hip.ptr(lse), hip.ptr(o), None, hip.ptr(q8), hip.ptr(sc), hip.ptr(site),
                                                    hip.ptr(scr), S, H, NP, 0, hip.stream())
                else:
                    rc = lib_.atst_attention_fwd_rs(hip.ptr(qkv), hip.ptr(vt), hip.ptr(o), hip.ptr(q8), hip.ptr(sc), hip.ptr(site), None, hip.ptr(lse),
                                                    S, H, NP, 0, hip.stream())
            torch.cuda.synchronize()
            assert rc == 1001 and bool((q8 == SENT).all()), (hook, NP, b)


# ---------------------------------------------------------------------------------------------------------------------------- 7. determinism
def _bytes(*ts):
    return [t.contiguous().view(torch.uint8).clone() if t is not None else None for t in ts]


@pytest.mark.parametrize("NP", [256, 128, 64, 32])
def test_deterministic(NP):
    """two identical launches of every branch write identical bytes (lse, codes, amax, clip count included)"""
    H = 12
    S, qkv, vt, d_o, _ = case(NP, H, "plain")
    for name in (n for n, b in FWD.items() if b[0] == NP):
        a, b = (run_fwd(name, qkv, vt, S, H, scale=4.0) for _ in range(2))
        for x, y in zip(_bytes(a.o, a.o8, a.lse, a.site, a.sat), _bytes(b.o, b.o8, b.lse, b.site, b.sat)):
            assert (x is None and y is None) or torch.equal(x, y), name
    f = run_fwd(DEF_FWD[NP], qkv, vt, S, H)
    for name in (n for n, b in BWD.items() if b[0] == NP):
        a, b = (run_bwd(name, qkv, vt, f.o, f.lse, d_o, S, H, scale=64.0) for _ in range(2))
        for x, y in zip(_bytes(a.dqkv, a.d8, a.site), _bytes(b.dqkv, b.d8, b.site)):
            assert (x is None and y is None) or torch.equal(x, y), name


# ---------------------------------------------------------------------------------------------------------------------------- 8. product sizes
def chunked_check(tag, qkv, vt, d_o, S, H, NP, o, lse, dqkv, RS=None, chunk=16):
    """per-pair statistics against fp64 over chunks of sequences (the padded twin qkv / d_o ; kernel outputs with RS rows per sequence)"""
    RS = RS or NP
    for s0 in range(0, S, chunk):
        s1 = min(S, s0 + chunk)
        ref = reference(qkv, vt, S, H, NP, d_o, s0, s1)
        check_pairs("o", tag, heads(o, S, RS, H, None, s0, s1), ref["o"][:, :, :RS])
        check_lse(tag, lse[s0:s1], ref["lse"])
        for i, t in enumerate(("dq", "dk", "dv")):
            check_pairs(t, tag, heads(dqkv, S, RS, H, i, s0, s1), ref[t][:, :, :RS], ref[t + "_s"][:, :, :RS])


def product_valid(S, full, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.full((S,), full, dtype=torch.int32)
    ragged = torch.rand(S, generator=g) < 0.25
    v[ragged] = torch.randint(1, full + 1, (int(ragged.sum()),), generator=g, dtype=torch.int32)
    v[:3] = torch.tensor([1, 2, full], dtype=torch.int32)
    return v.tolist()


def test_product_clip6_local():
    """the clip6 local views: S = 1024 packed sequences of 26 tokens in NP = 32 tiles, H = 6 (default branches)"""
    S, NP, H, stride = 1024, 32, 6, 26
    vl = product_valid(S, stride, 3)
    qkv, vt, d_o = make_inputs(S, H, NP, "plain", vl, seed=11)
    qkv = (qkv * (torch.arange(NP, device=DEV) < stride).repeat(S)[:, None]).contiguous()
    qkv_p, d_o_p = pack(qkv, S, NP, stride), pack(d_o, S, NP, stride)
    f = fwd(qkv_p, vt, S, H, NP, stride=stride)
    b = bwd(qkv_p, vt, f.o, f.lse, d_o_p, S, H, NP, stride=stride)
    chunked_check("clip6 local S1024", qkv, vt, d_o, S, H, NP, f.o, f.lse, b.dqkv, RS=stride, chunk=256)


def test_product_base512():
    """ATST-base: S = 512, NP = 256, H = 12 -- bf16 forward / backward against fp64, and the e4m3 forward / backward against their own bf16 runs"""
    S, NP, H = 512, 256, 12
    vl = product_valid(S, 251, 4)
    qkv, vt, d_o = make_inputs(S, H, NP, "plain", vl, seed=12)
    f = fwd(qkv, vt, S, H, NP)
    b = bwd(qkv, vt, f.o, f.lse, d_o, S, H, NP, scratch=True)
    chunked_check("base S512", qkv, vt, d_o, S, H, NP, f.o, f.lse, b.dqkv)
    amax = float(f.o.float().abs().max())
    sc = 448.0 / (0.5 * amax)
    m1 = fwd(qkv, vt, S, H, NP, mode=1, scale=sc)
    assert torch.equal(m1.o, f.o) and torch.equal(m1.o8.view(F8).float(), e4m3(f.o, sc))
    assert float(m1.site.max()) == amax and int(m1.sat) == nclip(f.o, sc) > 0
    gmax = float(b.dqkv.float().abs().max())
    sc = 448.0 / (1.5 * gmax)
    b8 = bwd(qkv, vt, f.o, f.lse, d_o, S, H, NP, scratch=True, q8=True, scale=sc)
    assert torch.equal(b8.d8.view(F8).float(), e4m3(b.dqkv, sc)) and float(b8.site.max()) == gmax


def test_product_rowdot_cap():
    """S = 768, NP = 256, H = 12: S * H = 9216 > 8192, so attn_rowdot_kernel runs at its 65536-block cap and its grid-stride loop takes a second pass"""
    S, NP, H = 768, 256, 12
    vl = product_valid(S, 251, 5)
    qkv, vt, d_o = make_inputs(S, H, NP, "plain", vl, seed=13)
    f = fwd(qkv, vt, S, H, NP)
    b = bwd(qkv, vt, f.o, f.lse, d_o, S, H, NP, scratch=True)
    chunked_check("rowdot cap S768", qkv, vt, d_o, S, H, NP, f.o, f.lse, b.dqkv)
