"""Fine-tuning through the encoder's inference API (downstream/train_finetune.py): the teacher encoder's get_intermediate_layers_chunks /
get_intermediate_layers / forward are differentiable when grad is on and its parameters require grad.  Against fp64 torch on random taps
(tap kernels), the reference golden (clip_finetune.npz), the oracle with DropPath, and a plain-torch FineTuningPLModule loop."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import finetune_ref as FR  # noqa: E402
from audiossl_amd import hip  # noqa: E402
from audiossl_amd.models.atst.atst import ATST  # noqa: E402
from audiossl_amd.models.atst.audio_transformer import AST_small  # noqa: E402
from oracle import atst_oracle as O  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
# sums over the batch of per-clip terms that cancel behind the head's BatchNorm (its input gradient sums to zero over the batch per feature)
CANCELLING = ("pos_embed", "norm.bias", "norm.weight")


def sample_idx(n, k=192):
    return np.unique(np.linspace(0, n - 1, num=min(n, k)).astype(np.int64))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def teacher_encoder(seed, depth=None, **kw):
    model = ATST("small", depth=depth, **kw)
    model.engine.load_weights(O.recipe_weights("small", depth=depth, seed=seed))
    enc = model.teacher.encoder
    enc._owner = [model]
    return enc


def test_finetune_gradients_reach_the_encoder():
    enc = teacher_encoder(43)
    enc.requires_grad_(True)
    enc.eval()
    x = O.recipe_mel(3, 1201, seed=41).cuda()
    feats = enc.get_intermediate_layers_chunks(x, torch.tensor([1201, 900, 500]), 12, 601, True)
    assert feats.shape == (3, 2 * 12 * 384) and feats.grad_fn is not None
    head = FR.LinearHead(feats.shape[1], 3).cuda()
    F.cross_entropy(head(feats), torch.tensor([0, 1, 2], device="cuda")).backward()
    for name, p in enc.named_parameters():
        if name == "mask_embed":
            assert p.grad is None
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert float(enc.blocks[0].attn.qkv.weight.grad.norm()) > 0


def test_finetune_vs_reference_golden():
    """Features against the reference's; encoder gradients from the reference head's gradient at the reference features.  The head's
    BatchNorm runs on a batch of 3: measured on the CPU, a 5e-3 relative error in the features (bf16 encoder: 4.8e-3) moves d(loss)/d(features)
    by 0.28, so the HIP head gradient on HIP features would pin that amplification, not the encoder backward (see smoke(): oracle heads on HIP's
    own features).  The loss of the reference head on HIP's features is checked against the golden loss."""
    G = np.load(os.path.join(GOLD, "clip_finetune.npz"))
    enc = teacher_encoder(int(G["weight_seed"]))
    enc.requires_grad_(True)
    enc.eval()
    x = O.recipe_mel(3, 1201, seed=int(G["mel_seed"])).cuda()
    feats = enc.get_intermediate_layers_chunks(x, torch.from_numpy(G["length"]), 12, 601, True)
    fr = rel(feats.detach().cpu().numpy(), G["feats"])
    head = FR.LinearHead(feats.shape[1], 3).double()
    with torch.no_grad():
        head.linear.weight.copy_(torch.from_numpy(G["head_w"]))
        head.linear.bias.copy_(torch.from_numpy(G["head_b"]))
    labels = torch.from_numpy(G["labels"])
    with torch.no_grad():
        loss_hip = float(F.cross_entropy(head(feats.detach().double().cpu()), labels))
    f_ref = torch.from_numpy(G["feats"]).double().requires_grad_(True)
    F.cross_entropy(head(f_ref), labels).backward()
    feats.backward(f_ref.grad.float().cuda())
    tab = {}
    for name, p in enc.named_parameters():
        if "gnone/" + name in G:
            assert p.grad is None, name
            continue
        g = p.grad.reshape(-1).double().cpu()
        tab[name] = (rel(g[sample_idx(g.numel())].numpy(), G["gsamp/" + name]), g.numel())
    assert len(tab) == 138
    kept = {k: v for k, v in tab.items() if k not in CANCELLING}
    mean = sum(r * n for r, n in kept.values()) / sum(n for _, n in kept.values())
    worst = max(kept.items(), key=lambda kv: kv[1][0])
    print("\n[finetune vs reference] cancelling sums " + ", ".join(f"{k} {tab[k][0]:.2e}" for k in CANCELLING))
    print(f"[finetune vs reference] features {fr:.3e}; loss {loss_hip:.5f} vs {float(G['loss']):.5f}; grad weighted mean {mean:.3e}; "
          f"worst {worst[0]} {worst[1][0]:.3e}")
    assert fr < 1e-2                                    # measured 4.8e-3 ; loss 1.26294 vs 1.26373
    assert abs(loss_hip - float(G["loss"])) < 5e-2 * max(1.0, float(G["loss"]))
    assert mean < 1e-2 and worst[1][0] < 2.4e-2        # measured 6.2e-3 / 1.22e-2 (blocks.9.norm1.bias)


@pytest.mark.parametrize("n", [1, 3])
def test_finetune_droppath_vs_oracle(n):
    """Train mode, depth 3, injected DropPath draws; autograd through the oracle's encoder + the restated taps and pooling."""
    D, S = 3, 3
    W = O.recipe_weights("small", depth=D, seed=51)
    enc = teacher_encoder(51, depth=D)
    enc.requires_grad_(True)
    enc.train()
    x = O.recipe_mel(S, 1201, seed=53)
    length = torch.tensor([1201, 1000, 420])
    rng = np.random.default_rng(55)
    keep = [torch.from_numpy((rng.random((D, 2, S)) > 0.3).astype(np.float32)) for _ in range(2)]
    enc._keep = keep
    try:
        feats = enc.get_intermediate_layers_chunks(x.cuda(), length, n, 601, True)
    finally:
        enc._keep = None
    R = torch.from_numpy(rng.standard_normal(tuple(feats.shape)).astype(np.float32))
    (feats * R.cuda()).sum().backward()
    pre = "teacher.encoder."
    leaves = {k: v.clone().requires_grad_(True) for k, v in W.items() if k.startswith(pre) and v.dtype == torch.float32}
    ref = FR.chunk_features(leaves, pre, x, length, n, depth=D, keep=keep)
    (ref * R).sum().backward()
    fr = rel(feats.detach().cpu().numpy(), ref.detach().numpy())
    tab = {}
    for k, v in leaves.items():
        name = k[len(pre):]
        p = dict(enc.named_parameters())[name]
        if v.grad is None:
            assert p.grad is None, name
            continue
        tab[name] = (rel(p.grad.reshape(-1).cpu().numpy(), v.grad.reshape(-1).numpy()), v.numel())
    mean = sum(r * m for r, m in tab.values()) / sum(m for _, m in tab.values())
    worst = max(tab.items(), key=lambda kv: kv[1][0])
    print(f"\n[finetune droppath n={n}] features {fr:.3e}; grad weighted mean {mean:.3e}; worst {worst[0]} {worst[1][0]:.3e}")
    assert fr < 1e-2                                    # measured 4.4e-3 (n 1) / 4.0e-3 (n 3)
    assert mean < 1e-2 and worst[1][0] < 2.4e-2        # measured 4.9e-3 / 5.7e-3 (n 1), 4.7e-3 / 5.5e-3 (n 3)


def _tap_pass(enc, S, width, length):
    """A teacher training pass of `enc` with random fp32 taps written into its tape; -> (pass, plen, taps [D, S*RS, C] fp64)."""
    eng = enc._eng[0]
    ep = eng._pass("teacher", S, width, True, ("tap-test", width))
    plen = (length - length % 4) // 4
    ep.forward(O.recipe_mel(S, width, seed=61).cuda(), (torch.clamp(plen, max=ep.n_tok) + 1).to(torch.int32), None, None)
    g = torch.Generator(device="cuda").manual_seed(63)
    taps = []
    for i in range(eng.depth):
        t = ep.block_out(i)
        t.copy_(torch.randn(t.shape, generator=g, device="cuda") * 2.0 + 0.5)
        taps.append(t.double().cpu())
    return ep, plen, torch.stack(taps)


def _ln64(x, enc):
    return F.layer_norm(x, (x.shape[-1],), enc.norm.weight.detach().double().cpu(), enc.norm.bias.detach().double().cpu(), 1e-6)


@pytest.mark.parametrize("n,avgpool", [(1, False), (3, True), (12, True), (12, False)])
def test_tap_kernels_vs_fp64(n, avgpool):
    """Pooled tap forward (accumulated over two calls with their chunk weights, one zero) and the tap backward's final-norm and top fc2.bias
    gradients, on random taps: pad rows, patch_length > n_tok (1201 frames in a 601-frame pass), a zero-weight sequence."""
    enc = teacher_encoder(57)
    eng, C, S, width = enc._eng[0], 384, 3, 601
    length = torch.tensor([1201, 300, 77])                   # plen 300 > n_tok 150 ; 75 ; 19
    ep, plen, taps = _tap_pass(enc, S, width, length)
    RS, D = ep.RS, eng.depth
    ldf = (2 if avgpool else 1) * n * C
    w = torch.tensor([0.5, 0.0, 1.0])
    feat = torch.full((S, ldf), 0.25, device="cuda")
    t = hip.Tap()
    t.n, t.tap_first, t.avgpool, t.dense, t.ldf = n, D - n, int(avgpool), 0, ldf
    pl, wt = plen.to(torch.int32).cuda(), w.cuda()
    t.plen, t.weight, t.feat = pl.data_ptr(), wt.data_ptr(), feat.data_ptr()
    hip.check(hip.load().atst_encoder_tap_fwd(ctypes.byref(ep.e), ctypes.byref(t), hip.stream()))
    y = _ln64(taps[D - n:].view(n, S, RS, C), enc)           # [n, S, RS, C]
    npat = torch.clamp(plen, max=ep.n_tok)
    cls = y[:, :, 0] * w.double()[None, :, None]
    m = (torch.arange(RS)[None, :] >= 1) & (torch.arange(RS)[None, :] <= npat[:, None])
    avg = (y * m[None, :, :, None]).sum(2) / (plen.double()[None, :, None] + 1e-6) * w.double()[None, :, None]
    ref = 0.25 + torch.cat([cls.permute(1, 0, 2).reshape(S, -1)] + ([avg.permute(1, 0, 2).reshape(S, -1)] if avgpool else []), dim=1)
    fe = rel(feat.cpu().numpy(), ref.numpy())
    # backward: dgamma / dbeta of the final norm and fc2.bias of the top block come from the tap kernels alone
    dfeat = torch.randn(S, ldf, device="cuda")
    t.dfeat = dfeat.data_ptr()
    buf = eng.teacher_grad_state()
    buf.zero_()
    hip.check(hip.load().atst_encoder_bwd_taps(ctypes.byref(ep.e), ctypes.byref(t), hip.stream()))
    yl = taps[D - n:].view(n, S, RS, C).clone().requires_grad_(True)
    gw = enc.norm.weight.detach().double().cpu().requires_grad_(True)
    gb = enc.norm.bias.detach().double().cpu().requires_grad_(True)
    yy = F.layer_norm(yl, (C,), gw, gb, 1e-6)
    cls = yy[:, :, 0] * w.double()[None, :, None]
    avg = (yy * m[None, :, :, None]).sum(2) / (plen.double()[None, :, None] + 1e-6) * w.double()[None, :, None]
    f = torch.cat([cls.permute(1, 0, 2).reshape(S, -1)] + ([avg.permute(1, 0, 2).reshape(S, -1)] if avgpool else []), dim=1)
    (f * dfeat.double().cpu()).sum().backward()
    dg = rel(eng.param_view("teacher", "encoder.norm.weight", grad=True).cpu().numpy(), gw.grad.numpy())
    db = rel(eng.param_view("teacher", "encoder.norm.bias", grad=True).cpu().numpy(), gb.grad.numpy())
    dfc2 = rel(eng.param_view("teacher", f"encoder.blocks.{D - 1}.mlp.fc2.bias", grad=True).cpu().numpy(), yl.grad[-1].sum((0, 1)).numpy())
    print(f"\n[tap kernels n={n} avgpool={avgpool}] feat {fe:.2e} dgamma {dg:.2e} dbeta {db:.2e} fc2.bias {dfc2:.2e}")
    assert fe < 1e-5 and dg < 1e-5 and db < 1e-5 and dfc2 < 1e-5       # measured <= 7.2e-8 / 2.5e-7 / 4.3e-7 / 1.2e-7


def test_dense_layers_and_forward():
    """get_intermediate_layers (dense taps) and forward (n = 1 CLS) on the differentiable path against the no-grad path and the oracle."""
    D, S = 3, 2
    W = O.recipe_weights("small", depth=D, seed=71)
    enc = teacher_encoder(71, depth=D)
    x = O.recipe_mel(S, 801, seed=73)
    length = torch.tensor([801, 500])
    with torch.no_grad():
        ref_layers = enc.get_intermediate_layers(x.cuda(), length, 2)
        ref_cls = enc(x.cuda(), length=length)
    enc.requires_grad_(True)
    enc.eval()
    cls = enc(x.cuda(), length=length)
    assert cls.grad_fn is not None and rel(cls.detach().cpu().numpy(), ref_cls.cpu().numpy()) < 1e-2
    del cls                                          # (its tape is the next call's: one live differentiable call per geometry)
    layers = enc.get_intermediate_layers(x.cuda(), length, 2)
    assert all(l.grad_fn is not None for l in layers)
    for a, b in zip(layers, ref_layers):
        assert a.shape == b.shape and rel(a.detach().cpu().numpy(), b.cpu().numpy()) < 1e-2
    R = [torch.randn(l.shape) for l in layers]
    sum((l * r.cuda()).sum() for l, r in zip(layers, R)).backward()
    pre = "teacher.encoder."
    leaves = {k: v.clone().requires_grad_(True) for k, v in W.items() if k.startswith(pre) and v.dtype == torch.float32}
    h, plen = O.encoder_tokens(leaves, pre, x, length, True)
    bias = O.key_padding_bias(h.shape[1], plen + 1)
    outs = []
    for j in range(D):
        h = O.block_forward(leaves, f"{pre}blocks.{j}.", h, bias, 6)
        if D - j <= 2:
            outs.append(F.layer_norm(h, (384,), leaves[pre + "norm.weight"], leaves[pre + "norm.bias"], 1e-6))
    sum((o * r).sum() for o, r in zip(outs, R)).backward()
    params = dict(enc.named_parameters())
    num = sum(float((params[k[len(pre):]].grad.cpu() - v.grad).norm() ** 2) for k, v in leaves.items() if v.grad is not None)
    den = sum(float(v.grad.norm() ** 2) for v in leaves.values() if v.grad is not None)
    print(f"\n[dense taps] grad rel-L2 {math.sqrt(num / den):.3e}")
    assert math.sqrt(num / den) < 1e-2                 # measured 4.7e-3 - 5.0e-3


def test_gradients_accumulate_like_torch():
    enc = teacher_encoder(81, depth=2)
    enc.requires_grad_(True)
    enc.eval()
    x, length = O.recipe_mel(2, 700, seed=83).cuda(), torch.tensor([700, 650])
    enc.get_intermediate_layers_chunks(x, length, 2, 601, True).sum().backward()
    g1 = enc.blocks[0].mlp.fc1.weight.grad.clone()
    enc.get_intermediate_layers_chunks(x, length, 2, 601, True).sum().backward()
    assert torch.allclose(enc.blocks[0].mlp.fc1.weight.grad, 2 * g1, rtol=1e-4, atol=1e-6)
    for p in enc.parameters():
        p.grad = None
    enc.get_intermediate_layers_chunks(x, length, 2, 601, True).sum().backward()
    assert torch.allclose(enc.blocks[0].mlp.fc1.weight.grad, g1, rtol=1e-4, atol=1e-6)


def test_finetune_loop_trains():
    """FineTuningPLModule.training_step restated: LinearHead, cross-entropy, SGD(momentum 0.9) with layer-wise lr scales, clip_grad_norm_(3.0)."""
    torch.manual_seed(0)
    enc = teacher_encoder(91, depth=4)
    enc.requires_grad_(True)
    enc.train()
    B = 8
    base = O.recipe_mel(B, 1201, seed=93)
    y = torch.tensor([0, 1] * (B // 2))
    x = (base + 0.6 * (2 * y.float() - 1)[:, None, None, None] * torch.linspace(-1, 1, 64)[None, None, :, None]).cuda()
    length = torch.tensor([1201, 1100, 900, 1201, 700, 1201, 1000, 800])
    head = FR.LinearHead(2 * 4 * 384, 2).cuda()
    # layer-wise lr (downstream/model.py:129-169): block i gets decay^(depth - i), the token stage decay^(depth + 1), the final norm 1
    decay, groups = 0.75, {}
    for name, p in enc.named_parameters():
        if name.startswith("blocks."):
            scale = decay ** (4 - int(name.split(".")[1]))
        elif name.startswith("norm."):
            scale = 1.0
        else:
            scale = decay ** 5                                   # patch / cls / pos embeddings
        groups.setdefault(scale, []).append(p)
    lr = 0.05
    opt = torch.optim.SGD([{"params": ps, "lr": lr * s} for s, ps in groups.items()] + [{"params": head.parameters(), "lr": lr}],
                          lr=lr, momentum=0.9)
    w0 = enc.blocks[1].attn.qkv.weight.detach().clone()
    losses = []
    for step in range(20):
        opt.zero_grad(set_to_none=True)
        feats = enc.get_intermediate_layers_chunks(x, length, 4, 601, True)
        loss = F.cross_entropy(head(feats), y.cuda())
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(enc.parameters()) + list(head.parameters()), 3.0)
        opt.step()
        losses.append(float(loss.detach()))
    print(f"\n[finetune loop] loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert losses[-1] < 0.5 * losses[0]
    assert float((enc.blocks[1].attn.qkv.weight.detach() - w0).norm()) > 0
    # the bf16 shadows follow SGD: the next call equals one made after a forced re-sync
    enc.eval()
    f1 = enc.get_intermediate_layers_chunks(x, length, 4, 601, True).detach()
    enc._eng[0].sync_shadows(force=True)
    f2 = enc.get_intermediate_layers_chunks(x, length, 4, 601, True).detach()
    assert torch.equal(f1, f2)


def test_refusals():
    """fp8 and precise engines refuse the differentiable path.  A Frame teacher has no tap backward either: it says so, and its inference
    API keeps returning features without a graph (the ATST-Frame embedding helpers call it with trainable parameters under grad mode)."""
    x, length = O.recipe_mel(2, 601, seed=95).cuda(), torch.tensor([601, 500])
    for kw in (dict(fp8=True), dict(precise=True)):
        enc = ATST("small", depth=2, **kw).teacher.encoder
        enc.requires_grad_(True)
        assert not enc.tap_backward_supported()
        with pytest.raises(NotImplementedError):
            enc.get_intermediate_layers(x, length, 1)
    model = ATST("small", depth=2, frame=True)
    enc = model.teacher.encoder
    enc.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="Frame"):
        enc.tap_backward_supported(raise_=True)
    assert enc.get_intermediate_layers(x, length, 1).grad_fn is None


def test_student_and_frozen_teacher_stay_on_the_inference_path():
    model = ATST("small", depth=2)
    x, length = O.recipe_mel(2, 601, seed=97).cuda(), torch.tensor([601, 500])
    assert model.student.encoder.get_intermediate_layers_chunks(x, length, 2, 601, True).grad_fn is None
    assert model.teacher.encoder.get_intermediate_layers_chunks(x, length, 2, 601, True).grad_fn is None
    assert model.engine.tg32 is None
