"""The plain-torch restatement the fine-tuning GPU tests compare against (tests/finetune_ref.py) reproduces the reference's fine-tuning
recipe, pinned by tests/golden/clip_finetune.npz (make_golden_finetune.py): features, loss and encoder gradients, fp32 on the CPU."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import finetune_ref as FR  # noqa: E402
from oracle import atst_oracle as O  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sample_idx(n, k=192):
    return np.unique(np.linspace(0, n - 1, num=min(n, k)).astype(np.int64))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def test_restatement_matches_reference_finetune_golden():
    G = np.load(os.path.join(GOLD, "clip_finetune.npz"))
    W = O.recipe_weights("small", seed=int(G["weight_seed"]))
    pre = "teacher.encoder."
    leaves = {k: v.clone().requires_grad_(True) for k, v in W.items() if k.startswith(pre) and v.dtype == torch.float32}
    x = O.recipe_mel(3, 1201, seed=int(G["mel_seed"]))
    feats = FR.chunk_features(leaves, pre, x, torch.from_numpy(G["length"]), 12)
    head = FR.LinearHead(feats.shape[1], 3)
    with torch.no_grad():
        head.linear.weight.copy_(torch.from_numpy(G["head_w"]))
        head.linear.bias.copy_(torch.from_numpy(G["head_b"]))
    loss = F.cross_entropy(head(feats), torch.from_numpy(G["labels"]))
    loss.backward()
    assert rel(feats.detach().numpy(), G["feats"]) < 1e-5
    assert abs(float(loss.detach()) - float(G["loss"])) < 1e-5
    worst = 0.0
    for k, v in leaves.items():
        name = k[len(pre):]
        if "gnone/" + name in G:
            assert v.grad is None or float(v.grad.abs().max()) == 0.0, name
            continue
        g = v.grad.reshape(-1).double()
        worst = max(worst, rel(g[sample_idx(g.numel())].numpy(), G["gsamp/" + name]))
    print(f"\n[finetune restatement] worst gradient rel-L2 {worst:.3e}")
    assert worst < 1e-4                                  # measured 0: the same fp32 ops as the reference, in the same order
