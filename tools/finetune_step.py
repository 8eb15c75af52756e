"""ms per fine-tuning step of ATST-small (downstream/train_finetune.py recipe): 64 clips of 12 s, get_intermediate_layers_chunks with n = 12
and 6 s chunks (two chunks), LinearHead + cross-entropy, backward, clip_grad_norm_(3.0), SGD(momentum 0.9).  Next to it the bare encoder
training pass of the same geometry (EncoderPass forward + backward from a dout gradient, both chunks): the difference is what the taps,
pooling and chunk bookkeeping cost.

    python tools/finetune_step.py [--steps 10] [--warmup 3] [--clips 64]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from audiossl_amd.models.atst.audio_transformer import AST_small  # noqa: E402


class LinearHead(torch.nn.Module):                   # modules/head.py:48-70 (BatchNorm1d(affine=False) + Linear)
    def __init__(self, dim, num_labels):
        super().__init__()
        self.norm = torch.nn.BatchNorm1d(dim, affine=False)
        self.linear = torch.nn.Linear(dim, num_labels)

    def forward(self, x):
        return self.linear(self.norm(x.unsqueeze(2)).view(x.size(0), -1))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clips", type=int, default=64)
    args = ap.parse_args()
    torch.manual_seed(0)
    B, width, chunk = args.clips, 1201, 601
    enc = AST_small()
    enc.requires_grad_(True)
    enc.train()
    eng = enc._eng[0]
    x = torch.randn(B, 1, 64, width, device="cuda")
    length = torch.randint(700, width + 1, (B,))
    y = torch.randint(0, 10, (B,), device="cuda")
    head = LinearHead(2 * 12 * 384, 10).cuda()
    opt = torch.optim.SGD(list(enc.parameters()) + list(head.parameters()), lr=1e-3, momentum=0.9)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(head(enc.get_intermediate_layers_chunks(x, length, 12, chunk, True)), y)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(enc.parameters()) + list(head.parameters()), 3.0)
        opt.step()

    ms_step = timed(step, args.steps, args.warmup)
    passes = []
    for i, (a, b) in enumerate([(0, chunk), (chunk, width)]):
        ep = eng._pass("teacher", B, b - a, True, ("bare", i))
        valid = eng._valid(torch.clip(length - a, 0), 1, ep.n_tok + 1)
        passes.append((ep, x[..., a:b].contiguous(), valid))
        ep.dout.normal_()

    def bare():
        for ep, xc, valid in passes:
            ep.forward(xc, valid, None, eng.drop_path_scales(B))
            ep.backward()

    ms_bare = timed(bare, args.steps, args.warmup)
    print(json.dumps({"finetune_step_ms": round(ms_step, 3), "bare_encoder_fwd_bwd_ms": round(ms_bare, 3),
                      "overhead_ms": round(ms_step - ms_bare, 3), "clips": B, "n_blocks": 12, "chunks": 2}))


if __name__ == "__main__":
    main()
