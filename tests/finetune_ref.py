"""Plain-torch restatement of the fine-tuning recipe for the tests: the reference's get_intermediate_layers_chunks (audio_transformer.py:257-366)
on the oracle's encoder (O.encoder_tokens / O.block_forward) with the final LayerNorm at every tapped block and get_cls_avg's pooling, and
FineTuningPLModule's LinearHead (downstream/model.py, modules/head.py:48-70: BatchNorm1d(affine=False) + Linear)."""
import torch
import torch.nn.functional as F

from oracle import atst_oracle as O


def chunk_features(W, pre, x, length, n, chunk_len=601, avgpool=True, depth=12, num_heads=6, keep=None, drop_path_rate=0.1):
    """keep: optional list (one per chunk) of [depth, 2, S] 0/1 DropPath draws; None = eval mode."""
    total = x.shape[-1]
    length = torch.as_tensor(length)
    dpr = O.drop_path_rates(depth, drop_path_rate)
    cls, avg, marks = [], [], []
    for i in range(total // chunk_len + 1):
        start, end = i * chunk_len, min((i + 1) * chunk_len, total)
        if end <= start:
            continue
        cur = torch.clip(length - i * chunk_len, 0)
        marks.append((cur > 0) if i == 0 else (cur > chunk_len // 2))
        h, plen = O.encoder_tokens(W, pre, x[..., start:end], cur, True)
        bias = O.key_padding_bias(h.shape[1], plen + 1)
        outs = []
        for j in range(depth):
            k = keep[len(marks) - 1] if keep is not None else None
            h = O.block_forward(W, f"{pre}blocks.{j}.", h, bias, num_heads, None if k is None else k[j, 0], None if k is None else k[j, 1],
                                dpr[j] if k is not None else 0.0)
            if depth - j <= n:
                outs.append(F.layer_norm(h, (h.shape[-1],), W[pre + "norm.weight"], W[pre + "norm.bias"], 1e-6))
        lm = (torch.arange(outs[0].shape[1] - 1)[None, :] < plen[:, None]).unsqueeze(-1)
        cls.append([o[:, 0] for o in outs])
        avg.append([(o[:, 1:] * lm).sum(1) / (plen[:, None] + 1e-6) for o in outs])
    m = torch.stack(marks).float()[:, :, None]                          # [chunks, S, 1]
    cls_out = [(torch.stack([c[k] for c in cls]) * m).sum(0) / m.sum(0) for k in range(len(cls[0]))]
    avg_out = [(torch.stack([a[k] for a in avg]) * m).sum(0) / m.sum(0) for k in range(len(avg[0]))]
    return torch.cat(cls_out + (avg_out if avgpool else []), dim=-1)


class LinearHead(torch.nn.Module):
    """modules/head.py:48-70 with use_norm=True, affine=False."""

    def __init__(self, dim, num_labels):
        super().__init__()
        self.norm = torch.nn.BatchNorm1d(dim, affine=False)
        self.linear = torch.nn.Linear(dim, num_labels)

    def forward(self, x):
        return self.linear(self.norm(x.unsqueeze(2)).view(x.size(0), -1))
