"""Golden of the fine-tuning recipe (downstream/train_finetune.py): the reference AST_small's get_intermediate_layers_chunks at full depth,
n = 12, two chunks, eval mode (no DropPath), under a LinearHead in train mode (BatchNorm1d(affine=False) batch statistics + Linear) and a
cross-entropy loss.  Writes tests/golden/clip_finetune.npz: features, loss, the head's initial weights, and the encoder gradients in the
gnorm/ gsamp/ gnone/ format of clip_encoder_grad.npz.  Run on CPU with the reference on sys.path (see make_golden.py)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (sys.path, stubs, grad_digest, save)

O = MG.O

WEIGHT_SEED, MEL_SEED, HEAD_SEED = 43, 41, 47
LENGTH = [1201, 900, 500]
LABELS = [0, 1, 2]


def gen_finetune(name="clip_finetune"):
    from audiossl.models.atst.audio_transformer import AST_small
    from audiossl.modules.head import LinearHead
    enc = AST_small()
    W = O.recipe_weights("small", seed=WEIGHT_SEED)
    enc.load_state_dict({k[len("teacher.encoder."):]: v for k, v in W.items() if k.startswith("teacher.encoder.")})
    enc.eval()
    x = O.recipe_mel(3, 1201, seed=MEL_SEED)
    length = torch.tensor(LENGTH)
    torch.manual_seed(HEAD_SEED)
    head = LinearHead(2 * 12 * 384, 3)
    head.train()
    head_w, head_b = head.linear.weight.detach().clone(), head.linear.bias.detach().clone()
    feats = enc.get_intermediate_layers_chunks(x, length, 12, 601, True)
    loss = torch.nn.functional.cross_entropy(head(feats), torch.tensor(LABELS))
    loss.backward()
    arrs = dict(length=length.numpy(), labels=np.array(LABELS), feats=feats.detach().numpy(), loss=np.array(float(loss)),
                head_w=head_w.numpy(), head_b=head_b.numpy(), weight_seed=WEIGHT_SEED, mel_seed=MEL_SEED)
    arrs.update(MG.grad_digest(enc.named_parameters()))
    MG.save(name, **arrs)


if __name__ == "__main__":
    gen_finetune()
