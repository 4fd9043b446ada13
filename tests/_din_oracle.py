"""fp64 oracle of attention_by_dnn: the reference's own formulation (rec_now/rec_block/attention.py:41-82) restated in torch --
doc tiled to (B, L, D), concatenated to a (B, L, 2D) input, the Dense stack, sigmoid, the sums over l.  Autograd through it gives
every gradient the HIP kernels are compared against."""
import torch

_ACTS = {'linear': lambda x: x, None: lambda x: x, 'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}


def attention_by_dnn(user_emb, doc_emb, kernels, biases, activation='relu'):
    """user_emb (B, L, D), doc_emb (B, D), kernels[i] (in, out) with in = 2D for the first, biases[i] (out,).
    Returns attn_mat (B, D), attn_score_sum (B, 1)."""
    L = user_emb.shape[1]
    doc_tiled = doc_emb.unsqueeze(1).expand(-1, L, -1)
    x = torch.cat([user_emb, doc_tiled], dim=-1)
    act = _ACTS[activation]
    for i, (k, b) in enumerate(zip(kernels, biases)):
        x = x @ k + b
        if i < len(kernels) - 1:
            x = act(x)
    s = torch.sigmoid(x)                              # (B, L, 1)
    attn_mat = (user_emb * s).sum(dim=1)
    attn_score_sum = s.squeeze(2).sum(dim=1, keepdim=True)
    return attn_mat, attn_score_sum
