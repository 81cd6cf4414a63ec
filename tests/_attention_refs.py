"""Float64 attention and the spiky qkv generators that the attention tests share (not a test module).  Everything here runs
on the device of its input; the generators draw on the CPU."""
import torch


def attention_f64(qkv, heads, per_head=False, want_smax=False):
    """softmax((q / 8) k^T) v per 64-wide head in float64: qkv [B, T, 3 D] -> [B, T, D]; one image [T, 3 D] -> [T, D].
    ``per_head``: one (image, head) at a time instead of one batched product (T = 5330: 227 MB per head); ``want_smax``: also
    the largest |logit| of every query row over its heads, [B, T] (or [T])."""
    if qkv.dim() == 2:
        res = attention_f64(qkv[None], heads, per_head, want_smax)
        return (res[0][0], res[1][0]) if want_smax else res[0]
    B, T, D3 = qkv.shape
    q, k, v = qkv.double().reshape(B, T, 3, heads, 64).permute(2, 0, 3, 1, 4)          # each [B, heads, T, 64]
    if per_head:
        out = torch.empty(B, T, D3 // 3, dtype=torch.float64, device=qkv.device)
        smax = torch.zeros(B, T, dtype=torch.float64, device=qkv.device)
        for b in range(B):
            for h in range(heads):
                s = (q[b, h] * 0.125) @ k[b, h].t()
                smax[b] = torch.maximum(smax[b], s.abs().amax(dim=1))
                out[b, :, h * 64:(h + 1) * 64] = torch.softmax(s, dim=-1) @ v[b, h]
    else:
        s = (q * 0.125) @ k.transpose(-2, -1)
        smax = s.abs().amax(dim=(1, 3)) if want_smax else None
        out = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, D3 // 3)
    return (out, smax) if want_smax else out


def spiky_qkv(B, T, heads, seed):
    """A batch [B, T, 3 D]: a loud query / key pair (the running-max rescale path), small-magnitude tokens next to ordinary
    ones, one value row far above the others (sets the image scale), loud keys in the last key groups of the last image."""
    D = heads * 64
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3 * D, generator=g) * 1.5
    qkv[0, 3, :D] *= 6.0
    qkv[0, T - 2, D:2 * D] *= 6.0
    qkv[:, ::7] *= 0.05
    qkv[:, 5, 2 * D:] *= 40.0
    if T > 2080:
        qkv[0, 2048:2080, 2 * D:] = 0.0                   # an all-zero V tile beyond key group 64: must not set the scale
    qkv[B - 1, T - 40:, D:2 * D] *= 3.0
    return qkv


def spiky_qkv_image(T, heads, seed):
    """One image [T, 3 D] of any length (T = 2 included: the positions are clamped): the loud query / key pair, the small
    tokens and the loud value row of spiky_qkv, without its zero tile and its loud last keys."""
    D = heads * 64
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(T, 3 * D, generator=g) * 1.5
    qkv[min(3, T - 1), :D] *= 6.0
    qkv[max(T - 2, 0), D:2 * D] *= 6.0
    qkv[::7] *= 0.05
    qkv[min(5, T - 1), 2 * D:] *= 40.0
    return qkv
