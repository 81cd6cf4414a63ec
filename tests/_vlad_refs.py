"""The descriptor distance and the float64 hard VLAD that the VLAD tests share (not a test module)."""
import torch
import torch.nn.functional as F


def l2rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def hard_vlad_f64(x, centers, labels, norm_descs=True, intra_norm=True, slab=None):
    """The reference expression (utilities.py:959-962, :854-861, :889) for ONE image in float64 under a given assignment, on the
    device of ``x``: per-cluster sums of normalise(x) - c, intra-norm, global norm.  ``slab``: that many tokens at a time (an
    image of several GiB).  F.normalize IS x / ||x||.clamp_min(1e-12), the clamp the reference writes out."""
    K, D = centers.shape
    cd = centers.double()
    out = torch.zeros(K, D, dtype=torch.float64, device=x.device)
    step = slab or max(x.shape[0], 1)
    for r0 in range(0, x.shape[0], step):
        xs = x[r0:r0 + step].double()
        if norm_descs:
            xs = F.normalize(xs, dim=-1)
        lab = labels[r0:r0 + step]
        out.index_add_(0, lab, xs - cd[lab])
    if intra_norm:
        out = F.normalize(out, dim=1)
    return F.normalize(out.reshape(-1), dim=0)
