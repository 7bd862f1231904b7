"""Shared by the FPN-backward tests: plain-torch CPU references of K23's three entries, in any dtype."""
import torch
import torch.nn.functional as F


def ref_wgrad(x: torch.Tensor, dy: torch.Tensor, dtype):
    """x (pixels, C), dy (pixels, K) -> (dW (K, C) = dy.T @ x, db (K,)) evaluated in `dtype`."""
    return dy.to(dtype).t() @ x.to(dtype), dy.to(dtype).sum(0)


def patch_rows(x: torch.Tensor, h: int, w: int, relu: bool = False) -> torch.Tensor:
    """(h * w, C) channels-last -> the (ho * wo, 9 C) patch matrix of a 3x3 / stride-2 / pad-1 conv, taps in (ty, tx) order, by F.unfold."""
    C = x.shape[1]
    planes = x.view(1, h, w, C).permute(0, 3, 1, 2)
    cols = F.unfold(F.relu(planes) if relu else planes, 3, padding=1, stride=2)            # (1, C * 9, L), rows (c, ty, tx)
    return cols.view(C, 9, -1).permute(2, 1, 0).reshape(-1, 9 * C)


def ref_col2im(dcols: torch.Tensor, h: int, w: int, gate=None, add=None) -> torch.Tensor:
    """The input gradient of patch_rows by autograd: (gate > 0) * gathered sum + add, (h * w, C) in dcols' dtype."""
    C = dcols.shape[1] // 9
    x = (torch.ones((h * w, C), dtype=dcols.dtype) if gate is None else gate.to(dcols.dtype).clone()).requires_grad_(True)
    (patch_rows(x, h, w, relu=gate is not None) * dcols).sum().backward()
    return x.grad if add is None else x.grad + add.to(dcols.dtype)


def ref_upsample2_sum(d_child: torch.Tensor, h: int, w: int, add: torch.Tensor) -> torch.Tensor:
    """add + the gradient of F.interpolate(top, size=(h, w), mode="nearest") towards top, (ht * wt, C)."""
    C, ht, wt = d_child.shape[1], (h + 1) // 2, (w + 1) // 2
    top = torch.zeros((1, C, ht, wt), dtype=d_child.dtype, requires_grad=True)
    up = F.interpolate(top, size=(h, w), mode="nearest")
    (up * d_child.view(1, h, w, C).permute(0, 3, 1, 2)).sum().backward()
    return add.to(d_child.dtype) + top.grad.permute(0, 2, 3, 1).reshape(ht * wt, C)
