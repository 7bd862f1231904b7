"""Shared by the stem-backward tests: plain-torch CPU references of K30's two entries in any dtype, the first-max rule of the pool's
arg-max restated, and the stem + pool of the whole-ResNet replica under the GPU's own gates and routing."""
import torch
import torch.nn.functional as F


def out_hw(h: int, w: int):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def normalised_padded(frames: torch.Tensor, mean, std, padded_hw, dtype) -> torch.Tensor:
    """frames (B, 3, hi, wi) uint8 / fp32 on the CPU -> the normalised frames in `dtype`, zero-padded to padded_hw: what the stem convolves."""
    x = frames.to(dtype)
    if mean is not None:
        x = (x - mean.to(dtype).view(1, 3, 1, 1)) / std.to(dtype).view(1, 3, 1, 1)
    return F.pad(x, (0, int(padded_hw[1]) - x.shape[-1], 0, int(padded_hw[0]) - x.shape[-2]))


def ref_stem_wgrad(xn: torch.Tensor, ds: torch.Tensor, dtype) -> torch.Tensor:
    """xn (B, 3, H, W) normalised and padded, ds (B * Ho * Wo, 64) channels-last -> dW (64, 3, 7, 7) evaluated in `dtype`."""
    B, _, H, W = xn.shape
    ho, wo = out_hw(H, W)
    g = ds.view(B, ho, wo, 64).permute(0, 3, 1, 2).to(dtype).contiguous()
    return torch.nn.grad.conv2d_weight(xn.to(dtype), (64, 3, 7, 7), g, stride=2, padding=3)


def to_planes(t: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """(h * w, C) channels-last -> (1, C, h, w) on the CPU."""
    return t.detach().cpu().view(1, h, w, -1).permute(0, 3, 1, 2).contiguous()


def to_cl(planes: torch.Tensor) -> torch.Tensor:
    return planes.permute(0, 2, 3, 1).reshape(-1, planes.shape[1])


def ref_pool_backward(s: torch.Tensor, dp: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """CPU autograd of relu -> max_pool2d(3, 2, 1) in fp64 at the point s (h * w, C), against the cotangent dp: dS (h * w, C)."""
    x = to_planes(s, h, w).double().requires_grad_(True)
    hq, wq = out_hw(h, w)
    F.max_pool2d(torch.relu(x), 3, 2, 1).backward(to_planes(dp, hq, wq).double())
    return to_cl(x.grad)


def first_max_indices(planes: torch.Tensor) -> torch.Tensor:
    """The pool's arg-max as the kernel's contract states it: the 3x3 window scanned row-major over its pixels inside the map, a new
    maximum only on strict >.  planes (B, C, h, w) -> flat indices y * w + x, (B, C, hq, wq), as F.max_pool2d(return_indices=True) gives."""
    B, C, h, w = planes.shape
    hq, wq = out_hw(h, w)
    idx = torch.zeros((B, C, hq, wq), dtype=torch.long)
    for oy in range(hq):
        for ox in range(wq):
            best = torch.full((B, C), float("-inf"), dtype=planes.dtype)
            at = torch.full((B, C), -1, dtype=torch.long)
            for y in range(max(2 * oy - 1, 0), min(2 * oy + 2, h)):
                for x in range(max(2 * ox - 1, 0), min(2 * ox + 2, w)):
                    v = planes[:, :, y, x]
                    take = v > best
                    best = torch.where(take, v, best)
                    at = torch.where(take, torch.full_like(at, y * w + x), at)
            idx[:, :, oy, ox] = at
    return idx


def routed_pool(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """The max-pool as the linear map its backward differentiates: output (b, c, oy, ox) IS input pixel idx[b, c, oy, ox] of plane (b, c)."""
    B, C = x.shape[:2]
    return x.reshape(B, C, -1).gather(2, idx.reshape(B, C, -1)).view(idx.shape)


def replica_stem(stem_pair, xn: torch.Tensor, s_gpu: torch.Tensor) -> torch.Tensor:
    """The unfolded stem (conv, FrozenBN) and the pool in xn's dtype under the GPU's own gate and routing: s_gpu (B, 64, h, w), the stem's
    stored outputs.  The ReLU is a multiplication by s_gpu > 0, the pool takes the pixels torch's rule picks in s_gpu."""
    conv, bn = stem_pair
    y = bn(conv(xn)) * (s_gpu > 0).to(xn.dtype)
    _, idx = F.max_pool2d(s_gpu, 3, 2, 1, return_indices=True)
    return routed_pool(y, idx)
