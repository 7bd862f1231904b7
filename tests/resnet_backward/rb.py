"""Shared by the ResNet-backward tests: plain-torch CPU references of K24's two entries in any dtype, and the models the GPU tests run --
the real ResNet50 with random FrozenBN statistics, folded on the GPU beside its unfolded CPU twin."""
import copy

import torch

from pod_compare_amd import modeling
from pod_compare_amd.resnet_train import trainable_blocks


def out_hw(h: int, w: int, stride: int):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def gather_rows(x: torch.Tensor, images: int, h: int, w: int, stride: int) -> torch.Tensor:
    """x (images * h * w, C) -> the rows a 1x1 conv of `stride` reads, (images * ho * wo, C), contiguous."""
    C = x.shape[1]
    return x.view(images, h, w, C)[:, ::stride, ::stride].reshape(-1, C).contiguous()


def ref_wgrad_strided(x: torch.Tensor, dy: torch.Tensor, images: int, h: int, w: int, stride: int, dtype) -> torch.Tensor:
    """dW (K, C) = sum over output pixels of dy[p][k] x[pin(p)][c], evaluated in `dtype`."""
    return dy.to(dtype).t() @ gather_rows(x, images, h, w, stride).to(dtype)


def ref_scatter(d_small: torch.Tensor, h: int, w: int, gate=None, add=None) -> torch.Tensor:
    """(gate > 0) * (d_small on the pixels with even coordinates, zero elsewhere, + add), (h * w, C) in fp64."""
    C = d_small.shape[1]
    ho, wo = out_hw(h, w, 2)
    full = torch.zeros((h, w, C), dtype=torch.float64)
    full[::2, ::2] = d_small.double().view(ho, wo, C)
    full = full.view(h * w, C)
    if add is not None:
        full = full + add.double()
    if gate is not None:
        full = full * (gate > 0).double()
    return full


def randomise_frozen_bn(module, generator) -> None:
    """Statistics and affine terms a trained model could have: scales s = weight / sqrt(var + eps) between about 0.3 and 2.4, shifts about 0.1."""
    for m in module.modules():
        if isinstance(m, modeling.FrozenBatchNorm2d):
            n = m.weight.numel()
            m.weight.copy_(0.6 + 0.8 * torch.rand(n, generator=generator))
            m.bias.copy_(0.1 * torch.randn(n, generator=generator))
            m.running_mean.copy_(0.1 * torch.randn(n, generator=generator))
            m.running_var.copy_(0.3 + 1.7 * torch.rand(n, generator=generator))


def make_resnet(seed: int = 0, device: str = "cuda:0"):
    """(folded ResNet50 on the GPU, its unfolded CPU twin) from one seed, FrozenBN randomised before folding."""
    torch.manual_seed(seed)
    shadow = modeling.ResNet50().eval()
    with torch.no_grad():
        randomise_frozen_bn(shadow, torch.Generator().manual_seed(seed + 1))
    folded = copy.deepcopy(shadow).to(device)
    modeling.fold_frozen_bn(folded)
    return folded, shadow


def to_planes(t: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """(h * w, C) channels-last -> (1, C, h, w) on the CPU."""
    return t.detach().cpu().view(1, h, w, -1).permute(0, 3, 1, 2).contiguous()


def to_cl(planes: torch.Tensor) -> torch.Tensor:
    """(B, C, h, w) -> (B * h * w, C)."""
    return planes.permute(0, 2, 3, 1).reshape(-1, planes.shape[1])


def unfolded_grad(d_folded: torch.Tensor, bn) -> torch.Tensor:
    """What the optimiser is handed for the unfolded filter W, from the folded filter's gradient: s dW', in fp64 on the CPU."""
    scale = bn.weight.double() * (bn.running_var.double() + bn.eps).rsqrt()
    return d_folded.detach().cpu().double() * scale.reshape(-1, 1, 1, 1)


def unfolded_blocks(shadow) -> list:
    """The unfolded twin's res3 - res5 blocks, in trainable_blocks' order."""
    return trainable_blocks(shadow)


def masks_from_tap(tap, B: int) -> dict:
    """{(block, "a" | "b" | "y"): bool (B, C, h, w)}: where the GPU's stored activations are positive -- the gates its backward applies."""
    masks = {}
    for i in range(len(tap["saved"][0])):
        h, w = tap["saved"][0][i]["hw"]
        for key in ("a", "b", "y"):
            masks[(i, key)] = torch.cat([to_planes(tap["saved"][b][i][key], h, w) for b in range(B)]) > 0
    return masks


def replica_forward(blocks, x: torch.Tensor, masks=None) -> list:
    """Unfolded bottlenecks (conv + FrozenBN pairs) in plain torch, in x's dtype: every block's output.  masks: the ReLUs become
    multiplications by these given gates, so the replica is the linear map the GPU's backward differentiates, whatever a near-zero
    activation rounds to."""
    outs = []
    for i, block in enumerate(blocks):
        act = (lambda t, key: torch.relu(t)) if masks is None else (lambda t, key: t * masks[(i, key)].to(t.dtype))
        a = act(block.conv1(x), "a")
        b = act(block.conv2(a), "b")
        x = act(block.conv3(b) + (x if block.shortcut is None else block.shortcut(x)), "y")
        outs.append(x)
    return outs


def in_dtype(modules, dtype) -> list:
    """Fresh copies of the modules on the CPU in `dtype`, without gradients."""
    out = [copy.deepcopy(m).to("cpu", dtype) for m in modules]
    for m in out:
        for q in m.parameters():
            q.grad = None
            q.requires_grad_(True)
    return out


def pair_list(blocks) -> list:
    """The (conv, FrozenBN) pairs of unfolded blocks in the order the gradients come in: per block shortcut (if any), conv1, conv2, conv3."""
    return [(m[0], m[1]) for block in blocks for m in ((block.shortcut,) if block.shortcut is not None else ()) + (block.conv1, block.conv2, block.conv3)]


def conv_names(blocks) -> list:
    return ["block%d.%s" % (i, n) for i, block in enumerate(blocks) for n in (("shortcut",) if block.shortcut is not None else ()) + ("conv1", "conv2", "conv3")]
