"""res3 - res5 of the ResNet with a backward pass: detectron2's BottleneckBlocks above MODEL.BACKBONE.FREEZE_AT = 2 in training mode
(probabilistic_retinanet.py:96-100, `self.backbone(images.tensor)`, under train_net.py's loop) as ONE torch.autograd.Function over the
three stages (`_BlocksTrain`, over any chain of bottlenecks).  The stem and res2 stay frozen, as the reference's do (`res2_maps`, under no_grad),
unless FREEZE_AT says otherwise: at 1 res2's three blocks lead the chain and only the stem and its max-pool run under no_grad (`pool_maps`);
at 0 those two get a backward pass as well (`_StemTrain`, `stem_forward_train`: K30's pool backward with the stem's ReLU gate per image,
then one 7x7 weight gradient over the batch's stacked frames; the stem computes no input gradient).

Forward: Bottleneck.forward_cl's own launches, per image, unchanged; the input x, conv1's and conv2's outputs a and b and the output y of
every block are kept.  Backward, on the B images at once, from the last block of res5 down to the first block of res3:
    the output gate  dZ = (dY from above + dC from the FPN) (y > 0)    pod_relu_dropout_backward at p = 0, or the scatter below
    conv3            dW3 = pod_conv1x1_wgrad_strided(b, dZ) (K24); dB = dZ W3 on pod_conv1x1_split with the transposed filter, gated on b > 0
    conv2            dW2 = pod_conv3x3_wgrad(a, dB) (K22); dA = the GEMM of dB's patch matrix (head_train.backward_gemm), gated on a > 0
    conv1            dW1 = pod_conv1x1_wgrad_strided(x, dA, the block's stride)
    identity block   dX = dA W1 + dZ, dZ as the GEMM's residual
    conv shortcut    dWs = pod_conv1x1_wgrad_strided(x, dZ, 2); the half-resolution dA W1 + dZ Ws is one GEMM with the other's result as
                     residual, and pod_subsample2_scatter_cl (K24) expands it to the full map per image: its gate is the block below's
                     stored output, its `add` the FPN's gradient at that map -- the result is the block below's dZ
                     (res2's first block has its conv shortcut at stride 1: the same GEMM pair at full resolution and no scatter)
Every input-gradient GEMM above runs twice, on W and on -W, and half the difference is kept (`centred`): the two results share the mean of
the matrix cores' accumulation error, which 39 chained GEMMs would otherwise add up and the weight gradients sum over every pixel.
The first block of the chain computes no dX where nothing trains below it (a chain whose input requires grad gets it: tests).  The convs carry FrozenBN, folded: the gradients are those of the FOLDED
filters W' = W s, and no bias gradient exists (`FoldedMasters` hands the optimiser W with W.grad = s dW' and refolds after its step).
GPU only -- anything this path cannot take raises (hip.PodError): there is no fallback."""
from typing import List, Sequence, Tuple

import torch
from torch import nn

from . import amax, conv1x1, hip, modeling, wgrad, wino
from .conv_forms import stem_of
from .fpn_train import _stacked
from .head_train import backward_gemm, conv_params, flat_grads, flipped3x3, patch_matrix, transposed1x1

STAGES = ("res3", "res4", "res5")
FREEZE_POINTS = (0, 1, 2)         # MODEL.BACKBONE.FREEZE_AT: what stays frozen is the first `freeze_at` of (stem, res2)


def _conv_of(m) -> nn.Conv2d:
    """The conv of a (conv, FrozenBN) or folded (conv, Identity) pair."""
    return m[0] if isinstance(m, nn.Sequential) else m


def _check_freeze_at(freeze_at) -> int:
    if int(freeze_at) not in FREEZE_POINTS:
        raise hip.PodError("MODEL.BACKBONE.FREEZE_AT = {} has no training path: 0 (everything trains), 1 (the stem is frozen) or 2 (the stem and "
                           "res2 are)".format(freeze_at))
    return int(freeze_at)


def trainable_blocks(bottom_up, freeze_at: int = 2) -> list:
    """The bottlenecks detectron2 trains at MODEL.BACKBONE.FREEZE_AT = freeze_at, bottom to top: res3, res4 and res5, below 2 res2 in front."""
    stages = (("res2",) if _check_freeze_at(freeze_at) < 2 else ()) + STAGES
    return [block for name in stages for block in getattr(bottom_up, name)]


def block_convs(block) -> list:
    """One block's convs in the order their parameters enter the autograd function: shortcut (if any), conv1, conv2, conv3."""
    return [_conv_of(m) for m in ((block.shortcut,) if block.shortcut is not None else ()) + (block.conv1, block.conv2, block.conv3)]


def trainable_convs(bottom_up, freeze_at: int = 2) -> list:
    """The convs detectron2 trains at FREEZE_AT = freeze_at in a fixed order: the stem's (at 0), res2's (at 0 and 1), then those of res3,
    res4 and res5."""
    stem = [_conv_of(bottom_up.stem)] if _check_freeze_at(freeze_at) == 0 else []
    return stem + [c for block in trainable_blocks(bottom_up, freeze_at) for c in block_convs(block)]


def unfolded_pairs(bottom_up, freeze_at: int = 2) -> list:
    """The (conv, FrozenBatchNorm2d) pairs of an UNFOLDED backbone, in trainable_convs' order."""
    pairs = []
    modules = [bottom_up.stem] if _check_freeze_at(freeze_at) == 0 else []
    for block in trainable_blocks(bottom_up, freeze_at):
        modules += ((block.shortcut,) if block.shortcut is not None else ()) + (block.conv1, block.conv2, block.conv3)
    for m in modules:
        if not (isinstance(m, nn.Sequential) and len(m) == 2 and isinstance(m[1], modeling.FrozenBatchNorm2d) and m[0].bias is None):
            raise hip.PodError("training the backbone needs the unfolded (conv, FrozenBN) pairs of res3 - res5 beside the folded model")
        pairs.append((m[0], m[1]))
    return pairs


def _require(blocks) -> None:
    ok = modeling.CL_BACKBONE and modeling.WINO_BACKBONE and modeling.FUSE_CONV_TAIL and bool(wino.SPLIT_BF16)
    for block in blocks:
        ok = ok and block.cl_eligible()
        if not ok:
            break
        c1, c2, c3 = (_conv_of(block.conv1), _conv_of(block.conv2), _conv_of(block.conv3))
        s = c1.stride[0]
        ok = (c1.out_channels == c2.in_channels == c2.out_channels == c3.in_channels and c2.out_channels <= 512 and c3.out_channels <= 2048
              and c1.in_channels % 64 == 0 and c2.in_channels % 64 == 0)
        if block.shortcut is None:
            ok = ok and s == 1 and c1.in_channels == c3.out_channels
        else:
            sc = _conv_of(block.shortcut)
            ok = ok and s in (1, 2) and sc.stride[0] == s and sc.in_channels == c1.in_channels and sc.out_channels == c3.out_channels
    if not ok:
        raise hip.PodError("blocks_forward_train: these bottlenecks have no HIP training path (folded FrozenBN, the split kernels selected, bottlenecks of "
                           "1x1 / 3x3 / 1x1 with widths in multiples of 64, 3x3 width <= 512, output width <= 2048, and a 1x1 shortcut "
                           "of conv1's stride, 1 or 2)")


def _require_frame(model, image, padded=None) -> Tuple[int, int]:
    """The padded (h, w) of a frame the channels-last HIP backbone takes, as ProbabilisticRetinaNet._backbone_cl pads it (anchors.padded_size;
    padded: a batch's common padded size instead, checked to hold the frame)."""
    ok = (torch.is_tensor(image) and image.is_cuda and image.device == model.device and image.dim() == 3 and image.shape[0] == 3 and image.is_contiguous()
          and image.dtype in (torch.uint8, torch.float32) and model._cl_backbone(model.pixel_mean) and model.bottom_up.hip_stem_ok())
    if not ok:
        raise hip.PodError("training the backbone needs the channels-last HIP backbone (a (3, h, w) uint8 / fp32 frame on the model's GPU, FrozenBN "
                           "folded, the split kernels and the HIP stem selected)")
    if padded is not None:
        return modeling._check_padded(image, padded)
    return modeling._anchors.padded_size(int(image.shape[1]), int(image.shape[2]))


def res2_maps(model, image: torch.Tensor, padded=None) -> Tuple[torch.Tensor, int, int]:
    """The frozen stem, max-pool and res2 of one frame under no_grad, channels-last: (t (h * w, 256), h, w) -- what detectron2's FREEZE_AT = 2
    leaves untrained.  The frame is padded as ProbabilisticRetinaNet._backbone_cl pads it (anchors.padded_size; padded: to a batch's common size)."""
    padded = _require_frame(model, image, padded)
    with torch.no_grad():
        return model.bottom_up.forward_cl(None, frame=(image, model.pixel_mean.reshape(3), model.pixel_std.reshape(3), padded), stop_after_res2=True)


def _stem_pool(stem: nn.Conv2d, image: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, padded):
    """ResNet50.forward_cl's first two launches on one frame: (s, h, w), the stem's post-ReLU output, and (p, hq, wq), its max-pool."""
    s, h, w = stem_of(stem)(image, relu=True, mean=mean, std=std, padded_hw=padded)
    return (s, h, w), conv1x1.maxpool3x3s2_cl(s, h, w)


def pool_maps(model, image: torch.Tensor, padded=None) -> Tuple[torch.Tensor, int, int]:
    """The frozen stem and max-pool of one frame under no_grad, channels-last: (t (h * w, 64), h, w) -- what detectron2's FREEZE_AT = 1 leaves
    untrained, res2's input.  padded: a batch's common padded size (None: the frame's own)."""
    padded = _require_frame(model, image, padded)
    with torch.no_grad():
        return _stem_pool(_conv_of(model.bottom_up.stem), image, model.pixel_mean.reshape(3), model.pixel_std.reshape(3), padded)[1]


class _StemTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, stem, frames, mean, std, padded, tap, weight):
        # weight: the stem's folded filter (so that autograd asks for its gradient); the frames get none
        kept, outs = [], []
        for im in frames:
            (s, h, w), (p, _, _) = _stem_pool(stem, im, mean, std, padded)
            kept.append(s)
            outs.append(p)
        if tap is not None:                                 # tests: the stem's stored outputs, whose gates and arg-max routing the backward uses
            tap["stem"] = (kept, (h, w))
        ctx.state = (stem, frames, mean, std, padded, kept, (h, w))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *g_maps):
        stem, frames, mean, std, padded, kept, (h, w) = ctx.state
        B = len(frames)
        dp = [torch.zeros(((h - 1) // 2 + 1) * ((w - 1) // 2 + 1), 64, dtype=torch.float32, device=kept[0].device) if g is None else g.contiguous() for g in g_maps]
        ds = torch.empty((B * h * w, 64), dtype=torch.float32, device=kept[0].device)
        wgrad.over_images(B, ds, lambda b, rows, rec: wgrad.maxpool3x3s2_backward_cl(kept[b], dp[b], h, w, out=rows(ds), record=rec))
        if all(tuple(f.shape) == tuple(frames[0].shape) for f in frames):
            x = frames[0].unsqueeze(0) if B == 1 else torch.stack(list(frames))      # one shape: one weight gradient over the stacked frames
            dW = wgrad.stem7x7_wgrad(x, ds, padded, mean, std, bound=stem_of(stem)._input_bound(x, mean, std))
        else:
            # frames of several sizes against one padded size: a weight gradient per image on its rows of dS, added in image order
            dW, rows, rec = None, h * w, amax.of(ds)              # (the batch's record bounds every image's rows of dS)
            for b, f in enumerate(frames):
                g = wgrad.stem7x7_wgrad(f, amax.attach(ds[b * rows:(b + 1) * rows], rec), padded, mean, std, bound=stem_of(stem)._input_bound(f, mean, std))
                dW = g if dW is None else dW.add_(g)
        ctx.state = None
        return (None,) * 6 + (dW,)


def stem_forward_train(model, images: Sequence[torch.Tensor], tap=None, padded=None) -> list:
    """The stem and its max-pool with a backward pass (FREEZE_AT = 0): per image the (t (h * w, 64), h, w) res2 starts from, B frames of one
    shape -- or, with `padded`, the batch's common padded size, of any shapes it holds (the weight gradient is then K30 once per image,
    the results added in image order; a batch of one shape makes the launches it makes without `padded`).  The maps carry a grad_fn that reaches the stem's (folded) filter: K30's pool backward per image into one stacked dS, then one
    weight gradient over the batch's stacked frames.  The stem computes no input gradient."""
    images = list(images)
    if not images:
        raise hip.PodError("stem_forward_train: at least one frame")
    common = padded is not None
    padded = _require_frame(model, images[0], padded)
    for im in images[1:]:
        if _require_frame(model, im, padded if common else None) != padded or im.dtype != images[0].dtype or (not common and tuple(im.shape) != tuple(images[0].shape)):
            raise hip.PodError("stem_forward_train: a batch holds frames of one shape and type, got {} {} and {} {}".format(
                tuple(images[0].shape), images[0].dtype, tuple(im.shape), im.dtype))
    stem = _conv_of(model.bottom_up.stem)
    if not stem.weight.requires_grad:
        raise hip.PodError("stem_forward_train: the stem's filter does not require a gradient (FoldedMasters sets it)")
    with torch.cuda.device(images[0].device):
        outs = _StemTrain.apply(stem, images, model.pixel_mean.reshape(3), model.pixel_std.reshape(3), tuple(padded),
                                tap if tap is not None else getattr(model.bottom_up, "train_tap", None), stem.weight)
    h, w = (int(padded[0]) - 1) // 2 + 1, (int(padded[1]) - 1) // 2 + 1
    return [(t, (h - 1) // 2 + 1, (w - 1) // 2 + 1) for t in outs]


def centred(layout, conv, d: torch.Tensor, n: int, residual=None) -> torch.Tensor:
    """d W (+ residual) for one of the backward's input-gradient GEMMs (head_train.backward_gemm of `layout`).  The matrix cores'
    accumulation leaves every pod_conv1x1_split result an error whose MEAN is not zero and does not depend on the operands' signs
    (measured: -0.05 .. -0.19 of its rms; profiles/resnet_backward.md).  One launch's is far below fp32's own error, but it is the same
    for every pixel of a channel, the shortcuts hand it down unchanged, 13 blocks' add up, and a weight gradient sums it over every pixel
    against non-negative activations.  So the GEMM runs on W and on -W -- the f16 terms and products of the second are the exact
    negatives of the first's -- and half their difference keeps the product and drops what the two have in common:
    P = d W + r + e, M = -d W + e, (P - M + r) / 2 = d W + r."""
    y = backward_gemm(conv, layout)(d, n, 1, residual=residual)
    y.sub_(backward_gemm(conv, layout, negated=True)(d, n, 1))
    if residual is not None:
        y.add_(residual)
    return y.mul_(0.5)


def _taps(blocks) -> list:
    """The blocks whose output leaves the chain: the last of every stage (the block below one with a shortcut) and the last of all."""
    return [i for i in range(len(blocks)) if i + 1 == len(blocks) or blocks[i + 1].shortcut is not None]


class _BlocksTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, blocks, hw0, tap, B, *tensors):
        # tensors: the B input maps (so that autograd can ask for their gradient; the trainer's, res2's, never do), then the filters
        saved, outs, taps = [], [], _taps(blocks)
        for x in tensors[:B]:
            (h, w), keep = hw0, []
            for block in blocks:
                keep.append({})
                x, h, w = block.forward_cl(x, h, w, keep=keep[-1])
            saved.append(keep)
            outs += [keep[i]["y"] for i in taps]
        if tap is not None:                                 # tests: a dict that receives the saved activations (and the gates' outputs)
            tap["saved"], tap["dz"] = saved, {}
        ctx.state = (blocks, saved, tap)
        ctx.n_params = len(tensors) - B
        return tuple(outs)

    @staticmethod
    def backward(ctx, *g_maps):
        blocks, saved, tap = ctx.state
        B, taps = len(saved), _taps(blocks)
        dev = saved[0][0]["x"].device
        need_x = any(ctx.needs_input_grad[4:4 + B])

        def keep_dz(i, what, t):
            if tap is not None:
                tap["dz"][(i, what)] = t

        def from_above(i):
            """What the FPN (or whoever reads the maps) hands down at the output of block i, per image; None where nobody does."""
            if i not in taps:
                return None
            gs = [g_maps[len(taps) * b + taps.index(i)] for b in range(B)]
            if all(g is None for g in gs):
                return None
            some = next(g for g in gs if g is not None)
            return [torch.zeros_like(some) if g is None else g.contiguous() for g in gs]

        def all_images(i, key):
            return _stacked([saved[b][i][key] for b in range(B)])

        grads, dx = {}, None
        top = from_above(len(blocks) - 1) or [torch.zeros_like(saved[b][-1]["y"]) for b in range(B)]
        d, gated = torch.cat(top), False                    # (a copy: the gate below works in place)
        for i in range(len(blocks) - 1, -1, -1):
            block = blocks[i]
            (h, w), (h1, w1) = saved[0][i]["hw_in"], saved[0][i]["hw"]
            c1, c2, c3 = _conv_of(block.conv1), _conv_of(block.conv2), _conv_of(block.conv3)
            n1, stride = B * h1 * w1, c1.stride[0]
            x, a, b_ = all_images(i, "x"), all_images(i, "a"), all_images(i, "b")
            dz = d if gated else wgrad.relu_dropout_backward(all_images(i, "y"), d, 0.0)
            keep_dz(i, "z", dz)
            # conv3
            dW, _ = wgrad.conv1x1_wgrad_strided(b_, dz, B, h1, w1, 1)
            grads[c3] = (dW.view(c3.weight.shape),)
            db_ = wgrad.relu_dropout_backward(b_, centred(transposed1x1, c3, dz, n1), 0.0)
            keep_dz(i, "b", db_)
            # conv2 (K22's bias gradient is discarded: the bias is FrozenBN's shift)
            level = [(h1, w1)]
            grads[c2] = wgrad.conv3x3_wgrad(a, db_, level, B, c2.out_channels)[:1]
            da = wgrad.relu_dropout_backward(a, centred(flipped3x3, c2, patch_matrix(db_, level, B), n1), 0.0)
            keep_dz(i, "a", da)
            # conv1 and the shortcut
            dW, _ = wgrad.conv1x1_wgrad_strided(x, da, B, h, w, stride)
            grads[c1] = (dW.view(c1.weight.shape),)
            if block.shortcut is not None:
                sc = _conv_of(block.shortcut)
                dW, _ = wgrad.conv1x1_wgrad_strided(x, dz, B, h, w, stride)
                grads[sc] = (dW.view(sc.weight.shape),)
            if i == 0 and not need_x:
                break                                       # nothing trains below the first block
            if block.shortcut is None:
                d, gated = centred(transposed1x1, c1, da, n1, residual=dz), False
                continue
            # dA W1 + dZ Ws: one GEMM with the other's result as residual
            half = centred(transposed1x1, c1, da, n1, residual=centred(transposed1x1, sc, dz, n1))
            below = from_above(i - 1) if i else None
            if stride == 1:                                 # (res2's first block) nothing to expand: the gate of the block below, if there is one
                if below is not None:
                    half.add_(torch.cat(below))
                d, gated = half, False
                continue
            # at half resolution: expanded per image behind the gate of the block below, with what its output already carries
            d, gated = torch.empty((B * h * w, c1.in_channels), dtype=torch.float32, device=dev), True
            wgrad.over_images(B, d, lambda b, rows, rec: wgrad.subsample2_scatter_cl(
                rows(half), h, w, gate=saved[b][i]["x"] if i else None, add=None if below is None else below[b], out=rows(d), record=rec))
        if need_x:                                          # (the input is a leaf here, whatever made it: no gate of this pass's)
            n = int(d.shape[0]) // B
            dx = [d[b * n:(b + 1) * n] for b in range(B)]
        flat = flat_grads([c for block in blocks for c in block_convs(block)], grads)
        assert len(flat) == ctx.n_params
        ctx.state = None
        return (None, None, None, None) + tuple(dx or [None] * B) + tuple(flat)


def blocks_forward_train(blocks: Sequence, maps: Sequence[Tuple[torch.Tensor, int, int]], tap=None) -> List[list]:
    """A chain of bottlenecks with a backward pass.  maps: per image the (x, h, w) it starts from, B images of one size.  Returns per image
    the [(y, h, w), ...] of the blocks whose output leaves the chain (`_taps`); they carry a grad_fn that reaches the (folded) filter of
    every conv of the chain and, where they require it, the inputs."""
    blocks, maps = list(blocks), [tuple(m) for m in maps]
    if not blocks or not maps or any(len(m) != 3 for m in maps):
        raise hip.PodError("blocks_forward_train: at least one block, and per image the (x, h, w) it starts from")
    wgrad.require_maps("blocks_forward_train", maps)
    t0, h0, w0 = maps[0]
    _require(blocks)
    first = _conv_of(blocks[0].conv1)
    if first.in_channels != int(t0.shape[1]) or first.weight.device != t0.device:
        raise hip.PodError("blocks_forward_train: the first block takes {} channels on {}, the maps have {} on {}".format(
            first.in_channels, first.weight.device, int(t0.shape[1]), t0.device))
    weights = conv_params([c for block in blocks for c in block_convs(block)], bias=False)
    with torch.cuda.device(t0.device):
        flat = _BlocksTrain.apply(blocks, (int(h0), int(w0)), tap, len(maps), *[t for t, _, _ in maps], *weights)
    hw, (h, w) = [], (int(h0), int(w0))
    for block in blocks:
        stride = _conv_of(block.conv1).stride[0]
        h, w = (h - 1) // stride + 1, (w - 1) // stride + 1
        hw.append((h, w))
    taps = _taps(blocks)
    return [[(flat[len(taps) * b + k], hw[i][0], hw[i][1]) for k, i in enumerate(taps)] for b in range(len(maps))]


def resnet_forward_train(bottom_up, maps: Sequence[Tuple[torch.Tensor, int, int]], freeze_at: int = 2) -> List[list]:
    """maps: per image the (t, h, w) of res2_maps -- below freeze_at = 2 of pool_maps (1) or stem_forward_train (0): res2 then runs in the
    chain --, B images of one padded size.  Returns per image [(c3, h, w), (c4, h, w), (c5, h, w)], what ResNet50.forward_cl returns; the
    maps carry a grad_fn that reaches the (folded) filter of every conv of the chain and, where they require it, the maps.  A dict
    `bottom_up.train_tap`, if there is one, receives the saved activations and every gate's output (tests)."""
    blocks = trainable_blocks(bottom_up, freeze_at)
    stages = (("res2",) if int(freeze_at) < 2 else ()) + STAGES
    if [len(getattr(bottom_up, name)) > 0 and getattr(bottom_up, name)[0].shortcut is not None for name in stages] != [True] * len(stages) \
            or len(_taps(blocks)) != len(stages):
        raise hip.PodError("resnet_forward_train: every trained stage opens with a conv-shortcut block and continues with identity blocks")
    outs = blocks_forward_train(blocks, maps, tap=getattr(bottom_up, "train_tap", None))
    return [per_image[-3:] for per_image in outs]


class FoldedMasters:
    """The parameters the optimiser holds for convs that run with FrozenBN folded.  The device model computes with W' = W s; detectron2
    trains W and freezes s and the shift.  For every conv: the unfolded W as the master parameter on the device (from the unfolded model's
    conv), s from its FrozenBN by fold_frozen_bn's expression on the device; `collect_grads` turns the folded filters' gradients into
    W.grad = s dW', `refold` rewrites conv.weight = W s in place after the optimiser's step (the version bump rebuilds the derived filters),
    bit-equal to what fold_frozen_bn makes of a checkpoint that holds W.  The folded bias never changes."""

    def __init__(self, folded_convs: Sequence[nn.Conv2d], pairs: Sequence[Tuple[nn.Conv2d, nn.Module]], freeze_at: int = 2):
        self.freeze_at = int(freeze_at)          # which convs these are: trainable_convs(., freeze_at) / unfolded_pairs(., freeze_at)
        if len(folded_convs) != len(pairs):
            raise hip.PodError("FoldedMasters: {} folded convs against {} (conv, FrozenBN) pairs".format(len(folded_convs), len(pairs)))
        self.convs, self.params, self.scales = list(folded_convs), [], []
        with torch.no_grad():
            for conv, (src, bn) in zip(self.convs, pairs):
                if tuple(conv.weight.shape) != tuple(src.weight.shape):
                    raise hip.PodError("FoldedMasters: a folded {} filter against an unfolded {}".format(tuple(conv.weight.shape), tuple(src.weight.shape)))
                dev = conv.weight.device
                weight, var = bn.weight.detach().to(dev), bn.running_var.detach().to(dev)
                scale = weight * (var + bn.eps).rsqrt()                       # fold_frozen_bn's expression, evaluated where it evaluates it
                self.scales.append(scale.reshape(-1, 1, 1, 1))
                self.params.append(nn.Parameter(src.weight.detach().to(dev).clone()))
        for c in self.convs:
            c.weight.requires_grad_(True)                                      # (the autograd function hands the folded filter's gradient here)

    def collect_grads(self) -> None:
        for conv, p, s in zip(self.convs, self.params, self.scales):
            g = conv.weight.grad
            p.grad = None if g is None else g * s
            conv.weight.grad = None

    def refold(self) -> None:
        with torch.no_grad():
            for conv, p, s in zip(self.convs, self.params, self.scales):
                conv.weight.copy_(p)
                conv.weight.mul_(s)

    def copy_to(self, pairs: Sequence[Tuple[nn.Conv2d, nn.Module]]) -> None:
        """The master weights into the unfolded model's convs (what a checkpoint describes)."""
        with torch.no_grad():
            for p, (dst, _) in zip(self.params, pairs):
                dst.weight.copy_(p.detach().to(dst.weight.device))
