"""The FPN with a backward pass: detectron2's FPN + LastLevelP6P7 (probabilistic_retinanet.py:96-100, `self.backbone(images.tensor)`) in
training mode under train_net.py's loop, as ONE torch.autograd.Function over the whole FPN.

Forward: FPN.forward_cl's own launches, per image, unchanged; the summed laterals l3, l4, l5 and p6 of every image are kept, the two
patch matrices are re-formed in backward.  Backward, on the B images at once (a weight gradient sums over pixels, whichever image
they are of):
    p7               dW, db = pod_conv1x1_wgrad(cols(relu p6), dP7); dcols = dP7 W9 on pod_conv1x1_split; dP6 = pod_col2im3x3s2_cl(dcols,
                     gate = p6, add = the gradient p6 has from the head)
    p6               dW, db = pod_conv1x1_wgrad(cols(c5), dP6) -- c5 is the frozen backbone's: no input gradient
    output convs     dW, db = pod_conv3x3_wgrad(l_i, dP_i) (K22); dL_i = the GEMM of dP_i's patch matrix with the flipped, transposed filter
                     (head_train.backward_gemm)
    top-down         dL4 += up2_sum(dL3), dL5 += up2_sum(dL4) (pod_upsample2_sum_cl), l3 first
    laterals         dW, db = pod_conv1x1_wgrad(c_i, dL_i)
    below            only when the maps c3 - c5 require it (the ResNet trains: resnet_train.py): dC_i = dL_i W_lateral_i, the GEMM with the
                     transposed filter on pod_conv1x1_split, and for c5 also pod_col2im3x3s2_cl(dP6 W9(p6)), ungated -- the gate of a map is its
                     producer's and is applied there.  Otherwise nothing reaches below the laterals and p6, and nothing more is launched.
GPU only -- anything this path cannot take raises (hip.PodError): there is no fallback."""
from typing import List, Sequence, Tuple

import torch

from . import amax, conv1x1, hip, modeling, wgrad, wino
from .head_train import backward_gemm, conv_params, flat_grads, flipped3x3, patch_matrix, transposed1x1, transposed3x3s2


def fpn_convs(fpn) -> list:
    """The FPN's eight convolutions in the order their parameters enter the autograd function."""
    return list(fpn.lateral) + list(fpn.output) + [fpn.p6, fpn.p7]


def _require(fpn) -> None:
    K, S2 = fpn.p6.out_channels, conv1x1.Conv3x3S2
    ok = (len(fpn.lateral) == 3 and fpn.cl_eligible() and modeling.HIP_P6P7 and modeling.WINO_BACKBONE and bool(wino.SPLIT_BF16)
          and S2.eligible(fpn.p6) and S2.eligible(fpn.p7) and fpn.p6.bias is not None and fpn.p7.bias is not None
          and all(c.out_channels == K for c in fpn_convs(fpn)) and fpn.p7.in_channels == K and 9 * fpn.p6.in_channels <= 18432)
    if not ok:
        raise hip.PodError("fpn_forward_train: this FPN has no HIP training path (three biased 1x1 laterals of Cin % 16 == 0, 3x3 output convs and "
                           "stride-2 p6 / p7 of one width in (64, 128, 256, 512), the split kernels selected)")


def _cols(x: torch.Tensor, h: int, w: int, relu: bool, out: torch.Tensor) -> None:
    hip.check(hip.load().pod_im2col3x3s2_cl(x.data_ptr(), out.data_ptr(), int(h), int(w), int(x.shape[1]), 1 if relu else 0, hip.current_stream()),
              "pod_im2col3x3s2_cl")


def _batched_cols(maps: Sequence[torch.Tensor], h: int, w: int, relu: bool) -> torch.Tensor:
    """The patch matrices of B maps of one size, image after image (the images' own abs-max records bound them: entries are theirs or zero)."""
    ho, wo, C = (h - 1) // 2 + 1, (w - 1) // 2 + 1, int(maps[0].shape[1])
    cols = torch.empty((len(maps) * ho * wo, 9 * C), dtype=torch.float32, device=maps[0].device)
    for b, m in enumerate(maps):
        _cols(m, h, w, relu, cols[b * ho * wo:(b + 1) * ho * wo])
    return amax.joined(cols, *maps)


def _stacked(maps: Sequence[torch.Tensor]) -> torch.Tensor:
    return amax.joined(torch.cat(list(maps)), *maps)


def _grad_cl(g, B: int, K: int, h: int, w: int, device) -> torch.Tensor:
    """A level's gradient (B, K, h, w), any strides, or None -> channels-last (B h w, K), a tensor of this pass's own."""
    if g is None:
        return torch.zeros((B * h * w, K), dtype=torch.float32, device=device)
    out = torch.empty((B * h * w, K), dtype=torch.float32, device=device)
    out.view(B, h, w, K).copy_(g.permute(0, 2, 3, 1))
    return out


class _FpnTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fpn, feats, n_maps, *tensors):
        # tensors: the n_maps maps of `feats`, image-major (so that autograd sees them: they may carry the ResNet's grad_fn), then the parameters
        params = tensors[n_maps:]
        saved, per_image = [], []
        for f in feats:
            keep = {}
            outs = fpn.forward_cl(f, keep=keep)
            if not keep.get("hip_p6p7"):
                raise hip.PodError("fpn_forward_train: p6 / p7 did not take the pod_im2col3x3s2_cl + pod_conv1x1_split path")
            hw = [tuple(int(s) for s in o.shape[-2:]) for o in outs]
            p6 = outs[3].permute(0, 2, 3, 1).reshape(hw[3][0] * hw[3][1], -1).clone()  # (a copy: a view would hold the image's five-level buffer until backward)
            saved.append(dict(c=[t for t, _, _ in f], l=[keep["l3"], keep["l4"], keep["l5"]], p6=p6))
            per_image.append(outs)
        ctx.state = (fpn, saved, hw)
        ctx.n_params = len(params)
        return tuple(torch.cat([o[l] for o in per_image]).contiguous() for l in range(5))

    @staticmethod
    def backward(ctx, *g_levels):
        fpn, saved, hw = ctx.state
        B, K, dev = len(saved), fpn.p6.out_channels, saved[0]["p6"].device
        dP = [_grad_cl(g, B, K, h, w, dev) for g, (h, w) in zip(g_levels, hw)]
        (h5, w5), (h6, w6), (h7, w7) = hw[2], hw[3], hw[4]
        grads = {}

        # p7 on relu(p6): weight gradient on the patch matrix, dcols = dP7 W9, gathered back onto p6 behind the gate, plus p6's own gradient
        p6s = [s["p6"] for s in saved]
        dW, db = wgrad.conv1x1_wgrad(_batched_cols(p6s, h6, w6, True), dP[4])
        grads[fpn.p7] = (dW.view(K, 3, 3, K).permute(0, 3, 1, 2).contiguous(), db)
        dcols = backward_gemm(fpn.p7, transposed3x3s2)(dP[4], B * h7 * w7, 1)
        wgrad.over_images(B, dP[3], lambda b, rows, rec: wgrad.col2im3x3s2_cl(rows(dcols), h6, w6, gate=p6s[b], add=rows(dP[3]), out=rows(dP[3]), record=rec))
        # p6 on c5
        C5 = fpn.p6.in_channels
        dW, db = wgrad.conv1x1_wgrad(_batched_cols([s["c"][2] for s in saved], h5, w5, False), dP[3])
        grads[fpn.p6] = (dW.view(K, 3, 3, C5).permute(0, 3, 1, 2).contiguous(), db)
        # output convs: K22 for the weights, the GEMM of the gradient's patch matrix for the summed laterals' gradient
        dL = []
        for i in range(3):
            level, conv = [hw[i]], fpn.output[i]
            grads[conv] = wgrad.conv3x3_wgrad(_stacked([s["l"][i] for s in saved]), dP[i], level, B, K)
            dL.append(backward_gemm(conv, flipped3x3)(patch_matrix(dP[i], level, B), int(dP[i].shape[0]), 1))
        # top-down, l3 first: a summed lateral's gradient also reaches the coarser one it was upsampled from
        for i in (0, 1):
            (h, w), child, top = hw[i], dL[i], dL[i + 1]
            wgrad.over_images(B, top, lambda b, rows, rec: wgrad.upsample2_sum_cl(rows(child), h, w, rows(top), record=rec))
        # laterals
        for i in range(3):
            dW, db = wgrad.conv1x1_wgrad(_stacked([s["c"][i] for s in saved]), dL[i])
            grads[fpn.lateral[i]] = (dW.view(K, -1, 1, 1), db)
        # below the FPN, where the maps ask for it: every lateral's input gradient, and p6's on c5
        d_maps = [None] * (3 * B)
        if any(ctx.needs_input_grad[3:3 + 3 * B]):
            for i in range(3):
                (h, w), n = hw[i], hw[i][0] * hw[i][1]
                dC = backward_gemm(fpn.lateral[i], transposed1x1)(dL[i], B * n, 1)
                if i == 2:
                    dcols = backward_gemm(fpn.p6, transposed3x3s2)(dP[3], B * h6 * w6, 1)
                    wgrad.over_images(B, dC, lambda b, rows, rec: wgrad.col2im3x3s2_cl(rows(dcols), h, w, add=rows(dC), out=rows(dC), record=rec))
                for b in range(B):
                    d_maps[3 * b + i] = dC[b * n:(b + 1) * n]
        tap = getattr(fpn, "train_tap", None)               # tests: a dict that receives what this pass hands below the FPN
        if tap is not None:
            tap["d_maps"] = list(d_maps)
        flat = flat_grads(fpn_convs(fpn), grads)
        assert len(flat) == ctx.n_params
        ctx.state = None
        return (None, None, None) + tuple(d_maps) + tuple(flat)


def fpn_forward_train(fpn, feats: Sequence[Sequence[Tuple[torch.Tensor, int, int]]]) -> List[torch.Tensor]:
    """feats: per image the [(c3, h, w), (c4, h, w), (c5, h, w)] of ResNet50.forward_cl, B images of one padded size.  Returns the per-level
    (B, K, H, W) features; they carry a grad_fn that reaches every parameter of the FPN and, where the maps require grad (resnet_train's),
    the maps; otherwise nothing below it."""
    feats = [list(f) for f in feats]
    if not feats or any(len(f) != 3 for f in feats):
        raise hip.PodError("fpn_forward_train: per image the three maps (c3, h, w), (c4, h, w), (c5, h, w)")
    dev = getattr(feats[0][0][0], "device", None)
    for i, conv in enumerate(fpn.lateral):
        wgrad.require_maps("fpn_forward_train", [f[i] for f in feats], conv.in_channels, dev)
    _require(fpn)
    (h3, w3), (h4, w4), (h5, w5) = [(int(h), int(w)) for _, h, w in feats[0]]
    for (ht, wt), (h, w) in (((h4, w4), (h3, w3)), ((h5, w5), (h4, w4))):
        if (ht, wt) != ((h + 1) // 2, (w + 1) // 2):
            raise hip.PodError("fpn_forward_train: a top-down step from {} x {} to {} x {} is not a factor of two".format(ht, wt, h, w))
    if fpn.p6.weight.device != dev:
        raise hip.PodError("fpn_forward_train: the FPN is on {}, the maps on {}".format(fpn.p6.weight.device, dev))
    with torch.cuda.device(dev):
        maps = [t for f in feats for t, _, _ in f]
        return list(_FpnTrain.apply(fpn, feats, len(maps), *maps, *conv_params(fpn_convs(fpn))))


def backbone_maps(model, image: torch.Tensor, padded=None):
    """The frozen backbone of one frame, channels-last: ([(c3, h, w), (c4, h, w), (c5, h, w)], padded (h, w)) -- the part of
    ProbabilisticRetinaNet._trunk_eager ahead of the FPN (`_backbone_cl`).  padded: the batch's common padded size (None: the frame's own)."""
    with torch.no_grad():
        maps = model._backbone_cl(image, padded) if image.is_cuda else None
    if maps is None:
        raise hip.PodError("training the FPN needs the channels-last HIP backbone (a frame on the model's GPU, FrozenBN folded, the split kernels selected)")
    return maps
