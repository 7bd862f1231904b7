"""The head with a backward pass: ProbabilisticRetinaNetHead.forward_train (probabilistic_retinanet.py:403-537 in training mode, under
train_net.py's loop) as ONE torch.autograd.Function over the whole head.

Forward: the training form of the launch plan the inference head runs (modeling.ProbabilisticRetinaNetHead._trunk_plan, `_predict`), all
B images in every launch.  Backward, per layer from the predictors down:
    the gate         dZ = dOut (out > 0) / (1 - p)       pod_relu_dropout_backward (the stored output is its own mask; trunk layers only)
    dW, db           pod_conv3x3_wgrad(saved input, dZ)   K22, handed to autograd, which accumulates them into .grad
    dX               conv3x3(dZ, W'), W'[c][k][ky][kx] = W[k][c][2 - ky][2 - kx], as a GEMM: the patch matrix of dZ (torch) times the split
                     W' on pod_conv1x1_split (direct sums: the Winograd kernel's transforms round three times as much per layer)
A predictor's A*K = 63 / 36 gradient channels are zero-padded to 64 (and W' with them): Cin % 16 == 0.  The two predictors
on a trunk add their dX ahead of the trunk's last gate.  Only the head trains: the features' gradient is computed when they require it,
and nothing reaches further down.  GPU only -- anything this path cannot take raises (hip.PodError): there is no fallback."""
from typing import List, Optional, Sequence

import torch

from . import amax, conv1x1, conv_forms, hip, modeling, wgrad
from .synthetic import HeadOutputs


def head_convs(head) -> list:
    """The head's convolutions in the order their parameters enter the autograd function."""
    return (list(head.cls_subnet) + list(head.bbox_subnet) + [head.cls_score, head.bbox_pred]
            + [c for c in (head.cls_var, head.bbox_cov) if c is not None])


def transposed_weight(weight: torch.Tensor) -> torch.Tensor:
    """W (K, C, 3, 3) -> W' (C, Kpad, 3, 3), W'[c][k][ky][kx] = W[k][c][2 - ky][2 - kx], K zero-padded to a multiple of 64:
    conv3x3(dZ, W') is the input gradient of conv3x3(., W)."""
    K, C = int(weight.shape[0]), int(weight.shape[1])
    wt = torch.zeros((C, (K + 63) // 64 * 64, 3, 3), dtype=weight.dtype, device=weight.device)
    wt[:, :K] = weight.detach().flip(2, 3).transpose(0, 1)
    return wt


def flipped3x3(conv) -> torch.Tensor:
    """Layout of backward_gemm: a 3x3 / stride-1 conv's W' as (C, ty, tx, Kpad) rows, against the patch matrix of dZ."""
    wt = transposed_weight(conv.weight)
    return wt.permute(0, 2, 3, 1).reshape(wt.shape[0], 9 * wt.shape[1], 1, 1)


def transposed1x1(conv) -> torch.Tensor:
    """Layout of backward_gemm: dX = dY W for a 1x1 conv's (K, C) filter."""
    return conv.weight.detach().reshape(conv.out_channels, conv.in_channels).t().reshape(conv.in_channels, conv.out_channels, 1, 1)


def transposed3x3s2(conv) -> torch.Tensor:
    """Layout of backward_gemm: dcols = dY W9, W9 (K, ty, tx, Cin) a stride-2 conv's filter in the patch matrix's column order."""
    return conv.weight.detach().permute(0, 2, 3, 1).reshape(conv.out_channels, -1).t().reshape(9 * conv.in_channels, conv.out_channels, 1, 1)


def backward_gemm(conv, layout, negated: bool = False):
    """The conv's input gradient as a GEMM on pod_conv1x1_split: layout(conv) -- flipped3x3, transposed1x1 or transposed3x3s2 -- is the
    rearranged (Cin', Cout', 1, 1) filter, split once and cached by the weight's version (conv_forms.derived), one form per layout and sign.
    Called as gemm(dY (pixels, Cin'), pixels, 1[, residual=...]) -> (pixels, Cout').  negated: the same with the negated filter (every f16
    term and product the exact negative: the accumulation's error alone differs; resnet_train.centred uses the pair)."""
    def make(c):
        w = layout(c).contiguous()
        try:
            return conv1x1.Conv1x1(-w if negated else w, None, 1)
        except ValueError as e:
            raise hip.PodError("backward: the input gradient ({}) of a {} -> {} conv has no pod_conv1x1_split form ({})".format(
                layout.__name__, c.in_channels, c.out_channels, e))
    return conv_forms.derived(conv, "_pod_bwd_{}{}".format(layout.__name__, "_neg" if negated else ""), make)


def conv_params(convs, bias: bool = True) -> list:
    """The convs' parameters in the order they enter an autograd function (bias=False: the weights alone)."""
    return [p for c in convs for p in ((c.weight, c.bias) if bias else (c.weight,))]


def flat_grads(convs, grads: dict) -> list:
    """grads[conv] = one gradient per parameter conv_params lists, flattened in its order."""
    return [g for c in convs for g in grads[c]]


def patch_matrix(dz: torch.Tensor, levels, B: int) -> torch.Tensor:
    """(pixels, K) channels-last, level-major -> (pixels, 9 K): row (y, x) = the K-vectors of the nine taps in (ty, tx) order, zeros where a
    tap leaves its image (data movement only, plain torch; the record of dz bounds it)."""
    K = int(dz.shape[1])
    cols = torch.empty((int(dz.shape[0]), 9 * K), dtype=dz.dtype, device=dz.device)
    off = 0
    for h, w in levels:
        n = B * h * w
        v = torch.nn.functional.pad(dz[off:off + n].view(B, h, w, K), (0, 0, 1, 1, 1, 1))
        torch.cat([v[:, ty:ty + h, tx:tx + w] for ty in range(3) for tx in range(3)], dim=3, out=cols[off:off + n].view(B, h, w, 9 * K))
        off += n
    return amax.attach(cols, amax.of(dz))


def _planes_to_padded_cl(g: Optional[torch.Tensor], levels, B: int, K: int, device) -> torch.Tensor:
    """Gradient planes of one predictor -- flat, per level (B, K, H, W), level-major -- as the zero-padded channels-last (pixels, Kpad)."""
    Kpad, pixels = (K + 63) // 64 * 64, B * sum(h * w for h, w in levels)
    out = torch.zeros((pixels, Kpad), dtype=torch.float32, device=device)
    if g is None:
        return out
    off = 0
    for h, w in levels:
        n = B * h * w
        out[off:off + n, :K] = g[off * K:(off + n) * K].view(B, K, h, w).permute(0, 2, 3, 1).reshape(n, K)
        off += n
    return out


class _HeadTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, head, levels, B, x0, *params):
        if not all(conv_forms.wino_of(c).split for c in head_convs(head)):
            raise hip.PodError("head.forward_train needs the split Winograd kernel for every conv of the head (C % 16 == 0, POD_WINO_SPLIT=1)")
        x0 = x0.detach()
        # the training form of the head's launch plan (modeling._trunk_plan): B images per level, every layer's output kept; the tables'
        # channel bound covers the widest conv of the head (the full covariance predictor: 90 outputs, padded to 128)
        widest = max(conv_forms.wino_of(c).Kpad for c in head_convs(head))
        st = modeling.HeadPlan(x0=x0, levels=list(levels), dropout=False, grouped=True, images=int(B), channels=max(int(x0.shape[1]), 64, widest))
        last = [buf for buf, _ in head._trunks([(0, B), (1, B)], st)]
        saved = st.saved                                # saved[sid][l] = (input, output) of trunk layer l
        preds = [(head.cls_score, 0), (head.bbox_pred, 1)] + ([(head.cls_var, 0)] if head.cls_var is not None else []) + \
                ([(head.bbox_cov, 1)] if head.bbox_cov is not None else [])
        planes = head._predict([(conv, last[sid], B, 0, B, B) for conv, sid in preds], st, flat=True)
        tap = getattr(head, "train_tap", None)          # tests: a dict that receives the saved activations (and the gates' outputs)
        if tap is not None:
            tap["saved"], tap["dz"] = saved, {}
        ctx.state = (head, list(levels), int(B), x0, saved, preds, last)
        ctx.n_params = len(params)
        return tuple(planes)

    @staticmethod
    def backward(ctx, *g_planes):
        head, levels, B, x0, saved, preds, last = ctx.state
        dev, C, L = x0.device, int(x0.shape[1]), len(head.cls_subnet)
        pixels = int(x0.shape[0])
        grads = {}                                             # conv -> (dW, db)
        need_x = ctx.needs_input_grad[3]

        def input_grad(conv, dz):
            return backward_gemm(conv, flipped3x3)(patch_matrix(dz, levels, B), pixels, 1)

        d_trunk = [None, None]
        for (conv, sid), g in zip(preds, g_planes):
            dy = _planes_to_padded_cl(None if g is None else g.contiguous(), levels, B, conv.out_channels, dev)
            grads[conv] = wgrad.conv3x3_wgrad(last[sid], dy, levels, B, conv.out_channels)
            dx = input_grad(conv, dy)
            d_trunk[sid] = dx if d_trunk[sid] is None else d_trunk[sid] + dx
        dx0 = None
        for sid, sub in enumerate((head.cls_subnet, head.bbox_subnet)):
            d = d_trunk[sid]
            for l in range(L - 1, -1, -1):
                x_in, out = saved[sid][l]
                dz = wgrad.relu_dropout_backward(out, d, head.dropout_rate)          # in place; publishes dZ's abs-max record
                grads[sub[l]] = wgrad.conv3x3_wgrad(x_in, dz, levels, B, sub[l].out_channels)
                if getattr(head, "train_tap", None) is not None:
                    head.train_tap["dz"][(sid, l)] = dz
                if l or need_x:
                    d = input_grad(sub[l], dz)
            if need_x:
                dx0 = d if dx0 is None else dx0 + d
        flat = flat_grads(head_convs(head), grads)
        assert len(flat) == ctx.n_params
        ctx.state = None
        return (None, None, None, dx0) + tuple(flat)


def forward_train(head, features: Sequence[torch.Tensor], anchors: Optional[List[torch.Tensor]] = None, image_size=None) -> HeadOutputs:
    """features: per-level (B, C, H, W), B images of one padded size.  Returns HeadOutputs whose leading dimension is the image (what
    losses.ProbabilisticLosses expects); its tensors carry a grad_fn that reaches every parameter of the head and, where they require
    it, the features."""
    f0 = features[0]
    if not (f0.is_cuda and f0.dtype == torch.float32):
        raise hip.PodError("head.forward_train runs on the GPU in fp32 only (got {} on {}): there is no CPU path".format(f0.dtype, f0.device))
    B, C = int(f0.shape[0]), int(f0.shape[1])
    convs = head_convs(head)
    # C % 16: the split kernel, forward and (as the GEMM's Cin) backward; one of its four widths: a layer's output, unpadded, is the next one's input
    if C != head.cls_subnet[0].in_channels or C % 16 or C not in (64, 128, 256, 512) or any(c.bias is None for c in convs):
        raise hip.PodError("head.forward_train: {} input channels (conv {} -> {}) have no pod_wino_conv3x3_split form for both directions "
                           "(64, 128, 256 or 512 channels, biased convs)".format(C, head.cls_subnet[0].in_channels, head.cls_subnet[0].out_channels))
    levels = [(int(f.shape[2]), int(f.shape[3])) for f in features]
    if any(int(f.shape[0]) != B or int(f.shape[1]) != C or f.device != f0.device for f in features):
        raise hip.PodError("head.forward_train: every level holds the same images and channels")
    x0 = torch.cat([f.permute(0, 2, 3, 1).reshape(-1, C) for f in features]).contiguous()      # channels-last, level-major (autograd sees it)
    flats = _HeadTrain.apply(head, levels, B, x0, *conv_params(convs))
    A = head.num_anchors

    def per_level(flat, K):
        out, off = [], 0
        for h, w in levels:
            n = B * h * w * K
            out.append(flat[off:off + n].view(B, K, h, w))
            off += n
        return out

    it = iter(flats)
    cls, delta = per_level(next(it), head.cls_score.out_channels), per_level(next(it), head.bbox_pred.out_channels)
    cls_var = per_level(next(it), head.cls_var.out_channels) if head.cls_var is not None else None
    reg_var = per_level(next(it), head.bbox_cov.out_channels) if head.bbox_cov is not None else None
    h0, w0 = levels[0]
    return HeadOutputs(cls, delta, cls_var, reg_var, list(anchors) if anchors is not None else [], levels, A, head.num_classes,
                       tuple(image_size) if image_size is not None else (h0 * 8, w0 * 8))
