"""The kernels' forms of an nn.Conv2d's parameters -- the Winograd-transformed filter, the split 1x1 / 7x7 / patch-matrix weights -- made once
and cached on the conv, rebuilt when its parameters are modified or moved.  A leaf module: the model (modeling.py) and the backward passes
(head_train.py, fpn_train.py) all look their forms up here."""
import torch
from torch import nn

from . import conv1x1, wino


def derived(conv: nn.Conv2d, attr: str, make, *extra_key):
    """make(conv) -- a kernel's form of the conv's parameters -- cached on the conv as `attr`, rebuilt when the parameters (or extra_key) change."""
    w, b = conv.weight, conv.bias
    key = (w.data_ptr(), w._version, None if b is None else (b.data_ptr(), b._version)) + extra_key
    cached = getattr(conv, attr, None)
    if cached is None or cached[0] != key:
        cached = (key, make(conv))
        torch.cuda.current_stream(w.device).synchronize()      # made once, then read from any stream
        setattr(conv, attr, cached)
    return cached[1]


def wino_of(conv: nn.Conv2d):
    """The conv's Winograd-transformed filter (pod_wino_filter_transform), refreshed when the parameters change."""
    return derived(conv, "_pod_wino", lambda c: wino.WinoConv(c.weight, c.bias), wino.SPLIT_BF16)


def c1_of(conv: nn.Conv2d):
    """The conv's pod_conv1x1_split form (weight split once), refreshed when the parameters change."""
    return derived(conv, "_pod_c1", lambda c: conv1x1.Conv1x1(c.weight, c.bias, c.stride[0]))


def stem_of(conv: nn.Conv2d):
    """The stem conv's pod_stem7x7_split form (weight split once), refreshed when the parameters change."""
    return derived(conv, "_pod_stem", lambda c: conv1x1.Stem7x7(c.weight, c.bias))


def s2_of(conv: nn.Conv2d):
    """The conv's im2col + pod_conv1x1_split form (3x3 / stride 2: FPN's p6 / p7; weight re-laid and split once), refreshed when the parameters change."""
    return derived(conv, "_pod_s2", lambda c: conv1x1.Conv3x3S2(c.weight, c.bias))
