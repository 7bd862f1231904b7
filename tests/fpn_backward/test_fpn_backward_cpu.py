"""CPU side of the FPN's backward pass: the declarations of K23's entry points, the slice rule of its partials query, the fp64
identities the backward rests on, and the command's new flag.  No GPU."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from pod_compare_amd import hip
from tests.fpn_backward import fb

NEW = ("pod_conv1x1_wgrad", "pod_conv1x1_wgrad_partials", "pod_col2im3x3s2_cl", "pod_upsample2_sum_cl")


def test_header_binding_and_library_carry_the_fpn_backward_entry_points():
    """Additions only: the symbols are declared, bound and exported; the ABI number stays 18."""
    from pod_compare_amd import build
    from tests.test_abi_cpu import HEADER, declared_symbols
    for name in NEW:
        assert name in hip.EXPORTS and name in declared_symbols()
    assert "pod_conv1x1_wgrad_partials" in hip._SIZE_QUERIES
    assert hip.POD_ABI_VERSION == 18 and "#define POD_ABI_VERSION 18\n" in open(HEADER).read()
    lib = ctypes.CDLL(build.build_library())
    assert lib.pod_abi_version() == hip.POD_ABI_VERSION and all(hasattr(lib, n) for n in NEW)
    assert "k23_fpn_backward.hip" in build.SOURCES and "-fno-slp-vectorize" in build.SOURCE_FLAGS["k23_fpn_backward.hip"]
    bound = hip.load()
    assert bound.pod_conv1x1_wgrad_partials.restype is ctypes.c_int64 and len(bound.pod_conv1x1_wgrad.argtypes) == 11
    assert len(bound.pod_col2im3x3s2_cl.argtypes) == 9 and len(bound.pod_upsample2_sum_cl.argtypes) == 8


def test_partials_query_is_a_function_of_the_geometry():
    """db partials over chunks of 4096 pixels, then a whole number of (K, C) slices -- whatever the slice length is, it follows from
    (pixels, C, K) alone; 0 = invalid geometry."""
    q = hip.load().pod_conv1x1_wgrad_partials
    for pixels, C, K in ((4117, 80, 64), (6, 18432, 64), (32256, 512, 256), (2016, 2048, 256), (1, 16, 64)):
        n = q(pixels, C, K)
        rest = n - 2 * ((pixels + 4095) // 4096) * K
        assert n == q(pixels, C, K) and rest >= K * C and rest % (K * C) == 0, (pixels, C, K, n)
        assert rest // (K * C) <= pixels                                   # no slice without a pixel
    for bad in ((0, 16, 64), (5, 24, 64), (5, 16, 32), (5, 16, 576), (5, 18448, 64), (5, 8, 64)):
        assert q(*bad) == 0, bad


def test_null_and_misaligned_arguments_are_refused_before_any_launch():
    lib = hip.load()
    assert lib.pod_conv1x1_wgrad(None, None, 16, 16, 64, None, None, None, None, None, None) == -1
    assert lib.pod_conv1x1_wgrad(16, 16, 0, 16, 64, 16, 16, 16, 16, 16, None) == -1          # no pixels
    assert lib.pod_conv1x1_wgrad(8, 16, 16, 16, 64, 16, 16, 16, 16, 16, None) == -1          # x not 16-byte aligned
    # what pod_conv1x1_wgrad_strided refuses, every weight gradient refuses.  Pointers that are never dereferenced, distinct but for the defect
    good = dict(x=0x1000, dy=0x2000, xa=0x3000, da=0x3800, dW=0x4000, db=0x5000, part=0x6000)
    call = lambda **kw: (lambda a: lib.pod_conv1x1_wgrad(a["x"], a["dy"], 16, 16, 64, a["xa"], a["da"], a["dW"], a["db"], a["part"], None))({**good, **kw})
    assert call(dW=good["x"]) == -1 and call(dW=good["part"]) == -1 and call(db=good["dW"]) == -1              # aliased
    assert call(dW=good["dy"]) == -1 and call(part=good["x"]) == -1 and call(part=good["dy"]) == -1 and call(db=good["part"]) == -1
    assert call(xa=0x3002) == -1 and call(da=0x3802) == -1 and call(dW=0x4002) == -1 and call(db=0x5002) == -1  # a record or output off 4 bytes
    assert call(x=0x1008) == -1 and call(part=0x6008) == -1 and call(xa=None) == -1 and call(part=None) == -1
    assert lib.pod_col2im3x3s2_cl(None, None, None, None, 4, 4, 16, None, None) == -1
    assert lib.pod_col2im3x3s2_cl(16, None, None, 32, 4, 4, 6, None, None) == -1             # C % 4
    assert lib.pod_col2im3x3s2_cl(16, None, None, 16, 4, 4, 16, None, None) == -1            # in place on dcols
    assert lib.pod_upsample2_sum_cl(16, 4, 4, None, 32, 16, None, None) == -1                # add is not optional
    assert lib.pod_upsample2_sum_cl(16, 0, 4, 32, 32, 16, None, None) == -1


@pytest.mark.parametrize("h,w", [(5, 6), (4, 7), (1, 1)])
def test_patch_matrix_weight_gradient_and_col2im_are_the_stride2_convs_gradients(h, w):
    """What steps 1 and 2 of the backward rest on, in fp64: with cols = the patch matrix of relu(x), dW = (dY.T @ cols) re-laid from
    (K, ty, tx, C) and dx = gate * col2im(dY @ W9) equal autograd through conv2d(relu(x), W, stride 2, padding 1)."""
    g = torch.Generator().manual_seed(h * 8 + w)
    C, K = 8, 4
    x = torch.randn((h * w, C), generator=g, dtype=torch.float64)
    W = torch.randn((K, C, 3, 3), generator=g, dtype=torch.float64, requires_grad=True)
    planes = x.view(1, h, w, C).permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.conv2d(F.relu(planes), W, stride=2, padding=1)
    ho, wo = y.shape[-2:]
    assert (ho, wo) == ((h - 1) // 2 + 1, (w - 1) // 2 + 1)
    dy = torch.randn((ho * wo, K), generator=g, dtype=torch.float64)
    y.backward(dy.view(1, ho, wo, K).permute(0, 3, 1, 2))
    cols = fb.patch_rows(x, h, w, relu=True)
    dW, _ = fb.ref_wgrad(cols, dy, torch.float64)
    assert float((dW.view(K, 3, 3, C).permute(0, 3, 1, 2) - W.grad).abs().max()) <= 1e-12 * max(1.0, float(W.grad.abs().max()))
    dcols = dy @ W.detach().permute(0, 2, 3, 1).reshape(K, 9 * C)
    dx = fb.ref_col2im(dcols, h, w, gate=x)
    want = planes.grad.permute(0, 2, 3, 1).reshape(h * w, C)
    assert float((dx - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_train_head_accepts_train_fpn(capsys):
    from pod_compare_amd import train_head
    with pytest.raises(SystemExit) as e:
        train_head.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--train-fpn" in text and "ResNet stays frozen" in " ".join(text.split())
    import inspect
    assert inspect.signature(train_head.HeadTrainer.__init__).parameters["train_fpn"].default is False
    assert inspect.signature(train_head.save_checkpoint).parameters["train_fpn"].default is False
