"""CPU side of the ResNet's backward pass: the declarations of K24's entry points, its partials query, the refusals that come before
any launch, the command's new flag, and the fp64 identity the backward of a conv-shortcut block rests on.  No GPU."""
import ctypes
import inspect

import pytest
import torch
import torch.nn.functional as F

from pod_compare_amd import hip, modeling
from tests.resnet_backward import rb

NEW = ("pod_conv1x1_wgrad_strided_partials", "pod_conv1x1_wgrad_strided", "pod_subsample2_scatter_cl")


def test_header_binding_and_library_carry_the_resnet_backward_entry_points():
    """Additions only: the symbols are declared, bound and exported; the ABI number stays 18."""
    from pod_compare_amd import build
    from tests.test_abi_cpu import HEADER, declared_symbols
    for name in NEW:
        assert name in hip.EXPORTS and name in declared_symbols()
    assert "pod_conv1x1_wgrad_strided_partials" in hip._SIZE_QUERIES
    assert hip.POD_ABI_VERSION == 18 and "#define POD_ABI_VERSION 18\n" in open(HEADER).read()
    lib = ctypes.CDLL(build.build_library())
    assert lib.pod_abi_version() == hip.POD_ABI_VERSION and all(hasattr(lib, n) for n in NEW)
    assert "k24_resnet_backward.hip" in build.SOURCES and "-fno-slp-vectorize" in build.SOURCE_FLAGS["k24_resnet_backward.hip"]
    bound = hip.load()
    assert bound.pod_conv1x1_wgrad_strided_partials.restype is ctypes.c_int64 and len(bound.pod_conv1x1_wgrad_strided_partials.argtypes) == 6
    assert len(bound.pod_conv1x1_wgrad_strided.argtypes) == 14 and len(bound.pod_subsample2_scatter_cl.argtypes) == 9


def test_partials_query_is_a_function_of_the_geometry():
    """db partials over chunks of 4096 OUTPUT pixels, then a whole number of (K, C) slices; on the same output pixels the query is
    pod_conv1x1_wgrad's, so the slices are the same; 0 = invalid geometry."""
    lib = hip.load()
    q, q1 = lib.pod_conv1x1_wgrad_strided_partials, lib.pod_conv1x1_wgrad_partials
    for images, h, w, stride, C, K in ((3, 17, 25, 2, 80, 64), (2, 5, 7, 2, 1024, 2048), (2, 3, 4, 1, 512, 2048), (1, 1, 1, 2, 16, 64), (4, 90, 160, 1, 128, 512)):
        ho, wo = rb.out_hw(h, w, stride)
        pixels = images * ho * wo
        n = q(images, h, w, stride, C, K)
        rest = n - 2 * ((pixels + 4095) // 4096) * K
        assert n == q(images, h, w, stride, C, K) and rest >= K * C and rest % (K * C) == 0, (images, h, w, stride, C, K, n)
        assert rest // (K * C) <= pixels                                   # no slice without a pixel
        if K <= 512:
            assert n == q1(pixels, C, K)
    for bad in ((2, 5, 7, 2, 1024, 2112), (2, 5, 7, 3, 64, 64), (2, 5, 7, 2, 72, 64), (0, 5, 7, 2, 64, 64), (2, 0, 7, 1, 64, 64), (2, 5, 7, 0, 64, 64),
                (2, 5, 7, 2, 64, 32), (2, 5, 7, 1, 18448, 64), (70000, 128, 128, 2, 64, 64)):
        assert q(*bad) == 0, bad


def test_null_misaligned_and_aliased_arguments_are_refused_before_any_launch():
    """Host pointers that are never dereferenced: every call returns POD_E_INVALID from its argument checks."""
    lib = hip.load()
    w, s = lib.pod_conv1x1_wgrad_strided, lib.pod_subsample2_scatter_cl
    geo = (2, 5, 7, 2, 64, 64)
    assert w(None, None, *geo, None, None, None, None, None, None) == -1
    good = dict(x=0x1000, dy=0x2000, xa=0x3000, da=0x3800, dW=0x4000, db=0x5000, part=0x6000)
    call = lambda geometry=geo, **kw: (lambda a: w(a["x"], a["dy"], *geometry, a["xa"], a["da"], a["dW"], a["db"], a["part"], None))({**good, **kw})
    for name in ("x", "dy", "xa", "da", "dW", "part"):
        assert call(**{name: None}) == -1, name
    assert call(x=0x1008) == -1 and call(dy=0x2004) == -1 and call(part=0x6008) == -1 and call(dW=0x4002) == -1      # misaligned
    assert call(dW=good["x"]) == -1 and call(dW=good["dy"]) == -1 and call(part=good["dW"]) == -1 and call(db=good["dW"]) == -1   # aliased
    assert call(part=good["x"]) == -1 and call(db=good["part"]) == -1
    for bad in ((2, 5, 7, 3, 64, 64), (0, 5, 7, 2, 64, 64), (2, 5, 7, 2, 64, 2112), (2, 5, 7, 2, 24, 64)):
        assert call(geometry=bad) == -1, bad
    assert s(None, None, None, None, 4, 4, 16, None, None) == -1
    assert s(0x1000, None, None, None, 4, 4, 16, None, None) == -1
    assert s(0x1000, None, None, 0x2000, 4, 4, 6, None, None) == -1           # C % 4
    assert s(0x1000, None, None, 0x2000, 0, 4, 16, None, None) == -1
    assert s(0x1000, None, None, 0x1000, 4, 4, 16, None, None) == -1           # in place on d_small
    assert s(0x1000, 0x2000, None, 0x2000, 4, 4, 16, None, None) == -1         # the gate is read after dx is written
    assert s(0x1000, None, 0x3008, 0x2000, 4, 4, 16, None, None) == -1         # add not 16-byte aligned
    assert s(0x1000, None, None, 0x2000, 4, 4, 16, 0x3002, None) == -1         # the record not 4-byte aligned


def test_train_head_accepts_train_backbone(capsys):
    from pod_compare_amd import config, train_head
    with pytest.raises(SystemExit) as e:
        train_head.main(["--help"])
    assert e.value.code == 0
    text = " ".join(capsys.readouterr().out.split())
    assert "--train-backbone" in text and "the stem and res2 stay frozen" in text           # (argparse breaks lines at hyphens)
    params = inspect.signature(train_head.HeadTrainer.__init__).parameters
    assert params["train_backbone"].default is False and params["shadow"].default is None
    assert inspect.signature(train_head.save_checkpoint).parameters["train_backbone"].default is False
    # the defaults do not name the freeze point (tests/golden/reference_configs.json pins the MODEL section): absent means detectron2's 2
    assert config.get_cfg().MODEL.BACKBONE.get("FREEZE_AT", 2) == 2


def test_only_the_default_freeze_point_is_accepted(tmp_path):
    from pod_compare_amd import train_head
    yaml = tmp_path / "m.yaml"
    yaml.write_text("MODEL:\n  BACKBONE:\n    FREEZE_AT: 3\n")
    (tmp_path / "gt.json").write_text('{"images": [], "annotations": []}')
    with pytest.raises(SystemExit) as e:
        train_head.main(["--config-file", str(yaml), "--coco-json", str(tmp_path / "gt.json"), "--image-root", str(tmp_path), "--train-backbone"])
    assert "FREEZE_AT = 3 is not supported" in str(e.value)


def test_trainable_convs_are_those_of_res3_to_res5_in_block_order():
    from pod_compare_amd.resnet_train import trainable_convs, unfolded_pairs
    net = modeling.ResNet50()
    convs = trainable_convs(net)
    assert len(convs) == 3 * (4 + 6 + 3) + 3 and len(unfolded_pairs(net)) == len(convs)
    first = net.res3[0]
    assert convs[:4] == [first.shortcut[0], first.conv1[0], first.conv2[0], first.conv3[0]] and convs[4] is net.res3[1].conv1[0]
    assert convs[-1] is net.res5[2].conv3[0]
    frozen = {id(p) for part in (net.stem, net.res2) for p in part.parameters()}
    assert not frozen & {id(c.weight) for c in convs}


def test_the_conv_shortcut_blocks_backward_formulas_equal_fp64_autograd():
    """One conv-shortcut block (stride 2) at 5 x 7 on the ReLU output of a map p, which something else (the FPN) reads too.  In fp64: the
    strided weight-gradient formula is autograd's gradient of the two stride-2 1x1 convs, and the scatter formula -- zeros off the even
    pixels, `add` inside the gate -- applied to dA W1 + dZ Ws is autograd's gradient at p."""
    g = torch.Generator().manual_seed(57)
    h, w, cin, mid, cout, B = 5, 7, 8, 4, 16, 2
    block = modeling.Bottleneck(cin, cout, mid, 2).double()
    with torch.no_grad():
        rb.randomise_frozen_bn(block, g)
    p = torch.randn((B, cin, h, w), generator=g, dtype=torch.float64, requires_grad=True)
    x = F.relu(p)
    y = block(x)
    ho, wo = rb.out_hw(h, w, 2)
    assert tuple(y.shape) == (B, cout, ho, wo) == (B, cout, 3, 4)
    cot = torch.randn(y.shape, generator=g, dtype=torch.float64)
    from_fpn = torch.randn(p.shape, generator=g, dtype=torch.float64)
    ((y * cot).sum() + (x * from_fpn).sum()).backward()

    # the same by hand, channels-last, on the folded filters W' = W s
    def folded(m):
        conv, bn = m[0], m[1]
        s = bn.weight * (bn.running_var + bn.eps).rsqrt()
        return (conv.weight.detach() * s.reshape(-1, 1, 1, 1)), (bn.bias - bn.running_mean * s), s
    (Ws, bs, ss), (W1, b1, s1), (W2, b2, s2), (W3, b3, s3) = folded(block.shortcut), folded(block.conv1), folded(block.conv2), folded(block.conv3)
    xd = x.detach()
    a = F.relu(F.conv2d(xd, W1, b1, stride=2))
    b = F.relu(F.conv2d(a, W2, b2, padding=1))
    yy = F.relu(F.conv2d(b, W3, b3) + F.conv2d(xd, Ws, bs, stride=2))
    assert float((yy - y.detach()).abs().max()) <= 1e-12
    x_cl, a_cl, b_cl = rb.to_cl(xd), rb.to_cl(a), rb.to_cl(b)
    dz = rb.to_cl(cot) * (rb.to_cl(yy) > 0)
    dW3 = rb.ref_wgrad_strided(b_cl, dz, B, ho, wo, 1, torch.float64)
    db_ = (dz @ W3.reshape(cout, mid)) * (b_cl > 0)
    dW2 = torch.nn.grad.conv2d_weight(a, W2.shape, db_.view(B, ho, wo, mid).permute(0, 3, 1, 2), padding=1)
    da = rb.to_cl(torch.nn.grad.conv2d_input(a.shape, W2, db_.view(B, ho, wo, mid).permute(0, 3, 1, 2), padding=1)) * (a_cl > 0)
    dW1 = rb.ref_wgrad_strided(x_cl, da, B, h, w, 2, torch.float64)
    dWs = rb.ref_wgrad_strided(x_cl, dz, B, h, w, 2, torch.float64)
    half = da @ W1.reshape(mid, cin) + dz @ Ws.reshape(cout, cin)
    n, nh = h * w, ho * wo
    dp = torch.cat([rb.ref_scatter(half[i * nh:(i + 1) * nh], h, w, gate=rb.to_cl(p.detach())[i * n:(i + 1) * n], add=rb.to_cl(from_fpn)[i * n:(i + 1) * n])
                    for i in range(B)])
    close = lambda got, want: float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert close(dp, rb.to_cl(p.grad))
    # W.grad = s dW': what FoldedMasters hands the optimiser
    for m, dWf, s in ((block.shortcut, dWs, ss), (block.conv1, dW1, s1), (block.conv2, dW2, s2), (block.conv3, dW3, s3)):
        assert close(dWf.reshape(m[0].weight.shape) * s.reshape(-1, 1, 1, 1), m[0].weight.grad)
