"""What MODEL.BACKBONE.FREEZE_AT 0 and 1 need that no GPU is needed to check: the conv lists per freeze point, the command's handling of
the key, the declarations of K30's entries, and the pool's first-max rule as the GPU tests' referee restates it."""
import pytest
import torch
import torch.nn.functional as F

from pod_compare_amd import hip, modeling, train_head
from pod_compare_amd.resnet_train import block_convs, trainable_blocks, trainable_convs, unfolded_pairs
from tests.stem_backward import sb

NEW = ("pod_stem7x7_wgrad_partials", "pod_stem7x7_wgrad", "pod_maxpool3x3s2_backward_cl")


def test_trainable_convs_per_freeze_point():
    net = modeling.ResNet50()
    at2, at1, at0 = trainable_convs(net), trainable_convs(net, 1), trainable_convs(net, 0)
    assert (len(at2), len(at1), len(at0)) == (42, 52, 53)
    assert all(a is b for a, b in zip(at2, trainable_convs(net, 2))) and len(trainable_convs(net, 2)) == 42       # the default is what it was
    res2 = [c for block in net.res2 for c in block_convs(block)]
    assert len(res2) == 10 and res2[0] is net.res2[0].shortcut[0] and res2[1] is net.res2[0].conv1[0] and res2[-1] is net.res2[2].conv3[0]
    assert all(a is b for a, b in zip(at1, res2 + at2))                       # res2 in block order, then today's 42
    assert at0[0] is net.stem[0] and all(a is b for a, b in zip(at0[1:], at1))  # the stem first
    for fa, convs in ((2, at2), (1, at1), (0, at0)):
        pairs = unfolded_pairs(net, fa)
        assert len(pairs) == len(convs) and all(p[0] is c and isinstance(p[1], modeling.FrozenBatchNorm2d) for p, c in zip(pairs, convs))
    assert len(trainable_blocks(net)) == 13 and len(trainable_blocks(net, 1)) == len(trainable_blocks(net, 0)) == 16
    assert train_head.trained_parts(False, True) == ["head", "fpn", "backbone"]
    assert train_head.trained_parts(False, True, 1) == ["head", "fpn", "backbone", "res2"]
    assert train_head.trained_parts(False, True, 0) == ["head", "fpn", "backbone", "res2", "stem"]
    for bad in (3, -1):
        with pytest.raises(hip.PodError):
            trainable_convs(net, bad)


def _main_exit(tmp_path, freeze_at, *flags) -> str:
    yaml = tmp_path / "m.yaml"
    yaml.write_text("MODEL:\n  BACKBONE:\n    FREEZE_AT: %d\n" % freeze_at)
    (tmp_path / "gt.json").write_text('{"images": [], "annotations": []}')
    try:
        train_head.main(["--config-file", str(yaml), "--coco-json", str(tmp_path / "gt.json"), "--image-root", str(tmp_path), "--device", "cpu",
                         "--random-init", "--max-iter", "0", "--output-dir", str(tmp_path / "out")] + list(flags))
    except SystemExit as e:
        return str(e)
    except Exception as e:                               # past the check: whatever a machine without a GPU or data fails on later
        return "%s: %s" % (type(e).__name__, e)
    return ""


@pytest.mark.parametrize("freeze_at", [0, 1])
def test_a_lower_freeze_point_without_train_backbone_names_the_flag(tmp_path, freeze_at):
    msg = _main_exit(tmp_path, freeze_at)
    assert "FREEZE_AT = %d" % freeze_at in msg and "--train-backbone" in msg


def test_freeze_points_above_2_stay_refused(tmp_path):
    for flags in ((), ("--train-backbone",)):
        assert "FREEZE_AT = 3 is not supported" in _main_exit(tmp_path, 3, *flags)


def test_freeze_point_1_with_train_backbone_passes_the_check(tmp_path):
    msg = _main_exit(tmp_path, 1, "--train-backbone")
    assert "FREEZE_AT" not in msg, msg


def test_the_help_text_says_what_the_key_does():
    text = train_head.arg_parser().format_help()
    assert "the stem and res2 stay" in " ".join(text.split()) and "FREEZE_AT" in text


def test_header_and_binding_carry_k30():
    from tests.test_abi_cpu import declared_symbols
    for name in NEW:
        assert name in hip.EXPORTS and name in declared_symbols()
    assert "pod_stem7x7_wgrad_partials" in hip._SIZE_QUERIES


def test_the_first_max_rule_is_torchs_on_a_tied_map():
    """Pins the referee, not the kernel: on maps full of ties (three levels, odd extents, windows cut at every border) the restated rule --
    row-major scan of the in-bounds pixels, a new maximum only on strict > -- gives F.max_pool2d's indices."""
    g = torch.Generator().manual_seed(7)
    for h, w in ((7, 9), (8, 8), (1, 5)):
        planes = torch.randint(0, 3, (2, 4, h, w), generator=g).float()
        _, idx = F.max_pool2d(planes, 3, 2, 1, return_indices=True)
        assert torch.equal(sb.first_max_indices(planes), idx)
        pooled = sb.routed_pool(planes, idx)
        assert torch.equal(pooled, F.max_pool2d(planes, 3, 2, 1))
