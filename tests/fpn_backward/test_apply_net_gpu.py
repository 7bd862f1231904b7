"""train_head --train-fpn as a command: it writes a checkpoint that loads back into a fresh model with the trained FPN and head."""
import json
import os

import numpy as np
import pytest
import torch

from pod_compare_amd import checkpoint, config, train_head
from pod_compare_amd.fpn_train import fpn_convs
from pod_compare_amd.head_train import head_convs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_train_head_with_train_fpn_writes_a_checkpoint_whose_fpn_moved(tmp_path):
    from PIL import Image
    from pod_compare_amd.probabilistic_inference import build_model
    rng = np.random.default_rng(3)
    images = []
    for k in range(2):
        Image.fromarray(rng.integers(0, 256, size=(64, 96, 3), dtype=np.uint8)).save(tmp_path / ("f%d.png" % k))
        images.append({"id": 40 + k, "file_name": "f%d.png" % k, "height": 64, "width": 96})
    anns = [{"id": 1, "image_id": 40, "category_id": 1, "bbox": [10, 8, 34, 32], "iscrowd": 0},
            {"id": 2, "image_id": 40, "category_id": 4, "bbox": [50, 20, 40, 40], "iscrowd": 0}]
    (tmp_path / "gt.json").write_text(json.dumps({"images": images, "annotations": anns}))
    out_dir = tmp_path / "out"
    yaml = os.path.join(os.path.dirname(train_head.__file__), "configs/BDD-Detection/retinanet/retinanet_R_50_FPN_1x.yaml")
    res = train_head.main(["--config-file", yaml, "--coco-json", str(tmp_path / "gt.json"), "--image-root", str(tmp_path), "--random-init", "--train-fpn",
                           "--output-dir", str(out_dir), "--max-iter", "2", "--log-period", "1", "--min-size-test", "64", "--max-size-test", "96",
                           "--loader-workers", "0", "--device", DEV])
    assert res["iterations"] == 2 and res["last_line"].startswith("iter 2  loss_cls ")
    assert (out_dir / "last_checkpoint").read_text() == "model_final.pth" and (out_dir / "model_final.pth").is_file()
    cfg = config.setup_config(yaml)
    cfg.MODEL.DEVICE = "cpu"
    torch.manual_seed(0)
    initial = build_model(cfg, load_weights=False, fold=False)
    torch.manual_seed(123)
    fresh = build_model(cfg, load_weights=False, fold=False)
    assert checkpoint.load_model_weights(fresh, str(out_dir), "", strict=True) == str(out_dir / "model_final.pth")
    trained = res["model"]
    for what, convs in (("head", head_convs), ("fpn", fpn_convs)):
        part = lambda m: convs(getattr(m, what))
        assert len(part(trained)) == (8 if what == "fpn" else 10)
        for i, (a, b, c0) in enumerate(zip(part(fresh), part(trained), part(initial))):
            assert bool(torch.isfinite(b.weight).all()) and bool(torch.isfinite(b.bias).all()), (what, i)
            assert torch.equal(a.weight, b.weight.detach().cpu()) and torch.equal(a.bias, b.bias.detach().cpu()), (what, i)
            if b is trained.fpn.p7:
                # two iterations at the warm-up's 2.5e-6: a weight of 2e-2 moves by an fp32 ulp only under a gradient above 4e-4, which
                # p7's single output pixel on a 64 x 96 frame does not give; its bias starts at zero, where every non-zero step shows
                assert not torch.equal(a.bias, c0.bias), (what, i)
            else:
                assert not torch.equal(a.weight, c0.weight), (what, i)
    assert torch.equal(fresh.bottom_up.stem[0].weight, initial.bottom_up.stem[0].weight)          # the frozen part is the seeded one
