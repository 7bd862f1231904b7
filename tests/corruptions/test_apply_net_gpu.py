"""K35 where apply_net uses it: corruption then the loader's resize (K20) against Pillow's resize of the reference-corrupted frame; the
predictor sees another image; two apply_net --corruption runs write the same bytes; the torch op is the Python entry.

The module shares its name with tests/test_apply_net_gpu.py (its third test is two apply_net runs) so that the GPU run order in
tests/conftest.py (GPU_ORDER, keyed by module name) gives it a place."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from pod_compare_amd import anchors, apply_net, corruptions, resize
from tests.corruptions import corrupt_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda"


def _write_set(tmp_path, sizes, seed=3):
    rng = np.random.default_rng(seed)
    images = []
    for k, (h, w) in enumerate(sizes):
        name = "f%d.png" % k
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(tmp_path / name)
        images.append({"id": 900 + k, "file_name": name, "height": h, "width": w})
    (tmp_path / "set.json").write_text(json.dumps({"images": images}))
    return images


@pytest.mark.parametrize("name", ref.EXACT)
def test_corrupt_then_resize_equals_pillow_on_the_reference(name):
    for index, (hw, lo, hi) in enumerate((((72, 128), 80, 120), ((37, 53), 80, 200), ((130, 70), 64, 100))):
        f = ref.frame(hw, seed=17)
        key = corruptions.corruption_key(ref.SEED, index)
        got = resize.resize_frame_u8(corruptions.corrupt_frame_u8(torch.from_numpy(f).to(DEV), name, 3, key), lo, hi)
        nh, nw = anchors.resize_shortest_edge(hw[0], hw[1], lo, hi)
        im = Image.fromarray(ref.corrupt(f, name, 3, key))
        if (nh, nw) != hw:
            im = im.resize((nw, nh), Image.BILINEAR)
        want = torch.from_numpy(np.ascontiguousarray(np.asarray(im)[:, :, ::-1].transpose(2, 0, 1)))
        assert torch.equal(got.cpu(), want), (name, hw)


def test_torch_op_is_the_python_entry():
    import pod_compare_amd.torch_ops  # noqa: F401  (registers the library)
    src = torch.from_numpy(ref.frame((37, 53))).to(DEV)
    for name in corruptions.NAMES:
        a = torch.ops.pod_mi355x.corrupt_frame(src, name, 3, 11, 5)
        assert a.shape == src.shape and a.dtype == torch.uint8 and a.is_contiguous()
        assert torch.equal(a, corruptions.corrupt_frame_u8(src, name, 3, corruptions.corruption_key(11, 5))), name
    with pytest.raises(ValueError):
        torch.ops.pod_mi355x.corrupt_frame(src, "fog", 3, 11, 5)
    with pytest.raises(Exception):
        torch.ops.pod_mi355x.corrupt_frame(src.float(), "contrast", 3, 11, 5)


def test_a_corrupted_input_changes_the_detections(tmp_path):
    """The predictor as tests/loader/test_apply_net_gpu.py builds it (class bias shifted so that detections exist), through
    apply_net._network_input with and without --corruption contrast --severity 5: detections on both, and not the same ones."""
    import argparse
    from pod_compare_amd import config
    from pod_compare_amd.probabilistic_inference import build_predictor
    from tests.test_sparse_tower_gpu import build
    cfgs = os.path.join(ROOT, "pod_compare_amd", "configs")
    cfg = config.setup_config(os.path.join(cfgs, "BDD-Detection", "retinanet", "retinanet_R_50_FPN_1x_reg_cls_var.yaml"),
                              os.path.join(cfgs, "Inference", "bayes_od.yaml"))
    cfg.MODEL.DEVICE = DEV
    m = build()
    with torch.no_grad():
        m.head.cls_score.weight.mul_(40.0)
        m.head.cls_score.bias.fill_(-2.5)
    _write_set(tmp_path, [(180, 320), (200, 300)], seed=5)
    data = apply_net.CocoImages(str(tmp_path / "set.json"), str(tmp_path), cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, device_resize=True)
    p = build_predictor(cfg, model=m)
    p.return_device = True
    p.sparse_bbox_tower = True
    clean = argparse.Namespace(resize_on_gpu=True, corruption=None, severity=None, random_seed=0)
    bad = argparse.Namespace(resize_on_gpu=True, corruption="contrast", severity=5, random_seed=0)
    with torch.no_grad():
        for i in range(2):
            outs = []
            for args in (clean, bad):
                input_im, _ = apply_net._network_input(args, cfg, data[i], i, DEV)
                det = p(input_im)
                outs.append((det.records.clone(), int(det.n_det), input_im[0]["image"].clone()))
            (r0, n0, im0), (r1, n1, im1) = outs
            assert im0.shape == im1.shape and not torch.equal(im0, im1)
            assert n0 > 0 and n1 > 0, (n0, n1)
            assert n0 != n1 or not torch.equal(r0[:n0], r1[:n1]), i


def test_two_corrupted_runs_write_the_same_bytes(tmp_path):
    _write_set(tmp_path, [(180, 320), (200, 300), (180, 320), (200, 300)])
    env = dict(os.environ, PYTHONPATH=ROOT)
    outs = []
    for name in ("a", "b"):
        out, side = str(tmp_path / (name + ".json")), str(tmp_path / (name + ".podr"))
        cmd = [sys.executable, "-m", "pod_compare_amd.apply_net", "--coco-json", str(tmp_path / "set.json"), "--image-root", str(tmp_path),
               "--random-init", "--output", out, "--binary-output", side, "--corruption", "contrast", "--severity", "3"]
        r = subprocess.run(cmd, cwd=ROOT, env=env, timeout=900, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert "corrupted on the GPU: contrast, severity 3" in r.stdout and "resized on the GPU" in r.stdout
        outs.append((open(out, "rb").read(), open(side, "rb").read()))
    assert outs[0] == outs[1] and len(outs[0][1]) > 0
