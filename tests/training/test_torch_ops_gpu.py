"""K21 on the GPU: pod_label_anchors and pod_train_loss against the fp64 referee (tests/training/loss_ref.py, itself held against the
reference-made fixture by test_losses_cpu.py) and against the reference's recorded losses, at the smallest geometry that exercises
everything: a 64 x 96 frame, levels 8x12 / 4x6 / 2x3 / 1x2 / 1x1, R = 1161 anchors, K = 7, two images (one without ground truth).
Bounds: the project's bar 1e-4 max(1, |ref|) (tests/helpers.py), labels and repeatability exact."""
import json

import numpy as np
import pytest
import torch

from pod_compare_amd import hip, losses, synthetic
from tests.helpers import assert_close
from tests.training import loss_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, A, S = 7, 9, 3


@pytest.fixture(scope="module")
def fx():
    f = lr.load_fixture()
    f["shapes"], f["level_anchors"] = lr.fixture_geometry(f)
    return f


def head_outputs(fx, var, requires_grad=False):
    """The fixture's inputs as the product's per-level (N, A*C, H, W) planes on the device."""
    planes = lambda k, c: [p.to(DEV).requires_grad_(requires_grad) for p in lr.to_planes(torch.from_numpy(fx[k]), fx["shapes"], A)]
    return synthetic.HeadOutputs(planes("cls", K), planes("delta", 4), planes("cls_var", K) if var else None, planes("reg_var", 4) if var else None,
                                 [a.to(DEV) for a in fx["level_anchors"]], fx["shapes"], A, K, tuple(fx["meta"]["frame"]))


def device_labels(fx):
    return (torch.from_numpy(fx["labels"]).to(DEV), torch.from_numpy(fx["matched_gt"]).to(DEV), torch.from_numpy(fx["gt_boxes"]).to(DEV))


def referee_inputs(fx, var, eps_dense=None):
    d = lambda k: torch.from_numpy(fx[k]).double().requires_grad_(True)
    labels = torch.from_numpy(fx["labels"]).long()
    mb = torch.zeros(labels.shape + (4,))
    mb[0] = torch.from_numpy(fx["gt_boxes"])[torch.from_numpy(fx["matched_gt"][0]).long()]
    return dict(cls=d("cls"), delta=d("delta"), cls_var=d("cls_var") if var else None, reg_var=d("reg_var") if var else None, labels=labels,
                matched_boxes=mb, anchors=torch.from_numpy(fx["anchors"]), num_classes=K, eps=eps_dense)


def dense_eps(fx):
    return lr.scatter_eps(fx["eps"], torch.from_numpy(fx["labels"]) >= 0)


def test_labels_equal_the_restatement_exactly(fx):
    """Three images in one call: the five boxes of the fixture; no box at all; the five boxes and one wholly off every anchor's reach
    (its best IoU is 0, and the literal comparison promotes every anchor of that image)."""
    anchors = torch.from_numpy(fx["anchors"])
    gb, gc = torch.from_numpy(fx["gt_boxes"]), torch.from_numpy(fx["gt_classes"]).long()
    far_b, far_c = torch.cat([gb, torch.tensor([lr.FAR_BOX])]), torch.cat([gc, torch.tensor([1])])
    sets = [(gb, gc), (gb[:0], gc[:0]), (far_b, far_c)]
    labels, matched, num_pos = losses.label_anchors([a.to(DEV) for a in fx["level_anchors"]], [b for b, _ in sets], [c for _, c in sets], K)
    labels, matched, num_pos = labels.cpu(), matched.cpu(), num_pos.cpu()
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (3, 1161)
    off = 0
    for i, (b, c) in enumerate(sets):
        ref = lr.label_anchors(anchors, b, c, K)
        assert torch.equal(labels[i].long(), ref["labels"]), i
        assert int(num_pos[i]) == ref["num_pos"], i
        if b.shape[0] == 0:
            assert bool((labels[i] == K).all()) and int(num_pos[i]) == 0 and bool((matched[i] == -1).all())
        else:
            u = ref["unique"]
            assert torch.equal(matched[i][u].long(), ref["matched"][u] + off), i          # one comparison restricted to a unique maximum
            fg = (ref["labels"] >= 0) & (ref["labels"] < K)
            dup = fg & ~u & (ref["matched"] == 0)                                          # the duplicated box: the lowest index wins
            assert int(dup.sum()) >= 19 and bool((matched[i][dup] == off).all()), i
        off += b.shape[0]
    assert torch.equal(labels[0], torch.from_numpy(fx["labels"][0])) and torch.equal(labels[1], torch.from_numpy(fx["labels"][1]))
    assert int(num_pos[0]) == 81 and int((labels[0] == -1).sum()) == 78
    assert int(num_pos[2]) == 1161                                                          # best IoU 0: every anchor is promoted
    zero_iou = lr.iou_matrix(far_b, anchors).max(dim=0).values == 0
    assert bool(zero_iou.any()) and bool((matched[2][zero_iou] == 5).all())                # all-zero column: first arg-max, row 0 of the image


@pytest.mark.parametrize("case", ["plain", "var_step0", "var_mid", "var_annealed"])
def test_losses_equal_the_reference(fx, case):
    m, c = fx["meta"], fx["meta"]["cases"][case]
    var = c["variance_heads"]
    crit = losses.ProbabilisticLosses(num_classes=K, cls_var_num_samples=m["cls_var_num_samples"], annealing_step=m["annealing_step"],
                                      loss_normalizer=m["initial_loss_normalizer"], loss_normalizer_momentum=m["loss_normalizer_momentum"])
    crit.current_step = c["current_step"]
    labels, matched, gb = device_labels(fx)
    out = crit(head_outputs(fx, var), labels, matched, gb, eps=dense_eps(fx).to(DEV) if var else None)
    got_cls, got_reg = float(out["loss_cls"]), float(out["loss_box_reg"])
    print(case, "loss_cls", got_cls, float(fx["loss_cls_" + case]), "loss_box_reg", got_reg, float(fx["loss_box_reg_" + case]))
    assert out["loss_cls"].is_cuda and out["loss_cls"].dim() == 0
    assert abs(float(crit.loss_normalizer) - c["loss_normalizer"]) < 1e-9
    assert_close(got_cls, float(fx["loss_cls_" + case]), "loss_cls")
    assert_close(got_reg, float(fx["loss_box_reg_" + case]), "loss_box_reg")
    assert int(crit.last_sums[3]) == 81


@pytest.mark.parametrize("var", [False, True], ids=["plain", "variance_heads"])
def test_gradient_planes_equal_fp64_autograd(fx, var):
    ho = head_outputs(fx, var)
    labels, matched, gb = device_labels(fx)
    eps = dense_eps(fx)
    w = torch.ones(3, device=DEV)
    sums, grads = losses.train_loss_sums(ho.cls, ho.delta, ho.cls_var, ho.reg_var, labels, matched, gb, ho.anchors, A, K, cls_samples=S,
                                         eps=eps.to(DEV) if var else None, w=w, want_grads=True)
    r = referee_inputs(fx, var, eps if var else None)
    cs, ss, ns, npos = lr.loss_sums(**r)
    (cs + ss + ns).backward()
    for name, got, want in (("cls_sum", sums[0], cs), ("std_reg_sum", sums[1], ss), ("nll_reg_sum", sums[2], ns)):
        assert_close(got.cpu(), want.detach(), name)
    assert int(sums[3]) == npos == 81
    lab = r["labels"]
    ignored, background = lab < 0, lab == K
    g_cls, g_delta, g_cls_var, g_reg_var = grads
    for name, planes, c, ref in (("g_cls", g_cls, K, r["cls"]), ("g_delta", g_delta, 4, r["delta"]), ("g_cls_var", g_cls_var, K, r["cls_var"]),
                                 ("g_reg_var", g_reg_var, 4, r["reg_var"])):
        if planes is None:
            assert not var
            continue
        got = lr.from_planes([p.cpu() for p in planes], c)
        print(name, "max |ref|", float(ref.grad.abs().max()), "max |err|", float((got.double() - ref.grad).abs().max()))
        assert_close(got, ref.grad, name)
        assert bool((got[ignored] == 0).all()), name                           # exactly zero where an anchor contributes nothing
        if name in ("g_delta", "g_reg_var"):
            assert bool((got[background] == 0).all()), name
        assert bool((got != 0).any())
    if var:      # the clamp's gradient: zero outside [-7, 7] (the inputs reach past it on both sides)
        rv = r["reg_var"].detach()
        outside = ((rv < -7) | (rv > 7)) & ((lab >= 0) & (lab < K))[..., None]
        assert int(outside.sum()) > 0 and bool((lr.from_planes([p.cpu() for p in g_reg_var], 4)[outside] == 0).all())


def test_native_draws_are_refereed_on_their_own_normals(fx):
    ho = head_outputs(fx, True)
    labels, matched, gb = device_labels(fx)
    n_rows = labels.numel()

    def run(seed):
        eps_out = torch.full((S, n_rows, K), float("nan"), device=DEV)
        sums, _ = losses.train_loss_sums(ho.cls, ho.delta, ho.cls_var, ho.reg_var, labels, matched, gb, ho.anchors, A, K, cls_samples=S,
                                         eps=None, eps_out=eps_out, seed=seed)
        return sums.cpu(), eps_out.cpu()

    s1, e1 = run(11)
    s2, e2 = run(11)
    s3, e3 = run(12)
    assert torch.equal(s1, s2) and torch.equal(e1, e2)                                      # the same seed: the same bits
    assert not torch.equal(e1, e3) and float(s1[0]) != float(s3[0])                        # another seed: other draws
    assert torch.equal(s1[1:], s3[1:])                                                      # (the regression sums draw nothing)
    valid = (torch.from_numpy(fx["labels"]) >= 0).reshape(-1)
    assert bool(torch.isfinite(e1).all()) and bool((e1[:, ~valid] == 0).all())
    drawn = e1[:, valid].double()
    assert abs(float(drawn.mean())) < 0.05 and abs(float(drawn.std()) - 1.0) < 0.05        # 47 124 standard normals
    cs, ss, ns, _ = lr.loss_sums(**referee_inputs(fx, True, e1))
    assert_close(s1[0], cs.detach(), "cls_sum on the kernel's own draws")
    assert_close(s1[1], ss.detach(), "std_reg_sum")
    assert_close(s1[2], ns.detach(), "nll_reg_sum")


def test_two_launches_give_the_same_bits_and_backward_delivers_the_planes(fx):
    labels, matched, gb = device_labels(fx)
    eps = dense_eps(fx).to(DEV)
    ho = head_outputs(fx, True, requires_grad=True)
    crit = losses.ProbabilisticLosses(num_classes=K, cls_var_num_samples=S, annealing_step=80000)
    crit.current_step = 40000
    w = crit.weights(torch.tensor(37.0, device=DEV), True, True)
    det = lambda ts: [t.detach() for t in ts]
    runs = [losses.train_loss_sums(det(ho.cls), det(ho.delta), det(ho.cls_var), det(ho.reg_var), labels, matched, gb, ho.anchors, A, K,
                                   cls_samples=S, eps=eps, w=w, want_grads=True) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    out = crit(ho, labels, matched, gb, eps=eps, normalizer=37.0)
    (2.0 * out["loss_cls"] + 3.0 * out["loss_box_reg"]).backward()
    g_cls, g_delta, g_cls_var, g_reg_var = runs[0][1]
    for ts, planes, scale in ((ho.cls, g_cls, 2.0), (ho.cls_var, g_cls_var, 2.0), (ho.delta, g_delta, 3.0), (ho.reg_var, g_reg_var, 3.0)):
        for t, p in zip(ts, planes):
            assert t.grad is not None and torch.equal(t.grad, p * torch.tensor(scale, device=DEV))
    sums = runs[0][0].cpu()
    assert_close(float(out["loss_cls"].detach()), float(w[0].double().cpu() * sums[0]), "loss_cls", rtol=1e-6, atol=1e-6)
    assert_close(float(out["loss_box_reg"].detach()), float(w[1].double().cpu() * sums[1] + w[2].double().cpu() * sums[2]), "loss_box_reg", rtol=1e-6, atol=1e-6)


def test_full_covariance_is_refused(fx):
    ho = head_outputs(fx, True)
    labels, matched, gb = device_labels(fx)
    rv10 = [torch.zeros(2, A * 10, h, w, device=DEV) for h, w in fx["shapes"]]
    with pytest.raises(hip.PodError, match="code -1"):
        losses.train_loss_sums(ho.cls, ho.delta, ho.cls_var, rv10, labels, matched, gb, ho.anchors, A, K, cls_samples=S)


def test_model_losses_agree_with_the_kernel_entry():
    """model.losses on a random-init model's outputs for one 64 x 96 frame against pod_label_anchors + pod_train_loss called directly."""
    from pod_compare_amd import modeling
    torch.manual_seed(5)
    model = modeling.ProbabilisticRetinaNet(num_classes=K, cls_var_loss="loss_attenuation", cls_var_num_samples=S,
                                            bbox_cov_loss="negative_log_likelihood").to(DEV).eval()
    frame = synthetic.synthetic_frame(0, device=DEV)[:, :64, :96].contiguous()
    out = model(frame)
    assert [tuple(t.shape[-2:]) for t in out.cls] == [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
    gb, gc = [torch.tensor([[10.0, 8.0, 44.0, 40.0], [50.0, 20.0, 90.0, 60.0]])], [torch.tensor([0, 3])]
    eps = torch.randn(S, 1161, K, device=DEV)
    res = model.losses(out, gb, gc, eps=eps, normalizer=5.0)
    labels, matched, num_pos = losses.label_anchors(out.anchors, gb, gc, K)
    c = lambda ts: [t.contiguous() for t in ts]
    sums, _ = losses.train_loss_sums(c(out.cls), c(out.delta), c(out.cls_var), c(out.reg_var), labels, matched, gb[0].to(DEV), out.anchors, A, K,
                                     cls_samples=S, eps=eps)
    sums = sums.cpu()
    lam = losses.annealing_weight(model.loss_state.current_step, model.loss_state.annealing_step)
    assert int(num_pos[0]) > 0 and int(sums[3]) == int(num_pos[0]) and lam == 0.0
    assert_close(float(res["loss_cls"]), float(sums[0]) / (S * 5.0), "loss_cls", rtol=1e-6, atol=1e-6)
    assert_close(float(res["loss_box_reg"]), float((1 - lam) * sums[1] + lam * sums[2]) / 5.0, "loss_box_reg", rtol=1e-6, atol=1e-6)
    assert np.isfinite(float(res["loss_cls"])) and float(res["loss_cls"]) > 0


def test_compute_losses_entry_point(tmp_path):
    """python -m pod_compare_amd.compute_losses on two synthetic frames (one annotated, with a crowd box that is dropped; one without
    annotations) and a random-init model: finite means, positives counted."""
    from PIL import Image
    from pod_compare_amd import compute_losses
    rng = np.random.default_rng(3)
    images = []
    for k in range(2):
        Image.fromarray(rng.integers(0, 256, size=(64, 96, 3), dtype=np.uint8)).save(tmp_path / ("f%d.png" % k))
        images.append({"id": 40 + k, "file_name": "f%d.png" % k, "height": 64, "width": 96})
    anns = [{"id": 1, "image_id": 40, "category_id": 1, "bbox": [10, 8, 34, 32], "iscrowd": 0},
            {"id": 2, "image_id": 40, "category_id": 4, "bbox": [50, 20, 40, 40], "iscrowd": 0},
            {"id": 3, "image_id": 40, "category_id": 2, "bbox": [0, 0, 96, 64], "iscrowd": 1}]
    (tmp_path / "gt.json").write_text(json.dumps({"images": images, "annotations": anns}))
    res = compute_losses.main(["--coco-json", str(tmp_path / "gt.json"), "--image-root", str(tmp_path), "--random-init", "--min-size-test", "64",
                               "--max-size-test", "96", "--loader-workers", "0", "--device", DEV])
    assert res["images"] == 2 and res["annealing_weight"] == 1.0
    assert np.isfinite(res["loss_cls"]) and np.isfinite(res["loss_box_reg"]) and res["loss_cls"] > 0
    ref = lr.label_anchors(torch.cat(lr._anchors.grid_anchors([(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)])),
                           torch.tensor([[10.0, 8.0, 44.0, 40.0], [50.0, 20.0, 90.0, 60.0]]), torch.tensor([0, 3]), K)
    assert res["positives_per_image"] == ref["num_pos"] / 2.0
