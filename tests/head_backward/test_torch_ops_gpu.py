"""The head's backward pass end to end (pod_compare_amd/head_train.py, train_head.py) against fp64 CPU autograd of the same module on the
same dropout masks: every parameter gradient and the feature gradient, bare and through model.losses; the production dropout path; the
trainer's step function and the command."""
import copy
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pod_compare_amd import checkpoint, losses, modeling, train_head
from pod_compare_amd.head_train import head_convs
from tests.head_backward import hb
from tests.training import loss_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVELS, B, C = [(12, 20), (6, 10), (3, 5)], 2, 64
NAMES = ["cls_subnet.%d" % i for i in range(4)] + ["bbox_subnet.%d" % i for i in range(4)] + ["cls_score", "bbox_pred", "cls_var", "bbox_cov"]


def reference_forward(head, feats, masks, p):
    """The head in plain torch (any dtype / device): conv + ReLU (+ the recorded keep-mask / (1 - p)) per trunk layer, then the predictors."""
    outs = [[], [], [], []]
    for lv, f in enumerate(feats):
        trunks = []
        for sid, sub in enumerate((head.cls_subnet, head.bbox_subnet)):
            x = f
            for l, conv in enumerate(sub):
                x = F.relu(conv(x))
                if masks is not None:
                    keep = torch.stack([masks[(sid, l, lv, c)] for c in range(x.shape[0])]).to(x.dtype)
                    x = x * keep / (1.0 - p)
            trunks.append(x)
        outs[0].append(head.cls_score(trunks[0]))
        outs[1].append(head.bbox_pred(trunks[1]))
        outs[2].append(head.cls_var(trunks[0]))
        outs[3].append(head.bbox_cov(trunks[1]))
    return outs


def reference_grads(head, feats, masks, p, out_grads, dtype):
    h = copy.deepcopy(head).to("cpu", dtype)
    fs = [f.detach().to("cpu", dtype).requires_grad_(True) for f in feats]
    outs = reference_forward(h, fs, masks, p)
    flat = [t for group in outs for t in group]
    torch.autograd.backward(flat, [g.to("cpu", dtype) for group in out_grads for g in group])
    params = [q.grad for c in head_convs(h) for q in (c.weight, c.bias)]
    return params, [f.grad for f in fs]


def make_head(p, seed=0):
    torch.manual_seed(seed)
    head = modeling.ProbabilisticRetinaNetHead(in_channels=C, num_classes=7, dropout_rate=p, compute_cls_var=True, compute_bbox_cov=True)
    for conv in head_convs(head):                     # activations of order one through the five chained layers
        torch.nn.init.normal_(conv.weight, std=0.05)
        torch.nn.init.normal_(conv.bias, std=0.1)
    return head.to(DEV)


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["dropout0", "dropout0.1_replay"])
def test_every_gradient_of_the_head_matches_fp64_autograd(p):
    """Every parameter gradient and the feature gradients, e <= 1e-4 and e <= 4 e_f32 (tests/head_backward/hb.py), behind five chained
    layers.  Measured figures: profiles/head_backward.md."""
    head = make_head(p)
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn((B, C, h, w), generator=g).to(DEV).requires_grad_(True) for h, w in LEVELS]
    masks = None
    if p > 0:
        masks = {(sid, l, lv, c): torch.rand((C, h, w), generator=g) >= p for sid in range(2) for l in range(4)
                 for lv, (h, w) in enumerate(LEVELS) for c in range(B)}
        head.dropout_replay = lambda sid, layer, level, copy_: masks[(sid, layer, level, copy_)]
    out = head.forward_train(feats)
    groups = [out.cls, out.delta, out.cls_var, out.reg_var]
    assert all(t.grad_fn is not None and t.shape[0] == B for grp in groups for t in grp)
    assert [tuple(t.shape[1:]) for t in out.cls] == [(63, h, w) for h, w in LEVELS] and out.delta[0].shape[1] == 36
    out_grads = [[torch.randn(t.shape, generator=g) for t in grp] for grp in groups]
    torch.autograd.backward([t for grp in groups for t in grp], [x.to(DEV) for grp in out_grads for x in grp])
    ref64 = reference_forward(copy.deepcopy(head).to("cpu", torch.float64), [f.detach().cpu().double() for f in feats], masks, p)
    for name, got, want in zip(("cls", "delta", "cls_var", "reg_var"), groups, ref64):       # the forward first: the project's bar
        for t, r in zip(got, want):
            assert hb.rel_err(t, r.detach()) <= hb.BAR, name
    p32, f32 = reference_grads(head, feats, masks, p, out_grads, torch.float32)
    p64, f64 = reference_grads(head, feats, masks, p, out_grads, torch.float64)
    got = [q.grad for c in head_convs(head) for q in (c.weight, c.bias)]
    assert all(x is not None and bool(torch.isfinite(x).all()) for x in got)
    tag, chk = "p=%.1f " % p, hb.Checker()
    for i, (a, b32, b64) in enumerate(zip(got, p32, p64)):
        chk.add(tag + NAMES[i // 2] + (".bias" if i % 2 else ".weight"), a, b32, b64)
    for lv, (f, b32, b64) in enumerate(zip(feats, f32, f64)):
        chk.add(tag + "features[%d]" % lv, f.grad, b32, b64)
    chk.finish()


def test_gradients_accumulate_and_skip_the_features_when_they_do_not_ask():
    head = make_head(0.0)
    g = torch.Generator().manual_seed(2)
    feats = [torch.randn((B, C, h, w), generator=g).to(DEV) for h, w in LEVELS]
    loss = lambda: sum(t.sum() for t in head.forward_train(feats).cls)
    loss().backward()
    first = head.cls_subnet[0].weight.grad.clone()
    assert head.bbox_pred.weight.grad is not None and bool((head.bbox_pred.weight.grad == 0).all())      # an output nobody used: zero, not garbage
    loss().backward()
    assert torch.equal(head.cls_subnet[0].weight.grad, first + first)                                      # .grad accumulates; launches repeat to the bit


def test_production_dropout_gates_on_the_saved_activation():
    """No replay: the Philox masks of the store pass.  Weights and biases chosen so that every pre-activation is positive -- an element
    of a stored activation is zero exactly where its mask dropped it.  The gate's output is nonzero only there, the kept fraction of
    every layer lies in the binomial 6-sigma band around 1 - p, and the layers' masks differ."""
    p = 0.1
    head = make_head(p)
    with torch.no_grad():
        for conv in list(head.cls_subnet) + list(head.bbox_subnet):
            conv.weight.mul_(0.04)                    # std 0.002: |w . x| stays far below the bias
            conv.bias.fill_(3.0)
    g = torch.Generator().manual_seed(3)
    feats = [torch.rand((B, C, h, w), generator=g).to(DEV) for h, w in LEVELS]
    head.train_tap = {}
    out = head.forward_train(feats)
    torch.autograd.backward(out.cls + out.delta, [torch.randn(t.shape, generator=g).to(DEV) for t in out.cls + out.delta])
    saved, dz = head.train_tap["saved"], head.train_tap["dz"]
    n = B * sum(h * w for h, w in LEVELS) * C
    band = 6.0 * (p * (1 - p) / n) ** 0.5
    patterns = []
    for sid in range(2):
        for l in range(4):
            act, d = saved[sid][l][1], dz[(sid, l)]
            kept = act != 0
            frac = float(kept.float().mean())
            print("kept fraction trunk %d layer %d: %.4f (band %.4f)" % (sid, l, frac, band))
            assert abs(frac - (1 - p)) <= band
            assert bool((d[~kept] == 0).all()) and bool((d[kept] != 0).float().mean() > 0.99)
            assert bool((act[kept] > 2.0).all())                                    # relu(z) / (1 - p), z = 3 +- 0.2 at most: every pre-activation is positive
            patterns.append(kept)
    assert all(not torch.equal(patterns[i], patterns[j]) for i in range(8) for j in range(i))
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for c in head_convs(head) for q in (c.weight, c.bias))


def test_training_forward_of_one_image_equals_the_inference_forward():
    """p = 0, B = 1: the two forwards run one launch plan (modeling._trunk_plan) -- the same kernels, tables and abs-max records, so the
    same bits.  (B > 1 stands the images at other canvas positions: Winograd tiles fall differently and the rounding with them.)"""
    head = make_head(0.0)
    g = torch.Generator().manual_seed(4)
    feats = [torch.randn((1, C, h, w), generator=g).to(DEV) for h, w in LEVELS]
    out = head.forward_train(feats)
    with torch.no_grad():
        want = head(feats, 1)
    for name, got, ref in zip(("cls", "delta", "cls_var", "reg_var"), (out.cls, out.delta, out.cls_var, out.reg_var), want):
        assert len(got) == len(ref) == len(LEVELS)
        for t, r in zip(got, ref):
            assert t.shape == r.shape and torch.equal(t.detach(), r), name


def test_both_forwards_draw_their_philox_offsets_from_one_counter():
    """p = 0.1, production masks: a training forward and an MC-dropout inference forward each advance head._drop_calls by one offset per
    trunk layer and subnet, so two successive training forwards draw different masks."""
    head = make_head(0.1)
    L = len(head.cls_subnet)
    g = torch.Generator().manual_seed(5)
    feats = [torch.randn((B, C, h, w), generator=g).to(DEV) for h, w in LEVELS]
    head.train_tap = {}
    patterns = []
    for _ in range(2):
        before = head._drop_calls
        head.forward_train(feats)
        assert head._drop_calls == before + 2 * L
        patterns.append([head.train_tap["saved"][sid][l][1] != 0 for sid in range(2) for l in range(L)])
    assert all(not torch.equal(a, b) for a, b in zip(*patterns))
    before = head._drop_calls
    with torch.no_grad():
        head([f[:1] for f in feats], 3, mc_dropout=True)
    assert head._drop_calls == before + 2 * L


def test_cpu_features_and_untileable_channels_raise():
    from pod_compare_amd import hip
    head = make_head(0.0)
    with pytest.raises(hip.PodError):
        head.forward_train([torch.zeros((1, C, 4, 4))])
    with pytest.raises(hip.PodError):
        head.forward_train([torch.zeros((1, 48, 4, 4), device=DEV)])


# ---- through model.losses, on the loss fixture's frame -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    f = lr.load_fixture()
    f["shapes"], f["level_anchors"] = lr.fixture_geometry(f)
    return f


def make_model(seed=5):
    torch.manual_seed(seed)
    model = modeling.ProbabilisticRetinaNet(num_classes=7, cls_var_loss="loss_attenuation", cls_var_num_samples=3,
                                            bbox_cov_loss="negative_log_likelihood").to(DEV).eval()
    model.loss_state = losses.ProbabilisticLosses(num_classes=7, cls_var_num_samples=3, annealing_step=80000)
    model.loss_state.current_step = 40000           # all three loss weights non-zero
    return model


def batch_of(fx, seed=6):
    g = torch.Generator().manual_seed(seed)
    feats = [(0.5 * torch.randn((2, 256, h, w), generator=g)).to(DEV) for h, w in fx["shapes"]]
    gb, gc = torch.from_numpy(fx["gt_boxes"]), torch.from_numpy(fx["gt_classes"]).long()
    eps = lr.scatter_eps(fx["eps"], torch.from_numpy(fx["labels"]) >= 0)
    return feats, [gb, gb[:0]], [gc, gc[:0]], eps


def referee_loss(head64, feats64, fx, eps, norm, lam, samples=3):
    outs = reference_forward(head64, feats64, None, 0.0)
    cls, delta, cls_var, reg_var = (lr.from_planes(o, c) for o, c in zip(outs, (7, 4, 7, 4)))
    labels = torch.from_numpy(fx["labels"]).long()
    mb = torch.zeros(labels.shape + (4,))
    mb[0] = torch.from_numpy(fx["gt_boxes"])[torch.from_numpy(fx["matched_gt"][0]).long()]
    cs, ss, ns, _ = lr.loss_sums(cls, delta, cls_var, reg_var, labels, mb, torch.from_numpy(fx["anchors"]), 7, eps)
    return cs / (samples * norm), ((1 - lam) * ss + lam * ns) / norm


def test_losses_backward_fills_every_head_gradient(fx):
    """model.losses on the loss fixture's frame: backward() fills every head parameter's .grad, finite and not all zero, equal to the
    fp64 autograd of head + referee within e <= 1e-4 and e <= 4 e_f32.  Measured figures: profiles/head_backward.md."""
    model = make_model()
    feats, gb, gc, eps = batch_of(fx)
    assert [tuple(f.shape[-2:]) for f in feats] == [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
    out = model.head.forward_train(feats, model.anchors_for((64, 96)), (64, 96))
    res = model.losses(out, gb, gc, eps=eps.to(DEV), normalizer=81.0)
    (res["loss_cls"] + res["loss_box_reg"]).backward()
    lam = lr.annealing_lambda(40000, 80000)
    grads = {}
    for dtype in (torch.float32, torch.float64):
        h = copy.deepcopy(model.head).to("cpu", dtype)
        for q in h.parameters():
            q.grad = None
        lc, lb = referee_loss(h, [f.cpu().to(dtype) for f in feats], fx, eps, 81.0, lam)
        (lc + lb).backward()
        grads[dtype] = [q.grad for c in head_convs(h) for q in (c.weight, c.bias)]
        if dtype == torch.float64:
            assert abs(float(res["loss_cls"]) - float(lc)) <= 1e-4 * max(1.0, abs(float(lc)))
            assert abs(float(res["loss_box_reg"]) - float(lb)) <= 1e-4 * max(1.0, abs(float(lb)))
    got = [q.grad for c in head_convs(model.head) for q in (c.weight, c.bias)]
    chk = hb.Checker()
    for i, (a, b32, b64) in enumerate(zip(got, grads[torch.float32], grads[torch.float64])):
        assert a is not None and bool(torch.isfinite(a).all()) and bool((a != 0).any()), NAMES[i // 2]
        chk.add("losses " + NAMES[i // 2] + (".bias" if i % 2 else ".weight"), a, b32, b64)
    chk.finish()


def test_twenty_sgd_steps_lower_the_loss_and_the_first_equals_an_fp64_replica(fx):
    model = make_model()
    feats, gb, gc, eps = batch_of(fx)
    lr0, mom, wd = 0.01, 0.9, 1e-4
    trainer = train_head.HeadTrainer(model, base_lr=lr0, momentum=mom, weight_decay=wd, steps=(1000, 2000), warmup_iters=0)
    assert not any(q.requires_grad for q in model.bottom_up.parameters()) and all(q.requires_grad for q in model.head.parameters())
    h64 = copy.deepcopy(model.head).to("cpu", torch.float64)
    lc, lb = referee_loss(h64, [f.cpu().double() for f in feats], fx, eps, 81.0, lr.annealing_lambda(40000, 80000))
    (lc + lb).backward()
    eps_d = eps.to(DEV)
    history = []
    for it in range(20):
        res = trainer.step(feats, (64, 96), (64, 96), gb, gc, eps=eps_d, normalizer=81.0)
        history.append(res["loss_cls"] + res["loss_box_reg"])
        if it == 0:       # one SGD step from zero momentum: w - lr (g + wd w); the gradient bar times lr, plus the fp32 rounding of w itself
            for name, c, c64 in zip(NAMES, head_convs(model.head), head_convs(h64)):
                for q, q64 in ((c.weight, c64.weight), (c.bias, c64.bias)):
                    want = q64.detach() - lr0 * (q64.grad + wd * q64.detach())
                    bound = lr0 * hb.BAR * float(q64.grad.abs().max()) + 2.0 ** -24 * float(want.abs().max())
                    err = float((q.detach().cpu().double() - want).abs().max())
                    print("HB_STEP %-16s err %.3e bound %.3e" % (name, err, bound))
                    assert err <= bound, name
    history = [float(x) for x in torch.stack(history).cpu()]
    print("loss over 20 steps:", " ".join("%.4f" % x for x in history))
    assert trainer.iteration == 20 and model.loss_state.current_step == 40020
    assert abs(history[0] - float(lc + lb)) <= 1e-4 * max(1.0, float(lc + lb))
    assert history[-1] < history[0] and all(np.isfinite(history))


def test_train_head_writes_a_checkpoint_that_loads_back(tmp_path):
    from PIL import Image
    from pod_compare_amd import config
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
    # (the plain model: a random-init backbone hands the head features of several thousand, under which the variance heads' sampled
    #  logits overflow the classification loss -- as they would in the reference; a checkpoint's features are of order one)
    import os
    yaml = os.path.join(os.path.dirname(train_head.__file__), "configs/BDD-Detection/retinanet/retinanet_R_50_FPN_1x.yaml")
    res = train_head.main(["--config-file", yaml, "--coco-json", str(tmp_path / "gt.json"), "--image-root", str(tmp_path), "--random-init", "--output-dir", str(out_dir),
                           "--max-iter", "3", "--log-period", "1", "--min-size-test", "64", "--max-size-test", "96", "--loader-workers", "0",
                           "--device", DEV])
    assert res["iterations"] == 3 and res["last_line"].startswith("iter 3  loss_cls ")
    assert (out_dir / "last_checkpoint").read_text() == "model_final.pth" and (out_dir / "model_final.pth").is_file()
    cfg = config.setup_config(yaml)
    cfg.MODEL.DEVICE = "cpu"
    torch.manual_seed(0)
    initial = build_model(cfg, load_weights=False, fold=False)
    torch.manual_seed(123)
    fresh = build_model(cfg, load_weights=False, fold=False)
    assert checkpoint.load_model_weights(fresh, str(out_dir), "", strict=True) == str(out_dir / "model_final.pth")
    trained = res["model"].head
    assert len(head_convs(trained)) == 10
    for name, a, b, c0 in zip(NAMES, head_convs(fresh.head), head_convs(trained), head_convs(initial.head)):
        assert bool(torch.isfinite(b.weight).all()) and bool(torch.isfinite(b.bias).all()), name
        assert torch.equal(a.weight, b.weight.detach().cpu()) and torch.equal(a.bias, b.bias.detach().cpu()), name
        assert not torch.equal(a.weight, c0.weight), name
    assert torch.equal(fresh.bottom_up.stem[0].weight, initial.bottom_up.stem[0].weight)          # the frozen part is the seeded one
