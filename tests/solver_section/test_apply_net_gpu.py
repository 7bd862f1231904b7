"""The trainer under the SOLVER section: HeadTrainer's fused step (K29) beside torch.optim.SGD with two groups, nesterov and torch's clipping
utilities; train_head --resume under the new keys and --guard-nonfinite; the stop at a non-finite gradient; two data-parallel ranks.

Fused against torch: both are held against the fp64 expression of one step from the same fp32 state and gradients (m = 0: a first step),
each within its one-step bound (tests/solver_section/test_torch_ops_gpu.py's derivation, with mu |m| = 0):
    |w' - w^| <= 2 u |w^| + 2 lr (d's bound),   extra = (2 u + (n + 4) 2^-53) |a| on the fused side
so they agree within the sum of the two.  Torch's side forms its norm in fp32 (torch.linalg.vector_norm, the function clip_grad_norm_
calls) and the coefficient from it in three fp32 operations before the product: its extra is (4 u + e) |a|, with e the relative error
of that fp32 norm itself against the fp64 norm -- the referee's own error, measured on the gradients of the case, not assumed."""
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

from pod_compare_amd import train_head
from pod_compare_amd.config import setup_config
from pod_compare_amd.sgd_step import SolverSettings
from tests.data_parallel import dp
from tests.fpn_backward import test_torch_ops_gpu as fpn_tests
from tests.resnet_backward import test_torch_ops_gpu as resnet_tests

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
BASE_YAML = os.path.join(os.path.dirname(train_head.__file__), "configs/BDD-Detection/retinanet/retinanet_R_50_FPN_1x.yaml")
f32 = lambda x: float(np.float32(x))


def solver_yaml(path, clip_type, base=None):
    text = ("_BASE_: %s\n" % base if base else "") + (
        "SOLVER:\n  NESTEROV: True\n  BIAS_LR_FACTOR: 2.0\n  WEIGHT_DECAY_BIAS: 0.0\n"
        "  CLIP_GRADIENTS:\n    ENABLED: True\n    CLIP_TYPE: %s\n    CLIP_VALUE: 1.0\n" % clip_type)
    path.write_text(text)
    return str(path)


# ---- 1: fused against torch ------------------------------------------------------------------------------------------------------------
def _trainer(train_backbone, fused, settings):
    model, shadow = resnet_tests.make_models()
    return train_head.HeadTrainer(model, base_lr=0.01, warmup_iters=0, steps=(1000, 2000), train_backbone=train_backbone,
                                  shadow=shadow if train_backbone else None, fused_step=fused, solver=settings)


def _owners(tr):
    n_plain = len(tr.params) - (len(tr.masters.params) if tr.masters is not None else 0)
    return tr.params[:n_plain] + ([c.weight for c in tr.masters.convs] if tr.masters is not None else [])


@pytest.mark.parametrize("train_backbone", [False, True], ids=["head_only", "backbone"])
@pytest.mark.parametrize("clip_type", ["value", "norm", "full_model"])
def test_the_fused_trainer_steps_as_the_torch_one_under_the_solver_keys(tmp_path, clip_type, train_backbone):
    settings = train_head.solver_settings(setup_config(solver_yaml(tmp_path / "solver.yaml", clip_type)))
    assert settings == SolverSettings(nesterov=True, bias_lr_factor=2.0, weight_decay_bias=0.0, clip_type=clip_type, clip_value=1.0)
    images, gb, gc = fpn_tests.batch()
    fused, plain = _trainer(train_backbone, True, settings), _trainer(train_backbone, False, settings)
    assert fused.fused is not None and plain.fused is None and len(plain.opt.param_groups) == 2 and plain.opt.param_groups[0]["nesterov"]
    assert fused.groups == plain.groups and 0 < sum(fused.groups) < len(fused.groups) and fused.lrs_at(0) == [0.01, 0.01 * 2.0]
    for a, b in zip(fused.params, plain.params):                               # one state
        assert torch.equal(a.detach(), b.detach())
    feats, padded = fused.features(images)
    fused.forward_backward(feats, padded, (64, 96), gb, gc)
    grads = [None if o.grad is None else o.grad.detach().clone() for o in _owners(fused)]
    assert sum(g is not None for g in grads) >= len(grads) - 4
    for o, g in zip(_owners(plain), grads):                                    # the same gradients: the comparison is of the optimisers alone
        o.grad = None if g is None else g.clone()
    n_plain = len(fused.params) - (len(fused.masters.params) if fused.masters is not None else 0)
    scales = [None] * n_plain + (list(fused.masters.scales) if fused.masters is not None else [])
    w0 = [p.detach().cpu().double().numpy() for p in fused.params]
    # a0 = fl32(s g) and its norms in fp64; torch's own fp32 norms of the same a0
    a0 = [None if g is None else ((g if s is None else g * s).cpu().double().numpy()) for g, s in zip(grads, scales)]
    sumsq = [0.0 if a is None else float((a * a).sum()) for a in a0]
    norm32 = [0.0 if g is None else float(torch.linalg.vector_norm(g if s is None else g * s)) for g, s in zip(grads, scales)]
    total = float(np.sum(sumsq))
    n_all = sum(a.size for a in a0 if a is not None)
    fused.optimizer_step(fused.lr)
    plain.optimizer_step(plain.lr)
    lr, wd, mu, v = [f32(0.01), f32(0.01 * 2.0)], [f32(1e-4), 0.0], f32(0.9), 1.0
    coef_of = lambda ss: min(1.0, v / (np.sqrt(ss) + 1e-6))
    if clip_type == "full_model":
        e_total = abs(float(plain._grad_norm) - np.sqrt(total)) / np.sqrt(total)
        assert e_total <= 1e-4                                                 # (a sanity check of the measured error, not a tolerance of the test)
    worst = {"fused": 0.0, "torch": 0.0}
    clipped = 0
    for i, (w, a, G) in enumerate(zip(w0, a0, fused.groups)):
        got = {"fused": fused.params[i].detach().cpu().double().numpy(), "torch": plain.params[i].detach().cpu().double().numpy()}
        if a is None:
            assert np.array_equal(got["fused"], w) and np.array_equal(got["torch"], w), i
            continue
        if clip_type == "value":
            c, e32 = 1.0, 0.0
            a_hat = np.clip(a, -v, v)
            clipped += int((np.abs(a) > v).any())
        else:
            ss = sumsq[i] if clip_type == "norm" else total
            c = coef_of(ss)
            e32 = abs(norm32[i] - np.sqrt(ss)) / np.sqrt(ss) if (clip_type == "norm" and ss > 0) else (e_total if clip_type == "full_model" else 0.0)
            a_hat = c * a
            clipped += int(c < 1.0)
        g1 = a_hat + wd[G] * w
        w_hat = w - lr[G] * (g1 + mu * g1)
        terms = np.abs(a_hat) + wd[G] * np.abs(w)
        for side, extra_rel in (("fused", 2 * U + (n_all + 4) * 2.0 ** -53), ("torch", 4 * U + e32)):
            extra = extra_rel * np.abs(a_hat) if clip_type != "value" else 0.0
            bound_m = 4 * U * terms + extra
            bound_d = 3 * U * terms + extra + mu * bound_m + 2 * U * (1 + mu) * terms
            bound_w = 2 * U * np.abs(w_hat) + 2 * lr[G] * bound_d
            err = np.abs(got[side] - w_hat)
            assert bool((err <= bound_w).all()), (side, i, float((err / np.maximum(bound_w, 1e-300)).max()))
            worst[side] = max(worst[side], float((err / np.maximum(bound_w, 1e-300)).max()))
        assert not np.array_equal(got["fused"], w) or not (a.any() or w.any()), i
    assert clipped > 0                                                         # the threshold bites: the case is not K25's
    print("SOLVER_TRAINER %s %s: err_w / bound <= %.3f fused, %.3f torch, over %d tensors (%d clipped)" % (
        "backbone" if train_backbone else "head", clip_type, worst["fused"], worst["torch"], len(w0), clipped))
    if fused.masters is not None:
        for tr in (fused, plain):
            for c, p, s in zip(tr.masters.convs, tr.masters.params, tr.masters.scales):
                assert torch.equal(c.weight.detach(), p.detach() * s)
    assert (fused.grad_norm() is not None) == (clip_type != "value") and (plain.grad_norm() is not None) == (clip_type == "full_model")
    if clip_type != "value":
        assert abs(fused.grad_norm() - np.sqrt(total)) <= (n_all + 4) * 2.0 ** -53 * np.sqrt(total)


# ---- 2 and 3: the command ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("frames")
    rng = np.random.default_rng(3)
    images = []
    for k in range(2):
        Image.fromarray(rng.integers(0, 256, size=(64, 96, 3), dtype=np.uint8)).save(root / ("f%d.png" % k))
        images.append({"id": 40 + k, "file_name": "f%d.png" % k, "height": 64, "width": 96})
    anns = [{"id": 1, "image_id": 40, "category_id": 1, "bbox": [10, 8, 34, 32], "iscrowd": 0},
            {"id": 2, "image_id": 40, "category_id": 4, "bbox": [50, 20, 40, 40], "iscrowd": 0}]
    (root / "gt.json").write_text(json.dumps({"images": images, "annotations": anns}))
    solver_yaml(root / "solver.yaml", "full_model", base=BASE_YAML)
    return root


def run(data, out_dir, max_iter, *flags):
    return train_head.main(["--config-file", str(data / "solver.yaml"), "--coco-json", str(data / "gt.json"), "--image-root", str(data), "--random-init",
                            "--output-dir", str(out_dir), "--max-iter", str(max_iter), "--log-period", "1", "--min-size-test", "64", "--max-size-test", "96",
                            "--loader-workers", "0", "--device", DEV] + list(flags))


def test_resume_under_the_solver_keys_and_the_guard_is_bit_for_bit(data, tmp_path, capsys):
    from tests.optimizer_step.test_apply_net_gpu import assert_same_run, final
    flags = ("--guard-nonfinite",)                                             # (implies --fused-step)
    a = run(data, tmp_path / "a", 3, *flags)
    a2 = run(data, tmp_path / "a2", 3, *flags)
    assert a["trainer"].fused is not None and a["trainer"].solver.guard_nonfinite and a["trainer"].solver.clip_type == "full_model"
    assert_same_run(final(tmp_path / "a"), final(tmp_path / "a2"), "two uninterrupted runs")
    assert a["last_line"] == a2["last_line"] and a["last_line"].startswith("iter 3  loss_cls ") and "  grad_norm " in a["last_line"]
    st = final(tmp_path / "a")[train_head.TRAINER_KEY]
    assert st["iteration"] == 3 and all(bool(v.any()) for k, v in st["momentum"].items() if k.endswith(".weight"))
    assert sorted(st) == ["iteration", "loss_state", "momentum", "momentum_mu", "random_seed", "sampler", "trained"]      # nothing new enters pod_trainer
    assert run(data, tmp_path / "b", 2, *flags)["iterations"] == 2
    capsys.readouterr()
    b = run(data, tmp_path / "b", 3, "--resume", *flags)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("iter ")]
    assert b["iterations"] == 3 and len(lines) == 1 and b["last_line"] == a["last_line"]
    assert_same_run(final(tmp_path / "b"), final(tmp_path / "a"), "stopped at 2 and resumed against uninterrupted")
    assert a["trainer"].check_finite()["bad_steps"] == 0


def test_a_non_finite_gradient_stops_the_trainer_before_anything_is_written():
    model, _ = resnet_tests.make_models()
    tr = train_head.HeadTrainer(model, base_lr=0.01, warmup_iters=0, steps=(1000, 2000), fused_step=True, guard_nonfinite=True, iteration=17)
    assert tr.solver.guard_nonfinite and not tr.solver.plain_step
    images, gb, gc = fpn_tests.batch()
    feats, padded = tr.features(images)
    tr.forward_backward(feats, padded, (64, 96), gb, gc)
    assert tr.check_finite()["bad_steps"] == 0
    tr.params[3].grad.view(-1)[5] = float("inf")
    before = [p.detach().clone() for p in tr.params] + [m.clone() for m in tr.fused.buffers]
    tr.optimizer_step(tr.lr)
    tr.advance()
    with pytest.raises(FloatingPointError) as e:
        tr.check_finite()
    assert str(e.value) == "gradient or loss became infinite or NaN at iteration 17"
    after = [p.detach() for p in tr.params] + list(tr.fused.buffers)
    assert all(torch.equal(a, b) for a, b in zip(after, before))
    # the next step, with finite gradients, is not taken either; after reset() it is
    tr.forward_backward(feats, padded, (64, 96), gb, gc)
    tr.optimizer_step(tr.lr)
    assert all(torch.equal(a, b) for a, b in zip([p.detach() for p in tr.params] + list(tr.fused.buffers), before))
    with pytest.raises(FloatingPointError):
        tr.check_finite()
    tr.fused.reset()
    tr.optimizer_step(tr.lr)
    assert tr.check_finite()["bad_steps"] == 0 and not torch.equal(tr.params[3].detach(), before[3])


def test_the_command_raises_at_the_first_check_and_writes_no_checkpoint(data, tmp_path, monkeypatch):
    """An infinity planted in one gradient of iteration 1; no log steps, so the first check is the final checkpoint's: train_head raises
    FloatingPointError naming iteration 1 and save_checkpoint is not reached."""
    inner, saves = train_head.HeadTrainer.forward_backward, []

    def planting(self, *a, **k):
        res = inner(self, *a, **k)
        if self.iteration == 1:
            self.params[0].grad.view(-1)[0] = float("inf")
        return res
    monkeypatch.setattr(train_head.HeadTrainer, "forward_backward", planting)
    monkeypatch.setattr(train_head, "save_checkpoint", lambda *a, **k: saves.append(a) or "never")
    with pytest.raises(FloatingPointError) as e:
        train_head.main(["--config-file", str(data / "solver.yaml"), "--coco-json", str(data / "gt.json"), "--image-root", str(data), "--random-init",
                         "--output-dir", str(tmp_path / "out"), "--max-iter", "3", "--log-period", "0", "--min-size-test", "64", "--max-size-test", "96",
                         "--loader-workers", "0", "--device", DEV, "--guard-nonfinite"])
    assert "at iteration 1" in str(e.value) and saves == [] and not (tmp_path / "out" / "last_checkpoint").exists()


# ---- 4: data parallel ------------------------------------------------------------------------------------------------------------------
def solver_rank_worker(rank, world, port, tmp):
    """One real rank (gloo, every rank on cuda:0): two steps of the small --train-backbone trainer under full_model clipping and the guard."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=dp.TIMEOUT)
    try:
        model, shadow = resnet_tests.make_models()
        settings = SolverSettings(nesterov=True, bias_lr_factor=2.0, weight_decay_bias=0.0, clip_type="full_model", clip_value=1.0, guard_nonfinite=True)
        tr = train_head.HeadTrainer(model, base_lr=dp.LR, warmup_iters=0, steps=(1000, 2000), train_backbone=True, shadow=shadow, fused_step=True,
                                    data_parallel=(rank, world, None), solver=settings)
        for _ in range(2):
            images, gb, gc = dp.share(dp.frames(), rank, world, DEV)
            feats, padded = tr.features(images)
            tr.step(feats, padded, dp.HW, gb, gc)
        status = tr.check_finite()
        torch.cuda.synchronize()
        torch.save(dict(dp.state_of(tr), status=status), os.path.join(tmp, "rank_%d.pt" % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _spawned_solver_rank(i, *args):
    solver_rank_worker(i + 1, *args)


def test_two_ranks_under_full_model_clipping_end_with_the_same_bits_and_status(tmp_path):
    port = 37500 + os.getpid() % 2000
    dp.with_one_spawned_rank(solver_rank_worker, _spawned_solver_rank, (2, port, str(tmp_path)))
    r0, r1 = (torch.load(str(tmp_path / ("rank_%d.pt" % r)), weights_only=True) for r in range(2))
    dp.assert_same_state(r0, r1, "rank 0 against rank 1")
    assert r0["status"] == r1["status"] and r0["status"]["bad_steps"] == 0 and not r0["status"]["poisoned"]
    assert np.isfinite(r0["status"]["last_norm"]) and r0["status"]["last_norm"] > 0 and r0["iteration"] == 2
    assert all(bool(m.any()) for m in r0["momentum"])
