"""CPU side of training under the whole SOLVER section (K29): the referee against torch's optimiser and clipping utilities in fp64, the
schedules, the parameter groups and settings, every refused key, the new declarations and every refusal of pod_sgd_step_solver that comes
before a launch.  No GPU."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from pod_compare_amd import hip, losses, modeling, train_head
from pod_compare_amd.config import CfgNode
from pod_compare_amd.sgd_step import SolverSettings
from tests.solver_section import solver_ref

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NEW = ("pod_sgd_solver_workspace_bytes", "pod_sgd_step_solver", "pod_sgd_solver_reset")


# ---- the referee is torch's semantics ------------------------------------------------------------------------------------------------
SIZES = [1, 2, 3, 4, 5, 7, 9, 16, 17, 31, 36, 63, 64, 65, 100, 127, 128, 200, 255, 300]


@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
@pytest.mark.parametrize("clip_type", solver_ref.CLIP_TYPES)
def test_the_referee_is_torchs_sgd_with_two_groups_and_torchs_clipping(clip_type, nesterov):
    """20 small fp64 tensors, every third a `bias` (group 1), one without .grad and one with an all-zero gradient, two steps (the second
    with momentum): torch.optim.SGD(nesterov, two groups) behind torch.nn.utils.clip_grad_value_ / clip_grad_norm_ -- per parameter, or
    once over all of them for full_model -- against solver_ref.step, to 1e-12 relative to the terms' magnitudes."""
    gen = torch.Generator().manual_seed(11)
    params = [torch.nn.Parameter(torch.randn(n, generator=gen, dtype=torch.float64)) for n in SIZES]
    group = [1 if k % 3 == 1 else 0 for k in range(len(SIZES))]
    lr, wd, mu, v = [0.05, 0.11], [1e-2, 0.0], 0.9, 0.75
    opt = torch.optim.SGD([{"params": [p for p, g in zip(params, group) if g == 0]},
                           {"params": [p for p, g in zip(params, group) if g == 1], "lr": lr[1], "weight_decay": wd[1]}],
                          lr=lr[0], momentum=mu, weight_decay=wd[0], nesterov=nesterov)
    owner = np.concatenate([np.full(n, t) for t, n in enumerate(SIZES)])
    w = np.concatenate([p.detach().numpy() for p in params])
    m = np.zeros_like(w)
    torch_w, torch_m = w.copy(), m.copy()
    NO_GRAD, ZERO = 4, 9
    for call in range(2):
        has_grad = np.ones(len(SIZES), dtype=bool)
        for t, p in enumerate(params):
            p.grad = torch.randn(p.shape, generator=gen, dtype=torch.float64) * (3.0 if t % 2 else 0.2)
        params[ZERO].grad.zero_()
        params[(NO_GRAD + call) % len(SIZES)].grad = None
        has_grad[(NO_GRAD + call) % len(SIZES)] = False
        g = np.concatenate([np.zeros(p.numel()) if p.grad is None else p.grad.numpy().copy() for p in params])
        have = [p for p in params if p.grad is not None]
        if clip_type == "value":
            for p in have:
                torch.nn.utils.clip_grad_value_(p, v)
        elif clip_type == "norm":
            for p in have:
                torch.nn.utils.clip_grad_norm_(p, v)
        elif clip_type == "full_model":
            total = torch.nn.utils.clip_grad_norm_(have, v)
        opt.step()
        ref = solver_ref.step(w, m, g, np.ones_like(w), owner, has_grad, group, lr, wd, mu, nesterov=nesterov, clip_type=clip_type, clip_value=v)
        got_w = np.concatenate([p.detach().numpy() for p in params])
        got_m = np.concatenate([opt.state[p]["momentum_buffer"].numpy() if "momentum_buffer" in opt.state.get(p, {}) else np.zeros(p.numel()) for p in params])
        # relative to the magnitudes of the terms a result is the sum of (a stepped weight may cancel to nearly nothing)
        live = ref["live"]
        scale_w, scale_m = np.abs(w), np.abs(m)
        scale_w[live] += np.abs(ref["lr"] * ref["d"])
        scale_m[live] = mu * np.abs(m[live]) + np.abs(ref["a"]) + ref["wd"] * np.abs(w[live])
        assert np.all(np.abs(got_w - ref["w"]) <= 1e-12 * scale_w), (call, float(np.abs(got_w - ref["w"]).max()))
        assert np.all(np.abs(got_m - ref["m"]) <= 1e-12 * scale_m), (call, float(np.abs(got_m - ref["m"]).max()))
        assert np.array_equal(got_w[~live], torch_w[~live]) and np.array_equal(got_m[~live], torch_m[~live])      # torch skips it too
        if clip_type == "full_model":
            assert abs(float(total) - math.sqrt(ref["total"])) <= 1e-12 * float(total)
            assert ref["coef_all"] < 1.0                                    # (the threshold bites: the case is not the identity)
        assert ref["coef"][ZERO] == 1.0 and ref["sumsq"][ZERO] == 0.0
        assert ref["sumsq"][(NO_GRAD + call) % len(SIZES)] == 0.0 and not ref["live"][owner == (NO_GRAD + call) % len(SIZES)].any()
        assert (ref["coef"] < 1.0).any() and (ref["coef"] == 1.0).sum() >= 2  # some tensors over the threshold, some under it
        if clip_type == "value":
            assert (np.abs(ref["a0"]) > v).any() and np.abs(ref["a"]).max() == v
        w, m, torch_w, torch_m = ref["w"], ref["m"], got_w, got_m
    skipped = params[NO_GRAD]
    assert skipped.grad is not None                                         # it was skipped in call 0 and stepped in call 1


def test_the_referee_keeps_a_nan_through_value_clipping_and_the_coefficient():
    r = solver_ref.step([1.0, 1.0], [0.0, 0.0], [float("nan"), 5.0], [1.0, 1.0], [0, 0], [True], [0], [0.1], [0.0], 0.9, clip_type="value", clip_value=1.0)
    assert math.isnan(r["a"][0]) and r["a"][1] == 1.0
    assert math.isnan(float(solver_ref.clip_coef(float("nan"), 1.0))) and float(solver_ref.clip_coef(float("inf"), 1.0)) == 0.0


# ---- schedules ---------------------------------------------------------------------------------------------------------------------
SCHEDULE = dict(steps=(60000, 80000), gamma=0.1, warmup_iters=1000, warmup_factor=1e-3)


def test_default_keys_give_warmup_multistep_lr_to_the_bit():
    for it in (0, 1, 999, 1000, 60000, 80000):
        for base in (0.001, 0.001 * 2.0):
            assert train_head.scheduled_lr(it, base, **SCHEDULE) == train_head.warmup_multistep_lr(it, base, **SCHEDULE), it


def test_cosine_schedule_and_constant_warmup_against_their_closed_forms():
    base, max_iter = 0.01, 90000
    for it in (0, 1, 500, 999, 1000, 45000, 89999):
        warm_lin = 1.0 if it >= 1000 else 1e-3 * (1 - it / 1000.0) + it / 1000.0
        warm_const = 1.0 if it >= 1000 else 1e-3
        cos = 0.5 * (1.0 + math.cos(math.pi * it / max_iter))
        got = train_head.scheduled_lr(it, base, lr_scheduler_name="WarmupCosineLR", max_iter=max_iter, **SCHEDULE)
        assert got == pytest.approx(base * warm_lin * cos, rel=1e-15), it
        got = train_head.scheduled_lr(it, base, lr_scheduler_name="WarmupCosineLR", warmup_method="constant", max_iter=max_iter, **SCHEDULE)
        assert got == pytest.approx(base * warm_const * cos, rel=1e-15), it
        got = train_head.scheduled_lr(it, base, warmup_method="constant", **SCHEDULE)
        assert got == pytest.approx(base * warm_const * 0.1 ** ((it >= 60000) + (it >= 80000)), rel=1e-15), it
    assert train_head.warmup_factor_at(999, 1000, 1e-3, "constant") == 1e-3 and train_head.warmup_factor_at(1000, 1000, 1e-3, "constant") == 1.0
    assert train_head.scheduled_lr(45000, base, lr_scheduler_name="WarmupCosineLR", max_iter=max_iter, **SCHEDULE) == pytest.approx(base * 0.5, rel=1e-12)
    with pytest.raises(ValueError):
        train_head.scheduled_lr(0, base, lr_scheduler_name="Other", **SCHEDULE)


# ---- groups and settings -----------------------------------------------------------------------------------------------------------
def _cfg(**solver):
    base = {"BASE_LR": 0.001, "MOMENTUM": 0.9, "WEIGHT_DECAY": 1e-4}
    base.update(solver)
    return CfgNode({"SOLVER": CfgNode({k: CfgNode(v) if isinstance(v, dict) else v for k, v in base.items()})})


def test_a_config_that_names_none_of_the_keys_gives_the_default_settings_and_todays_path():
    assert train_head.solver_settings(_cfg()) == SolverSettings() and SolverSettings().plain_step
    # what collapses to the defaults: a factor of 1 with equal decays, clipping that is not enabled, the default names
    same = _cfg(BIAS_LR_FACTOR=1.0, WEIGHT_DECAY_BIAS=1e-4, WEIGHT_DECAY_NORM=0.0, NESTEROV=False, LR_SCHEDULER_NAME="WarmupMultiStepLR",
                WARMUP_METHOD="linear", CLIP_GRADIENTS={"ENABLED": False, "CLIP_TYPE": "norm", "CLIP_VALUE": 5.0, "NORM_TYPE": 2.0})
    s = train_head.solver_settings(same)
    assert s == SolverSettings() and s.plain_step and not s.two_groups and not s.computes_norm
    s = train_head.solver_settings(_cfg(NESTEROV=True, BIAS_LR_FACTOR=2.0, WEIGHT_DECAY_BIAS=0.0, LR_SCHEDULER_NAME="WarmupCosineLR", WARMUP_METHOD="constant",
                                        CLIP_GRADIENTS={"ENABLED": True, "CLIP_TYPE": "full_model", "CLIP_VALUE": 0.5}), guard_nonfinite=True)
    assert s == SolverSettings(nesterov=True, bias_lr_factor=2.0, weight_decay_bias=0.0, clip_type="full_model", clip_value=0.5,
                               lr_scheduler_name="WarmupCosineLR", warmup_method="constant", guard_nonfinite=True)
    assert not s.plain_step and s.two_groups and s.computes_norm
    assert train_head.solver_settings(_cfg(CLIP_GRADIENTS={"ENABLED": True})) == SolverSettings(clip_type="value", clip_value=1.0)
    assert not SolverSettings(clip_type="value").computes_norm and SolverSettings(guard_nonfinite=True).computes_norm
    assert SolverSettings(weight_decay_bias=0.0).two_groups and not SolverSettings(nesterov=True).two_groups


def test_biases_of_head_and_fpn_go_to_group_1_weights_and_masters_to_group_0():
    names = ["head.cls_subnet.0.weight", "head.cls_subnet.0.bias", "head.cls_score.bias", "backbone.fpn_lateral3.weight", "backbone.fpn_lateral3.bias",
             "backbone.fpn_output5.bias", "backbone.top_block.p6.weight", "backbone.bottom_up.res3.0.conv1.weight", "backbone.bottom_up.res5.2.conv3.weight"]
    two = SolverSettings(bias_lr_factor=2.0)
    assert train_head.parameter_groups(names, two) == [0, 1, 1, 0, 1, 1, 0, 0, 0]
    assert train_head.parameter_groups(names, SolverSettings(nesterov=True)) == [0] * len(names)
    # the trainer: torch's optimiser gets the biases as a second group with their own rate and decay, and nesterov
    torch.manual_seed(5)
    model = modeling.ProbabilisticRetinaNet(num_classes=7).eval()
    model.loss_state = losses.ProbabilisticLosses(num_classes=7, cls_var_num_samples=3, annealing_step=80000, seed=11)
    tr = train_head.HeadTrainer(model, base_lr=0.01, warmup_iters=10, warmup_factor=0.1, train_fpn=True,
                                solver=SolverSettings(nesterov=True, bias_lr_factor=2.0, weight_decay_bias=0.0))
    assert tr.groups == [1 if n.endswith(".bias") else 0 for n in tr.param_names()] and 0 < sum(tr.groups) < len(tr.groups)
    assert len(tr.opt.param_groups) == 2 and tr.opt.param_groups[0]["nesterov"] and tr.opt.param_groups[1]["weight_decay"] == 0.0
    assert tr.opt.param_groups[0]["weight_decay"] == 1e-4
    assert {id(p) for p in tr.opt.param_groups[1]["params"]} == {id(p) for p, g in zip(tr.params, tr.groups) if g == 1}
    assert tr.lrs_at(0) == [train_head.warmup_multistep_lr(0, **tr.schedule), train_head.warmup_multistep_lr(0, **dict(tr.schedule, base_lr=0.01 * 2.0))]
    assert tr.lr == tr.lrs_at(0)[0] and tr.check_finite() is None and tr.grad_norm() is None
    # the default settings: one group, as before
    plain = train_head.HeadTrainer(model, base_lr=0.01)
    assert len(plain.opt.param_groups) == 1 and not plain.opt.param_groups[0]["nesterov"] and plain.groups == [0] * len(plain.params)
    assert plain.lrs_at(7) == [train_head.warmup_multistep_lr(7, **plain.schedule)]
    with pytest.raises(ValueError):
        train_head.HeadTrainer(model, guard_nonfinite=True)                  # the guard is the fused step's


@pytest.mark.parametrize("key,text", [
    ("CLIP_GRADIENTS.CLIP_TYPE", "SOLVER:\n  CLIP_GRADIENTS:\n    ENABLED: True\n    CLIP_TYPE: median\n"),
    ("LR_SCHEDULER_NAME", "SOLVER:\n  LR_SCHEDULER_NAME: WarmupStepWithFixedGammaLR\n"),
    ("WARMUP_METHOD", "SOLVER:\n  WARMUP_METHOD: burnin\n"),
    ("CLIP_GRADIENTS.NORM_TYPE", "SOLVER:\n  CLIP_GRADIENTS:\n    ENABLED: True\n    CLIP_TYPE: norm\n    NORM_TYPE: 1.0\n"),
    ("CLIP_GRADIENTS.CLIP_VALUE", "SOLVER:\n  CLIP_GRADIENTS:\n    ENABLED: True\n    CLIP_VALUE: 0.0\n"),
    ("CLIP_GRADIENTS.CLIP_VALUE", "SOLVER:\n  CLIP_GRADIENTS:\n    ENABLED: True\n    CLIP_VALUE: -1.0\n"),
    ("CLIP_GRADIENTS.CLIP_VALUE", "SOLVER:\n  CLIP_GRADIENTS:\n    ENABLED: True\n    CLIP_VALUE: .inf\n"),
    ("CLIP_GRADIENTS.CLIP_VALUE", "SOLVER:\n  CLIP_GRADIENTS:\n    ENABLED: True\n    CLIP_VALUE: .nan\n"),
    ("BIAS_LR_FACTOR", "SOLVER:\n  BIAS_LR_FACTOR: -2.0\n"),
    ("BIAS_LR_FACTOR", "SOLVER:\n  BIAS_LR_FACTOR: .inf\n"),
    ("WEIGHT_DECAY_BIAS", "SOLVER:\n  WEIGHT_DECAY_BIAS: -0.0001\n"),
    ("WEIGHT_DECAY_BIAS", "SOLVER:\n  WEIGHT_DECAY_BIAS: .nan\n"),
])
def test_every_bad_solver_key_is_refused_by_name_before_a_model_is_built(tmp_path, key, text):
    """test_only_the_default_freeze_point_is_accepted's construction: an empty ground-truth file, no GPU touched."""
    yaml = tmp_path / "m.yaml"
    yaml.write_text(text)
    (tmp_path / "gt.json").write_text('{"images": [], "annotations": []}')
    with pytest.raises(SystemExit) as e:
        train_head.main(["--config-file", str(yaml), "--coco-json", str(tmp_path / "gt.json"), "--image-root", str(tmp_path)])
    assert "SOLVER." + key in str(e.value) and "not supported" in str(e.value)


def test_the_command_offers_the_guard():
    ap = train_head.arg_parser()
    base = ["--coco-json", "x", "--image-root", "y"]
    assert ap.parse_args(base).guard_nonfinite is False and ap.parse_args(base + ["--guard-nonfinite"]).guard_nonfinite is True


# ---- the declarations --------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_carry_the_solver_step():
    from pod_compare_amd import build
    from tests.test_abi_cpu import HEADER, declared_symbols
    for name in NEW:
        assert name in hip.EXPORTS and name in declared_symbols()
    assert "pod_sgd_solver_workspace_bytes" in hip._SIZE_QUERIES
    header = open(HEADER).read()
    assert hip.POD_ABI_VERSION == 18 and "#define POD_ABI_VERSION 18\n" in header
    assert "#define POD_SGD_MAX_GROUPS %d\n" % hip.POD_SGD_MAX_GROUPS in header and hip.POD_SGD_MAX_GROUPS == 8
    for name, value in (("OFF", 0), ("VALUE", 1), ("NORM", 2), ("FULL_MODEL", 3)):
        assert getattr(hip, "POD_SGD_CLIP_" + name) == value and ("#define POD_SGD_CLIP_%s" % name) in header
    assert "k29_sgd_solver.hip" in build.SOURCES
    lib = ctypes.CDLL(build.build_library())
    assert lib.pod_abi_version() == hip.POD_ABI_VERSION and all(hasattr(lib, n) for n in NEW)
    bound = hip.load()
    assert bound.pod_sgd_solver_workspace_bytes.restype is ctypes.c_size_t and len(bound.pod_sgd_step_solver.argtypes) == 10
    assert bound.pod_sgd_solver_workspace_bytes(0, 0) == 48 and bound.pod_sgd_solver_workspace_bytes(3, 5) == 96      # 32 + 8 * 5 + 4 * 4 = 88 -> 96
    assert bound.pod_sgd_solver_workspace_bytes(-1, 0) == 0 and bound.pod_sgd_solver_workspace_bytes(0, -1) == 0


def test_solver_record_and_status_layouts_match_c(tmp_path):
    """sizeof / offsetof of hip.PodSgdSolver and hip.PodSgdSolverStatus against the header, compiled with gcc."""
    src = tmp_path / "layout.c"
    body = ""
    for cls in (hip.PodSgdSolver, hip.PodSgdSolverStatus):
        body += 'printf(" %%zu", sizeof(%s));\n' % cls.__name__
        body += "".join('printf(" %%zu", offsetof(%s, %s));\n' % (cls.__name__, f) for f, _ in cls._fields_)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pod_mi355x.h"\nint main(void){\n' + body + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for cls in (hip.PodSgdSolver, hip.PodSgdSolverStatus):
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    assert got == want and ctypes.sizeof(hip.PodSgdSolverStatus) == 32 and ctypes.sizeof(hip.PodSgdSolver) % 8 == 0


# ---- refusals before any launch ------------------------------------------------------------------------------------------------------
GOOD = dict(w=0x10000, grad=0x20000, momentum=0x30000, folded=0x40000, scale=0x50000, n=27 * 64, per_channel=27)
PLAIN = dict(w=0x60000, grad=0x70000, momentum=0x80000, n=63)
VALID_CHUNKS = -(-GOOD["n"] // hip.POD_SGD_CHUNK) + 1
WS, GROUP_DEV, TABLE_DEV, MAP = 0xB0000, 0xC0000, 0x90000, 0xA0000


def _record(**kw):
    r = hip.PodSgdSolver()
    r.n_groups, r.momentum, r.clip_value = 2, 0.9, 1.0
    r.lr[0], r.lr[1], r.wd[0], r.wd[1] = 0.01, 0.02, 1e-4, 0.0
    for k, v in kw.items():
        if isinstance(v, tuple):                                             # (index, value) into an array field
            getattr(r, k)[v[0]] = v[1]
        else:
            setattr(r, k, v)
    return r


def _call(rows=(GOOD, PLAIN), group=(0, 1), record=None, n_tensors=None, n_chunks=VALID_CHUNKS, table_dev=TABLE_DEV, chunk_map=MAP, group_dev=GROUP_DEV,
          workspace=WS, null_table=False, null_group=False, null_record=False):
    """pod_sgd_step_solver on host addresses that are never dereferenced: whatever it returns comes from the argument checks."""
    t = (hip.PodSgdTensor * max(1, len(rows)))()
    for d, r in zip(t, rows):
        for k, v in r.items():
            setattr(d, k, v)
    g = (ctypes.c_uint8 * max(1, len(group)))(*group)
    rec = _record() if record is None else record
    return hip.load().pod_sgd_step_solver(None if null_table else t, table_dev, len(rows) if n_tensors is None else n_tensors, chunk_map, n_chunks,
                                          None if null_group else g, group_dev, None if null_record else ctypes.byref(rec), workspace, None)


def test_the_valid_call_passes_every_check_that_comes_before_the_device_is_touched():
    """The refusals below each differ from the valid call in one argument.  With the device-side pointers missing it is refused last of
    all, after every check of the descriptors, groups and settings; with nothing to do it returns POD_OK without touching anything."""
    for kw in (dict(table_dev=None), dict(chunk_map=None), dict(workspace=None), dict(group_dev=None), dict(workspace=WS + 8)):
        assert _call(**kw) == -1, kw
    empty = [dict(GOOD, n=0), dict(PLAIN, n=0)]
    assert _call(rows=empty, n_chunks=0, table_dev=None, chunk_map=None, workspace=None, group_dev=None) == 0           # every n == 0
    assert _call(rows=(), group=(), n_tensors=0, n_chunks=0, null_table=True, null_group=True, table_dev=None, chunk_map=None, workspace=None, group_dev=None) == 0
    for rec in (_record(nesterov=1), _record(clip_type=3, guard=1), _record(n_groups=8), _record(clip_type=0, clip_value=float("nan"))):
        assert _call(rows=empty, n_chunks=0, record=rec) == 0                # valid settings of every kind
    assert hip.load().pod_sgd_solver_reset(None, None) == -1 and hip.load().pod_sgd_solver_reset(WS + 4, None) == -1


@pytest.mark.parametrize("name,kw", [
    ("null table", dict(null_table=True)),
    ("n_tensors < 0", dict(n_tensors=-1)),
    ("null w", dict(rows=(dict(GOOD, w=None), PLAIN))),
    ("grad misaligned", dict(rows=(dict(GOOD, grad=0x20004), PLAIN))),
    ("folded without scale", dict(rows=(dict(GOOD, scale=None), PLAIN))),
    ("n % per_channel", dict(rows=(dict(GOOD, per_channel=25), PLAIN))),
    ("w == momentum", dict(rows=(GOOD, dict(PLAIN, momentum=PLAIN["w"])))),
    ("another table's chunk count", dict(n_chunks=VALID_CHUNKS + 1)),
    ("null record", dict(null_record=True)),
    ("n_groups 0", dict(record=_record(n_groups=0))),
    ("n_groups 9", dict(record=_record(n_groups=9))),
    ("a group at n_groups", dict(group=(0, 2))),
    ("a group at n_groups, one group", dict(record=_record(n_groups=1))),
    ("null group", dict(null_group=True)),
    ("lr nan", dict(record=_record(lr=(0, float("nan"))))),
    ("lr of group 1 inf", dict(record=_record(lr=(1, float("inf"))))),
    ("lr negative", dict(record=_record(lr=(1, -0.01)))),
    ("wd negative", dict(record=_record(wd=(0, -1e-4)))),
    ("wd of group 1 nan", dict(record=_record(wd=(1, float("nan"))))),
    ("momentum 1", dict(record=_record(momentum=1.0))),
    ("momentum < 0", dict(record=_record(momentum=-0.1))),
    ("momentum nan", dict(record=_record(momentum=float("nan")))),
    ("nesterov with momentum 0", dict(record=_record(nesterov=1, momentum=0.0))),
    ("clip_type 4", dict(record=_record(clip_type=4))),
    ("clip_type -1", dict(record=_record(clip_type=-1))),
    ("clip value 0", dict(record=_record(clip_type=1, clip_value=0.0))),
    ("clip norm negative", dict(record=_record(clip_type=2, clip_value=-1.0))),
    ("clip full_model inf", dict(record=_record(clip_type=3, clip_value=float("inf")))),
    ("clip value nan", dict(record=_record(clip_type=1, clip_value=float("nan")))),
    ("watch misaligned", dict(record=_record(guard=1, watch=(1, 0xD0002)))),
])
def test_refusals_before_any_launch(name, kw):
    """Each call is the valid one with ONE argument changed.  Nothing is enqueued: the addresses are not device memory."""
    assert _call(**kw) == -1, name
