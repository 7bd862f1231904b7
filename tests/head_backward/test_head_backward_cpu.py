"""CPU side of the head's backward pass: the fp64 identities the design rests on, the declarations of the new entry points, their
argument validation, the solver defaults and the learning-rate schedule; the head's launch plan in its two forms.  No GPU."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from pod_compare_amd import config, hip
from pod_compare_amd.head_train import transposed_weight
from pod_compare_amd.train_head import warmup_multistep_lr

NEW = ("pod_conv3x3_wgrad", "pod_conv3x3_wgrad_partials", "pod_relu_dropout_backward")


@pytest.mark.parametrize("K,C", [(64, 16), (63, 32), (36, 64)])
def test_input_gradient_is_a_forward_convolution_with_the_flipped_transposed_filter(K, C):
    """conv2d(dZ, W'), W'[c][k][ky][kx] = W[k][c][2 - ky][2 - kx], equals autograd's input gradient -- also with the predictor's
    channels zero-padded to 64 in dZ and in W' (padding changes nothing: the padded products are zeros)."""
    g = torch.Generator().manual_seed(K)
    w = torch.randn((K, C, 3, 3), generator=g, dtype=torch.float64)
    x = torch.randn((2, C, 7, 9), generator=g, dtype=torch.float64, requires_grad=True)
    dz = torch.randn((2, K, 7, 9), generator=g, dtype=torch.float64)
    F.conv2d(x, w, padding=1).backward(dz)
    wt = transposed_weight(w)
    Kpad = (K + 63) // 64 * 64
    assert tuple(wt.shape) == (C, Kpad, 3, 3) and bool((wt[:, K:] == 0).all())
    dz_pad = torch.zeros((2, Kpad, 7, 9), dtype=torch.float64)
    dz_pad[:, :K] = dz
    got = F.conv2d(dz_pad, wt, padding=1)
    assert float((got - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    unpadded = F.conv2d(dz, wt[:, :K].contiguous(), padding=1)
    assert float((got - unpadded).abs().max()) <= 1e-12 * float(unpadded.abs().max())


def test_patch_matrix_times_the_laid_out_filter_is_that_convolution(monkeypatch):
    """The form the input gradient runs in: rows of nine shifted channel vectors (zeros outside each image, never a neighbouring image's
    or level's pixels) times W' as (C, ty, tx, Kpad) equal conv2d(dZ, W') per level and image.  (The abs-max record is a GPU matter.)"""
    from pod_compare_amd import amax, head_train
    monkeypatch.setattr(amax, "of", lambda t: None)
    monkeypatch.setattr(amax, "attach", lambda t, w: t)
    levels, B, K, C = [(5, 7), (3, 4), (1, 1)], 2, 36, 64
    g = torch.Generator().manual_seed(0)
    wt = transposed_weight(torch.randn((K, C, 3, 3), generator=g, dtype=torch.float64))
    Kpad, pixels = wt.shape[1], B * sum(h * w for h, w in levels)
    dz = torch.randn((pixels, Kpad), generator=g, dtype=torch.float64)
    dx = head_train.patch_matrix(dz, levels, B) @ wt.permute(0, 2, 3, 1).reshape(C, 9 * Kpad).t()
    off = 0
    for h, w in levels:
        n = B * h * w
        want = F.conv2d(dz[off:off + n].view(B, h, w, Kpad).permute(0, 3, 1, 2), wt, padding=1)
        got = dx[off:off + n].view(B, h, w, C).permute(0, 3, 1, 2)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
        off += n


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_gate_identity(p):
    """dOut (out > 0) / (1 - p) equals autograd through dropout(relu(z)) on a fixed mask: the stored output is its own gate."""
    g = torch.Generator().manual_seed(11)
    z = torch.randn((3, 8, 5, 6), generator=g, dtype=torch.float64, requires_grad=True)
    keep = (torch.rand((3, 8, 5, 6), generator=g) >= p).double()
    out = torch.relu(z) * keep / (1.0 - p)
    d_out = torch.randn((3, 8, 5, 6), generator=g, dtype=torch.float64)
    out.backward(d_out)
    gate = d_out * (out.detach() > 0).double() / (1.0 - p)
    assert torch.equal(gate, z.grad)
    assert bool(((out.detach() == 0) == ((z.detach() <= 0) | (keep == 0))).all())


def test_header_binding_and_library_carry_the_backward_entry_points():
    """Additions only: the three symbols are declared, bound and exported; the ABI number stays where K20 / K21 left it."""
    from pod_compare_amd import build
    from tests.test_abi_cpu import HEADER, declared_symbols
    for name in NEW:
        assert name in hip.EXPORTS and name in declared_symbols()
    assert "pod_conv3x3_wgrad_partials" in hip._SIZE_QUERIES
    assert hip.POD_ABI_VERSION == 18 and "#define POD_ABI_VERSION 18\n" in open(HEADER).read()
    lib = ctypes.CDLL(build.build_library())
    assert lib.pod_abi_version() == hip.POD_ABI_VERSION and all(hasattr(lib, n) for n in NEW)
    assert "k22_conv3x3_wgrad.hip" in build.SOURCES and "-fno-slp-vectorize" in build.SOURCE_FLAGS["k22_conv3x3_wgrad.hip"]
    bound = hip.load()
    assert bound.pod_conv3x3_wgrad_partials.restype is ctypes.c_int64 and len(bound.pod_conv3x3_wgrad.argtypes) == 14
    assert len(bound.pod_relu_dropout_backward.argtypes) == 7


def _levels(*hw):
    arr = (ctypes.c_int32 * (2 * len(hw)))()
    for i, (h, w) in enumerate(hw):
        arr[2 * i], arr[2 * i + 1] = h, w
    return arr


def test_partials_query_follows_the_slice_rule():
    """Slices of 256 row segments of 16 pixels and db chunks of 4096 pixels, from the geometry alone."""
    lib = hip.load()
    q = lambda lv, n, copies, C, K, Kpad: lib.pod_conv3x3_wgrad_partials(lv, n, copies, C, K, Kpad)
    assert q(_levels((256, 16)), 1, 1, 16, 64, 64) == 2 * 1 * 64 + 1 * 9 * 64 * 16                 # exactly one slice, one chunk
    assert q(_levels((300, 20)), 1, 1, 16, 64, 64) == 2 * 2 * 64 + 3 * 9 * 64 * 16                 # 600 segments, 6000 pixels
    assert q(_levels((9, 13), (5, 7)), 2, 2, 32, 63, 64) == 2 * 1 * 64 + 1 * 9 * 64 * 32
    assert q(_levels((92, 160), (46, 80), (23, 40), (12, 20), (6, 10)), 5, 4, 256, 256, 256) == 2 * 20 * 256 + 20 * 9 * 256 * 256
    for bad in ((_levels((5, 7)), 1, 1, 24, 64, 64), (_levels((5, 7)), 1, 1, 16, 65, 64), (_levels((5, 7)), 1, 1, 16, 64, 96),
                (_levels((0, 7)), 1, 1, 16, 64, 64), (_levels((5, 7)), 0, 1, 16, 64, 64), (_levels((5, 7)), 1, 0, 16, 64, 64),
                (None, 1, 1, 16, 64, 64), (_levels((5, 7)), 9, 1, 16, 64, 64), (_levels((5, 7)), 1, 1, 16, 576, 576)):
        assert q(*bad) == 0, bad[1:]


def test_backward_entry_points_reject_invalid_arguments_without_a_gpu():
    lib = hip.load()
    buf = ctypes.create_string_buffer(2048)
    X = (ctypes.addressof(buf) + 15) & ~15
    lv = _levels((5, 7))

    # (never dereferenced; distinct, so that each call below has the one defect it names)
    def wg(x=X, dy=X + 256, levels=lv, n=1, copies=1, C=16, K=64, Kpad=64, xa=X + 512, da=X + 516, dW=X + 768, db=X + 1024, partials=X + 1280):
        return lib.pod_conv3x3_wgrad(x, dy, levels, n, copies, C, K, Kpad, xa, da, dW, db, partials, None)

    for kw in ({"x": None}, {"dy": None}, {"levels": None}, {"xa": None}, {"da": None}, {"dW": None}, {"db": None}, {"partials": None},
               {"n": 0}, {"copies": 0}, {"C": 8}, {"C": 24}, {"K": 0}, {"K": 65}, {"Kpad": 32}, {"x": X + 4}, {"partials": X + 1288}):
        assert wg(**kw) == -1, kw
    # what pod_conv1x1_wgrad_strided refuses, every weight gradient refuses: aliased outputs, a record or output off 4 bytes
    for kw in ({"dW": X}, {"dW": X + 1280}, {"db": X + 768}, {"xa": X + 514}, {"da": X + 518}, {"dW": X + 770}, {"db": X + 1026},
               {"dW": X + 256}, {"partials": X}, {"partials": X + 256}, {"db": X + 1280}):
        assert wg(**kw) == -1, kw
    gate = lambda out=X, d=X, dz=X, n=64, p=0.1: lib.pod_relu_dropout_backward(out, d, dz, n, p, None, None)
    for kw in ({"out": None}, {"d": None}, {"dz": None}, {"n": -4}, {"n": 6}, {"p": 1.0}, {"p": -0.1}, {"out": X + 4}):
        assert gate(**kw) == -1, kw
    assert gate(n=0) == 0


def test_solver_defaults_are_detectron2s():
    s = config.get_cfg().SOLVER
    assert (s.BASE_LR, s.MOMENTUM, s.WEIGHT_DECAY, s.WARMUP_ITERS, s.WARMUP_FACTOR, s.GAMMA, s.MAX_ITER, s.CHECKPOINT_PERIOD) == \
        (0.001, 0.9, 0.0001, 1000, 0.001, 0.1, 40000, 5000)
    import os
    here = os.path.dirname(os.path.abspath(config.__file__))
    cfg = config.setup_config(os.path.join(here, "configs/BDD-Detection/retinanet/retinanet_R_50_FPN_1x_reg_cls_var_dropout.yaml"))
    s = cfg.SOLVER                      # the BDD base file's own values over the defaults
    assert (s.IMS_PER_BATCH, s.BASE_LR, tuple(s.STEPS), s.MAX_ITER, s.CHECKPOINT_PERIOD, s.MOMENTUM, s.WARMUP_ITERS) == \
        (4, 0.0025, (60000, 80000), 90000, 30000, 0.9, 1000)


def test_learning_rate_schedule_at_its_corners():
    """detectron2's WarmupMultiStepLR by hand: base 0.0025, warm-up 1000 iterations from factor 1/1000, x 0.1 at 60000 and 80000."""
    lr = lambda it: warmup_multistep_lr(it, 0.0025, (60000, 80000), 0.1, 1000, 0.001)
    close = lambda a, b: abs(a - b) <= 1e-15 + 1e-12 * abs(b)
    assert close(lr(0), 0.0025 * 0.001)                                     # warm-up start: base x factor
    assert close(lr(500), 0.0025 * (0.001 * 0.5 + 0.5))                     # half way: linear in the iteration
    assert close(lr(999), 0.0025 * (0.001 * 0.001 + 0.999))                 # the last warm-up iteration
    assert lr(1000) == 0.0025 and lr(59999) == 0.0025                       # warm-up end .. the first boundary
    assert close(lr(60000), 0.00025) and close(lr(79999), 0.00025)
    assert close(lr(80000), 0.000025) and close(lr(89999), 0.000025)
    assert close(warmup_multistep_lr(10, 0.01, (5, 20), 0.5, 100, 0.1), 0.01 * (0.1 * 0.9 + 0.1) * 0.5)   # a boundary inside the warm-up


# ---- the head's launch plan (modeling.ProbabilisticRetinaNetHead._trunk_plan), which the inference and the training forward both run -------
PLAN_LEVELS, PLAN_C, PLAN_PIXELS = [(12, 20), (6, 10), (3, 5)], 64, 12 * 20 + 6 * 10 + 3 * 5


def plan_of(monkeypatch, p, subnets, **st):
    """-> (head, the plan of a 4-layer head of 64 channels at _drop_calls = 7 on CPU tensors, x0, the block_table calls it made)"""
    from pod_compare_amd import modeling, wino
    head = modeling.ProbabilisticRetinaNetHead(in_channels=PLAN_C, num_convs=4, dropout_rate=p, compute_cls_var=True, compute_bbox_cov=True)
    head._drop_calls = 7
    tables, real = [], wino.block_table

    def block_table(levels, copies, device, **kw):
        tables.append((list(levels), copies, kw))
        return real(levels, copies, device, **kw)
    monkeypatch.setattr(wino, "block_table", block_table)
    x0 = torch.zeros(PLAN_PIXELS * st.get("images", 1), PLAN_C)
    plan = head._trunk_plan(subnets, modeling.HeadPlan(x0=x0, levels=PLAN_LEVELS, grouped=True, **st))
    assert len(plan["layers"]) == 4 and all(len(sets) == len(subnets) for sets in plan["layers"])
    assert all(s["conv"] is (head.cls_subnet, head.bbox_subnet)[sid][l] for l, sets in enumerate(plan["layers"]) for s, (sid, _) in zip(sets, subnets))
    return head, plan, x0, tables


def test_inference_plan_with_mc_dropout(monkeypatch):
    head, plan, x0, tables = plan_of(monkeypatch, 0.1, [(0, 4), (1, 6)], dropout=True)
    layers = plan["layers"]
    assert [[s["offset"] for s in sets] for sets in layers] == [[8 << 34, 12 << 34], [9 << 34, 13 << 34], [10 << 34, 14 << 34], [11 << 34, 15 << 34]]
    assert [[s.get("replicas") for s in sets] for sets in layers] == [[4, 6], [None, None], [None, None], [None, None]]
    assert head._drop_calls == 7 + 8 and plan["copies"] == [4, 6] and not plan["replay"]
    assert plan["kw"] == {"relu": True, "dropout_p": 0.1, "seed": head.dropout_seed, "epoch": head._epoch}
    for i, c in enumerate((4, 6)):
        a, b = layers[0][i]["dst"], layers[1][i]["dst"]
        assert layers[0][i]["src"] is x0 and a is not b and tuple(a.shape) == tuple(b.shape) == (c * PLAN_PIXELS, PLAN_C)
        assert all(sets[i]["src"] is x and sets[i]["dst"] is y for sets, x, y in zip(layers[1:], (a, b, a), (b, a, b)))       # ping-pong
        assert layers[0][i]["table"].pod_pixels == PLAN_PIXELS and all(sets[i]["table"].pod_pixels == c * PLAN_PIXELS for sets in layers[1:])
    assert layers[0][0]["dst"] is not layers[0][1]["dst"]
    assert tables == [(PLAN_LEVELS, 4, {"channels": 512}), (PLAN_LEVELS, 6, {"channels": 512}),
                      (PLAN_LEVELS, 1, {"out_copies": 4, "channels": 512}), (PLAN_LEVELS, 1, {"out_copies": 6, "channels": 512})]


def test_inference_plan_without_dropout(monkeypatch):
    head, plan, x0, tables = plan_of(monkeypatch, 0.1, [(0, 4), (1, 6)], dropout=False)
    assert plan["copies"] == [1, 1] and plan["kw"] == {"relu": True} and head._drop_calls == 7
    assert all(s["offset"] == 0 and "replicas" not in s and tuple(s["dst"].shape) == (PLAN_PIXELS, PLAN_C) for sets in plan["layers"] for s in sets)
    assert tables == [(PLAN_LEVELS, 1, {"channels": 512})] * 2


@pytest.mark.parametrize("p", [0.1, 0.0])
def test_training_plan(monkeypatch, p):
    head, plan, x0, tables = plan_of(monkeypatch, p, [(0, 2), (1, 2)], dropout=False, images=2, channels=max(PLAN_C, 64))
    layers = plan["layers"]
    assert not any("replicas" in s for sets in layers for s in sets)
    dsts = [s["dst"] for sets in layers for s in sets]
    assert len({id(t) for t in dsts}) == 8 and all(tuple(t.shape) == (2 * PLAN_PIXELS, PLAN_C) for t in dsts)
    for i in range(2):
        assert layers[0][i]["src"] is x0 and all(layers[l][i]["src"] is layers[l - 1][i]["dst"] for l in range(1, 4))
    assert tables == [(PLAN_LEVELS, 2, {"channels": 64})] * 2
    assert [[s["offset"] for s in sets] for sets in layers] == [[8 << 34, 12 << 34], [9 << 34, 13 << 34], [10 << 34, 14 << 34], [11 << 34, 15 << 34]]
    assert head._drop_calls == 7 + 8 and plan["copies"] == [2, 2]
    assert plan["kw"] == {"relu": True, "dropout_p": p, "seed": head.dropout_seed, "epoch": head._epoch}
    if p > 0.0:                                                    # replay: the launches draw no masks, the recorded ones are applied after them
        head._drop_calls = 7
        head.dropout_replay = lambda sid, layer, level, copy_: None
        from pod_compare_amd.modeling import HeadPlan
        again = head._trunk_plan([(0, 2), (1, 2)], HeadPlan(x0=x0, levels=PLAN_LEVELS, grouped=True, dropout=False, images=2, channels=64))
        assert again["replay"] and again["kw"]["dropout_p"] == 0.0 and again["layers"][3][1]["offset"] == 15 << 34
