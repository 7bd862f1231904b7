"""Structural checks of the PyTorch model (the reference model cannot be imported without detectron2, so the
build's model is validated against the reference's constructor constants and layer shapes, PR:370-484, and against
naive restatements of its own forward)."""
import math

import pytest
import torch
import torch.nn.functional as F

from pod_compare_amd import modeling


def make(**kw):
    torch.manual_seed(0)
    return modeling.ProbabilisticRetinaNet(**kw).eval()


def test_head_layers_and_initialisation_constants():
    m = make(dropout_rate=0.2, cls_var_loss="loss_attenuation", cls_var_num_samples=10, bbox_cov_loss="negative_log_likelihood")
    h = m.head
    assert len(h.cls_subnet) == 4 and len(h.bbox_subnet) == 4                       # NUM_CONVS
    for conv in list(h.cls_subnet) + list(h.bbox_subnet):
        assert conv.weight.shape == (256, 256, 3, 3) and float(conv.bias.abs().max()) == 0.0
        assert abs(float(conv.weight.std()) - 0.01) < 5e-4                           # PR:447-450
    assert h.cls_score.weight.shape == (9 * 7, 256, 3, 3) and h.bbox_pred.weight.shape == (9 * 4, 256, 3, 3)
    assert torch.allclose(h.cls_score.bias, torch.full((63,), -math.log(99.0)))      # PR:454-455, prior 0.01
    assert h.cls_var.weight.shape == (63, 256, 3, 3) and torch.allclose(h.cls_var.bias, torch.full((63,), -10.0))   # PR:458-470
    assert h.bbox_cov.weight.shape == (36, 256, 3, 3) and abs(float(h.bbox_cov.weight.std()) - 1e-4) < 1e-5        # PR:473-484
    full = make(bbox_cov_loss="negative_log_likelihood", bbox_cov_type="full")
    assert full.head.bbox_cov.weight.shape[0] == 9 * 10                               # PR:37-44
    plain = make()
    assert plain.head.cls_var is None and plain.head.bbox_cov is None and not plain.use_dropout


def test_output_shapes_and_anchor_grid_agree():
    m = make(cls_var_loss="loss_attenuation", bbox_cov_loss="negative_log_likelihood")
    ho = m(torch.randint(0, 256, (3, 100, 150), dtype=torch.uint8))
    assert ho.image_size == (100, 150) and ho.shapes == [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)]
    for l, (h, w) in enumerate(ho.shapes):
        assert ho.cls[l].shape == (1, 63, h, w) and ho.delta[l].shape == (1, 36, h, w)
        assert ho.cls_var[l].shape == (1, 63, h, w) and ho.reg_var[l].shape == (1, 36, h, w)
        assert ho.anchors[l].shape == (h * w * 9, 4) and ho.cls[l].is_contiguous()


def test_eval_mode_trunk_sharing_equals_two_evaluations():
    """Without dropout the reference evaluates each subnet twice on the same input (PR:518-523); sharing the trunk is exact."""
    m = make(cls_var_loss="loss_attenuation", bbox_cov_loss="negative_log_likelihood")
    h = m.head
    f = torch.randn(1, 256, 12, 16)

    def subnet(convs, x):
        for c in convs:
            x = F.relu(c(x))
        return x

    with torch.no_grad():
        cls, delta, cls_var, reg_var = h([f], 1, mc_dropout=False)
        assert torch.equal(cls[0], h.cls_score(subnet(h.cls_subnet, f)))
        assert torch.equal(cls_var[0], h.cls_var(subnet(h.cls_subnet, f)))
        assert torch.equal(delta[0], h.bbox_pred(subnet(h.bbox_subnet, f)))
        assert torch.equal(reg_var[0], h.bbox_cov(subnet(h.bbox_subnet, f)))


def test_mc_runs_are_batched_with_independent_masks_and_shared_first_conv():
    m = make(dropout_rate=0.2, cls_var_loss="loss_attenuation", bbox_cov_loss="negative_log_likelihood")
    h = m.head
    f = torch.randn(1, 256, 12, 16)
    with torch.no_grad():
        torch.manual_seed(1)
        cls, delta, cls_var, reg_var = h([f], 6, mc_dropout=True)
        assert cls[0].shape == (6, 63, 12, 16) and reg_var[0].shape == (6, 36, 12, 16)
        assert not torch.equal(cls[0][0], cls[0][1]) and not torch.equal(delta[0][2], delta[0][3])     # different masks per run
        # dropout is unbiased: the mean over many runs approaches the dropout-free output of a LINEAR probe; here just sanity:
        # with p = 0 the MC path degenerates to the eval path
        h.dropout_rate = 0.0
        c0, d0, _, _ = h([f], 3, mc_dropout=True)
        e0, g0, _, _ = h([f], 1, mc_dropout=False)
        assert torch.allclose(c0[0][1], e0[0][0], atol=1e-6) and torch.allclose(d0[0][2], g0[0][0], atol=1e-6)


def test_skip_unused_last_run_keeps_everything_the_merge_reads():
    """The quirky merge never reads run N-1 of cls / cls_var / reg_var; deltas of every run are still produced."""
    m = make(dropout_rate=0.2, cls_var_loss="loss_attenuation", bbox_cov_loss="negative_log_likelihood")
    img = torch.randint(0, 256, (3, 64, 96), dtype=torch.uint8)
    torch.manual_seed(5)
    a = m(img, num_mc_dropout_runs=4, skip_unused_last_run=True)
    assert a.cls[0].shape[0] == 4 and a.delta[0].shape[0] == 4 and a.reg_var[0].shape[0] == 4
    assert bool(torch.isfinite(a.delta[0]).all()) and bool(torch.isfinite(a.cls[0][:3]).all())


def test_preprocess_pads_to_fpn_divisibility_and_normalises():
    m = make()
    x = m.preprocess_image(torch.full((3, 50, 70), 128, dtype=torch.uint8))
    assert x.shape == (1, 3, 64, 96)
    assert torch.allclose(x[0, :, 0, 0], torch.tensor([128 - 103.530, 128 - 116.280, 128 - 123.675]))
    assert float(x[0, :, 60, 90].abs().max()) == 0.0                                   # zero padding
    r = modeling.resize_test_image(torch.zeros(3, 720, 1280))
    assert r.shape == (3, 750, 1333)


@pytest.mark.parametrize("mc_dropout, want", [(True, dict(n=10, m=9, skip=1, cls_copies=18, box_copies=19)),
                                              (False, dict(n=10, m=10, skip=0))])      # skipping the last run needs dropout
def test_head_plan_run_arithmetic(mc_dropout, want):
    """`_plan` of 10 runs with skip_unused_last_run: m = n - skip runs need cls / cls_var / reg_var; the cls trunk evaluates m for the mean
    and m for the variance, the bbox trunk n for the mean and m for the covariance.  CPU features never take the Winograd path."""
    torch.manual_seed(0)
    head = modeling.ProbabilisticRetinaNetHead(compute_cls_var=True, compute_bbox_cov=True, dropout_rate=0.1)
    st = head._plan([torch.zeros(1, 256, 4, 6), torch.zeros(1, 256, 2, 3)], 10, mc_dropout, True)
    assert isinstance(st, modeling.HeadPlan) and st.wino is False
    assert {k: getattr(st, k) for k in want} == want


def test_head_plan_rejects_a_misspelt_field():
    with pytest.raises(TypeError):
        modeling.HeadPlan(levls=[(4, 6)])
