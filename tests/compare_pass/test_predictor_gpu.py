"""build_comparison: several inference configs on shared model evaluations and shared fronts.  Config k's Instances for image i must be
bit-equal to build_predictor(cfg_k)'s over the same image sequence -- the separate predictors here start from the model state a process
of their own starts from (dropout call counter and graph serial at zero) -- while the model is evaluated once per family.

The module shares its name with tests/rng/test_predictor_gpu.py so that the GPU run order in tests/conftest.py (GPU_ORDER, keyed by module
name) gives it a place."""
import os

import pytest
import torch

from pod_compare_amd import config, hotpath, modeling
from pod_compare_amd.probabilistic_inference import build_comparison, build_predictor

pytestmark = pytest.mark.gpu

CONFIGS = os.path.join(os.path.dirname(os.path.abspath(config.__file__)), "configs")
MODEL = os.path.join(CONFIGS, "BDD-Detection", "retinanet", "retinanet_R_50_FPN_1x_reg_cls_var_dropout.yaml")
SIX = ("standard_nms", "anchor_statistics", "bayes_od", "bayes_od_mc_dropout", "mc_dropout_ensembles_pre_nms", "mc_dropout_ensembles_post_nms")
FIELDS = ("pred_classes", "scores", "pred_cls_probs", "pred_boxes_covariance")


def cfg_of(name, *opts):
    cfg = config.setup_config(MODEL, os.path.join(CONFIGS, "Inference", name + ".yaml"),
                              opts=["PROBABILISTIC_INFERENCE.MC_DROPOUT.NUM_RUNS", "3"] + list(opts))
    cfg.MODEL.DEVICE = "cuda"
    return cfg


def build_model(seed):
    """A random-init model whose class bias lets every level of a 64 x 96 frame keep candidates."""
    torch.manual_seed(seed)
    m = modeling.ProbabilisticRetinaNet(dropout_rate=0.1, cls_var_loss="loss_attenuation", cls_var_num_samples=10,
                                        bbox_cov_loss="negative_log_likelihood").cuda().eval()
    modeling.fold_frozen_bn(m)
    for q in m.parameters():
        q.requires_grad_(False)
    with torch.no_grad():
        m.head.cls_score.weight.mul_(40.0)
        m.head.cls_score.bias.fill_(-2.5)
    return m


@pytest.fixture(scope="module")
def models():
    return [build_model(s) for s in (0, 1000)]


@pytest.fixture(scope="module")
def images():
    g = torch.Generator(device="cuda").manual_seed(4)
    return [[{"image": torch.randint(0, 256, (3, 64, 96), dtype=torch.uint8, device="cuda", generator=g), "height": 128, "width": 192,
              "image_id": 20 + i}] for i in range(3)]


def fresh(*ms):
    """The state a model has when its process starts: what keys the dropout masks besides the seed."""
    for m in ms:
        m.head._drop_calls, m._graph_serial = 0, 0


def separately(cfgs, images, model, sparse, model_list=None):
    out = []
    for cfg in cfgs:
        fresh(model, *(model_list or []))
        p = build_predictor(cfg, model=model, model_list=model_list)
        p.sparse_bbox_tower = sparse
        out.append([p(im) for im in images])
    return out


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(got, want, what=""):
    """Bit for bit: fp32 fields are compared as the words they are (a NaN a degenerate cluster leaves equals itself)."""
    assert len(got) == len(want) and len(want) > 0, what
    assert torch.equal(bits(got.pred_boxes.tensor), bits(want.pred_boxes.tensor)), what
    for name in FIELDS:
        assert torch.equal(bits(getattr(got, name)), bits(getattr(want, name))), (name, what)


class Spy:
    """Counts a model's forwards (a forward hook) and the calls of the two front forms."""

    def __init__(self, monkeypatch, *ms):
        self.forwards, self.dense_fronts, self.sparse_fronts = [0] * len(ms), 0, 0
        self.handles = [m.register_forward_hook(lambda *a, k=k: self.forwards.__setitem__(k, self.forwards[k] + 1)) for k, m in enumerate(ms)]
        run_modes, finish_modes = hotpath.HotPath.run_modes, hotpath.HotPath.finish_modes

        def dense(hp, *a, **kw):
            self.dense_fronts += 1
            return run_modes(hp, *a, **kw)

        def sparse(hp, *a, **kw):
            self.sparse_fronts += 1
            return finish_modes(hp, *a, **kw)

        monkeypatch.setattr(hotpath.HotPath, "run_modes", dense)
        monkeypatch.setattr(hotpath.HotPath, "finish_modes", sparse)

    def close(self):
        for h in self.handles:
            h.remove()


@pytest.mark.parametrize("sparse", [True, False])
def test_six_configs_of_a_dropout_model(models, images, monkeypatch, sparse):
    """The reference's six YAMLs for one dropout model, NUM_RUNS = 3, over three images: every config's Instances are its own predictor's,
    bit for bit -- with the sparse bbox tower (each family here has ONE candidate list, so it stays sparse: the sparse rule) and without.

    Model evaluations per image: THREE, not six -- the single run, the 3 runs that skip the last run's unread outputs (BayesOD and the
    pre-NMS merge; their own runs skip too), and all 3 runs (the post-NMS merge).  One evaluation for both MC families -- two per image --
    cannot keep this test's first assertion: a dropout mask is keyed by the element's index in the head's trunk buffers, and those hold
    2m + (n + m) images per level with m = n - 1 when the last run is skipped, 2n + 2n when it is not.  Measured on this model and frame
    size, the skipping evaluation and the full one differ in cls, cls_var, delta and reg_var of the runs they share at every one of the
    five levels, while two skipping evaluations agree bit for bit (pod_compare_amd/comparison.py).  Fronts per image: three."""
    m = models[0]
    cfgs = [cfg_of(n) for n in SIX]
    want = separately(cfgs, images, m, sparse)
    fresh(m)
    cmp = build_comparison(cfgs, model=m)
    cmp.sparse_bbox_tower = sparse
    spy = Spy(monkeypatch, m)
    got = [cmp(im) for im in images]
    spy.close()
    for k in range(len(cfgs)):
        for i in range(len(images)):
            same(got[i][k], want[k][i], (k, i))
    assert spy.forwards == [3 * len(images)] and cmp.evaluations == 3 * len(images)
    assert cmp.fronts == 3 * len(images)
    assert (spy.sparse_fronts, spy.dense_fronts) == ((2 * len(images), 0) if sparse else (0, 2 * len(images)))
    # the configs are not six copies of one answer: the dropout runs at least cannot give the single run's (two modes may agree on 9 detections)
    prints = {tuple((len(w[i]),) + tuple(bits(getattr(w[i], n)).cpu().numpy().tobytes() for n in FIELDS) + (w[i].pred_boxes.tensor.cpu().numpy().tobytes(),)
                    for i in range(len(images))) for w in want}
    assert len(prints) >= 2


def test_five_configs_share_two_evaluations(models, images, monkeypatch):
    """Without the post-NMS merge: two model evaluations and two fronts per image, not five."""
    m = models[0]
    cfgs = [cfg_of(n) for n in SIX[:5]]
    fresh(m)
    cmp = build_comparison(cfgs, model=m)
    cmp.sparse_bbox_tower = True
    spy = Spy(monkeypatch, m)
    got = [cmp(im) for im in images]
    spy.close()
    assert spy.forwards == [2 * len(images)] and cmp.fronts == 2 * len(images) and all(len(g) == 5 for g in got)


def test_draws_follow_the_position_when_images_carry_no_id(models, images):
    """Without an integer image_id the draw id is the workspace's own count of images: each sub-family counts as its predictor does."""
    m = models[0]
    cfgs = [cfg_of(n) for n in ("anchor_statistics", "bayes_od")]
    anon = [[{k: v for k, v in im[0].items() if k != "image_id"}] for im in images]
    want = separately(cfgs, anon, m, False)
    cmp = build_comparison(cfgs, model=m)
    cmp.sparse_bbox_tower = False
    got = [cmp(im) for im in anon]
    for k in range(2):
        for i in range(len(anon)):
            same(got[i][k], want[k][i], (k, i))


def test_ensembles_pre_and_post_nms_share_the_members_forwards(models, images, monkeypatch):
    """Two members, both merges: every member is evaluated once per image, not twice.  The two merges do not share a candidate list, so the
    family's bbox side is dense even with the sparse tower switched on (the dense rule): the outputs are those of the separate DENSE runs."""
    seeds = ["PROBABILISTIC_INFERENCE.ENSEMBLES.RANDOM_SEED_NUMS", "[0, 1000]"]
    cfgs = [cfg_of("ensembles_pre_nms", *seeds), cfg_of("ensembles_post_nms", *seeds)]
    want = separately(cfgs, images, models[0], False, model_list=models)
    cmp = build_comparison(cfgs, model=models[0], model_list=models)
    cmp.sparse_bbox_tower = True
    spy = Spy(monkeypatch, *models)
    got = [cmp(im) for im in images]
    spy.close()
    for k in range(2):
        for i in range(len(images)):
            same(got[i][k], want[k][i], (k, i))
    assert spy.forwards == [len(images)] * 2 and cmp.evaluations == len(images) and cmp.fronts == 2 * len(images)
    assert spy.sparse_fronts == 0 and spy.dense_fronts == len(images)


def test_one_sparse_ensemble_config_stays_sparse(models, images, monkeypatch):
    seeds = ["PROBABILISTIC_INFERENCE.ENSEMBLES.RANDOM_SEED_NUMS", "[0, 1000]"]
    cfgs = [cfg_of("ensembles_pre_nms", *seeds)]
    want = separately(cfgs, images[:1], models[0], True, model_list=models)
    cmp = build_comparison(cfgs, model=models[0], model_list=models)
    cmp.sparse_bbox_tower = True
    spy = Spy(monkeypatch, *models)
    got = cmp(images[0])
    spy.close()
    same(got[0], want[0][0])
    assert (spy.sparse_fronts, spy.dense_fronts) == (1, 0)


def test_two_affinity_thresholds_make_two_fronts_and_a_dense_bbox_side(models, images, monkeypatch):
    """The dense rule on one model: anchor statistics at 0.9 and BayesOD at 0.8 share the single-run evaluation, not the PodConfig their
    tails read, so they are two sub-families -- two fronts on one DENSE evaluation, each config equal to its own dense run."""
    m = models[0]
    cfgs = [cfg_of("anchor_statistics"), cfg_of("bayes_od", "PROBABILISTIC_INFERENCE.AFFINITY_THRESHOLD", "0.8")]
    want = separately(cfgs, images, m, False)
    cmp = build_comparison(cfgs, model=m)
    cmp.sparse_bbox_tower = True
    spy = Spy(monkeypatch, m)
    got = [cmp(im) for im in images]
    spy.close()
    for k in range(2):
        for i in range(len(images)):
            same(got[i][k], want[k][i], (k, i))
    assert spy.forwards == [len(images)] and (spy.sparse_fronts, spy.dense_fronts) == (0, 2 * len(images))


def test_replayed_graphs_keep_every_family_on_its_own_masks(models):
    """apply_net's default: forwards replayed as HIP graphs, captured once a (stream, frame shape, call) has come back twice.  Eight frames
    of two shapes taking turns on one stream, so every key is run eagerly twice, captured, and replayed; the six configs' Instances must
    still be their own predictors' bit for bit -- a family's masks come from ITS call counter and ITS graph serial (item 2 of the identity
    contract), and the model's graph cache holds a family's graphs as long as the config's own run holds them.  The cache is set to the
    two graphs one call needs for two shapes: the comparison scales it by its three calls; unscaled, the six keys would evict each other,
    every re-capture would take a new serial, and the MC configs would draw other masks than their own runs."""
    m = models[0]
    cfgs = [cfg_of(n) for n in SIX]
    g = torch.Generator(device="cuda").manual_seed(9)
    frames = [[{"image": torch.randint(0, 256, (3,) + hw, dtype=torch.uint8, device="cuda", generator=g), "height": hw[0], "width": hw[1],
                "image_id": 40 + i}] for i, hw in enumerate([(64, 96), (96, 64)] * 4)]

    def start():
        m._drop_graphs()
        m._graph_seen.clear()
        fresh(m)
        m.max_graphs = 2

    try:
        m.enable_graphs(True)
        m.graph_after_seen = 2
        want = []
        for cfg in cfgs:
            start()
            p = build_predictor(cfg, model=m)
            p.sparse_bbox_tower = True
            want.append([p(im) for im in frames])
            assert len(m._graphs) == 2 and m._graph_serial == 2          # both shapes captured once, nothing evicted
        start()
        cmp = build_comparison(cfgs, model=m)
        cmp.sparse_bbox_tower = True
        assert m.max_graphs == 6
        got = [cmp(im) for im in frames]
        for k in range(len(cfgs)):
            for i in range(len(frames)):
                same(got[i][k], want[k][i], (k, i))
        assert len(m._graphs) == 6 and [st[1] for st in cmp._mask_state.values()] == [2, 2, 2]
    finally:
        m.enable_graphs(False)
        m._graph_seen.clear()
        m.max_graphs = 16
