"""CPU side of K21: the fp64 referee of the GPU tests (tests/training/loss_ref.py) against the fixture the reference itself produced,
the fixture's regeneration, the declarations of the new entry points and the annealing arithmetic.  No GPU."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import refimport
from pod_compare_amd import hip, losses
from tests.helpers import assert_close, is_predictor_fixture
from tests.training import loss_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.fixture(scope="module")
def fx():
    return lr.load_fixture()


def test_fixture_is_not_a_predictor_fixture(fx):
    assert not is_predictor_fixture(lr.FIXTURE)
    assert fx["meta"]["kind"] == "train_loss" and sorted(fx["meta"]["cases"]) == ["plain", "var_annealed", "var_mid", "var_step0"]
    assert os.path.getsize(lr.FIXTURE) < 1 << 20


def test_restated_labels_equal_the_fixture(fx):
    """The geometry the issue describes: 60 positives by threshold, 78 ignored, two boxes reached only through low-quality promotion
    (21 anchors), 19 foreground anchors whose arg-max ties on the duplicated box -- and the labels of both images."""
    anchors = torch.from_numpy(fx["anchors"])
    gb, gc = torch.from_numpy(fx["gt_boxes"]), torch.from_numpy(fx["gt_classes"])
    a = lr.label_anchors(anchors, gb, gc, 7)
    b = lr.label_anchors(anchors, gb[:0], gc[:0], 7)
    assert np.array_equal(a["labels"].numpy(), fx["labels"][0]) and np.array_equal(b["labels"].numpy(), fx["labels"][1])
    assert int((a["by_threshold"] == 1).sum()) == 60 and int((a["labels"] == -1).sum()) == 78 and int(a["promoted"].sum()) == 21
    assert a["num_pos"] == 81 and b["num_pos"] == 0 and bool((b["labels"] == 7).all())
    u = a["unique"]
    assert np.array_equal(a["matched"][u].numpy(), fx["matched_gt"][0][u.numpy()])
    fg = (a["labels"] >= 0) & (a["labels"] < 7)
    assert int(((a["by_threshold"] == 1) & ~u).sum()) == 19 and int((fg & ~u).sum()) == 27      # (8 more tie among the promoted ones)
    assert bool((a["matched"][fg & ~u] == 0).all())                                             # ties: the lowest box index
    q = lr.iou_matrix(gb, anchors)
    reached = sorted(float(q[g].max()) for g in range(5) if float(q[g].max()) < 0.4)
    assert len(reached) == 2 and abs(reached[0] - 0.094) < 1e-3 and abs(reached[1] - 0.188) < 1e-3


def _case_inputs(fx, var):
    d = lambda k: torch.from_numpy(fx[k]).double()
    labels = torch.from_numpy(fx["labels"]).long()
    gb = torch.from_numpy(fx["gt_boxes"])
    mb = torch.zeros(labels.shape + (4,))
    mb[0] = gb[torch.from_numpy(fx["matched_gt"][0]).long()]
    eps = lr.scatter_eps(fx["eps"], labels >= 0) if var else None
    return d("cls"), d("delta"), d("cls_var") if var else None, d("reg_var") if var else None, labels, mb, torch.from_numpy(fx["anchors"]), eps


@pytest.mark.parametrize("case", ["plain", "var_step0", "var_mid", "var_annealed"])
def test_restated_losses_reproduce_the_reference(fx, case):
    m, c = fx["meta"], fx["meta"]["cases"][case]
    var = c["variance_heads"]
    cls, delta, cls_var, reg_var, labels, mb, anchors, eps = _case_inputs(fx, var)
    cs, ss, ns, npos = lr.loss_sums(cls, delta, cls_var, reg_var, labels, mb, anchors, 7, eps)
    norm = 0.9 * m["initial_loss_normalizer"] + 0.1 * max(npos, 1)
    assert abs(norm - c["loss_normalizer"]) < 1e-9
    lam = lr.annealing_lambda(c["current_step"], m["annealing_step"]) if var else 0.0
    loss_cls = cs / ((m["cls_var_num_samples"] if var else 1) * max(1.0, norm))
    loss_reg = ((1 - lam) * ss + lam * ns) / max(1.0, norm)
    print(case, float(loss_cls), float(fx["loss_cls_" + case]), float(loss_reg), float(fx["loss_box_reg_" + case]))
    assert_close(loss_cls, torch.tensor(float(fx["loss_cls_" + case])), "loss_cls")
    assert_close(loss_reg, torch.tensor(float(fx["loss_box_reg_" + case])), "loss_box_reg")


@pytest.mark.skipif(not refimport.reference_available(), reason="reference tree not present")
def test_fixture_regenerates_bit_identically(fx):
    spec = importlib.util.spec_from_file_location("make_golden_loss", os.path.join(ROOT, "tools", "make_golden_loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    again = mod.build()
    with np.load(lr.FIXTURE, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(again)
        for k in z.files:
            a, b = z[k], np.asarray(again[k])
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_annealing_weight_at_the_three_steps():
    """--iteration -> lambda (PR:320-321): 0 at step 0, (10 - 1) / 99 half way, 1 from the annealing step on."""
    anneal = 80000
    assert losses.annealing_weight(0, anneal) == 0.0
    assert abs(losses.annealing_weight(anneal // 2, anneal) - 9.0 / 99.0) < 1e-15
    assert losses.annealing_weight(anneal, anneal) == 1.0 and losses.annealing_weight(3 * anneal, anneal) == 1.0
    crit = losses.ProbabilisticLosses(annealing_step=anneal)
    for step, lam in ((0, 0.0), (anneal // 2, 1.0 / 11.0), (anneal, 1.0)):
        crit.current_step = step
        w = crit.weights(torch.tensor(4.0), has_cls_var=True, has_reg_var=True).double()
        assert_close(w, torch.tensor([1.0 / (3 * 4.0), (1 - lam) / 4.0, lam / 4.0], dtype=torch.float64), "weights", rtol=1e-6, atol=1e-7)
    assert_close(crit.weights(torch.tensor(0.25), False, False).double(), torch.tensor([1.0, 1.0, 0.0], dtype=torch.float64), "weights", rtol=1e-6, atol=1e-7)


def test_header_binding_and_library_carry_the_loss_entry_points():
    """Additions only: the three symbols are declared, bound and exported, and the ABI number the header, the binding and the library
    state is one number (it stays where K20 left it: nothing that existed changed)."""
    from pod_compare_amd import build
    from tests.test_abi_cpu import HEADER, declared_symbols
    for name in ("pod_label_anchors", "pod_train_loss", "pod_train_loss_partials"):
        assert name in hip.EXPORTS and name in declared_symbols()
    assert "#define POD_ABI_VERSION %d\n" % hip.POD_ABI_VERSION in open(HEADER).read()
    lib = ctypes.CDLL(build.build_library())
    assert lib.pod_abi_version() == hip.POD_ABI_VERSION and all(hasattr(lib, n) for n in ("pod_label_anchors", "pod_train_loss", "pod_train_loss_partials"))
    assert ctypes.sizeof(hip.PodLevelGrad) == 4 * ctypes.sizeof(ctypes.c_void_p)


def test_loss_entry_points_reject_invalid_arguments_without_a_gpu():
    """Validation happens on the host before any launch.  cov_dims = 10: the reference defines no loss for the full covariance."""
    lib = hip.load()
    buf = ctypes.create_string_buffer(64)
    X = ctypes.addressof(buf)
    lv = (hip.PodLevel * hip.POD_MAX_LEVELS)()
    lv[0].H, lv[0].W, lv[0].anchor_base = 2, 3, 0
    for n in ("cls", "cls_var", "delta", "reg_var"):
        setattr(lv[0], n, X)

    def cfg_with(**kw):
        c = hip.PodConfig()
        c.n_levels, c.n_runs, c.num_anchors, c.num_classes, c.cov_dims, c.has_cls_var, c.cls_samples = 1, 1, 9, 7, 4, 1, 3
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def loss(c, R=54, labels=X, partials=X, grads=None, w=None, levels=lv):
        return lib.pod_train_loss(c, levels, grads, labels, X, X, 1, X, R, 0.25, 2.0, 0.0, None, None, w, partials, X, None)

    assert lib.pod_train_loss_partials(cfg_with(), lv) == 4 and lib.pod_train_loss_partials(cfg_with(n_runs=3), lv) == 12
    assert loss(cfg_with(cov_dims=10)) == -1
    for kw in ({"n_levels": 0}, {"n_levels": hip.POD_MAX_LEVELS + 1}, {"n_runs": 0}, {"num_classes": 16}, {"cls_samples": 0},
               {"cls_samples": hip.POD_MAX_CLS_SAMPLES + 1}):
        assert loss(cfg_with(**kw)) == -1, kw
    assert loss(cfg_with(), R=55) == -1 and loss(cfg_with(), labels=None) == -1 and loss(cfg_with(), partials=None) == -1
    assert loss(cfg_with(), grads=(hip.PodLevelGrad * hip.POD_MAX_LEVELS)(), w=None) == -1          # gradient planes need their weights
    assert loss(None) == -1 and loss(cfg_with(), levels=None) == -1
    # pod_label_anchors
    lab = lambda R=54, n=1, g=1, K=7, lo=0.4, hi=0.5, anchors=X, off=X, scratch=X: lib.pod_label_anchors(
        anchors, R, X, X, off, n, g, K, lo, hi, X, X, X, scratch, None)
    assert lab(R=0) == -1 and lab(n=0) == -1 and lab(g=-1) == -1 and lab(K=0) == -1 and lab(lo=0.6) == -1
    assert lab(anchors=None) == -1 and lab(off=None) == -1 and lab(scratch=None) == -1
