"""The sparse bbox tower -- apply_net's default order: csrc/k15_sparse_blocks.hip, the need bits K12 turns into zero reads,
sparse.LiveBlocks, head.forward_cls / forward_bbox -- held to something outside this repository: the reference head's recorded outputs
(tests/golden/head_*.npz, geometry A) and a float64 restatement of that head (tests/sparse_reference/head_f64.py, pinned to those
fixtures by test_head_f64_cpu.py; geometry A and a geometry B of partial edge blocks, canvas gutters inside blocks and dead blocks).
tests/test_sparse_tower_gpu.py compares the sparse order with the dense HIP tower only: an error the two share cannot show there.

Candidates always come from the production HotPath.select + sparse.LiveBlocks on class tensors the test builds; the masks of the MC
variants reach HIP and referee alike through head.dropout_replay (the fixture's recorded ones on A, seeded numpy ones on B).  Every
figure these tests measure is printed before it is asserted; the tables stand in profiles/sparse_reference.md."""
import functools

import numpy as np
import pytest
import torch

from oracle import model_fixture as mf
from pod_compare_amd import anchors as anchor_mod
from pod_compare_amd import hotpath, modeling, sparse, wino
from pod_compare_amd.synthetic import anchor_major_from_nchw, nchw_from_anchor_major
from tests.head_fixture import HeadFixture
from tests.sparse_reference import head_f64 as hf

pytestmark = pytest.mark.gpu
TOL = 1e-4                                   # the project's bar: tests/test_head_reference_gpu.py
A, K = hf.NUM_ANCHORS, hf.NUM_CLASSES
VARIANTS = ("reg_cls_var", "reg_cls_var_dropout", "reg_cls_var_dropout_full", "plain")
# geometry B: 33 rows = two blocks and one row, 47 columns = three blocks less one; six bbox copies of a level on one canvas put the
# gutters inside blocks; a sparse candidate set leaves whole blocks dead
LEVELS_B = ((33, 47), (17, 24), (9, 12), (5, 6), (3, 3))
SEED_B, RUNS_B = 7301, 3
DRAW_ID = 3
HOT, COLD = 4.0, -20.0                       # class logits of the chosen cells / everywhere else (sigmoid: 0.98 / 2e-9, threshold 0.05)


@pytest.fixture(autouse=True)
def split_kernel():
    """Sparse launches need K12."""
    old = wino.SPLIT_BF16
    wino.SPLIT_BF16 = True
    yield
    wino.SPLIT_BF16 = old


class Geometry:
    """Levels, features, masks, anchors of one (geometry, variant), and the float64 referee's outputs on them -- computed once, shared by
    every test, never written to."""

    def __init__(self, geom, variant):
        self.geom, self.variant, self.v = geom, variant, mf.VARIANTS[variant]
        self.p = self.v["dropout_rate"]
        self.mc = self.p > 0.0
        if geom == "A":
            self.fx = fx = HeadFixture(variant)
            self.levels, self.seed, self.C, self.n = fx.levels, fx.meta["seed"], fx.meta["channels"], fx.runs if self.mc else 1
            self.feats, self.masks = fx.features(), fx.masks
            self.anchors = [fx.t("anchors_l%d" % l) for l in range(len(self.levels))]
        else:
            self.fx = None
            self.levels, self.seed, self.C, self.n = [tuple(s) for s in LEVELS_B], SEED_B, mf.CHANNELS, RUNS_B if self.mc else 1
            self.feats = mf.seeded_features(self.seed, self.C, self.levels)
            self.masks = hf.SeededMasks(self.seed, self.p) if self.mc else None
            self.anchors = anchor_mod.grid_anchors(self.levels)
        self.image = (self.levels[0][0] * 8, self.levels[0][1] * 8)
        self.D = self.v["cov_dims"] if self.v["bbox_cov"] else 0
        replay = hf.replay_of(self.masks, self.levels, self.C, self.n) if self.mc else None
        ref = hf.head_f64(hf.seeded_parameters(self.v, self.seed, self.C), self.feats, self.v, replay, self.n, torch.float64, sides=(1,))
        self.ref = {"box_delta": ref["box_delta"], "box_reg_var": ref["box_reg_var"]}          # per level (n, H*W*A, C) float64

    def fixture_values(self, field, l):
        return self.fx.t("%s_%s_l%d" % ("mc" if self.mc else "eval", field, l)).double()

    def head(self, skip):
        """A fresh head (its sparse buffers zero, no abs-max record of an earlier case) with the seeded parameters; -> head, m."""
        v = self.v
        head = modeling.ProbabilisticRetinaNetHead(self.C, A, K, 4, 0.01, v["dropout_rate"], v["cls_var"], v["bbox_cov"], v["cov_dims"])
        mf.load_seeded_state(head, self.seed, rename=lambda k: mf.build_to_reference_key(k, self.mc))
        for q in head.parameters():
            q.requires_grad_(False)
        head = head.cuda().eval()
        m = self.n - 1 if (skip and self.mc) else self.n
        if self.mc:
            head.dropout_replay = hf.replay_of(self.masks, self.levels, self.C, self.n, m)
        return head, m


@functools.lru_cache(maxsize=None)
def geometry(geom, variant):
    return Geometry(geom, variant)


def chosen_cells(levels, cset):
    """Candidate set -> [(level, y, x)]."""
    h0, w0 = levels[0]
    if cset == "a":
        return [(0, 0, 0)]
    if cset == "b":
        return [(0, h0 - 1, w0 - 1)]
    if cset == "c":
        return [(l, h // 2, w // 2) for l, (h, w) in enumerate(levels)]
    if cset == "d":
        l = len(levels) - 1
        return [(l, y, x) for y in range(levels[l][0]) for x in range(levels[l][1])]
    if cset == "e":                          # 9 columns apart: at reach 1 the boxes (4 columns either side) touch without overlapping
        return [(0, 0, w0 // 2 - 5), (0, 0, w0 // 2 + 4)]
    raise ValueError(cset)


def class_tensors(g, cells):
    cls = [torch.full((g.n, A * K, h, w), COLD) for h, w in g.levels]
    for l, y, x in cells:
        cls[l][:, 0::K, y, x] = HOT                                  # class 0 of every anchor of the cell (plane a * K + k)
    cls_var = [torch.full((g.n, A * K, h, w), -10.0).cuda() for h, w in g.levels] if g.v["cls_var"] else None
    return [t.cuda() for t in cls], cls_var


def recorded_class_tensors(g):
    """Set f: the reference's recorded class outputs and a score threshold, computed here on the host, that some 20 anchors pass."""
    fx = g.fx
    pre = "mc" if g.mc else "eval"
    rec = lambda f, l: nchw_from_anchor_major(fx.t("%s_%s_l%d" % (pre, f, l)), g.levels[l][0], g.levels[l][1], A)
    cls = [rec("box_cls", l) for l in range(len(g.levels))]
    cls_var = [rec("box_cls_var", l).cuda() for l in range(len(g.levels))] if g.v["cls_var"] else None
    scores = []
    for l, t in enumerate(cls):
        runs = t.double()
        mean = (runs[0] + runs[:-1].sum(0)) / g.n if g.n > 1 else runs[0]        # PI:216-222: run 0 twice, the last run never
        scores.append(anchor_major_from_nchw(mean[None], K)[0].sigmoid().max(1).values)
    s = torch.cat(scores).sort(descending=True).values
    thresh = float(0.5 * (s[19] + s[20]))
    return [t.cuda() for t in cls], cls_var, thresh


def host_reach(levels, cells):
    """reach per level (k15_sparse_blocks.hip): the smallest j <= 5 with the cell inside candidates (+) box(2 j rows, 4 j columns), else 255."""
    out = []
    for l, (h, w) in enumerate(levels):
        r = np.full((h, w), 255, dtype=np.int64)
        ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
        for cl, cy, cx in cells:
            if cl == l:
                j = np.maximum((np.abs(ys - cy) + 1) // 2, (np.abs(xs - cx) + 3) // 4)
                r = np.minimum(r, np.where(j <= 5, j, 255))
        out.append(r)
    return out


class Case:
    """One evaluation of the production order on a candidate set: forward_cls, HotPath.select, LiveBlocks, forward_bbox sparse -- and the
    dense K12 bbox side from the same plan."""

    def __init__(self, g, cset, skip, head=None):
        self.g = g
        self.head, self.m = (head, g.n - 1 if (skip and g.mc) else g.n) if head is not None else g.head(skip)
        thresh = hotpath.PathParams().score_thresh
        if cset == "f":
            self.cls, self.cls_var, thresh = recorded_class_tensors(g)
            cells = None
        else:
            cells = chosen_cells(g.levels, cset)
            self.cls, self.cls_var = class_tensors(g, cells)
        self.hp = hp = hotpath.HotPath(g.levels, g.anchors, hotpath.PathParams(score_thresh=thresh), n_runs=g.n, has_cls_var=g.v["cls_var"],
                                       cov_dims=g.D, device="cuda:0")
        feats = [f.cuda() for f in g.feats]
        with torch.no_grad():
            self.st = self.head.forward_cls(feats, g.n, mc_dropout=g.mc, skip_unused_last_run=skip)
            hp.select(self.cls, self.cls_var, draw_id=DRAW_ID)
            self.live = sparse.LiveBlocks(hp)
            self.n_cand = int(hp.n_total.item())
            keys, lv = hp.cat_keys[:self.n_cand].cpu().tolist(), hp.cat_level[:self.n_cand].cpu().tolist()
            got = sorted({(l, (0xFFFFFFFF - (int(k) & 0xFFFFFFFF)) // A) for k, l in zip(keys, lv)})
            self.cells = [(l,) + divmod(c, g.levels[l][1]) for l, c in got]
            if cells is not None:                                     # the production selection took the chosen cells, every anchor of them
                assert self.cells == sorted(cells) and self.n_cand == A * len(cells), (self.cells, self.n_cand)
            self.reach = host_reach(g.levels, self.cells)
            assert np.array_equal(self.live.reach.cpu().numpy().astype(np.int64), np.concatenate([r.reshape(-1) for r in self.reach]))

    def bbox(self, live):
        with torch.no_grad():
            delta, reg_var = self.head.forward_bbox(self.st, live)
        return [t.clone() for t in delta], (None if reg_var is None else [t.clone() for t in reg_var])

    def rows(self, l):
        """Rows of level l's (N, H*W*A, C) tensors that belong to the candidate cells: all anchors of them."""
        w = self.g.levels[l][1]
        cells = [y * w + x for cl, y, x in self.cells if cl == l]
        return torch.tensor([c * A + a for c in cells for a in range(A)], dtype=torch.int64)

    def live_records(self, reach):
        """Live records per level of the bbox trunk's table for a launch whose output has reach `reach`."""
        table = wino.block_table(self.g.levels, self.st.box_copies if self.g.mc else 1, "cuda")
        rec = self.live.records(table, reach).cpu().tolist()
        lv = table.pod_rec_level.cpu().tolist()
        return [sum(1 for r in rec if lv[r] == l) for l in range(len(self.g.levels))], len(lv)


def stats(got, want, scale):
    d = (got - want).abs()
    return float(d.max()) / scale, float(d.pow(2).mean().sqrt()) / scale


def measure(case, sp, dn, label):
    """Errors of the sparse and the dense K12 tower against the float64 referee (and, on geometry A, the reference's recorded values) at all
    anchors of the candidate cells, per field and level, in units of the level tensor's scale max(1, max |.|); printed, then returned."""
    g = case.g
    out = []
    for field, per, tensors in (("box_delta", 4, (sp[0], dn[0])), ("box_reg_var", g.D, (sp[1], dn[1]))):
        if tensors[0] is None:
            continue
        valid = g.n if field == "box_delta" else case.m             # the runs the merge reads (PI:216-222)
        for l in range(len(g.levels)):
            rows = case.rows(l)
            if rows.numel() == 0:
                continue
            ref = g.ref[field][l][:valid]
            scale = max(1.0, float(ref.abs().max()))
            s, d = (anchor_major_from_nchw(t[l].cpu().double(), per)[:valid][:, rows] for t in tensors)
            r = ref[:, rows]
            rec = {"field": field, "level": l, "scale": scale, "sparse": stats(s, r, scale), "dense": stats(d, r, scale),
                   "sparse_dense": stats(s, d, scale), "ulp": float(np.spacing(np.float32(scale))) / scale}
            if g.fx is not None:
                fxv = g.fixture_values(field, l)[:valid]
                fscale = max(1.0, float(fxv.abs().max()))
                rec["fixture"] = stats(fxv[:, rows], r, scale)
                rec["sparse_fixture"] = stats(s, fxv[:, rows], fscale)
            print("sparse_reference: %s %s l%d scale %.3g | sparse max %.3e rms %.3e | dense max %.3e rms %.3e | ratio max %.2f rms %.2f | "
                  "sparse-dense max %.3e%s" % (label, field, l, scale, *rec["sparse"], *rec["dense"], rec["sparse"][0] / max(rec["dense"][0], 1e-30),
                                             rec["sparse"][1] / max(rec["dense"][1], 1e-30), rec["sparse_dense"][0],
                                             "" if g.fx is None else " | reference max %.3e rms %.3e | sparse-fixture max %.3e" % (*rec["fixture"], rec["sparse_fixture"][0])))
            out.append(rec)
    return out


def cases():
    for geom, sets in (("A", "abcdef"), ("B", "abcde")):
        for variant in VARIANTS:
            for skip in ((False, True) if mf.VARIANTS[variant]["dropout_rate"] > 0 else (False,)):
                for cset in sets:
                    yield pytest.param(geom, variant, cset, skip, id="%s-%s-%s-%s" % (geom, variant, cset, "skip" if skip else "all"))


@pytest.mark.parametrize("geom,variant,cset,skip", list(cases()))
def test_sparse_tower_equals_the_f64_referee_and_the_reference_at_the_candidates(geom, variant, cset, skip):
    """Bounds (measured figures: profiles/sparse_reference.md):
    - sparse against float64, and on geometry A against the reference's recorded values: 1e-4 of the level tensor's scale, the bar of
      tests/test_head_reference_gpu.py;
    - sparse against dense against the SAME float64 values: a sparse launch's abs-max record covers a subset of the dense launch's cells and
      zeros elsewhere, so its operand scale is never coarser: max and rms error at most 2 x the dense tower's + 4 ulps of the scale (the
      rule of tests/fp64_referee)."""
    g = geometry(geom, variant)
    case = Case(g, cset, skip)
    r0 = case.reach[0]
    if cset == "d":                                               # candidates on the coarsest level only: levels 0 .. 3 run no block at all
        for reach in (0, 4):
            per_level, _ = case.live_records(reach)
            assert per_level[:-1] == [0] * (len(g.levels) - 1) and per_level[-1] > 0, per_level
    elif geom == "A" and cset in "cf":
        # a 12 x 20 map has no cell further than reach 3 from its centre (nor from some 20 scattered candidates): what these cases can
        # still meet are the zero reads of the launches whose input has reach <= 1 and <= 2
        assert int(r0.max()) >= 2, int(r0.max())
    else:                                                         # ... otherwise the case tests nothing
        assert (r0 == 255).any()
    if cset == "f":
        print("sparse_reference: %s-%s set f: %d candidates on %d cells at score_thresh %.4f" % (geom, variant, case.n_cand, len(case.cells), case.hp.p.score_thresh))
        assert 5 <= case.n_cand <= 50, case.n_cand
    if geom == "B" and cset != "d":
        per_level, n_rec = case.live_records(0)
        assert 0 < sum(per_level) < n_rec                          # whole blocks are dead
    sp, dn = case.bbox(case.live), case.bbox(None)
    recs = measure(case, sp, dn, "%s-%s-%s-%s" % (geom, variant, cset, "skip" if skip else "all"))
    assert {r["level"] for r in recs} == {l for l, _, _ in case.cells}
    for r in recs:
        what = (r["field"], r["level"])
        assert r["sparse"][0] <= TOL, what
        if g.fx is not None:
            assert r["sparse_fixture"][0] <= TOL, what
        assert r["sparse"][0] <= 2.0 * r["dense"][0] + 4.0 * r["ulp"], what
        assert r["sparse"][1] <= 2.0 * r["dense"][1] + 4.0 * r["ulp"], what
    if skip:                                                      # a skipped slab is zero, never stale memory
        for t in sp[1]:
            assert float(t[case.m:].abs().max()) == 0.0


@pytest.mark.parametrize("variant", ["reg_cls_var", "reg_cls_var_dropout"])
def test_sparse_tower_runs_to_the_detections_of_the_f64_referee(variant):
    """Geometry B, a candidate at every level's centre, to the detections: everything the sparse tower did not compute for the candidates is
    NaN before hp.finish reads it -- the detections are finite, and they are those of hp.run_image on the referee's dense outputs rounded
    to float32: same keep list and classes, boxes and covariances within 1e-4 of scale (tests/test_sparse_tower_gpu.py's bound)."""
    g = geometry("B", variant)
    case = Case(g, "c", True)
    hp = case.hp
    delta, reg_var = case.bbox(case.live)
    for l, (h, w) in enumerate(g.levels):
        dead = torch.ones(h, w, dtype=torch.bool)
        for cl, y, x in case.cells:
            if cl == l:
                dead[y, x] = False
        delta[l][:, :, dead.cuda()] = float("nan")
        reg_var[l][:, :, dead.cuda()] = float("nan")
    got = hp.finish("bayes_od", case.cls, delta, case.cls_var, reg_var, g.image, g.image)
    k, n = got.count(), int(hp.n_total.item())
    keep = hp.keep[:int(hp.n_keep.item())].clone()
    got = {f: getattr(got, f)[:k].clone() for f in ("boxes", "cov", "scores", "classes")}
    as_planes = lambda field, per: [nchw_from_anchor_major(t.float(), h, w, A).cuda() for t, (h, w) in zip(g.ref[field], g.levels)]
    want = hp.run_image("bayes_od", case.cls, as_planes("box_delta", 4), case.cls_var, as_planes("box_reg_var", g.D), g.image, g.image, draw_id=DRAW_ID)
    assert n == int(hp.n_total.item()) == A * len(g.levels) and k == want.count() and k > 0
    assert torch.equal(keep, hp.keep[:int(hp.n_keep.item())]) and torch.equal(got["classes"], want.classes[:k])
    for f in ("boxes", "cov", "scores"):
        assert bool(torch.isfinite(got[f]).all()), f
    for f in ("boxes", "cov"):
        w_ = getattr(want, f)[:k]
        err, scale = float((got[f] - w_).abs().max()), max(1.0, float(w_.abs().max()))
        print("sparse_reference: detections B-%s-c %s: %d kept of %d candidates, error %.3e of scale %.3g" % (variant, f, k, n, err / scale, scale))
        assert err <= 1e-4 * scale, f


def test_a_reach_one_layer_short_is_seen(monkeypatch):
    """Sensitivity: with every subnet layer launched one reach short (not below 0) the predictors read cells the last trunk layer never
    computed -- zeros of a fresh head's buffers -- and the error at the candidate's cell must exceed the bar the tests above hold.
    On set b of geometry B: the candidate (32, 46) stands in the first row of block row 2, so the cells of row 31 the predictors read
    lie in blocks that are live for reach 1 and dead for reach 0.  (Set a cannot show it, measured 1.4e-7 = the dense error, bit for bit:
    a live block is computed whole, and everything the cell (0, 0) depends on -- one cell per layer, against the reach box's 2 rows and
    4 columns per layer -- lies in its own block.)"""
    g = geometry("B", "reg_cls_var")
    true_reach = sparse.reach_of_subnet_layer
    monkeypatch.setattr(sparse, "reach_of_subnet_layer", lambda layer, num_convs=4: max(0, true_reach(layer, num_convs) - 1))
    case = Case(g, "b", False)
    assert case.cells == [(0, 32, 46)] and case.live_records(0)[0][0] < case.live_records(1)[0][0]
    sp = case.bbox(case.live)
    monkeypatch.setattr(sparse, "reach_of_subnet_layer", true_reach)
    recs = measure(case, sp, case.bbox(None), "B-reg_cls_var-b-short")
    assert recs and all(r["dense"][0] <= TOL for r in recs)
    for r in recs:
        assert r["sparse"][0] > TOL, (r["field"], r["level"])
