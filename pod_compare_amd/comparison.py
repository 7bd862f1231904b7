"""Several inference configs of one model on one pass over the data (DESIGN.md "Comparison pass").

    cmp = probabilistic_inference.build_comparison([cfg_standard_nms, cfg_anchor_statistics, cfg_bayes_od, ...])
    per_config = cmp(input_im)          # one Instances (or DeviceDetections) per config, in config order

The configs differ in their PROBABILISTIC_INFERENCE section only.  They are grouped, in config order, into

  * FAMILIES: the configs whose model evaluation is the same call.  One model: the same (MC_DROPOUT.ENABLE, effective NUM_RUNS,
    skip_unused_last_run).  `ensembles`: the same member list.  A family's evaluation runs once per image.
  * SUB-FAMILIES inside a family: the configs that share the front of the post-processing chain -- merge + score, top-k, gather + decode,
    NMS on the same merged candidate list, with the same PathParams as far as their chain reads them.  A sub-family's front runs once per
    image (pod_run_image_modes, or select / finish_modes around the sparse bbox tower); every config adds its tail.  A post-NMS merge
    (mc_dropout_ensembles / ensembles with BOX_MERGE_MODE post_nms) has a front per member: it is a sub-family of its own kind.

The identity contract: config k's detections for image i are bit-equal to `build_predictor(cfg_k)`'s on image i, called in a process of its
own over the same image sequence.  What makes that hold:

  * the in-kernel draws are keyed by (SEED, draw id); the draw id is the image's id, or the position in the sequence -- each sub-family
    counts its own images as its predictor would;
  * the dropout masks are keyed by the head's call counter and the serial number of the HIP graph that replays the forward.  Each family
    carries its OWN pair of counters, swapped into the model around its evaluation, so that a family's masks do not depend on which other
    families ride along;
  * skip_unused_last_run is part of the evaluation call: it changes how many images the head's trunk buffers hold, and a mask is keyed by
    the element's index in its buffer.  An evaluation of all runs therefore draws other masks than one that skips the last run's unread
    outputs -- a post-NMS MC-dropout config (which needs every run) and a pre-NMS one (whose own run skips) cannot both be served by one
    evaluation and both keep their own run's bits.  They are two families.
  * the sparse bbox tower's live blocks and abs-max records follow from the candidate list.  A family with ONE sub-family has one list: it
    runs sparse exactly as its configs' own runs do.  A family with several sub-families evaluates its bbox side densely; its configs are
    then bit-equal to their own runs with the dense bbox side (apply_net --dense-bbox).
"""
from collections import namedtuple
from typing import List, Sequence

from . import hip, hotpath, modeling

Family = namedtuple("Family", "key members subfamilies")          # key: see family_key; members: config indices, in order
SubFamily = namedtuple("SubFamily", "kind affinity members")      # kind: "merged" | "post_nms"; affinity: None = no member reads it

_AFFINITY_MODES = ("anchor_statistics", "bayes_od")               # the tails that read AFFINITY_THRESHOLD (K5 / K6); K7 alone does not


def _pi(cfg):
    return cfg["PROBABILISTIC_INFERENCE"]


def is_post_nms(cfg) -> bool:
    pi = _pi(cfg)
    mode = pi["INFERENCE_MODE"]
    return ((mode == "mc_dropout_ensembles" and pi["ENSEMBLES_DROPOUT"]["BOX_MERGE_MODE"] != "pre_nms") or
            (mode == "ensembles" and pi["ENSEMBLES"]["BOX_MERGE_MODE"] != "pre_nms"))


def family_key(cfg) -> tuple:
    """The model evaluation of a config as a value: ("ensembles", seeds) or ("model", MC dropout on, runs, last run's unread outputs
    skipped) -- what RetinaNetProbabilisticPredictor._head_outputs / post_processing_ensembles call the model(s) with."""
    pi = _pi(cfg)
    if pi["INFERENCE_MODE"] == "ensembles":
        return ("ensembles", tuple(int(s) for s in pi["ENSEMBLES"]["RANDOM_SEED_NUMS"]))
    enable = bool(pi["MC_DROPOUT"]["ENABLE"])
    runs = int(pi["MC_DROPOUT"]["NUM_RUNS"]) if enable and int(pi["MC_DROPOUT"]["NUM_RUNS"]) > 1 else 1
    return ("model", enable, runs, runs > 1 and not is_post_nms(cfg))


def group_families(cfgs: Sequence) -> List[Family]:
    """Pure function of the configs' PROBABILISTIC_INFERENCE sections: families in order of their first config, sub-families likewise."""
    fams = {}
    for i, cfg in enumerate(cfgs):
        fams.setdefault(family_key(cfg), []).append(i)
    out = []
    for key, members in fams.items():
        subs = []                                                  # [kind, affinity, members]
        for i in members:
            pi = _pi(cfgs[i])
            kind = "post_nms" if is_post_nms(cfgs[i]) else "merged"
            reads = kind == "post_nms" or pi["INFERENCE_MODE"] in _AFFINITY_MODES
            aff = float(pi["AFFINITY_THRESHOLD"]) if reads else None
            for s in subs:
                if s[0] == kind and (aff is None or s[1] is None or s[1] == aff):
                    s[2].append(i)
                    if s[1] is None:
                        s[1] = aff
                    break
            else:
                subs.append([kind, aff, [i]])
        out.append(Family(key, tuple(members), tuple(SubFamily(k, a, tuple(m)) for k, a, m in subs)))
    return out


def _flat(node, prefix=""):
    for k, v in node.items():
        if isinstance(v, dict):
            yield from _flat(v, prefix + k + ".")
        else:
            yield prefix + k, v


def check_same_outside_inference(cfgs: Sequence) -> None:
    """Raises ValueError naming the first key outside PROBABILISTIC_INFERENCE in which a config differs from the first one."""
    strip = lambda c: dict(_flat({k: v for k, v in c.items() if k != "PROBABILISTIC_INFERENCE"}))
    first = strip(cfgs[0])
    for n, cfg in enumerate(cfgs[1:], 1):
        other = strip(cfg)
        for key in sorted(set(first) | set(other)):
            a, b = first.get(key, "<absent>"), other.get(key, "<absent>")
            if (list(a) if isinstance(a, (list, tuple)) else a) != (list(b) if isinstance(b, (list, tuple)) else b):
                raise ValueError("configs of a comparison may differ in PROBABILISTIC_INFERENCE only: config {} has {} = {!r}, config 0 has {!r}"
                                 .format(n, key, b, a))


class Comparison:
    """N predictors on shared models; see the module docstring.  Attributes: `families`, `predictors` (one per config), `return_device`,
    `sparse_bbox_tower` (as the predictor's), and per call counters for tests and tools: `evaluations` (model evaluations: one per family
    and image, however many members an ensemble has), `fronts` (sub-family fronts)."""

    def __init__(self, cfgs, model=None, model_list=None):
        from .probabilistic_inference import RetinaNetProbabilisticPredictor, build_model
        cfgs = list(cfgs)
        if not cfgs:
            raise ValueError("a comparison needs at least one config")
        for cfg in cfgs:
            if cfg.MODEL.META_ARCHITECTURE != "ProbabilisticRetinaNet":
                raise ValueError("Invalid meta-architecture {}.".format(cfg.MODEL.META_ARCHITECTURE))
            if _pi(cfg)["INFERENCE_MODE"] not in hotpath.MODES:
                raise ValueError("Invalid inference mode {}.".format(_pi(cfg)["INFERENCE_MODE"]))
        check_same_outside_inference(cfgs)
        self.families = group_families(cfgs)
        ens = [f for f in self.families if f.key[0] == "ensembles"]
        if len(ens) > 1:
            raise ValueError("configs of a comparison share their models: one ENSEMBLES.RANDOM_SEED_NUMS list, got {}".format([f.key[1] for f in ens]))
        single = any(f.key[0] == "model" for f in self.families)
        if model is None:       # PI:58-84: a pure ensemble comparison keeps the model as built, like the predictor
            model = build_model(cfgs[0], load_weights=single)
        self.predictors = []
        for cfg in cfgs:
            p = RetinaNetProbabilisticPredictor(cfg, model=model, model_list=model_list)
            if _pi(cfg)["INFERENCE_MODE"] == "ensembles" and model_list is None:
                model_list = p.model_list                          # built once (PI:59-77), shared by the other ensemble config
            self.predictors.append(p)
        self.model, self.model_list = model, list(model_list or [])
        self.return_device = False
        self.sparse_bbox_tower = self.predictors[0].sparse_bbox_tower
        own = isinstance(model, modeling.ProbabilisticRetinaNet)
        start = (model.head._drop_calls, model._graph_serial) if own else None
        self._mask_state = {f.key: start for f in self.families}
        self.evaluations = self.fronts = 0
        if own:
            # The model keeps `max_graphs` captured forwards, sized for ONE evaluation call per (stream, frame shape); here every family
            # of the model is a call of its own (its graph key holds runs, dropout, skip and part), so the cache holds that many times as
            # many: a family's graphs are then evicted -- and re-captured under a new serial, i.e. with other masks -- when its config's
            # own run would evict them, not sooner.  (An ensemble's members each see one call: theirs stand.)
            calls = sum(1 for f in self.families if f.key[0] == "model")
            before = getattr(model, "_max_graphs_per_call", None)
            per_call = before[0] if before is not None and before[1] == model.max_graphs else model.max_graphs
            model.max_graphs = per_call * max(1, calls)
            model._max_graphs_per_call = (per_call, model.max_graphs)

    # -- plumbing ------------------------------------------------------------------------------------
    def _sync_flags(self):
        for p in self.predictors:
            p.return_device, p.sparse_bbox_tower = True, self.sparse_bbox_tower

    class _Masks:
        """The family's dropout call counter and graph serial in place of the model's while the family's evaluation is enqueued."""

        def __init__(self, cmp, fam):
            self.cmp, self.fam = cmp, fam

        def __enter__(self):
            st, m = self.cmp._mask_state[self.fam.key], self.cmp.model
            if st is not None:
                self.saved = (m.head._drop_calls, m._graph_serial)
                m.head._drop_calls, m._graph_serial = st

        def __exit__(self, *exc):
            m = self.cmp.model
            if self.cmp._mask_state[self.fam.key] is not None:
                self.cmp._mask_state[self.fam.key] = (m.head._drop_calls, m._graph_serial)
                m.head._drop_calls, m._graph_serial = self.saved
            return False

    def _tails(self, sub: SubFamily):
        out = []
        for i in sub.members:
            pi = _pi(self.predictors[i].cfg)
            out.append((pi["INFERENCE_MODE"], pi["BAYES_OD"]["BOX_MERGE_MODE"], pi["BAYES_OD"]["CLS_MERGE_MODE"]))
        return out

    def _chunks(self, sub: SubFamily):
        """(tails, members) per front: at most POD_MAX_MODE_TAILS tails ride on one."""
        tails, n = self._tails(sub), hip.POD_MAX_MODE_TAILS
        return [(tails[a:a + n], sub.members[a:a + n]) for a in range(0, len(tails), n)]

    def _leader(self, sub: SubFamily):
        """The predictor whose workspace serves the sub-family: the first member configured with the affinity threshold its tails read
        (a standard-NMS config reads none and may carry another: the workspace's PodConfig must not be built from it)."""
        for i in sub.members:
            if sub.affinity is None or float(_pi(self.predictors[i].cfg)["AFFINITY_THRESHOLD"]) == sub.affinity:
                return self.predictors[i]
        raise AssertionError("a sub-family's affinity threshold is one of its members'")

    @staticmethod
    def _draw(leader, hp, input_im) -> int:
        """The draw id the sub-family's own predictor would use: the image's id, else the workspace's count of images."""
        did = leader._draw_id(input_im)
        if did is None:
            did = hp._draws
            hp._draws += 1
        return did

    def _merged(self, sub: SubFamily, input_im, ho, results):
        """One dense front, the sub-family's tails (RetinaNetProbabilisticPredictor._run for several configs)."""
        leader = self._leader(sub)
        hp = leader.last_path = leader._path_for(ho)
        if not ho.last_run_valid and not leader.merge_quirk:
            raise hip.PodError("the last MC run's cls / cls_var / reg_var were not computed (skip_unused_last_run)")
        image_size, out = leader._sizes(input_im, ho)
        did = self._draw(leader, hp, input_im)
        for tails, members in self._chunks(sub):
            dets = hp.run_modes(tails, ho.cls, ho.delta, ho.cls_var, ho.reg_var, image_size=image_size, out_size=out, draw_id=did)
            self.fronts += 1
            for i, det in zip(members, dets):
                results[i] = det

    def _merged_sparse(self, sub: SubFamily, input_im, select, bbox, results):
        """select(hook) runs the cls side(s) and calls hook(partial HeadOutputs, cov_dims) -> LiveBlocks; bbox(live) -> full HeadOutputs."""
        from . import sparse
        leader = self._leader(sub)
        state = {}

        def hook(partial, cov_dims):
            hp = leader._path_for(partial, cov_dims=cov_dims)
            hp.select(partial.cls, partial.cls_var, draw_id=self._draw(leader, hp, input_im))
            state["hp"] = hp
            return sparse.LiveBlocks(hp)

        ho = bbox(select(hook))
        hp = leader.last_path = state["hp"]
        image_size, out = leader._sizes(input_im, ho)
        chunks = self._chunks(sub)
        if len(chunks) > 1:
            raise hip.PodError("more than {} configs on one sparse front".format(hip.POD_MAX_MODE_TAILS))
        dets = hp.finish_modes(chunks[0][0], ho.cls, ho.delta, ho.cls_var, ho.reg_var, image_size, out)
        self.fronts += 1
        for i, det in zip(sub.members, dets):
            results[i] = det

    # -- families ------------------------------------------------------------------------------------
    def _model_family(self, fam: Family, input_im, results):
        from .probabilistic_inference import run_slice
        _, enable, runs, skip = fam.key
        leader = self.predictors[fam.members[0]]
        m, image = self.model, input_im[0]["image"]
        sub0 = fam.subfamilies[0]
        self.evaluations += 1
        if len(fam.subfamilies) == 1 and sub0.kind == "merged" and len(sub0.members) <= hip.POD_MAX_MODE_TAILS and leader._sparse_ok():
            cov_dims = m.bbox_cov_dims if m.compute_bbox_cov else 0
            mc = runs > 1
            with self._Masks(self, fam):       # RetinaNetProbabilisticPredictor._run_sparse's forward, the hook serving every config
                self._merged_sparse(sub0, input_im,
                                    lambda hook: m(image, num_mc_dropout_runs=runs if mc else -1, mc_dropout=enable,
                                                   skip_unused_last_run=mc and leader.merge_quirk,
                                                   sparse_bbox=lambda partial: hook(partial, cov_dims)),
                                    lambda ho: ho, results)
            return
        with self._Masks(self, fam):
            ho = leader._head_outputs(input_im, need_all_runs=not skip)
        for sub in fam.subfamilies:
            if sub.kind == "merged":
                self._merged(sub, input_im, ho, results)
            else:
                for i in sub.members:                               # PI:445-451: N runs, merged post-NMS
                    results[i] = self.predictors[i]._run_post_nms(input_im, [run_slice(ho, r) for r in range(ho.num_runs)])
                    self.fronts += 1

    def _ensemble_family(self, fam: Family, input_im, results):
        from .probabilistic_inference import input_is_cuda, stack_members
        leader = self.predictors[fam.members[0]]
        models, image = leader.model_list, input_im[0]["image"]
        sub0 = fam.subfamilies[0]
        self.evaluations += 1
        sparse_ok = (leader.sparse_bbox_tower and leader.eps_fn is None and
                     all(isinstance(m, modeling.ProbabilisticRetinaNet) and m.head.takes_wino_path() and input_is_cuda(m) for m in models))
        if len(fam.subfamilies) == 1 and sub0.kind == "merged" and len(sub0.members) <= hip.POD_MAX_MODE_TAILS and sparse_ok:
            first = models[0]
            cov_dims = first.bbox_cov_dims if first.compute_bbox_cov else 0
            sts = [m.cls_part(image) for m in models]              # RetinaNetProbabilisticPredictor._run_sparse_ensemble
            self._merged_sparse(sub0, input_im,
                                lambda hook: hook(stack_members([m.partial_outputs(st) for m, st in zip(models, sts)]), cov_dims),
                                lambda live: stack_members([m.bbox_part(st, live) for m, st in zip(models, sts)]), results)
            return
        members = [m(image) for m in models]
        for sub in fam.subfamilies:
            if sub.kind == "merged":
                self._merged(sub, input_im, stack_members(members), results)      # PI:495-505
            else:
                for i in sub.members:
                    results[i] = self.predictors[i]._run_post_nms(input_im, members)   # PI:506-534
                    self.fronts += 1

    def __call__(self, input_im):
        from .probabilistic_inference import detections_to_instances
        self._sync_flags()
        results = [None] * len(self.predictors)
        for fam in self.families:
            (self._ensemble_family if fam.key[0] == "ensembles" else self._model_family)(fam, input_im, results)
        for p, det in zip(self.predictors, results):
            p.last_detections = det
        return results if self.return_device else [detections_to_instances(d) for d in results]
