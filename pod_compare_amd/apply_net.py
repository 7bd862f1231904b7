"""Inference driver: the reference's apply_net.py loop (AN:82-102), image-sharded over the GPUs of one node.

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m pod_compare_amd.apply_net \
        --config-file <model.yaml> --inference-config <inference.yaml> --num-images 64 --output results.json

The reference pins inference to one process (AN:113-114).  Here rank r handles images r, r+world, ...
(independent units, batch 1 as AN:35, a few of them in flight on separate HIP streams); each rank keeps its detections
as fixed-stride records in HBM (K7) and ONE collective per flush (every --flush-every images per rank) gathers counts +
records to every rank (`all_gather`; backend "nccl" =
RCCL over xGMI on GPUs, "gloo" in the CPU tests of this sharding/re-ordering logic).  Rank 0 restores the
image order and writes `coco_instances_results.json` (AN:100-102 format).
"""
import argparse
import json
import os
import time
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from .inference_utils import record_width, records_to_json

# core/datasets/metadata.py as DATA: the thing classes of the data sets the reference registers (setup_datasets.py:36-117); dataset ids are
# 1 .. len(classes) in this order (metadata.py:9-15), contiguous ids 0 .. len - 1.  Lyft re-uses BDD's map (setup_datasets.py:117).
THING_CLASSES = {"bdd": ["car", "bus", "truck", "person", "rider", "bike", "motor"], "kitti": ["car", "person"]}
THING_CLASSES["lyft"] = THING_CLASSES["bdd"]


def _family(dataset: str) -> str:
    for fam in THING_CLASSES:
        if dataset.startswith(fam + "_") or dataset == fam:
            return fam
    raise ValueError("Unknown data set {!r}: known families are {} (e.g. bdd_val, kitti_val).".format(dataset, sorted(THING_CLASSES)))


def category_mapping(train_dataset: str, test_dataset: str) -> Dict[int, int]:
    """AN:52-80: model (contiguous, TRAIN data set) class id -> category_id of the TEST data set's annotations.
    Same classes (BDD -> BDD, BDD -> Lyft): the test set's contiguous -> dataset id map flipped (AN:60-63).  BDD -> KITTI: only the classes
    KITTI annotates survive, through metadata.BDD_TO_KITTI_CONTIGUOUS_ID (AN:70-73, 78-79); a detection of any other class gets -1 and is
    dropped by instances_to_json (IU:466-471).  Any other pair: the reference BUILDS a ValueError without raising it (AN:76-77)
    and then fails on an undefined name; here it is raised.  (COCO / VOC: their 80- / 20-class tables are not carried -- out of BASELINE's
    scope -- and are reported as such.)"""
    train, test = _family(train_dataset), _family(test_dataset)
    test_ids = {i: i + 1 for i in range(len(THING_CLASSES[test]))}               # contiguous -> dataset id of the test set
    if THING_CLASSES[train] == THING_CLASSES[test]:
        return test_ids
    if train == "bdd" and test == "kitti":
        to_kitti = {THING_CLASSES["bdd"].index(c): THING_CLASSES["kitti"].index(c) for c in THING_CLASSES["kitti"]}    # BDD_TO_KITTI_CONTIGUOUS_ID
        return {bdd: test_ids[kitti] for bdd, kitti in to_kitti.items()}
    raise ValueError("Cannot generate category mapping dictionary. Please check if training and inference datasets are compatible.")


BDD_CAT_MAP = category_mapping("bdd_train", "bdd_val")   # contiguous id -> dataset id (ids 1..7)


def evaluation_category_map(train_dataset: str, test_dataset: str) -> Dict[int, int]:
    """EU:370-397 (get_thing_dataset_id_to_contiguous_id_dict): TEST data set's category id -> the model's (TRAIN data set's) contiguous id,
    the map the evaluators convert ground-truth categories with.  Same classes (BDD -> BDD, BDD -> Lyft, KITTI -> KITTI): the test set's
    own dataset id -> contiguous map.  BDD -> KITTI: each KITTI id to the BDD class of the same name ({1: 0, 2: 3}).  Any other pair raises
    (the reference builds the ValueError without raising it; the COCO -> VOC branch is not carried, as in `category_mapping`)."""
    train, test = _family(train_dataset), _family(test_dataset)
    if THING_CLASSES[train] == THING_CLASSES[test]:
        return {i + 1: i for i in range(len(THING_CLASSES[test]))}
    if train == "bdd" and test == "kitti":
        return {k + 1: THING_CLASSES["bdd"].index(c) for k, c in enumerate(THING_CLASSES["kitti"])}
    raise ValueError("Cannot generate category mapping dictionary. Please check if training and inference datasets are compatible.")


def add_dataset_arguments(ap: argparse.ArgumentParser) -> None:
    """--train-dataset / --test-dataset of the offline evaluators: which category map the ground truth and the results are read with."""
    ap.add_argument("--train-dataset", default="bdd_train", help="the model's training data set (cfg.DATASETS.TRAIN[0]): its classes are the model's")
    ap.add_argument("--test-dataset", default="bdd_val", help="the data set of the results and the ground truth (EU:370-397: e.g. kitti_val "
                                                              "maps KITTI's car / person to the BDD model's classes 0 / 3)")


def shard_indices(num_images: int, rank: int, world: int) -> List[int]:
    """Images of rank `rank`: i = rank (mod world)."""
    return list(range(rank, num_images, world))


def gather_records(local_ids: Sequence[int], local_counts: torch.Tensor, local_records: torch.Tensor, num_images: int,
                   world: int, per_rank: Optional[int] = None) -> Tuple[List[int], torch.Tensor, torch.Tensor]:
    """One flush: every rank contributes (n_local, max_det, width) records + (n_local,) counts, padded to the
    common per-rank maximum (`per_rank`, default ceil(num_images / world)) so a single all_gather moves them.
    Returns (image ids, counts, records) in image order."""
    if per_rank is None:
        per_rank = -(-num_images // world)
    n_local = len(local_ids)
    dev = local_records.device
    ids = torch.full((per_rank,), -1, dtype=torch.int64, device=dev)
    ids[:n_local] = torch.as_tensor(list(local_ids), dtype=torch.int64, device=dev)
    cnt = torch.zeros((per_rank,), dtype=torch.int32, device=dev)
    cnt[:n_local] = local_counts.to(torch.int32)
    rec = torch.zeros((per_rank,) + tuple(local_records.shape[1:]), dtype=local_records.dtype, device=dev)
    rec[:n_local] = local_records
    if world > 1:
        if dist.get_backend() != "nccl":      # functional runs on gloo: collectives on host copies (RCCL gathers device buffers)
            ids, cnt, rec = ids.cpu(), cnt.cpu(), rec.cpu()
        all_ids = [torch.empty_like(ids) for _ in range(world)]
        all_cnt = [torch.empty_like(cnt) for _ in range(world)]
        all_rec = [torch.empty_like(rec) for _ in range(world)]
        dist.all_gather(all_ids, ids)
        dist.all_gather(all_cnt, cnt)
        dist.all_gather(all_rec, rec)
        ids, cnt, rec = torch.cat(all_ids), torch.cat(all_cnt), torch.cat(all_rec)
    valid = ids >= 0
    ids, cnt, rec = ids[valid], cnt[valid], rec[valid]
    order = torch.argsort(ids)
    return ids[order].tolist(), cnt[order], rec[order]


def results_json(ids: Sequence[int], counts: torch.Tensor, records: torch.Tensor, num_classes: int,
                 cat_map: Optional[Dict[int, int]] = None) -> List[dict]:
    out = []
    counts = counts.cpu().tolist()
    records = records.cpu()
    for i, image_id in enumerate(ids):
        out.extend(records_to_json(records[i], counts[i], image_id, num_classes, cat_map))
    return out


class CocoImages:
    """The reference's `build_detection_test_loader(cfg, dataset_name)` (AN:83-84) for a COCO-format image list, restated
    without detectron2: what detectron2's DatasetMapper(is_train=False) hands the predictor for every entry of `images` --
    the file read with PIL as RGB and flipped to BGR (cfg.INPUT.FORMAT), ResizeShortestEdge(MIN_SIZE_TEST, MAX_SIZE_TEST) applied
    with PIL's bilinear filter on the uint8 HWC array (detectron2's ResizeTransform does exactly that for uint8 images), then a
    (3, H, W) uint8 tensor; 'height' / 'width' are the ORIGINAL size from the json (the output resolution, PI:106-107) and
    'image_id' the dataset's id.  device_resize: the entry carries 'frame', the decoded RGB (h, w, 3) uint8 tensor, instead of 'image';
    resize, flip and transpose are then left to `resize.resize_frame_u8` on the device, which gives the same bytes."""

    def __init__(self, json_path: str, image_root: str, min_size: int = 800, max_size: int = 1333, device_resize: bool = False):
        with open(json_path, "r") as f:
            data = json.load(f)
        self.images = list(data["images"])
        self.root, self.min_size, self.max_size = image_root, int(min_size), int(max_size)
        self.device_resize = bool(device_resize)

    def __len__(self) -> int:
        return len(self.images)

    def image_id(self, i: int):
        return self.images[i]["id"]

    def __getitem__(self, i: int) -> dict:
        return self.entry(i)

    def entry(self, i: int, size=None) -> dict:
        """Entry i; size: the (nh, nw) the host path resizes to in place of ResizeShortestEdge(min_size, max_size) -- a training loader's
        drawn size (train_head --train-loader)."""
        import numpy as np
        from PIL import Image
        from . import anchors
        rec = self.images[i]
        with Image.open(os.path.join(self.root, rec["file_name"])) as im:
            im = im.convert("RGB")
            h, w = im.height, im.width
            if self.device_resize:
                return {"frame": torch.as_tensor(np.array(im)), "height": int(rec.get("height", h)), "width": int(rec.get("width", w)),
                        "image_id": rec["id"], "file_name": rec["file_name"]}
            nh, nw = anchors.resize_shortest_edge(h, w, self.min_size, self.max_size) if size is None else (int(size[0]), int(size[1]))
            if (nh, nw) != (h, w):
                im = im.resize((nw, nh), Image.BILINEAR)
            arr = np.asarray(im)[:, :, ::-1]                       # RGB -> BGR
        image = torch.as_tensor(np.ascontiguousarray(arr.transpose(2, 0, 1)))
        return {"image": image, "height": int(rec.get("height", h)), "width": int(rec.get("width", w)), "image_id": rec["id"],
                "file_name": rec["file_name"]}


class Prefetched:
    """The worker side of the reference's test loader (detectron2's build_detection_test_loader runs the mapper on
    cfg.DATALOADER.NUM_WORKERS processes): entries `dataset[i]` for `indices`, read / decoded / resized up to `depth` entries ahead on
    `workers` host threads (PIL drops the GIL while it decodes and resizes) and handed out IN ORDER; the uint8 frame is moved to pinned
    memory so that `.to(device, non_blocking=True)` is an asynchronous copy on the image's stream.  One decode thread feeds ~60 frames of
    1280x720 per second; a GPU takes 130 - 650.  workers = 0: the plain loop.  An exception of a worker surfaces at the entry it belongs to."""

    def __init__(self, dataset, indices: Sequence[int], workers: int = 4, depth: int = 0, pin: bool = True):
        self.dataset, self.indices, self.workers = dataset, list(indices), max(0, int(workers))
        self.depth = int(depth) if depth > 0 else 2 * max(1, self.workers)
        self.pin = bool(pin) and torch.cuda.is_available()

    def _load(self, i: int) -> dict:
        d = self.dataset[i]
        if self.pin:
            key = "image" if "image" in d else "frame"
            d[key] = d[key].pin_memory()
        return d

    def __len__(self) -> int:
        return len(self.indices)

    def __iter__(self):
        if self.workers == 0:
            for i in self.indices:
                yield i, self._load(i)
            return
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="pod-loader") as pool:
            pending = deque()
            it = iter(self.indices)
            try:
                for i in it:
                    pending.append((i, pool.submit(self._load, i)))
                    if len(pending) >= self.depth:
                        break
                while pending:
                    i, fut = pending.popleft()
                    entry = fut.result()
                    nxt = next(it, None)
                    if nxt is not None:
                        pending.append((nxt, pool.submit(self._load, nxt)))
                    yield i, entry
            finally:
                for _, fut in pending:
                    fut.cancel()


class EnsemblePerGpu:
    """Config 5 (`ensembles_pre_nms.yaml`) on one node: ensemble member s lives on rank s < M, every member rank runs the
    conv net on the SAME image, the dense pre-NMS head tensors meet on the image's merge rank (= the rank that owns the
    image in the sharded order) through `ensemble_dist.MemberPipeline` (two images in flight), K1..K7 run there
    (PI:495-505).  Ranks >= M only merge; they never build a model: the predictor reads the model's test-time
    attributes from `model_test_attributes(cfg)` and the level geometry comes from the anchor generator."""

    def __init__(self, cfg, rank: int, world: int, frame_hw=(720, 1280), net_hw=None, model=None):
        """frame_hw: output resolution ('height' / 'width' of input_im); net_hw: network-input size (default: the test
        transform of frame_hw, AN:83); model: this rank's member model (default: built and loaded per PI:59-77)."""
        from . import anchors, ensemble_dist, modeling
        from .probabilistic_inference import RetinaNetProbabilisticPredictor, build_model, ensemble_member_dir, model_test_attributes
        from .synthetic import HeadOutputs
        seeds = list(cfg.PROBABILISTIC_INFERENCE.ENSEMBLES.RANDOM_SEED_NUMS)
        self.M, self.rank, self.world, self.cfg = len(seeds), rank, world, cfg
        if world < self.M:
            raise SystemExit("one ensemble member per rank needs at least %d ranks, got %d" % (self.M, world))
        self.dev = torch.device(cfg.MODEL.DEVICE)
        self.model = model if rank < self.M else None
        if rank < self.M and self.model is None:
            state = torch.random.get_rng_state()
            torch.manual_seed(int(seeds[rank]))          # a member without a checkpoint is a random-init model seeded with its number
            self.model = build_model(cfg, save_dir=ensemble_member_dir(cfg, seeds[rank]))      # PI:59-77
            torch.random.set_rng_state(state)
        cfg.PROBABILISTIC_INFERENCE.ENSEMBLES.BOX_MERGE_MODE = "pre_nms"
        self.predictor = RetinaNetProbabilisticPredictor(cfg, model=self.model if self.model is not None else model_test_attributes(cfg),
                                                         model_list=[object()] * self.M)
        self.predictor.return_device = True
        self.frame_hw = tuple(frame_hw)
        self.net_hw = tuple(net_hw) if net_hw is not None else \
            anchors.resize_shortest_edge(frame_hw[0], frame_hw[1], cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)
        padded = anchors.padded_size(*self.net_hw)
        shapes = anchors.level_shapes(*padded)
        pm = cfg.MODEL.PROBABILISTIC_MODELING
        A, K = len(anchors.ANCHOR_SIZES[0]) * len(anchors.ASPECT_RATIOS), cfg.MODEL.RETINANET.NUM_CLASSES
        D = 0 if pm.BBOX_COV_LOSS.NAME == "none" else (4 if pm.BBOX_COV_LOSS.COVARIANCE_TYPE == "diagonal" else 10)
        self.layout = ensemble_dist.MemberLayout(shapes, A, K, D, pm.CLS_VAR_LOSS.NAME != "none")
        self.like = HeadOutputs(None, None, None, None, anchors.grid_anchors(shapes, device=self.dev), shapes, A, K, self.net_hw)
        self.pipe = ensemble_dist.MemberPipeline(self.layout, self.M, rank, world, self.dev)
        self._resize = lambda frame: modeling.resize_test_image(frame, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)

    def run(self, num_images: int, frame_of, on_detections=None):
        """`frame_of(i)` -> uint8 (3, H, W) frame of image i (every rank sees the same frames).  Returns this rank's
        ([image ids], [records], [counts]) -- device tensors, no host sync."""
        ids, recs, cnts = [], [], []
        h, w = self.frame_hw
        shape_only = torch.empty((3,) + tuple(self.net_hw), device="meta")     # the path only reads the network-input size (IU:39-41)

        def forward(i):
            return self.model(self._resize(frame_of(i)))

        def merge(i, stacked):
            input_im = [{"image": shape_only, "height": h, "width": w, "image_id": i}]
            det = self.predictor._run("standard_nms", input_im, self.layout.views(stacked, self.like))     # PI:502-505
            ids.append(i); recs.append(det.records); cnts.append(det.n_det)
            if on_detections is not None:
                on_detections(i, det)

        self.pipe.run(num_images, forward, merge)
        return ids, recs, cnts


def _run_ensemble_per_gpu(cfg, args, rank, world):
    from . import synthetic
    runner = EnsemblePerGpu(cfg, rank, world)
    _, recs, cnts = runner.run(args.num_images, lambda i: synthetic.synthetic_frame(i, device=runner.dev))
    return recs, cnts


def own_test_set(train_dataset: str) -> str:
    """The test split of the model's own data family (bdd_train -> bdd_val): where the AP step's threshold applies to PM and CE."""
    return _family(train_dataset) + "_val"


def has_ground_truth(coco_json: str) -> bool:
    if not coco_json:
        return False
    with open(coco_json, "r") as f:
        return "annotations" in json.load(f)


def evaluate_results(results: str, gt_json: str, train_dataset: str = "bdd_train", test_dataset: str = "bdd_val", binary: bool = False,
                     min_allowed_score: Optional[float] = None, map_results: str = "", device: str = "cuda", seed: int = 0,
                     scoring_rules: Sequence[str] = ("nll",), energy_samples: int = 1000, pdq: bool = False, p_min: float = 0.0027,
                     recalibration=None) -> dict:
    """AN:104-106: the offline chain on a result file, in this process on `device`.  1) AP on K17 (compute_average_precision, its
    default --cat-ids), mAP_res.txt written beside `results`; 2) PM; 3) CE with the calibration pass on the GPU (K18).  Prints the
    three tables the modules print.  The PM / CE threshold: `min_allowed_score`, else `map_results`' (PM:50-65 / CE:47-63), else --
    when the test set is the model's own (bdd_val for a BDD model) -- the threshold the AP step just wrote, else 0.0.  (The reference
    reads the training family's file; its AN:104 has the AP call commented out.)  torch is seeded with `seed` before CE's randperm.
    scoring_rules beside "nll" (energy, crps, brier) and energy_samples go to PM with `seed`: extra columns, nothing else changes.
    pdq: also PDQ (compute_pdq, K34) on the same detections under the same threshold, its table printed and its dict under "pdq".
    recalibration: a file `python -m pod_compare_amd.recalibrate fit` wrote (or a recalibration.Recalibration): the detections are
    transformed on the GPU (K36) after loading and before AP, and the AP step writes mAP_res_recalibrated.txt, never a raw run's file."""
    from . import compute_average_precision as cap
    from . import compute_calibration_errors as cce
    from . import compute_probabilistic_metrics as cpm
    torch.cuda.set_device(torch.device(device))
    if binary:
        from .inference_utils import binary_results_to_json
        predicted = binary_results_to_json(results, category_mapping(train_dataset, test_dataset))
    else:
        with open(results, "r") as f:
            predicted = json.load(f)
    with open(gt_json, "r") as f:
        gt = json.load(f)
    if recalibration is not None:
        from . import recalibration as rc
        recal = rc.Recalibration.load(recalibration) if isinstance(recalibration, str) else recalibration
        ids_of = category_mapping(train_dataset, test_dataset)
        unique = len(set(ids_of.values())) == len(ids_of)             # else the record's class is the arg-max of its probabilities
        predicted = rc.apply_to_results(predicted, recal, {v: k for k, v in ids_of.items()} if unique else None, device=device)
        print("recalibrated: beta %.6f, %s scales %s" % (recal.beta, "per-class" if recal.per_class else "global", recal.scales))
    ap = cap.coco_average_precision(predicted, gt, device=device)
    print(cap.format_summary(ap["stats"]))
    print("Classification Score at Optimal F-1 Score: {}".format(ap["optimal_score_threshold"]))
    map_path = os.path.join(os.path.dirname(os.path.abspath(results)), "mAP_res.txt" if recalibration is None else "mAP_res_recalibrated.txt")
    cap.write_map_results(map_path, ap["stats"], ap["optimal_score_threshold"])
    if min_allowed_score is not None or map_results:
        thr = cap.resolve_min_allowed_score(min_allowed_score, map_results)
    elif test_dataset == own_test_set(train_dataset):
        thr = cap.read_min_allowed_score(map_path)
    else:
        thr = 0.0
    cmap = evaluation_category_map(train_dataset, test_dataset)
    extra = {} if tuple(scoring_rules) == ("nll",) else {"scoring_rules": tuple(scoring_rules), "energy_samples": energy_samples, "seed": seed}
    pm = cpm.probabilistic_metrics(predicted, gt["annotations"], cat_mapping_dict=cmap, min_allowed_score=thr, device=device, **extra)
    print(cpm.format_table(pm))
    torch.manual_seed(seed)
    ce = cce.calibration_errors_of_results(predicted, gt["annotations"], cmap, thr, device=device)
    print(cce.format_table(ce))
    print("Cls Marginal Calibration Error computed by: " + ce["cls_marginal_calibration_error_source"])
    res = {"ap": ap, "pm": pm, "ce": ce, "min_allowed_score": thr, "map_results": map_path}
    if pdq:
        from . import compute_pdq
        res["pdq"] = compute_pdq.pdq_of_results(predicted, gt, cmap, thr, p_min, device)
        print(compute_pdq.format_table(res["pdq"]))
    return res


def _scoring_rule_options(args) -> dict:
    """--scoring-rules / --energy-samples and --pdq / --p-min as evaluate_results takes them; nothing when only the reference's rules are asked for."""
    opts = {} if tuple(args.scoring_rules) == ("nll",) else {"scoring_rules": tuple(args.scoring_rules), "energy_samples": args.energy_samples}
    if getattr(args, "pdq", False):
        opts.update(pdq=True, p_min=args.p_min)
    return opts


def _recalibration_option(args) -> dict:
    """One config's --recalibration FILE as evaluate_results takes it; nothing without the flag, so the call is what it was."""
    return {"recalibration": args.recalibration[0]} if getattr(args, "recalibration", None) else {}


def _check_recalibration(args) -> None:
    """--recalibration FILE [FILE ...]: one file per inference config, in order, for an evaluating run -- refused by name otherwise."""
    files = getattr(args, "recalibration", None)
    if not files:
        return
    if not (args.eval or args.eval_only):
        raise SystemExit("--recalibration transforms the detections an evaluation reads: it needs --eval or --eval-only")
    if len(files) != len(args.inference_config):
        raise SystemExit("--recalibration takes one file per --inference-config, in order: got %d file(s) for %d config(s)"
                         % (len(files), len(args.inference_config)))


def inference_output_dir(output_dir: str, test_dataset: str, inference_config: str, suffix: str = "") -> str:
    """AN:44-48: `<OUTPUT_DIR>/inference/<test data set>/<name of the inference YAML>`, the directory the reference's apply_net writes a
    config's coco_instances_results.json to and its evaluators read it from.  suffix: a corrupted run's `<NAME>_<N>`, which makes the
    data set's component `<test data set>_<NAME>_<N>` -- a corrupted data set is another data set."""
    return os.path.join(output_dir, "inference", test_dataset + ("_" + suffix if suffix else ""), os.path.split(inference_config)[-1][:-5])


def _check_corruption(args) -> None:
    """--corruption NAME --severity N (K35, corruptions.py): refused by name before a model is built or a rank is started where the run has
    no decoded frame on the device to corrupt, or draws / re-reads frames another way.  Implies --resize-on-gpu."""
    if args.corruption is None and args.severity is None:
        return
    if args.corruption is None or args.severity is None:
        raise SystemExit("--corruption and --severity are needed together")
    from . import corruptions
    try:
        corruptions.parameters(args.corruption, args.severity)
    except ValueError as e:
        raise SystemExit("--corruption / --severity: %s" % e)
    if not args.coco_json:
        raise SystemExit("--corruption corrupts decoded files: it needs --coco-json (synthetic frames are not supported)")
    for flag, given in (("--ensemble-per-gpu", args.ensemble_per_gpu), ("--vis-dir", bool(args.vis_dir)), ("--eval-only", args.eval_only)):
        if given:
            raise SystemExit("--corruption cannot be combined with %s" % flag)
    args.resize_on_gpu = True
    if int(os.environ.get("RANK", "0")) == 0:
        print("corrupted on the GPU: %s, severity %d" % (args.corruption, args.severity))


COMPARISON_COLUMNS = (      # (heading, evaluator, path into the dictionary evaluate_results returns for it, format)
    ("AP", "ap", ("stats", 0), "%.3f"), ("AP50", "ap", ("stats", 1), "%.3f"), ("AP75", "ap", ("stats", 2), "%.3f"),
    ("TP Cls NLL", "pm", ("average", "true_positives_cls_analysis", "ignorance_score_mean"), "%.4f"),
    ("TP Reg NLL", "pm", ("average", "true_positives_reg_analysis", "ignorance_score_mean"), "%.4f"),
    ("FP Cls NLL", "pm", ("average", "false_positives_cls_analysis", "ignorance_score_mean"), "%.4f"),
    ("FP Reg Entropy", "pm", ("average", "false_positives_reg_analysis", "total_entropy_mean"), "%.4f"),
    ("Cls MCE", "ce", ("cls_marginal_calibration_error",), "%.4f"), ("Reg ECE", "ce", ("reg_expected_calibration_error",), "%.4f"),
    ("Reg MaxCE", "ce", ("reg_maximum_calibration_error",), "%.4f"), ("Cls MUE", "ce", ("cls_minimum_uncertainty_error",), "%.4f"),
    ("Reg MUE", "ce", ("reg_minimum_uncertainty_error",), "%.4f"))
EXTRA_COMPARISON_COLUMNS = (      # appended, in this order, when a result carries the key: --scoring-rules brier / energy / crps, --pdq
    ("TP Cls Brier", "pm", ("average", "true_positives_cls_analysis", "brier_score_mean"), "%.4f"),
    ("FP Cls Brier", "pm", ("average", "false_positives_cls_analysis", "brier_score_mean"), "%.4f"),
    ("TP Reg Energy", "pm", ("average", "true_positives_reg_analysis", "energy_score_mean"), "%.4f"),
    ("TP Reg CRPS", "pm", ("average", "true_positives_reg_analysis", "crps_mean"), "%.4f"),
    ("PDQ", "pdq", ("PDQ",), "%.4f"))


def format_comparison_table(names: Sequence[str], results: Sequence[dict]) -> str:
    """One row per inference config, in order, from the dictionaries `evaluate_results` returned: AP / AP50 / AP75 (COCO's first three
    numbers), the four score columns of the PM table and the five of the CE table.  No number is computed here; one that an evaluator
    left undefined (no true positives, say) prints as "-".  The columns of the extra scoring rules follow when a result carries them."""
    def cell(res, which, path, fmt):
        v = res.get(which)
        if v is None:
            return "-"
        for k in path:
            v = v.get(k) if isinstance(v, dict) else v[k]
            if v is None:
                return "-"
        return fmt % float(v)

    def carries(res, which, path):
        v = res.get(which)
        for k in path:
            if not isinstance(v, dict) or k not in v:
                return False
            v = v[k]
        return True

    columns = COMPARISON_COLUMNS + tuple(c for c in EXTRA_COMPARISON_COLUMNS if any(carries(r, c[1], c[2]) for r in results))
    rows = [("Inference Config",) + tuple(c[0] for c in columns)]
    rows += [(n,) + tuple(cell(r, *c[1:]) for c in columns) for n, r in zip(names, results)]
    w = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    line = "+" + "+".join("-" * (x + 2) for x in w) + "+"
    body = ["| " + r[0].ljust(w[0]) + " | " + " | ".join(r[i].center(w[i]) for i in range(1, len(r))) + " |" for r in rows]
    return "\n".join([line, body[0], line] + body[1:] + [line])


def _start_rank(args, world: int, rank: int, local_rank: int) -> None:
    """This rank's process group, device and NUMA binding: the same for one inference config and for several."""
    if world > 1:
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(args.backend)
    torch.cuda.set_device(local_rank)
    if world > 1:                 # enqueue + loader threads of this rank on its GPU's NUMA node (hostbind.py; POD_BIND_NUMA=0: off)
        from . import hostbind
        b = hostbind.bind_rank_to_gpu_numa(local_rank)
        print("rank %d: cuda:%d pci %s numa node %s -> %s" % (rank, local_rank, b["pci"], b["numa_node"], b["cpus"] if b["bound"] else "not bound (%s)" % b.get("why_not", "off")))


def _network_input(args, cfg, d: Optional[dict], i: int, dev):
    """Image i as the predictor takes it, enqueued on the current stream: (input_im, the synthetic frame or None).  d: the loader's entry
    of a --coco-json run -- resized on the host exactly as detectron2's mapper does, or, with --resize-on-gpu, the decoded frame, which
    goes up and comes out as the host path's bytes (K20), outside any captured graph; with --corruption it is corrupted at its own size
    on the way (K35).  image_id is the position in the list: the data
    set's id is restored by _image_order."""
    from . import modeling, resize, synthetic
    if d is not None:
        if args.resize_on_gpu:
            frame = d["frame"].to(dev, non_blocking=True)
            if getattr(args, "corruption", None):       # K35, on this image's stream; the key names the image, not its place on a rank
                from . import corruptions
                frame = corruptions.corrupt_frame_u8(frame, args.corruption, args.severity, corruptions.corruption_key(args.random_seed, i))
            image = resize.resize_frame_u8(frame, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)
        else:
            image = d["image"].to(dev, non_blocking=True)
        return [{"image": image, "height": d["height"], "width": d["width"], "image_id": i}], None
    frame = synthetic.synthetic_frame(i, device=dev)
    image = modeling.resize_test_image(frame, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)
    return [{"image": image, "height": frame.shape[1], "width": frame.shape[2], "image_id": i}], frame


def _image_order(ids: List[int], all_cnt: list, all_rec: list, width: int, dataset):
    """The flushed chunks of one config as (ids, counts, records) in image order, the ids the data set's own."""
    order = sorted(range(len(ids)), key=lambda q: ids[q])
    ids = [ids[q] for q in order]
    cnt = torch.cat(all_cnt)[order] if all_cnt else torch.zeros((0,), dtype=torch.int32)
    rec = torch.cat(all_rec)[order] if all_rec else torch.zeros((0, 128, width))
    if dataset is not None:
        ids = [dataset.image_id(i) for i in ids]
    return ids, cnt, rec


def _main_comparison(args, paths: List[str]):
    """`main` for several --inference-config paths: the sharded loop with a `probabilistic_inference.build_comparison` in the predictor's
    place -- one decode, one model evaluation per family of configs, one front per sub-family -- every config's files written where its own
    run under the reference's directory layout writes them."""
    from . import modeling
    from .config import setup_config
    from .probabilistic_inference import build_comparison
    for flag, given in (("--output", args.output is not None), ("--vis-dir", bool(args.vis_dir)), ("--ensemble-per-gpu", args.ensemble_per_gpu)):
        if given:
            raise SystemExit("%s names one run's output: it cannot be combined with several --inference-config paths (every config writes "
                             "coco_instances_results.json to <OUTPUT_DIR>/inference/<test data set>/<its name>/)" % flag)
    if args.binary_output and os.path.dirname(args.binary_output):
        raise SystemExit("--binary-output with several --inference-config paths is a file NAME, written into every config's directory")
    names = [os.path.split(p)[-1][:-5] for p in paths]
    if len(set(names)) != len(names):
        raise SystemExit("--inference-config: two paths share the name %s, so they share an output directory" % sorted(n for n in names if names.count(n) > 1)[0])
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local_rank = 0 if args.share_gpu else int(os.environ.get("LOCAL_RANK", "0"))
    evaluating = args.eval or args.eval_only
    if evaluating and not has_ground_truth(args.coco_json):
        raise SystemExit("--eval / --eval-only need ground truth: --coco-json with `annotations`")
    cfgs = [setup_config(args.config_file, p, args.random_seed, data_dir=args.data_dir, is_testing=bool(args.data_dir)) for p in paths]
    suffix = "%s_%d" % (args.corruption, args.severity) if args.corruption else ""
    dirs = [inference_output_dir(cfgs[0].OUTPUT_DIR, args.test_dataset, p, suffix) for p in paths]
    outputs = [os.path.join(d, "coco_instances_results.json") for d in dirs]
    sidecars = [os.path.join(d, args.binary_output) if args.binary_output else "" for d in dirs]

    def evaluate_all(device):
        res = []
        recal = args.recalibration or [None] * len(names)
        for name, out, side, rc_file in zip(names, outputs, sidecars, recal):
            print("== %s" % name)
            binary = args.eval_only and bool(side)        # as one config's --eval-only: the sidecar when it is named
            extra = {} if rc_file is None else {"recalibration": rc_file}
            res.append(evaluate_results(side if binary else out, args.coco_json, args.train_dataset, args.test_dataset, binary=binary,
                                        min_allowed_score=args.min_allowed_score, map_results=args.map_results, device=device, seed=args.random_seed, **_scoring_rule_options(args), **extra))
        table = format_comparison_table(names, res)
        with open(os.path.join(dirs[0], "comparison_recalibrated.txt" if args.recalibration else "comparison.txt"), "w") as f:
            f.write(table + "\n")
        print(table)
        return res

    if args.eval_only:
        return evaluate_all("cuda:%d" % local_rank) if rank == 0 else None
    _start_rank(args, world, rank, local_rank)
    for cfg in cfgs:
        if args.weights is not None:
            cfg.MODEL.WEIGHTS = args.weights
        if args.random_init:
            cfg.MODEL.WEIGHTS, cfg.OUTPUT_DIR = "", ""
        cfg.MODEL.DEVICE = "cuda:%d" % local_rank
    cfg = cfgs[0]
    K, dev = cfg.MODEL.RETINANET.NUM_CLASSES, cfg.MODEL.DEVICE
    dataset = CocoImages(args.coco_json, args.image_root, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST,
                         device_resize=args.resize_on_gpu) if args.coco_json else None
    if dataset is not None:
        args.num_images = len(dataset)
    mine = shard_indices(args.num_images, rank, world)
    torch.manual_seed(args.random_seed)
    compare = build_comparison(cfgs)
    compare.return_device = True
    compare.sparse_bbox_tower = not args.dense_bbox and os.environ.get("POD_SPARSE_BBOX", "1") != "0"
    for m in [compare.model] + list(compare.model_list):
        if isinstance(m, modeling.ProbabilisticRetinaNet):
            m.enable_graphs(not args.no_graphs)
            m.graph_after_seen = 2
    # the streams of the config that asks for the fewest: an MC-dropout config's masks are keyed by the forward number of a stream, so
    # its files are those of its own run only on its own run's streams; the other configs' bytes do not depend on the stream count
    own_streams = [2 if p.mc_dropout_enabled and p.num_mc_dropout_runs > 1 else 3 if p.inference_mode == "ensembles" and len(p.model_list) > 1 else 4
                   for p in compare.predictors]
    n_streams = args.streams if args.streams > 0 else min(own_streams)
    streams = [torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(n_streams - 1)]
    width, F, N = record_width(K), max(1, args.flush_every), len(cfgs)
    n_mine = len(shard_indices(args.num_images, 0, world))
    all_ids: List[List[int]] = [[] for _ in range(N)]
    all_cnt, all_rec = [[] for _ in range(N)], [[] for _ in range(N)]

    def flush(chunk_ids, recs, cnts):
        """One collective per config: this chunk's records of every rank, image order restored."""
        for st in streams[1:]:
            streams[0].wait_stream(st)
        for k in range(N):
            rec = torch.stack(recs[k]) if recs[k] else torch.zeros((0, 128, width), device=dev)
            cnt = torch.stack(cnts[k]) if cnts[k] else torch.zeros((0,), dtype=torch.int32, device=dev)
            ids, cnt, rec = gather_records(chunk_ids, cnt, rec, args.num_images, world, per_rank=F)
            all_ids[k].extend(ids)
            all_cnt[k].append(cnt.cpu())
            all_rec[k].append(rec.cpu())

    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    chunk_ids, recs, cnts = [], [[] for _ in range(N)], [[] for _ in range(N)]
    workers = args.loader_workers if args.loader_workers >= 0 else int(cfg.DATALOADER.NUM_WORKERS)
    loaded = iter(Prefetched(dataset, mine, workers=workers)) if dataset is not None else None
    with torch.no_grad():
        for j in range(n_mine):
            if j < len(mine):
                i = mine[j]
                if loaded is not None:
                    _, d = next(loaded)
                with torch.cuda.stream(streams[j % len(streams)]):
                    input_im, _ = _network_input(args, cfg, d if dataset is not None else None, i, dev)
                    dets = compare(input_im)
                    chunk_ids.append(i)
                    for k, det in enumerate(dets):
                        recs[k].append(det.records)
                        cnts[k].append(det.n_det)
                if os.environ.get("POD_SYNC_EACH_IMAGE") == "1":
                    torch.cuda.synchronize()
            if (j + 1) % F == 0 or j + 1 == n_mine:
                flush(chunk_ids, recs, cnts)
                chunk_ids, recs, cnts = [], [[] for _ in range(N)], [[] for _ in range(N)]
    torch.cuda.synchronize()
    t_loop = time.perf_counter() - t_loop
    if rank == 0:
        cat_map = category_mapping(args.train_dataset, args.test_dataset)
        for k in range(N):
            ids, cnt, rec = _image_order(all_ids[k], all_cnt[k], all_rec[k], width, dataset)
            os.makedirs(dirs[k], exist_ok=True)
            with open(outputs[k], "w") as fp:
                json.dump(results_json(ids, cnt, rec, K, cat_map), fp, indent=4, separators=(",", ": "))
            if sidecars[k]:
                from .inference_utils import write_binary_results
                write_binary_results(sidecars[k], ids, cnt, rec, K)
            print("wrote %s: %d images, %d detections" % (outputs[k], len(ids), int(cnt.sum())))
        if t_loop > 0:
            print("comparison loop: %d images x %d configs on %d rank(s) in %.2f s = %.1f images/s; per image %d model evaluation(s) and %d "
                  "front(s) (%d stream(s) per GPU)" % (args.num_images, N, world, t_loop, args.num_images / t_loop,
                                                        len(compare.families), sum(len(f.subfamilies) for f in compare.families), n_streams))
    res = evaluate_all(dev) if rank == 0 and args.eval else None
    if world > 1:
        dist.destroy_process_group()
    return res


def main(argv=None):
    from .config import setup_config
    from .probabilistic_inference import build_predictor
    ap = argparse.ArgumentParser()
    here = os.path.dirname(os.path.abspath(__file__))
    ap.add_argument("--config-file", default=os.path.join(here, "configs/BDD-Detection/retinanet/retinanet_R_50_FPN_1x_reg_cls_var_dropout.yaml"))
    ap.add_argument("--inference-config", nargs="+", default=[os.path.join(here, "configs/Inference/bayes_od_mc_dropout.yaml")],
                    help="one inference YAML, or several to compare on ONE pass over the data: the configs whose model evaluation is the same call "
                         "share it, those that also share the candidate list share merge + score, top-k, decode and NMS, and every config writes "
                         "coco_instances_results.json (with --binary-output NAME its sidecar, with --eval its mAP_res.txt) to <OUTPUT_DIR>/inference/"
                         "<test data set>/<name of its YAML>/ -- the bytes of its own run; --eval ends with comparison.txt beside the first.  "
                         "Configs that share an evaluation but not the candidate list (pre- and post-NMS ensembles together) get the bbox side "
                         "evaluated on every cell: their files are those of their own runs under --dense-bbox.  --output, --vis-dir and "
                         "--ensemble-per-gpu take one config")
    ap.add_argument("--num-images", type=int, default=8, help="synthetic 1280x720 frames (ignored with --coco-json)")
    ap.add_argument("--coco-json", default="", help="COCO-format json whose `images` are run (the reference's test data loader, AN:83-84)")
    ap.add_argument("--image-root", default="", help="directory of the files named in --coco-json")
    ap.add_argument("--train-dataset", default="bdd_train", help="cfg.DATASETS.TRAIN[0] of the model (AN:53): with --test-dataset it fixes the category map (AN:52-80)")
    ap.add_argument("--test-dataset", default="bdd_val", help="the data set the detections are written for (AN:55, args.test_dataset)")
    ap.add_argument("--dense-bbox", action="store_true",
                    help="evaluate bbox_subnet / bbox_pred / bbox_cov on every cell, in the reference's order (PR:518-537).  Default since round 6: the "
                         "SPARSE order -- cls side first, candidates selected (PI:283-308), bbox side only over the blocks that can reach a candidate "
                         "(PI:310-331 reads nothing else; pod_compare_amd/sparse.py): the same detections, a function of the image alone "
                         "(tests/test_sparse_tower_gpu.py), 1.3 x the images/s with MC dropout.  --ensemble-per-gpu (one member per GPU) is always dense")
    ap.add_argument("--sparse-bbox", action="store_true", help="(the default; kept for round-5 command lines)")
    ap.add_argument("--random-seed", type=int, default=0)
    ap.add_argument("--output", default=None, help="the result file (default coco_instances_results.json)")
    ap.add_argument("--no-graphs", action="store_true", help="issue every launch of a forward from Python instead of replaying a HIP graph per (stream, frame shape)")
    ap.add_argument("--streams", type=int, default=0,
                    help="HIP streams per GPU; consecutive images of a rank go to different streams (batch 1 per stream, AN:35); 0 = 2 with "
                         "MC dropout (several runs per image), 3 for an in-process ensemble, 4 otherwise (profiles/r05_streams_sweep.txt)")
    ap.add_argument("--loader-workers", type=int, default=-1,
                    help="host threads that read / decode / resize the files of --coco-json ahead of the GPU (the reference's DATALOADER.NUM_WORKERS); "
                         "-1 = the config's value, 0 = in the main loop")
    ap.add_argument("--resize-on-gpu", action="store_true",
                    help="--coco-json: the loader threads only decode; ResizeShortestEdge (PIL's uint8 bilinear filter), the RGB -> BGR flip and the "
                         "HWC -> CHW transpose run on the GPU in one launch on the image's stream (K20).  Bit-identical to the host path: the same "
                         "network input, the same detections.  Off by default")
    ap.add_argument("--flush-every", type=int, default=64,
                    help="images per rank between two gathers of the device-resident records (SURVEY 8e: ~0.74 MB per rank and flush)")
    ap.add_argument("--ensemble-per-gpu", action="store_true",
                    help="BASELINE config 5: rank s < M runs ensemble member s, dense pre-NMS tensors meet on a rotating merge rank")
    ap.add_argument("--binary-output", default="", help="also write the detections as a binary sidecar (inference_utils.write_binary_results)")
    ap.add_argument("--data-dir", default="", help="the reference's core.data_dir(): OUTPUT_DIR = <data-dir>/<dataset>/<family>/<config>/"
                                                   "random_seed_<seed>, whose last_checkpoint is loaded (CS:170-182, PI:59-84)")
    ap.add_argument("--weights", default=None, help="overrides MODEL.WEIGHTS (a local .pth / .pkl with detectron2 names)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend: nccl = RCCL over xGMI (the real path); gloo for a "
                                                      "functional run, e.g. several ranks on one GPU with --share-gpu")
    ap.add_argument("--share-gpu", action="store_true", help="functional check only: every rank uses cuda:0")
    ap.add_argument("--random-init", action="store_true",
                    help="synthetic runs: clear MODEL.WEIGHTS / OUTPUT_DIR and keep the seeded random initialisation")
    ap.add_argument("--eval", action="store_true",
                    help="after writing --output, evaluate it as the reference's AN:104-106 does: AP (mAP_res.txt beside --output), PM and CE on "
                         "this GPU (needs --coco-json with `annotations`).  The PM / CE threshold: --min-allowed-score, else --map-results, else "
                         "the AP step's own when --test-dataset is the model's own test set (bdd_val for a BDD model), else 0.0 -- the reference "
                         "reads the training family's mAP_res.txt instead (PM:50-65 / CE:47-63)")
    ap.add_argument("--eval-only", action="store_true", help="build no model, run no inference: evaluate --output (or --binary-output if only "
                                                             "that is given) as --eval does")
    ap.add_argument("--min-allowed-score", type=float, default=None, help="--eval: the detections' score threshold of PM and CE")
    ap.add_argument("--map-results", default="", help="--eval: take the PM / CE threshold from this mAP_res.txt (PM:50-65)")
    from .compute_probabilistic_metrics import add_scoring_rule_arguments
    add_scoring_rule_arguments(ap)          # --eval: --scoring-rules nll [energy] [crps] [brier], --energy-samples (draws keyed by --random-seed)
    ap.add_argument("--pdq", action="store_true", help="--eval: also PDQ, the probability-based detection quality (compute_pdq, K34), under the PM / CE "
                                                       "threshold: its table, its dict under \"pdq\" and a PDQ column in comparison.txt")
    ap.add_argument("--p-min", type=float, default=0.0027, help="--pdq: a pixel belongs to a detection's segment when P(pixel in box) >= this")
    ap.add_argument("--vis-dir", default="", help="also write every image of this rank annotated as visualize_inference draws it (PI:113-146): "
                                                   "the first --vis-max-boxes detections with their corner-covariance ellipses over the frame at "
                                                   "its original size, rendered on the GPU (K19) and encoded on host threads as <dir>/<file stem>.png")
    ap.add_argument("--vis-max-boxes", type=int, default=20, help="--vis-dir: detections drawn per image (PI:125)")
    ap.add_argument("--vis-ellipse-pairing", choices=("reference", "box"), default="reference",
                    help="--vis-dir: reference = the ellipses as PV:70-86 pairs them (the box drawn k-th, by area, gets the k-th covariance of "
                         "the result order); box = every box with its own covariance")
    ap.add_argument("--corruption", default=None,
                    help="--coco-json: corrupt every decoded frame on the GPU before the resize (K35, corruptions.py): gaussian_noise, speckle_noise, "
                         "impulse_noise, gaussian_blur, defocus_blur, brightness, contrast or saturate, after ImageNet-C.  Needs --severity; implies "
                         "--resize-on-gpu.  The noise of image i is keyed by (--random-seed, i): the bytes do not depend on ranks or streams.  With "
                         "several --inference-config paths the directories are <test data set>_<NAME>_<N>")
    ap.add_argument("--severity", type=int, default=None, help="--corruption: 1 (mild) to 5")
    ap.add_argument("--recalibration", nargs="+", default=None, metavar="FILE",
                    help="--eval / --eval-only: recalibrate the detections on the GPU (K36) with the map `python -m pod_compare_amd.recalibrate fit` "
                         "wrote, after loading and before AP; one file per --inference-config, in order.  The AP step then writes "
                         "mAP_res_recalibrated.txt and a comparison pass comparison_recalibrated.txt: a raw run's files are never overwritten")
    args = ap.parse_args(argv)
    _check_corruption(args)
    _check_recalibration(args)
    if len(args.inference_config) > 1:
        return _main_comparison(args, list(args.inference_config))
    args.inference_config = args.inference_config[0]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    evaluating = args.eval or args.eval_only
    if evaluating:
        if not has_ground_truth(args.coco_json):
            raise SystemExit("--eval / --eval-only need ground truth: --coco-json with `annotations`")
        if args.ensemble_per_gpu:
            raise SystemExit("--ensemble-per-gpu runs on the synthetic frames only: it cannot be evaluated (--eval)")
    if args.vis_dir and args.ensemble_per_gpu:
        raise SystemExit("--vis-dir draws the images of the sharded loop; --ensemble-per-gpu is not supported")
    if args.eval_only:
        binary = bool(args.binary_output) and args.output is None
        if int(os.environ.get("RANK", "0")) != 0:
            return None
        local_rank = 0 if args.share_gpu else int(os.environ.get("LOCAL_RANK", "0"))
        return evaluate_results(args.binary_output if binary else (args.output or "coco_instances_results.json"), args.coco_json,
                                args.train_dataset, args.test_dataset, binary=binary, min_allowed_score=args.min_allowed_score,
                                map_results=args.map_results, device="cuda:%d" % local_rank, seed=args.random_seed, **_scoring_rule_options(args),
                                **_recalibration_option(args))
    if args.output is None:
        args.output = "coco_instances_results.json"
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.share_gpu:
        local_rank = 0
    _start_rank(args, world, rank, local_rank)
    cfg = setup_config(args.config_file, args.inference_config, args.random_seed, data_dir=args.data_dir, is_testing=bool(args.data_dir))
    if args.weights is not None:
        cfg.MODEL.WEIGHTS = args.weights
    if args.random_init:
        cfg.MODEL.WEIGHTS, cfg.OUTPUT_DIR = "", ""
    cfg.MODEL.DEVICE = "cuda:%d" % local_rank
    K = cfg.MODEL.RETINANET.NUM_CLASSES
    from . import modeling
    dataset = CocoImages(args.coco_json, args.image_root, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST,
                         device_resize=args.resize_on_gpu) if args.coco_json else None
    if dataset is not None:
        if args.ensemble_per_gpu:
            raise SystemExit("--ensemble-per-gpu runs on the synthetic frames only")
        args.num_images = len(dataset)
    mine = shard_indices(args.num_images, rank, world)
    recs, cnts = [], []
    if args.ensemble_per_gpu:
        recs, cnts = _run_ensemble_per_gpu(cfg, args, rank, world)
    torch.manual_seed(args.random_seed)
    predictor = build_predictor(cfg) if not args.ensemble_per_gpu else None
    if predictor is not None:
        predictor.return_device = True      # no per-image host sync: records and counts stay in HBM until the gather
        # every image is evaluated on ONE GPU here (image sharding): the sparse order is the default; POD_SPARSE_BBOX=0 / --dense-bbox give the dense one
        predictor.sparse_bbox_tower = not bool(getattr(args, "dense_bbox", False)) and os.environ.get("POD_SPARSE_BBOX", "1") != "0"
        for m in [predictor.model] + list(predictor.model_list):
            if isinstance(m, modeling.ProbabilisticRetinaNet):
                m.enable_graphs(not getattr(args, "no_graphs", False))      # one host call per forward instead of ~200 launches
                m.graph_after_seen = 2                                      # (a frame size is captured once it has come back: data sets of many sizes stay eager)
    # images are independent units: keep a few in flight on separate HIP streams so one image's low-occupancy backbone
    # stretches overlap another image's head convs (+12 % images/s on one MI355X); the predictor keeps a workspace per stream
    mc = getattr(predictor, "mc_dropout_enabled", False) and getattr(predictor, "num_mc_dropout_runs", 1) > 1
    n_streams = args.streams if args.streams > 0 else (2 if mc else 3 if len(getattr(predictor, "model_list", [])) > 1 else 4)
    streams = [torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(n_streams - 1)]
    width = record_width(K)
    dev = cfg.MODEL.DEVICE
    F = max(1, args.flush_every)
    n_mine = len(shard_indices(args.num_images, 0, world))          # rank 0 owns the most images: every rank flushes as often
    all_ids: List[int] = []
    all_cnt, all_rec = [], []
    flushed: List[Tuple[float, int]] = []

    def flush(chunk_ids, recs, cnts):
        """ONE collective: this chunk's records of every rank, image order restored (device memory stays bounded)."""
        for st in streams[1:]:
            streams[0].wait_stream(st)          # the gather reads every stream's records
        rec = torch.stack(recs) if recs else torch.zeros((0, 128, width), device=dev)
        cnt = torch.stack(cnts) if cnts else torch.zeros((0,), dtype=torch.int32, device=dev)
        ids, cnt, rec = gather_records(chunk_ids, cnt, rec, args.num_images, world, per_rank=F)
        all_ids.extend(ids)
        all_cnt.append(cnt.cpu())
        all_rec.append(rec.cpu())
        flushed.append((time.perf_counter(), len(all_ids)))       # (the host copies above waited for the records)

    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    if args.ensemble_per_gpu:
        flush_ids = list(mine)
        for a in range(0, max(n_mine, 1), F):
            flush(flush_ids[a:a + F], recs[a:a + F], cnts[a:a + F])
    else:
        chunk_ids: List[int] = []
        recs, cnts = [], []
        workers = args.loader_workers if args.loader_workers >= 0 else int(cfg.DATALOADER.NUM_WORKERS)
        loaded = iter(Prefetched(dataset, mine, workers=workers)) if dataset is not None else None
        vis = None
        if args.vis_dir:
            from .visualization import InferenceFrameWriter
            vis = InferenceFrameWriter(args.vis_dir, args.vis_max_boxes, bgr=str(cfg.INPUT.FORMAT) == "BGR", workers=max(1, workers),
                                       cov_pairing=args.vis_ellipse_pairing)
        with torch.no_grad():
            for j in range(n_mine):
                if j < len(mine):
                    i = mine[j]
                    if loaded is not None:
                        _, d = next(loaded)                             # resized on the host exactly as detectron2's mapper does, a few entries ahead
                    with torch.cuda.stream(streams[j % len(streams)]):
                        input_im, frame = _network_input(args, cfg, d if dataset is not None else None, i, dev)
                        det = predictor(input_im)
                        if vis is not None:           # enqueued behind the detections on this stream; not part of any captured graph
                            if dataset is not None:
                                vis.add(os.path.splitext(os.path.basename(d["file_name"]))[0] + ".png", input_im[0]["image"], d["height"], d["width"], det)
                            else:
                                vis.add("%06d.png" % i, frame, frame.shape[1], frame.shape[2], det)
                        chunk_ids.append(i)
                        recs.append(det.records)
                        cnts.append(det.n_det)
                    if os.environ.get("POD_SYNC_EACH_IMAGE") == "1":    # debugging aid: serialise the streams
                        torch.cuda.synchronize()
                if (j + 1) % F == 0 or j + 1 == n_mine:
                    flush(chunk_ids, recs, cnts)
                    chunk_ids, recs, cnts = [], [], []
        if vis is not None:
            vis.close()
            print("rank %d: wrote %d annotated frames to %s" % (rank, vis.count, args.vis_dir))
    torch.cuda.synchronize()
    t_loop = time.perf_counter() - t_loop
    ids, cnt, rec = _image_order(all_ids, all_cnt, all_rec, width, dataset)
    if rank == 0:
        with open(args.output, "w") as fp:
            json.dump(results_json(ids, cnt, rec, K, category_mapping(args.train_dataset, args.test_dataset)), fp, indent=4, separators=(",", ": "))
        if args.binary_output:
            from .inference_utils import write_binary_results
            write_binary_results(args.binary_output, ids, cnt, rec, K)
        print("wrote %s: %d images, %d detections" % (args.output, len(ids), int(cnt.sum())))
        if not args.ensemble_per_gpu and t_loop > 0:           # (first images included: eager forwards, then the graph captures)
            steady = ""
            if len(flushed) >= 2 and flushed[-1][0] > flushed[0][0]:
                steady = "; %.1f images/s after the first flush" % ((flushed[-1][1] - flushed[0][1]) / (flushed[-1][0] - flushed[0][0]))
            print("inference loop: %d images on %d rank(s) in %.2f s = %.1f images/s%s (%d stream(s) per GPU%s)" % (
                len(ids), world, t_loop, len(ids) / t_loop, steady, n_streams,
                ", %d loader thread(s)%s" % (workers, ", resized on the GPU" if args.resize_on_gpu else "") if dataset is not None else ", synthetic frames made on the device"))
    res = None
    if rank == 0 and args.eval:
        res = evaluate_results(args.output, args.coco_json, args.train_dataset, args.test_dataset, min_allowed_score=args.min_allowed_score,
                               map_results=args.map_results, device=dev, seed=args.random_seed, **_scoring_rule_options(args), **_recalibration_option(args))
    if world > 1:
        dist.destroy_process_group()
    return res


if __name__ == "__main__":
    main()
