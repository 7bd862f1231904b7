"""visualize_predictions.py (VP:20-142) without the GUI: every frame of a COCO-format ground-truth file drawn with its ground truth (light
green, class names) and the predictions of a result file (2-sigma corner-covariance ellipses, entropy colours, scores), at scale 1.5, on
the GPU (visualization.py, K19), written as <output-dir>/<file stem>.png.

    python -m pod_compare_amd.visualize_predictions --results coco_instances_results.json --gt val_coco_format.json \
        --image-root <dir> --output-dir <dir> [--max-images N] [--min-allowed-score 0.5]

VP:52 overrides any threshold it read with 0.5: that is the default here, and --min-allowed-score changes it.
"""
import argparse
import json
import os
from typing import List, Optional

import numpy as np
import torch

from . import apply_net, evaluation_utils, visualization


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--results", required=True, help="coco_instances_results.json (apply_net --output)")
    ap.add_argument("--gt", required=True, help="the COCO-format ground truth (images, annotations)")
    ap.add_argument("--image-root", required=True, help="directory of the files named in --gt")
    ap.add_argument("--output-dir", required=True)
    apply_net.add_dataset_arguments(ap)
    ap.add_argument("--min-allowed-score", type=float, default=0.5, help="predictions below this top class probability are not drawn (VP:52)")
    ap.add_argument("--scale", type=float, default=1.5, help="canvas scale of the frames (VP:72-75)")
    ap.add_argument("--max-images", type=int, default=0, help="only the first N images of --gt (0: all)")
    ap.add_argument("--batch", type=int, default=8, help="frames per render launch")
    ap.add_argument("--writers", type=int, default=4, help="host threads encoding the PNG files")
    ap.add_argument("--ellipse-pairing", choices=sorted(visualization.COV_PAIRINGS), default="reference",
                    help="reference: as PV:70-86 draws them -- boxes are sorted by area but the covariances are not, so the box drawn k-th "
                         "gets the k-th covariance of the result order; box: every box with its own covariance")
    ap.add_argument("--device", default="cuda")
    return ap.parse_args(argv)


def output_name(output_dir: str, file_name: str) -> str:
    return os.path.join(output_dir, os.path.splitext(os.path.basename(file_name))[0] + ".png")


def _read_rgb(path: str) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"))


def main(argv=None) -> List[str]:
    args = parse_args(argv)
    dev = torch.device(args.device)
    if dev.type == "cuda" and dev.index is not None:
        torch.cuda.set_device(dev)
    with open(args.gt, "r") as f:
        gt = json.load(f)
    with open(args.results, "r") as f:
        results = json.load(f)
    images = list(gt["images"])
    if args.max_images > 0:
        images = images[:args.max_images]
    # VP:67, VP:119-122 label ground truth with the test set's class names; through the evaluators' map (EU:370-397: test id -> the model's
    # contiguous id) and the model's (training set's) class names that is the same name for every pair the map accepts, and a pair it
    # does not accept is refused here as the evaluators refuse it
    to_model = apply_net.evaluation_category_map(args.train_dataset, args.test_dataset)
    classes = apply_net.THING_CLASSES[apply_net._family(args.train_dataset)]
    pred = evaluation_utils.eval_predictions_preprocess(results, min_allowed_score=args.min_allowed_score, device=dev)
    gts = evaluation_utils.eval_gt_preprocess(gt.get("annotations", []), device=dev)
    os.makedirs(args.output_dir, exist_ok=True)
    writer = visualization.ImageWriter(args.writers)
    written = []
    try:
        for a in range(0, len(images), max(1, args.batch)):
            chunk = images[a:a + max(1, args.batch)]
            frames = []
            for info in chunk:
                image_id = info["id"]
                img = torch.from_numpy(_read_rgb(os.path.join(args.image_root, info["file_name"]))).to(dev)
                lists = []
                gb = gts["gt_boxes"].get(image_id)
                if gb is not None and gb.shape[0] > 0:
                    cats = gts["gt_cat_idxs"][image_id][:, 0].long().tolist()
                    labels = [classes[to_model[c]] if c in to_model else str(c) for c in cats]
                    lists.append(visualization.InstanceList(gb, colour=visualization.LIGHTGREEN, labels=labels, alpha=1.0))
                pb = pred["predicted_boxes"].get(image_id)
                if pb is not None and pb.shape[0] > 0:
                    probs = pred["predicted_cls_probs"][image_id]
                    scores = probs.max(1).values.cpu().numpy()
                    lists.append(visualization.InstanceList(pb, cov=pred["predicted_covar_mats"][image_id], probs=probs,
                                                            labels=[str(np.float32(s)) for s in scores], alpha=1.0,
                                                            cov_pairing=args.ellipse_pairing))
                frames.append(visualization.Frame(img, lists=lists))
            canvases = visualization.render_frames(frames, args.scale)
            for info, canvas in zip(chunk, canvases):
                path = output_name(args.output_dir, info["file_name"])
                writer.submit(path, canvas.cpu().numpy())
                written.append(path)
    finally:
        writer.close()
    print("wrote %d annotated frames to %s" % (len(written), args.output_dir))
    return written


if __name__ == "__main__":
    main()
