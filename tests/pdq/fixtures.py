"""The fixtures of tests/pdq/: small frames (96x64, 97x61: a ragged last row and column is where the kernel can go wrong) and one 301-wide
strip whose region of interest spans two 256-column chunks.  Every image is a dict of numpy arrays: frame (W, H), means (D, 4),
covs (D, 4, 4), probs (D, K) fp32, gt_boxes (G, 4) fp32, gt_classes (G,) int.  Seeded, so the condition on the fixtures
(test_probabilistic_metrics.py) is a property of these very numbers."""
import numpy as np

K = 7
GT_BOX = [20.3, 12.7, 70.2, 50.1]


def _probs(rng, n):
    e = np.exp(rng.normal(size=(n, K)))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def _full_cov(rng):
    L = np.tril(rng.normal(scale=0.7, size=(4, 4)), -1) + np.diag(rng.uniform(1.0, 3.0, size=4))
    return (L @ L.T).astype(np.float32)


def image(frame, means, covs, probs, gt_boxes, gt_classes):
    f32 = lambda a, shape: np.asarray(a, dtype=np.float32).reshape(shape)
    return {"frame": tuple(frame), "means": f32(means, (-1, 4)), "covs": f32(covs, (-1, 4, 4)), "probs": f32(probs, (-1, K)),
            "gt_boxes": f32(gt_boxes, (-1, 4)), "gt_classes": np.asarray(gt_classes, dtype=np.int64).reshape(-1)}


def jittered(seed=34, n=3, frame=(96, 64)):
    """The first family: the ground truth with detections jittered by N(0, 2^2) and random full covariances L L^T, diag(L) in [1, 3]."""
    rng = np.random.default_rng(seed)
    means = np.asarray(GT_BOX) + rng.normal(scale=2.0, size=(n, 4))
    return image(frame, means, [_full_cov(rng) for _ in range(n)], _probs(rng, n), [GT_BOX], [2])


def edge_cases(frame=(97, 61)):
    """Partly and wholly off the frame; a region of interest that is the whole frame (sd 40); the variance floor (cov = 0: P is nearly a
    step); rho beyond the clamp on both signs."""
    rng = np.random.default_rng(35)
    eye = np.eye(4)
    beyond = lambda s: np.array([[4.0, s * 3.999, 0, 0], [s * 3.999, 4.0, 0, 0], [0, 0, 9.0, s * 8.999], [0, 0, s * 8.999, 9.0]])
    means = [[-15.2, -8.4, 40.3, 30.6], [120.5, 70.5, 160.5, 100.5], [22.1, 14.2, 68.4, 48.9], [20.9, 13.1, 69.6, 49.4],
             [21.2, 11.9, 71.3, 51.2], [19.4, 13.6, 69.1, 49.0]]
    covs = [4.0 * eye, 4.0 * eye, 1600.0 * eye, 0.0 * eye, beyond(1.0), beyond(-1.0)]
    return image(frame, means, covs, _probs(rng, 6), [GT_BOX, [-10.0, -5.0, 30.4, 20.2]], [1, 4])


def zero_rules(frame=(96, 64)):
    """A ground truth with n_i = 0 (no pixel centre inside), one disjoint from every detection's segment, and an invalid detection (a
    negative variance) between two valid ones; a second invalid one (a mean that is not finite) follows."""
    rng = np.random.default_rng(36)
    means = [[21.0, 13.0, 69.0, 49.5], [20.0, 12.0, 70.0, 50.0], [19.7, 12.2, 70.9, 50.8], [np.inf, 12.0, 70.0, 50.0]]
    bad = np.diag([4.0, -1.0, 4.0, 4.0])
    covs = [_full_cov(rng), bad, _full_cov(rng), 4.0 * np.eye(4)]
    gts = [GT_BOX, [30.6, 20.6, 30.9, 20.9], [84.0, 1.0, 95.0, 7.0]]
    return image(frame, means, covs, _probs(rng, 4), gts, [0, 3, 6])


def no_ground_truth(frame=(96, 64)):
    im = jittered(37, 2, frame)
    return image(frame, im["means"], im["covs"], im["probs"], [], [])


def no_detections(frame=(97, 61)):
    return image(frame, [], [], [], [GT_BOX, [5.0, 5.0, 15.0, 15.0]], [2, 5])


def many_ground_truths(frame=(96, 64)):
    """G = 70 small boxes (more ground truths than a wavefront has lanes) under three detections."""
    rng = np.random.default_rng(38)
    gts = [[3.2 + 9.1 * c, 2.6 + 8.7 * r, 3.2 + 9.1 * c + 5.9, 2.6 + 8.7 * r + 5.3] for r in range(7) for c in range(10)]
    picks = (12, 37, 58)
    means = [np.asarray(gts[i]) + rng.normal(scale=1.0, size=4) for i in picks]
    return image(frame, means, [_full_cov(rng) for _ in picks], _probs(rng, 3), gts, rng.integers(0, K, size=70))


def two_chunks(frame=(301, 7)):
    """A strip wider than one 256-column chunk: the detection's region of interest is the whole frame, the ground truth spans the seam."""
    rng = np.random.default_rng(39)
    return image(frame, [[236.4, 1.2, 272.3, 5.8]], [np.diag([90000.0, 1.0, 90000.0, 1.0])], _probs(rng, 1), [[240.2, 1.3, 270.7, 5.6], [2.0, 0.0, 12.0, 7.0]], [1, 1])


def all_images():
    return [jittered(), edge_cases(), zero_rules(), no_ground_truth(), no_detections(), many_ground_truths(), two_chunks()]


def permuted(im, order):
    order = np.asarray(order)
    return dict(im, means=im["means"][order], covs=im["covs"][order], probs=im["probs"][order])
