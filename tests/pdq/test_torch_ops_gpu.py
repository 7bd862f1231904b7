"""torch.ops.pod_mi355x.pdq_pairs gives the direct call's bits and checks its arguments.

The module shares its name with tests/test_torch_ops_gpu.py for its place in the GPU run order (tests/conftest.py: GPU_ORDER)."""
import numpy as np
import pytest
import torch

from tests.pdq import fixtures as fx
from tests.pdq import gpu_common as gc
from tests.pdq import pdq_ref as pr

pytestmark = pytest.mark.gpu


def test_pdq_pairs_operator_gives_the_direct_calls_bits():
    import pod_compare_amd.torch_ops  # noqa: F401  (registers the library)
    ims = [fx.jittered(), fx.zero_rules(), fx.no_detections(), fx.two_chunks()]
    frames, det_off, gt_off, pair_off = gc.tables(ims)
    cat = lambda key, shape, dt: torch.from_numpy(np.concatenate([np.asarray(im[key]).reshape(shape) for im in ims]).astype(dt)).to(gc.DEV)
    args = (frames, det_off, gt_off, cat("means", (-1, 4), np.float32), cat("covs", (-1, 4, 4), np.float32), cat("probs", (-1, fx.K), np.float32),
            cat("gt_boxes", (-1, 4), np.float32), cat("gt_classes", (-1,), np.int64))
    quality, invalid = torch.ops.pod_mi355x.pdq_pairs(*args)
    assert quality.dtype == torch.float64 and tuple(quality.shape) == (5, int(pair_off[-1])) and invalid.dtype == torch.int32
    direct = gc.pairs(ims)
    for m, r in enumerate(direct):
        a, b = int(pair_off[m]), int(pair_off[m + 1])
        for k, name in enumerate(pr.PLANES):
            assert quality[k, a:b].cpu().numpy().tobytes() == r[name].tobytes(), (m, name)
        assert np.array_equal(invalid[int(det_off[m]):int(det_off[m + 1])].cpu().numpy().astype(bool), r["invalid"])
    other, _ = torch.ops.pod_mi355x.pdq_pairs(*args, 0.05)
    assert not torch.equal(other, quality)
    with pytest.raises(RuntimeError):
        torch.ops.pod_mi355x.pdq_pairs(*args, 1.0)                              # p_min outside (0, 1)
    with pytest.raises(RuntimeError):
        torch.ops.pod_mi355x.pdq_pairs(*args[:3], args[3][:-1], *args[4:])      # a row short
    with pytest.raises(RuntimeError):
        torch.ops.pod_mi355x.pdq_pairs(frames.to(gc.DEV), *args[1:])            # the tables are host tables
