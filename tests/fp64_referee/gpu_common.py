"""What the fp64 referee's GPU tests share: the acceptance rule applied to one quantity, with its rows in the parity report."""
import torch

from tests import helpers
from tests.fp64_referee import f64_ref as fr


def hold_records(det, m, k):
    """K7's fixed-stride records carry the XYWH box and T cov T^T (instances_to_json).  T's entries are 0 and +-1, so every entry of
    T cov T^T is one or two fp32 subtractions whatever the summation order (adding a zero product is exact): the records must be the
    float32 transform of K7's OWN output rows bit for bit, and those rows are held to fp64 by the rule.  (The rule itself does not
    apply to T cov T^T: Var(w) = C_00 + C_22 - 2 C_02 cancels to a fraction of the variances, so the worst of a few hundred entries is
    one entry's amplified ulp -- two equally good fp32 covariances then differ by more than 2x in max, 1.2x in rms.)"""
    rec = det.records[:m].cpu()
    b, c = det.boxes[:m].cpu(), det.cov[:m].cpu()
    assert torch.equal(rec[:, 0:4], torch.stack((b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]), 1))
    assert torch.equal(rec[:, 6 + k:].reshape(m, 4, 4), fr.cov_xyxy_to_xywh(c))


def hold(what, kind, hip, ref32, ref64, must_beat=False):
    """The rule of profiles/fp64_referee.md for one quantity: e_hip = normalised error of the HIP result against the fp64 referee,
    e_ref = the fp32 oracle's over the same entries; max(e_hip) <= 2 max(e_ref) + 4 ulp and the same for the rms.
    kind: "box" (error over max(1, |ref|)) or "cov" (over sqrt(C_ii C_jj) of the fp64 matrix).
    must_beat: additionally max(e_hip) <= max(e_ref) (the cluster kernels' fused covariance at condition >= 1e4: inversion in fp64).
    Prints the figures before it asserts; returns them."""
    hip, ref32, ref64 = torch.as_tensor(hip).cpu(), torch.as_tensor(ref32), torch.as_tensor(ref64)
    assert hip.shape == ref32.shape == ref64.shape, (what, tuple(hip.shape), tuple(ref32.shape), tuple(ref64.shape))
    assert ref64.dtype == torch.float64 and hip.dtype == torch.float32 and ref32.dtype == torch.float32
    err = fr.box_error if kind == "box" else fr.cov_error
    e_hip, e_ref = err(hip, ref64), err(ref32, ref64)
    ok, fig = fr.within_rule(e_hip, e_ref)
    helpers.record_referee(what, fig)
    if e_hip.numel():
        allowed = torch.full_like(e_hip, fr.MARGIN * fig["ref_max"] + fr.FLOOR)
        helpers._record("fp64 referee: " + what + ", e_hip", e_hip, allowed, ref64)
        helpers._record("fp64 referee: " + what + ", e_ref", e_ref, allowed, ref64)
    print("%s: n=%d e_hip max %.3e rms %.3e | e_ref max %.3e rms %.3e | ratio max %.2f rms %.2f" % (
        what, fig["n"], fig["hip_max"], fig["hip_rms"], fig["ref_max"], fig["ref_rms"], fig["ratio_max"], fig["ratio_rms"]))
    assert ok, (what, fig)
    if must_beat:
        assert fig["hip_max"] <= fig["ref_max"], (what, "HIP further from fp64 than the fp32 reference", fig)
    return fig
