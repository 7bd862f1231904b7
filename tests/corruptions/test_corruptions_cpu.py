"""K35 without a GPU: the severity table, the filters' tables against scipy, the key and counter map, the impulse threshold, the proof that
fp32 against fp64 meets the GPU tests' cap, the ABI's additions and apply_net's refusals and directory names."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from pod_compare_amd import apply_net, build, corruptions, hip
from tests.corruptions import corrupt_ref as ref
from tests.rng import rng_ref

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def test_table_and_names():
    assert corruptions.NAMES == ("gaussian_noise", "speckle_noise", "impulse_noise", "gaussian_blur", "defocus_blur", "brightness", "contrast",
                                 "saturate") == ref.NAMES
    assert corruptions.SEVERITY == ref.TABLE and set(corruptions.SEVERITY) == set(corruptions.NAMES)
    assert corruptions.parameters("gaussian_noise", 1) == 0.08 and corruptions.parameters("gaussian_noise", 5) == 0.38
    assert corruptions.parameters("defocus_blur", 5) == (10, 0.5) and corruptions.parameters("saturate", 4) == (5, 0.1)
    assert corruptions.parameters("contrast", 5) == 0.05 and corruptions.parameters("gaussian_blur", 5) == 6
    for name in corruptions.NAMES:
        assert len(corruptions.SEVERITY[name]) == 5
        for bad in (0, 6, -1, 2.0, None, True):
            with pytest.raises(ValueError, match="1, 2, 3, 4, 5"):
                corruptions.parameters(name, bad)
    with pytest.raises(ValueError, match="gaussian_noise.*saturate"):
        corruptions.parameters("fog", 1)
    assert [corruptions.KINDS[n] for n in corruptions.NAMES] == list(range(8)) == [
        hip.POD_CORRUPT_GAUSSIAN_NOISE, hip.POD_CORRUPT_SPECKLE_NOISE, hip.POD_CORRUPT_IMPULSE_NOISE, hip.POD_CORRUPT_GAUSSIAN_BLUR,
        hip.POD_CORRUPT_DEFOCUS_BLUR, hip.POD_CORRUPT_BRIGHTNESS, hip.POD_CORRUPT_CONTRAST, hip.POD_CORRUPT_SATURATE]


@pytest.mark.parametrize("sigma", corruptions.SEVERITY["gaussian_blur"])
def test_gaussian_taps_equal_scipys_kernel(sigma):
    t = corruptions.gaussian_taps(sigma)
    r = int(4 * sigma + 0.5)
    assert t.dtype == np.float64 and t.shape == (2 * r + 1,) and r <= 24
    e = np.zeros(2 * r + 1)
    e[r] = 1.0
    assert np.abs(t - ndimage.gaussian_filter1d(e, sigma, mode="constant", truncate=4.0)).max() <= 1e-15
    assert np.abs(t - ref.gaussian_kernel(sigma)).max() <= 1e-15


@pytest.mark.parametrize("radius,alias", corruptions.SEVERITY["defocus_blur"])
def test_defocus_stencil(radius, alias):
    s = corruptions.defocus_stencil(radius, alias)
    assert s.dtype == np.float64 and s.shape == ((17, 17) if radius <= 8 else (21, 21))
    assert np.abs(s - ref.stencil(radius, alias)).max() <= 1e-15
    assert np.array_equal(s, s.T) and np.array_equal(s, s[::-1]) and np.array_equal(s, s[:, ::-1])
    assert abs(s.sum() - 1.0) <= 1e-12 and s.min() >= 0.0
    r, taps = corruptions.filter_table("defocus_blur", corruptions.SEVERITY["defocus_blur"].index((radius, alias)) + 1)
    assert r == (8 if radius <= 8 else radius) <= corruptions.DEFOCUS_MAX_RADIUS and taps.dtype == np.float32 and taps.shape == s.shape


def test_key_and_counter():
    assert corruptions.corruption_key(0, 0) == 0
    assert corruptions.corruption_key(7, 3) == 7 | (3 << 32) == ref.key_of(7, 3)
    assert corruptions.corruption_key((5 << 32) | 9, (1 << 32) | 2) == 9 | (2 << 32)        # both masked to 32 bits
    assert corruptions.corruption_key(-1, 1) == 0xFFFFFFFF | (1 << 32)
    assert corruptions.STREAM_CORRUPT == ref.STREAM_CORRUPT == 0x636f7200
    assert ref.STREAM_CORRUPT not in set(rng_ref.STREAMS.values()) | {0x65767300}
    c = ref.counter(3, 5, 1)
    assert c.shape == (3, 5, 4) and c.dtype == np.uint32
    assert tuple(c[2, 4]) == (4, 2, 1, 0x636f7200) and tuple(ref.counter(3, 5, 0)[0, 0]) == (0, 0, 0, 0x636f7200)
    # pixels and the two calls never share a counter
    both = np.concatenate([ref.counter(37, 53, 0).reshape(-1, 4), ref.counter(37, 53, 1).reshape(-1, 4)])
    assert len(np.unique(both, axis=0)) == len(both)
    src = open(os.path.join(ROOT, "pod_compare_amd", "csrc", "k35_corrupt_u8.hip")).read()
    assert re.search(r"STREAM_CORRUPT\s*=\s*0x636f7200u", src)


def test_impulse_threshold():
    want = {0.03: 128849018, 0.06: 257698037, 0.09: 386547056, 0.17: 730144440, 0.27: 1159641169}
    for amount in corruptions.SEVERITY["impulse_noise"]:
        t = corruptions.impulse_threshold(amount)
        assert t == min(int(np.floor(np.float64(amount) * 2.0 ** 32)), 2 ** 32 - 1) == ref.impulse_threshold(amount) == want[amount]
    assert corruptions.impulse_threshold(1.0) == 2 ** 32 - 1 and corruptions.impulse_threshold(0.0) == 0


@pytest.mark.parametrize("name", ref.CAPPED)
def test_fp32_against_fp64_has_room_under_the_cap(name):
    """The cap of the GPU tests is a condition, not a measurement: fp32 arithmetic alone must meet it with a factor of 3 to spare."""
    for severity in ref.SEVERITIES:
        pairs = [(ref.corrupt_fp32(ref.frame(hw), name, severity, ref.key_of(ref.SEED, i)), ref.reference(name, severity, i))
                 for i, hw in enumerate(ref.FRAMES)]
        worst, differing, total, allowed = ref.within_cap(pairs)
        print("%s severity %d: %d of %d bytes differ, largest difference %d" % (name, severity, differing, total, worst))
        assert worst <= ref.CAP_BYTE and 3 * differing <= allowed, (name, severity, worst, differing, total)


def test_abi_additions():
    header = open(os.path.join(ROOT, "include", "pod_mi355x.h")).read()
    assert re.search(r"^#define POD_ABI_VERSION 18$", header, re.M) and hip.POD_ABI_VERSION == 18
    for sym in ("pod_corrupt_scratch_bytes", "pod_corrupt_frame_u8"):
        assert sym in hip.EXPORTS and re.search(r"\b%s\(" % sym, header)
    assert "typedef struct PodCorruption" in header and "k35_corrupt_u8.hip" in build.SOURCES
    if os.path.exists(hip.library_path()):
        out = subprocess.run(["nm", "-D", "--defined-only", hip.library_path()], capture_output=True, text=True, check=True).stdout
        names = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert {"pod_corrupt_scratch_bytes", "pod_corrupt_frame_u8"} <= names
    import ctypes
    assert ctypes.sizeof(hip.PodCorruption) == 48 and hip.PodCorruption.taps.offset == 24 and hip.PodCorruption.key.offset == 40


REFUSED = (
    (["--corruption", "contrast"], "together"),
    (["--severity", "3"], "together"),
    (["--corruption", "fog", "--severity", "3", "--coco-json", "x.json"], "unknown corruption"),
    (["--corruption", "contrast", "--severity", "6", "--coco-json", "x.json"], "severity"),
    (["--corruption", "contrast", "--severity", "3"], "--coco-json"),
    (["--corruption", "contrast", "--severity", "3", "--coco-json", "x.json", "--ensemble-per-gpu"], "--ensemble-per-gpu"),
    (["--corruption", "contrast", "--severity", "3", "--coco-json", "x.json", "--vis-dir", "v"], "--vis-dir"),
    (["--corruption", "contrast", "--severity", "3", "--coco-json", "x.json", "--eval-only"], "--eval-only"),
    (["--corruption", "contrast", "--severity", "3", "--coco-json", "x.json", "--eval-only", "--inference-config", "a.yaml", "b.yaml"], "--eval-only"),
)


@pytest.mark.parametrize("argv,word", REFUSED, ids=[" ".join(a[:6]) + " " + w for a, w in REFUSED])
def test_apply_net_refuses(argv, word, monkeypatch):
    import torch

    def no_device(*a, **k):
        raise AssertionError("a refusal must come before any device is touched")
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.setattr(apply_net, "_start_rank", no_device)
    with pytest.raises(SystemExit) as e:
        apply_net.main(argv)
    assert word in str(e.value), str(e.value)


def test_inference_output_dir_suffix():
    plain = apply_net.inference_output_dir("/out", "bdd_val", "configs/Inference/standard_nms.yaml")
    assert plain == os.path.join("/out", "inference", "bdd_val", "standard_nms")
    assert apply_net.inference_output_dir("/out", "bdd_val", "configs/Inference/standard_nms.yaml", "") == plain
    assert apply_net.inference_output_dir("/out", "kitti_val", "a/bayes_od.yaml", "defocus_blur_5") == \
        os.path.join("/out", "inference", "kitti_val_defocus_blur_5", "bayes_od")
