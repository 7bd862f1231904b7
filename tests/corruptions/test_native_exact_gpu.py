"""K35 (csrc/k35_corrupt_u8.hip) on the GPU against the fp64 referee of corrupt_ref.py: the four integer / fp64 kinds to the byte, the four
fp32 kinds inside the cap that test_corruptions_cpu.py shows fp32 alone meets with room to spare; flat frames, determinism, one frame at
the real size, the refusals.  Every launch writes between 128 guard bytes on either side, checked afterwards.

The module shares its name with tests/test_native_exact_gpu.py so that the GPU run order of tests/conftest.py (GPU_ORDER, keyed by
module name) places it among the kernels' own arithmetic tests."""
import ctypes

import numpy as np
import pytest
import torch

from pod_compare_amd import corruptions, hip
from tests.corruptions import corrupt_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 128


def _on_device(f, pad):
    """f (h, w, 3) uint8 numpy -> device view with rows `pad` bytes apart from one another."""
    h, w = f.shape[:2]
    if not pad:
        return torch.from_numpy(f).to(DEV)
    buf = torch.full((h, 3 * w + pad), 201, dtype=torch.uint8, device=DEV)
    buf[:, :3 * w] = torch.from_numpy(f).to(DEV).reshape(h, 3 * w)
    v = buf[:, :3 * w].unflatten(1, (w, 3))
    assert v.stride() == (3 * w + pad, 3, 1)
    return v


def _record(name, severity, key, radius=None):
    p = corruptions.parameters(name, severity)
    r, taps = corruptions.filter_table(name, severity)
    t = None if taps is None else torch.from_numpy(taps).to(DEV)
    pair = p if isinstance(p, tuple) else (p, 0.0)
    rec = hip.PodCorruption(kind=corruptions.KINDS[name], radius=r if radius is None else radius, p0=float(pair[0]), p1=float(pair[1]),
                            taps=None if t is None else t.data_ptr(), impulse_threshold=corruptions.impulse_threshold(p) if name == "impulse_noise" else 0,
                            reserved=0, key=key)
    return rec, t


def _launch(src, name, severity, key, expect=0, radius=None, short_scratch=False, dst=None):
    """pod_corrupt_frame_u8 on src (h, w, 3) uint8 device tensor whose rows may be padded -> (return code, output, whole guarded buffer)."""
    lib = hip.load()
    h, w = src.shape[:2]
    rec, taps = _record(name, severity, key, radius)
    need = int(lib.pod_corrupt_scratch_bytes(rec.kind, h, w))
    have = need - 8 if short_scratch else need
    scratch = torch.zeros((max(need, 8) // 8 + 1,), dtype=torch.int64, device=DEV)
    buf = torch.full((3 * h * w + 2 * GUARD,), 77, dtype=torch.uint8, device=DEV)
    out = buf[GUARD:GUARD + 3 * h * w].view(h, w, 3)
    rc = lib.pod_corrupt_frame_u8(src.data_ptr(), h, w, src.stride(0), (out if dst is None else dst).data_ptr(), 3 * w, ctypes.byref(rec),
                                  scratch.data_ptr() if need else None, have, hip.current_stream())
    torch.cuda.synchronize()
    assert rc == expect, (name, severity, rc)
    assert bool((buf[:GUARD] == 77).all()) and bool((buf[-GUARD:] == 77).all()), "guard bytes written"
    del taps
    return rc, out, buf


def _gpu(name, severity, index):
    f = ref.frame(ref.FRAMES[index])
    _, out, _ = _launch(_on_device(f, 13 if ref.FRAMES[index] == (48, 80) else 0), name, severity, ref.key_of(ref.SEED, index))
    return out.cpu()


def test_scratch_sizes():
    lib = hip.load()
    assert lib.pod_corrupt_scratch_bytes(hip.POD_CORRUPT_GAUSSIAN_BLUR, 37, 53) == 37 * 53 * 12
    assert lib.pod_corrupt_scratch_bytes(hip.POD_CORRUPT_CONTRAST, 130, 70) == 32 + 12 * 3 and lib.pod_corrupt_scratch_bytes(hip.POD_CORRUPT_CONTRAST, 64, 64) == 44
    for kind in (hip.POD_CORRUPT_GAUSSIAN_NOISE, hip.POD_CORRUPT_DEFOCUS_BLUR, hip.POD_CORRUPT_BRIGHTNESS, 99):
        assert lib.pod_corrupt_scratch_bytes(kind, 37, 53) == 0
    assert lib.pod_corrupt_scratch_bytes(hip.POD_CORRUPT_CONTRAST, 0, 5) == 0 and lib.pod_corrupt_scratch_bytes(hip.POD_CORRUPT_CONTRAST, 5, hip.POD_RESIZE_MAX_SIDE + 1) == 0


@pytest.mark.parametrize("severity", ref.SEVERITIES)
@pytest.mark.parametrize("name", ref.EXACT)
def test_exact_kinds_equal_the_reference(name, severity):
    for i, hw in enumerate(ref.FRAMES):
        got, want = _gpu(name, severity, i), torch.from_numpy(ref.reference(name, severity, i).copy())
        assert torch.equal(got, want), (name, severity, hw, int((got != want).sum()))
    if name != "impulse_noise":                 # saturation 0, value 0 and 1, grey, the six sextants' corners
        edge = np.array([[[0, 0, 0], [255, 255, 255], [128, 128, 128], [255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255],
                          [255, 0, 255], [255, 0, 1], [1, 0, 255], [254, 255, 255], [1, 1, 0]]], dtype=np.uint8)
        _, out, _ = _launch(_on_device(edge, 0), name, severity, 0)
        assert torch.equal(out.cpu(), torch.from_numpy(ref.corrupt(edge, name, severity)))


@pytest.mark.parametrize("severity", ref.SEVERITIES)
@pytest.mark.parametrize("name", ref.CAPPED)
def test_capped_kinds_stay_inside_the_cap(name, severity):
    pairs = [(_gpu(name, severity, i).numpy(), ref.reference(name, severity, i)) for i in range(len(ref.FRAMES))]
    worst, differing, total, allowed = ref.within_cap(pairs)
    print("%s severity %d: %d of %d bytes differ (allowed %d), largest difference %d" % (name, severity, differing, total, allowed, worst))
    assert worst <= ref.CAP_BYTE and differing <= allowed, (name, severity, worst, differing, total)


@pytest.mark.parametrize("name", ("gaussian_blur", "defocus_blur"))
def test_flat_frames_stay_flat(name):
    for value in (100, 255):
        for hw in ((37, 53), (130, 70)):
            src = torch.full(hw + (3,), value, dtype=torch.uint8, device=DEV)
            for severity in (1, 2, 3, 4, 5):
                _, out, _ = _launch(src, name, severity, 0)
                assert bool((out == value).all()), (name, value, hw, severity)


def test_determinism_and_keys():
    f = ref.frame((130, 70))
    src = _on_device(f, 0)
    for name in ("gaussian_noise", "speckle_noise", "impulse_noise"):
        key = ref.key_of(ref.SEED, 3)
        a = corruptions.corrupt_frame_u8(src, name, 3, key)
        b = corruptions.corrupt_frame_u8(src, name, 3, key)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            c = corruptions.corrupt_frame_u8(src, name, 3, key)
        s.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c), name
        other = corruptions.corrupt_frame_u8(src, name, 3, ref.key_of(ref.SEED, 4))
        assert not torch.equal(a, other), name
        assert not torch.equal(a, corruptions.corrupt_frame_u8(src, name, 3, ref.key_of(ref.SEED + 1, 3))), name
    for name in ("brightness", "gaussian_blur"):            # the key is not read
        assert torch.equal(corruptions.corrupt_frame_u8(src, name, 3, 1), corruptions.corrupt_frame_u8(src, name, 3, 2))
    # the wrapper on a strided view: the bytes of the direct launch
    v = _on_device(ref.frame((48, 80)), 13)
    assert torch.equal(corruptions.corrupt_frame_u8(v, "contrast", 5, 0).cpu(), torch.from_numpy(ref.reference("contrast", 5, 2).copy()))
    with pytest.raises(ValueError):
        corruptions.corrupt_frame_u8(src.permute(2, 0, 1), "contrast", 3, 0)
    with pytest.raises(ValueError):
        corruptions.corrupt_frame_u8(src, "contrast", 0, 0)


@pytest.mark.parametrize("severity", (1, 2, 3, 4, 5))
def test_impulse_share(severity):
    """Flipped elements are Binomial(n, amount); a flip to the byte's own value cannot be seen, so the frame holds neither 0 nor 255."""
    amount = corruptions.parameters("impulse_noise", severity)
    f = np.random.default_rng(11).integers(1, 255, size=(130, 70, 3), dtype=np.uint8)
    _, out, _ = _launch(_on_device(f, 0), "impulse_noise", severity, ref.key_of(ref.SEED, 3))
    out = out.cpu().numpy()
    flipped = out != f
    n = f.size
    assert set(np.unique(out[flipped]).tolist()) <= {0, 255}
    assert abs(int(flipped.sum()) - n * amount) <= 4.0 * np.sqrt(n * amount * (1.0 - amount)), (severity, int(flipped.sum()), n * amount)
    high = int((out[flipped] == 255).sum())
    assert abs(high - 0.5 * flipped.sum()) <= 4.0 * np.sqrt(0.25 * flipped.sum())


@pytest.mark.parametrize("name,severity", (("gaussian_noise", 3), ("gaussian_blur", 5)))
def test_full_size_frame(name, severity):
    f = np.random.default_rng(5).integers(0, 256, size=(720, 1280, 3), dtype=np.uint8)
    key = ref.key_of(ref.SEED, 123456)
    _, out, _ = _launch(_on_device(f, 0), name, severity, key)
    worst, differing, total, allowed = ref.within_cap([(out.cpu().numpy(), ref.corrupt(f, name, severity, key))])
    print("%s severity %d at 720 x 1280: %d of %d bytes differ (allowed %d), largest difference %d" % (name, severity, differing, total, allowed, worst))
    assert worst <= ref.CAP_BYTE and differing <= allowed


def test_refusals_leave_the_output_alone():
    lib = hip.load()
    f = ref.frame((37, 53))
    src = _on_device(f, 0)
    E = -1          # POD_E_INVALID
    for kw in (dict(name="gaussian_blur", short_scratch=True), dict(name="contrast", short_scratch=True), dict(name="defocus_blur", radius=13),
               dict(name="gaussian_blur", radius=25), dict(name="defocus_blur", radius=-1)):
        _, out, buf = _launch(src, kw.pop("name"), 3, 0, expect=E, **kw)
        assert bool((buf == 77).all())
    # overlap: the output inside the input, and the input's last bytes
    whole = torch.from_numpy(f).to(DEV)
    before = whole.clone()
    for dst in (whole, whole.view(-1)[3 * 53 * 36 + 3 * 52:]):
        _launch(whole, "brightness", 3, 0, expect=E, dst=dst)
    assert torch.equal(whole, before)
    # NULL pointers, sides, kind, taps
    rec, taps = _record("gaussian_blur", 3, 0)
    out = torch.full((37, 53, 3), 77, dtype=torch.uint8, device=DEV)
    scratch = torch.zeros((37 * 53 * 12 // 8 + 1,), dtype=torch.int64, device=DEV)
    st = hip.current_stream()

    def call(src_p=src.data_ptr(), h=37, w=53, stride=3 * 53, dst_p=out.data_ptr(), dstride=3 * 53, record=rec, scr=scratch.data_ptr(), n=37 * 53 * 12):
        return lib.pod_corrupt_frame_u8(src_p, h, w, stride, dst_p, dstride, None if record is None else ctypes.byref(record), scr, n, st)
    assert call(src_p=None) == E and call(dst_p=None) == E and call(record=None) == E and call(scr=None) == E and call(scr=scratch.data_ptr() + 4) == E
    assert call(h=0) == E and call(w=0) == E and call(h=hip.POD_RESIZE_MAX_SIDE + 1) == E and call(stride=3 * 53 - 1) == E and call(dstride=3 * 53 - 1) == E
    for kind in (-1, hip.POD_CORRUPT_KINDS):
        bad, _ = _record("gaussian_blur", 3, 0)
        bad.kind = kind
        assert call(record=bad) == E
    for name in ("gaussian_blur", "defocus_blur"):
        bad, _ = _record(name, 3, 0)
        bad.taps = None
        assert call(record=bad) == E
    torch.cuda.synchronize()
    assert bool((out == 77).all())
    assert call() == 0                           # (the same call, nothing wrong with it)
    torch.cuda.synchronize()
    assert not bool((out == 77).all())
    del taps
