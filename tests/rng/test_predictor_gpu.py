"""The dropout masks of the model-side kernels against the rule csrc/pod_device.h writes down, restated on the host
(tests/rng/rng_ref.py: dropout_keep): bit for bit, for pod_relu_dropout, pod_bias_act (its three layouts), pod_bias_act_to_nchw,
pod_expand_dropout and the store pass of pod_wino_conv3x3_split with replicas and an epoch word.

The inputs are all ones (or a convolution's known positive output), so an output element is non-zero exactly where the mask keeps it and
a survivor is fp32(value * 1 / (1 - p)): every comparison is torch.equal, and the number of survivors is the host's count.

The module shares its name with tests/test_predictor_gpu.py (where the fused ReLU + dropout has lived) so that the GPU run order in
tests/conftest.py (GPU_ORDER, keyed by module name) gives it a place."""
import numpy as np
import pytest
import torch

from pod_compare_amd import hip
from pod_compare_amd.wino import WinoConv, block_table, level_pixel_offsets
from tests.rng import rng_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x0D50ED
SIZES = [1, 3, 4, 5] + [8 * 257 + r for r in range(8)]              # no whole group; one; a tail; 514 / 515 groups (even / odd) with every tail
PS = [0.0, 0.1, 0.2, 0.5]
OFFSETS = [0, 1 << 34, (1 << 33) + 12345]                            # the head's blocks; a counter whose high word is set


def masked_ones(keep, p):
    """What a kernel must leave of an all-ones tensor: fp32 1 / (1 - p) where kept, 0 elsewhere."""
    return torch.from_numpy(np.where(keep, rr.dropout_scale(p), np.float32(0.0)).astype(np.float32))


def check(got, keep, p):
    got = got.cpu().reshape(keep.shape)
    assert torch.equal(got, masked_ones(keep, p))
    assert int((got != 0).sum()) == int(keep.sum())               # the host's count, no statistical tolerance


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("n", SIZES)
def test_relu_dropout_mask_equals_the_host_rule(n, p):
    lib = hip.load()
    for off in OFFSETS:
        x = torch.ones(n, device=DEV)
        hip.check(lib.pod_relu_dropout(x.data_ptr(), n, p, SEED, off, hip.current_stream()), "pod_relu_dropout")
        check(x, rr.dropout_keep(SEED, off, n, p, "inplace"), p)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("n", SIZES)
def test_bias_act_mask_equals_the_host_rule(n, p):
    """Zero bias on the same elements, through each of the kernel's layouts: planes with H W % 4 == 0, channels-last with C % 4 == 0,
    and the per-element form; the mask is keyed by the flat index whatever the layout."""
    lib = hip.load()
    shapes = [(1, n)] + ([(n, 1)] if n % 4 == 0 else []) + ([(3, n // 3)] if n % 3 == 0 and n // 3 % 4 else [])
    assert n % 4 or len(shapes) >= 2
    for C, HW in shapes:
        bias = torch.zeros(C, device=DEV)
        for off in OFFSETS:
            x = torch.ones(n, device=DEV)
            hip.check(lib.pod_bias_act(x.data_ptr(), bias.data_ptr(), None, None, n, C, HW, 1, p, SEED, off, hip.current_stream()), "pod_bias_act")
            check(x, rr.dropout_keep(SEED, off, n, p, "inplace"), p)


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_bias_act_to_nchw_mask_is_keyed_by_the_nchw_index(p):
    """Channels-last in, planes out: the float4 group of the mask is the one of the NCHW result.  Proof: the output, read in its own flat
    order, IS the host mask of a flat tensor of N C H W floats -- and is not that mask laid over the channels-last order of the input.
    Two images, 12 channels (a partial channel tile), 68 cells (two cell tiles, the second partial)."""
    N, C, HW, off = 2, 12, 68, 7 << 34
    src = torch.ones(N, HW, C, device=DEV)
    dst = torch.full((N, C, HW), float("nan"), device=DEV)
    bias = torch.zeros(C, device=DEV)
    hip.check(hip.load().pod_bias_act_to_nchw(src.data_ptr(), dst.data_ptr(), bias.data_ptr(), N, C, HW, 1, p, SEED, off, hip.current_stream()),
              "pod_bias_act_to_nchw")
    keep = rr.dropout_keep(SEED, off, N * C * HW, p, "inplace")
    check(dst, keep, p)
    as_if_channels_last = keep.reshape(N, HW, C).transpose(0, 2, 1)
    assert not np.array_equal(as_if_channels_last, keep.reshape(N, C, HW))
    assert not torch.equal(dst.cpu(), masked_ones(as_if_channels_last, p))


EPOCHS = [None, 0, 1, (1 << 40) + 7]


@pytest.mark.parametrize("epoch", EPOCHS, ids=["no-epoch", "epoch-0", "epoch-1", "epoch-2^40+7"])
@pytest.mark.parametrize("copies", [1, 3])
def test_expand_dropout_mask_equals_the_host_rule(copies, epoch):
    """Replicas: counter word 2, group index copy * n4 + g -- n4 = 515 is odd, so copy 1 starts in the second half of a Philox call --
    and the epoch word folded into the key (a device word: 0 is the plain seed)."""
    lib = hip.load()
    word = None if epoch is None else torch.tensor([epoch], dtype=torch.int64, device=DEV)
    for n, p, off in ((8 * 257 + 4, 0.2, 1 << 34), (8, 0.5, 0), (4, 0.1, (1 << 33) + 12345), (8 * 257, 0.0, 0)):
        src = torch.ones(n, device=DEV)
        dst = torch.full((copies, n), float("nan"), device=DEV)
        hip.check(lib.pod_expand_dropout(src.data_ptr(), dst.data_ptr(), n, copies, p, SEED, off, hip.ptr(word), hip.current_stream()), "pod_expand_dropout")
        check(dst, rr.dropout_keep(SEED, off, n, p, "replicas", copies=copies, epoch=epoch), p)
    if epoch:
        assert not np.array_equal(rr.dropout_keep(SEED, 0, 8 * 257, 0.2, "replicas", copies=copies, epoch=epoch),
                                  rr.dropout_keep(SEED, 0, 8 * 257, 0.2, "replicas", copies=copies))


@pytest.mark.parametrize("epoch", [None, (1 << 40) + 7], ids=["no-epoch", "epoch-2^40+7"])
def test_store_pass_masks_with_an_epoch_word_equal_the_host_rule(epoch):
    """One pod_wino_conv3x3_split launch per form.  Replicas: three masked copies of each level's image, keyed by the element's index in the
    whole buffer with counter word 2 (= pod_expand_dropout per level at offset + first float of the level / 8).  In place: counter word 0.
    The bias (+12, eight standard deviations of the convolution's sum) keeps every output positive, so the observed survivors are the mask's."""
    levels, p, off, C, K, reps = [(6, 11), (3, 5), (1, 1)], 0.25, 9 << 34, 16, 64, 3
    g = torch.Generator(device=DEV).manual_seed(11)
    w = torch.randn(K, C, 3, 3, device=DEV, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.full((K,), 12.0, device=DEV)
    src = torch.cat([torch.randn(h * wd, C, device=DEV, generator=g) for h, wd in levels]).contiguous()
    word = None if epoch is None else torch.tensor([epoch], dtype=torch.int64, device=DEV)
    conv = WinoConv(w, b, split=True)
    off1, offn = level_pixel_offsets(levels, 1), level_pixel_offsets(levels, reps)
    y = conv(src, torch.empty(src.shape[0], K, device=DEV), block_table(levels, 1, DEV), relu=True).cpu()
    assert float(y.min()) > 0.0
    scale = torch.tensor(rr.dropout_scale(p))
    # ---- the replica form
    fused = torch.full((offn[-1], K), float("nan"), device=DEV)
    conv.replicas(src, fused, block_table(levels, 1, DEV, out_copies=reps), reps, relu=True, dropout_p=p, seed=SEED, offset=off, epoch=word)
    fused = fused.cpu()
    for i, (h, wd) in enumerate(levels):
        n = h * wd * K
        keep = torch.from_numpy(rr.dropout_keep(SEED, rr.level_offset(off, offn[i], K), n, p, "replicas", copies=reps, epoch=epoch))
        whole = rr.dropout_fields(off, offn[-1] * K, "replicas")[0]                              # the same counters, read off the whole buffer's index
        assert int(whole[0, offn[i] * K]) == rr.level_offset(off, offn[i], K)
        got = fused[offn[i]:offn[i + 1]].reshape(reps, n)
        yl = y[off1[i]:off1[i + 1]].reshape(1, n)
        assert torch.equal(got, torch.where(keep, yl * scale, torch.zeros(()))), i
        assert int((got != 0).sum()) == int(keep.sum())
    # ---- in place (one image per level)
    masked = conv(src, torch.full((src.shape[0], K), float("nan"), device=DEV), block_table(levels, 1, DEV), relu=True, dropout_p=p, seed=SEED,
                  offset=off, epoch=word).cpu()
    keep = torch.from_numpy(rr.dropout_keep(SEED, off, src.shape[0] * K, p, "inplace", epoch=epoch)).reshape(-1, K)
    assert torch.equal(masked, torch.where(keep, y * scale, torch.zeros(())))
    assert int((masked != 0).sum()) == int(keep.sum())
