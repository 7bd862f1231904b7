"""GPU box: compare two builds of the library on the model-side element-wise kernels (k8_model_ops.hip's seven entry points and
pod_reduce_partials), bit for bit and by launch time:

    POD_MI355X_LIB=<lib> python tools/model_ops_ab.py [--time]

Hashes (always): one sha256 per case over everything the case writes (outputs and abs-max records), on seeded inputs that hold
-0.0 among the normals.  Two builds that print the same table computed the same bits.  Cases: pod_bias_act in its three layouts
(NCHW planes, NHWC, per-element channel) x {no operand, bias, bias + residual, bias + residual + res_bias, residual} x p in {0, 0.3},
ReLU on and off, the per-element layout with and without the n % 4 tail; pod_relu_dropout with a tail; pod_expand_dropout with and
without an epoch word; pod_bias_act_to_nchw / _to_nhwc on full and ragged tiles (to_nhwc also with H*W % 4 != 0); pod_wino_reduce
with K < Kpad for H*W % 4 both ways, with and without a record; pod_reduce_partials; pod_absmax with a tail.
--time: HIP events around single launches at the shapes of the benchmark frame (p3 trunk activation: 16128 cells x 256 channels x
19 copies; res4 / res5 planes for the reduces), 100 launches after 10 of warm-up, five repeats: median per repeat, then their
median and range."""
import hashlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pod_compare_amd import hip  # noqa: E402

RECORD = 512      # floats of an abs-max record (include/pod_mi355x.h: POD_AMAX_FLOATS)


def sha(tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def row(name, tensors):
    print("hash | %-64s | %s" % (name, sha(tensors)), flush=True)


def call(name, *args):
    hip.check(getattr(hip.load(), name)(*args, hip.current_stream()), name)


def randn(g, *shape):
    x = torch.randn(*shape, device="cuda", generator=g)
    x.view(-1)[::7] = -0.0
    return x


def hash_cases():
    g = torch.Generator(device="cuda").manual_seed(8)
    P = hip.ptr
    operands = (("plain", 0, 0, 0), ("bias", 1, 0, 0), ("bias+res", 1, 1, 0), ("bias+res+res_bias", 1, 1, 1), ("res", 0, 1, 0))
    shapes = (("planes", (3, 16, 12, 20)), ("nhwc", (700, 8, 1, 1)), ("per-element", (4, 7, 6, 11)), ("per-element, tail 3", (3, 7, 5, 11)),
              ("per-element, one thread's tail", (1, 5, 3, 3)))
    for layout, shape in shapes:
        x, r = randn(g, *shape), randn(g, *shape)
        b, rb = randn(g, shape[1]), randn(g, shape[1])
        C, HW = shape[1], shape[2] * shape[3]
        for tag, ub, ur, urb in operands:
            for p in (0.0, 0.3):
                outs = []
                for relu in (1, 0):
                    y = x.clone()
                    call("pod_bias_act", y.data_ptr(), P(b if ub else None), P(r if ur else None), P(rb if urb else None), y.numel(), C, HW, relu, p, 99, 5 << 34)
                    outs.append(y)
                row("pod_bias_act %s %s %s p=%.1f" % (layout, shape, tag, p), outs)
    x = randn(g, 11523)
    for p in (0.0, 0.3):
        y = x.clone()
        call("pod_relu_dropout", y.data_ptr(), y.numel(), p, 1234, 1 << 34)
        row("pod_relu_dropout n=11523 (tail 3) p=%.1f" % p, [y])
    y = x[:2].clone()
    call("pod_relu_dropout", y.data_ptr(), 2, 0.3, 1234, 1 << 34)
    row("pod_relu_dropout n=2 (tail only) p=0.3", [y])
    src = randn(g, 11520)
    for name, epoch in (("no epoch", None), ("epoch word", torch.tensor([5], dtype=torch.int64, device="cuda"))):
        dst = torch.full((3, 11520), float("nan"), device="cuda")
        call("pod_expand_dropout", src.data_ptr(), dst.data_ptr(), src.numel(), 3, 0.3, 5, 3 << 34, P(epoch))
        row("pod_expand_dropout n=11520 copies=3 %s" % name, [dst])
    for shape in ((2, 64, 8, 8), (2, 68, 9, 28), (1, 132, 7, 9)):
        N, C, H, W = shape
        nchw, b = randn(g, *shape), randn(g, C)
        nhwc = nchw.permute(0, 2, 3, 1).contiguous()
        for ub in (1, 0):
            if (H * W) % 4 == 0:
                outs = []
                for relu, p in ((1, 0.0), (0, 0.0), (1, 0.3), (0, 0.3)):
                    out = torch.full(shape, float("nan"), device="cuda")
                    call("pod_bias_act_to_nchw", nhwc.data_ptr(), out.data_ptr(), P(b if ub else None), N, C, H * W, relu, p, 7, 2 << 34)
                    outs.append(out)
                row("pod_bias_act_to_nchw %s bias=%d" % (shape, ub), outs)
            outs = []
            for relu in (1, 0):
                out = torch.full((N, H * W, C), float("nan"), device="cuda")
                call("pod_bias_act_to_nhwc", nchw.data_ptr(), out.data_ptr(), P(b if ub else None), N, C, H * W, relu)
                outs.append(out)
            row("pod_bias_act_to_nhwc %s bias=%d" % (shape, ub), outs)
    Kpad, K, splits = 128, 100, 3
    for hw in (252, 63):
        part = randn(g, splits, hw, Kpad)
        bias = torch.cat([randn(g, K), torch.zeros(Kpad - K, device="cuda")])
        for ub, relu, record in ((1, 1, 0), (1, 1, 1), (0, 0, 1), (1, 0, 0)):
            planes = torch.full((K, hw), float("nan"), device="cuda")
            rec = torch.zeros(RECORD, device="cuda")
            call("pod_wino_reduce", part.data_ptr(), splits, hw * Kpad, P(bias if ub else None), planes.data_ptr(), hw, Kpad, K, relu, P(rec if record else None))
            row("pod_wino_reduce HW=%d Kpad=128 K=100 splits=3 bias=%d relu=%d record=%d" % (hw, ub, relu, record), [planes, rec])
        one = torch.full((K, hw), float("nan"), device="cuda")
        call("pod_wino_reduce", part.data_ptr(), 1, 0, P(bias), one.data_ptr(), hw, Kpad, K, 1, None)
        row("pod_wino_reduce HW=%d Kpad=128 K=100 splits=1" % hw, [one])
    n, cout = 252 * 64, 64
    part, bias, res = randn(g, 3, n), randn(g, cout), randn(g, n)
    for ub, ur, relu, record in ((1, 1, 1, 1), (0, 0, 0, 0), (1, 0, 1, 0), (0, 1, 0, 1)):
        y = torch.full((n,), float("nan"), device="cuda")
        rec = torch.zeros(RECORD, device="cuda")
        call("pod_reduce_partials", part.data_ptr(), 3, n, P(bias if ub else None), P(res if ur else None), y.data_ptr(), n, cout, relu, P(rec if record else None))
        row("pod_reduce_partials n=252x64 splits=3 bias=%d res=%d relu=%d record=%d" % (ub, ur, relu, record), [y, rec])
    for n in (11523, 3):
        rec = torch.zeros(RECORD, device="cuda")
        call("pod_absmax", x.data_ptr(), n, rec.data_ptr())
        row("pod_absmax n=%d (tail 3)" % n, [rec])


def launch_times(name, launch, reset=None, repeats=5, warm=10, n=100):
    meds = []
    for _ in range(repeats):
        if reset is not None:
            reset()
        for _ in range(warm):
            launch()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in ev:
            a.record()
            launch()
            b.record()
        torch.cuda.synchronize()
        meds.append(statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev))
    print("time | %-58s | median %8.2f us | repeats %8.2f .. %8.2f" % (name, statistics.median(meds), min(meds), max(meds)), flush=True)


def time_cases():
    g = torch.Generator(device="cuda").manual_seed(9)
    cells, C, copies, p = 16128, 256, 19, 0.3
    P = hip.ptr
    fresh = torch.randn(copies, C, cells, device="cuda", generator=g)
    x, out = fresh.clone(), torch.empty_like(fresh)
    b = torch.randn(C, device="cuda", generator=g)
    tag = "%d x %d x %d" % (copies, C, cells)
    reset = lambda: x.copy_(fresh)           # (the in-place kernels scale what they keep: start every repeat from the same values)
    launch_times("pod_relu_dropout %s" % tag, lambda: call("pod_relu_dropout", x.data_ptr(), x.numel(), p, 7, 1 << 34), reset)
    launch_times("pod_bias_act planes, bias %s" % tag, lambda: call("pod_bias_act", x.data_ptr(), b.data_ptr(), None, None, x.numel(), C, cells, 1, p, 7, 1 << 34), reset)
    launch_times("pod_bias_act planes, no operand %s" % tag, lambda: call("pod_bias_act", x.data_ptr(), None, None, None, x.numel(), C, cells, 1, p, 7, 1 << 34), reset)
    launch_times("pod_bias_act nhwc, bias %s" % tag, lambda: call("pod_bias_act", x.data_ptr(), b.data_ptr(), None, None, x.numel(), C, 1, 1, p, 7, 1 << 34), reset)
    launch_times("pod_bias_act per-element, bias %d x %d x 16127" % (copies, C),
                 lambda: call("pod_bias_act", x.data_ptr(), b.data_ptr(), None, None, copies * C * 16127, C, 16127, 1, p, 7, 1 << 34), reset)
    launch_times("pod_expand_dropout %d x %d, %d copies" % (C, cells, copies),
                 lambda: call("pod_expand_dropout", fresh.data_ptr(), out.data_ptr(), C * cells, copies, p, 7, 1 << 34, None))
    launch_times("pod_bias_act_to_nchw %s" % tag, lambda: call("pod_bias_act_to_nchw", fresh.data_ptr(), out.data_ptr(), b.data_ptr(), copies, C, cells, 1, p, 7, 1 << 34))
    launch_times("pod_bias_act_to_nhwc %s" % tag, lambda: call("pod_bias_act_to_nhwc", fresh.data_ptr(), out.data_ptr(), b.data_ptr(), copies, C, cells, 1))
    rec = torch.zeros(RECORD, device="cuda")
    launch_times("pod_absmax %s" % tag, lambda: call("pod_absmax", fresh.data_ptr(), fresh.numel(), rec.data_ptr()))
    for name, hw, K, s in (("res4", 48 * 84, 256, 2), ("res5", 24 * 42, 512, 4)):        # the splits wino.py picks on a 768 x 1344 frame
        part = torch.randn(s, hw, K, device="cuda", generator=g)
        bias, y = torch.randn(K, device="cuda", generator=g), torch.empty(K * hw, device="cuda")
        launch_times("pod_wino_reduce %s: HW=%d K=%d splits=%d" % (name, hw, K, s),
                     lambda: call("pod_wino_reduce", part.data_ptr(), s, hw * K, bias.data_ptr(), y.data_ptr(), hw, K, K, 1, None))
        launch_times("pod_wino_reduce %s, record" % name,
                     lambda: call("pod_wino_reduce", part.data_ptr(), s, hw * K, bias.data_ptr(), y.data_ptr(), hw, K, K, 1, rec.data_ptr()))
        launch_times("pod_reduce_partials %s: n=%dx%d splits=%d" % (name, hw, K, s),
                     lambda: call("pod_reduce_partials", part.data_ptr(), s, hw * K, bias.data_ptr(), None, y.data_ptr(), hw * K, K, 1, rec.data_ptr()))


def main():
    print("library:", hip.library_path())
    hash_cases()
    if "--time" in sys.argv:
        time_cases()


if __name__ == "__main__":
    main()
