"""Shared by the head-backward tests: the fp64 / fp32 CPU references of K22 and the issue's two-sided tolerance."""
import torch

BAR = 1e-4            # (a) the project's parity bar, read against the tensor's abs-max
MARGIN = 4.0          # (b) e_hip <= MARGIN * e_f32: torch's own fp32 evaluation of the same gradient on the CPU


def rel_err(g: torch.Tensor, g64: torch.Tensor) -> float:
    return float((g.detach().cpu().double() - g64).abs().max() / g64.abs().max())


def check(name: str, g_hip: torch.Tensor, g32: torch.Tensor, g64: torch.Tensor) -> None:
    """Prints e_hip, e_f32 and their ratio, then asserts (a) and (b)."""
    e_hip, e_f32 = rel_err(g_hip, g64), rel_err(g32, g64)
    print("HB_ERR %-44s e_hip %.3e  e_f32 %.3e  ratio %.2f" % (name, e_hip, e_f32, e_hip / e_f32 if e_f32 > 0 else (0.0 if e_hip == 0 else float("inf"))))
    assert e_hip <= BAR, (name, e_hip)
    assert e_hip <= MARGIN * e_f32, (name, e_hip, e_f32)


def ref_wgrad(x: torch.Tensor, dy: torch.Tensor, levels, copies: int, K: int, dtype):
    """x (pixels, C), dy (pixels, Kpad) channels-last on the CPU, level-major -> (dW (K, C, 3, 3), db (K,)) evaluated in `dtype`."""
    C = x.shape[1]
    dW = torch.zeros((K, C, 3, 3), dtype=dtype)
    off = 0
    for h, w in levels:
        n = copies * h * w
        xl = x[off:off + n].view(copies, h, w, C).permute(0, 3, 1, 2).to(dtype).contiguous()
        gl = dy[off:off + n, :K].reshape(copies, h, w, K).permute(0, 3, 1, 2).to(dtype).contiguous()
        dW += torch.nn.grad.conv2d_weight(xl, (K, C, 3, 3), gl, padding=1)
        off += n
    return dW, dy[:, :K].to(dtype).sum(0)


class Checker:
    """`check` for a list of tensors: every figure is printed before anything is asserted, so one miss does not hide the others."""

    def __init__(self):
        self.missed = []

    def add(self, name: str, g_hip: torch.Tensor, g32: torch.Tensor, g64: torch.Tensor) -> None:
        try:
            check(name, g_hip, g32, g64)
        except AssertionError as e:
            self.missed.append(e.args[0])

    def finish(self) -> None:
        assert not self.missed, self.missed
