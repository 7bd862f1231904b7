"""The referee of the solver step (K29): the expressions of include/pod_mi355x.h's K29 block in numpy fp64 over a flat arena.

An arena is one 1-D array per role (w, m, g, s) plus `owner`, the tensor every element belongs to (-1: no tensor, e.g. a sentinel).  A tensor
without a gradient (has_grad[t] False) is in no norm and is not stepped.  test_solver_section_cpu.py pins this file to torch.optim.SGD and
torch's clipping utilities in fp64; the GPU tests then hold the kernels against it."""
import numpy as np

CLIP_TYPES = ("off", "value", "norm", "full_model")


def clip_coef(sumsq, clip_value):
    """torch's clip_grad_norm_: max_norm / (norm + 1e-6), clamped to 1 from above (a NaN stays a NaN)."""
    c = np.float64(clip_value) / (np.sqrt(np.asarray(sumsq, dtype=np.float64)) + 1e-6)
    return np.where(c > 1.0, 1.0, c)


def step(w, m, g, s, owner, has_grad, group, lr, wd, mu, nesterov=False, clip_type="off", clip_value=1.0, a0_fp32=False):
    """One step.  w, m, g, s: (E,) float64 (s: 1 where no scale applies); owner: (E,) int, -1 outside every tensor; has_grad: (T,) bool;
    group: (T,) int; lr, wd: one float per group; a0_fp32: a0 = s g is rounded to fp32 before anything else reads it (the kernels' a0 --
    the norm is of exactly the gradient that is stepped).  Returns a dict: w, m (stepped where live, unchanged elsewhere), live (E,),
    a0, a, g1 (= g'), d, sumsq (T,), total, coef (T,), coef_all."""
    assert clip_type in CLIP_TYPES
    w, m, g, s = (np.asarray(x, dtype=np.float64) for x in (w, m, g, s))
    owner, has_grad, group = np.asarray(owner, dtype=np.int64), np.asarray(has_grad, dtype=bool), np.asarray(group, dtype=np.int64)
    T = len(has_grad)
    live = (owner >= 0) & has_grad[np.clip(owner, 0, None)]
    own = owner[live]
    a0 = s[live] * g[live]
    if a0_fp32:
        with np.errstate(over="ignore"):
            a0 = a0.astype(np.float32).astype(np.float64)
    sumsq = np.bincount(own, weights=a0 * a0, minlength=T).astype(np.float64)
    total = float(sumsq.sum())
    coef = np.where(has_grad, clip_coef(sumsq, clip_value), 1.0)
    coef_all = float(clip_coef(total, clip_value))
    v = np.float64(clip_value)
    if clip_type == "value":
        a = np.where(a0 < -v, -v, a0)
        a = np.where(a > v, v, a)
    elif clip_type == "norm":
        a = coef[own] * a0
    elif clip_type == "full_model":
        a = coef_all * a0
    else:
        a = a0
    lr_e, wd_e = np.asarray(lr, dtype=np.float64)[group[own]], np.asarray(wd, dtype=np.float64)[group[own]]
    g1 = a + wd_e * w[live]
    m1 = mu * m[live] + g1
    d = g1 + mu * m1 if nesterov else m1
    w1 = w[live] - lr_e * d
    w_out, m_out = w.copy(), m.copy()
    w_out[live], m_out[live] = w1, m1
    return {"w": w_out, "m": m_out, "live": live, "a0": a0, "a": a, "g1": g1, "d": d, "sumsq": sumsq, "total": total, "coef": coef,
            "coef_all": coef_all, "lr": lr_e, "wd": wd_e}
