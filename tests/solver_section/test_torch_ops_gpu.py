"""pod_sgd_step_solver (K29) on the table tests/optimizer_step builds for K25 -- ~300 descriptors, ~430 k elements: sizes 0, 1, 3, 4, 5, 63,
4095 - 4097, 3 chunks + 3; per_channel 1 - 2048 with channel boundaries inside a float4; every 7th tensor without a gradient; 64 sentinel
floats around every buffer -- against the fp64 referee solver_ref, which test_solver_section_cpu.py pins to torch.

The bounds, u = 2^-24, by counting roundings on the magnitudes of the TERMS (so that cancellation does not tighten them), as
tests/optimizer_step does for K25.  x^ is the referee's value, from the fp32 state the call started from, with lr, wd, mu and clip_value
rounded to fp32 and -- the norm being of exactly the gradient that is stepped -- the norms taken of a0 rounded to fp32.
    K25:      |m' - m^| <= 4 u (|a| + wd |w| + mu |m|)                     (at most three roundings on any term of m')
    clipped by a norm: a = fl(coef32 * a0), coef32 = fl32(c).  Two more roundings on the term a, and c itself differs from the referee's
              c^ by the fp64 arithmetic: the sum of n non-negative squares in any order is within n 2^-53 relative, sqrt, the addition of
              1e-6 and the division add one 2^-53 each.  So the term a gains (2 u + (n + 4) 2^-53) |a|, n the elements of the WHOLE table
              (an upper bound for every tensor's own n): with n = 4.3e5 the fp64 part is 4.8e-11 |a|, 0.04 % of the 2 u = 1.2e-7 beside
              it -- negligible, and in the bound all the same.
    clipped by value: the clamp is exact and does not expand a difference: no more roundings.
              |m' - m^| <= 4 u (|a| + wd |w| + mu |m|) + extra,   extra = (2 u + (n + 4) 2^-53) |a| for norm / full_model, 0 otherwise
    Nesterov: d = fl(g' + fl(mu m')) -- two more roundings on the way to w', each at most u (|a| + wd |w| + mu (|a| + wd |w| + mu |m|)):
              |g' - g^| <= 3 u (|a| + wd |w|) + extra;   |d - d^| <= that + mu (m's bound) + 2 u (|a| + wd |w| + mu (|a| + wd |w| + mu |m|))
              without Nesterov d = m'.
    the step: |w' - w^| <= 2 u |w^| + 2 lr (d's bound)                      (K25's, with d in m's place)
Every live element of every tensor is compared; nothing is filtered.  The grid: pod_sgd_step_solver exposes no cap, so grid independence is
shown on a second table -- the same tensors listed in reverse, a table pod_sgd_chunk_map cuts like any other -- whose chunks land on
other workgroups: under per-tensor clipping every tensor's bits are those of the first table."""
import ctypes

import numpy as np
import pytest
import torch

from pod_compare_amd import hip
from tests.optimizer_step.test_torch_ops_gpu import DEV, MU, SENTINEL, WD, Table
from tests.solver_section import solver_ref

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
CLIP = {"off": 0, "value": 1, "norm": 2, "full_model": 3}
WD_BIAS = 0.0
V = 0.75


class Solver:
    """The group array (a `bias` = a plain tensor of at most 64 elements), the workspace and the calls, for one Table."""

    def __init__(self, tab: Table, two_groups=True):
        self.tab, n = tab, len(tab.specs)
        self.group = [1 if two_groups and pc == 0 and k <= 64 else 0 for k, pc, _ in tab.specs]
        assert not two_groups or 30 <= sum(self.group) < n
        self.group_host = (ctypes.c_uint8 * n)(*self.group)
        self.group_dev = torch.tensor(self.group, dtype=torch.uint8).to(DEV)
        self.n_groups = 2 if two_groups else 1
        self.ws = torch.zeros(int(hip.load().pod_sgd_solver_workspace_bytes(n, tab.n_chunks)), dtype=torch.uint8, device=DEV)
        assert self.ws.numel() >= 32 + 8 * tab.n_chunks + 4 * (n + 1) and self.ws.data_ptr() % 16 == 0

    def record(self, lr, clip="off", nesterov=False, guard=False, v=V, iteration=0, watch=()):
        r = hip.PodSgdSolver()
        r.n_groups, r.nesterov, r.clip_type, r.guard, r.momentum, r.clip_value, r.iteration = self.n_groups, int(nesterov), CLIP[clip], int(guard), MU, v, iteration
        lrs = [lr, 2.5 * lr]
        for g in range(self.n_groups):
            r.lr[g], r.wd[g] = lrs[g], (WD, WD_BIAS)[g]
        for q, t in enumerate(watch):
            r.watch[q] = t.data_ptr()
        return r

    def call(self, rec, table=None, cmap=None, n_chunks=None, group_host=None, group_dev=None):
        tab = self.tab
        hip.check(hip.load().pod_sgd_step_solver(tab.table if table is None else table, tab.table_dev.data_ptr(), len(tab.specs),
                                                 (tab.cmap if cmap is None else cmap).data_ptr(), tab.n_chunks if n_chunks is None else n_chunks,
                                                 self.group_host if group_host is None else group_host,
                                                 (self.group_dev if group_dev is None else group_dev).data_ptr(), ctypes.byref(rec), self.ws.data_ptr(),
                                                 hip.current_stream()), "pod_sgd_step_solver")
        torch.cuda.synchronize()

    def status(self):
        return hip.PodSgdSolverStatus.from_buffer_copy(self.ws[:32].cpu().numpy().tobytes())

    def partial(self):
        return np.frombuffer(self.ws[32:32 + 8 * self.tab.n_chunks].cpu().numpy().tobytes(), dtype=np.float64)

    def coef(self):
        o = 32 + 8 * self.tab.n_chunks
        return np.frombuffer(self.ws[o:o + 4 * (len(self.tab.specs) + 1)].cpu().numpy().tobytes(), dtype=np.float32)

    def reset(self):
        hip.check(hip.load().pod_sgd_solver_reset(self.ws.data_ptr(), hip.current_stream()), "pod_sgd_solver_reset")
        torch.cuda.synchronize()


def referee(tab, sol, w0, m0, rec, clip, nesterov):
    """solver_ref on the arena from the fp32 state (w0, m0: CPU tensors) with the record's fp32 rates; returns it with the bounds."""
    lr = [float(rec.lr[g]) for g in range(sol.n_groups)]
    wd = [float(rec.wd[g]) for g in range(sol.n_groups)]
    mu, v = float(rec.momentum), float(rec.clip_value)
    ref = solver_ref.step(w0.double().numpy(), m0.double().numpy(), tab.g.cpu().double().numpy(), tab.s_elem.double().numpy(), tab.owner.numpy(),
                          tab.has_grad.numpy(), sol.group, lr, wd, mu, nesterov=nesterov, clip_type=clip, clip_value=v, a0_fp32=True)
    live = ref["live"]
    assert np.array_equal(live, tab.live.numpy())
    a, wdw, mum = np.abs(ref["a"]), ref["wd"] * np.abs(w0.double().numpy()[live]), mu * np.abs(m0.double().numpy()[live])
    n_all = int(live.sum())
    extra = (2 * U + (n_all + 4) * 2.0 ** -53) * a if clip in ("norm", "full_model") else 0.0 * a
    ref["bound_m"] = 4 * U * (a + wdw + mum) + extra
    if nesterov:
        bound_g = 3 * U * (a + wdw) + extra
        bound_d = bound_g + mu * ref["bound_m"] + 2 * U * (a + wdw + mu * (a + wdw + mum))
    else:
        bound_d = ref["bound_m"]
    ref["bound_w"] = 2 * U * np.abs(ref["w"][live]) + 2 * ref["lr"] * bound_d
    return ref


def check_against_referee(tab, sol, before, ref, what):
    """Every live element within its bound; everything else -- sentinels, operands, tensors without a gradient -- untouched to the bit;
    the folded filter the single fp32 product w' s.  Returns (worst err_m / bound, worst err_w / bound)."""
    w0, m0, f0 = before
    w1, m1, f1 = tab.w.cpu(), tab.m.cpu(), tab.f.cpu()
    live = tab.live
    dead = ~live
    assert torch.equal(w1[dead], w0[dead]) and torch.equal(m1[dead], m0[dead]), what
    wrote_f = live & tab.is_folded
    assert torch.equal(f1[~wrote_f], f0[~wrote_f]), what
    assert torch.equal(tab.scale.cpu(), tab.scale_host), what
    assert torch.equal(tab.g.cpu()[~tab.inside], torch.full((int((~tab.inside).sum()),), SENTINEL)), what
    err_m = np.abs(m1[live].double().numpy() - ref["m"][ref["live"]])
    err_w = np.abs(w1[live].double().numpy() - ref["w"][ref["live"]])
    ok = ref["bound_m"] > 0
    worst = float((err_m[ok] / ref["bound_m"][ok]).max()), float((err_w[ok] / ref["bound_w"][ok]).max())
    assert bool((err_m <= ref["bound_m"]).all()) and bool((err_w <= ref["bound_w"]).all()), (what, worst)
    assert bool((m1[live] != m0[live]).any()) and bool((w1[live] != w0[live]).any()), what
    want_f = (tab.w * tab.s_elem.to(DEV)).cpu()
    assert torch.equal(f1[wrote_f], want_f[wrote_f]) and int(wrote_f.sum()) > 0, what
    return worst


def cpu_state(tab):
    return [t.cpu() for t in tab.state()]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_default_record_is_k25_to_the_bit():
    tab = Table()
    sol = Solver(tab, two_groups=False)
    for call, lr in enumerate((0.05, 0.01)):
        tab.new_gradients(call)
        before = tab.state()
        tab.step(lr)
        k25 = cpu_state(tab)
        tab.restore(before)
        sol.call(sol.record(lr))
        got = cpu_state(tab)
        assert all(torch.equal(a, b) for a, b in zip(got, k25)), "call %d" % call
        assert not torch.equal(got[0], before[0].cpu())
        st = sol.status()                                                      # one launch: the status is not touched
        assert (st.bad_steps, st.first_bad_iteration, st.last_norm, st.poisoned) == (0, 0, 0.0, 0)
        # the same record with the guard: three launches, the solver's own step kernel -- K25's bits again
        tab.restore(before)
        sol.call(sol.record(lr, guard=True))
        assert all(torch.equal(a, b) for a, b in zip(cpu_state(tab), k25)), "call %d, guarded" % call
        st = sol.status()
        assert st.bad_steps == 0 and st.poisoned == 0 and st.last_norm > 0
        sol.ws.zero_()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
@pytest.mark.parametrize("clip", ["value", "norm", "full_model"])
def test_every_combination_against_the_referee(clip, nesterov):
    tab = Table()
    sol = Solver(tab)
    for call, lr in enumerate((0.05, 0.01)):
        tab.new_gradients(call)
        before = cpu_state(tab)
        rec = sol.record(lr, clip=clip, nesterov=nesterov)
        sol.call(rec)
        ref = referee(tab, sol, before[0], before[1], rec, clip, nesterov)
        worst = check_against_referee(tab, sol, before, ref, (clip, nesterov, call))
        print("SOLVER_K29 %s %s call %d lr %g: %d live elements, err_m / bound <= %.3f, err_w / bound <= %.3f" % (
            clip, "nesterov" if nesterov else "plain", call, lr, int(tab.live.sum()), worst[0], worst[1]))
        if clip == "value":
            assert bool((np.abs(ref["a0"]) > V).any()) and float(np.abs(ref["a"]).max()) == V
            continue
        # the coefficients and the norm: fp64 sums of at most n terms, one rounding to fp32
        n_all, hg = int(tab.live.sum()), tab.has_grad.numpy()
        coef, st = sol.coef(), sol.status()
        tol = (n_all + 4) * 2.0 ** -53
        assert st.bad_steps == 0 and st.poisoned == 0
        assert abs(st.last_norm - np.sqrt(ref["total"])) <= tol * np.sqrt(ref["total"])
        want = np.append(ref["coef"], ref["coef_all"])
        assert bool((np.abs(coef.astype(np.float64) - want) <= (U + tol) * want).all())
        assert bool((coef[:-1][~hg] == 1.0).all()) and bool((coef[:-1][hg] < 1.0).any()) and bool((coef[:-1][hg] == 1.0).any()) and coef[-1] < 1.0


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", ["value", "norm", "full_model"])
def test_under_the_threshold_nothing_changes(clip):
    """clip_value = 1e30: far above every norm (the table's is below 1e3) and far above every |a0|."""
    tab = Table()
    sol = Solver(tab)
    tab.new_gradients(0)
    before = tab.state()
    sol.call(sol.record(0.05, clip="off", nesterov=True))
    off = cpu_state(tab)
    tab.restore(before)
    sol.call(sol.record(0.05, clip=clip, nesterov=True, v=1e30))
    assert all(torch.equal(a, b) for a, b in zip(cpu_state(tab), off))
    assert not torch.equal(off[0], before[0].cpu())
    if clip != "value":
        assert bool((sol.coef() == 1.0).all()) and 1.0 < sol.status().last_norm < 1e4


# ---- 4 and 5 ---------------------------------------------------------------------------------------------------------------------------
def tensor_with(tab, n, pc=0, has_grad=True):
    return next(t for t, (k, p, _) in enumerate(tab.specs) if k == n and p == pc and bool(tab.has_grad[t]) == has_grad)


def test_membership_a_tensor_without_a_gradient_is_in_no_norm_and_a_zero_gradient_has_coefficient_one():
    tab = Table()
    sol = Solver(tab)
    tab.new_gradients(0)
    zero = tensor_with(tab, 4097)
    tab.g[tab.off[zero]:tab.off[zero] + 4097] = 0.0
    before = cpu_state(tab)
    rec = sol.record(0.05, clip="full_model", guard=True)
    sol.call(rec)
    ref = referee(tab, sol, before[0], before[1], rec, "full_model", False)
    check_against_referee(tab, sol, before, ref, "membership")
    st, coef = sol.status(), sol.coef()
    assert abs(st.last_norm ** 2 - ref["total"]) <= 2 * (int(tab.live.sum()) + 4) * 2.0 ** -53 * ref["total"] and st.bad_steps == 0
    assert ref["sumsq"][zero] == 0.0 and coef[zero] == 1.0 and bool((coef[:-1][~tab.has_grad.numpy()] == 1.0).all())
    # what lies in the gradient arena where a tensor has NO gradient is not read: the same norm, to the bit
    for t in torch.nonzero(~tab.has_grad).flatten().tolist():
        tab.g[tab.off[t]:tab.off[t] + tab.specs[t][0]] = 1e19
    tab.restore([b.to(DEV) for b in before])
    sol.call(rec)
    assert sol.status().last_norm == st.last_norm and np.array_equal(sol.coef(), coef)


def test_a_large_finite_gradient_has_a_finite_norm_is_clipped_and_is_not_called_bad():
    """1e30 throughout one tensor: its squares overflow fp32, their fp64 sum does not."""
    tab = Table()
    sol = Solver(tab)
    tab.new_gradients(0)
    big = tensor_with(tab, 4097)
    tab.g[tab.off[big]:tab.off[big] + 4097] = 1e30
    for clip in ("norm", "full_model"):
        before = cpu_state(tab)
        rec = sol.record(0.05, clip=clip, guard=True)
        sol.call(rec)
        st, coef = sol.status(), sol.coef()
        assert st.bad_steps == 0 and st.poisoned == 0 and np.isfinite(st.last_norm) and st.last_norm >= 1e30 * 64, clip
        assert 0.0 < coef[big] < 1e-30 and np.isfinite(coef).all(), clip
        ref = referee(tab, sol, before[0], before[1], rec, clip, False)
        check_against_referee(tab, sol, before, ref, ("large", clip))
        sl = slice(tab.off[big], tab.off[big] + 4097)
        a = coef[big if clip == "norm" else -1] * np.float32(1e30)               # the clipped gradient: the tensor's norm is clip_value
        assert abs(float(a) * np.sqrt(4097.0) - V) <= 1e-5 * V if clip == "norm" else float(a) * np.sqrt(4097.0) <= V, clip
        assert bool(torch.isfinite(tab.w[sl]).all()) and bool(torch.isfinite(tab.m[sl]).all())


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
def plant_inf_in_the_tail(tab):
    t = tensor_with(tab, 4097)
    tab.g[tab.off[t] + 4096] = float("inf")


def plant_nan_in_a_one_element_tensor(tab):
    tab.g[tab.off[tensor_with(tab, 1)]] = float("nan")


def plant_inf_under_a_zero_scale(tab):
    t = next(t for t, (n, pc, _) in enumerate(tab.specs) if pc == 27 and n == 27 * 64 and bool(tab.has_grad[t]))
    tab.scale[tab.soff[t] + 5] = 0.0
    tab.scale_host[tab.soff[t] + 5] = 0.0
    tab.s_elem[tab.off[t] + 5 * 27:tab.off[t] + 6 * 27] = 0.0
    tab.g[tab.off[t] + 5 * 27 + 3] = float("inf")                              # finite s elsewhere; here only the product is not finite


@pytest.mark.parametrize("plant,clip", [(plant_inf_in_the_tail, "off"), (plant_nan_in_a_one_element_tensor, "full_model"),
                                        (plant_inf_under_a_zero_scale, "norm"), (None, "value")],
                         ids=["inf_in_the_tail_of_4097", "nan_in_a_one_element_tensor", "inf_times_zero_scale", "watched_scalar"])
def test_the_guard_writes_nothing(plant, clip):
    """Arithmetic NaNs and infinities in the gradients (or, with all gradients finite, in a watched scalar): the step writes nothing, the
    status says so, the next finite step is a no-op too, and after the reset the same call steps within the bounds."""
    tab = Table()
    sol = Solver(tab)
    tab.new_gradients(0)
    watch = torch.tensor([0.25, 1.5], device=DEV)
    if plant is None:
        watch[1] = float("inf")
    else:
        plant(tab)
    watched = (watch[0:1], watch[1:2])
    arenas = lambda: [t.cpu() for t in (tab.w, tab.m, tab.f, tab.g, tab.scale)]
    before = arenas()
    sol.call(sol.record(0.05, clip=clip, nesterov=True, guard=True, iteration=41, watch=watched))
    after = arenas()
    assert all(a.view(torch.int32).equal(b.view(torch.int32)) for a, b in zip(after, before))          # every arena, sentinels included, to the bit
    st = sol.status()
    assert st.bad_steps == 1 and st.first_bad_iteration == 41 and st.poisoned != 0
    # a following call with finite gradients and losses: a no-op as well
    tab.new_gradients(0)
    watch[1] = 1.5
    before = arenas()
    rec = sol.record(0.05, clip=clip, nesterov=True, guard=True, iteration=42, watch=watched)
    sol.call(rec)
    assert all(a.view(torch.int32).equal(b.view(torch.int32)) for a, b in zip(arenas(), before))
    st = sol.status()
    assert st.bad_steps == 1 and st.first_bad_iteration == 41 and st.poisoned != 0
    # after the reset the same call steps
    sol.reset()
    st = sol.status()
    assert (st.bad_steps, st.first_bad_iteration, st.poisoned) == (0, 0, 0)
    sol.call(rec)
    ref = referee(tab, sol, before[0], before[1], rec, clip, True)
    check_against_referee(tab, sol, before[:3], ref, ("after reset", clip))
    st = sol.status()
    assert st.bad_steps == 0 and st.poisoned == 0 and np.isfinite(st.last_norm) and st.last_norm > 0


def test_without_the_guard_a_bad_step_is_counted_and_taken():
    """guard = 0 with a norm: the status counts the step, nothing is poisoned, and the NaN reaches the weights as torch would let it."""
    tab = Table()
    sol = Solver(tab)
    tab.new_gradients(0)
    plant_nan_in_a_one_element_tensor(tab)
    t = tensor_with(tab, 1)
    sol.call(sol.record(0.05, clip="norm", iteration=7))
    st = sol.status()
    assert st.bad_steps == 1 and st.first_bad_iteration == 7 and st.poisoned == 0
    assert bool(torch.isnan(tab.w[tab.off[t]])) and int(torch.isnan(tab.w).sum()) == 1


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits_and_the_grid_has_no_part_in_them():
    tab = Table()
    sol = Solver(tab)
    tab.new_gradients(0)
    before = tab.state()
    n = len(tab.specs)
    runs = {}
    for clip in ("norm", "full_model"):
        rec = sol.record(0.05, clip=clip, nesterov=True, guard=True)
        for k in range(2):
            tab.restore(before)
            sol.ws.zero_()
            sol.call(rec)
            runs[clip, k] = cpu_state(tab) + [sol.ws.cpu()]
        assert all(torch.equal(a, b) for a, b in zip(runs[clip, 0], runs[clip, 1])), clip        # w, m, folded, and partial + coef + status
        assert not torch.equal(runs[clip, 0][0], before[0].cpu())
    # the same tensors listed in reverse: every chunk is another map entry, on another workgroup
    rev = (hip.PodSgdTensor * n)()
    for k in range(n):
        ctypes.memmove(ctypes.byref(rev[k]), ctypes.byref(tab.table[n - 1 - k]), ctypes.sizeof(hip.PodSgdTensor))
    lib = hip.load()
    assert lib.pod_sgd_chunk_map(rev, n, None, 0) == tab.n_chunks
    cmap = torch.zeros((tab.n_chunks, 2), dtype=torch.int32)
    assert lib.pod_sgd_chunk_map(rev, n, cmap.data_ptr(), tab.n_chunks) == tab.n_chunks
    group_rev = list(reversed(sol.group))
    tab.restore(before)
    sol.ws.zero_()
    sol.call(sol.record(0.05, clip="norm", nesterov=True, guard=True))
    coef_fwd, partial_fwd = sol.coef().copy(), sol.partial().copy()
    tab.restore(before)
    sol.ws.zero_()
    sol.call(sol.record(0.05, clip="norm", nesterov=True, guard=True), table=rev, cmap=cmap.to(DEV), group_host=(ctypes.c_uint8 * n)(*group_rev),
             group_dev=torch.tensor(group_rev, dtype=torch.uint8).to(DEV))
    assert all(torch.equal(a, b) for a, b in zip(cpu_state(tab), runs["norm", 0][:3]))
    hg = tab.has_grad.numpy()
    assert np.array_equal(sol.coef()[:-1][::-1], coef_fwd[:-1])
    # the partials, per tensor in chunk order, are the first table's (those of a tensor without a gradient are never written: zero)
    fwd_map, rev_map = tab.cmap.cpu().numpy(), cmap.numpy()
    by_tensor = lambda m, p, flip: {((n - 1 - int(t)) if flip else int(t), int(c)): float(x) for (t, c), x in zip(m, p)}
    a, b = by_tensor(fwd_map, partial_fwd, False), by_tensor(rev_map, sol.partial(), True)
    assert a == b and len(a) == tab.n_chunks and sum(1 for (t, _), x in a.items() if hg[t] and x > 0) > 300
