"""GPU: ogs_separation_loss (csrc/mask_ops.hip) at the edges of what it serves -- N = 2 .. 1024 (four columns per thread,
a 1024-slot LDS row), C = 1 .. 16, early and late weights -- against float64 on the CPU, and against the reference's own
separation_loss (tests/golden/separation_golden.npz).

The loss weights every pair by the RANK of its inverse distance inside its row, so a comparison of results alone has to
budget for rank swaps between two float32 evaluations (test_30's `flip` term).  The C ABI leaves the weights it used in
its scratch (tmp[0 : N*N], then the N row losses), so here nothing is budgeted: the weights are read back, checked for
what they must be bit for bit (a permutation of the N rank weights per row, in the order of the float64 inverse distances
up to a tie width derived from the reference formula's own float32 error), and value and gradient are then held to float64
evaluations WITH THOSE WEIGHTS at the plain rounding bars: 2e-6 relative on values, 1e-5 of the largest entry on
gradients.

Measured on an MI355X (printed by the tests; e32 = largest deviation of the reference formula's float32 inverse distances
on the CPU from its float64 ones, tau = 4 * e32, near = share of float64-neighbouring pairs closer than tau, then the
worst relative errors of loss / row losses and the worst gradient error over its largest entry, early | late):
    N    C  e32      tau      near     inversions<tau  loss            rows            grad
    2    6  1.28e-08 5.13e-08 0.0000%     0 / 2        2.1e-08|2.1e-08 2.1e-08|2.1e-08 6.1e-08|6.1e-08
    3    6  3.27e-08 1.31e-07 0.0000%     0 / 6        2.7e-09|1.4e-07 4.6e-08|8.6e-08 1.6e-07|1.4e-07
   10    6  5.31e-08 2.13e-07 0.0000%     0 / 90       3.5e-08|2.7e-08 7.5e-08|8.8e-08 7.9e-08|1.2e-07
   19    6  6.63e-08 2.65e-07 0.0000%     0 / 342        7e-08|6.7e-08 1.2e-07|1.1e-07 8.4e-08|1.6e-07
  255    6  8.66e-08 3.46e-07 0.0216%     2 / 64770    2.4e-07|5.8e-08 1.1e-07|1.2e-07 1.5e-07|1.6e-07
  256    6  8.33e-08 3.33e-07 0.0199%     3 / 65280    8.3e-07|6.4e-08 1.1e-07|1.4e-07 1.5e-07|1.7e-07
  257    6  8.3e-08  3.32e-07 0.0274%     1 / 65792    9.9e-08|8.1e-08 1.2e-07|1.4e-07 1.1e-07|1.2e-07
 1000    6  9.22e-08 3.69e-07 0.0986%    41 / 999000   2.8e-07|9.2e-07 1.5e-07|1.3e-07 1.3e-07|1.2e-07
 1023    6  9.19e-08 3.68e-07 0.0947%    43 / 1045506  4.9e-07|1.4e-07 1.3e-07|1.5e-07 1.5e-07|1.2e-07
 1024    6  9.88e-08 3.95e-07 0.1015%    53 / 1047552  1.7e-07|3.2e-08 1.3e-07|1.4e-07 1.2e-07|1.3e-07
   10    1  7.61e-08 3.04e-07 0.0000%     0 / 90       1.2e-07|4.5e-08 7.8e-08|4.5e-08 1.3e-07|8.1e-08
   10   16  3.77e-08 1.51e-07 0.0000%     0 / 90       1.2e-07|5.2e-08 6.7e-08|7.9e-08 7.1e-08|6.8e-08
  257    1  8.75e-08 3.5e-07  0.0654%     7 / 65792      6e-08|5e-07   1.2e-07|1.1e-07 1.2e-07|1e-07  
  257   16  6.51e-08 2.6e-07  0.0365%     0 / 65792    3.8e-08|8.5e-09   1e-07|1.2e-07 1.5e-07|1.2e-07
 1024    1  8.9e-08  3.56e-07 0.4475%   393 / 1047552  1.2e-06|3e-08   1.5e-07|1.1e-07 1.6e-07|1.3e-07
 1024   16  8.57e-08 3.43e-07 0.1803%    63 / 1047552    1e-07|2.4e-07 1.3e-07|1.4e-07 1.2e-07|1.1e-07
Against the reference golden (N = 2 .. 37, C = 1, 6, 16, early and late): loss 1.9e-07, gradient 2.0e-07 at worst
(e32 of the file: 4.9e-08 .. 1.6e-07).  Before the contraction pragma in separation_rows_kernel the first check
failed at every N >= 10: the weights came out of one fused multiply-add.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests.golden import make_separation_golden as sg

pytestmark = pytest.mark.gpu
SEP_GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "separation_golden.npz"))

# every N with C = 6; the smallest, a middle and the largest N with the smallest and the largest C
SIZES = [(N, 6) for N in (2, 3, 10, 19, 255, 256, 257, 1000, 1023, 1024)] + \
        [(N, C) for N in (10, 257, 1024) for C in (1, 16)]
VALUE_RTOL, GRAD_TOL, TIE_FACTOR, NEAR_CAP = 2e-6, 1e-5, 4.0, 0.01


@functools.lru_cache(maxsize=None)
def reference(N, C):
    """means (float32, CPU, seeded), their float64 inverse distances, e32 and the share of near-tied neighbours"""
    from oracle import mask_oracle as mo
    means = torch.rand(N, C, generator=torch.Generator().manual_seed(34000 + 17 * N + C))
    inv64 = mo.separation_inverse_distance(means, torch.float64)
    e32 = float((mo.separation_inverse_distance(means, torch.float32).double() - inv64).abs().max())
    tau = TIE_FACTOR * e32
    s = inv64.sort(dim=1).values
    near = float(((s[:, 1:] - s[:, :-1]) < tau).double().mean())
    return means, inv64, e32, tau, near


def call_c_abi(means_gpu, late, want_grad=True):
    """ogs_separation_loss with its scratch kept: (loss [], grad [N,C] or None, weights [N,N], row_loss [N]) on the CPU"""
    from opengaussian_amd import _lib
    from opengaussian_amd._lib import check, ptr
    N, C = means_gpu.shape
    assert means_gpu.is_contiguous() and means_gpu.dtype == torch.float32
    dev = means_gpu.device
    loss = torch.full((), float("nan"), device=dev)
    grad = torch.full((N, C), float("nan"), device=dev) if want_grad else None
    tmp = torch.full((N * N + N,), float("nan"), device=dev)
    check(_lib.lib().ogs_separation_loss(ptr(means_gpu), N, C, int(late), ptr(loss), ptr(grad), ptr(tmp),
                                         torch.cuda.current_stream().cuda_stream), "ogs_separation_loss")
    tmp = tmp.cpu()
    return loss.cpu(), None if grad is None else grad.cpu(), tmp[:N * N].view(N, N), tmp[N * N:]


def grad_with_weights(means, inv64, w):
    """-2 / (N (N-1)) * sum_j (w_ij + w_ji) * inv_ij^2 * (m_i - m_j) in float64; sum_j k_ij (m_i - m_j) =
    m_i sum_j k_ij - (k m)_i"""
    N = means.shape[0]
    m = means.double()
    k = (w.double() + w.double().t()) * inv64 * inv64
    return -2.0 / (N * (N - 1)) * (k.sum(1, keepdim=True) * m - k @ m)


@pytest.mark.parametrize("N,C", SIZES, ids=lambda v: str(v))
def test_c_abi_weights_value_and_gradient(gpu_device, N, C):
    from oracle import mask_oracle as mo
    means, inv64, e32, tau, near = reference(N, C)
    assert near <= NEAR_CAP, f"input condition: {near:.4%} of the neighbouring pairs lie within tau = {tau:.3g}"
    mg = means.to(gpu_device)
    table = mo.separation_weights(torch.arange(N), 1000)                 # the N rank weights, float32, as the reference writes them
    assert bool((table[1:] > table[:-1]).all())                          # strictly increasing: a weight names its rank
    report = [f"N={N} C={C} e32={e32:.3g} tau={tau:.3g} near={near:.4%}"]

    loss, grad, w_early, row_loss = call_c_abi(mg, late=0)
    # 1. early weights are ranks
    rank = torch.searchsorted(table, w_early.contiguous()).clamp(max=N - 1)
    assert torch.equal(table[rank], w_early), "a weight that is none of (r / (N-1)) * 0.9 + 0.1"
    assert torch.equal(rank.sort(dim=1).values, torch.arange(N).expand(N, N)), "a row's ranks are no permutation"
    assert bool((rank.diagonal() == 0).all())
    # 2. the ranks follow the float64 inverse distances, up to the tie width
    by_rank = inv64.gather(1, rank.argsort(dim=1))
    step = by_rank[:, 1:] - by_rank[:, :-1]
    assert int((step <= -tau).sum()) == 0, f"rank inversions beyond tau: worst step {float(step.min()):.3g}"
    report.append(f"inversions inside tau: {int((step < 0).sum())} of {step.numel()}")

    errors = []
    for mode, late in (("early", 0), ("late", 1)):
        if late:
            loss, grad, w, row_loss = call_c_abi(mg, late=1)
            # 3. late weights: the float32 threshold on the early ones, bit for bit
            assert torch.equal(w, mo.separation_weights(rank, 40000))
            assert torch.equal(w, torch.where(w_early < 0.9, torch.full_like(w_early, 0.1), w_early))
            if (N - 1) % 9 == 0:                                         # a rank exactly on the boundary is kept
                on = rank == 8 * (N - 1) // 9
                assert bool((w[on] == float(np.float32(0.90000004))).all()) and int(on.sum()) == N
        else:
            w = w_early
        # 4. value, with the weights the kernel used
        rows64 = (inv64 * w.double()).sum(1)
        want = float(rows64.sum() / (N * (N - 1)))
        err_v = abs(float(loss) - want) / abs(want)
        err_r = float(((row_loss.double() - rows64).abs() / rows64.abs()).max())
        # 5. gradient, with the weights the kernel used
        want_g = grad_with_weights(means, inv64, w)
        err_g = float((grad.double() - want_g).abs().max() / want_g.abs().max())
        report.append(f"{mode}: loss {err_v:.2g} rows {err_r:.2g} grad {err_g:.2g}")
        errors += [err_v, err_r, err_g]
        loss_only = call_c_abi(mg, late, want_grad=False)
        assert loss_only[0].view(torch.int32).item() == loss.view(torch.int32).item()     # grad == NULL: the same loss bits
        assert torch.equal(loss_only[2], w)
    print(" | ".join(report))
    for err_v, err_r, err_g in (errors[:3], errors[3:]):
        assert err_v <= VALUE_RTOL and err_r <= VALUE_RTOL and err_g <= GRAD_TOL, report


# ---- the reference's own numbers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C", sg.CASES, ids=lambda v: str(v))
def test_kernel_matches_reference_golden(gpu_device, N, C):
    """early and late, value at 2e-6 relative, gradient at max(1e-5, 4 * e32) of the largest entry (e32: the reference's
    own float32 gradient against its float64 one, from the file); means with every row's ranks at least 2e-6 apart"""
    from opengaussian_amd import mask_ops as mk
    base = sg.case_means(N, C)
    for mode, it in sg.ITERATIONS.items():
        k = f"n{N}_c{C}_{mode}"
        value, want, e32 = float(SEP_GOLD[k + "_value"]), SEP_GOLD[k + "_grad"], float(SEP_GOLD[k + "_e32"])
        m = base.to(gpu_device).requires_grad_(True)
        loss = mk.separation_loss(m, it)
        loss.backward()
        err_v = abs(float(loss.detach()) - value) / abs(value)
        err_g = np.abs(m.grad.double().cpu().numpy() - want).max() / np.abs(want).max()
        print(f"golden {k}: loss {err_v:.2g} grad {err_g:.2g} (e32 {e32:.2g})")
        assert err_v <= VALUE_RTOL
        assert err_g <= max(GRAD_TOL, 4 * e32)


# ---- tied rows ------------------------------------------------------------------------------------------------------------
def tied_means(N, C=6):
    """the first N // 2 rows zero (empty masks share the zero mean); the other rows redrawn until, in every row, two
    float64 inverse distances are either exactly equal (the ties) or at least GAP apart"""
    g = torch.Generator().manual_seed(3434 + N)
    from oracle import mask_oracle as mo
    for _ in range(2000):
        m = torch.rand(N, C, generator=g)
        m[:N // 2] = 0.0
        s = mo.separation_inverse_distance(m).sort(dim=1).values
        gaps = s[:, 1:] - s[:, :-1]
        if bool(((gaps == 0) | (gaps >= sg.GAP)).all()):
            assert int((gaps == 0).sum()) >= N * (N // 2 - 2)
            return m
    raise AssertionError(f"no well-separated tied means for N = {N}")


@pytest.mark.parametrize("N", [9, 96])
def test_tied_rows(gpu_device, N):
    from opengaussian_amd import mask_ops as mk
    from oracle import mask_oracle as mo
    tied = tied_means(N)
    T = N // 2
    for it in (1000, 40000):
        a = tied.to(gpu_device).requires_grad_(True)
        la = mk.separation_loss(a, it)
        la.backward()
        b = tied.to(gpu_device).requires_grad_(True)
        lb = mk.separation_loss(b, it)
        lb.backward()
        assert torch.isfinite(la) and float(la.detach()) == float(lb.detach()) and torch.equal(a.grad, b.grad)   # run to run
        # ties by column (stable), the rule the kernel documents -- and ties by descending column, as good an argsort
        m = tied.double().requires_grad_(True)
        stable = mo.separation_loss(m, it)
        stable.backward()
        inv = mo.separation_inverse_distance(tied)
        other_rank = inv.flip(1).argsort(dim=1, stable=True).argsort(dim=1).flip(1)
        m2 = tied.double().requires_grad_(True)
        other = mo.separation_loss(m2, it, weights=mo.separation_weights(other_rank, it))
        other.backward()
        big = float(m.grad.abs().max())
        assert abs(float(other.detach()) - float(stable.detach())) <= 1e-12 * float(stable.detach())            # the value does not depend on the order
        assert float((m2.grad[T:] - m.grad[T:]).abs().max()) <= 1e-12 * big        # nor does an untied row's gradient
        if it == 1000:      # a tied row's does: the rule is tested.  (Late, the tied columns are the far ones: all 0.1.)
            assert float((m2.grad[:T] - m.grad[:T]).abs().max()) > 100 * GRAD_TOL * big
        got = a.grad.double().cpu()
        assert abs(float(la.detach()) - float(stable.detach())) <= VALUE_RTOL * float(stable.detach())
        assert float((got[T:] - m2.grad[T:]).abs().max()) <= GRAD_TOL * big
        assert float((got - m.grad).abs().max()) <= GRAD_TOL * big


# ---- upstream scale, layout, dispatch ---------------------------------------------------------------------------------------
def test_upstream_scale_and_sliced_means(gpu_device):
    from opengaussian_amd import mask_ops as mk
    from oracle import mask_oracle as mo
    N, C = 19, 6
    base = sg.case_means(N, C)
    m64 = base.double().requires_grad_(True)
    mo.separation_loss(m64, 1000).backward()
    one = base.to(gpu_device).requires_grad_(True)
    l1 = mk.separation_loss(one, 1000)
    l1.backward()
    three = base.to(gpu_device).requires_grad_(True)
    (3.0 * mk.separation_loss(three, 1000)).backward()
    assert torch.equal(three.grad, 3.0 * one.grad)
    assert float((three.grad.double().cpu() - 3.0 * m64.grad).abs().max()) <= GRAD_TOL * 3.0 * float(m64.grad.abs().max())
    wide = torch.rand(N, 12, generator=torch.Generator().manual_seed(5)).to(gpu_device)
    wide[:, 2:8] = base.to(gpu_device)
    wide.requires_grad_(True)
    cols = wide[:, 2:8]
    assert not cols.is_contiguous()
    l2 = mk.separation_loss(cols, 1000)
    l2.backward()
    assert float(l2.detach()) == float(l1.detach())
    assert torch.equal(wide.grad[:, 2:8], one.grad)
    assert float(wide.grad[:, :2].abs().max()) == 0.0 and float(wide.grad[:, 8:].abs().max()) == 0.0


@pytest.mark.parametrize("N,C", [(1025, 6), (10, 17)])
def test_sizes_past_the_kernel_take_the_torch_formulation(gpu_device, N, C):
    """one past the 1024-slot row, one past the 16 channels: ogs_separation_loss refuses these, so a wrong dispatch is an
    error, and the torch formulation on the GPU meets the float64 oracle at test_30's bars (with its once-per-element
    allowance for a rank swap: here two float32 evaluations are compared by their results alone)"""
    from opengaussian_amd import mask_ops as mk
    from oracle import mask_oracle as mo
    base = torch.rand(N, C, generator=torch.Generator().manual_seed(N + C))
    for it in (1000, 40000):
        m64 = base.double().requires_grad_(True)
        want = mo.separation_loss(m64, it)
        want.backward()
        m = base.to(gpu_device).requires_grad_(True)
        loss = mk.separation_loss(m, it)
        loss.backward()
        torch.testing.assert_close(loss.detach().cpu().double(), want.detach(), rtol=2e-6, atol=1e-7)
        flip = 3.6 / ((N - 1) ** 2 * N)
        assert float((m.grad.double().cpu() - m64.grad).abs().max()) <= 1e-5 * float(m64.grad.abs().max()) + flip


def test_other_dtypes_and_a_single_mask(gpu_device):
    from opengaussian_amd import mask_ops as mk
    from oracle import mask_oracle as mo
    base = sg.case_means(19, 6)
    for it in (1000, 40000):
        m = base.double().to(gpu_device).requires_grad_(True)
        loss = mk.separation_loss(m, it)                                  # float64 means: torch, in float64
        loss.backward()
        m64 = base.double().requires_grad_(True)
        want = mo.separation_loss(m64, it)
        want.backward()
        # The weights are float32 whatever the means are (`sorted_indices.float()`), and torch on the GPU divides by the
        # scalar N - 1 as a product with its float32 reciprocal: rank * fl(1 / (N-1)) lies within an ulp of the quotient,
        # a weight within 1.5 ulp = 1.8e-7 of the oracle's.  The value is a sum of positive terms: 2e-7 relative.  A
        # gradient element is a sum of N - 1 signed terms, each that good: 2e-7 of their absolute sum, bounded here by
        # (N - 1) times the largest term and stated against the largest entry as 2e-7 * (N - 1) = 3.6e-6.
        assert loss.dtype == torch.float64 and abs(float(loss.detach()) - float(want.detach())) <= 2e-7 * float(want.detach())
        assert float((m.grad.cpu() - m64.grad).abs().max()) <= 3.6e-6 * float(m64.grad.abs().max())
    # one mask: train.py:146 divides rank 0 by N - 1 = 0 and :153 the sum by N (N-1) = 0 -- the reference returns NaN
    single = mk.separation_loss(torch.rand(1, 6, device=gpu_device), 1000)
    assert single.shape == () and bool(torch.isnan(single))
