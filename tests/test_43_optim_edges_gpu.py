"""GPU: opengaussian_amd.optim.FusedAdam against torch.optim.Adam on the CPU where tests/test_40_optim_gpu.py does not
go: element counts either side of the float4 vector and the 4096-element chunk, a second launch (more than 16
tensors), two (betas, eps) buckets, unaligned storage (the scalar path), exactly-zero gradient rows and a resumed step
count.  Same bars and the same ulp measure as test_40."""
import pytest
import torch

from tests.test_40_optim_gpu import PARAM_ULP_BAR, ULP_BAR, _max_ulp

pytestmark = pytest.mark.gpu
REFERENCE_LRS = (1.6e-4, 2.5e-3, 1.25e-4, 0.05, 5e-3, 1e-3, 1e-3)


def _pair(shapes, dev, seed, cfgs=None, lr=None):
    """the same tensors as one-tensor groups of a CPU torch.optim.Adam and a GPU FusedAdam"""
    from opengaussian_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(*s, generator=g) for s in shapes]
    cpu = [torch.nn.Parameter(t.clone()) for t in init]
    gpu = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    cfgs = cfgs or [{} for _ in shapes]
    # learning rates the reference uses (scene/gaussian_model.py:216-224): PARAM_ULP_BAR is derived for updates of at most
    # ~0.05 per step (see test_40); a larger rate moves the parameter by more ulps of the bar's floor per step
    lrs = lr or [REFERENCE_LRS[i % len(REFERENCE_LRS)] for i in range(len(shapes))]
    mk = lambda ps: [dict(params=[p], lr=l, **c) for p, l, c in zip(ps, lrs, cfgs)]
    return init, cpu, gpu, torch.optim.Adam(mk(cpu), lr=0.0, eps=1e-15), FusedAdam(mk(gpu), lr=0.0, eps=1e-15), g


def _feed(cpu, gpu, g, dev, zero_rows=None):
    for pc, pg in zip(cpu, gpu):
        grad = torch.randn(pc.shape, generator=g) * (10.0 ** float(torch.randint(-4, 2, (1,), generator=g)))
        if zero_rows is not None:
            grad[zero_rows] = 0.0
        pc.grad, pg.grad = grad.clone(), grad.to(dev)


def _compare(cpu, gpu, ref, opt, rows=None):
    for i, (pc, pg) in enumerate(zip(cpu, gpu)):
        sel = (lambda t: t.detach()) if rows is None else (lambda t: t.detach()[rows])
        sa, sb = opt.state[pg], ref.state[pc]
        ulp = (_max_ulp(sel(pg), sel(pc)), _max_ulp(sel(sa["exp_avg"]), sel(sb["exp_avg"])), _max_ulp(sel(sa["exp_avg_sq"]), sel(sb["exp_avg_sq"])))
        print(f"tensor {i} {tuple(pc.shape)}: ulp param {ulp[0]:.2f} exp_avg {ulp[1]:.2f} exp_avg_sq {ulp[2]:.2f}")
        assert ulp[0] <= PARAM_ULP_BAR, (i, ulp)
        assert float(sa["step"]) == float(sb["step"]), i
        assert ulp[1] <= ULP_BAR and ulp[2] <= ULP_BAR, (i, ulp)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 4095, 4096, 4097, 8193])
def test_element_counts_around_vector_and_chunk(gpu_device, n):
    """tails shorter than a float4, a last float4 that is partly past the end, and one element before / on / past
    one and two 4096-element chunks"""
    init, cpu, gpu, ref, opt, g = _pair([(n,)], gpu_device, 100 + n, lr=[1e-2])
    for _ in range(6):
        _feed(cpu, gpu, g, gpu_device)
        ref.step(); opt.step()
        assert opt.last_step_launches == 1
    _compare(cpu, gpu, ref, opt)


def test_twenty_groups_take_two_launches(gpu_device):
    """more tensors than one launch carries descriptors for: the seventeenth is the first of the second launch"""
    shapes = [(61 + 97 * i, 1 + i % 4) for i in range(20)]
    init, cpu, gpu, ref, opt, g = _pair(shapes, gpu_device, 7)
    for _ in range(4):
        _feed(cpu, gpu, g, gpu_device)
        ref.step(); opt.step()
        assert opt.last_step_launches == 2
    _compare(cpu, gpu, ref, opt)
    for i in (15, 16, 19):                     # last of the first launch, first and last of the second: they moved at all
        assert not torch.equal(gpu[i].detach().cpu(), init[i])


def test_two_hyperparameter_buckets(gpu_device):
    """groups with different (betas, eps) cannot share a launch: one launch per bucket, each with its own constants"""
    a, b = dict(betas=(0.9, 0.999), eps=1e-15), dict(betas=(0.8, 0.99), eps=1e-8)
    shapes = [(700, 3), (700, 3), (4097,), (4097,), (33, 15, 3), (33, 15, 3)]
    init, cpu, gpu, ref, opt, g = _pair(shapes, gpu_device, 8, cfgs=[a, b, b, a, a, b], lr=[1e-2] * 6)
    for _ in range(5):
        _feed(cpu, gpu, g, gpu_device)
        ref.step(); opt.step()
        assert opt.last_step_launches == 2
    _compare(cpu, gpu, ref, opt)


def test_unaligned_storage_takes_the_scalar_path(gpu_device):
    """parameter, gradient and both moments one element into larger buffers (data_ptr % 16 == 4): compared with torch
    directly, and bit for bit with the same data in aligned tensors (the float4 path)"""
    from opengaussian_amd.optim import FusedAdam
    dev, n = gpu_device, 4096 + 4 + 3                                   # two chunks; ends inside a float4
    g = torch.Generator().manual_seed(9)
    init = torch.randn(n, generator=g)
    bufs = [torch.zeros(n + 8, device=dev) for _ in range(3)]
    bufs[0][1:1 + n] = init.to(dev)
    p_un = torch.nn.Parameter(bufs[0][1:1 + n])
    p_al = torch.nn.Parameter(init.clone().to(dev))
    p_cpu = torch.nn.Parameter(init.clone())
    o_un, o_al = FusedAdam([p_un], lr=1e-2, eps=1e-15), FusedAdam([p_al], lr=1e-2, eps=1e-15)
    ref = torch.optim.Adam([p_cpu], lr=1e-2, eps=1e-15)
    o_un.state[p_un] = {"step": torch.tensor(0.0), "exp_avg": bufs[1][1:1 + n], "exp_avg_sq": bufs[2][1:1 + n]}
    for _ in range(5):
        grad = torch.randn(n, generator=g)
        gbuf = torch.zeros(n + 8, device=dev)
        gbuf[1:1 + n] = grad.to(dev)
        p_un.grad, p_al.grad, p_cpu.grad = gbuf[1:1 + n], grad.to(dev), grad.clone()
        for t in (p_un, p_un.grad, o_un.state[p_un]["exp_avg"], o_un.state[p_un]["exp_avg_sq"]):
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        for t in (p_al, p_al.grad):
            assert t.data_ptr() % 16 == 0
        o_un.step(); o_al.step(); ref.step()
    assert o_al.state[p_al]["exp_avg"].data_ptr() % 16 == 0
    _compare([p_cpu], [p_un], ref, o_un)
    assert torch.equal(p_un.detach(), p_al.detach())
    for m in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(o_un.state[p_un][m], o_al.state[p_al][m])
    for b in bufs:                                                        # nothing written outside the views
        assert float(b[0]) == 0.0 and not b[1 + n:].any()


def test_zero_gradient_rows_do_not_move(gpu_device):
    """rows whose gradient is exactly zero from the first step on: 0 / (0 + eps) -- the parameter keeps its initial
    bits on both sides; the other rows stay within the bars"""
    P = 1000
    shapes = [(P, 3), (P, 1), (P, 6)]
    init, cpu, gpu, ref, opt, g = _pair(shapes, gpu_device, 10, lr=[1e-2, 5e-2, 1e-3])
    zero = torch.arange(P) % 3 == 0
    for _ in range(6):
        _feed(cpu, gpu, g, gpu_device, zero_rows=zero)
        ref.step(); opt.step()
    for i in range(len(shapes)):
        assert torch.equal(cpu[i].detach()[zero], init[i][zero]), i
        assert torch.equal(gpu[i].detach().cpu()[zero], init[i][zero]), i
        assert not opt.state[gpu[i]]["exp_avg"][zero.to(gpu_device)].any() and not opt.state[gpu[i]]["exp_avg_sq"][zero.to(gpu_device)].any()
        assert not torch.equal(gpu[i].detach().cpu()[~zero], init[i][~zero])
    _compare(cpu, gpu, ref, opt, rows=~zero)
    _compare(cpu, gpu, ref, opt)


def test_resumed_step_count(gpu_device):
    """a run resumed at step 29999: beta^t has underflowed to where only the bias corrections' last bits matter"""
    shapes = [(4097, 3), (513,)]
    init, cpu, gpu, ref, opt, g = _pair(shapes, gpu_device, 11, lr=[1e-2, 1e-3])
    for _ in range(3):                                                    # moments from the CPU optimizer
        for pc in cpu:
            pc.grad = torch.randn(pc.shape, generator=g)
        ref.step()
    for pc, pg in zip(cpu, gpu):
        ref.state[pc]["step"] = torch.tensor(29999.0)
        with torch.no_grad():
            pg.copy_(pc.detach().to(gpu_device))
        opt.state[pg] = {"step": torch.tensor(29999.0), "exp_avg": ref.state[pc]["exp_avg"].clone().to(gpu_device),
                         "exp_avg_sq": ref.state[pc]["exp_avg_sq"].clone().to(gpu_device)}
    for _ in range(3):
        _feed(cpu, gpu, g, gpu_device)
        ref.step(); opt.step()
    assert float(opt.state[gpu[0]]["step"]) == 30002.0
    _compare(cpu, gpu, ref, opt)
