"""No GPU: the restated update rules of tests/optim_ref.py against torch.optim.Adam / SGD with clip_grad_norm_ /
clip_grad_value_ on the CPU (bound: 1e-6 relative per tensor, the bound of tests/test_gpu_optim.py for this kernel family;
mistakes in the rules land outside it), construct_optimizer's `adam` branch, and what focus_optim_step and the Fused*
classes refuse before anything is launched."""
import ctypes

import pytest
import torch

import optim_ref as R

BOUND = 1e-6

ADAM_CASES = [dict(weight_decay=0.0), dict(weight_decay=5e-2)]
SGD_CASES = [dict(momentum=0.0, dampening=0.0, nesterov=False, weight_decay=1e-4),
             dict(momentum=0.9, dampening=0.1, nesterov=False, weight_decay=1e-4),
             dict(momentum=0.9, dampening=0.0, nesterov=True, weight_decay=1e-4)]
CLIPS = [(0.05, 0.0), (1e9, 0.0), (0.0, 0.0), (0.0, 0.01)]            # (max_norm, clip_value), never both


def _torch_run(kind, hyper, max_norm, clip_value):
    """torch's own sequence; returns per step (params, grads left in .grad, state tensors, total norm)."""
    ps = [torch.nn.Parameter(p.clone()) for p in R.make_params()]
    groups = [{"params": [ps[i] for i in idx], "lr": R.LR[gi][0]} for gi, idx in enumerate(R.GROUPS)]
    opt = torch.optim.Adam(groups, foreach=False, **hyper) if kind == "adam" else torch.optim.SGD(groups, foreach=False, **hyper)
    out = []
    for step, gs in enumerate(R.make_grads()):
        for gi, g in enumerate(opt.param_groups):
            g["lr"] = R.LR[gi][step]
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.clone()
        tn = None
        if clip_value > 0:
            torch.nn.utils.clip_grad_value_(ps, clip_value)
        elif max_norm > 0:
            tn = float(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False))
        opt.step()
        st = []
        for p in ps:
            s = opt.state.get(p, {})
            st.append((s.get("exp_avg"), s.get("exp_avg_sq")) if kind == "adam" else (s.get("momentum_buffer"), None))
        out.append(([p.detach().clone() for p in ps], [None if p.grad is None else p.grad.clone() for p in ps],
                    [tuple(None if t is None else t.clone() for t in s) for s in st], tn))
    return out


def _worst(kind, hyper, max_norm, clip_value, dtype, mutant=None):
    """largest per-tensor relative distance between the restated rule and torch over the four steps"""
    want = _torch_run(kind, hyper, max_norm, clip_value)
    ref = R.Ref(kind, R.make_params(), dtype, mutant=mutant, **hyper)
    worst = 0.0
    for step, gs in enumerate(R.make_grads()):
        left = ref.step(gs, [R.LR[gi][step] for gi in range(3)], max_norm, clip_value)
        wp, wg, ws, tn = want[step]
        if tn is not None:
            worst = max(worst, abs(ref.last_total_norm - tn) / tn)
        for i in range(len(wp)):
            worst = max(worst, R.rel(ref.p[i], wp[i], R.P_FLOOR))
            if wg[i] is not None:
                worst = max(worst, R.rel(left[i], wg[i]))
            st = ref.state[i]
            for got, w in zip((st.get("m", st.get("buf")), st.get("v")), ws[i]):
                assert (got is None) == (w is None), "step %d tensor %d: state presence differs from torch's" % (step, i)
                if w is not None:
                    worst = max(worst, R.rel(got, w))
    return worst


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("hyper", ADAM_CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_adam_rule_matches_torch(dtype, hyper, clip):
    w = _worst("adam", hyper, clip[0], clip[1], dtype)
    print("adam %s %s %s: %.3e" % (dtype, hyper, clip, w))
    assert w <= BOUND


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("hyper", SGD_CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_sgd_rule_matches_torch(dtype, hyper, clip):
    w = _worst("sgd", hyper, clip[0], clip[1], dtype)
    print("sgd %s %s %s: %.3e" % (dtype, hyper, clip, w))
    assert w <= BOUND


@pytest.mark.parametrize("kind,hyper,mutant", [
    ("sgd", SGD_CASES[1], "dampened_first_use"),
    ("adam", ADAM_CASES[1], "decoupled_decay"),
    ("sgd", SGD_CASES[2], "nesterov_without_lookahead")])
def test_a_mistaken_rule_lands_outside_the_bound(kind, hyper, mutant):
    assert _worst(kind, hyper, 0.05, 0.0, torch.float32) <= BOUND
    assert _worst(kind, hyper, 0.05, 0.0, torch.float32, mutant=mutant) > 10 * BOUND


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(8, 4)
        self.norm = torch.nn.LayerNorm(4)
        self.cls_token = torch.nn.Parameter(torch.zeros(1, 1, 4))

    def forward(self, x):
        return self.norm(self.fc(x)) + self.cls_token[0]

    def no_weight_decay(self):
        return {"cls_token"}


def _cfg(method):
    from focus_amd.slowfast.config.defaults import get_cfg
    cfg = get_cfg()
    cfg.SOLVER.OPTIMIZING_METHOD = method
    cfg.SOLVER.BASE_LR, cfg.SOLVER.WEIGHT_DECAY, cfg.SOLVER.ZERO_WD_1D_PARAM = 0.25, 0.125, True
    return cfg


def test_construct_optimizer_adam_on_a_cpu_model():
    """optimizer.py:155-161: Adam with L2 weight decay, betas (0.9, 0.999), the no-weight-decay grouping of the other methods.
    A CPU model gets torch's class (the fused one needs fp32 parameters on the GPU)."""
    from focus_amd.slowfast.models.optimizer import construct_optimizer
    net = _Net()
    opt = construct_optimizer(net, _cfg("adam"))
    assert type(opt) is torch.optim.Adam
    assert len(opt.param_groups) == 2
    decay, no_decay = opt.param_groups
    assert [id(p) for p in decay["params"]] == [id(net.fc.weight)]
    assert {id(p) for p in no_decay["params"]} == {id(net.cls_token), id(net.fc.bias), id(net.norm.weight), id(net.norm.bias)}
    assert decay["weight_decay"] == 0.125 and no_decay["weight_decay"] == 0.0
    for g in opt.param_groups:
        assert g["lr"] == 0.25 and tuple(g["betas"]) == (0.9, 0.999) and not g["amsgrad"]
        assert not g.get("decoupled_weight_decay", False)
    # the step works and tells the weight shadows (post-step hook) without a GPU
    net(torch.randn(2, 8)).square().sum().backward()
    before = net.fc.weight.detach().clone()
    opt.step()
    assert not torch.equal(before, net.fc.weight.detach())
    assert type(construct_optimizer(net, _cfg("sgd"))) is torch.optim.SGD
    with pytest.raises(NotImplementedError):
        construct_optimizer(net, _cfg("lars"))


@pytest.fixture(scope="module")
def lib():
    from focus_amd.build import build
    build(verbose=False)
    from focus_amd import _lib
    return _lib.lib()


def test_focus_optim_step_refuses_before_launching(lib):
    """Host pointers, no GPU: every refusal returns its code before a launch could touch them."""
    from focus_amd import _lib
    NULL, SHAPE, WORKSPACE, OK = -5, -1, -6, 0
    ADAMW, ADAM, SGD = 0, 1, 2
    buf = ctypes.create_string_buffer(1 << 13)
    a = ctypes.addressof(buf)
    ptr = ctypes.c_void_p(a + (-a % 16))
    ws = lib.focus_adamw_workspace_bytes()
    assert ws == 4096 and ctypes.sizeof(_lib.OptimHyper) == 56
    good = _lib.OptimHyper(beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.05)
    call = lambda mode, h, items=ptr, grads=ptr, groups=ptr, steps=ptr, wsp=ptr, nbytes=ws, n=1: lib.focus_optim_step(
        mode, items, grads, n, n, groups, steps, wsp, nbytes, None, None if h is None else ctypes.byref(h), None)
    for k in ("items", "grads", "groups", "steps", "wsp"):
        assert call(ADAM, good, **{k: None}) == NULL, k
    assert call(ADAM, None) == NULL
    assert call(3, good) == SHAPE and call(-1, good) == SHAPE                                 # unknown mode
    both = _lib.OptimHyper(beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.05, clip_value=0.01)
    for mode in (ADAMW, ADAM, SGD):
        assert call(mode, both) == SHAPE                                                      # both clips
    assert call(SGD, _lib.OptimHyper(nesterov=1)) == SHAPE                                    # nesterov without momentum
    assert call(SGD, _lib.OptimHyper(nesterov=1, momentum=-0.5)) == SHAPE
    assert call(SGD, _lib.OptimHyper(nesterov=1, momentum=0.9, dampening=0.1)) == SHAPE        # nesterov with dampening
    for mode, h in ((ADAMW, good), (ADAM, good), (SGD, _lib.OptimHyper(nesterov=1, momentum=0.9))):
        assert call(mode, h, nbytes=ws - 1) == WORKSPACE                                      # short workspace
        assert call(mode, h, nbytes=0, n=0) == OK                                             # nothing to do: no launch
    # the refusals come in the documented order: NULL before the mode, the mode before the workspace
    assert call(3, good, items=None) == NULL and call(3, good, nbytes=0) == SHAPE
    # focus_adamw_step keeps its signature and its own refusals
    assert lib.focus_adamw_step(None, ptr, 1, 1, ptr, ptr, ptr, ws, None, 0.9, 0.999, 1e-8, 0.0, 1, None) == NULL
    assert lib.focus_adamw_step(ptr, ptr, 1, 1, ptr, ptr, ptr, ws - 1, None, 0.9, 0.999, 1e-8, 0.0, 1, None) == WORKSPACE
    assert lib.focus_abi_version() == 2


def test_fused_classes_refuse_what_is_not_built():
    from focus_amd.slowfast.models.optimizer import FusedAdam, FusedSGD
    w = lambda: torch.nn.Parameter(torch.randn(4, 4))
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True)):
        with pytest.raises(NotImplementedError):
            FusedAdam([w()], **kw)
    for kw in (dict(maximize=True), dict(differentiable=True)):
        with pytest.raises(NotImplementedError):
            FusedSGD([w()], momentum=0.9, **kw)
    with pytest.raises(NotImplementedError, match="betas"):
        FusedAdam([{"params": [w()]}, {"params": [w()], "betas": (0.8, 0.999)}])
    with pytest.raises(NotImplementedError, match="betas"):
        FusedAdam([{"params": [w()]}, {"params": [w()], "eps": 1e-6}])
    with pytest.raises(NotImplementedError, match="momentum"):
        FusedSGD([{"params": [w()]}, {"params": [w()], "momentum": 0.5}], momentum=0.9)
    with pytest.raises(NotImplementedError, match="momentum"):
        FusedSGD([{"params": [w()]}, {"params": [w()], "dampening": 0.5}], momentum=0.9)
    # a group edited after construction is judged at the step
    opt = FusedAdam([w()])
    opt.param_groups[0]["amsgrad"] = True
    opt.param_groups[0]["params"][0].grad = torch.zeros(4, 4)
    with pytest.raises(NotImplementedError):
        opt.step()
    # parameters the kernels cannot take: not fp32, not on the GPU, sparse gradients
    for make in (lambda p: FusedAdam([p]), lambda p: FusedSGD([p], momentum=0.9)):
        p = torch.nn.Parameter(torch.randn(4, 4, dtype=torch.float64))
        p.grad = torch.zeros_like(p)
        with pytest.raises(NotImplementedError, match="fp32"):
            make(p).step()
        p = w()
        p.grad = torch.zeros(4, 4).to_sparse()
        with pytest.raises(NotImplementedError):
            make(p).step()
        p = w()
        p.grad = torch.zeros(4, 4)
        with pytest.raises(ValueError, match="exclude"):
            make(p).step_clipped(max_norm=1.0, clip_value=1.0)
    # nothing carries a gradient: nothing to do, nothing refused
    assert FusedSGD([w()], momentum=0.9).step() is None
