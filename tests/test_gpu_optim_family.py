"""focus_optim_step through optimizer.FusedAdam / FusedSGD against torch's own clip_grad_norm_ / clip_grad_value_ +
torch.optim.Adam / SGD on identical parameters and gradients (the sequence of tools/steve_train_net.py:116-126 and
tools/train_net.py:108-120): fp32 arithmetic, 1e-6 relative per tensor over 4 steps (tests/optim_ref.py holds the case and
the measure); the bf16 weight copies, the state_dict interchange with torch's classes, the STEVE parameter set with the
wiring of construct_optimizer_slot / slot_train_step, and FusedAdamW through both entry points."""
import copy

import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

CLIPS = [(0.05, 0.0), (1e9, 0.0), (0.0, 0.0), (0.0, 0.01)]            # (max_norm, clip_value), never both
SGD_RULES = [(0.0, 0.0, False), (0.9, 0.1, False), (0.9, 0.0, True)]   # (momentum, dampening, nesterov)


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _groups(ps):
    return [{"params": [ps[i] for i in idx], "lr": R.LR[gi][0]} for gi, idx in enumerate(R.GROUPS)]


def _state(opt, p, kind):
    s = opt.state.get(p, {})
    return (s.get("exp_avg"), s.get("exp_avg_sq")) if kind == "adam" else (s.get("momentum_buffer"),)


def _make(kind, fused, ps, hyper, foreach=None):
    from focus_amd.slowfast.models.optimizer import FusedAdam, FusedSGD
    if kind == "adam":
        return FusedAdam(_groups(ps), **hyper) if fused else torch.optim.Adam(_groups(ps), foreach=foreach, **hyper)
    return FusedSGD(_groups(ps), **hyper) if fused else torch.optim.SGD(_groups(ps), foreach=foreach, **hyper)


@pytest.fixture(scope="module")
def case():
    """the shared parameters and the four steps of gradients, on the device once"""
    return [p.to(dev()) for p in R.make_params()], [[None if g is None else g.to(dev()) for g in gs] for gs in R.make_grads()]


def _run(kind, fused, hyper, max_norm, clip_value, case):
    """-> per step: (params, .grad as left behind, state tensors, total norm or None)"""
    from focus_amd import ops
    ops.drop_caches()
    ps = [torch.nn.Parameter(p.clone()) for p in case[0]]
    opt = _make(kind, fused, ps, hyper)
    out = []
    for step, gs in enumerate(case[1]):
        for gi, g in enumerate(opt.param_groups):
            g["lr"] = R.LR[gi][step]
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.clone()
        if fused:
            opt.step_clipped(max_norm=max_norm, clip_value=clip_value)
            tn = opt.last_total_norm.clone()
        else:
            tn = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad.double()) for p in ps if p.grad is not None]))
            if clip_value > 0:
                torch.nn.utils.clip_grad_value_(ps, clip_value)
            elif max_norm > 0:
                tn32 = torch.nn.utils.clip_grad_norm_(ps, max_norm)
                assert abs(float(tn32) - float(tn)) <= 1e-6 * float(tn)
            opt.step()
        out.append(([p.detach().clone() for p in ps], [None if p.grad is None else p.grad.clone() for p in ps],
                    [tuple(None if t is None else t.clone() for t in _state(opt, p, kind)) for p in ps], tn))
    return out


def _compare(kind, hyper, max_norm, clip_value, case):
    want = _run(kind, False, hyper, max_norm, clip_value, case)
    got = _run(kind, True, hyper, max_norm, clip_value, case)
    again = _run(kind, True, hyper, max_norm, clip_value, case)
    worst = {"norm": 0.0, "param": 0.0, "grad": 0.0, "state": 0.0}
    for step in range(R.STEPS):
        (wp, wg, ws, wn), (gp, gg, gs, gn), (ap, ag, as_, an) = want[step], got[step], again[step]
        e = abs(float(gn) - float(wn)) / float(wn)
        worst["norm"] = max(worst["norm"], e)
        assert e <= 2e-6, "step %d: last_total_norm %.9g, torch %.9g" % (step, float(gn), float(wn))
        assert torch.equal(gn, an)
        for i in range(len(wp)):
            tag = "step %d tensor %d %s" % (step, i, R.SHAPES[i])
            e = R.rel(gp[i], wp[i], R.P_FLOOR)
            worst["param"] = max(worst["param"], e)
            assert e <= 1e-6, tag
            assert torch.equal(gp[i], ap[i]), tag + ": two identical runs differ"
            assert (gg[i] is None) == (wg[i] is None)
            if wg[i] is not None:
                e = R.rel(gg[i], wg[i])
                worst["grad"] = max(worst["grad"], e)
                assert e <= 2e-6, "%s grad %.3e" % (tag, e)
                assert torch.equal(gg[i], ag[i]), tag
                if clip_value > 0:        # what clip_grad_value_ leaves in .grad, bit for bit
                    assert torch.equal(gg[i], case[1][step][i].clamp(min=-clip_value, max=clip_value)), tag
                    assert torch.equal(gg[i], wg[i]), tag
            assert len(gs[i]) == len(ws[i])
            for g_, w_, a_ in zip(gs[i], ws[i], as_[i]):
                assert (g_ is None) == (w_ is None), tag + ": state presence differs from torch's"
                if w_ is not None:
                    e = R.rel(g_, w_)
                    worst["state"] = max(worst["state"], e)
                    assert e <= 1e-6, tag
                    assert torch.equal(g_, a_), tag
    print("%s %s clip %s: worst relative distances %s" % (kind, hyper, (max_norm, clip_value), worst))
    # lr = 0.0 on the first step: the moments / buffers moved, the parameters did not
    for i in R.GROUPS[1]:
        if case[1][0][i] is not None:
            assert torch.equal(got[0][0][i], case[0][i])
            if kind == "adam" or hyper["momentum"] > 0:
                assert float(got[0][2][i][0].abs().max()) > 0
    return got


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("weight_decay", [0.0, 5e-2])
def test_fused_adam_matches_torch(weight_decay, clip, case):
    _compare("adam", dict(weight_decay=weight_decay), clip[0], clip[1], case)


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("rule", SGD_RULES)
def test_fused_sgd_matches_torch(rule, clip, case):
    got = _compare("sgd", dict(momentum=rule[0], dampening=rule[1], nesterov=rule[2], weight_decay=1e-4), clip[0], clip[1], case)
    if rule[0] == 0.0:
        assert all(s == (None,) for s in got[-1][2])                  # no momentum, no buffer: torch keeps no state either


# ------------------------------------------------------------------------------------------------
# the bf16 weight copies
# ------------------------------------------------------------------------------------------------
W_SHAPES = [(64, 68), (132, 68), (6, 10), (4100,)]       # a tiled weight, a second one of the same width, a non-tiled one, a vector


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_weight_copies_are_written_by_the_step(kind):
    from focus_amd import ops
    from focus_amd.slowfast.models.optimizer import FusedAdam, FusedSGD
    ops.drop_caches()
    g = torch.Generator(device="cpu").manual_seed(1)
    ws = [torch.nn.Parameter((torch.randn(*s, generator=g) * 0.05).to(dev())) for s in W_SHAPES]
    bf = torch.bfloat16
    sh = [(ws[0], ops.shadow(ws[0], bf), ops.shadow(ws[0], bf, transposed=True)),     # as after a forward / backward
          (ws[1], ops.shadow(ws[1], bf), None),
          (ws[2], ops.shadow(ws[2], bf), None)]
    stacked = ops.stacked_weights([ws[0], ws[1]], bf)                                    # [64 + 132, 68]
    ptr = stacked.data_ptr()
    opt = FusedAdam(ws, lr=3e-3, weight_decay=5e-2) if kind == "adam" else FusedSGD(ws, lr=3e-2, momentum=0.9, weight_decay=1e-4)
    x = (torch.randn(8, 68, generator=g) * 0.5).to(dev()).to(bf)
    for step in range(2):
        for w in ws:
            w.grad = (torch.randn(*w.shape, generator=g) * 0.3).to(dev())
        before = [w.detach().clone() for w in ws]
        opt.step_clipped(max_norm=0.05)
        assert all(not torch.equal(b, w.detach()) for b, w in zip(before, ws))
        for w, d, dT in sh:
            assert torch.equal(d, w.detach().to(bf)), "row-major shadow is not the rounded master"
            assert ops.shadow(w, bf) is d, "the shadow written by the step must be the fresh one"
            if dT is not None:
                assert torch.equal(dT, w.detach().to(bf).t().contiguous())
                assert ops.shadow(w, bf, transposed=True) is dT
        st = ops.stacked_weights([ws[0], ws[1]], bf)
        assert st is stacked and st.data_ptr() == ptr, "the stacked operand must be rebuilt in place"
        assert torch.equal(st, torch.cat([ws[0].detach().to(bf), ws[1].detach().to(bf)], dim=0))
        # ... and the two projections of one input are the products of the NEW weights (bf16 outputs: 2^-8 of the largest)
        k, v = ops.linear_kv(x, ws[0], ws[1])
        for y, w in ((k, ws[0]), (v, ws[1])):
            want = x.double() @ w.detach().to(bf).double().t()
            assert float((y.detach().double() - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())


# ------------------------------------------------------------------------------------------------
# state_dict interchange with torch's classes
# ------------------------------------------------------------------------------------------------
def _interchange(kind, hyper, case, scale=1.0):
    """two steps in one class -> state_dict -> the other class -> one more step on each side"""
    from focus_amd import ops
    for first_fused in (False, True):
        ops.drop_caches()
        pa = [torch.nn.Parameter(p.clone()) for p in case[0]]
        pb = [torch.nn.Parameter(p.clone()) for p in case[0]]
        a = _make(kind, first_fused, pa, hyper)
        for step in range(2):
            for gi, g in enumerate(a.param_groups):
                g["lr"] = R.LR[gi][step] * scale
            for p, g in zip(pa, case[1][step]):
                p.grad = None if g is None else g.clone()
            a.step()
        sd = copy.deepcopy(a.state_dict())            # (state_dict() hands out the live tensors: a file would not share them)
        if not first_fused and kind == "adam":                       # a torch checkpoint as torch.load(map_location="cpu") hands it over
            for s in sd["state"].values():
                assert s["step"].device.type == "cpu"
        b = _make(kind, not first_fused, pb, hyper, foreach=False)      # (its step counters may sit on two devices now)
        ref_sd = b.state_dict()
        assert sd["param_groups"][0].keys() == ref_sd["param_groups"][0].keys()
        b.load_state_dict(sd)
        with torch.no_grad():
            for p, q in zip(pa, pb):
                q.copy_(p)
        for opt, ps in ((a, pa), (b, pb)):
            for gi, g in enumerate(opt.param_groups):
                g["lr"] = R.LR[gi][3] * scale
            for p, g in zip(ps, case[1][3]):
                p.grad = g.clone()
            opt.step()
        for i, (p, q) in enumerate(zip(pa, pb)):
            assert R.rel(q.detach(), p.detach(), R.P_FLOOR) <= 1e-6, (first_fused, i)
            assert float((q.detach() - case[0][i]).abs().max()) > 0
        sa, sb = a.state_dict(), b.state_dict()
        assert sa["state"].keys() == sb["state"].keys()
        for k in sa["state"]:
            assert sa["state"][k].keys() == sb["state"][k].keys()
            for name, t in sa["state"][k].items():
                u = sb["state"][k][name]
                if name == "step":
                    assert float(t) == float(u)
                elif t is None:
                    assert u is None
                else:
                    assert R.rel(u, t) <= 1e-6, (first_fused, k, name)


def test_adam_state_moves_between_torch_and_fused(case):
    _interchange("adam", dict(weight_decay=5e-2), case)


@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_sgd_state_moves_between_torch_and_fused(momentum, case):
    _interchange("sgd", dict(momentum=momentum, dampening=0.1 if momentum else 0.0, weight_decay=1e-4), case, scale=10.0)


def test_sgd_buffer_from_a_checkpoint_is_not_new(case):
    """The first step after load_state_dict dampens: a loaded buffer has been used before."""
    from focus_amd.slowfast.models.optimizer import FusedSGD
    hyper = dict(lr=0.1, momentum=0.9, dampening=0.5)
    p = torch.nn.Parameter(case[0][0].clone())
    q = torch.nn.Parameter(case[0][0].clone())
    a, b = FusedSGD([p], **hyper), FusedSGD([q], **hyper)
    g = case[1][0][0]
    p.grad = g.clone()
    a.step()
    assert torch.equal(a.state[p]["momentum_buffer"], g)                             # first use: the gradient as it is
    b.load_state_dict(a.state_dict())
    with torch.no_grad():
        q.copy_(p)
    q.grad = g.clone()
    b.step()
    want = 0.9 * g + 0.5 * g
    assert R.rel(b.state[q]["momentum_buffer"], want) <= 1e-6


# ------------------------------------------------------------------------------------------------
# the STEVE parameter set and the wiring of the slot loop
# ------------------------------------------------------------------------------------------------
def _steve_small():
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.models import MODEL_REGISTRY
    cfg = get_cfg()
    cfg.MODEL.MODEL_NAME = "STEVE"
    cfg.NUM_GPUS = 1
    cfg.TRAIN.MIXED_PRECISION = True
    cfg.SOLVER.OPTIMIZING_METHOD = "adam"
    cfg.SOLVER.CLIP_GRAD_L2NORM = 0.05
    cfg.SLOTS_OPTIM.WARMUP_STEPS, cfg.SLOTS_OPTIM.TAU_STEPS, cfg.SLOTS_OPTIM.HALF_LIFE = 10, 20, 50
    s = cfg.SLOTS
    s.NUM_ITERS, s.NUM_SLOTS, s.CNN_HID_SIZE, s.SIZE, s.DIM, s.MLP_HID_SIZE, s.IMG_SIZE, s.VOCAB_SIZE = 2, 3, 16, 16, 32, 32, 16, 32
    s.NUM_PREDICTOR_BLOCKS, s.NUM_PREDICTOR_HEADS = 1, 2
    s.DECODER.DIM, s.DECODER.NUM_BLOCKS, s.DECODER.NUM_HEADS = 32, 2, 2
    torch.manual_seed(3)
    return cfg, MODEL_REGISTRY.get("STEVE")(cfg).to(dev()).train()


def test_steve_parameter_set_and_slot_loop_wiring(monkeypatch):
    from focus_amd import ops
    from focus_amd.slowfast.models import optimizer as optim
    from focus_amd.train import slot_train_step
    monkeypatch.delenv("FOCUS_FUSED_OPT", raising=False)
    ops.drop_caches()
    cfg, m = _steve_small()
    opt = optim.construct_optimizer_slot(m, cfg)
    assert type(opt) is optim.FusedAdam and len(opt.param_groups) == 3
    assert optim.fused_route(m, opt)
    video = torch.rand(2, 2, 3, 16, 16, generator=torch.Generator().manual_seed(0)).to(dev())
    # one forward / backward of the slot loop (it creates the shadows), then the two sequences on the same numbers
    optim.set_slot_lr(opt, cfg, 0.9, 0.3, 0.3)
    recon, ce, mse, attns = m(video, 1.0, cfg.SLOTS.HARD)
    (mse.mean() + ce.mean()).backward()
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    copies = [torch.nn.Parameter(p.detach().clone()) for _, p in named]
    for c, (_, p) in zip(copies, named):
        c.grad = None if p.grad is None else p.grad.detach().clone().float()
    assert sum(c.grad is not None for c in copies) > 50             # (a few hundred small tensors at full size)
    idx = {id(p): i for i, (_, p) in enumerate(named)}
    ref = torch.optim.Adam([{"params": [copies[idx[id(p)]] for p in g["params"] if id(p) in idx], "lr": g["lr"]} for g in opt.param_groups])
    tn = torch.nn.utils.clip_grad_norm_(copies, cfg.SOLVER.CLIP_GRAD_L2NORM)
    ref.step()
    opt.step_clipped(max_norm=cfg.SOLVER.CLIP_GRAD_L2NORM)
    assert abs(float(opt.last_total_norm) - float(tn)) <= 2e-6 * float(tn)
    worst = 0.0
    for c, (n, p) in zip(copies, named):
        e = R.rel(p.detach(), c.detach(), R.P_FLOOR)
        worst = max(worst, e)
        assert e <= 1e-6, n
    print("STEVE parameter set: %d tensors, worst %.3e" % (len(named), worst))
    # the loop itself: two steps, finite loss, every group moves
    before = {n: p.detach().clone() for n, p in named}
    for step in range(2):
        loss = slot_train_step(m, opt, video, step, cfg)[0]
        assert torch.isfinite(loss)
    moved = {n.split(".")[0] for n, p in named if not torch.equal(p.detach(), before[n])}
    assert moved == {"dvae", "steve_encoder", "steve_decoder"}
    assert opt.last_total_norm is not None and float(opt.state[named[0][1]]["step"]) == 3.0
    # switched off: torch's class, as before
    monkeypatch.setenv("FOCUS_FUSED_OPT", "0")
    assert type(optim.construct_optimizer_slot(m, cfg)) is torch.optim.Adam
    cfg.SOLVER.OPTIMIZING_METHOD = "sgd"
    assert type(optim.construct_optimizer_slot(m, cfg)) is torch.optim.SGD
    monkeypatch.delenv("FOCUS_FUSED_OPT")
    assert type(optim.construct_optimizer_slot(m, cfg)) is optim.FusedSGD
    # an optimizer that does not hold every trainable parameter measures another norm: no fused route
    part = optim.FusedAdam([p for n, p in named if "dvae" in n])
    assert not optim.fused_route(m, part)


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(20, 12)

    def forward(self, inputs, meta=None):
        return self.fc(inputs[0])


@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_train_step_routes(method):
    """construct_optimizer builds the fused classes for a model on the GPU and train_step hands them the clipping
    (CLIP_GRAD_L2NORM and CLIP_GRAD_VAL); a gradient-carrying parameter outside the groups sends it down the unfused
    sequence, whose norm counts that parameter too."""
    from focus_amd import ops
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.models import optimizer as optim
    from focus_amd.train import train_step
    ops.drop_caches()
    cfg = get_cfg()
    cfg.SOLVER.OPTIMIZING_METHOD, cfg.SOLVER.BASE_LR, cfg.SOLVER.WEIGHT_DECAY, cfg.SOLVER.MOMENTUM = method, 0.01, 1e-4, 0.9
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(16, 20, generator=g).to(dev()), torch.randint(0, 12, (16,), generator=g).to(dev())
    loss_fun = torch.nn.CrossEntropyLoss()
    torch.manual_seed(0)
    proto = _Tiny().to(dev())

    def twin():
        t = _Tiny().to(dev())
        t.load_state_dict(proto.state_dict())
        return t

    def torch_opt(params):
        if method == "sgd":
            return torch.optim.SGD(params, lr=0.01, momentum=0.9, weight_decay=1e-4, nesterov=True)    # SOLVER.NESTEROV
        return torch.optim.Adam(params, lr=0.01, weight_decay=1e-4)

    for clip_norm, clip_val in ((0.05, None), (None, 0.01)):
        cfg.SOLVER.CLIP_GRAD_L2NORM, cfg.SOLVER.CLIP_GRAD_VAL = clip_norm, clip_val
        # every parameter in the groups: the fused route
        m, r = twin(), twin()
        opt = optim.construct_optimizer(m, cfg)
        assert type(opt) is (optim.FusedSGD if method == "sgd" else optim.FusedAdam) and optim.fused_route(m, opt)
        ropt = torch_opt([{"params": [r.fc.weight]}, {"params": [r.fc.bias]}])
        for _ in range(2):
            opt.last_total_norm = None
            train_step(m, opt, loss_fun, [x], y, None, cfg)
            assert opt.last_total_norm is not None
            ropt.zero_grad()
            loss_fun(r([x]), y).backward()
            if clip_val:
                torch.nn.utils.clip_grad_value_(r.parameters(), clip_val)
            else:
                tn = torch.nn.utils.clip_grad_norm_(r.parameters(), clip_norm)
                assert abs(float(opt.last_total_norm) - float(tn)) <= 2e-6 * float(tn)
            ropt.step()
        for p, q in zip(m.parameters(), r.parameters()):
            assert R.rel(p.detach(), q.detach(), R.P_FLOOR) <= 1e-6
        # the bias outside the groups: clip_grad_norm_(model.parameters()) counts it, so does this route
        m, r = twin(), twin()
        cls = optim.FusedSGD if method == "sgd" else optim.FusedAdam
        opt = cls([m.fc.weight], lr=0.01, weight_decay=1e-4, **({"momentum": 0.9, "nesterov": True} if method == "sgd" else {}))
        assert not optim.fused_route(m, opt)
        ropt = torch_opt([r.fc.weight])
        train_step(m, opt, loss_fun, [x], y, None, cfg)
        loss_fun(r([x]), y).backward()
        if clip_val:
            torch.nn.utils.clip_grad_value_(r.parameters(), clip_val)
        else:
            tn = torch.nn.utils.clip_grad_norm_(r.parameters(), clip_norm)
            assert float(opt.last_total_norm) < float(tn)            # the step saw the weight's clipped gradient alone
        ropt.step()
        assert R.rel(m.fc.weight.detach(), r.fc.weight.detach(), R.P_FLOOR) <= 1e-6
        assert torch.equal(m.fc.bias.detach(), proto.fc.bias.detach())
        assert R.rel(m.fc.bias.grad, r.fc.bias.grad) <= 2e-6         # ... and the bias's gradient was clipped with the rest


# ------------------------------------------------------------------------------------------------
# what exists keeps its bits
# ------------------------------------------------------------------------------------------------
def _adamw_case(case):
    pa = [torch.nn.Parameter(p.clone()) for p in case[0]]
    groups = [{"params": [p for p in pa if p.dim() > 1], "weight_decay": 5e-2},
              {"params": [p for p in pa if p.dim() <= 1], "weight_decay": 0.0}]
    from focus_amd.slowfast.models.optimizer import FusedAdamW
    return pa, FusedAdamW(groups, lr=3e-3, eps=1e-8)


def test_fused_adamw_is_the_same_through_both_entries(case):
    """focus_adamw_step is focus_optim_step in mode ADAMW: parameters, moments and the clipped gradients agree bit for bit
    after 3 steps.  The second optimizer's tables go to the C entry directly."""
    import ctypes
    from focus_amd import _lib, ops
    ops.drop_caches()
    (pa, a), (pb, b) = _adamw_case(case), _adamw_case(case)
    L = _lib.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    for step in range(3):
        for p, q, g in zip(pa, pb, case[1][step]):
            p.grad = None if g is None else g.clone()
            q.grad = None if g is None else g.clone()
        a.step_clipped(0.05)
        b._prepare()
        tab, norm = b._table, b._ws[-1:]
        h = _lib.OptimHyper(beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.05, write_clipped_grads=1)
        _lib.check(L.focus_optim_step(0, vp(tab["items"]), vp(tab["gptrs"]), len(tab["entries"]), tab["units"], vp(b._groups[1]),
                                      vp(tab["steps"]), vp(b._ws), (b._ws.numel() - 1) * 4, vp(norm), ctypes.byref(h),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "optim_step")
        assert torch.equal(a.last_total_norm, norm[0])
    for i, (p, q) in enumerate(zip(pa, pb)):
        assert torch.equal(p.detach(), q.detach()), i
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad), i
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(a.state[p][k], b.state[q][k]), (i, k)


def test_fused_adamw_keeps_the_bits_of_the_kernel_it_replaced(case):
    """tests/golden/adamw_step_bits.npz holds parameters and moments after 3 clipped steps of this case as the AdamW kernel
    gave them before it became one instantiation of the family's template (recorded on an MI355X)."""
    import os
    import numpy as np
    from conftest import ROOT
    from focus_amd import ops
    ops.drop_caches()
    z = np.load(os.path.join(ROOT, "tests", "golden", "adamw_step_bits.npz"))
    pa, a = _adamw_case(case)
    for step in range(3):
        for p, g in zip(pa, case[1][step]):
            p.grad = None if g is None else g.clone()
        a.step_clipped(0.05)
    for i, p in enumerate(pa):
        for name, t in (("p", p.detach()), ("m", a.state[p]["exp_avg"]), ("v", a.state[p]["exp_avg_sq"])):
            assert np.array_equal(t.cpu().numpy().view(np.uint32), z["%s%d" % (name, i)].view(np.uint32)), (name, i)


# ------------------------------------------------------------------------------------------------
# channels-last convolution weights (STEVE's dVAE and CNN): the update runs in storage order
# ------------------------------------------------------------------------------------------------
CL_SHAPES = [(16, 3, 4, 4), (8, 8, 3, 3), (12, 20)]


def _cl_params():
    g = torch.Generator(device="cpu").manual_seed(2)
    ps = [(torch.randn(*s, generator=g) * 0.05).to(dev()) for s in CL_SHAPES]
    return [torch.nn.Parameter(p.contiguous(memory_format=torch.channels_last) if p.dim() == 4 else p) for p in ps]


def _cl_grads(step):
    """gradients in the parameter's layout on odd steps and in the plain one on even steps (autograd may hand back either)"""
    g = torch.Generator(device="cpu").manual_seed(20 + step)
    gs = [(torch.randn(*s, generator=g) * 0.3).to(dev()) for s in CL_SHAPES]
    return [x.contiguous(memory_format=torch.channels_last) if x.dim() == 4 and step % 2 else x for x in gs]


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_channels_last_parameters_match_torch_and_take_a_checkpoint_in_another_layout(kind):
    from focus_amd import ops
    from focus_amd.slowfast.models.optimizer import FusedAdam, FusedSGD
    ops.drop_caches()
    hyper = dict(lr=2e-3, weight_decay=5e-2) if kind == "adam" else dict(lr=2e-2, momentum=0.9, dampening=0.1, weight_decay=1e-4)
    make = lambda ps, fused: ((FusedAdam if fused else torch.optim.Adam) if kind == "adam" else
                              (FusedSGD if fused else torch.optim.SGD))(ps, **hyper)
    pa, pb = _cl_params(), _cl_params()
    assert not pa[0].is_contiguous()
    ref, fus = make(pa, False), make(pb, True)
    for step in range(3):
        for p, q, g in zip(pa, pb, _cl_grads(step)):
            p.grad, q.grad = g.clone(), g.clone()
        tn = torch.nn.utils.clip_grad_norm_(pa, 0.05)
        ref.step()
        fus.step_clipped(max_norm=0.05)
        assert abs(float(fus.last_total_norm) - float(tn)) <= 2e-6 * float(tn)
        for i, (p, q) in enumerate(zip(pa, pb)):
            assert q.stride() == p.stride()
            assert R.rel(q.detach(), p.detach(), R.P_FLOOR) <= 1e-6, (step, i)
            assert R.rel(q.grad, p.grad) <= 2e-6, (step, i)
            for t, u in zip(_state(ref, p, kind), _state(fus, q, kind)):
                assert R.rel(u, t) <= 1e-6, (step, i)
    # a checkpoint whose moments / buffers lie in the plain layout (and on the CPU) loads and keeps stepping like torch
    sd = copy.deepcopy(ref.state_dict())
    for s in sd["state"].values():
        for k, t in s.items():
            if torch.is_tensor(t) and t.dim() == 4:
                s[k] = t.contiguous().cpu()
                assert s[k].is_contiguous()
    pc = _cl_params()
    with torch.no_grad():
        for p, q in zip(pa, pc):
            q.copy_(p)
    fus2 = make(pc, True)
    fus2.load_state_dict(sd)
    for p, q, g in zip(pa, pc, _cl_grads(3)):
        p.grad, q.grad = g.clone(), g.clone()
    ref.step()
    fus2.step()
    for i, (p, q) in enumerate(zip(pa, pc)):
        assert R.rel(q.detach(), p.detach(), R.P_FLOOR) <= 1e-6, i
        for t, u in zip(_state(ref, p, kind), _state(fus2, q, kind)):
            assert u.stride() == q.stride() and R.rel(u, t) <= 1e-6, i
