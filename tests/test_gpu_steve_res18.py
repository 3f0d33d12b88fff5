"""STEVE's ResNet-18 trunk (MODEL.CNN_NAME = res18) on the HIP BatchNorm / max-pool kernels, and the model around it.

  fp32 trunk: Res18Block on the GPU at 2 frames of 3x16x16 against the fp64 CPU restatement of tests/bn_ref.py with the same
    weights: the output and all 18 gradients, norm-wise relative error per tensor, no element left out, bound 1e-3 (the
    project's fp32 parity bound, README.md).  One of the 18 has an exact value of ZERO: conv1.bias shifts the input of a
    training-mode BatchNorm, which removes the shift, so its gradient is a sum that cancels completely and the reference holds
    rounding noise only.  Its error is taken relative to the norm of the sum of the ABSOLUTE terms (what a sum of that size is
    accurate to) -- the only reading under which a relative error of that tensor says anything.
  bf16 trunk: the yardstick is the FOCUS_STEVE_BN=0 path (ATen BatchNorm / max-pool on the same bf16 convolutions) against
    fp64, measured in the same test; the HIP path's error has to be within 2x of it per tensor.  Both columns are printed.
  STEVE with res18 (IMG_SIZE 64, B = 1, T = 2, small vocabulary, 1 decoder block): forward, one slot_train_step, running
    statistics against the fp64 update of the trunk's own batch (bounds of bn_ref.py), dead parameters untouched, eval mode
    bit-repeatable and different from training mode, reconstruct_autoregressive, state_dict round trip."""
import types

import pytest
import torch

import bn_ref as br
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64


def _trunk(hip, d_model=32):
    from focus_amd.slowfast.models.STEVE.steve import Res18Block
    args = types.SimpleNamespace(SLOTS=types.SimpleNamespace(IMG_CHANNELS=3, CNN_HID_SIZE=64, IMG_SIZE=64,
                                                             DECODER=types.SimpleNamespace(DIM=d_model)))
    torch.manual_seed(0)
    m = Res18Block(args)
    m.hip_bn = hip
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for mod in m.fenc.modules():                                  # BatchNorm away from its 1 / 0 initialisation
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.copy_(1 + 0.3 * torch.randn(64, generator=g))
                mod.bias.copy_(0.3 * torch.randn(64, generator=g))
    return m


def _live(m):
    return {n: p for n, p in m.named_parameters() if not n.startswith(("res18.layer2", "res18.layer3", "res18.layer4", "res18.fc"))}


def _reference(m, x, ct):
    """The fp64 restatement with m's weights -> output, the 18 gradients, and the scale of conv1.bias's cancelling sum."""
    ref = br.Res18Restated(3, m.upconv.out_channels).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in m.state_dict().items()}, strict=True)
    ref.train()
    keep = {}

    def hook(mod, i, o):
        o.retain_grad()
        keep["conv1"] = o

    h = ref.res18.conv1.register_forward_hook(hook)
    y = ref(x.double().cpu())
    (y * ct.double().cpu()).sum().backward()
    h.remove()
    grads = {n: p.grad for n, p in _live(ref).items()}
    assert len(grads) == br.N_LIVE and all(g is not None for g in grads.values())
    return y.detach(), grads, keep["conv1"].grad.abs().sum(dim=(0, 2, 3))


def _run(m, x, ct, autocast):
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        y = m(x)
    (y.float() * ct).sum().backward()
    return y.detach(), {n: p.grad for n, p in _live(m).items()}


def _errors(y, grads, y_ref, g_ref, bias_scale):
    e = {"output": float((y.double().cpu() - y_ref).norm() / y_ref.norm())}
    for n, g in g_ref.items():
        den = bias_scale.norm() if n == "res18.conv1.bias" else g.norm()
        e[n] = float((grads[n].double().cpu() - g).norm() / den)
    return e


def _inputs(d):
    g = torch.Generator().manual_seed(2)
    x = torch.rand(2, 3, 16, 16, generator=g).to(d).contiguous(memory_format=torch.channels_last)
    ct = torch.randn(2, 32, 16, 16, generator=g).to(d)
    return x, ct


def test_trunk_fp32_against_the_fp64_restatement():
    d = dev()
    m = _trunk(True).to(d).to(memory_format=torch.channels_last).train()
    x, ct = _inputs(d)
    y_ref, g_ref, scale = _reference(m, x, ct)
    y, grads = _run(m, x, ct, autocast=False)
    assert tuple(y.shape) == (2, 32, 16, 16) and y.dtype == F32
    dead = [p for n, p in m.named_parameters() if n not in _live(m)]
    assert len(dead) == br.N_DEAD and all(p.grad is None for p in dead)
    e = _errors(y, grads, y_ref, g_ref, scale)
    for n in sorted(e):
        print("fp32 trunk  %-34s %.3e" % (n, e[n]))
    assert len(e) == 1 + br.N_LIVE
    bad = {n: v for n, v in e.items() if not v <= 1e-3}
    assert not bad, bad


def test_trunk_bf16_is_within_2x_of_the_aten_path():
    d = dev()
    x, ct = _inputs(d)
    cols = {}
    for hip in (False, True):
        m = _trunk(hip).to(d).to(memory_format=torch.channels_last).train()
        if not cols:
            y_ref, g_ref, scale = _reference(m, x, ct)
        y, grads = _run(m, x, ct, autocast=True)
        assert y.dtype == BF16
        cols[hip] = _errors(y, grads, y_ref, g_ref, scale)
    for n in sorted(cols[True]):
        print("bf16 trunk  %-34s hip %.3e   aten %.3e   ratio %.2f" % (n, cols[True][n], cols[False][n], cols[True][n] / cols[False][n]))
    bad = {n: (cols[True][n], cols[False][n]) for n in cols[True] if not cols[True][n] <= 2 * cols[False][n]}
    assert not bad, bad


# ---- the model ------------------------------------------------------------------------------------------------------------
def _steve_res18(mixed):
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.models import MODEL_REGISTRY
    cfg = get_cfg()
    cfg.MODEL.MODEL_NAME, cfg.MODEL.CNN_NAME = "STEVE", "res18"
    cfg.NUM_GPUS = 1
    cfg.TRAIN.MIXED_PRECISION = mixed
    s = cfg.SLOTS
    s.NUM_ITERS, s.NUM_SLOTS, s.CNN_HID_SIZE, s.SIZE, s.DIM, s.MLP_HID_SIZE, s.IMG_SIZE, s.VOCAB_SIZE = 2, 3, 64, 16, 32, 32, 64, 32
    s.NUM_PREDICTOR_BLOCKS, s.NUM_PREDICTOR_HEADS = 1, 2
    s.DECODER.DIM, s.DECODER.NUM_BLOCKS, s.DECODER.NUM_HEADS = 32, 1, 2
    cfg.SOLVER.OPTIMIZING_METHOD = "adam"
    cfg.SOLVER.CLIP_GRAD_L2NORM = 1.0
    cfg.SLOTS_OPTIM.WARMUP_STEPS, cfg.SLOTS_OPTIM.TAU_STEPS, cfg.SLOTS_OPTIM.HALF_LIFE = 10, 20, 50
    torch.manual_seed(0)
    return cfg, MODEL_REGISTRY.get("STEVE")(cfg)


def _noise(d, B=1, T=2):
    g = torch.Generator().manual_seed(3)
    e = lambda: torch.empty(B * T, 32, 16, 16).exponential_(generator=g).to(d)
    return {"gumbel_soft": e(), "gumbel_hard": e(), "slots": torch.randn(B, 3, 16, generator=g).to(d)}


@pytest.mark.parametrize("mixed", [False, True], ids=["fp32", "bf16"])
def test_steve_res18_trains(mixed):
    from focus_amd.slowfast.models.optimizer import construct_optimizer_slot
    from focus_amd.train import slot_train_step
    d = dev()
    cfg, m = _steve_res18(mixed)
    m = m.to(d).train()
    cnn = m.steve_encoder.cnn
    assert cnn.hip_bn
    video = torch.rand(1, 2, 3, 64, 64, generator=torch.Generator().manual_seed(4)).to(d)
    recon, ce, mse, attns = m(video, 1.0, False)
    assert tuple(recon.shape) == (1, 2, 3, 64, 64) and tuple(attns.shape) == (1, 2, 3, 3, 64, 64)
    assert bool(torch.isfinite(ce).all()) and bool(torch.isfinite(mse).all())
    assert int(cnn.res18.bn1.num_batches_tracked) == 1

    opt = construct_optimizer_slot(m, cfg)
    names = dict(m.named_parameters())
    dead = {n: p for n, p in names.items() if ".cnn.res18.layer" in n and ".layer1." not in n or ".cnn.res18.fc." in n}
    assert len(dead) == br.N_DEAD
    before = {n: p.detach().clone() for n, p in names.items()}
    run0 = (cnn.res18.bn1.running_mean.clone(), cnn.res18.bn1.running_var.clone())
    seen = {}
    h = cnn.res18.conv1.register_forward_hook(lambda mod, i, o: seen.__setitem__("conv1", o.detach().clone()))
    loss, *_ = slot_train_step(m, opt, video, 5, cfg)
    h.remove()
    assert bool(torch.isfinite(loss))
    assert all(p.grad is None for p in dead.values())
    assert all(torch.equal(p.detach(), before[n]) for n, p in dead.items()), "a dead parameter moved"
    live_cnn = [n for n in names if ".cnn." in n and n not in dead]
    assert len(live_cnn) == br.N_LIVE and all(names[n].grad is not None for n in live_cnn)
    # (conv1.bias is left out of this one: its exact gradient is zero, see the module docstring)
    assert all(not torch.equal(names[n].detach(), before[n]) for n in live_cnn if not n.endswith("res18.conv1.bias")), \
        "a live trunk parameter did not move"
    assert int(cnn.res18.bn1.num_batches_tracked) == 2 and int(cnn.res18.layer2[0].bn1.num_batches_tracked) == 0
    assert float(cnn.res18.layer2[0].bn1.running_mean.abs().max()) == 0.0

    # the running statistics of bn1 are the fp64 update of the batch the trunk itself saw (the stored conv1 output)
    o = seen["conv1"]
    assert o.dtype == (BF16 if mixed else F32)
    rows = o.permute(0, 2, 3, 1).reshape(-1, 64)
    sb = br.stats_bounds(rows, cnn.res18.bn1.eps)
    rm_ref, rv_ref, bm, bv = br.running_bounds(run0[0], run0[1], sb, rows.shape[0], cnn.res18.bn1.momentum)
    rm_err = float(((cnn.res18.bn1.running_mean.double() - rm_ref).abs() / bm).max())
    rv_err = float(((cnn.res18.bn1.running_var.double() - rv_ref).abs() / bv).max())
    print("steve res18 %s: running_mean error / bound %.3f  running_var %.3f" % ("bf16" if mixed else "fp32", rm_err, rv_err))
    assert rm_err <= 1.0 and rv_err <= 1.0


def test_steve_res18_eval_generation_and_state_dict():
    d = dev()
    cfg, m = _steve_res18(False)
    m = m.to(d)
    cnn = m.steve_encoder.cnn
    video = torch.rand(1, 2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(d)
    noise = _noise(d)
    m.train()
    with torch.no_grad():
        for _ in range(2):                                            # move the running statistics off their initial 0 / 1
            trunk_train = cnn(m._frames(video))
        train_out = m(video, 1.0, False, noise=noise)
    m.eval()
    stats = [b.clone() for b in cnn.buffers()]
    with torch.no_grad():
        trunk_eval = cnn(m._frames(video))
        a = m(video, 1.0, False, noise=noise)
        b = m(video, 1.0, False, noise=noise)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "eval forward is not bit-repeatable"
    assert all(torch.equal(x, y) for x, y in zip(stats, cnn.buffers())), "eval mode moved a BatchNorm buffer"
    assert not torch.equal(trunk_eval, trunk_train) and not torch.equal(a[0], train_out[0])
    with torch.no_grad():
        rec = m.reconstruct_autoregressive(video)
    assert tuple(rec.shape) == (1, 2, 3, 64, 64) and float(rec.min()) >= 0.0 and float(rec.max()) <= 1.0
    # state_dict round trip: a fresh model that loads it strictly computes the same bits
    _, m2 = _steve_res18(False)
    m2.load_state_dict(m.state_dict(), strict=True)
    m2 = m2.to(d).eval()
    with torch.no_grad():
        c = m2(video, 1.0, False, noise=noise)
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    # eval-mode gradients flow (frozen statistics) and leave the buffers alone
    y = cnn(m._frames(video))
    y.square().mean().backward()
    assert cnn.res18.bn1.weight.grad is not None and bool(torch.isfinite(cnn.res18.conv1.weight.grad).all())
