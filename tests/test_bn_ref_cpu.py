"""tests/bn_ref.py checked without a GPU: the fp64 references against torch.nn.functional and autograd, an fp32 twin of every
stage inside the derived bounds and every mutant outside them, the in-tree ResNet-18 trunk of STEVE (construction, state_dict
keys, aliasing, live and dead parameters, strict loading both ways), and the refusals of csrc/batchnorm.hip's entry points."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import bn_ref as br

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64


@pytest.fixture(scope="module")
def built():
    from focus_amd.build import build
    return build(verbose=False)


def _close(a, b, tol=1e-10):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def _ratio(err, bound):
    return float((err.abs() / bound.clamp_min(1e-300)).max())


def test_references_are_torch_in_fp64():
    g = torch.Generator().manual_seed(3)
    for N, C, H, W, relu, res in ((2, 8, 3, 5, False, False), (3, 16, 4, 4, True, True), (1, 8, 1, 2, True, False)):
        x = torch.randn(N, C, H, W, generator=g, dtype=F64).requires_grad_()
        r = torch.randn(N, C, H, W, generator=g, dtype=F64).requires_grad_()
        gamma, beta = (torch.randn(C, generator=g, dtype=F64).requires_grad_() for _ in range(2))
        rm, rv = torch.randn(C, generator=g, dtype=F64), torch.rand(C, generator=g, dtype=F64) + 0.5
        ct = torch.randn(N, C, H, W, generator=g, dtype=F64)
        rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1, C)
        for training in (True, False):
            rm_t, rv_t = rm.clone(), rv.clone()
            y = F.batch_norm(x, rm_t, rv_t, gamma, beta, training, br.MOMENTUM, br.EPS)
            if res:
                y = y + r
            if relu:
                y = F.relu(y)
            dx, dr, dg, db = torch.autograd.grad(y, (x, r, gamma, beta), ct, allow_unused=True)
            R = N * H * W
            mean, var = br.stats(rows(x)) if training else (rm, rv)
            rstd = 1.0 / torch.sqrt(var + br.EPS)
            y_ref = br.fwd(rows(x), mean, rstd, gamma.detach(), beta.detach(), rows(r) if res else None, relu)
            _close(y_ref, rows(y))
            dx_ref, g_ref, dg_ref, db_ref = br.bwd(rows(ct), rows(x), y_ref, mean, rstd, gamma.detach(), relu, frozen=not training)
            _close(dx_ref, rows(dx)), _close(dg_ref, dg), _close(db_ref, db)
            if res:
                _close(g_ref, rows(dr))
            if training:
                rm_ref, rv_ref = br.running_update(rm, rv, mean, var, R, br.MOMENTUM)
                _close(rm_ref, rm_t), _close(rv_ref, rv_t)
                wm, wq, _ = br.stats_walk(rows(x))
                _close(wm, mean), _close(wq / R, var)


def test_pool_reference_is_aten_with_its_tie_rule():
    g = torch.Generator().manual_seed(4)
    for (H, W) in br.POOL_HW + ((7, 4),):
        for kind in ("randn", "relu", "zero"):
            x = torch.randn(2, 8, H, W, generator=g, dtype=F64)
            x = {"randn": x, "relu": x.clamp_min(0), "zero": torch.zeros_like(x)}[kind].requires_grad_()
            y = F.max_pool2d(x, 3, 2, 1)
            ct = torch.randn(y.shape, generator=g, dtype=F64)
            dx, = torch.autograd.grad(y, x, ct)
            nhwc = lambda t: t.detach().permute(0, 2, 3, 1)
            y_ref, idx = br.maxpool(nhwc(x))
            assert torch.equal(y_ref, nhwc(y))
            dx_ref, _ = br.maxpool_bwd(nhwc(ct), idx, H, W)
            _close(dx_ref, nhwc(dx))
            if kind == "randn":
                assert br.window_ties(nhwc(x)) == 0
    # the issue's example: an all-zero 4x4 map sends its gradient to (0,0), (0,1), (1,0), (1,1)
    _, idx = br.maxpool(torch.zeros(1, 4, 4, 8, dtype=F64))
    dx, _ = br.maxpool_bwd(torch.ones(1, 2, 2, 8, dtype=F64), idx, 4, 4)
    assert dx[0, :, :, 0].nonzero().tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]


def _stage_cases():
    for dtype in (F32, BF16):
        for C in br.CHANNELS:
            for R in br.ROWS_SMALL + (br.first_rows_with_blocks_over(64, br.blocks),):
                yield dtype, R, C, "randn"
        yield dtype, 4096, 64, "offset"
        yield dtype, 64, 256, "offset"


def test_fp32_twins_keep_the_bounds_and_mutants_do_not():
    worst = dict(mean=0.0, rstd=0.0, run=0.0, y=0.0, dx=0.0, dg=0.0, db=0.0)
    out = dict(naive=0.0, biased=0.0, mask=0.0)
    for dtype, R, C, kind in _stage_cases():
        t = br.inputs(R, C, dtype, seed=1, kind=kind)
        sb = br.stats_bounds(t["x"], br.EPS)
        mean, rstd, m2 = br.twin_stats(t["x"], br.EPS)
        worst["mean"] = max(worst["mean"], _ratio(mean - sb["ref_mean"], sb["mean"]))
        worst["rstd"] = max(worst["rstd"], _ratio(rstd - sb["ref_rstd"], sb["rstd"]))
        rm_ref, rv_ref, bm, bv = br.running_bounds(t["running_mean"], t["running_var"], sb, R, br.MOMENTUM)
        rm, rv = br.twin_running(t["running_mean"], t["running_var"], mean, m2, R, br.MOMENTUM)
        worst["run"] = max(worst["run"], _ratio(rm - rm_ref, bm), _ratio(rv - rv_ref, bv))
        _, nrstd, _ = br.twin_stats(t["x"], br.EPS, naive=True)
        out["naive"] = max(out["naive"], _ratio(nrstd - sb["ref_rstd"], sb["rstd"]))
        _, rvb = br.twin_running(t["running_mean"], t["running_var"], mean, m2, R, br.MOMENTUM, biased=True)
        out["biased"] = max(out["biased"], _ratio(rvb - rv_ref, bv))
        for relu, res, frozen in br.FLAGS:
            r = t["res"] if res else None
            y = br.twin_fwd(t["x"], mean, rstd, t["gamma"], t["beta"], r, relu, dtype)
            worst["y"] = max(worst["y"], _ratio(y.to(F64) - br.fwd(t["x"], mean, rstd, t["gamma"], t["beta"], r, relu),
                                                br.fwd_bound(t["x"], mean, rstd, t["gamma"], t["beta"], r, relu, dtype == BF16)))
            dx, g, dg, db = br.twin_bwd(t["dy"], t["x"], y, mean, rstd, t["gamma"], relu, frozen, dtype)
            dx_ref, g_ref, dg_ref, db_ref = br.bwd(t["dy"], t["x"], y, mean, rstd, t["gamma"], relu, frozen)
            bx, bg, bb = br.bwd_bounds(t["dy"], t["x"], y, mean, rstd, t["gamma"], relu, frozen, dtype == BF16)
            worst["dx"] = max(worst["dx"], _ratio(dx.to(F64) - dx_ref, bx))
            worst["dg"] = max(worst["dg"], _ratio(dg - dg_ref, bg))
            worst["db"] = max(worst["db"], _ratio(db - db_ref, bb))
            assert torch.equal(g.to(F64), g_ref)
            if relu and res:
                _, gm, _, _ = br.twin_bwd(t["dy"], t["x"], y, mean, rstd, t["gamma"], relu, frozen, dtype, mask_from_x=True)
                out["mask"] = max(out["mask"], float((gm.to(F64) - g_ref).abs().max()))
    print("twins: error / bound", "  ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    print("mutants: error / bound (mask: largest difference)", "  ".join("%s %.3g" % kv for kv in sorted(out.items())))
    assert all(v <= 1.0 for v in worst.values()), worst
    assert out["naive"] > 1.0 and out["biased"] > 1.0 and out["mask"] > 0.0, out


def test_pool_mutants_are_seen():
    g = torch.Generator().manual_seed(9)
    zero = torch.zeros(1, 4, 4, 8, dtype=F64)
    assert not torch.equal(br.maxpool(zero)[1], br.maxpool(zero, last=True)[1])
    post_relu = torch.randn(3, 8, 8, 8, generator=g, dtype=F64).clamp_min(0)
    assert br.window_ties(post_relu) > 0
    assert not torch.equal(br.maxpool(post_relu)[1], br.maxpool(post_relu, last=True)[1])
    neg = -torch.rand(1, 3, 5, 8, generator=g, dtype=F64) - 1.0
    assert not torch.equal(br.maxpool(neg)[0], br.maxpool(neg, admit_pad=True)[0])


# ---- the model ------------------------------------------------------------------------------------------------------------
def _cfg(extra=()):
    from focus_amd.slowfast.config.defaults import get_cfg
    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.MODEL_NAME", "STEVE", "MODEL.CNN_NAME", "res18", "NUM_GPUS", 0, "SLOTS.IMG_SIZE", 64,
                         "SLOTS.DECODER.DIM", 192, "SLOTS.DIM", 192, "SLOTS.SIZE", 192, "SLOTS.VOCAB_SIZE", 64,
                         "SLOTS.DECODER.NUM_BLOCKS", 1, "SLOTS.DECODER.NUM_HEADS", 4, "SLOTS.NUM_PREDICTOR_HEADS", 4] + list(extra))
    return cfg


def test_steve_constructs_with_res18_and_matches_the_reference_tree(monkeypatch):
    from focus_amd.slowfast.models import MODEL_REGISTRY
    monkeypatch.setenv("FOCUS_STEVE_BN", "0")
    torch.manual_seed(0)
    model = MODEL_REGISTRY.get("STEVE")(_cfg())
    cnn = model.steve_encoder.cnn
    sd = cnn.state_dict()
    assert len(sd) == br.N_STATE
    assert sum(k.startswith("fenc.") for k in sd) == br.N_FENC
    assert all(k.startswith(("fenc.", "res18.")) or k in ("upconv.weight", "upconv.bias") for k in sd)
    alias = {"fenc.0.": "res18.conv1.", "fenc.1.": "res18.bn1.", "fenc.4.0.": "res18.layer1.0.", "fenc.4.1.": "res18.layer1.1."}
    for k, v in sd.items():
        if k.startswith("fenc."):
            pre = next(p for p in sorted(alias, key=len, reverse=True) if k.startswith(p))
            assert sd[alias[pre] + k[len(pre):]].data_ptr() == v.data_ptr(), k
    assert sum(p.numel() for p in cnn.res18.parameters()) == br.NUMEL_RES18
    assert sum(p.numel() for p in cnn.parameters()) == br.NUMEL_BLOCK_192
    params = list(cnn.parameters())
    assert len(params) == br.N_PARAMS
    assert cnn.res18.conv1.bias is not None and tuple(cnn.res18.conv1.weight.shape) == (64, 3, 3, 3)
    # initialisation as the stock net: BatchNorm 1 / 0, residual convolutions kaiming_normal_(fan_out): std = sqrt(2 / (9 * 64))
    assert float(cnn.res18.layer1[0].bn1.weight.min()) == 1.0 and float(cnn.res18.layer1[0].bn1.bias.abs().max()) == 0.0
    assert abs(float(cnn.res18.layer1[0].conv1.weight.std()) / (2.0 / 576) ** 0.5 - 1) < 0.05

    # the restatement takes the state_dict strictly, and gives it back
    ref = br.Res18Restated(3, 192)
    assert sorted(ref.state_dict()) == sorted(sd)
    ref.load_state_dict(sd, strict=True)
    cnn.load_state_dict(ref.state_dict(), strict=True)

    # a backward through the ATen path on the CPU: 18 parameters receive a gradient, 47 never do; same values as the restatement
    x = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(1))
    cnn.train(), ref.train()
    y, y_ref = cnn(x), ref(x)
    assert tuple(y.shape) == (2, 192, 16, 16)
    # (the model's convolutions run channels-last, the restatement's do not: fp32 summation orders differ)
    assert float((y - y_ref).norm() / y_ref.norm()) < 1e-5
    y.square().sum().backward()
    assert sum(p.grad is not None for p in params) == br.N_LIVE and sum(p.grad is None for p in params) == br.N_DEAD
    assert int(cnn.res18.bn1.num_batches_tracked) == 1 and int(cnn.res18.layer2[0].bn1.num_batches_tracked) == 0
    named = dict(cnn.named_parameters())
    assert all(n.startswith(("res18.layer2", "res18.layer3", "res18.layer4", "res18.fc")) for n, p in named.items() if p.grad is None)


def test_res18_refuses_what_the_reference_cannot_run(monkeypatch):
    from focus_amd.slowfast.models import MODEL_REGISTRY
    with pytest.raises(ValueError, match="steve.py"):
        MODEL_REGISTRY.get("STEVE")(_cfg(["SLOTS.CNN_HID_SIZE", 32]))
    with pytest.raises(ValueError, match="steve.py"):
        MODEL_REGISTRY.get("STEVE")(_cfg(["SLOTS.IMG_SIZE", 128]))
    # the HIP path has no CPU fallback: only FOCUS_STEVE_BN=0 runs on the CPU
    monkeypatch.setenv("FOCUS_STEVE_BN", "1")
    cnn = MODEL_REGISTRY.get("STEVE")(_cfg()).steve_encoder.cnn
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cnn(torch.rand(2, 3, 16, 16))


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------
def test_entry_points_validate_before_launching(built):
    from focus_amd import _lib, ops
    lib = _lib.lib()
    f32, bf16, fp8 = _lib.F32, _lib.BF16, _lib.FP8_E4M3
    for R in (0, 1, 31, 32, 33, 2048, 2049, 32768, 32769, 1 << 20, 1 << 31):
        assert lib.focus_bn_blocks(R) == br.blocks(R)
        for C in br.CHANNELS:
            assert lib.focus_bn_workspace_bytes(R, C) == br.workspace_bytes(R, C)
    assert lib.focus_bn_workspace_bytes(64, 12) == 0 and lib.focus_bn_workspace_bytes(64, 264) == 0
    assert br.first_rows_with_blocks_over(64, lib.focus_bn_blocks) == 2049
    buf = ctypes.create_string_buffer(1 << 16)
    a = ctypes.addressof(buf)
    a += -a % 16
    ptr, odd = ctypes.c_void_p(a), ctypes.c_void_p(a + 4)
    OK, NULL, SHAPE, DTYPE, ALIGN = 0, -5, -1, -2, -3
    st = lambda x=ptr, mean=ptr, rstd=ptr, rm=ptr, rv=ptr, ws=ptr, R=4, C=64, dt=f32: \
        lib.focus_bn_stats(x, mean, rstd, rm, rv, ws, R, C, 1e-5, 0.1, dt, None)
    assert st(x=None) == NULL and st(mean=None) == NULL and st(ws=None) == NULL
    assert st(rm=None) == NULL and st(rv=None) == NULL                       # both running buffers, or neither
    assert st(C=60) == SHAPE and st(C=0) == SHAPE and st(C=264) == SHAPE
    assert st(R=1) == SHAPE and st(R=0) == SHAPE                              # training statistics of fewer than 2 rows
    assert st(dt=fp8) == DTYPE and st(x=odd) == ALIGN and st(rv=odd) == ALIGN
    ap = lambda x=ptr, mean=ptr, rstd=ptr, g=ptr, b=ptr, res=None, y=ptr, R=4, C=64, dt=f32: \
        lib.focus_bn_apply(x, mean, rstd, g, b, res, y, R, C, 1, dt, None)
    assert ap(x=None) == NULL and ap(y=None) == NULL and ap(g=None) == NULL and ap(rstd=None) == NULL
    assert ap(C=12) == SHAPE and ap(R=-1) == SHAPE and ap(dt=fp8) == DTYPE
    assert ap(res=odd) == ALIGN and ap(y=odd) == ALIGN
    assert ap(R=0) == OK and ap(R=0, x=None, y=None) == OK                    # no rows: nothing to launch
    bw = lambda dy=ptr, x=ptr, y=ptr, mean=ptr, g=ptr, dx=ptr, dres=None, dg=ptr, db=ptr, ws=ptr, R=4, C=64, relu=1, dt=bf16: \
        lib.focus_bn_bwd(dy, x, y, mean, ptr, g, dx, dres, dg, db, ws, R, C, relu, 0, dt, None)
    assert bw(dy=None) == NULL and bw(dx=None) == NULL and bw(dg=None) == NULL and bw(ws=None) == NULL
    assert bw(y=None) == NULL                                                 # the ReLU mask is read from y
    assert bw(C=4) == SHAPE and bw(R=-2) == SHAPE and bw(dt=7) == DTYPE
    assert bw(dres=odd) == ALIGN and bw(db=odd) == ALIGN
    pf = lambda x=ptr, y=ptr, idx=ptr, N=1, H=4, W=4, C=8, dt=f32: lib.focus_maxpool_fwd(x, y, idx, N, H, W, C, dt, None)
    pb = lambda dy=ptr, idx=ptr, dx=ptr, N=1, H=4, W=4, C=8, dt=f32: lib.focus_maxpool_bwd(dy, idx, dx, N, H, W, C, dt, None)
    for f in (pf, pb):
        assert f(idx=None) == NULL and f(H=0) == SHAPE and f(W=0) == SHAPE and f(C=20) == SHAPE and f(N=-1) == SHAPE
        assert f(N=1 << 20, H=64, W=64) == SHAPE and f(dt=fp8) == DTYPE and f(idx=odd) == ALIGN
        assert f(N=0) == OK
    x = torch.randn(2, 8, 4, 4)
    w = torch.ones(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.batch_norm(x, w, w, w.clone(), w.clone(), True, 0.1, 1e-5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.max_pool_3x3_s2(x)
