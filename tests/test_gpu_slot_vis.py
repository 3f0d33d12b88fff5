"""focus_slot_vis_grid (csrc/slot_vis.hip) and what is built on it, on the GPU: the kernel through the C ABI and through
ops.slot_vis_grid against the numpy twin of tests/slot_vis_ref.py -- EXACT equality, both slot forms, fp32 and bf16 sources
mixed per argument, fp32 and bf16 attention, both output types, into a buffer with sentinel guard rows on both sides; every
status code of the contract with the output untouched after a refusal; STEVE.forward(..., attns="raw"), visualize_slots
against visualize on the default forward's overlays, reconstruct_autoregressive against decode(encode(...)), and the two loops
(slot_train_epoch's add_video, slot_val_epoch's val_loss)."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import slot_vis_ref as ref

pytestmark = pytest.mark.gpu

NULL, SHAPE, DTYPE, ALIGN = -5, -1, -2, -3
# (B, T, K, (He, We), H, W): the smallest shapes that exercise every index.  SMALL: sy = 2 != sx = 4, H != W, Wg = 134 is no
# multiple of 4 (canvas rows start at every alignment), N = 8 > B clamps the rows to 3.  WIDE: K = 11, B = 9 > N = 8.
SMALL = (3, 2, 3, (3, 5), 6, 20)
WIDE = (9, 2, 11, (4, 4), 16, 16)
DEV = "cuda:0"


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def cases():
    """Per shape, computed once and left alone: the fp32 inputs, their bf16 roundings (as float32), the overlays."""
    out = {}
    for name, shape in (("small", SMALL), ("wide", WIDE)):
        B, T, K, grid, H, W = shape
        f = ref.inputs(B, T, K, grid, H, W, seed=11)
        out[name] = dict(shape=shape, f32=f, bf16=tuple(ref.bf16_round(x) for x in f))
    return out


def pick(case, kinds):
    """kinds: four letters, 'f' or 'b', for video, recon, gen, attn -> (numpy float32 values, device tensors in that dtype)."""
    vals = tuple(case["bf16"][i] if k == "b" else case["f32"][i] for i, k in enumerate(kinds))
    dev = tuple(torch.from_numpy(v).to(DEV).to(torch.bfloat16 if k == "b" else torch.float32) for v, k in zip(vals, kinds))
    return vals, dev


def expected(case, vals, N, u8):
    B, T, K, grid, H, W = case["shape"]
    want = ref.visualize_slots(vals[0], vals[1], vals[2], vals[3], grid, N)
    return ref.to_uint8(want) if u8 else want


def dt(t):
    from focus_amd import _lib
    return _lib.BF16 if t.dtype == torch.bfloat16 else _lib.F32


@pytest.mark.parametrize("u8", [False, True], ids=["f32out", "u8out"])
@pytest.mark.parametrize("kinds", ["ffff", "bfbf", "fbfb", "bbbb"])
@pytest.mark.parametrize("name,N", [("small", 2), ("small", 3), ("wide", 8)])
def test_c_abi_raw_form_equals_the_twin_and_writes_the_canvas_alone(cases, name, N, kinds, u8):
    from focus_amd import _lib
    case = cases[name]
    B, T, K, (He, We), H, W = case["shape"]
    vals, (video, recon, gen, attn) = pick(case, kinds)
    want = expected(case, vals, N, u8)
    _, _, _, Hg, Wg = want.shape
    n = T * 3 * Hg * Wg
    # guard rows on both sides; 2 Wg + 1 elements in front puts the canvas at an odd element offset from an aligned address
    front, back = 2 * Wg + 1, 2 * Wg
    sentinel = 0xA5 if u8 else -777.25
    buf = torch.full((front + n + back,), sentinel, device=DEV, dtype=torch.uint8 if u8 else torch.float32)
    out = buf[front:front + n]
    st = _lib.lib().focus_slot_vis_grid(p(video), dt(video), p(recon), dt(recon), p(gen), dt(gen), p(attn), dt(attn), 1, B,
                                        gen.shape[0], T, 3, H, W, K, He, We, N, p(out), int(u8), None)
    torch.cuda.synchronize()
    assert st == 0
    got = buf.cpu().numpy()
    assert (got[:front] == np.array(sentinel, got.dtype)).all() and (got[front + n:] == np.array(sentinel, got.dtype)).all()
    canvas = got[front:front + n].reshape(want.shape)
    if u8:                                     # a byte equal to the sentinel could hide an unwritten one: a second fill tells
        buf.fill_(0x3C)
        _lib.lib().focus_slot_vis_grid(p(video), dt(video), p(recon), dt(recon), p(gen), dt(gen), p(attn), dt(attn), 1, B,
                                       gen.shape[0], T, 3, H, W, K, He, We, N, p(out), 1, None)
        assert np.array_equal(buf.cpu().numpy()[front:front + n].reshape(want.shape), canvas)
    else:
        assert not (canvas == np.float32(sentinel)).any()
    assert np.array_equal(bits(canvas), bits(want))


@pytest.mark.parametrize("u8", [False, True], ids=["f32out", "u8out"])
@pytest.mark.parametrize("kinds", ["fff", "bfb", "fbf"])
@pytest.mark.parametrize("name,N", [("small", 2), ("small", 3), ("wide", 8)])
def test_c_abi_vis_form_copies_the_overlays(cases, name, N, kinds, u8):
    from focus_amd import _lib
    case = cases[name]
    B, T, K, grid, H, W = case["shape"]
    vals, (video, recon, gen, _) = pick(case, kinds + "f")
    # overlays as forward makes them -- of the fp32 video whatever the tile sources are, so a kernel that rebuilt them from
    # its video argument would not pass
    vis = ref.overlay(case["f32"][0], ref.upsample(case["f32"][3], grid, H, W))
    want = ref.visualize(vals[0], vals[1], vals[2], vis, K, N)
    want = ref.to_uint8(want) if u8 else want
    out = torch.full(want.shape, 0xA5 if u8 else -777.25, device=DEV, dtype=torch.uint8 if u8 else torch.float32)
    st = _lib.lib().focus_slot_vis_grid(p(video), dt(video), p(recon), dt(recon), p(gen), dt(gen), p(torch.from_numpy(vis).to(DEV)),
                                        _lib.F32, 0, B, B, T, 3, H, W, K, 0, 0, N, p(out), int(u8), None)
    torch.cuda.synchronize()
    assert st == 0
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))


@pytest.mark.parametrize("name,N,rows", [("small", 2, 2), ("small", 8, 3), ("wide", 8, 8)])
def test_ops_and_mirror_equal_the_twin(cases, name, N, rows):
    from focus_amd import ops
    from focus_amd.slowfast.utils import slot_misc
    case = cases[name]
    B, T, K, grid, H, W = case["shape"]
    for kinds in ("ffff", "bfbb"):
        vals, (video, recon, gen, attn) = pick(case, kinds)
        want = ref.visualize_slots(*vals, grid, N)
        assert want.shape == ref.grid_shape(T, H, W, K, rows)
        got = ops.slot_vis_grid(video, recon, gen[:rows].contiguous(), attn=attn, grid=grid, rows=N)      # gen of exactly the rows
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))
        got8 = slot_misc.visualize_slots(video, recon, gen, attn, grid, N=N, out_dtype=torch.uint8)
        assert got8.dtype == torch.uint8 and np.array_equal(got8.cpu().numpy(), ref.to_uint8(want))
        vis = torch.from_numpy(ref.overlay(vals[0], ref.upsample(vals[3], grid, H, W))).to(DEV)
        for got in (ops.slot_vis_grid(video, recon, gen, attns_vis=vis, rows=N), slot_misc.visualize(video, recon, gen, vis, K, N)):
            assert np.array_equal(bits(got.cpu().numpy()), bits(want))
        # the mirror's loop on the device is the composition the kernel replaces: the same bits
        loop = slot_misc.visualize_loop(video, recon, gen, vis, K, N)
        assert loop.dtype == torch.float32 and np.array_equal(bits(loop.cpu().numpy()), bits(want))
    with pytest.raises(ValueError, match="num_slots"):
        slot_misc.visualize(video, recon, gen, vis, K + 1, N)
    with pytest.raises(ValueError, match="is on"):
        ops.slot_vis_grid(video, recon.cpu(), gen, attn=attn, grid=grid)


def test_uint8_output_clips_and_takes_nan_to_zero():
    """Values outside [0,1] and a NaN in every kind of tile: the fp32 output carries them, the uint8 output follows the rule."""
    from focus_amd import ops
    B, T, K, grid, H, W = SMALL
    video, recon, gen, attn = (x.copy() for x in ref.inputs(B, T, K, grid, H, W, seed=5))
    video[0, 0, 0, 0, :4] = (np.nan, -0.5, 1.75, np.inf)
    recon[1, 1, 2, 5, 16:] = (-np.inf, 2.0, -1e-3, np.nan)
    gen[2, 0, 1, 3, 7] = np.nan
    attn[0, 1, 7, 1] = np.nan
    d = [torch.from_numpy(x).to(DEV) for x in (video, recon, gen, attn)]
    want = ref.visualize_slots(video, recon, gen, attn, grid, 8)
    got = ops.slot_vis_grid(*d[:3], attn=d[3], grid=grid).cpu().numpy()
    nan = np.isnan(want)
    assert nan.sum() >= 4 + 2 * 4 * 3 and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan])
    got8 = ops.slot_vis_grid(*d[:3], attn=d[3], grid=grid, out_dtype=torch.uint8).cpu().numpy()
    assert np.array_equal(got8, ref.to_uint8(want)) and (got8[nan] == 0).all()


def test_every_status_code_and_a_refusal_writes_nothing(cases):
    from focus_amd import _lib
    lib = _lib.lib()
    F32, BF16, FP8 = _lib.F32, _lib.BF16, _lib.FP8_E4M3
    case = cases["small"]
    B, T, K, (He, We), H, W = case["shape"]
    _, (video, recon, gen, attn) = pick(case, "ffff")
    shape = ref.grid_shape(T, H, W, K, 3)
    out = torch.full(shape, -3.5, device=DEV)
    vis = torch.zeros(B, T, K, 3, H, W, device=DEV)

    def call(video=video, dv=F32, recon=recon, dr=F32, gen=gen, dg=F32, slots=attn, ds=F32, form=1, B=B, Bg=B, T=T, C=3, H=H,
             W=W, K=K, He=He, We=We, rows=3, out=out, ot=0):
        ptr = lambda t: None if t is None else (t if isinstance(t, ctypes.c_void_p) else p(t))
        return lib.focus_slot_vis_grid(ptr(video), dv, ptr(recon), dr, ptr(gen), dg, ptr(slots), ds, form, B, Bg, T, C, H, W, K,
                                       He, We, rows, ptr(out), ot, None)
    odd = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
    for name in ("video", "recon", "gen", "slots", "out"):
        assert call(**{name: None}) == NULL, name
    assert call(video=None, C=4) == NULL and call(out=None, dv=FP8) == NULL                  # NULL first
    for kw in (dict(form=2), dict(C=1), dict(C=4), dict(K=0), dict(K=33), dict(B=0), dict(Bg=0), dict(H=0), dict(W=0),
               dict(T=-1), dict(rows=-1), dict(rows=4), dict(rows=3, Bg=2), dict(He=0), dict(We=0), dict(He=4), dict(We=3),
               dict(T=1 << 22), dict(form=0, slots=vis, K=40)):
        assert call(**kw) == SHAPE, kw
    for kw in (dict(dv=FP8), dict(dr=FP8), dict(dg=7), dict(ds=FP8), dict(form=0, slots=vis, ds=BF16), dict(ot=2)):
        assert call(**kw) == DTYPE, kw
    assert call(dv=FP8, C=4) == SHAPE and call(dv=FP8, video=odd(video, 2)) == DTYPE         # SHAPE, then DTYPE, then ALIGN
    for kw in (dict(video=odd(video, 2)), dict(recon=odd(recon, 1)), dict(gen=odd(gen, 2)), dict(slots=odd(attn, 2)),
               dict(out=odd(out, 2)), dict(video=odd(video, 1), dv=BF16)):
        assert call(**kw) == ALIGN, kw
    assert call(rows=0) == 0 and call(T=0) == 0                                              # nothing to do: no launch
    torch.cuda.synchronize()
    assert (out == -3.5).all()
    assert call() == 0 and call(form=0, slots=vis, He=0, We=0) == 0                           # and the accepted calls do write
    torch.cuda.synchronize()
    assert not (out == -3.5).any()


# ---- the model and the loops -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def steve():
    from test_gpu_steve import _steve_small
    torch.manual_seed(3)
    cfg, m = _steve_small(False)
    cfg.SOLVER.OPTIMIZING_METHOD = "adam"
    cfg.SOLVER.CLIP_GRAD_L2NORM = 1.0
    return cfg, m.to(DEV)


def steve_noise(m, B, T, grid):
    g = torch.Generator().manual_seed(9)
    n = B * T
    return {"gumbel_soft": torch.empty(n, m.vocab_size, grid[0], grid[1]).exponential_(generator=g).to(DEV),
            "gumbel_hard": torch.empty(n, m.vocab_size, grid[0], grid[1]).exponential_(generator=g).to(DEV),
            "slots": torch.randn(B, m.num_slots, m.steve_encoder.savi.slot_size, generator=g).to(DEV)}


@contextlib.contextmanager
def repeatable_convolutions():
    """MIOpen held to its deterministic kernels, as STEVE._repeatable does for the res18 trunk: two passes of the small model's
    convolution stacks may otherwise differ in the last bits, which has nothing to do with what these tests compare."""
    keep = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = keep


def test_forward_raw_returns_the_slot_updates_attention_and_the_same_losses(steve):
    from focus_amd.slowfast.utils import slot_misc
    cfg, m = steve
    m.eval()
    video = torch.rand(3, 2, 3, 16, 16, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad(), repeatable_convolutions():
        tgrid = m.dvae.encoder(video.flatten(end_dim=1)).shape[-2:]
        noise = steve_noise(m, 3, 2, tgrid)
        recon, ce, mse, vis = m(video, 1.0, cfg.SLOTS.HARD, noise=noise)
        recon_r, ce_r, mse_r, attn = m(video, 1.0, cfg.SLOTS.HARD, noise=noise, attns="raw")
        _, own, He, We = m._slot_attns(video, noise["slots"])
    K = m.num_slots
    assert vis.shape == (3, 2, K, 3, 16, 16) and attn.shape == (3, 2, He * We, K) and m.slot_grid == (He, We)
    assert not attn.requires_grad and torch.equal(attn, own)
    assert torch.equal(recon, recon_r) and torch.equal(ce, ce_r) and torch.equal(mse, mse_r)
    with pytest.raises(ValueError, match="'vis' or 'raw'"):
        m(video, 1.0, cfg.SLOTS.HARD, attns="both")
    # the pictures: visualize_slots on the raw attention == visualize on the overlays, bit for bit, and both == the twin
    gen = torch.rand(3, 2, 3, 16, 16, generator=torch.Generator().manual_seed(2)).to(DEV)
    with pytest.raises(ValueError, match="contiguous"):                     # forward's recon is a channels-last view
        slot_misc.visualize_slots(video, recon, gen, attn.contiguous(), (He, We), N=8)
    recon = recon.contiguous()
    a = slot_misc.visualize_slots(video, recon, gen, attn.contiguous(), (He, We), N=8)
    b = slot_misc.visualize(video, recon, gen, vis.contiguous(), K, N=8)
    assert a.shape == ref.grid_shape(2, 16, 16, K, 3) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    want = ref.visualize_slots(*(x.float().cpu().numpy() for x in (video, recon, gen, attn)), (He, We), 8)
    assert np.array_equal(bits(a.cpu().numpy()), bits(want))


def test_reconstruct_autoregressive_is_decode_of_encode_under_one_seed(steve):
    cfg, m = steve
    m.eval()
    video = torch.rand(2, 2, 3, 16, 16, generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad(), repeatable_convolutions():
        torch.manual_seed(21)
        got = m.reconstruct_autoregressive(video)
        state = torch.cuda.get_rng_state(DEV)
        torch.manual_seed(21)
        slots, _, _ = m.encode(video)
        want = m.decode(slots.flatten(end_dim=1)).reshape(video.shape)
        assert torch.equal(torch.cuda.get_rng_state(DEV), state)           # the same draws were made
    assert got.shape == video.shape and torch.equal(got, want)


class Recorder:
    def __init__(self):
        self.scalars, self.videos = [], []

    def add_scalars(self, d, global_step=None):
        self.scalars.append((dict(d), global_step))

    def add_video(self, frames, tag=None, global_step=None):
        self.videos.append((frames, tag, global_step))


class ScalarsOnly:
    def __init__(self):
        self.scalars = []

    def add_scalars(self, d, global_step=None):
        self.scalars.append((dict(d), global_step))


def test_slot_train_epoch_hands_one_video_to_the_writer_and_restores_the_mode(steve):
    from focus_amd.slowfast.models.optimizer import construct_optimizer_slot
    from focus_amd.train import slot_train_epoch
    cfg, m = steve
    opt = construct_optimizer_slot(m, cfg)
    g = torch.Generator().manual_seed(6)
    loader = [torch.rand(2, 2, 3, 16, 16, generator=g) for _ in range(2)]
    w = Recorder()
    m.eval()
    opd = slot_train_epoch(loader, m, opt, None, None, 4, cfg, writer=w)
    assert m.training                                                       # train mode set by the loop, restored after the generation
    assert opd["global_step"] == 4 * 2 + 1 and len(w.scalars) == 2 and len(w.videos) == 1
    frames, tag, step = w.videos[0]
    K = m.num_slots
    assert tag == "TRAIN_recons/epoch=5" and step == 5
    assert frames.dtype == torch.uint8 and frames.is_cuda and tuple(frames.shape) == ref.grid_shape(2, 16, 16, K, 2)
    f = frames.cpu().numpy()
    assert (f[0, :, :, :2] == 204).all() and (f[0, :, :, :, :2] == 204).all()
    assert np.array_equal(f[0, :, :, 2:18, 2:18], ref.to_uint8(loader[1][0].numpy()))         # tile (0, 0) is the last batch's video
    s = ScalarsOnly()
    opd = slot_train_epoch(loader, m, opt, None, None, 5, cfg, writer=s)    # a writer without add_video: scalars alone
    assert len(s.scalars) == 2 and m.training
    assert slot_train_epoch(loader, m, opt, None, None, 6, cfg)["global_step"] == 13          # and no writer at all


def test_slot_val_epoch_means_are_the_double_sums_of_the_batches(steve):
    """val_loss against the reference's MetricTracker arithmetic on the very losses the loop's forwards returned (a forward hook
    records them): python-float sums of mse.item() and cross_entropy.item() over the batches, each divided by the count.  The
    device table holds the same double sums of the same fp32 values added in the same order (tests/step_stats_ref.py: one
    thread, step order), so the bound is zero."""
    from focus_amd.train import slot_val_epoch
    cfg, m = steve
    g = torch.Generator().manual_seed(8)
    loader = [torch.rand(b, 2, 3, 16, 16, generator=g) for b in (2, 3, 1)]
    seen = []
    hook = m.register_forward_hook(lambda _m, _i, out: seen.append((out[2].mean().item(), out[1].mean().item(), out[3])))
    m.train()
    w = ScalarsOnly()
    try:
        val_loss, out = slot_val_epoch(loader, m, 2, cfg, {"tau": 0.7}, writer=w)
    finally:
        hook.remove()
    assert not m.training and len(seen) == 3
    mse_sum = ce_sum = 0.0
    for mse, ce, _ in seen:
        mse_sum += mse
        ce_sum += ce
    assert val_loss == mse_sum / 3 + ce_sum / 3
    assert w.scalars == [({"VAL/loss": val_loss, "VAL/cross_entropy": ce_sum / 3, "VAL/mse": mse_sum / 3}, 3)]
    K = m.num_slots
    He, We = m.slot_grid
    assert set(out) == {"video", "recon", "attns"} and out["video"].shape == (1, 2, 3, 16, 16) and out["video"].is_cuda
    assert out["recon"].shape == out["video"].shape and out["attns"].shape == (1, 2, He * We, K)
    assert out["attns"] is seen[-1][2]
