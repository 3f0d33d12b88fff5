"""CPU-side checks of the STEVE epoch visualisation: the numpy twin of tests/slot_vis_ref.py against the mirror module
focus_amd/slowfast/utils/slot_misc.py on CPU tensors (bit for bit), the twin's raw form against its vis form fed the torch
chain of steve.py:314-319, the grid size and the pad value, five mutants that must each change the twin's result on the test
inputs, and every refusal of ops.slot_vis_grid, visualize_slots and focus_slot_vis_grid that needs no device."""
import ctypes

import numpy as np
import pytest
import torch

import slot_vis_ref as ref

NULL, SHAPE, DTYPE, ALIGN = -5, -1, -2, -3
# (B, T, K, (He, We), H, W): sy = 2 != sx = 4, H != W, Wg = 134 is no multiple of 4; and the README's slot count at 4x4 -> 16x16
SMALL = (3, 2, 3, (3, 5), 6, 20)
WIDE = (9, 2, 11, (4, 4), 16, 16)


@pytest.fixture(scope="module")
def built():
    from focus_amd.build import build
    return build(verbose=False)


def torch_overlays(video, attn, grid):
    """steve.py:314-319 in torch on the CPU: the chain STEVE._slots and STEVE.forward run."""
    B, T, _, H, W = video.shape
    He, We = grid
    K = attn.shape[3]
    a = torch.from_numpy(attn).float().transpose(-1, -2).reshape(B, T, K, 1, He, We) \
        .repeat_interleave(H // He, dim=-2).repeat_interleave(W // We, dim=-1)
    v = torch.from_numpy(video)
    return (v.unsqueeze(2) * a + (1.0 - a)).numpy()


@pytest.mark.parametrize("shape", [SMALL, WIDE])
@pytest.mark.parametrize("N", [2, 8])
def test_twin_equals_the_mirror_on_cpu_tensors_bit_for_bit(shape, N):
    from focus_amd.slowfast.utils import slot_misc
    B, T, K, grid, H, W = shape
    video, recon, gen, attn = ref.inputs(B, T, K, grid, H, W, seed=1)
    vis = torch_overlays(video, attn, grid)
    want = ref.visualize(video, recon, gen, vis, K, N)
    got = slot_misc.visualize(*(torch.from_numpy(x) for x in (video, recon, gen, vis)), num_slots=K, N=N)
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.grid_shape(T, H, W, K, min(N, B)) == want.shape
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    # the mirror's make_grid alone, at a row length that leaves the last grid row short
    tiles = np.ascontiguousarray(video[:, 0])
    g = slot_misc.make_grid(torch.from_numpy(tiles), nrow=2, padding=3, pad_value=0.25)
    assert np.array_equal(g.numpy(), ref.make_grid(tiles, 2, 3, 0.25))


@pytest.mark.parametrize("shape", [SMALL, WIDE])
def test_twin_raw_form_equals_its_vis_form_fed_the_torch_chain(shape):
    B, T, K, grid, H, W = shape
    video, recon, gen, attn = ref.inputs(B, T, K, grid, H, W, seed=2)
    vis = torch_overlays(video, attn, grid)
    assert np.array_equal(ref.overlay(video, ref.upsample(attn, grid, H, W)).view(np.uint32), vis.view(np.uint32))
    a = ref.visualize_slots(video, recon, gen, attn, grid, 8)
    b = ref.visualize(video, recon, gen, vis, K, 8)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # bf16 sources widen exactly: torch's promotion in the chain and in cat is the twin's float32 view of the same values
    vb, ab = ref.bf16_round(video), ref.bf16_round(attn)
    tv, ta = torch.from_numpy(vb).bfloat16(), torch.from_numpy(ab).bfloat16()
    assert torch.equal(tv.float(), torch.from_numpy(vb)) and torch.equal(ta.float(), torch.from_numpy(ab))
    He, We = grid
    chain = tv.unsqueeze(2) * ta.float().transpose(-1, -2).reshape(B, T, K, 1, He, We).repeat_interleave(H // He, dim=-2) \
        .repeat_interleave(W // We, dim=-1)
    assert chain.dtype == torch.float32
    assert np.array_equal(ref.overlay(vb, ref.upsample(ab, grid, H, W)),
                          torch_overlays(vb, ab, grid))


def test_grid_size_and_pad_value():
    from focus_amd import ops
    B, T, K, grid, H, W = SMALL
    video, recon, gen, attn = ref.inputs(B, T, K, grid, H, W, seed=3)
    for N, rows in ((2, 2), (8, 3), (3, 3)):
        out = ref.visualize_slots(video, recon, gen, attn, grid, N)
        assert out.shape == (1, T, 3, rows * (H + 2) + 2, (K + 3) * (W + 2) + 2) == ops.slot_vis_grid_shape(T, H, W, K, rows)
    assert out.shape[-1] % 4 != 0
    pad = np.ones(out.shape[-2:], dtype=bool)
    for r in range(3):
        for j in range(K + 3):
            pad[r * (H + 2) + 2:r * (H + 2) + 2 + H, j * (W + 2) + 2:j * (W + 2) + 2 + W] = False
    assert pad.sum() == pad.size - 3 * (K + 3) * H * W
    assert (out[0][:, :, pad].view(np.uint32) == np.float32(0.8).view(np.uint32)).all()
    assert np.float32(0.8).view(np.uint32) == 0x3F4CCCCD
    assert (ref.to_uint8(out)[0][:, :, pad] == 204).all()
    # tile (r, j): the sources in the order video, recon, gen, slots
    assert np.array_equal(out[0, 1, :, 2:2 + H, 2:2 + W], video[0, 1])
    assert np.array_equal(out[0, 1, :, (H + 2) + 2:(H + 2) + 2 + H, (W + 2) + 2:(W + 2) + 2 + W], recon[1, 1])
    assert np.array_equal(out[0, 0, :, 2 * (H + 2) + 2:2 * (H + 2) + 2 + H, 2 * (W + 2) + 2:2 * (W + 2) + 2 + W], gen[2, 0])


def test_uint8_rule_truncates_clips_and_zeroes_nan():
    x = np.array([0.0, 0.8, 1.0, 1.5, -0.25, 0.999, 0.5, 1.0 / 255, 0.00392, np.nan, np.inf, -np.inf], dtype=np.float32)
    assert ref.to_uint8(x).tolist() == [0, 204, 255, 255, 0, 254, 127, 1, 0, 0, 255, 0]
    t = torch.from_numpy(x[:9])
    assert (t * 255).clip(0, 255).numpy().astype(np.uint8).tolist() == ref.to_uint8(x[:9]).tolist()


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_differs_from_the_twin_on_the_test_inputs(mutant):
    assert set(ref.MUTANTS) == {"fma", "swap_strides", "origin", "transposed", "round"}
    for B, T, K, grid, H, W in (SMALL, WIDE):
        video, recon, gen, attn = ref.inputs(B, T, K, grid, H, W, seed=1)
        good = ref.visualize_slots(video, recon, gen, attn, grid, 8)
        if mutant == "round":
            assert not np.array_equal(ref.to_uint8(good), ref.to_uint8(good, mutant))
            continue
        bad = ref.visualize_slots(video, recon, gen, attn, grid, 8, mutant)
        assert bad.shape == good.shape
        if mutant == "swap_strides" and H // grid[0] == W // grid[1]:
            assert np.array_equal(bad, good)                       # square cells cannot tell: SMALL is there for this one
            continue
        assert not np.array_equal(bad.view(np.uint32), good.view(np.uint32)), (mutant, H, W)
        if mutant == "fma":                                        # a fraction of the overlay pixels, and only those
            diff = bad != good
            assert 0.01 < diff.mean() < 0.3
            assert np.array_equal(ref.to_uint8(good)[..., :3 * (W + 2) + 2], ref.to_uint8(bad)[..., :3 * (W + 2) + 2])


# ---- refusals that need no device ------------------------------------------------------------------------------------
def cpu_args(shape=SMALL, Bg=None):
    B, T, K, grid, H, W = shape
    video, recon, gen, attn = (torch.from_numpy(x) for x in ref.inputs(B, T, K, grid, H, W, seed=4, Bg=Bg))
    return video, recon, gen, attn, torch.zeros(B, T, K, 3, H, W), grid


def test_ops_and_visualize_slots_refuse_on_the_host():
    from focus_amd import ops
    from focus_amd.slowfast.utils import slot_misc
    video, recon, gen, attn, vis, grid = cpu_args()
    ok = dict(attn=attn, grid=grid)
    with pytest.raises(ValueError, match="exactly one"):
        ops.slot_vis_grid(video, recon, gen)
    with pytest.raises(ValueError, match="exactly one"):
        ops.slot_vis_grid(video, recon, gen, attns_vis=vis, attn=attn, grid=grid)
    with pytest.raises(ValueError, match="grid"):
        ops.slot_vis_grid(video, recon, gen, attn=attn)
    with pytest.raises(ValueError, match="grid"):
        ops.slot_vis_grid(video, recon, gen, attns_vis=vis, grid=grid)
    with pytest.raises(ValueError, match="float32 or uint8"):
        ops.slot_vis_grid(video, recon, gen, out_dtype=torch.float16, **ok)
    with pytest.raises(ValueError, match=r"\[B,T,3,H,W\]"):
        ops.slot_vis_grid(video[:, :, :2], recon[:, :, :2], gen[:, :, :2], **ok)             # C != 3
    with pytest.raises(ValueError, match=r"\[B,T,3,H,W\]"):
        ops.slot_vis_grid(video[0], recon[0], gen[0], **ok)
    with pytest.raises(ValueError, match=r"\[B,T,3,H,W\]"):
        ops.slot_vis_grid(video[:, :0], recon[:, :0], gen[:, :0], **ok)                      # T == 0
    with pytest.raises(ValueError, match="do not match"):
        ops.slot_vis_grid(video, recon[:, :1], gen, **ok)
    with pytest.raises(ValueError, match="do not match"):
        ops.slot_vis_grid(video, recon, gen[..., :4], **ok)
    with pytest.raises(ValueError, match="rows"):
        ops.slot_vis_grid(video, recon, gen[:1], rows=2, **ok)                               # gen holds too few clips
    with pytest.raises(ValueError, match="rows"):
        ops.slot_vis_grid(video, recon, gen, rows=0, **ok)
    with pytest.raises(ValueError, match="does not divide"):
        ops.slot_vis_grid(video, recon, gen, attn=attn, grid=(5, 3))
    with pytest.raises(ValueError, match="does not divide"):
        ops.slot_vis_grid(video, recon, gen, attn=attn, grid=(0, 5))
    with pytest.raises(ValueError, match="grid is"):
        ops.slot_vis_grid(video, recon, gen, attn=attn, grid=3)
    with pytest.raises(ValueError, match=r"attn \[B,T,He\*We,K\]"):
        ops.slot_vis_grid(video, recon, gen, attn=attn, grid=(3, 10))                        # N != He We
    with pytest.raises(ValueError, match=r"attn \[B,T,He\*We,K\]"):
        ops.slot_vis_grid(video, recon, gen, attn=torch.zeros(3, 2, 15, 33), grid=grid)      # K > 32
    with pytest.raises(ValueError, match=r"attn \[B,T,He\*We,K\]"):
        ops.slot_vis_grid(video, recon, gen, attn=attn[:2], grid=grid)
    with pytest.raises(ValueError, match=r"attns_vis \[B,T,K,3,H,W\]"):
        ops.slot_vis_grid(video, recon, gen, attns_vis=vis[:, :, :, :1])
    with pytest.raises(ValueError, match=r"attns_vis \[B,T,K,3,H,W\]"):
        ops.slot_vis_grid(video, recon, gen, attns_vis=torch.zeros(3, 2, 33, 3, 6, 20))
    with pytest.raises(ValueError, match="attns_vis is float32"):
        ops.slot_vis_grid(video, recon, gen, attns_vis=vis.bfloat16())
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        ops.slot_vis_grid(video.double(), recon, gen, **ok)
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        ops.slot_vis_grid(video, recon, gen, attn=attn.half(), grid=grid)
    with pytest.raises(ValueError, match="contiguous"):
        ops.slot_vis_grid(video, recon.transpose(3, 4).contiguous().transpose(3, 4), gen, **ok)
    with pytest.raises(ValueError, match="contiguous"):
        ops.slot_vis_grid(video, recon, gen, attn=attn.transpose(2, 3).contiguous().transpose(2, 3), grid=grid)
    with pytest.raises(ValueError, match="2\\^31"):
        big = torch.zeros(1, 1, 3, 8192, 8192).expand(8, 4, 3, 8192, 8192)                    # no memory behind it
        ops.slot_vis_grid(big, big, big, attn=torch.zeros(1).expand(8, 4, 1, 1), grid=(1, 1))
    for call in (lambda: ops.slot_vis_grid(video, recon, gen, **ok),
                 lambda: ops.slot_vis_grid(video, recon, gen, attns_vis=vis, out_dtype=torch.uint8),
                 lambda: slot_misc.visualize_slots(video, recon, gen, attn, grid),
                 lambda: slot_misc.visualize_slots(video, recon, gen, attn, grid, N=2, out_dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="does not divide"):
        slot_misc.visualize_slots(video, recon, gen, attn, (4, 5))


def test_entry_point_validates_before_launching(built):
    from focus_amd import _lib
    lib = _lib.lib()
    F32, BF16, FP8 = _lib.F32, _lib.BF16, _lib.FP8_E4M3
    buf = ctypes.create_string_buffer(1 << 12)
    a = ctypes.addressof(buf)
    a += -a % 16
    ptr, odd2, odd1 = ctypes.c_void_p(a), ctypes.c_void_p(a + 2), ctypes.c_void_p(a + 1)

    def call(video=ptr, dv=F32, recon=ptr, dr=F32, gen=ptr, dg=F32, slots=ptr, ds=F32, form=1, B=3, Bg=3, T=2, C=3, H=6, W=20,
             K=3, He=3, We=5, rows=2, out=ptr, ot=0):
        return lib.focus_slot_vis_grid(video, dv, recon, dr, gen, dg, slots, ds, form, B, Bg, T, C, H, W, K, He, We, rows, out,
                                       ot, None)
    for name in ("video", "recon", "gen", "slots", "out"):
        assert call(**{name: None}) == NULL, name
    assert call(out=None, rows=0) == NULL and call(video=None, C=4, dv=FP8) == NULL          # NULL is judged first
    for kw in (dict(form=2), dict(form=-1), dict(C=1), dict(C=4), dict(K=0), dict(K=33), dict(B=0), dict(Bg=0), dict(H=0),
               dict(W=0), dict(T=-1), dict(rows=-1), dict(rows=4), dict(rows=3, Bg=2), dict(rows=3, B=2), dict(He=0),
               dict(We=0), dict(He=4), dict(We=3), dict(He=5, We=3), dict(T=1 << 20, H=64, W=64),
               dict(B=30000, Bg=30000, rows=30000, H=30000, W=30000, He=1, We=1, T=1)):
        assert call(**kw) == SHAPE, kw
    for kw in (dict(dv=FP8), dict(dr=7), dict(dg=-1), dict(ds=FP8), dict(form=0, ds=BF16), dict(ot=2), dict(ot=-1)):
        assert call(rows=0, **kw) == DTYPE, kw                                               # judged before rows == 0
    assert call(dv=FP8, C=4) == SHAPE and call(dv=FP8, video=odd1) == DTYPE                   # the order: SHAPE, DTYPE, ALIGN
    for kw in (dict(video=odd2), dict(recon=odd2), dict(gen=odd1), dict(slots=odd2), dict(out=odd2),
               dict(video=odd1, dv=BF16), dict(slots=odd1, ds=BF16)):
        assert call(rows=0, **kw) == ALIGN, kw
    assert call(rows=0, video=odd2, dv=BF16, out=odd1, ot=1) == 0                             # 2-byte bf16, 1-byte uint8
    assert call(rows=0) == 0 and call(T=0) == 0 and call(rows=0, form=0, He=0, We=7) == 0    # nothing to do; vis ignores He, We
    assert bytes(buf) == bytes(1 << 12)


def test_library_header_and_mirror_surface(built):
    from focus_amd import _lib, ops
    import focus_amd.slowfast as fs
    decl = _lib.parse_header()
    L = ctypes.CDLL(built)
    assert "focus_slot_vis_grid" in decl and hasattr(L, "focus_slot_vis_grid")
    v, i = ctypes.c_void_p, ctypes.c_int
    assert decl["focus_slot_vis_grid"][1] == [v, i, v, i, v, i, v, i] + [i] * 11 + [v, i, v]
    src = open(_lib.HEADER).read()
    assert "FOCUS_SLOT_FORM_VIS = 0, FOCUS_SLOT_FORM_RAW = 1" in src and "FOCUS_VIS_OUT_F32 = 0, FOCUS_VIS_OUT_U8 = 1" in src
    assert (ops.SLOT_FORM_VIS, ops.SLOT_FORM_RAW, ops.VIS_OUT_F32, ops.VIS_OUT_U8) == (0, 1, 0, 1)
    assert "NaN becomes 0" in src
    assert _lib.lib().focus_abi_version() == 2
    fs.install_as_slowfast()
    import importlib
    m = importlib.import_module("slowfast.utils.slot_misc")
    assert m is importlib.import_module("focus_amd.slowfast.utils.slot_misc")
    assert all(hasattr(m, n) for n in ("make_grid", "visualize", "visualize_slots"))


def test_model_and_loops_expose_the_raw_form():
    import inspect
    from focus_amd import train
    from focus_amd.slowfast.models.STEVE.steve import STEVE
    assert inspect.signature(STEVE.forward).parameters["attns"].default == "vis"
    assert inspect.signature(train.slot_train_step).parameters["raw_attns"].default is False
    assert list(inspect.signature(train.slot_val_epoch).parameters) == ["val_loader", "model", "cur_epoch", "cfg", "opd", "writer"]
