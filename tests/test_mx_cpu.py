"""MX e4m3 activations (TRAIN.FP8_ACTIVATIONS) without a GPU: the numpy reference (tests/mx_ref.py) pinned on hand-derived
blocks, the config key, and the argument checks of focus_mx_quant / focus_gemm_mx before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import mx_ref


def _block(*vals):
    """One row of one 32-element block: vals, then zeros (float32 values that are bf16 values)."""
    x = np.zeros((1, 32), dtype=np.float32)
    x[0, :len(vals)] = vals
    return x


def _q(*vals):
    codes, scales = mx_ref.quantize(_block(*vals))
    return codes[0], int(scales[0, 0])


def test_powers_of_two():
    # amax = 1.0 = 2^0: e = 0 - 8, scale 119, 1.0 * 2^8 = 256 = e4m3 0x78 (exponent field 15, mantissa 0)
    c, s = _q(1.0, 0.5, -0.25)
    assert s == 119 and list(c[:3]) == [0x78, 0x70, 0xE8]
    c, s = _q(2.0 ** 20)
    assert s == 127 + 12 and c[0] == 0x78
    c, s = _q(2.0 ** -20)
    assert s == 127 - 28 and c[0] == 0x78


def test_ceiling_boundary_at_1_75():
    # amax = 1.75 * 2^E exactly: m = 0.75 is not above 0.75, e = E - 8, the block maximum lands on 448 (0x7E)
    c, s = _q(1.75, 1.0)
    assert s == 127 - 8 and c[0] == 0x7E and c[1] == 0x78
    c, s = _q(1.75 * 2.0 ** 10)
    assert s == 127 + 2 and c[0] == 0x7E
    # the next bf16 above 1.75 (1.7578125 = 1.75 + 2^-7): e = E - 7, 1.7578125 * 128 = 225 -> 224 (0x76); 1.75 -> 224
    c, s = _q(1.7578125, 1.75)
    assert s == 127 - 7 and c[0] == 0x76 and c[1] == 0x76


def test_all_zero_block_and_clamps():
    c, s = _q()
    assert s == 0 and not c.any()                       # all zero: e = -127
    c, s = _q(-0.0)
    assert s == 0 and c[0] == 0x80
    # tiny: amax = 2^-120 gives e = -128, clamped to -127: 2^-120 * 2^127 = 128 (0x70)
    c, s = _q(2.0 ** -120)
    assert s == 0 and c[0] == 0x70
    # bf16 subnormal 2^-133: e clamped to -127, 2^-133 * 2^127 = 2^-6 (0x08)
    c, s = _q(2.0 ** -133)
    assert s == 0 and c[0] == 0x08
    # the largest finite bf16 (1.9921875 * 2^127): e = 120, the top of the block rounds up to 256 (0x78); 2^127 -> 128 (0x70)
    big = np.float32(np.frombuffer(np.uint32(0x7F7F0000).tobytes(), dtype=np.float32)[0])
    c, s = _q(big, 2.0 ** 127)
    assert s == 127 + 120 and c[0] == 0x78 and c[1] == 0x70


def test_negative_values_and_ties_to_even():
    # amax 1.1875 -> e = -8.  -1.0625 * 256 = -272: halfway between 256 (mantissa 0) and 288 (mantissa 1) -> 256;
    # 1.1875 * 256 = 304: halfway between 288 (1) and 320 (2) -> 320
    c, s = _q(1.0, -1.0625, 1.1875, -1.1875)
    assert s == 119 and list(c[:4]) == [0x78, 0xF8, 0x7A, 0xFA]
    # the smallest subnormal code 2^-9 against a scale of 2^-8 (amax 1): 2^-17 * 256 = 2^-9 -> 0x01, 1.5 * 2^-18 * 256 -> 0x01
    c, s = _q(1.0, 2.0 ** -17, 1.5 * 2.0 ** -18, -(2.0 ** -18))
    assert s == 119 and list(c[1:4]) == [0x01, 0x01, 0x80]   # 0.5 of the smallest step: tie to even (0)


def test_nonfinite_blocks_and_layout():
    x = np.zeros((2, 96), dtype=np.float32)
    x[0, 5] = np.nan
    x[0, 40] = 3.0
    x[1, 70] = -np.inf
    codes, scales = mx_ref.quantize(x)
    assert codes.shape == (2, 96) and scales.shape == (2, 3)
    assert list(scales[0]) == [0xFF, 127 - 7, 0] and list(scales[1]) == [0, 0, 0xFF]
    d = mx_ref.dequantize(codes, scales)
    assert np.isnan(d[0, :32]).all() and d[0, 40] == 3.0 and np.isnan(d[1, 64:]).all()


def test_random_roundtrip_bound():
    g = np.random.default_rng(0)
    x = (g.standard_normal((64, 256)) * np.exp2(g.integers(-20, 20, (64, 1)))).astype(np.float32)
    x = torch.from_numpy(x).bfloat16().float().numpy()
    d = mx_ref.dequantize(*mx_ref.quantize(x))
    amax = np.abs(x).reshape(64, 8, 32).max(-1, keepdims=True)
    # half an e4m3 step of the block scale: 2^-4 relative to 2^floor(log2 |x|) for normals, 2^-10 * scale below them
    err = np.abs(d - x).reshape(64, 8, 32)
    assert np.all(err <= np.maximum(np.abs(x).reshape(64, 8, 32) * 2.0 ** -4, amax * 2.0 ** -18))


def test_fp8_activations_key():
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.models import build_model
    cfg = get_cfg()
    assert cfg.TRAIN.FP8_ACTIVATIONS is False and cfg.TRAIN.FP8_WEIGHTS is False
    cfg.merge_from_list(["MODEL.MODEL_NAME", "Motionformer", "TRAIN.MIXED_PRECISION", True, "TRAIN.FP8_ACTIVATIONS", True,
                         "MF.DEPTH", 1, "MF.EMBED_DIM", 64, "MF.NUM_HEADS", 4, "NUM_GPUS", 0])
    with pytest.raises(ValueError, match="FP8_ACTIVATIONS needs TRAIN.FP8_WEIGHTS"):
        build_model(cfg)


@pytest.fixture(scope="module")
def built():
    from focus_amd.build import build
    return build(verbose=False)


def test_mx_entry_points_validate_before_launching(built):
    """focus_mx_quant / focus_gemm_mx refuse bad arguments with the ABI's codes before any launch (no GPU needed); the
    operators above them refuse CPU tensors."""
    from focus_amd import _lib, ops
    lib = _lib.lib()
    F32, BF16, FP8 = _lib.F32, _lib.BF16, _lib.FP8_E4M3
    buf = ctypes.create_string_buffer(1 << 16)
    a = ctypes.addressof(buf)
    a += -a % 16
    ptr, odd = ctypes.c_void_p(a), ctypes.c_void_p(a + 4)
    NULL, SHAPE, DTYPE, ALIGN = -5, -1, -2, -3
    q = lambda x=ptr, ldx=64, rows=4, cols=64, dt=BF16, c=ptr, ldc=64, s=ptr, lds=4: lib.focus_mx_quant(
        x, ldx, rows, cols, dt, c, ldc, s, lds, None)
    assert q(x=None) == NULL and q(c=None) == NULL and q(s=None) == NULL
    assert q(dt=F32) == DTYPE and q(dt=FP8) == DTYPE
    assert q(cols=48) == SHAPE and q(cols=0) == SHAPE and q(rows=-1) == SHAPE and q(ldx=32) == SHAPE and q(lds=1) == SHAPE
    assert q(x=odd) == ALIGN and q(ldx=68) == ALIGN and q(c=odd) == ALIGN and q(ldc=72) == ALIGN and q(lds=6) == ALIGN
    assert q(rows=0) == 0                                         # nothing to do, nothing launched

    def g(**kw):
        d = _lib.GemmDesc()
        d.M, d.N, d.K, d.batch0, d.batch1 = 64, 64, 128, 1, 1
        d.A, d.rsA, d.csA = a, 128, 1
        d.B, d.rsB, d.csB = a, 1, 128
        d.C, d.rsC, d.csC = a, 64, 1
        d.alpha, d.dtype_ab, d.dtype_b, d.dtype_c, d.b_scale = 1.0, FP8, FP8, BF16, a
        sc, ld = kw.pop("scales", ptr), kw.pop("ld", 4)
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.focus_gemm_mx(ctypes.byref(d), sc, ld, None)
    assert g(scales=None) == NULL and g(b_scale=None) == NULL and g(A=None) == NULL and g(C=None) == NULL
    assert g(dtype_ab=BF16) == DTYPE and g(dtype_b=0) == DTYPE and g(dtype_c=F32) == DTYPE
    assert g(K=192, rsA=192, csB=192) == SHAPE and g(N=96, rsC=96) == SHAPE and g(batch0=2) == SHAPE
    assert g(epilogue=_lib.EPI_TANH) == SHAPE and g(csA=2) == SHAPE and g(ld=2) == SHAPE and g(rsA=64) == SHAPE
    assert g(A=a + 8) == ALIGN and g(rsA=136) == ALIGN and g(scales=ctypes.c_void_p(a + 2)) == ALIGN and g(ld=8 + 2) == ALIGN
    assert g(residual=a + 8) == ALIGN
    x = torch.randn(4, 64).bfloat16()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mx_quantize(x)
