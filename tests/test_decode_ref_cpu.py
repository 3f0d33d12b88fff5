"""CPU-side checks of cached generation: the incremental reference of tests/decode_ref.py against the oracle's full pass,
and the argument validation of focus_decode_attn / focus_greedy_next, which happens before any launch."""
import ctypes

import pytest
import torch

import decode_ref
from conftest import load_golden


@pytest.fixture(scope="module")
def built():
    from focus_amd.build import build
    return build(verbose=False)


def test_incremental_reference_reproduces_the_full_pass(oracle):
    """Teacher-forced over a random sequence, decode_ref.IncrementalDecoder returns every row of
    oracle.transformer_decoder (pinned by the reference's steve_forward_small fixture) in fp64."""
    _, p = load_golden("steve_forward_small", torch.float64)
    B, T, K, D, H, NB = 3, 16, 3, 32, 2, 2
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    enc = torch.randn(B, K, D, generator=g, dtype=torch.float64)
    full = oracle.transformer_decoder(p, "steve_decoder.tf", x, enc, H, NB)
    dec = decode_ref.IncrementalDecoder(oracle, p, "steve_decoder.tf", enc, H, NB, T)
    rows = torch.stack([dec.step(x[:, t], t) for t in range(T)], dim=1)
    assert rows.shape == full.shape
    assert float((rows - full).abs().max()) <= 1e-12
    # a cache longer than the sequence and garbage behind the valid rows change nothing
    dec = decode_ref.IncrementalDecoder(oracle, p, "steve_decoder.tf", enc, H, NB, T + 5)
    for j in range(NB):
        dec.k[j].fill_(float("nan"))
        dec.v[j].fill_(float("nan"))
    rows2 = torch.stack([dec.step(x[:, t], t) for t in range(T)], dim=1)
    assert torch.equal(rows2, rows)


def test_decode_kernels_validate_before_launching(built):
    """focus_decode_attn and focus_greedy_next refuse bad arguments with the ABI's error codes before any launch (no GPU
    needed), and the operators above them refuse CPU tensors and inputs that want a gradient."""
    from focus_amd import _lib, ops
    lib = _lib.lib()
    F32, BF16 = _lib.F32, _lib.BF16
    assert lib.focus_abi_version() == 2
    assert lib.focus_decode_attn_ok(1024, 48, BF16) == 1
    for d in (16, 32, 48, 64):
        assert lib.focus_decode_attn_ok(4096, d, BF16) == 1 and lib.focus_decode_attn_ok(4096, d, F32) == 1
    assert lib.focus_decode_attn_ok(1024, 50, BF16) == 0 and lib.focus_decode_attn_ok(1024, 128, F32) == 0
    assert lib.focus_decode_attn_ok(0, 48, BF16) == 0 and lib.focus_decode_attn_ok(1024, 48, _lib.FP8_E4M3) == 0
    buf = ctypes.create_string_buffer(1 << 16)
    a = ctypes.addressof(buf)
    a += -a % 16
    ptr, odd = ctypes.c_void_p(a), ctypes.c_void_p(a + 4)
    NULL, SHAPE, ALIGN = -5, -1, -3

    def call(q=ptr, ldq=192, kn=ptr, vn=ptr, ldn=192, kc=ptr, vc=ptr, ldc=192, bsc=1024 * 192, out=ptr, ldo=192, B=2,
             heads=4, d=48, length=5, Lmax=1024, dtype=BF16):
        return lib.focus_decode_attn(q, ldq, kn, vn, ldn, kc, vc, ldc, bsc, out, ldo, B, heads, d, length, Lmax, 0.1, dtype,
                                     None)

    assert call(q=None) == NULL and call(kc=None) == NULL and call(vc=None) == NULL and call(out=None) == NULL
    assert call(kn=None) == NULL and call(vn=None) == NULL                  # one of the pair without the other
    assert call(length=0) == SHAPE and call(length=1025) == SHAPE
    assert call(B=0) == SHAPE and call(heads=0) == SHAPE and call(d=0) == SHAPE and call(d=50) == SHAPE
    assert call(ldq=191) == ALIGN and call(ldc=100) == ALIGN and call(ldo=8) == ALIGN and call(ldn=190) == ALIGN
    assert call(ldq=196) == ALIGN and call(ldq=194, dtype=F32) == ALIGN     # rows of 16-byte vectors: 8 bf16, 4 fp32
    assert call(q=odd) == ALIGN and call(kn=odd) == ALIGN and call(out=odd) == ALIGN
    assert call(bsc=192) == ALIGN                                           # clips overlapping in the cache

    def nxt(lg=ptr, ldl=64, dic=ptr, pe=ptr, tok=ptr, ts=1, x=ptr, ldx=32, B=2, V=64, D=32, dtype=F32):
        return lib.focus_greedy_next(lg, ldl, dic, pe, tok, ts, x, ldx, B, V, D, dtype, None)

    assert nxt(lg=None) == NULL and nxt(dic=None) == NULL and nxt(pe=None) == NULL and nxt(tok=None) == NULL
    assert nxt(x=None) == NULL
    assert nxt(B=0) == SHAPE and nxt(V=0) == SHAPE and nxt(D=0) == SHAPE and nxt(ts=0) == SHAPE
    assert nxt(ldl=60) == ALIGN and nxt(ldx=16) == ALIGN and nxt(tok=odd) == ALIGN

    assert ops.decode_attention_ok(1024, 192, 4, torch.bfloat16) and ops.decode_attention_ok(16, 32, 2, torch.float32)
    assert not ops.decode_attention_ok(1024, 192, 5, torch.bfloat16)        # heads do not divide the width
    assert not ops.decode_attention_ok(1024, 192, 4, torch.float16)
    q, kc = torch.randn(2, 32), torch.zeros(2, 8, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.decode_attention(q, q, q, kc, kc, 1, 2, 0.25)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.greedy_next(torch.randn(2, 8), torch.randn(8, 4), torch.randn(4))
    with pytest.raises(RuntimeError, match="inference only"):
        ops.decode_attention(q.clone().requires_grad_(), q, q, kc, kc, 1, 2, 0.25)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.greedy_next(torch.randn(2, 8).requires_grad_(), torch.randn(8, 4), torch.randn(4))
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.decode_attention(q.clone().requires_grad_(), q, q, kc, kc, 1, 2, 0.25)
