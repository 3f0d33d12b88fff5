"""MX e4m3 activations in numpy (the checker of csrc/mx_quant.hip and of the MX GEMM; the product never imports this).

X [M, K] (bf16 values), blocks of 32 consecutive elements along K within a row.  For a block with largest magnitude
amax = 1.m x 2^E:  e = E - 8 + (m > 0.75), the smallest integer with amax <= 448 x 2^e, clamped to [-127, 127] (-127 for an
all-zero block); scale byte = e + 127 (0xFF when the block holds a NaN or an Inf); code = RNE_e4m3(x * 2^-e) in fp32, as
OCP e4m3fn bytes (oracle/fp8.py)."""
import numpy as np

from oracle import fp8


def bf16_bits(x):
    """uint16 bf16 bit patterns of float32 values that are bf16 values (the low 16 bits must be zero)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    assert not np.any(u & 0xFFFF), "not bf16 values"
    return (u >> 16).astype(np.uint16)


def block_exponents(x):
    """(e int32 [M, K/32], nonfinite bool [M, K/32]) of bf16-valued float32 x [M, K]."""
    x = np.asarray(x, dtype=np.float32)
    M, K = x.shape
    assert K % 32 == 0
    a = (bf16_bits(x) & 0x7FFF).astype(np.int32).reshape(M, K // 32, 32).max(-1)   # integer order = magnitude order
    E = (a >> 7) - 127
    e = E - 8 + ((a & 0x7F) > 0x60)
    return np.clip(e, -127, 127).astype(np.int32), a >= 0x7F80


def quantize(x):
    """-> (codes uint8 [M, K], scales uint8 [M, K/32])."""
    x = np.asarray(x, dtype=np.float32)
    M, K = x.shape
    e, bad = block_exponents(x)
    scales = np.where(bad, 0xFF, e + 127).astype(np.uint8)
    inv = np.ldexp(np.float32(1.0), -np.repeat(e, 32, axis=1)).astype(np.float32)    # 2^-e, exact in fp32
    codes = fp8.encode((x * inv).astype(np.float32))
    return codes, scales


def dequantize(codes, scales):
    """float64 [M, K] of the values the MX GEMM multiplies by (NaN for a non-finite block)."""
    codes = np.asarray(codes, dtype=np.uint8)
    s = np.asarray(scales, dtype=np.int32)
    v = fp8.decode(codes).astype(np.float64)
    f = np.where(s == 0xFF, np.nan, np.ldexp(1.0, s - 127))
    return v * np.repeat(f, 32, axis=1)
