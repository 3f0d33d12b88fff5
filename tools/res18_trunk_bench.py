"""STEVE's ResNet-18 trunk (MODEL.CNN_NAME = res18) at the base.yaml shape: 16 clips x 4 frames = 64 frames of 3x64x64.

Trunk forward + backward with the BatchNorm / max-pool on the HIP kernels (FOCUS_STEVE_BN=1) and on ATen / MIOpen
(FOCUS_STEVE_BN=0) -- same module, same weights, same convolutions -- in alternated rounds, fp32 and bf16 (autocast, as
STEVE._conv runs it), each round --iters steps between two device events.  Then every entry point of csrc/batchnorm.hip by
itself at the two row counts of the trunk (R = 262144 before the pool, 65536 after it; C = 64) with the bytes it has to
move: calls between device events; focus_bn_stats is two kernels and focus_bn_bwd three, so their per-kernel times come
from a kernel trace of `--kernels-only` (the same calls, nothing else), which profiles/res18_trunk.txt quotes.

usage: python tools/res18_trunk_bench.py [--rounds 5] [--iters 20] [--out FILE] [--kernels-only] [--rows R]"""
import argparse
import ctypes
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

FRAMES, SIDE, C = 64, 64, 64


def trunk(dev):
    from focus_amd.slowfast.models.STEVE.steve import Res18Block
    args = types.SimpleNamespace(SLOTS=types.SimpleNamespace(IMG_CHANNELS=3, CNN_HID_SIZE=64, IMG_SIZE=64,
                                                             DECODER=types.SimpleNamespace(DIM=192)))
    torch.manual_seed(0)
    return Res18Block(args).to(dev).to(memory_format=torch.channels_last).train()


def step(m, x, ct, bf16):
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        y = m(x)
    y.backward(ct.to(y.dtype))


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def entry_points(R, dtype, dev):
    """[(name, bytes moved, callable)] for one row count: every tensor of the call read or written once per kernel."""
    from focus_amd import _lib
    L = _lib.lib()
    es = 2 if dtype == torch.bfloat16 else 4
    dt = _lib.BF16 if dtype == torch.bfloat16 else _lib.F32
    s = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(0)
    t = lambda: torch.randn(R, C, generator=g).to(dtype).to(dev)
    x, dy, res, y, dx, dres = t(), t(), t(), t(), t(), t()
    v = lambda: torch.ones(C, device=dev)
    mean, rstd, gamma, beta, dg, db, rm, rv = v(), v(), v(), v(), v(), v(), v(), v()
    ws = torch.empty(L.focus_bn_workspace_bytes(R, C), device=dev, dtype=torch.uint8)
    p = lambda a: a.data_ptr()
    n = R * C * es
    N, H = R // (SIDE * SIDE) if R >= SIDE * SIDE else 1, SIDE
    out = [
        ("bn_stats", n, lambda: L.focus_bn_stats(p(x), p(mean), p(rstd), p(rm), p(rv), p(ws), R, C, 1e-5, 0.1, dt, s())),
        ("bn_apply relu", 2 * n, lambda: L.focus_bn_apply(p(x), p(mean), p(rstd), p(gamma), p(beta), None, p(y), R, C, 1, dt, s())),
        ("bn_apply relu+residual", 3 * n, lambda: L.focus_bn_apply(p(x), p(mean), p(rstd), p(gamma), p(beta), p(res), p(y), R, C, 1, dt, s())),
        ("bn_bwd relu (reduce + dx)", 3 * n + 4 * n, lambda: L.focus_bn_bwd(p(dy), p(x), p(y), p(mean), p(rstd), p(gamma), p(dx), None, p(dg), p(db), p(ws), R, C, 1, 0, dt, s())),
        ("bn_bwd relu+dres (reduce + dx)", 3 * n + 5 * n, lambda: L.focus_bn_bwd(p(dy), p(x), p(y), p(mean), p(rstd), p(gamma), p(dx), p(dres), p(dg), p(db), p(ws), R, C, 1, 0, dt, s())),
    ]
    if R == FRAMES * SIDE * SIDE:                                      # the pool sits at the larger map only
        OH = (H - 1) // 2 + 1
        no = N * OH * OH * C
        py, pidx, pdy = torch.empty(no, device=dev, dtype=dtype), torch.empty(no, device=dev, dtype=torch.int8), torch.randn(no, device=dev).to(dtype)
        out += [
            ("maxpool_fwd", n + no * (es + 1), lambda: L.focus_maxpool_fwd(p(x), p(py), p(pidx), N, H, H, C, dt, s())),
            ("maxpool_bwd", n + no * (es + 1), lambda: L.focus_maxpool_bwd(p(pdy), p(pidx), p(dx), N, H, H, C, dt, s())),
        ]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--rows", type=int, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    rows = [a.rows] if a.rows else [FRAMES * SIDE * SIDE, FRAMES * SIDE * SIDE // 4]
    if a.kernels_only:                                                  # for a kernel trace: the entry points alone
        for dtype in (torch.float32, torch.bfloat16):
            for R in rows:
                for name, nbytes, fn in entry_points(R, dtype, dev):
                    for _ in range(30):
                        assert fn() == 0
        torch.cuda.synchronize()
        return

    m = trunk(dev)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(FRAMES, 3, SIDE, SIDE, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    ct = torch.randn(FRAMES, 192, SIDE, SIDE, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    say("ResNet-18 trunk of STEVE, forward + backward, %d frames of 3x%dx%d, ms per step (device events, %d steps per round)"
        % (FRAMES, SIDE, SIDE, a.iters))
    for bf16 in (False, True):
        for hip in (True, False):                                      # warm-up: code objects, MIOpen's algorithm choice
            m.hip_bn = hip
            for _ in range(5):
                step(m, x, ct, bf16)
        ts = {True: [], False: []}
        for _ in range(a.rounds):
            for hip in (True, False):
                m.hip_bn = hip
                ts[hip].append(timed(lambda: step(m, x, ct, bf16), a.iters))
        for hip in (True, False):
            v = sorted(ts[hip])
            say("  %-5s FOCUS_STEVE_BN=%d  median %.3f  min %.3f  max %.3f   rounds %s"
                % ("bf16" if bf16 else "fp32", int(hip), v[len(v) // 2], v[0], v[-1], " ".join("%.3f" % t for t in ts[hip])))
    say()
    say("entry points of csrc/batchnorm.hip alone, C = %d: us per call (device events, 50 calls), bytes each kernel has to move, GB/s" % C)
    for dtype in (torch.float32, torch.bfloat16):
        for R in rows:
            for name, nbytes, fn in entry_points(R, dtype, dev):
                for _ in range(10):
                    assert fn() == 0
                ms = min(timed(fn, 50) for _ in range(3))
                say("  %-5s R=%-7d %-32s %8.1f us  %7.1f MB  %7.0f GB/s"
                    % ("bf16" if dtype == torch.bfloat16 else "fp32", R, name, ms * 1e3, nbytes / 1e6, nbytes / ms / 1e6))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
