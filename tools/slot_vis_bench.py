"""STEVE epoch visualisation on the device: utils/slot_misc.visualize_slots (one launch of csrc/slot_vis.hip) against the
reference's composition, and the training step with and without the per-step overlays.

    python tools/slot_vis_bench.py [--rounds 7] [--iters 5] [--step-rounds 5] [--steps 3] [--batch 16] [--out FILE]

(a) Visualisation at N=8 clips, T=24, K=11, 128x128 frames, the slot grid 64x64 (N = 4096 cells, sy = sx = 2):
      visualize_slots uint8 / fp32   from the slot update's attention [8,24,4096,11], no overlays in memory;
      torch loop                     utils/slot_misc.visualize_loop on the overlays [8,24,11,3,128,128] that forward made: per
                                     frame one cat and one make_grid (a fill and N (K + 3) narrow().copy_()) -- what the
                                     reference runs, and the only thing the parent commit could run.
    Whole calls, host clock around `iters` calls that end in a device synchronise, after a warm-up, the arms alternating round
    by round; median, min and max over the rounds and the per-round ratio.  Then the kernel alone with device events: its time
    and its algorithmic bytes (the canvas once, every source once) per second against the HBM peak (8 TB/s; about 6.3 TB/s
    achievable).
(b) The whole-model training step of bench.py's steve_model workload (24x128x128, 11 slots, bf16 token path) at --batch:
    slot_train_step(..., raw_attns=True) against the default, alternating round by round; ms per step over `steps` steps and
    torch.cuda.max_memory_allocated of each arm."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from focus_amd import _lib, ops  # noqa: E402
from focus_amd.slowfast.utils import slot_misc  # noqa: E402

N, T, K, H, W, GRID = 8, 24, 11, 128, 128, (64, 64)
HBM_PEAK = 8.0e12


def wall(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3                         # ms per call


def stat(t):
    return "median %9.3f ms   min %9.3f   max %9.3f" % (statistics.median(t), min(t), max(t))


def part_a(args, say):
    g = torch.Generator().manual_seed(0)
    video, recon, gen = (torch.rand(N, T, 3, H, W, generator=g).cuda() for _ in range(3))
    attn = torch.softmax(torch.randn(N, T, GRID[0] * GRID[1], K, generator=g), dim=-1).cuda()
    a = attn.transpose(-1, -2).reshape(N, T, K, 1, *GRID).repeat_interleave(H // GRID[0], dim=-2) \
        .repeat_interleave(W // GRID[1], dim=-1)
    vis = video.unsqueeze(2) * a + (1.0 - a)                               # steve.py:314-319, what forward returns
    del a
    arms = (("visualize_slots uint8", lambda: slot_misc.visualize_slots(video, recon, gen, attn, GRID, N=N, out_dtype=torch.uint8)),
            ("visualize_slots fp32", lambda: slot_misc.visualize_slots(video, recon, gen, attn, GRID, N=N)),
            ("torch loop on overlays", lambda: slot_misc.visualize_loop(video, recon, gen, vis, K, N)))
    ref = arms[2][1]()
    same = torch.equal(arms[1][1]().view(torch.int32), ref.view(torch.int32))
    same8 = torch.equal(arms[0][1](), (ref * 255).clip(0, 255).to(torch.uint8))
    say("(a) N=%d, T=%d, K=%d, %dx%d, grid %dx%d -> video %s; fp32 bit-equal to the loop: %s, uint8 equal to its bytes: %s" % (
        N, T, K, H, W, GRID[0], GRID[1], list(ref.shape), same, same8))
    del ref
    for _name, fn in arms:
        wall(fn, 2)
    times = {name: [] for name, _f in arms}
    for _ in range(args.rounds):
        for name, fn in arms:
            times[name].append(wall(fn, args.iters))
    say("  whole calls, %d rounds x %d calls, alternated:" % (args.rounds, args.iters))
    for name, _f in arms:
        say("    %-24s %s" % (name, stat(times[name])))
    for name in ("visualize_slots uint8", "visualize_slots fp32"):
        ratio = [b / c for b, c in zip(times["torch loop on overlays"], times[name])]
        say("    torch loop / %s per round: median %.1fx, min %.1fx, max %.1fx" % (name, statistics.median(ratio), min(ratio), max(ratio)))
    shape = ops.slot_vis_grid_shape(T, H, W, K, N)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    say("  kernel alone (10 back-to-back launches per round, device events):")
    for name, u8, form, slots in (("raw -> uint8", 1, ops.SLOT_FORM_RAW, attn), ("raw -> fp32", 0, ops.SLOT_FORM_RAW, attn),
                                  ("vis -> fp32", 0, ops.SLOT_FORM_VIS, vis)):
        out = torch.empty(shape, device="cuda", dtype=torch.uint8 if u8 else torch.float32)
        nbytes = out.numel() * out.element_size() + 3 * video.numel() * 4 + slots.numel() * 4

        def kernel():
            _lib.check(_lib.lib().focus_slot_vis_grid(p(video), _lib.F32, p(recon), _lib.F32, p(gen), _lib.F32, p(slots), _lib.F32,
                                                      form, N, N, T, 3, H, W, K, GRID[0], GRID[1], N, p(out), u8, stream), "slot_vis_grid")
        for _ in range(5):
            kernel()
        tk = []
        for _ in range(args.rounds):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(10):
                kernel()
            e.record()
            e.synchronize()
            tk.append(s.elapsed_time(e) / 10)
        med = statistics.median(tk)
        say("    %-13s median %7.3f ms   min %7.3f   max %7.3f   %7.1f MB algorithmic, %.2f TB/s, %.0f%% of the %.0f TB/s HBM peak" % (
            name, med, min(tk), max(tk), nbytes / 1e6, nbytes / (med * 1e-3) / 1e12, 100.0 * nbytes / (med * 1e-3) / HBM_PEAK,
            HBM_PEAK / 1e12))
        del out


def part_b(args, say):
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.models import MODEL_REGISTRY
    from focus_amd.slowfast.models.optimizer import construct_optimizer_slot
    from focus_amd.train import slot_train_step
    cfg = get_cfg()                                                        # bench.py: bench_steve_model
    cfg.MODEL.MODEL_NAME = "STEVE"
    cfg.NUM_GPUS = 1
    cfg.TRAIN.MIXED_PRECISION = True
    cfg.SOLVER.OPTIMIZING_METHOD = "adam"
    cfg.SOLVER.CLIP_GRAD_L2NORM = 0.05
    sl = cfg.SLOTS
    sl.NUM_ITERS, sl.NUM_SLOTS, sl.CNN_HID_SIZE, sl.SIZE, sl.DIM, sl.MLP_HID_SIZE, sl.IMG_SIZE, sl.VOCAB_SIZE = 3, 11, 64, 192, 192, 768, 128, 4096
    sl.NUM_PREDICTOR_BLOCKS, sl.NUM_PREDICTOR_HEADS, sl.PREDICTOR_DROPOUT = 1, 4, 0.0
    sl.DECODER.DIM, sl.DECODER.NUM_BLOCKS, sl.DECODER.NUM_HEADS, sl.DECODER.DROPOUT = 192, 8, 4, 0.1
    B = args.batch
    torch.manual_seed(0)
    m = MODEL_REGISTRY.get("STEVE")(cfg).cuda().train()
    opt = construct_optimizer_slot(m, cfg)
    video = torch.rand(B, 24, 3, 128, 128, device="cuda")
    step = [0]

    def run(raw, n):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(n):
            out = slot_train_step(m, opt, video, step[0], cfg, raw_attns=raw)
            step[0] += 1
            shape = tuple(out[4].shape)
            del out
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, torch.cuda.max_memory_allocated(), shape
    for raw in (True, False, True, False):
        run(raw, 1)
    arms = (("raw_attns=True", True), ("default (overlays)", False))
    ms = {name: [] for name, _r in arms}
    peak, shapes = {}, {}
    for _ in range(args.step_rounds):
        for name, raw in arms:
            t, pk, shapes[name] = run(raw, args.steps)
            ms[name].append(t)
            peak[name] = max(peak.get(name, 0), pk)
    say("(b) STEVE training step, 24x128x128, 11 slots, bf16 token path, batch %d; %d rounds x %d steps, alternated:" % (
        B, args.step_rounds, args.steps))
    for name, _r in arms:
        say("    %-20s %s   peak %8.1f MiB   attns %s" % (name, stat(ms[name]), peak[name] / 2 ** 20, list(shapes[name])))
    d = peak["default (overlays)"] - peak["raw_attns=True"]
    say("    peak memory: default - raw = %.1f MiB (overlays %.1f MiB + upsampled masks %.1f MiB by their shapes)" % (
        d / 2 ** 20, B * 24 * 11 * 3 * 128 * 128 * 4 / 2 ** 20, B * 24 * 11 * 128 * 128 * 4 / 2 ** 20))
    ratio = [a / b for a, b in zip(ms["raw_attns=True"], ms["default (overlays)"])]
    say("    raw / default per round: median %.4f, min %.4f, max %.4f" % (statistics.median(ratio), min(ratio), max(ratio)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slot_vis_bench: needs the MI355X (timings from a CPU say nothing about it)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("device: %s" % torch.cuda.get_device_name(0))
    part_a(args, say)
    torch.cuda.empty_cache()
    if not args.skip_step:
        part_b(args, say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
