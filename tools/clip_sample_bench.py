"""Device clip sampling: the one-launch sampler (datasets/device_sampling.sample_clips -> clip_sample.hip) against the
composition of the existing torch functions on the same device clips, at the sizes of the shipped ORViT configs.

    python tools/clip_sample_bench.py [--rounds 7] [--iters 20] [--out FILE]

Workloads: batch 8 of 16x240x427 uint8 clips -> 224^2 bf16 (jitter [256, 320]) and the HR variant -> 336^2 (jitter [384, 480]).
Both sides get the same seeds, so they sample the same rectangles; their outputs are compared.  The two are timed with device
events after a warm-up, alternating round by round, and the spread over the rounds is printed beside the medians.  Both
timings are whole calls (host parameter draws, the descriptor copy and the launches included), which is what a training loop
pays; the `kernel only` line calls the C entry point back to back on a prebuilt descriptor table.  The share of HBM peak is
the algorithm's bytes (the unique source bytes inside the sampled rectangles + the output bytes) over the kernel-only time:
the kernel does no arithmetic to speak of, so HBM bandwidth is the bound it is measured against."""
import argparse
import ctypes
import os
import random
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from focus_amd import _lib, ops  # noqa: E402
from focus_amd.slowfast.config.defaults import get_cfg  # noqa: E402
from focus_amd.slowfast.datasets import device_sampling as ds  # noqa: E402
from focus_amd.slowfast.datasets import transform  # noqa: E402
from focus_amd.slowfast.datasets import utils as du  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E specification


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)


def composition(cfg, clips, lo, hi, crop):
    """What the data path does today with the existing functions, per clip, on the device."""
    out = []
    for c in clips:
        f = du.tensor_normalize(c, cfg.DATA.MEAN, cfg.DATA.STD).permute(0, 3, 1, 2)
        f, _ = transform.random_short_side_scale_jitter(f, lo, hi)
        f, _ = transform.random_crop(f, crop)
        f, _ = transform.horizontal_flip(0.5, f)
        f = du.pack_pathway_output(cfg, f.permute(1, 0, 2, 3))[0]
        out.append(f.to(torch.bfloat16))
    return torch.stack(out)


def timed(fn, iters, seed):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    seed_all(seed)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # microseconds per call


def run(name, crop, lo, hi, rounds, iters, emit):
    cfg = get_cfg()
    cfg.DATA.MEAN, cfg.DATA.STD, cfg.DATA.REVERSE_INPUT_CHANNEL = [0.5] * 3, [0.5] * 3, True
    cfg.DATA.TRAIN_JITTER_SCALES, cfg.DATA.TRAIN_CROP_SIZE = [lo, hi], crop
    cfg.MODEL.ARCH, cfg.MODEL.MODEL_NAME, cfg.TRAIN.MIXED_PRECISION = "mformer", "Motionformer", True
    B, T, H, W, O = 8, 16, 240, 427, 4
    g = torch.Generator().manual_seed(1)
    clips = [torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(B)]
    boxes = [np.tile(np.array([10.0, 20.0, 200.0, 180.0], dtype=np.float32), (T, O, 1)) for _ in range(B)]
    new = lambda: ds.sample_clips(cfg, clips, boxes, -1)[0]
    old = lambda: composition(cfg, clips, lo, hi, crop)

    seed_all(3)
    x_new = new()
    seed_all(3)
    x_old = old()
    diff = float((x_new.float() - x_old.float()).abs().max())
    emit("%s: batch %d of %dx%dx%d uint8 -> %d^2 bf16, jitter [%d, %d]" % (name, B, T, H, W, crop, lo, hi))
    emit("  outputs, same seed: max |kernel - composition| = %.4f at |value| <= %.2f (bf16 spacing there %.4f)" % (
        diff, float(x_old.float().abs().max()), 2.0 ** -7))

    # kernel only: a prebuilt descriptor table, the C entry point called back to back
    seed_all(3)
    params = [ds.sampling_params(H, W, -1, lo, hi, crop)[0] for _ in range(B)]
    items = torch.from_numpy(ops.clip_items(clips, params, crop, crop)).cuda()
    out = torch.empty(B, 3, T, crop, crop, device="cuda", dtype=torch.bfloat16)
    mean3, std3 = (ctypes.c_float * 3)(*cfg.DATA.MEAN), (ctypes.c_float * 3)(*cfg.DATA.STD)
    L, vp = _lib.lib(), lambda t: ctypes.c_void_p(t.data_ptr())
    launch = lambda: _lib.check(L.focus_clip_sample(
        vp(items), B, T, crop, crop, vp(out), 3 * T * crop * crop, T * crop * crop, crop * crop, ctypes.cast(mean3, ctypes.c_void_p),
        ctypes.cast(std3, ctypes.c_void_p), 1, _lib.BF16, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "clip_sample")
    for fn in (new, old, launch):
        timed(fn, 5, 100)
    t_new, t_old, t_launch = [], [], []
    for r in range(rounds):
        t_new.append(timed(new, iters, 200 + r))
        t_old.append(timed(old, iters, 200 + r))
        t_launch.append(timed(launch, iters, 200 + r))
    med = statistics.median
    for label, t in (("sample_clips (new)", t_new), ("composition (parent)", t_old), ("kernel only", t_launch)):
        emit("  %-22s median %9.1f us   min %9.1f   max %9.1f   (%d rounds x %d calls)" % (label, med(t), min(t), max(t), rounds, iters))
    ratios = [o / n for o, n in zip(t_old, t_new)]
    emit("  composition / sample_clips per round: median %.2fx, min %.2fx, max %.2fx" % (med(ratios), min(ratios), max(ratios)))
    src = sum(T * p["sh"] * p["sw"] * 3 for p in params)
    dst = B * 3 * T * crop * crop * 2
    emit("  algorithmic bytes %.1f MB (source rectangles %.1f + output %.1f): %.2f TB/s over the kernel-only time = %.1f%% of the "
         "%.1f TB/s HBM peak (HBM-bound)" % (
             (src + dst) / 1e6, src / 1e6, dst / 1e6, (src + dst) / (med(t_launch) * 1e-6) / 1e12,
             100.0 * (src + dst) / (med(t_launch) * 1e-6) / HBM_PEAK, HBM_PEAK / 1e12))
    return med(ratios), min(ratios)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_sample_bench: needs the GPU (nothing is measured without one)")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("device: %s" % torch.cuda.get_device_name(0))
    run("224", 224, 256, 320, args.rounds, args.iters, emit)
    run("HR 336", 336, 384, 480, args.rounds, args.iters, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
