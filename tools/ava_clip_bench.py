"""Device AVA clip preprocessing: the sampler with the colour stage (datasets/device_sampling.sample_ava_clips ->
clip_color.hip, at most two launches) against the same plans run through the mirror's torch functions (datasets/transform.py)
on the same device clips -- the composition that is all there is without the kernels.

    python tools/ava_clip_bench.py [--rounds 7] [--iters 20] [--trace DIR] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ava_clip_bench.py --kernels-only 20

Workload: batch 8 of 16x240x427 uint8 BGR clips -> 224^2 bf16, jitter [256, 320], AVA.TRAIN_USE_COLOR_AUGMENTATION with the
full colour jitter (brightness, contrast, saturation in a drawn order + PCA lighting) and with PCA lighting only.  Both arms
get the same seeds, so they draw the same plans; their outputs are compared.  The arms are timed with device events after a
warm-up, alternating round by round, each timing ending in a synchronise; the spread over the rounds is printed beside the
medians.  Both timings are whole calls (host draws, the table copy and the launches included).  Kernel times come from a
separate traced run (--kernels-only calls the two C entry points back to back on a prebuilt table; --trace DIR reads its
*_kernel_trace.csv): the algorithm's bytes (the unique source bytes inside the sampled rectangles, read once, + the output
bytes) over the kernels' time against the HBM peak.  The temporaries of an arm are the peak of the allocator above the
resident clips during one call, minus the returned batch."""
import argparse
import collections
import csv
import ctypes
import glob
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from focus_amd import _lib, ops  # noqa: E402
from focus_amd.slowfast.config.defaults import get_cfg  # noqa: E402
from focus_amd.slowfast.datasets import device_sampling as ds  # noqa: E402
from focus_amd.slowfast.datasets import transform  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E specification
B, T, H, W, CROP, LO, HI = 8, 16, 240, 427, 224, 256, 320


def make_cfg(pca_only):
    cfg = get_cfg()
    cfg.DATA.MEAN, cfg.DATA.STD = [0.45, 0.45, 0.45], [0.225, 0.225, 0.225]
    cfg.DATA.TRAIN_JITTER_SCALES, cfg.DATA.TRAIN_CROP_SIZE = [LO, HI], CROP
    cfg.AVA.TRAIN_USE_COLOR_AUGMENTATION, cfg.AVA.TRAIN_PCA_JITTER_ONLY = True, pca_only
    cfg.TRAIN.MIXED_PRECISION = True
    return cfg


def composition(cfg, clips):
    """ava_dataset.py:268-365 with the mirror functions, per clip, on the device."""
    out = []
    ev, evec = np.array(cfg.DATA.TRAIN_PCA_EIGVAL).astype(np.float32), np.array(cfg.DATA.TRAIN_PCA_EIGVEC).astype(np.float32)
    mean, std = np.array(cfg.DATA.MEAN, dtype=np.float32), np.array(cfg.DATA.STD, dtype=np.float32)
    for c in clips:
        f = c.permute(0, 3, 1, 2).float() / 255.0
        f, _ = transform.random_short_side_scale_jitter(f, LO, HI)
        f, _ = transform.random_crop(f, CROP)
        f, _ = transform.horizontal_flip(0.5, f)
        if not cfg.AVA.TRAIN_PCA_JITTER_ONLY:
            f = transform.color_jitter(f, 0.4, 0.4, 0.4)
        f = transform.lighting_jitter(f, 0.1, ev, evec)
        f = transform.color_normalization(f, mean, std)
        if not cfg.AVA.BGR:
            f = f[:, [2, 1, 0], ...]
        out.append(f.permute(1, 0, 2, 3).to(torch.bfloat16))
    return torch.stack(out)


def timed(fn, iters, seed):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    np.random.seed(seed)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # microseconds per call


def temporaries(fn):
    """Peak bytes the allocator held above what was resident before the call, minus the returned batch."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    np.random.seed(3)
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base - out.numel() * out.element_size()


def prebuilt(cfg, clips, boxes):
    """The tables of one batch on the device and the two C calls on them."""
    np.random.seed(3)
    plans = [ds.ava_plan(cfg, H, W, b, "train") for b in boxes]
    params, colors = [p for p, _, _ in plans], [c for _, c, _ in plans]
    items = torch.from_numpy(ops.clip_items(clips, params, CROP, CROP)).cuda()
    cols = torch.from_numpy(ops.clip_colors(colors, B)).cuda()
    out = torch.empty(B, 3, T, CROP, CROP, device="cuda", dtype=torch.bfloat16)
    fm = torch.zeros(B * T, device="cuda")
    L, vp = _lib.lib(), lambda t: ctypes.c_void_p(t.data_ptr())
    nbytes = int(L.focus_clip_color_workspace_bytes(B, T, CROP, CROP))
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    f3 = lambda v: ctypes.cast((ctypes.c_float * 3)(*v), ctypes.c_void_p)
    keep = [f3(cfg.DATA.MEAN), f3(cfg.DATA.STD), f3(ds.GRAY_BGR)]
    contrast = any(ops.COLOR_CONTRAST in c["op"] for c in colors)
    plane = CROP * CROP

    def launch():
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if contrast:
            _lib.check(L.focus_clip_gray_mean(vp(items), vp(cols), B, T, CROP, CROP, keep[2], vp(fm), vp(ws), nbytes, s), "clip_gray_mean")
        _lib.check(L.focus_clip_sample_color(vp(items), vp(cols), vp(fm), B, T, CROP, CROP, vp(out), 3 * T * plane, T * plane, plane,
                                             keep[0], keep[1], keep[2], 1, _lib.BF16, s), "clip_sample_color")
    src = sum(T * p["sh"] * p["sw"] * 3 for p in params)
    return launch, src, out.numel() * 2, (items, cols, out, fm, ws, keep)


def kernel_times(trace_dir):
    """name -> [calls, total us] of the two kernels from a rocprofv3 --kernel-trace CSV."""
    files = glob.glob(os.path.join(trace_dir, "**", "*_kernel_trace.csv"), recursive=True)
    agg = collections.defaultdict(lambda: [0, 0.0])
    for f in files:
        for r in csv.DictReader(open(f)):
            for key in ("clip_gray_mean_kernel", "clip_sample_color_kernel"):
                if key in r["Kernel_Name"]:
                    agg[key][0] += 1
                    agg[key][1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    return agg


def run(name, pca_only, clips, boxes, rounds, iters, emit):
    cfg = make_cfg(pca_only)
    new = lambda: ds.sample_ava_clips(cfg, clips, boxes, "train")[0]
    old = lambda: composition(cfg, clips)
    np.random.seed(3)
    x_new = new()
    np.random.seed(3)
    x_old = old()
    diff = float((x_new.float() - x_old.float()).abs().max())
    emit("%s: batch %d of %dx%dx%d uint8 -> %d^2 bf16, jitter [%d, %d]" % (name, B, T, H, W, CROP, LO, HI))
    top = float(x_old.float().abs().max())
    emit("  outputs, same seed: max |kernels - composition| = %.4f at |value| <= %.2f (bf16 spacing there %.4f)" % (
        diff, top, 2.0 ** (int(np.floor(np.log2(top))) - 7)))
    launch, src, dst, keep = prebuilt(cfg, clips, boxes)
    for fn in (new, old, launch):
        timed(fn, 5, 100)
    t_new, t_old, t_launch = [], [], []
    for r in range(rounds):
        t_new.append(timed(new, iters, 200 + r))
        t_old.append(timed(old, iters, 200 + r))
        t_launch.append(timed(launch, iters, 200 + r))
    med = statistics.median
    for label, t in (("sample_ava_clips (new)", t_new), ("torch composition", t_old), ("C calls back to back", t_launch)):
        emit("  %-24s median %9.1f us   min %9.1f   max %9.1f   (%d rounds x %d calls)" % (label, med(t), min(t), max(t), rounds, iters))
    ratios = [o / n for o, n in zip(t_old, t_new)]
    emit("  composition / sample_ava_clips per round: median %.2fx, min %.2fx, max %.2fx%s" % (
        med(ratios), min(ratios), max(ratios), "" if min(ratios) > 1 else "   (NOT faster in every round)"))
    emit("  temporaries of one call: sample_ava_clips %.2f MB, composition %.1f MB (the batch itself: %.1f MB)" % (
        temporaries(new) / 1e6, temporaries(old) / 1e6, dst / 1e6))
    emit("  algorithmic bytes %.1f MB (source rectangles %.1f, read once, + output %.1f): %.2f TB/s over the back-to-back time"
         % ((src + dst) / 1e6, src / 1e6, dst / 1e6, (src + dst) / (med(t_launch) * 1e-6) / 1e12))
    return src + dst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernels-only", type=int, default=0, help="only N back-to-back pairs of C calls (for a traced run)")
    ap.add_argument("--trace", default="", help="directory of a rocprofv3 --kernel-trace run of --kernels-only")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ava_clip_bench: needs the GPU (nothing is measured without one)")
    g = torch.Generator().manual_seed(1)
    clips = [torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(B)]
    boxes = [np.array([[0.1, 0.2, 0.6, 0.9], [0.4, 0.1, 0.95, 0.7]]) for _ in range(B)]
    if args.kernels_only:
        launch, _, _, keep = prebuilt(make_cfg(False), clips, boxes)
        for _ in range(args.kernels_only):
            launch()
        torch.cuda.synchronize()
        return
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("device: %s" % torch.cuda.get_device_name(0))
    nbytes = run("full colour jitter", False, clips, boxes, args.rounds, args.iters, emit)
    run("PCA lighting only", True, clips, boxes, args.rounds, args.iters, emit)
    if args.trace:
        agg = kernel_times(args.trace)
        emit("kernel times, full colour jitter (rocprofv3 --kernel-trace of --kernels-only, every launch):")
        total = 0.0
        for k, (n, us) in sorted(agg.items()):
            emit("  %-26s %4d launches   average %8.1f us" % (k, n, us / max(n, 1)))
            total += us / max(n, 1)
        if total:
            emit("  both: %.1f us -> %.2f TB/s of algorithmic bytes = %.1f%% of the %.1f TB/s HBM peak" % (
                total, nbytes / (total * 1e-6) / 1e12, 100.0 * nbytes / (total * 1e-6) / HBM_PEAK, HBM_PEAK / 1e12))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
