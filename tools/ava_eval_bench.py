"""The AVA evaluation on the device against the host evaluation, on one synthetic validation set.

    python tools/ava_eval_bench.py [--images 50000] [--rounds 3] [--out profiles/ava_eval_bench.txt]

The table: `images` key frames over 64 videos, 3 persons each with 2-3 labels out of 80 classes (60 of them in the label
map, frequencies ~ 1 / rank), and 3 detection boxes per frame -- the persons' boxes with some jitter -- with random scores.

  1  The two arms alternate round by round (A, B, A, B, ...); every round is a wall clock that ends in a device synchronise,
     every round is printed, the medians are compared.  A: meters.AVAMeter.finalize_metrics on the rows on the host (the
     vectorised numpy evaluation; not the reference's Python loop, which is not part of this repository).
     B: meters.DeviceAVAMeter.finalize_metrics on the rows on the device: the grouping sort, focus_ava_match, focus_voc_ap, one copy.
  2  The kernels alone (device time from the profiler's kernel records), with what bounds them: ava_match_kernel reads 16
     bytes per row and writes one byte per (row, class) -- the byte table against the HBM rate of 8 TB/s; voc_rank_kernel
     makes (rows of the class) comparisons per row of every wave that holds a true positive -- against the VALU issue
     rate, 256 CUs x 4 SIMDs x 16 lanes per clock at 2.4 GHz: the instructions per comparison that rate would allow.

No figure is gated: the tool reports what it finds."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def synthetic(images, root, seed=0):
    """Writes the annotation directory and returns (preds [K,80], ori_boxes [K,5], metadata [K,2]) float32 / float64 arrays."""
    g = np.random.RandomState(seed)
    C, V = 80, 64
    ids = np.sort(g.permutation(np.arange(1, C + 1))[:60])
    freq = 1.0 / (1.0 + g.permutation(60))
    freq /= freq.sum()
    vid = np.arange(images) % V
    sec = 902 + np.arange(images) // V
    lo = g.uniform(0.0, 0.5, (images, 3, 2))
    persons = np.round(np.concatenate([lo, lo + g.uniform(0.15, 0.5, (images, 3, 2))], axis=2), 3)      # x1, y1, x2, y2
    with open(os.path.join(root, "gt.csv"), "w") as f:
        for i in range(images):
            for p in range(3):
                b = persons[i, p]
                for c in g.choice(ids, size=g.randint(2, 4), replace=False, p=freq):
                    f.write("v%02d,%04d,%.3f,%.3f,%.3f,%.3f,%d,%d\n" % (vid[i], sec[i], b[0], b[1], b[2], b[3], c, p))
    with open(os.path.join(root, "excl.csv"), "w") as f:
        for i in g.permutation(images)[:images // 100]:
            f.write("v%02d,%04d\n" % (vid[i], sec[i]))
    with open(os.path.join(root, "labelmap.pbtxt"), "w") as f:
        for c in ids:
            f.write('item {\n  name: "action %d"\n  id: %d\n}\n' % (c, c))
    with open(os.path.join(root, "val.csv"), "w") as f:
        f.write("original_video_id video_id frame_id path labels\n")
        for v in range(V):
            f.write('v%02d %d 0 v%02d/0.jpg ""\n' % (v, v, v))
    boxes = (persons + g.normal(0, 0.03, persons.shape)).reshape(-1, 4).astype(np.float32)
    K = boxes.shape[0]
    ori = np.concatenate([np.zeros((K, 1), np.float32), boxes], axis=1)
    metadata = np.stack([np.repeat(vid, 3), np.repeat(sec, 3)], axis=1).astype(np.float64)
    preds = g.rand(K, C).astype(np.float32)
    return preds, ori, metadata


def make_cfg(root):
    from focus_amd.slowfast.config.defaults import get_cfg
    cfg = get_cfg()
    cfg.AVA.ANNOTATION_DIR = cfg.AVA.FRAME_LIST_DIR = root
    cfg.AVA.GROUNDTRUTH_FILE, cfg.AVA.EXCLUSION_FILE, cfg.AVA.LABEL_MAP_FILE = "gt.csv", "excl.csv", "labelmap.pbtxt"
    return cfg


def kernel_times(fn, names, iters=5):
    from torch.profiler import ProfilerActivity, profile
    fn()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    out = {}
    for name in names:
        d = [getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0) for e in prof.events() if name in e.name]
        out[name] = (statistics.median(d) if d else float("nan"), len(d))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=50000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ava_eval_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ava_eval_bench: needs the GPU (a timing taken elsewhere says nothing)")
    from focus_amd.slowfast.utils import meters
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("ava_eval_bench on %s: %d key frames, 3 boxes each, 80 classes, 60 in the label map" % (
        torch.cuda.get_device_name(0), args.images))
    with tempfile.TemporaryDirectory() as root:
        t = time.perf_counter()
        preds, ori, metadata = synthetic(args.images, root)
        say("  table written in %.1f s: %d rows" % (time.perf_counter() - t, preds.shape[0]))
        cfg = make_cfg(root)
        t = time.perf_counter()
        host = meters.AVAMeter(1, cfg, "test")
        say("  AVAMeter read the annotations in %.1f s" % (time.perf_counter() - t))
        t = time.perf_counter()
        device = meters.DeviceAVAMeter(1, cfg, "test")
        torch.cuda.synchronize()
        say("  DeviceAVAMeter read and uploaded them in %.1f s: %d ground-truth rows" % (time.perf_counter() - t, device.total_gt))
    rows = [torch.from_numpy(a) for a in (preds, ori, metadata)]
    host.update_stats(*rows)
    device.update_stats(*[r.cuda() for r in rows])
    torch.cuda.synchronize()
    device.finalize_metrics(log=False)                                         # warm-up: the library loads, the allocator fills
    ta, tb = [], []
    for r in range(args.rounds):
        t = time.perf_counter()
        a = host.finalize_metrics(log=False)
        ta.append(time.perf_counter() - t)
        torch.cuda.synchronize()
        t = time.perf_counter()
        b = device.finalize_metrics(log=False)
        torch.cuda.synchronize()
        tb.append(time.perf_counter() - t)
        say("    round %d   A %9.3f s   B %9.5f s   mAP host %.17g device %.17g difference %.3g" % (r, ta[-1], tb[-1], a, b, abs(a - b)))
    ma, mb = statistics.median(ta), statistics.median(tb)
    say("1  finalize_metrics: A (host AVAMeter) median %.3f s (min %.3f max %.3f), B (DeviceAVAMeter) median %.5f s (min %.5f "
        "max %.5f), A / B = %.0f" % (ma, min(ta), max(ta), mb, min(tb), max(tb), ma / mb))
    kt = kernel_times(lambda: device.finalize_metrics(log=False), ("ava_match_kernel", "voc_pack_kernel", "voc_rank_kernel", "voc_finish_kernel"))
    K, C = preds.shape
    by = device.bytes
    us, n = kt["ava_match_kernel"]
    say("2  ava_match_kernel: median %.1f us over %d launches; %.3g bytes of the table written and %.3g of boxes read = %.1f %% "
        "of 8 TB/s" % (us, n, K * 60, K * 16, 100 * (K * 60 + K * 16) / (us * 1e-6) / 8e12))
    tp = torch.zeros((-(-K // 64) * 64, C), dtype=torch.bool, device=by.device)
    tp[:K] = by == 2
    us, n = kt["voc_rank_kernel"]
    cmp_ = float(tp.reshape(-1, 64, C).any(dim=1).sum()) * 64 * (-(-K // 256) * 256)
    lanes = 256 * 4 * 16 * 2.4e9                                               # VALU lane-instructions per second
    rate = cmp_ / (us * 1e-6)
    say("   voc_rank_kernel: median %.1f us over %d launches; %.3g comparisons, %.3g per second; the whole VALU issue rate "
        "(%.3g lane-instructions / s) would be %.1f instructions per comparison -- the loop has about four (compare, add, "
        "and, add) plus its share of the LDS reads; %d true positives" % (us, n, cmp_, rate, lanes, lanes / rate,
                                                                         int((by == 2).sum())))
    us, n = kt["voc_pack_kernel"]
    say("   voc_pack_kernel: median %.1f us over %d launches (the class-major copy: 5 bytes written per (row, class))" % (us, n))
    us, n = kt["voc_finish_kernel"]
    say("   voc_finish_kernel: median %.1f us over %d launches (one workgroup per class; the largest class walks its true "
        "positives 256 threads wide)" % (us, n))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
