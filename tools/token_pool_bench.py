"""Pooling attention, forward + backward: ops.token_pool (csrc/token_pool.hip) against the route it replaces, at every
distinct pooling call of MViT-B 16x4.

  python tools/token_pool_bench.py [--rounds 10] [--inner 10] [--batch 8] [--out profiles/token_pool_bench.txt]

Shapes: the model is constructed on the CPU from the published MViT-B 16x4 settings (depth 16, embed 96, heads 1, dim and head
multipliers x2 at blocks 1, 3, 14, 3x3x3 pooling windows, adaptive kv stride 1x8x8, q stride 1x2x2 at blocks 1, 3, 14, 16 frames
at 224 with a 2x4x4 patch stride) and every block's pool modules are read off it with the grid they see; equal calls are
counted.  Batch 8, bf16 activations, fp32 parameters.
Arm A is ops.token_pool on the [B, N, C] rows.  Arm B is the route of the parent commit restated here: heads split off by a
permute, the cls row cut, permute to NCDHW + contiguous, .float(), F.conv3d / F.max_pool3d, cast back, reshape / transpose, cat
of the cls row, contiguous, ops.layer_norm, permute back to rows + contiguous (what the attention kernels read).
The two arms alternate round by round; a round times `inner` forward + backward calls of one arm between two device events.
Reported per shape: median and spread (max - min) of the rounds of each arm, arm A's rate against the algorithmic bytes of a
forward + backward (forward: x read, y written, the saved pooled rows / statistics / indices written; backward: dy and the saved
tensors read, dx written, x and dpooled read once more for dw), kernel launches of one forward + backward (counted by the
profiler in a pass of its own) and the allocator peak above the live inputs.  Last: one model's worth of calls, every shape
weighted by its count, per round; the verdict compares the medians of those sums with the larger spread.
Needs the GPU: there is no CPU path."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
from focus_amd import ops  # noqa: E402

MVIT_B_16X4 = ["MODEL.MODEL_NAME", "MViT", "MODEL.NUM_CLASSES", 80, "MODEL.DROPOUT_RATE", 0.5, "MODEL.HEAD_ACT", "sigmoid",
               "DATA.NUM_FRAMES", 16, "DATA.SAMPLING_RATE", 4, "DATA.TRAIN_CROP_SIZE", 224, "DATA.TEST_CROP_SIZE", 224,
               "DATA.INPUT_CHANNEL_NUM", [3], "MVIT.ZERO_DECAY_POS_CLS", False, "MVIT.SEP_POS_EMBED", True, "MVIT.DEPTH", 16,
               "MVIT.NUM_HEADS", 1, "MVIT.EMBED_DIM", 96, "MVIT.PATCH_KERNEL", [3, 7, 7], "MVIT.PATCH_STRIDE", [2, 4, 4],
               "MVIT.PATCH_PADDING", [1, 3, 3], "MVIT.MLP_RATIO", 4.0, "MVIT.QKV_BIAS", True, "MVIT.DROPPATH_RATE", 0.4,
               "MVIT.NORM", "layernorm", "MVIT.MODE", "conv", "MVIT.CLS_EMBED_ON", True,
               "MVIT.DIM_MUL", [[1, 2.0], [3, 2.0], [14, 2.0]], "MVIT.HEAD_MUL", [[1, 2.0], [3, 2.0], [14, 2.0]],
               "MVIT.POOL_KVQ_KERNEL", [3, 3, 3], "MVIT.POOL_KV_STRIDE_ADAPTIVE", [1, 8, 8],
               "MVIT.POOL_Q_STRIDE", [[1, 1, 2, 2], [3, 1, 2, 2], [14, 1, 2, 2]], "MVIT.DROPOUT_RATE", 0.0,
               "TRAIN.DATASET", "ava", "TRAIN.MIXED_PRECISION", True, "NUM_GPUS", 1]


def _t3(v):
    return (v, v, v) if isinstance(v, int) else tuple(int(a) for a in v)


def model_calls():
    """-> [(key, count)] with key = (thw, C, heads, mode, kernel, stride, padding, norm): the distinct pooling calls of one
    forward of MViT-B 16x4, in the order they first occur."""
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.models.attention import MultiScaleBlock
    from focus_amd.slowfast.models.build import MODEL_REGISTRY
    import focus_amd.slowfast.models  # noqa: F401  (registers the models)
    cfg = get_cfg()
    cfg.merge_from_list(MVIT_B_16X4)
    model = MODEL_REGISTRY.get("MViT")(cfg)                             # on the CPU: construction needs no GPU
    st = cfg.MVIT.PATCH_STRIDE
    thw = (cfg.DATA.NUM_FRAMES // st[0], cfg.DATA.TRAIN_CROP_SIZE // st[1], cfg.DATA.TRAIN_CROP_SIZE // st[2])
    calls = {}
    for blk in (m for m in model.modules() if isinstance(m, MultiScaleBlock)):
        at = blk.attn
        C, heads = blk.dim, at.num_heads
        for pool, h, norm in ((at.pool_q, heads, True), (at.pool_k, heads, True), (at.pool_v, heads, True), (blk.pool_skip, 1, False)):
            if pool is None:
                continue
            mode = "conv" if isinstance(pool, nn.Conv3d) else "max" if isinstance(pool, nn.MaxPool3d) else "avg"
            key = (thw, C, h, mode, _t3(pool.kernel_size), _t3(pool.stride), _t3(pool.padding), norm and mode == "conv")
            calls[key] = calls.get(key, 0) + 1
        if at.pool_q is not None:
            k, s, p = _t3(at.pool_q.kernel_size), _t3(at.pool_q.stride), _t3(at.pool_q.padding)
            thw = tuple((thw[i] + 2 * p[i] - k[i]) // s[i] + 1 for i in range(3))
    return list(calls.items())


class Call:
    def __init__(self, key, B, dev, seed=0):
        self.thw, self.C, self.heads, self.mode, self.k, self.s, self.p, self.norm = key
        g = torch.Generator().manual_seed(seed)
        self.hd = self.C // self.heads
        N = 1 + self.thw[0] * self.thw[1] * self.thw[2]
        self.out = tuple((self.thw[i] + 2 * self.p[i] - self.k[i]) // self.s[i] + 1 for i in range(3))
        No = 1 + self.out[0] * self.out[1] * self.out[2]
        self.x = torch.randn(B, N, self.C, generator=g).to(dev).bfloat16().requires_grad_(True)
        self.dy = torch.randn(B, No, self.C, generator=g).to(dev).bfloat16()
        self.w = self.ln = None
        if self.mode == "conv":
            self.pool = nn.Conv3d(self.hd, self.hd, self.k, stride=self.s, padding=self.p, groups=self.hd, bias=False).to(dev)
            self.w = self.pool.weight
        else:
            self.pool = nn.MaxPool3d(self.k, self.s, self.p)
        if self.norm:
            self.ln = nn.LayerNorm(self.hd).to(dev)
        self.params = [q for m in (self.pool, self.ln) if m is not None for q in m.parameters()]
        e, n_in, n_out = 2, B * N * self.C, B * No * self.C
        saved = (n_out * e + 2 * 4 * B * No * self.heads) if self.norm else 0            # pooled rows, mean, rstd
        saved += n_out if self.mode == "max" else 0                                      # int8 indices
        fwd = n_in * e + n_out * e + saved
        bwd = n_out * e + saved + n_in * e + ((n_out * e) if self.norm else 0)            # dy, saved, dx; dpooled written
        bwd += (n_in * e + n_out * e) if self.mode == "conv" else 0                     # dw: x and dpooled once more
        self.bytes = fwd + bwd

    def name(self):
        return "%dx%dx%d dim %d (%d x %d) %s k%s s%s%s" % (*self.thw, self.C, self.heads, self.hd, self.mode, "".join(map(str, self.k)),
                                                            "".join(map(str, self.s)), " +LN" if self.norm else "")

    def zero(self):
        self.x.grad = None
        for q in self.params:
            q.grad = None

    def hip(self):
        y, _ = ops.token_pool(self.x, self.thw, self.mode, self.w, self.k, self.s, self.p, True, self.hd, self.ln)
        y.backward(self.dy)
        return y

    def aten(self):
        x = self.x
        B, N, C = x.shape
        t = x.reshape(B, N, self.heads, -1).permute(0, 2, 1, 3)
        cls_tok, t = t[:, :, :1, :], t[:, :, 1:, :]
        t = t.reshape(B * self.heads, *self.thw, self.hd).permute(0, 4, 1, 2, 3).contiguous()
        t = self.pool(t.float()).to(x.dtype)
        L = t.shape[2] * t.shape[3] * t.shape[4]
        t = torch.cat((cls_tok, t.reshape(B, self.heads, self.hd, L).transpose(2, 3)), dim=2)
        if self.ln is not None:
            t = ops.layer_norm(t.contiguous(), self.ln.weight, self.ln.bias, self.ln.eps)
        y = t.permute(0, 2, 1, 3).reshape(B, -1, C).contiguous()
        y.backward(self.dy)
        return y


def timed(c, fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        c.zero()
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner                     # us per forward + backward


def launches(c, fn):
    from torch.profiler import ProfilerActivity, profile
    c.zero()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return len([e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")])


def temp_bytes(c, fn):
    c.zero()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del y
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "token_pool_bench.txt"))
    a = ap.parse_args()

    def save(lines):                                              # after every shape: a later pass cannot lose the timings
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not torch.cuda.is_available():
        raise SystemExit("token_pool_bench: needs the GPU (no CPU path, no timing without one)")
    dev = torch.device("cuda:0")
    calls = model_calls()
    lines = ["Pooling attention of MViT-B 16x4, forward + backward, batch %d, bf16, %s; %d rounds x %d calls per arm, arms "
             "alternating; us per fwd+bwd" % (a.batch, torch.cuda.get_device_name(0), a.rounds, a.inner),
             "A = ops.token_pool (HIP, token layout, LayerNorm fused); B = permute + .float() + ATen conv3d / max_pool3d + cast + "
             "cat + ops.layer_norm + permute back",
             "%d pooling calls per model forward in %d distinct shapes" % (sum(n for _, n in calls), len(calls))]
    sum_a, sum_b = [0.0] * a.rounds, [0.0] * a.rounds
    losers = []
    for key, count in calls:
        c = Call(key, a.batch, dev)
        ya = c.hip().detach().float()
        ga = c.x.grad.float().clone()
        c.zero()
        yb = c.aten().detach().float()
        gb = c.x.grad.float().clone()
        lines.append("%s   x %d per forward" % (c.name(), count))
        lines.append("  agreement  max |y| diff %.3e (|y| max %.2f)   max |dx| diff %.3e (|dx| max %.2f)" % (
            float((ya - yb).abs().max()), float(ya.abs().max()), float((ga - gb).abs().max()), float(ga.abs().max())))
        del ya, yb, ga, gb
        for fn in (c.hip, c.aten):                                 # warm-up of both arms at this shape
            timed(c, fn, 3)
        ta, tb = [], []
        for r in range(a.rounds):
            ta.append(timed(c, c.hip, a.inner))
            tb.append(timed(c, c.aten, a.inner))
            sum_a[r] += count * ta[-1]
            sum_b[r] += count * tb[-1]
        ma, mb = statistics.median(ta), statistics.median(tb)
        for label, t in (("A hip", ta), ("B aten", tb)):
            lines.append("  %-7s median %9.1f us   min %9.1f   max %9.1f   spread %8.1f" % (label, statistics.median(t), min(t), max(t), max(t) - min(t)))
        lines.append("  A: %.1f MB algorithmic per fwd+bwd -> %.0f GB/s;   median ratio B / A %.2f;   A not slower in %d of %d rounds" % (
            c.bytes / 1e6, c.bytes / ma / 1e3, mb / ma, sum(x <= y for x, y in zip(ta, tb)), a.rounds))
        if ma >= mb:
            losers.append(c.name())
        save(lines)
        for label, fn in (("A hip", c.hip), ("B aten", c.aten)):
            try:
                n = launches(c, fn)
                ln = "%d" % n if n else "not measured (the profiler returned no device events)"
            except Exception as ex:                               # the profiler, not the measurement above
                ln = "not measured (%s)" % type(ex).__name__
            lines.append("  %-7s launches per fwd+bwd %s   temporary bytes (allocator peak) %d" % (label, ln, temp_bytes(c, fn)))
        save(lines)
        del c
        torch.cuda.empty_cache()
    ma, mb = statistics.median(sum_a), statistics.median(sum_b)
    sa, sb = max(sum_a) - min(sum_a), max(sum_b) - min(sum_b)
    lines.append("one model's worth of pooling (every shape x its count), per round:")
    lines.append("  A hip   median %9.1f us   spread %8.1f" % (ma, sa))
    lines.append("  B aten  median %9.1f us   spread %8.1f" % (mb, sb))
    lines.append("  summary: A %.2f ms against B %.2f ms per model forward + backward of pooling (B / A %.2f); the gap %.1f us is %s "
                 "the larger spread %.1f us" % (ma / 1e3, mb / 1e3, mb / ma, mb - ma, "above" if mb - ma > max(sa, sb) else "NOT above", max(sa, sb)))
    lines.append("  shapes at which A's median is not below B's: %s" % (", ".join(losers) if losers else "none"))
    save(lines)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
