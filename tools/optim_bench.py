"""The tail of the training step -- gradient clipping, the optimizer update and everything needed until the bf16 weight
copies that exist are fresh again -- on the two parameter sets of the project, fused against the parent sequence:

  fused    optimizer.FusedAdam / FusedSGD .step_clipped(max_norm)            (csrc/optim.hip, two launches)
  parent   clip_grad_norm_(model.parameters()) + torch.optim.Adam / SGD .step() + the ops.invalidate_shadows post-step
           hook: what construct_optimizer_slot / construct_optimizer build with FOCUS_FUSED_OPT=0

Parameter sets: the STEVE model of bench.py:bench_steve_model with `adam` (three groups, set_slot_lr's rates) and the
ORViT-MF model of bench.py:make_cfg with `sgd`.  Both paths step the SAME model (each with an optimizer and a state of its own), so they
read and refresh the same weight copies; one real training step creates those, then the gradients are synthetic (refilled before every call, outside the timed window, so that
every call clips).  Rounds alternate between the paths; every call is timed by HIP events (device time) and by the host
clock from the call to the end of a device synchronise (wall time).  Launches per call come from one profiled call per
path (torch.profiler, outside the timed rounds).  Last, the STEVE `model_step` of bench.py with and without the fused
optimizer, alternated (see model_step).

  python tools/optim_bench.py [--rounds 7] [--calls 20] [--out profiles/optim_family_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def steve_set(dev):
    import torch
    from focus_amd.slowfast.config.defaults import get_cfg
    from focus_amd.slowfast.models import MODEL_REGISTRY
    from focus_amd.slowfast.models.optimizer import construct_optimizer_slot
    from focus_amd.train import slot_train_step
    cfg = get_cfg()
    cfg.MODEL.MODEL_NAME = "STEVE"
    cfg.NUM_GPUS = 1
    cfg.TRAIN.MIXED_PRECISION = True
    cfg.SOLVER.OPTIMIZING_METHOD = "adam"
    cfg.SOLVER.CLIP_GRAD_L2NORM = 0.05
    sl = cfg.SLOTS
    sl.NUM_ITERS, sl.NUM_SLOTS, sl.CNN_HID_SIZE, sl.SIZE, sl.DIM, sl.MLP_HID_SIZE, sl.IMG_SIZE, sl.VOCAB_SIZE = 3, 11, 64, 192, 192, 768, 128, 4096
    sl.NUM_PREDICTOR_BLOCKS, sl.NUM_PREDICTOR_HEADS, sl.PREDICTOR_DROPOUT = 1, 4, 0.0
    sl.DECODER.DIM, sl.DECODER.NUM_BLOCKS, sl.DECODER.NUM_HEADS, sl.DECODER.DROPOUT = 192, 8, 4, 0.1
    torch.manual_seed(0)
    m = MODEL_REGISTRY.get("STEVE")(cfg).to(dev).train()
    opt = _construct(construct_optimizer_slot, m, cfg, True)
    video = torch.rand(1, 4, 3, 128, 128, device=dev)              # the parameter set does not depend on the clip's size
    slot_train_step(m, opt, video, 1000, cfg)                     # past the warm-up start: all three rates are non-zero
    return m, opt, _construct(construct_optimizer_slot, m, cfg, False), cfg.SOLVER.CLIP_GRAD_L2NORM


def orvit_set(dev):
    import torch
    import bench
    from focus_amd.slowfast.models import build_model
    from focus_amd.slowfast.models.losses import get_loss_func
    from focus_amd.slowfast.models.optimizer import construct_optimizer
    from focus_amd.train import synthetic_batch, train_step
    cfg = bench.make_cfg(1, 1)
    cfg.SOLVER.OPTIMIZING_METHOD = "sgd"
    cfg.SOLVER.BASE_LR = 1e-3
    cfg.SOLVER.CLIP_GRAD_L2NORM = 1.0
    torch.manual_seed(0)
    m = build_model(cfg, gpu_id=dev.index)
    m.train()
    opt = _construct(construct_optimizer, m, cfg, True)
    inputs, labels, meta = synthetic_batch(cfg, 1, dev, seed=0)
    train_step(m, opt, get_loss_func(cfg)(reduction="mean"), inputs, labels, meta, cfg)
    return m, opt, _construct(construct_optimizer, m, cfg, False), cfg.SOLVER.CLIP_GRAD_L2NORM


def _construct(fn, model, cfg, fused):
    old = os.environ.get("FOCUS_FUSED_OPT")
    os.environ["FOCUS_FUSED_OPT"] = "1" if fused else "0"
    try:
        opt = fn(model, cfg)
    finally:
        if old is None:
            del os.environ["FOCUS_FUSED_OPT"]
        else:
            os.environ["FOCUS_FUSED_OPT"] = old
    assert hasattr(opt, "step_clipped") == fused, type(opt)
    return opt


class Path:
    def __init__(self, name, model, opt, max_norm):
        import torch
        self.name, self.model, self.opt, self.max_norm = name, model, opt, max_norm
        self.params = [p for p in model.parameters() if p.requires_grad]
        g = torch.Generator(device="cpu").manual_seed(1)
        self.saved = [(torch.randn(p.shape, generator=g) * 1e-2).to(p.device) for p in self.params]    # norm far above max_norm
        self.dev_ms, self.wall_ms = [], []

    def refill(self):
        import torch
        for p in self.params:
            if p.grad is None:
                p.grad = torch.empty_like(p)
        torch._foreach_copy_([p.grad for p in self.params], self.saved)

    def call(self):
        import torch
        if hasattr(self.opt, "step_clipped"):
            self.opt.step_clipped(max_norm=self.max_norm)
        else:
            torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.max_norm)
            self.opt.step()                                         # + the invalidate_shadows post-step hook

    def timed(self, calls, record=True):
        import torch
        for _ in range(calls):
            self.refill()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            self.call()
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if record:
                self.dev_ms.append(e0.elapsed_time(e1))
                self.wall_ms.append(1e3 * (t1 - t0))

    def launches(self):
        """(kernels, copies) of one call, or None where the profiler gives no device events"""
        import torch
        from torch.profiler import ProfilerActivity, profile
        self.refill()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:      # a profiler that fails, fails the run
            self.call()
            torch.cuda.synchronize()
        devs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        if not devs:
            return None
        copies = sum(1 for e in devs if "memcpy" in e.name.lower() or "memset" in e.name.lower() or "copybuffer" in e.name.lower())
        return len(devs) - copies, copies


def model_step(a, dev):
    """The STEVE `model_step` record of `python bench.py --full --workload steve` (bench.bench_steve_model: the whole
    slot_train_step at 24 x 128 x 128, its own warm-up and timed steps), alternated between FOCUS_FUSED_OPT=0 (the parent
    sequence: clip_grad_norm_ + torch.optim.Adam + the shadow hook) and the fused default; the rounds give the spread."""
    import bench
    args = argparse.Namespace(steve_model_batch=a.steve_model_batch, steps=3, steve_model_eval=False)
    ms = {"0": [], "1": []}
    old = os.environ.get("FOCUS_FUSED_OPT")
    try:
        for r in range(a.model_step_rounds):
            for f in (("0", "1") if r % 2 == 0 else ("1", "0")):
                os.environ["FOCUS_FUSED_OPT"] = f
                ms[f].append(bench.bench_steve_model(args, dev)["ms_per_step"])
    finally:
        if old is None:
            os.environ.pop("FOCUS_FUSED_OPT", None)
        else:
            os.environ["FOCUS_FUSED_OPT"] = old
    out = ["STEVE model_step (bench.py:bench_steve_model, batch %d, ms_per_step of its 3 timed steps), %d alternated rounds:" % (
        a.steve_model_batch, a.model_step_rounds)]
    for f, name in (("0", "parent sequence (FOCUS_FUSED_OPT=0)"), ("1", "FusedAdam (default)")):
        out.append("  %-36s min %8.2f  median %8.2f  max %8.2f   rounds: %s" % (
            name, min(ms[f]), statistics.median(ms[f]), max(ms[f]), " ".join("%.2f" % x for x in ms[f])))
    return out


def mmm(xs):
    return "%8.3f %8.3f %8.3f" % (min(xs), statistics.median(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sets", default="steve,orvit")
    ap.add_argument("--model-step-rounds", type=int, default=5, help="0: leave the STEVE model_step comparison out")
    ap.add_argument("--steve-model-batch", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_family_bench.txt"))
    a = ap.parse_args()
    import torch
    from focus_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench: no GPU (there is nothing to measure without one)")
    if a.rounds < 7:
        raise SystemExit("optim_bench: at least seven alternated rounds")
    dev = torch.device("cuda", 0)
    lines = ["optimizer step tail: clip + update + weight copies; %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "%d alternated rounds x %d calls per path; per call: device ms (HIP events) and host wall ms (call .. end of synchronise)" % (
                 a.rounds, a.calls),
             "%-7s %-7s %7s %9s %8s %7s | %26s | %26s" % ("set", "path", "tensors", "elements", "kernels", "copies",
                                                        "device ms  min  median  max", "wall ms  min  median  max")]
    verdict = []
    for name in a.sets.split(","):
        build = {"steve": steve_set, "orvit": orvit_set}[name]
        ops.drop_caches()
        m, fused_opt, parent_opt, max_norm = build(dev)
        if name == "steve":                                         # the rates slot_train_step set on the fused optimizer
            for g, h in zip(parent_opt.param_groups, fused_opt.param_groups):
                g["lr"] = h["lr"]
        paths = [Path("fused", m, fused_opt, max_norm), Path("parent", m, parent_opt, max_norm)]
        for p in paths:
            p.timed(5, record=False)                                # warm-up: code objects, tables, allocator
        for r in range(a.rounds):
            for p in (paths if r % 2 == 0 else paths[::-1]):
                p.timed(a.calls)
        for p in paths:
            n = p.launches()
            lines.append("%-7s %-7s %7d %9d %8s %7s | %s | %s" % (
                name, p.name, len(p.params), sum(q.numel() for q in p.params), "n/a" if n is None else n[0],
                "n/a" if n is None else n[1], mmm(p.dev_ms), mmm(p.wall_ms)))
        fw, pw = statistics.median(paths[0].wall_ms), statistics.median(paths[1].wall_ms)
        verdict.append("%s: median wall per call fused %.3f ms, parent %.3f ms (%.2fx)" % (name, fw, pw, pw / fw))
        del paths, m, fused_opt, parent_opt
        ops.drop_caches()
        torch.cuda.empty_cache()
    lines += verdict
    if a.model_step_rounds:
        lines += model_step(a, dev)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
