"""Optimizer construction for the Motionformer path (mirror of slowfast/models/optimizer.py:48-172 for
OPTIMIZING_METHOD adamw/adam/sgd: parameters named in model.no_weight_decay() and, with ZERO_WD_1D_PARAM, all 1-D
parameters get zero weight decay) and for the slot loop (optimizer.py:13-40).  With fp32 parameters on the GPU the update
is one of the Fused* classes below (csrc/optim.hip); otherwise it stays torch.optim with a post-step hook."""
import os

import torch


ADAMW, ADAM, SGD = 0, 1, 2          # enum focus_optim_mode (include/focus_amd.h)


class _FusedStep:
    """What FusedAdamW, FusedAdam and FusedSGD share: the device tables of focus_optim_step (items, gradient pointers,
    (lr, weight_decay) per group, per-item step counters, the norm workspace) and `step_clipped`.  A class names its rule
    (`_mode`), checks its groups (`_check_groups`), hands out a parameter's state tensors (`_slots`) and the
    hyper-parameters of the call (`_hyper`)."""
    _mode = ADAMW
    _refusal = RuntimeError      # what a parameter the kernels cannot take raises

    def _fused_init(self):
        self._table = None          # dict: the device tables of the last step (see _prepare)
        self._groups = None         # (values, device tensor)
        self._ws = None
        self.table_builds = 0       # how often _prepare had to rebuild the item table (steady state: never)
        self.last_total_norm = None
        self.write_clipped_grads = True

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._table = None

    def _prepare(self):
        import numpy as np
        from focus_amd import _lib, ops
        name = type(self).__name__
        self._check_groups()
        live = []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is not None:
                    live.append((p, gi))
        if not live:
            return None
        for p, _ in live:                                 # judged before the library is even looked for
            if p.grad.is_sparse or p.dtype != torch.float32 or not p.is_cuda or not self._dense(p):
                raise self._refusal("%s wants dense contiguous fp32 parameters on the GPU" % name)
        L = _lib.lib()
        dev = live[0][0].device
        ident = (tuple(id(p) for p, _ in live), ops.shadow_epoch())
        tab = self._table
        if tab is None or tab["ident"] != ident:
            # parameters, moments, step counters and shadows: these pointers only change when the set of live
            # parameters, the optimizer state (load_state_dict) or the shadow cache (first forward) does
            n = len(live)
            self.table_builds += 1
            slots = [self._slots(p, self.param_groups[gi]) for p, gi in live]
            steps = self._steps([p for p, _ in live], slots, dev)
            rec = np.zeros((n, 8), dtype=np.int64)
            unit, entries = 0, []
            for i, (p, gi) in enumerate(live):
                m, v = slots[i][0], slots[i][1]
                rows, cols = (p.shape[0], p.numel() // p.shape[0]) if p.dim() >= 2 else (1, p.numel())
                tile = int(p.dim() == 2 and rows % 4 == 0 and cols % 4 == 0 and p.data_ptr() % 16 == 0
                           and (m is None or m.data_ptr() % 16 == 0) and (v is None or v.data_ptr() % 16 == 0))
                dst = ops.cached_shadow(p, torch.bfloat16, False) if p.dim() == 2 else None
                dstT = ops.cached_shadow(p, torch.bfloat16, True) if tile else None
                rec[i, 0] = p.data_ptr()
                rec[i, 1] = m.data_ptr() if m is not None else 0
                rec[i, 2] = v.data_ptr() if v is not None else 0
                rec[i, 3] = dst.data_ptr() if dst is not None else 0
                rec[i, 4] = dstT.data_ptr() if dstT is not None else 0
                rec[i, 5] = int(rows) | (int(cols) << 32)
                rec[i, 6] = int(gi) | (int(unit) << 32)
                rec[i, 7] = tile
                entries.append((p, dst, dstT))
                unit += L.focus_adamw_units(int(rows), int(cols), tile)
            tab = self._table = {"ident": ident, "items": torch.from_numpy(rec).pin_memory().to(dev, non_blocking=True),
                                 "units": unit, "steps": steps, "entries": entries, "tile": rec[:, 7].copy(),
                                 "gsig": None, "gptrs": None}
        grads = []
        for i, (p, _) in enumerate(live):
            g = p.grad
            if not p.is_contiguous():
                # a channels-last convolution weight: the update is element-wise over the storage, so the gradient (and
                # the moments, see _like) only have to lie in memory as the parameter does
                if g.dtype != torch.float32 or g.stride() != p.stride():
                    p.grad = g = torch.empty_like(p).copy_(g)
            elif g.dtype != torch.float32 or not g.is_contiguous() or (tab["tile"][i] and g.data_ptr() % 16):
                p.grad = g = g.float().contiguous().clone() if tab["tile"][i] and g.data_ptr() % 16 else g.float().contiguous()
            grads.append(g.data_ptr())
        gsig = tuple(grads)
        if tab["gsig"] != gsig:
            tab["gsig"] = gsig
            tab["gptrs"] = torch.tensor(grads, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        vals = tuple((float(g["lr"]), float(g["weight_decay"])) for g in self.param_groups)
        if self._groups is None or self._groups[0] != vals or self._groups[1].device != dev:
            self._groups = (vals, torch.tensor(vals, dtype=torch.float32).reshape(-1, 2).pin_memory().to(dev, non_blocking=True))
        if self._ws is None or self._ws.device != dev:
            self._ws = torch.empty(L.focus_adamw_workspace_bytes() // 4 + 1, dtype=torch.float32, device=dev)
        return dev

    _channels_last = False       # FusedAdam / FusedSGD also take 4-D parameters that are dense in channels-last order

    def _dense(self, p):
        return p.is_contiguous() or (self._channels_last and p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last))

    def _like(self, p, t):
        """the state tensor `t` as fp32 on p's device and laid out in memory as `p` is (one that came from elsewhere, e.g. a
        checkpoint, may not be).  FusedAdamW takes its state as it always has."""
        if not self._channels_last:
            return t
        same = t.is_contiguous() if p.is_contiguous() else t.stride() == p.stride()
        if same and t.dtype == torch.float32 and t.device == p.device:
            return t
        return torch.empty_like(p).copy_(t)

    def _adam_slots(self, p, group):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        else:
            st["exp_avg"], st["exp_avg_sq"] = self._like(p, st["exp_avg"]), self._like(p, st["exp_avg_sq"])
        return st["exp_avg"], st["exp_avg_sq"]

    def _adam_steps(self, params, slots, dev):
        steps = torch.stack([self.state[p]["step"].to(dev, torch.float32).reshape(()) for p in params])
        for i, p in enumerate(params):
            self.state[p]["step"] = steps[i]              # 0-dim view: state_dict() still sees one tensor per param
        return steps

    def _adam_hyper(self, name):
        b1, b2 = self.param_groups[0]["betas"]
        eps = self.param_groups[0]["eps"]
        for g in self.param_groups[1:]:
            if tuple(g["betas"]) != (b1, b2) or g["eps"] != eps:
                raise NotImplementedError("%s: one (betas, eps) for all groups" % name)
        return {"beta1": float(b1), "beta2": float(b2), "eps": float(eps)}

    @torch.no_grad()
    def _step(self, max_norm, clip_value, closure):
        import ctypes
        from focus_amd import _lib, ops
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        max_norm, clip_value = float(max_norm or 0.0), float(clip_value or 0.0)
        if max_norm > 0.0 and clip_value > 0.0:
            raise ValueError("%s: max_norm and clip_value exclude each other (the training loops' if / elif)" % type(self).__name__)
        dev = self._prepare()
        if dev is None:
            return loss
        tab = self._table
        hy = self._hyper()
        L = _lib.lib()
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        norm = self._ws[-1:]
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        with torch.cuda.device(dev):
            if self._mode == ADAMW and clip_value == 0.0:
                _lib.check(L.focus_adamw_step(vp(tab["items"]), vp(tab["gptrs"]), len(tab["entries"]), tab["units"],
                                              vp(self._groups[1]), vp(tab["steps"]), vp(self._ws), (self._ws.numel() - 1) * 4,
                                              vp(norm), hy["beta1"], hy["beta2"], hy["eps"], max_norm,
                                              int(self.write_clipped_grads), stream), "adamw_step")
            else:
                h = _lib.OptimHyper(max_norm=max_norm, clip_value=clip_value,
                                    write_clipped_grads=int(self.write_clipped_grads), **hy)
                _lib.check(L.focus_optim_step(self._mode, vp(tab["items"]), vp(tab["gptrs"]), len(tab["entries"]), tab["units"],
                                              vp(self._groups[1]), vp(tab["steps"]), vp(self._ws), (self._ws.numel() - 1) * 4,
                                              vp(norm), ctypes.byref(h), stream), "optim_step")
        self.last_total_norm = norm[0]
        ops.shadows_written(tab["entries"])
        return loss

    def step_clipped(self, max_norm=0.0, clip_value=0.0, closure=None):
        return self._step(max_norm, clip_value, closure)

    def step(self, closure=None):
        return self._step(0.0, 0.0, closure)


class FusedAdamW(_FusedStep, torch.optim.AdamW):
    """torch.optim.AdamW (same param_groups / state_dict layout: state['step'], ['exp_avg'], ['exp_avg_sq']) whose step
    is focus_adamw_step: gradient-norm clipping (train_net.py:112-117), the AdamW update and the bf16 weight shadows of
    focus_amd.ops in two launches over all parameters.  `step_clipped(max_norm)` is what focus_amd.train.train_step calls
    in place of clip_grad_norm_ + step(); plain `step()` is the same without clipping.  `last_total_norm` is the device
    scalar clip_grad_norm_ would have returned."""
    _mode = ADAMW

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, fused=False, foreach=False)
        self._fused_init()

    def _check_groups(self):
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise NotImplementedError("FusedAdamW: amsgrad / maximize are not built")

    _slots = _FusedStep._adam_slots
    _steps = _FusedStep._adam_steps

    def _hyper(self):
        return self._adam_hyper("FusedAdamW")

    def step_clipped(self, max_norm=0.0, closure=None):
        return self._step(max_norm, 0.0, closure)


class FusedAdam(_FusedStep, torch.optim.Adam):
    """torch.optim.Adam (coupled weight decay; the same param_groups / state_dict layout, so checkpoints move between the
    two classes) whose step is focus_optim_step in mode ADAM: `step_clipped(max_norm=, clip_value=)` does clip_grad_norm_
    or clip_grad_value_ (steve_train_net.py:116-123), the update and the bf16 weight shadows in two launches over all
    parameters; `step()` is the same without clipping.  Per-group lr and weight_decay are read at every step."""
    _mode = ADAM
    _refusal = NotImplementedError
    _channels_last = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 capturable=False, differentiable=False, decoupled_weight_decay=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                         capturable=capturable, differentiable=differentiable, decoupled_weight_decay=decoupled_weight_decay,
                         fused=False, foreach=False)
        self._fused_init()
        self._check_groups()

    def _check_groups(self):
        for group in self.param_groups:
            for k in ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay"):
                if group.get(k):
                    raise NotImplementedError("FusedAdam: %s is not built" % k)
        self._adam_hyper("FusedAdam")

    _slots = _FusedStep._adam_slots
    _steps = _FusedStep._adam_steps

    def _hyper(self):
        return self._adam_hyper("FusedAdam")


class FusedSGD(_FusedStep, torch.optim.SGD):
    """torch.optim.SGD (momentum, dampening, nesterov, coupled weight decay; state['momentum_buffer'] as torch keeps it,
    no state at all with momentum 0) whose step is focus_optim_step in mode SGD, with `step_clipped` as in FusedAdam.
    A momentum buffer takes the gradient as it is on its first use, whenever that is: a parameter whose first gradient
    arrives late starts its buffer then, and a buffer that load_state_dict brought is not new."""
    _mode = SGD
    _refusal = NotImplementedError
    _channels_last = True

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 differentiable=False):
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                         maximize=maximize, differentiable=differentiable, fused=False, foreach=False)
        self._fused_init()
        self._check_groups()

    def _sgd_rule(self):
        g0 = self.param_groups[0]
        rule = (float(g0["momentum"]), float(g0["dampening"]), bool(g0["nesterov"]))
        for g in self.param_groups[1:]:
            if (float(g["momentum"]), float(g["dampening"]), bool(g["nesterov"])) != rule:
                raise NotImplementedError("FusedSGD: one (momentum, dampening, nesterov) for all groups")
        return rule

    def _check_groups(self):
        for group in self.param_groups:
            for k in ("maximize", "differentiable"):
                if group.get(k):
                    raise NotImplementedError("FusedSGD: %s is not built" % k)
        mu, damp, nesterov = self._sgd_rule()
        if mu < 0.0 or (nesterov and (mu <= 0.0 or damp != 0.0)):
            raise ValueError("FusedSGD: nesterov needs a momentum and zero dampening; momentum >= 0")

    def _slots(self, p, group):
        """(momentum buffer or None, None, the buffer existed before this step)"""
        if float(group["momentum"]) == 0.0:
            return None, None, False
        st = self.state[p]
        buf = st.get("momentum_buffer")
        had = buf is not None
        if had:
            buf = st["momentum_buffer"] = self._like(p, buf)
        if not had:
            buf = st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return buf, None, had

    def _steps(self, params, slots, dev):
        # uses of each buffer so far: the kernel counts this step's use and treats the one that reaches 1 as the first
        return torch.tensor([1.0 if had else 0.0 for _, _, had in slots], dtype=torch.float32).pin_memory().to(dev, non_blocking=True)

    def _hyper(self):
        mu, damp, nesterov = self._sgd_rule()
        return {"momentum": mu, "dampening": damp, "nesterov": int(nesterov)}


def covers_model(model, optimizer):
    """True if every parameter of `model` that can carry a gradient sits in one of `optimizer`'s groups: only then does
    step_clipped measure the gradient norm clip_grad_norm_(model.parameters()) measures.  Judged once per (model,
    optimizer) pair and again whenever the number of trainable parameters or of held parameters changes (a parameter
    unfrozen later, add_param_group); swapping one parameter for another at equal counts is not noticed."""
    import weakref
    trainable = [p for p in model.parameters() if p.requires_grad]
    key = (len(trainable), sum(len(g["params"]) for g in optimizer.param_groups))
    hit = getattr(optimizer, "_covers", None)
    if hit is not None and hit[0]() is model and hit[1] == key:
        return hit[2]
    held = {id(p) for g in optimizer.param_groups for p in g["params"]}
    ok = all(id(p) in held for p in trainable)
    optimizer._covers = (weakref.ref(model), key, ok)
    return ok


def fused_route(model, optimizer):
    """FusedAdam / FusedSGD take clipping into their step when they hold all of the model's trainable parameters."""
    return isinstance(optimizer, (FusedAdam, FusedSGD)) and covers_model(model, optimizer)


def _fusable(params):
    return bool(params) and all(p.is_cuda and p.dtype == torch.float32 for p in params) and \
        os.environ.get("FOCUS_FUSED_OPT", "1") != "0"


def construct_optimizer(model, cfg):
    skip = set()
    base = model.module if hasattr(model, "module") else model
    if hasattr(base, "no_weight_decay"):
        skip = base.no_weight_decay()
    decay, no_decay = [], []
    for name, p in base.named_parameters():
        if not p.requires_grad:
            continue
        if name in skip or (cfg.SOLVER.ZERO_WD_1D_PARAM and p.dim() == 1):
            no_decay.append(p)
        else:
            decay.append(p)
    groups = [{"params": decay, "weight_decay": cfg.SOLVER.WEIGHT_DECAY},
              {"params": no_decay, "weight_decay": 0.0}]
    assert len(decay) + len(no_decay) == len([p for p in base.parameters() if p.requires_grad])
    method = cfg.SOLVER.OPTIMIZING_METHOD
    if method == "adamw":
        on_gpu = all(p.is_cuda and p.dtype == torch.float32 for p in decay + no_decay)
        if on_gpu and os.environ.get("FOCUS_FUSED_OPT", "1") != "0":
            # clip + AdamW + bf16 shadows in two launches (csrc/optim.hip); no post-step hook: the step writes the shadows
            return FusedAdamW(groups, lr=cfg.SOLVER.BASE_LR, eps=1e-08)
        opt = torch.optim.AdamW(groups, lr=cfg.SOLVER.BASE_LR, eps=1e-08, fused=on_gpu)
    elif method == "sgd":
        if _fusable(decay + no_decay):
            return FusedSGD(groups, lr=cfg.SOLVER.BASE_LR, momentum=cfg.SOLVER.MOMENTUM, dampening=cfg.SOLVER.DAMPENING,
                            nesterov=cfg.SOLVER.NESTEROV)
        opt = torch.optim.SGD(groups, lr=cfg.SOLVER.BASE_LR, momentum=cfg.SOLVER.MOMENTUM,
                              dampening=cfg.SOLVER.DAMPENING, nesterov=cfg.SOLVER.NESTEROV)
    elif method == "adam":
        # optimizer.py:155-161: L2 (coupled) weight decay
        if _fusable(decay + no_decay):
            return FusedAdam(groups, lr=cfg.SOLVER.BASE_LR, betas=(0.9, 0.999), weight_decay=cfg.SOLVER.WEIGHT_DECAY)
        opt = torch.optim.Adam(groups, lr=cfg.SOLVER.BASE_LR, betas=(0.9, 0.999), weight_decay=cfg.SOLVER.WEIGHT_DECAY)
    else:
        raise NotImplementedError("Does not support {} optimizer".format(method))
    # fused optimizers do not bump Tensor._version: tell the bf16 weight shadows that the masters moved
    from focus_amd import ops
    opt.register_step_post_hook(lambda *_a, **_k: ops.invalidate_shadows())
    return opt


def construct_optimizer_slot(model, cfg):
    """optimizer.py:13-40: three parameter groups -- dVAE, encoder, decoder -- whose learning rates set_slot_lr rewrites
    every step.  With fp32 parameters on the GPU the classes are FusedSGD / FusedAdam (clip + update + bf16 shadows in two
    launches, no post-step hook); FOCUS_FUSED_OPT=0 keeps torch's."""
    base = model.module if hasattr(model, "module") else model
    named = list(base.named_parameters())
    optim_params = [
        {"params": [p for n, p in named if "dvae" in n], "lr": cfg.SLOTS_OPTIM.DVAE},
        {"params": [p for n, p in named if "steve_encoder" in n], "lr": 0.0},
        {"params": [p for n, p in named if "steve_decoder" in n], "lr": 0.0},
    ]
    # (the decoder keeps its boolean masks as frozen parameters: what can never carry a gradient never reaches the step)
    fusable = _fusable([p for g in optim_params for p in g["params"] if p.requires_grad])
    method = cfg.SOLVER.OPTIMIZING_METHOD
    if method == "sgd":
        kw = dict(lr=cfg.SOLVER.BASE_LR, momentum=cfg.SOLVER.MOMENTUM, weight_decay=cfg.SOLVER.WEIGHT_DECAY,
                  dampening=cfg.SOLVER.DAMPENING, nesterov=cfg.SOLVER.NESTEROV)
        if fusable:
            return FusedSGD(optim_params, **kw)
        opt = torch.optim.SGD(optim_params, **kw)
    elif method == "adam":
        if fusable:
            return FusedAdam(optim_params)
        opt = torch.optim.Adam(optim_params)
    else:
        raise NotImplementedError("Does not support {} optimizer".format(method))
    from focus_amd import ops
    opt.register_step_post_hook(lambda *_a, **_k: ops.invalidate_shadows())
    return opt


def set_slot_lr(optimizer, cfg, lr_decay_factor, lr_warmup_factor_enc, lr_warmup_factor_dec):
    """optimizer.py:213-222."""
    optimizer.param_groups[0]["lr"] = cfg.SLOTS_OPTIM.DVAE
    optimizer.param_groups[1]["lr"] = lr_decay_factor * lr_warmup_factor_enc * cfg.SLOTS_OPTIM.ENC
    optimizer.param_groups[2]["lr"] = lr_decay_factor * lr_warmup_factor_dec * cfg.SLOTS_OPTIM.DEC
