"""The three update rules of focus_optim_step (include/focus_amd.h) restated in plain torch on the CPU, with norm clipping,
value clipping and the first-use rule of the SGD momentum buffer.  One body, two precisions: dtype=torch.float64 is the
reference restatement; dtype=torch.float32 is its "kernel-order" twin -- every tensor operation is rounded to fp32 in the
order csrc/optim.hip performs it, with 1 - beta and the bias corrections formed in double and rounded once, as the kernel
does.  `mutant` switches in one deliberate mistake (tests/test_optim_ref_cpu.py shows that each is caught).

Also the test case that the CPU and the GPU tests share: shapes, groups, learning rates and gradients of four steps."""
import math

import torch

# full and partial 64x64 tiles in both directions, rows not a multiple of 4 (flat mode), a flat chunk boundary (4096), a
# 1-element tensor, 4-D and 3-D tensors
SHAPES = [(64, 68), (12, 20), (132, 8), (174, 48), (6, 10), (1,), (3,), (4100,), (16, 3, 4, 4), (1, 1, 192)]
GROUPS = [[0, 3, 6, 9], [1, 4, 7], [2, 5, 8]]               # parameter indices of the three groups
LR = [[1e-3, 2e-3, 3e-3, 1e-3], [0.0, 1e-3, 2e-3, 3e-3], [3e-3, 1e-3, 5e-4, 2e-3]]       # [group][step]; one group starts at 0
STEPS = 4
NO_GRAD = (3, 2)          # parameter 3 carries no gradient on step 2
LATE = 1                  # parameter 1 gets its first gradient at step 2 (the third step)


def make_params(seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randn(*s, generator=g) * 0.05 for s in SHAPES]


def make_grads(seed=7):
    """[step][param] -> fp32 tensor or None; step 1 has gradients of scale 1e-4."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for step in range(STEPS):
        gs = [torch.randn(*s, generator=g) * (0.3 if step != 1 else 1e-4) for s in SHAPES]
        if step == NO_GRAD[1]:
            gs[NO_GRAD[0]] = None
        if step < 2:
            gs[LATE] = None
        out.append(gs)
    return out


def group_of(i):
    return next(gi for gi, idx in enumerate(GROUPS) if i in idx)


class Ref:
    """kind: 'adam' | 'adamw' | 'sgd'.  params: fp32 CPU tensors (copied into `dtype`).  state[i] is
    {'step', 'm', 'v'} (Adam) or {'buf'} (SGD, absent until the buffer's first use)."""

    def __init__(self, kind, params, dtype, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, momentum=0.0, dampening=0.0,
                 nesterov=False, mutant=None):
        self.kind, self.dtype, self.mutant = kind, dtype, mutant
        self.p = [p.detach().clone().to(dtype) for p in params]
        self.wd, self.betas, self.eps = weight_decay, betas, eps
        self.mu, self.damp, self.nesterov = momentum, dampening, nesterov
        self.state = [dict() for _ in params]
        self.last_total_norm = None

    def _s(self, x):
        """a scalar of the working precision: formed in double by the caller, rounded once here"""
        return torch.tensor(x, dtype=self.dtype)

    def step(self, grads, lrs, max_norm=0.0, clip_value=0.0):
        """grads: [param] tensor or None; lrs: [group].  Returns the gradients as .grad holds them afterwards."""
        assert not (max_norm > 0 and clip_value > 0)
        dt = self.dtype
        gs = [None if g is None else g.detach().clone().to(dt) for g in grads]
        total = math.sqrt(sum(float(g.double().pow(2).sum()) for g in gs if g is not None))
        self.last_total_norm = total
        coef = self._s(1.0)
        if max_norm > 0:
            coef = torch.clamp(self._s(max_norm) / (self._s(total) + self._s(1e-6)), max=1.0)
        for i, g in enumerate(gs):
            if g is None:
                continue
            if clip_value > 0:
                g = g.clamp(min=-clip_value, max=clip_value)
            g = g * coef
            gs[i] = g
            lr = lrs[group_of(i)]
            if self.kind == "sgd":
                self._sgd(i, g, lr)
            else:
                self._adam(i, g, lr)
        return gs

    def _adam(self, i, g, lr):
        p, st = self.p[i], self.state[i]
        if not st:
            st.update(step=0, m=torch.zeros_like(p), v=torch.zeros_like(p))
        st["step"] += 1
        b1, b2 = self.betas
        bc1, bc2 = 1.0 - b1 ** st["step"], 1.0 - b2 ** st["step"]
        decoupled = (self.kind == "adamw") != (self.mutant == "decoupled_decay")
        if decoupled:
            p = p - self._s(lr) * self._s(self.wd) * p
        elif self.wd:
            g = g + self._s(self.wd) * p
        m = st["m"] + self._s(1.0 - b1) * (g - st["m"])
        v = self._s(b2) * st["v"] + self._s(1.0 - b2) * g * g
        denom = v.sqrt() * self._s(1.0 / math.sqrt(bc2)) + self._s(self.eps)
        p = p - self._s(lr / bc1) * (m / denom)
        self.p[i], st["m"], st["v"] = p, m, v

    def _sgd(self, i, g, lr):
        p, st = self.p[i], self.state[i]
        if self.wd:
            g = g + self._s(self.wd) * p
        if self.mu > 0:
            if "buf" not in st:                                      # first use of THIS buffer, at whatever step
                st["buf"] = g * self._s(1.0 - self.damp) if self.mutant == "dampened_first_use" else g.clone()
            else:
                st["buf"] = self._s(self.mu) * st["buf"] + self._s(1.0 - self.damp) * g
            if self.nesterov and self.mutant != "nesterov_without_lookahead":
                g = g + self._s(self.mu) * st["buf"]
            else:
                g = st["buf"]
        self.p[i] = p - self._s(lr) * g


P_FLOOR, S_FLOOR = 1e-3, 1e-12


def rel(got, want, floor=S_FLOOR):
    """max |got - want| relative to the largest magnitude of `want`, the per-tensor measure of tests/test_gpu_optim.py with its
    floors: P_FLOOR = 1e-3 under a parameter tensor's magnitude (a 1-element parameter that an update carries through zero
    has no magnitude of its own to be relative to: the (1,) tensor of SHAPES passes 2.5e-5 on its way), S_FLOOR = 1e-12 under
    gradients, moments and buffers."""
    d = float((got.double() - want.double()).abs().max())
    return d / max(float(want.double().abs().max()), floor)
