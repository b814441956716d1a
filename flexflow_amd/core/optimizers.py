"""SGD and Adam (reference include/flexflow/optimizer.h:15-120, src/runtime/optimizer.cc:23-610,
optimizer_kernel.cu).

The reference launches one update task per weight (with a NCCL all-reduce inside each). Here
every weight shard of a replica group lives in one flat fp32 arena, so an update is ONE fused HIP
kernel per arena (multi-tensor apply) that also refreshes the bf16 compute copy. AdamW and LAMB
(not in the reference) decay each weight by its own lambda: their kernels walk a chunk table of the
arena (kernels.lamb_table), AdamW in one pass per update range, LAMB in two with the norms between.

The runtime reads what an optimizer needs from what Optimizer declares, each with a default: ranged
(step_range is implemented: the overlapped and the sharded update), two_phase (LAMB), chunk_table
(AdamW: set_table), capturable (a captured whole step may hold the update, after use_device_alpha)
and state_tensors(arena). AdamW and LAMB share _MomentOptimizer.
"""
from __future__ import annotations

import bisect
import math

import torch

from .. import kernels as K


def _resolve_clip_norm(ffmodel, clip_norm):
    """clip_norm=None takes the model's --clip-grad-norm (0 = off); returns None when off."""
    if clip_norm is None:
        clip_norm = getattr(getattr(ffmodel, "config", None), "clip_grad_norm", 0.0)
    c = float(clip_norm)
    if not math.isfinite(c) or c < 0:
        raise ValueError(f"clip_norm must be a finite value >= 0 (0 or None = off), got {clip_norm!r}")
    return c or None


class Optimizer:
    # what the runtime (Executor, runtime/graph.py) asks; the defaults suit one that implements step() alone
    two_phase = False     # the update is moments() / apply() with the norms' all-reduce between
    chunk_table = False   # step_range runs over a chunk table the executor hands to set_table()
    capturable = False    # a captured whole-step hipGraph may hold the update

    def __init__(self, ffmodel=None, lr=0.01, clip_norm=None):
        self.lr = lr
        self.ffmodel = ffmodel
        self.state = {}
        # gradient clipping by global L2 norm (torch's clip_grad_norm_ over all trainable weights,
        # world-wide): the executor leaves coef = min(1, clip_norm / (norm + 1e-6)) in
        # clip_coef_dev before the step* calls of an update, which hand it to the kernels
        self.clip_norm = _resolve_clip_norm(ffmodel, clip_norm)
        self.clip_coef_dev = None

    def _gscale_dev(self):
        return self.clip_coef_dev if self.clip_norm else None

    def set_learning_rate(self, learning_rate):
        self.lr = learning_rate

    def init_state(self, arena):
        pass

    def state_tensors(self, arena) -> tuple:
        """The arena's state tensors, in checkpoint order (SGD: the momentum; the others: m, v)."""
        st = self.state.get(id(arena))
        return () if st is None else tuple(st) if isinstance(st, (tuple, list)) else (st,)

    def use_device_alpha(self, device):
        """Called before a whole step is captured: put what changes per step on the device."""

    def next(self):
        pass

    def step(self, arena):
        raise NotImplementedError

    def step_range(self, arena, lo, hi, max_blocks=0):
        """Update elements [lo, hi) of the arena only (sharded optimizer: this rank's chunk; the
        overlapped update: one gradient bucket, launched with at most max_blocks workgroups)."""
        raise NotImplementedError

    @property
    def ranged(self) -> bool:  # step_range is implemented (with or without max_blocks)
        return type(self).step_range is not Optimizer.step_range


class SGDOptimizer(Optimizer):
    def __init__(self, ffmodel=None, lr=0.01, momentum=0.0, nesterov=False, weight_decay=0.0, clip_norm=None):
        super().__init__(ffmodel, lr, clip_norm)
        self.momentum = momentum
        self.nesterov = nesterov
        self.weight_decay = weight_decay

    def init_state(self, arena):
        if self.momentum > 0:
            self.state[id(arena)] = torch.zeros_like(arena.master)

    def step(self, arena):
        K.sgd_update(arena.master, arena.grad, self.state.get(id(arena)), arena.lowp, self.lr, self.momentum,
                     self.nesterov, self.weight_decay, gscale_dev=self._gscale_dev())

    def step_range(self, arena, lo, hi, max_blocks=0):
        mom = self.state.get(id(arena))
        K.sgd_update(arena.master[lo:hi], arena.grad[lo:hi], mom[lo:hi] if mom is not None else None,
                     arena.lowp[lo:hi] if arena.lowp is not None else None, self.lr, self.momentum, self.nesterov,
                     self.weight_decay, max_blocks=max_blocks, gscale_dev=self._gscale_dev())


class AdamOptimizer(Optimizer):
    capturable = True

    def __init__(self, ffmodel=None, alpha=0.001, beta1=0.9, beta2=0.999, weight_decay=0.0, epsilon=1e-8,
                 clip_norm=None):
        super().__init__(ffmodel, alpha, clip_norm)
        self.alpha = alpha
        self.beta1, self.beta2 = beta1, beta2
        self.weight_decay = weight_decay
        self.epsilon = epsilon
        self.beta1_t = 1.0
        self.beta2_t = 1.0
        self.alpha_t = alpha
        # device copy of alpha_t, set up by a captured whole-step hipGraph (runtime/graph.py): the
        # replayed Adam launches read the step size from it, next() refreshes it before each step
        self.alpha_dev = None

    def use_device_alpha(self, device):
        if self.alpha_dev is None:
            self.alpha_dev = torch.full((1,), float(self.alpha_t), device=device, dtype=torch.float32)

    def set_learning_rate(self, learning_rate):
        self.alpha = learning_rate
        self.lr = learning_rate

    def init_state(self, arena):
        self.state[id(arena)] = (torch.zeros_like(arena.master), torch.zeros_like(arena.master))

    def next(self):
        # reference optimizer.cc:371-376
        self.beta1_t *= self.beta1
        self.beta2_t *= self.beta2
        self.alpha_t = self.alpha * math.sqrt(1 - self.beta2_t) / (1 - self.beta1_t)
        if self.alpha_dev is not None:
            self.alpha_dev.fill_(self.alpha_t)

    def step(self, arena):
        m, v = self.state[id(arena)]
        K.adam_update(arena.master, arena.grad, m, v, arena.lowp, self.alpha_t, self.beta1, self.beta2,
                      self.weight_decay, self.epsilon, alpha_dev=self.alpha_dev, gscale_dev=self._gscale_dev())

    def step_range(self, arena, lo, hi, max_blocks=0):
        m, v = self.state[id(arena)]
        K.adam_update(arena.master[lo:hi], arena.grad[lo:hi], m[lo:hi], v[lo:hi],
                      arena.lowp[lo:hi] if arena.lowp is not None else None, self.alpha_t, self.beta1, self.beta2,
                      self.weight_decay, self.epsilon, max_blocks=max_blocks, alpha_dev=self.alpha_dev,
                      gscale_dev=self._gscale_dev())


def _check_hyper(cls, **kw):
    """ValueError naming the first hyper-parameter that is not a finite number in its range."""
    rules = {"lr": lambda x: x >= 0, "beta1": lambda x: 0 <= x < 1, "beta2": lambda x: 0 <= x < 1,
             "weight_decay": lambda x: x >= 0, "epsilon": lambda x: x > 0}
    for name, val in kw.items():
        try:
            good = not isinstance(val, (bool, str)) and math.isfinite(float(val)) and rules[name](float(val))
        except (TypeError, ValueError):
            good = False
        if not good:
            raise ValueError(f"{cls}: invalid {name}={val!r}")


class _MomentOptimizer(Optimizer):
    """What AdamW and LAMB share: checked hyper-parameters, Adam moments (m, v) per arena, and
    hyper_dev on the device, refreshed by next() and set_learning_rate(), so a captured whole-step
    hipGraph replays the same launches. bias_correction=False keeps both corrections at 1."""

    capturable = True

    def __init__(self, ffmodel, lr, beta1, beta2, weight_decay, epsilon, exclude_1d, clip_norm, bias_correction=True):
        _check_hyper(type(self).__name__, lr=lr, beta1=beta1, beta2=beta2, weight_decay=weight_decay, epsilon=epsilon)
        super().__init__(ffmodel, float(lr), clip_norm)
        self.beta1, self.beta2 = float(beta1), float(beta2)
        self.weight_decay, self.epsilon = float(weight_decay), float(epsilon)
        self.bias_correction, self.exclude_1d = bool(bias_correction), bool(exclude_1d)
        self.beta1_t = self.beta2_t = 1.0
        self.hyper_dev = None  # fp32 [3] on the arenas' device: lr, 1 / (1 - beta1^t), 1 / (1 - beta2^t)

    def _hyper(self):
        if not self.bias_correction or self.beta1_t == 1.0:  # before the first next(): no correction yet
            return self.lr, 1.0, 1.0
        return self.lr, 1.0 / (1.0 - self.beta1_t), 1.0 / (1.0 - self.beta2_t)

    def _refresh(self):
        if self.hyper_dev is not None:
            for i, x in enumerate(self._hyper()):
                self.hyper_dev[i].fill_(x)

    def use_device_alpha(self, device):  # always on: the kernels read hyper_dev
        if self.hyper_dev is None:
            self.hyper_dev = torch.zeros(3, device=device, dtype=torch.float32)
            self._refresh()

    def set_learning_rate(self, learning_rate):
        self.lr = float(learning_rate)
        self._refresh()

    def init_state(self, arena):
        self.state[id(arena)] = (torch.zeros_like(arena.master), torch.zeros_like(arena.master))
        self.use_device_alpha(arena.master.device)

    def next(self):
        self.beta1_t *= self.beta1
        self.beta2_t *= self.beta2
        self._refresh()


class _ChunkPlan:
    """AdamW's chunk tables of one arena: the table entries, the sorted cut points, the tables built
    so far as (table, chunk starts, chunk ends) — never freed: captured graphs hold their pointers —
    and the cache {(lo, hi): (table, c0, c1)} of resolved ranges."""

    def __init__(self, arena, entries, cuts, tables):
        self.size, self.device = arena.master.numel(), arena.master.device
        self.entries, self.tables, self.cache = list(entries), tables, {}
        self.cuts = sorted(set(int(c) for c in cuts))
        self.build()

    def build(self):  # one more table, cut at every cut point
        pts = sorted({0, self.size, *(c for c in self.cuts if 0 < c < self.size)})
        tab = K.lamb_table(self.entries, list(zip(pts[:-1], pts[1:])), len(self.entries), self.size, self.device)
        self.tables.append((tab, [int(s) for s in tab.chunks_host[:, 0]], [s + ln for s, ln, _ in tab.rows()]))

    def resolve(self, lo, hi):
        """(table, c0, c1): the run of whole chunks that is [lo, hi), on the newest table."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo <= hi <= self.size:
            raise RuntimeError(f"AdamWOptimizer.step_range: [{lo}, {hi}) is outside the arena")
        if (lo, hi) in self.cache:
            return self.cache[(lo, hi)]
        for _ in range(2):
            tab, starts, ends = self.tables[-1]
            c0, c1 = bisect.bisect_left(starts, lo), bisect.bisect_left(starts, hi)
            # a bound is a cut when no chunk lies across it (the end of an entry is one, whatever its size)
            across = [b for b, c in ((lo, c0), (hi, c1)) if c > 0 and ends[c - 1] > b]
            if not across:
                self.cache[(lo, hi)] = (tab, c0, c1)
                return self.cache[(lo, hi)]
            if any(b % 4 for b in across):
                raise RuntimeError(f"AdamWOptimizer.step_range: [{lo}, {hi}) cuts a weight at an element that is "
                                   "not a multiple of 4")
            self.cuts = sorted(set(self.cuts) | set(across))  # a new range: one more table, built once
            self.build()
        raise RuntimeError(f"AdamWOptimizer.step_range: no chunk run for [{lo}, {hi})")


class AdamWOptimizer(_MomentOptimizer):
    """AdamW (Loshchilov & Hutter, "Decoupled Weight Decay Regularization", ICLR 2019), which is
    torch.optim.AdamW with amsgrad=False: Adam moments of the (clipped) gradient alone, bias
    correction inside epsilon, and the decay lambda_p * w added to the update, not to the gradient.
    With exclude_1d, weights of one dimension or fewer (biases, LayerNorm / RMSNorm vectors) get
    lambda_p = 0, the rule LAMBOptimizer uses; exclude_1d=False decays everything, as torch does
    over one parameter group.

    One HIP pass per update range (kernels.adamw_update) over a chunk table of the arena
    (kernels.lamb_table) that the executor hands over at init_optimizer (set_table): a range
    [lo, hi) is a run of consecutive chunks, found on the host and cached. The hyper-parameters live
    on the device (_MomentOptimizer). State is (m, v) per arena, as Adam's."""

    chunk_table = True

    def __init__(self, ffmodel=None, lr=1e-3, beta1=0.9, beta2=0.999, weight_decay=0.01, epsilon=1e-8,
                 exclude_1d=True, clip_norm=None):
        super().__init__(ffmodel, lr, beta1, beta2, weight_decay, epsilon, exclude_1d, clip_norm)
        self._plans = {}  # id(arena) -> _ChunkPlan

    def weight_rule(self, shape):
        """lambda_p of a weight of this (shard) shape."""
        return 0.0 if self.exclude_1d and len(shape) <= 1 else self.weight_decay

    def set_table(self, arena, entries, cuts):
        """entries: [(offset, numel, weight, lambda, False)] of the arena (kernels.lamb_table);
        cuts: every bound (a multiple of 4) of a range step_range will be given. Builds the arena's
        table; a table built earlier stays alive."""
        old = self._plans.get(id(arena))
        self._plans[id(arena)] = _ChunkPlan(arena, entries, cuts, old.tables if old else [])

    def step(self, arena):
        self.step_range(arena, 0, arena.master.numel() if arena is not None else 0)

    def step_range(self, arena, lo, hi, max_blocks=0):
        plan = self._plans.get(id(arena))
        if plan is None:
            raise RuntimeError("AdamWOptimizer updates through a chunk table of the arena that "
                               "Executor.init_optimizer() builds (FFModel.compile())")
        tab, c0, c1 = plan.resolve(lo, hi)
        m, v = self.state[id(arena)]
        K.adamw_update(arena.master, arena.grad, m, v, arena.lowp, tab, c0, c1, self.hyper_dev, self._gscale_dev(),
                       self.beta1, self.beta2, self.epsilon, max_blocks=max_blocks)


class LAMBOptimizer(_MomentOptimizer):
    """LAMB (You et al., "Large Batch Optimization for Deep Learning", ICLR 2020): Adam moments,
    decoupled weight decay and a trust ratio |w| / |update| per logical weight, taken over the
    whole weight on every rank. With exclude_1d, weights of one dimension or fewer (biases,
    LayerNorm gamma / beta) get no decay and no ratio: plain bias-corrected Adam.

    An update is two passes with the norms in between (Executor._lamb_update): moments(),
    the per-weight norms and their all-reduce, then apply(). The hyper-parameters live on the
    device (_MomentOptimizer). State is (m, v) per arena, as Adam's."""

    two_phase = True

    def __init__(self, ffmodel=None, lr=1e-3, beta1=0.9, beta2=0.999, weight_decay=0.01, epsilon=1e-6,
                 bias_correction=True, exclude_1d=True, clip_norm=None):
        super().__init__(ffmodel, lr, beta1, beta2, weight_decay, epsilon, exclude_1d, clip_norm, bias_correction)

    def weight_rule(self, shape):
        """(lambda_p, adapt_p) of a weight of this (shard) shape."""
        if self.exclude_1d and len(shape) <= 1:
            return 0.0, False
        return self.weight_decay, True

    def moments(self, arena, table, partials):
        m, v = self.state[id(arena)]
        K.lamb_moments(arena.master, arena.grad, m, v, table, self.hyper_dev, self._gscale_dev(), self.beta1,
                       self.beta2, self.epsilon, partials)

    def apply(self, arena, table, norms):
        m, v = self.state[id(arena)]
        K.lamb_apply(arena.master, m, v, arena.lowp, table, self.hyper_dev, self.epsilon, norms)

    def step(self, arena):
        raise RuntimeError("LAMBOptimizer updates in two passes (moments / apply) through Executor.update()")
