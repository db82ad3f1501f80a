"""The fused optimizer step (csrc/optim.hip, optim.py) as numpy float32: an IEEE-754 restatement of the kernel's own
contract, op for op.  Shared by tests/test_optim_oracle_host.py and tests/test_gpu_optim_elementwise.py (test
infrastructure; numpy only, no GPU and no torch here).

The contract is the header comment of optim.hip: per element the reference's torch calls in their order, every op
rounded ONCE, add(a, b, alpha) = fma(alpha, b, a), addcmul(a, b, c, s) = fma(s*b, c, a), addcdiv(a, b, c, s) =
a + (s*b)/c, no contraction beyond that, and an element's result depends on that element alone.  Every op below is
therefore one numpy float32 op (numpy's + - * / and sqrt on float32 arrays are the correctly rounded IEEE ops) or one
``fma32``.  The scalars are formed in float64 from the group's hyper-parameter row and the tensor's own step count and
rounded to float32 once (``scalars`` follows make_scalars).  ``sqrt`` is a parameter of ``update``: the kernel promises
the correctly rounded one (numpy's); the host test injects aten's CPU sqrt to reproduce the reference's fixtures.

max / min are C's fmaxf / fminf (np.fmax / np.fmin), as the kernel calls them; they differ from aten's max / clamp only
on a NaN, which no test input produces.
"""
import math

import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
ADAMW, ADABOUND, SGDW = "adamw", "adabound", "sgdw"
CHUNK = 4096                 # elements per chunk of the persistent grid (unetpp_optim_chunk_elems)


def fma32(a, b, c):
    """The correctly rounded float32 fma(a, b, c) = RN32(a*b + c), element-wise.

    The product of two float32 is exact in float64 (48 bits).  p + c is added with TwoSum (s = RN64(p + c), e = the
    exact error); where e != 0 and s's last mantissa bit is even, s moves one float64 ulp towards e: s is then the
    exact sum rounded TO ODD at 53 bits, which rounds to float32 (24 bits, or fewer for a denormal) as the exact sum
    does.  A plain float32(float64(a)*b + c) rounds twice and is wrong at ties."""
    a, b, c = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32), np.asarray(c, dtype=F32)
    with np.errstate(all="ignore"):
        p = a.astype(F64) * b.astype(F64)
        c64 = np.broadcast_to(c.astype(F64), np.broadcast(p, c).shape)
        s = p + c64
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)
        fix = np.isfinite(s) & (e != 0) & ((s.view(I64) & 1) == 0)
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(F32)


class Scalars:
    __slots__ = ("b1", "omb1", "b2", "omb2", "eps", "wd", "neg_step", "step", "lo", "hi", "first")

    def bits(self):
        """name -> uint32 bit pattern of every float32 member (for messages and tables)"""
        return {k: int(np.asarray(getattr(self, k), dtype=F32).view(np.uint32)) for k in self.__slots__ if k != "first"}


def scalars(kind, hyper_row, t):
    """make_scalars: the per-segment float32 scalars from a group's row of float64 and the segment's step count t (the
    count of THIS update, >= 1).  Formed in float64 (Python floats, the host's pow and sqrt), each rounded once."""
    h = [float(x) for x in hyper_row]
    t = float(t)
    s = Scalars()
    s.b1, s.b2 = F32(h[1]), F32(h[2])
    s.omb1, s.omb2 = F32(1.0 - h[1]), F32(1.0 - h[2])          # SGDW: b1 = momentum, omb2 = 1 - dampening
    s.eps, s.wd = F32(h[3]), F32(h[4])
    s.first = t <= 1.0
    s.step = s.neg_step = s.lo = s.hi = F32(0.0)
    if kind != SGDW:
        bc1 = 1.0 - math.pow(h[1], t)
        bc2 = 1.0 - math.pow(h[2], t)
        step_size = h[0] * math.sqrt(bc2) / bc1
        s.step, s.neg_step = F32(step_size), F32(-step_size)
        if kind == ADABOUND:
            f, gamma = h[5], h[6]
            s.lo = F32(f * (1.0 - 1.0 / (gamma * t + 1.0)))
            s.hi = F32(f * (1.0 + 1.0 / (gamma * t)))
    return s


AUX_KEY = {ADAMW: "max_exp_avg_sq", ADABOUND: "max_exp_avg_sq", SGDW: "momentum_buffer"}


def update(kind, ams, p, g, state, s, has_aux, coef=None, sqrt=np.sqrt):
    """update<KIND, AMS> on whole float32 arrays -> (p, state) after the step; the inputs are not modified.
    state: {"exp_avg", "exp_avg_sq"} (AdamW, AdaBound), + "max_exp_avg_sq" (ams) or {"momentum_buffer"} (SGDW with
    momentum).  coef (float32): the clip coefficient, g = g * coef as one rounded multiply where g is read."""
    p, g = np.asarray(p), np.asarray(g)
    assert p.dtype == F32 and g.dtype == F32 and p.shape == g.shape
    out = dict(state)
    with np.errstate(all="ignore"):
        if coef is not None:
            g = g * F32(coef)
        decay = bool(s.wd != F32(0.0))
        if kind == SGDW:
            if has_aux:
                a = state["momentum_buffer"]
                out["momentum_buffer"] = F32(0.0) + g if s.first else fma32(s.omb2, g, a * s.b1)
            if decay:
                p = fma32(-s.wd, p, p)
            return p, out
        m, v = state["exp_avg"], state["exp_avg_sq"]
        if kind == ADABOUND and decay:
            g = fma32(s.wd, p, g)
        m = fma32(s.omb1, g, m * s.b1)
        v = fma32(s.omb2 * g, g, v * s.b2)
        out["exp_avg"], out["exp_avg_sq"] = m, v
        if ams:
            a = np.fmax(state["max_exp_avg_sq"], v)
            out["max_exp_avg_sq"] = a
            denom = np.asarray(sqrt(a), dtype=F32) + s.eps
        else:
            denom = np.asarray(sqrt(v), dtype=F32) + s.eps
        if kind == ADAMW:
            d = p * s.wd if decay else None
            p = p + (s.neg_step * m) / denom
            if decay:
                p = p - d
        else:
            r = s.step / denom
            r = np.fmin(np.fmax(r, s.lo), s.hi)
            r = r * m
            p = p - r
        assert p.dtype == F32 and m.dtype == F32 and v.dtype == F32 and denom.dtype == F32
    return p, out


def clip_coef(total_norm_f32, max_norm):
    """clip_prologue: c = max_norm / (total + 1e-6f); coef = c > 1 ? 1 : c, all float32; a NaN stays a NaN."""
    with np.errstate(all="ignore"):
        c = F32(max_norm) / (F32(total_norm_f32) + F32(1e-6))
        return F32(1.0) if c > F32(1.0) else F32(c)


def hyper_row(kind, group, base_lr=None):
    """optim.py's _hyper_row: the group's row of float64 (max_norm's slot is left 0: clip_coef takes it directly)."""
    if kind == SGDW:
        return [0.0, group["momentum"], group["dampening"], 0.0, group["weight_decay"], 0.0, 0.0, 0.0]
    b1, b2 = group["betas"]
    row = [group["lr"], b1, b2, group["eps"], group["weight_decay"], 0.0, 0.0, 0.0]
    if kind == ADABOUND:
        row[5], row[6] = group["final_lr"] * group["lr"] / base_lr, group["gamma"]
    return row


DEFAULTS = {
    ADAMW: dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0),
    ADABOUND: dict(lr=1e-3, betas=(0.9, 0.999), final_lr=0.1, gamma=1e-3, eps=1e-8, weight_decay=0),
    SGDW: dict(lr=1e-3, momentum=0, dampening=0, weight_decay=0),
}


class Driver:
    """Several steps over a list of tensors in parameter groups, as optim.py's step() drives the kernel: counts are per
    tensor (a tensor without a gradient is skipped and its count stays), rows are per group and re-read at every step
    (``groups[i]["lr"]`` may change between steps; AdaBound's base_lrs are the lr at construction).

    kind: ADAMW / ADABOUND / SGDW;  groups: list of dicts of hyper-parameters (missing keys: the class defaults);
    params: float32 arrays;  group_of: group index per tensor."""

    def __init__(self, kind, groups, params, group_of, ams=False, sqrt=np.sqrt):
        self.kind, self.ams, self.sqrt = kind, bool(ams), sqrt
        self.groups = [dict(DEFAULTS[kind], **g) for g in groups]
        self.base_lrs = [g["lr"] for g in self.groups]
        self.params = [np.array(p, dtype=F32, copy=True) for p in params]
        self.group_of = list(group_of)
        self.state = [{} for _ in self.params]
        self.count = [None] * len(self.params)        # None: no update yet
        self.last_scalars = [None] * len(self.params)

    def has_aux(self, i):
        g = self.groups[self.group_of[i]]
        return g["momentum"] != 0 if self.kind == SGDW else self.ams

    def set_counts(self, n):
        """every existing count becomes n (the next update of those tensors is their (n+1)-th)"""
        self.count = [None if c is None else n for c in self.count]

    def step(self, grads, coef=None):
        """One step(): grads[i] is a float32 array or None; coef: the clip coefficient of this step, or None."""
        rows = [hyper_row(self.kind, g, b) for g, b in zip(self.groups, self.base_lrs)]
        for i, g in enumerate(grads):
            if g is None:
                continue
            p = self.params[i]
            if self.count[i] is None:
                self.count[i] = 0
                if self.kind != SGDW:
                    self.state[i] = {"exp_avg": np.zeros_like(p), "exp_avg_sq": np.zeros_like(p)}
                if self.has_aux(i):
                    self.state[i][AUX_KEY[self.kind]] = np.zeros_like(p)
            self.count[i] += 1
            s = scalars(self.kind, rows[self.group_of[i]], self.count[i])
            self.last_scalars[i] = s
            self.params[i], self.state[i] = update(self.kind, self.ams, p, np.asarray(g, dtype=F32), self.state[i], s,
                                                   self.has_aux(i), coef=coef, sqrt=self.sqrt)


# ---- the configurations both test files run (group A: even tensor index, group B: odd) ---------------------------------
# name -> (kind, ams, group A, group B, {after step: factor on every group's lr})
CONFIGS = {
    "adamw": (ADAMW, False, dict(),
              dict(lr=3e-4, betas=(0.8, 0.95), eps=1e-6, weight_decay=1e-2), {}),
    "adamw_amsgrad": (ADAMW, True, dict(),
                      dict(lr=3e-4, betas=(0.8, 0.95), eps=1e-6, weight_decay=1e-2), {}),
    "adabound": (ADABOUND, False, dict(weight_decay=1e-4),
                 dict(lr=5e-4, final_lr=0.05, gamma=5e-3, betas=(0.85, 0.98)), {2: 0.1}),
    "adabound_amsbound": (ADABOUND, True, dict(weight_decay=1e-4),
                          dict(lr=5e-4, final_lr=0.05, gamma=5e-3, betas=(0.85, 0.98)), {2: 0.1}),
    "sgdw": (SGDW, False, dict(momentum=0, weight_decay=1e-4),
             dict(momentum=0.9, dampening=0.1, weight_decay=1e-3), {}),
    "sgdw_nesterov": (SGDW, False, dict(momentum=0.9, nesterov=True, weight_decay=0),
                      dict(momentum=0.9, nesterov=True, weight_decay=0), {}),
}
CLIPPED = ("adamw_amsgrad", "adabound", "sgdw")      # one per kind (sgdw: group B has momentum)


def group_kwargs(kind, group):
    """the keys the kernel reads per group, for the driver (nesterov changes nothing and is not one of them)"""
    return {k: v for k, v in group.items() if k != "nesterov"}
