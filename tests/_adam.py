"""Float64 numpy oracle of the optimiser step (include/coattn.h v0.13.0): torch.optim.Adam / AdamW's update and
torch.nn.utils.clip_grad_norm_, written from their definitions (Kingma & Ba 2015, algorithm 1; Loshchilov & Hutter 2019,
algorithm 2), independent of the product code -- and the seeded inputs the CPU and GPU tests share."""
import numpy as np

SIZES = (1, 3, 63, 64, 65, 255, 1024, 1025, 4097, 70001)
STEPS = 5


def clip_coef(grads, max_norm):
    """(global norm, min(1, max_norm / (norm + 1e-6))) of a list of float64 arrays."""
    norm = float(np.sqrt(sum(float(np.sum(np.square(g.astype(np.float64)))) for g in grads)))
    return norm, min(1.0, max_norm / (norm + 1e-6))


class Adam:
    """State of one parameter list; step() applies one update in place and returns the gradient norm (None unclipped)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, t=0,
                 exp_avg=None, exp_avg_sq=None):
        self.p = [np.array(p, dtype=np.float64) for p in params]
        self.m = [np.zeros_like(p) for p in self.p] if exp_avg is None else [np.array(x, dtype=np.float64) for x in exp_avg]
        self.v = [np.zeros_like(p) for p in self.p] if exp_avg_sq is None else [np.array(x, dtype=np.float64) for x in exp_avg_sq]
        self.lr, self.betas, self.eps, self.wd, self.max_norm, self.t = lr, betas, eps, weight_decay, max_grad_norm, t

    def step(self, grads):
        b1, b2 = self.betas
        self.t += 1
        norm, coef = None, 1.0
        if self.max_norm is not None:
            norm, coef = clip_coef(grads, self.max_norm)
        bc1, bc2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
        for p, g, m, v in zip(self.p, grads, self.m, self.v):
            g = g.astype(np.float64) * coef
            if self.wd:
                p *= 1.0 - self.lr * self.wd
            m[...] = b1 * m + (1.0 - b1) * g
            v[...] = b2 * v + (1.0 - b2) * g * g
            p -= (self.lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + self.eps)
        return norm


def make_inputs(sizes=SIZES, steps=STEPS, seed=2024):
    """(params, grads[step][tensor]) in fp32: values N(0, 1), gradients N(0, 1) * 10^U{-6..1} with one exponent per tensor;
    the same bits at every call."""
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    expo = rng.integers(-6, 2, size=len(sizes))
    grads = [[(rng.standard_normal(n) * 10.0 ** int(e)).astype(np.float32) for n, e in zip(sizes, expo)] for _ in range(steps)]
    return params, grads


def ulp32(x):
    """One fp32 unit in the last place at magnitude x."""
    return float(np.spacing(np.float32(abs(x))))


def max_err(got, ref):
    """Largest |got - ref| over a list of arrays (float64 arithmetic), and the largest |ref|."""
    err = max(float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b))) for a, b in zip(got, ref))
    return err, max(float(np.max(np.abs(b))) for b in ref)
