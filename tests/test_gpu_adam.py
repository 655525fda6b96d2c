"""The optimiser step on the GPU (include/coattn.h v0.13.0, csrc/adam.hip): values, clipping, repeatability and isolation of
the C-ABI call, then ``HipAdam`` and ``Trainer(optimizer="hip")``.

The bound of the value tests is taken in the test from the stock fp32 optimiser (``foreach=False``) run on the same GPU on the
same bits, both measured against the float64 oracle of tests/_adam.py: for each of p, exp_avg and exp_avg_sq (over all tensors)
    err_hip <= 2 * err_stock + one fp32 ulp of the array's largest magnitude
(2: another, equally valid order of roundings -- fma against lerp; the ulp covers a stock error of zero).  The gradients of
the tensors differ in scale by up to 10^7, so exp_avg and exp_avg_sq of a small-scale tensor are invisible in a figure taken
over all tensors; as a net under it, each tensor's exp_avg (exp_avg_sq) is also held to 32 ulp of the largest magnitude among
its own gradients (of its square): five steps of at most six roundings each (g * clip, its square, times 1 - beta2, the fma,
and the clip coefficient's own two), each no larger than an ulp at that magnitude.  p needs no such net: the values are N(0, 1)
and Adam's step is about lr in every tensor, whatever its gradient scale.
"""
import copy
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import _adam as A

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000


def dev():
    return torch.device("cuda:0")


class Flat:
    """p, g, exp_avg, exp_avg_sq of a tensor list as views into four NaN-filled flat buffers: every view starts at an element
    offset = 1 (mod 4) (4-byte aligned only) or = 0 (mod 4) (16-byte aligned), with at least one guard element on each side."""

    def __init__(self, sizes, aligned):
        self.sizes = tuple(sizes)
        self.starts = []
        off = 4
        for n in self.sizes:
            start = (off + 3) // 4 * 4 + (0 if aligned else 1)
            self.starts.append(start)
            off = start + n + 1
        self.total = off + 4
        self.buf = {k: torch.full((self.total,), float("nan"), device=dev()) for k in "pgmv"}
        inside = np.zeros(self.total, dtype=bool)
        for s, n in zip(self.starts, self.sizes):
            inside[s:s + n] = True
        self.outside = torch.from_numpy(~inside)
        for k in "pgmv":
            assert self.buf[k].data_ptr() % 16 == 0
            for t in self.views(k):
                assert t.data_ptr() % 16 == (0 if aligned else 4)

    def views(self, k):
        return [self.buf[k][s:s + n] for s, n in zip(self.starts, self.sizes)]

    def put(self, k, arrays):
        for t, a in zip(self.views(k), arrays):
            t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))

    def get(self, k):
        return [t.cpu().numpy().copy() for t in self.views(k)]

    def guards_intact(self):
        return all(bool((self.buf[k].cpu().view(torch.int32)[self.outside] == NAN_BITS).all()) for k in "pgmv")

    def snapshot(self):
        return {k: self.buf[k].clone() for k in "pgmv"}

    def restore(self, snap):
        for k in "pgmv":
            self.buf[k].copy_(snap[k])


def hip_step(entries, step, lr, wd=0.0, max_norm=0.0, norm_out=None, betas=(0.9, 0.999), eps=1e-8):
    """One coattn_adam_step over entries = [(p, g, m, v, n)] of CUDA tensors, on the current stream; the workspace of a clipped
    call is handed over full of NaN bits (its contents need no initialisation)."""
    from vqa_amd import _lib
    lib = _lib.load()
    arr = (_lib.AdamTensor * len(entries))()
    for e, (p, g, m, v, n) in zip(arr, entries):
        e.p, e.g, e.m, e.v, e.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n
    ws, nbytes = None, 0
    if max_norm > 0:
        nbytes = lib.coattn_adam_workspace_bytes(arr, len(entries))
        assert nbytes >= 64
        ws = torch.full(((nbytes + 7) // 8,), float("nan"), device=dev(), dtype=torch.float64)
    _lib.check(lib.coattn_adam_step(arr, len(entries), step, lr, betas[0], betas[1], eps, wd, max_norm,
                                    C.c_void_p(norm_out.data_ptr() if norm_out is not None else 0),
                                    C.c_void_p(ws.data_ptr() if ws is not None else 0), nbytes,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), "coattn_adam_step")
    torch.cuda.synchronize()


def entries_of(flat):
    return [(*quad, quad[0].numel()) for quad in zip(*(flat.views(k) for k in "pgmv"))]


@functools.lru_cache(maxsize=None)
def inputs():
    return A.make_inputs()


@functools.lru_cache(maxsize=None)
def run(aligned, wd, lr, max_norm):
    """STEPS steps of the library, the stock fp32 optimiser on the same GPU and the float64 oracle on the same bits.
    max_norm: None = unclipped."""
    params, grads = inputs()
    flat = Flat(A.SIZES, aligned)
    flat.put("p", params)
    flat.put("m", [np.zeros_like(p) for p in params])
    flat.put("v", [np.zeros_like(p) for p in params])
    ref = A.Adam(params, lr=lr, weight_decay=wd, max_grad_norm=max_norm)
    tp = [torch.nn.Parameter(torch.from_numpy(p).to(dev())) for p in params]
    stock = (torch.optim.AdamW if wd else torch.optim.Adam)(tp, lr=lr, weight_decay=wd, foreach=False)
    norm_out = torch.full((), float("nan"), device=dev())
    out = dict(norm_hip=[], norm_stock=[], norm_ref=[], grads_kept=True)
    for t, gs in enumerate(grads, start=1):
        flat.put("g", gs)
        before = flat.buf["g"].clone()
        hip_step(entries_of(flat), t, lr, wd, max_norm or 0.0, norm_out if max_norm else None)
        out["grads_kept"] &= bool(torch.equal(before.view(torch.int32), flat.buf["g"].view(torch.int32)))
        for p, g in zip(tp, gs):
            p.grad = torch.from_numpy(g).to(dev())
        if max_norm:
            out["norm_stock"].append(float(torch.nn.utils.clip_grad_norm_(tp, max_norm, foreach=False).double()))
            out["norm_hip"].append(float(norm_out.double()))
        stock.step()
        out["norm_ref"].append(ref.step(gs))
    out["guards"] = flat.guards_intact()
    out["hip"] = {k: flat.get(k) for k in "pmv"}
    out["stock"] = dict(p=[p.detach().cpu().numpy() for p in tp], m=[stock.state[p]["exp_avg"].cpu().numpy() for p in tp],
                        v=[stock.state[p]["exp_avg_sq"].cpu().numpy() for p in tp])
    out["ref"] = dict(p=ref.p, m=ref.m, v=ref.v)
    return out


def hold(hip, stock, ref, what, scales=None):
    """The bound of this file's docstring for one array; prints the figures it compares.  scales: per tensor, the magnitude
    whose ulp the per-tensor net is taken at (None: no net)."""
    e_hip, top = A.max_err(hip, ref)
    e_stock, _ = A.max_err(stock, ref)
    print("%s: err hip %.3e, stock %.3e, ulp(max |x| = %.4g) = %.3e" % (what, e_hip, e_stock, top, A.ulp32(top)))
    assert e_hip <= 2.0 * e_stock + A.ulp32(top), what
    for i, scale in enumerate(scales or ()):
        e, _ = A.max_err([hip[i]], [ref[i]])
        assert e <= 32.0 * A.ulp32(scale), (what, i, e, scale)


def grad_scales(power):
    _, grads = inputs()
    return [max(float(np.max(np.abs(gs[i]))) for gs in grads) ** power for i in range(len(A.SIZES))]


def hold_all(r, suffix=""):
    for k, name, scales in (("p", "p", None), ("m", "exp_avg", grad_scales(1)), ("v", "exp_avg_sq", grad_scales(2))):
        hold(r["hip"][k], r["stock"][k], r["ref"][k], name + suffix, scales)


CONFIGS = list(itertools.product((False, True), (0.0, 0.01), (1e-3, 1e-4)))
IDS = ["%s-wd%g-lr%g" % ("aligned16" if a else "aligned4", wd, lr) for a, wd, lr in CONFIGS]


@pytest.mark.parametrize("aligned,wd,lr", CONFIGS, ids=IDS)
def test_values_follow_the_oracle_as_closely_as_the_stock_optimiser(aligned, wd, lr):
    r = run(aligned, wd, lr, None)
    hold_all(r)
    assert r["grads_kept"] and r["guards"]


@pytest.mark.parametrize("aligned,wd,lr", CONFIGS, ids=IDS)
def test_clipping_by_global_norm(aligned, wd, lr):
    r = run(aligned, wd, lr, 1.0)
    for t, (got, stock, ref) in enumerate(zip(r["norm_hip"], r["norm_stock"], r["norm_ref"])):
        print("step %d: norm %.9g, err hip %.3e, stock %.3e" % (t + 1, ref, abs(got - ref), abs(stock - ref)))
        assert ref > 1.0                                  # the clip is active
        assert abs(got - ref) <= 2.0 * abs(stock - ref) + 2.0 ** -22 * ref
    hold_all(r, " (clipped)")
    assert r["grads_kept"] and r["guards"]


@pytest.mark.parametrize("aligned", [False, True], ids=["aligned4", "aligned16"])
def test_a_clip_that_does_not_bind_changes_no_bit(aligned):
    free, loose = run(aligned, 0.01, 1e-3, None), run(aligned, 0.01, 1e-3, 1e9)
    for k in "pmv":
        for a, b in zip(free["hip"][k], loose["hip"][k]):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert loose["grads_kept"] and loose["guards"] and all(n > 1.0 for n in loose["norm_hip"])


@pytest.mark.parametrize("aligned", [False, True], ids=["aligned4", "aligned16"])
def test_the_clipped_call_repeats_bit_for_bit(aligned):
    params, grads = inputs()
    flat = Flat(A.SIZES, aligned)
    flat.put("p", params)
    for k in "mv":
        flat.put(k, [np.zeros_like(p) for p in params])
    norm = torch.full((), float("nan"), device=dev())
    for t in (1, 2):
        flat.put("g", grads[t - 1])
        hip_step(entries_of(flat), t, 1e-3, 0.01, 1.0, norm)
    flat.put("g", grads[2])
    snap = flat.snapshot()
    outs = []
    for _ in range(2):
        flat.restore(snap)
        norm.fill_(float("nan"))
        hip_step(entries_of(flat), 3, 1e-3, 0.01, 1.0, norm)
        outs.append({k: flat.buf[k].clone().view(torch.int32) for k in "pgmv"} | {"norm": norm.clone().view(torch.int32)})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert torch.equal(outs[0]["g"], snap["g"].view(torch.int32)) and flat.guards_intact()
    assert bool(torch.isfinite(norm))


def test_empty_entries_and_a_second_launch_change_nothing_per_tensor():
    """70 non-empty tensors (the launch takes 64) around an n = 0 entry, against the same tensors updated one call each; the
    clipped form of the long list counts its tickets over both launches."""
    sizes = [(1, 3, 63, 65, 255, 1025, 4097)[i % 7] for i in range(70)]
    params, grads = A.make_inputs(sizes=sizes, steps=2, seed=7)
    results = []
    for one_by_one in (False, True):
        flat = Flat(sizes, aligned=False)
        flat.put("p", params)
        for k in "mv":
            flat.put(k, [np.zeros_like(p) for p in params])
        for t in (1, 2):
            flat.put("g", grads[t - 1])
            ents = entries_of(flat)
            if one_by_one:
                for e in ents:
                    hip_step([e], t, 1e-3, 0.01)
            else:
                empty = (*ents[5][:4], 0)                  # live pointers, no elements: skipped
                hip_step(ents[:33] + [empty] + ents[33:], t, 1e-3, 0.01)
        assert flat.guards_intact()
        results.append({k: flat.buf[k].clone().view(torch.int32) for k in "pmv"})
    for k in "pmv":
        assert torch.equal(results[0][k], results[1][k]), k
    # clipped, over both launches: the norm against the oracle (double accumulation, one fp32 rounding: 2^-23 relative;
    # 2^-22 asserted), twice the same bits
    flat = Flat(sizes, aligned=True)
    flat.put("p", params)
    for k in "mv":
        flat.put(k, [np.zeros_like(p) for p in params])
    flat.put("g", grads[0])
    snap = flat.snapshot()
    want, _ = A.clip_coef(grads[0], 1.0)
    seen = []
    for _ in range(2):
        flat.restore(snap)
        norm = torch.full((), float("nan"), device=dev())
        hip_step(entries_of(flat), 1, 1e-3, 0.0, 1.0, norm)
        assert abs(float(norm.double()) - want) <= 2.0 ** -22 * want
        seen.append({k: flat.buf[k].clone().view(torch.int32) for k in "pmv"} | {"norm": norm.view(torch.int32).clone()})
    for k in seen[0]:
        assert torch.equal(seen[0][k], seen[1][k]), k
    ref = A.Adam(params, lr=1e-3, max_grad_norm=1.0)
    ref.step(grads[0])
    for k, want_k in (("p", ref.p), ("m", ref.m), ("v", ref.v)):
        for a, b in zip(flat.get(k), want_k):
            e, top = A.max_err([a], [b])                      # one step from zero moments: at most six roundings (this file's
            assert e <= 8.0 * A.ulp32(max(top, 1.0) if k == "p" else top), (k, e, top)   # docstring); p at its unit scale


# ---- HipAdam ---------------------------------------------------------------------------------------------------------

def _params_and_grads(sizes=(3, 65, 1025, 4097), steps=5, seed=11):
    params, grads = A.make_inputs(sizes=sizes, steps=steps, seed=seed)
    return params, grads


def _drive(opt, tp, grads):
    for gs in grads:
        for p, g in zip(tp, gs):
            p.grad = torch.from_numpy(g).to(dev())
        opt.step()


def _state(opt, tp):
    return dict(p=[p.detach().cpu().numpy() for p in tp], m=[opt.state[p]["exp_avg"].cpu().numpy() for p in tp],
                v=[opt.state[p]["exp_avg_sq"].cpu().numpy() for p in tp])


@pytest.mark.parametrize("first", ["torch", "hip"])
def test_state_dicts_move_between_hipadam_and_the_stock_adam(first):
    """Two steps on one optimiser, its state_dict loaded into the other kind, three more steps: the result agrees with the
    first kind continuing, each way, to the bound of this file (the oracle continues from the fp32 state after step 2)."""
    from vqa_amd import HipAdam
    params, grads = _params_and_grads()
    make = dict(torch=lambda ps: torch.optim.Adam(ps, lr=1e-3, foreach=False), hip=lambda ps: HipAdam(ps, lr=1e-3))
    other = "hip" if first == "torch" else "torch"
    tp = [torch.nn.Parameter(torch.from_numpy(p).to(dev())) for p in params]
    opt = make[first](tp)
    _drive(opt, tp, grads[:2])
    mid = _state(opt, tp)
    assert all(float(opt.state[p]["step"]) == 2.0 for p in tp)
    tp2 = [torch.nn.Parameter(p.detach().clone()) for p in tp]
    moved = make[other](tp2)
    moved.load_state_dict(copy.deepcopy(opt.state_dict()))       # (as a checkpoint does: load_state_dict keeps the tensors it is given)
    _drive(opt, tp, grads[2:])
    _drive(moved, tp2, grads[2:])
    assert all(float(moved.state[p]["step"]) == 5.0 for p in tp2)
    ref = A.Adam(mid["p"], lr=1e-3, t=2, exp_avg=mid["m"], exp_avg_sq=mid["v"])
    for gs in grads[2:]:
        ref.step(gs)
    a, b = _state(opt, tp), _state(moved, tp2)
    for k, want in (("p", ref.p), ("m", ref.m), ("v", ref.v)):
        hold(a[k], b[k], want, "%s continuing vs loaded %s: %s" % (first, other, k))
        hold(b[k], a[k], want, "loaded %s vs %s continuing: %s" % (other, first, k))


def test_a_parameter_without_gradient_keeps_its_bits_and_has_no_state():
    from vqa_amd import HipAdam
    params, grads = _params_and_grads(steps=1)
    tp = [torch.nn.Parameter(torch.from_numpy(p).to(dev())) for p in params]
    opt = HipAdam(tp, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    for i, (p, g) in enumerate(zip(tp, grads[0])):
        p.grad = None if i == 1 else torch.from_numpy(g).to(dev())
    opt.step()
    assert tp[1] not in opt.state and np.array_equal(tp[1].detach().cpu().numpy().view(np.int32), params[1].view(np.int32))
    assert all(len(opt.state[p]) == 3 and float(opt.state[p]["step"]) == 1.0 for i, p in enumerate(tp) if i != 1)
    assert not np.array_equal(tp[0].detach().cpu().numpy(), params[0])
    want, _ = A.clip_coef([g for i, g in enumerate(grads[0]) if i != 1], 1.0)
    assert opt.grad_norm.is_cuda and abs(float(opt.grad_norm) - want) <= 2.0 ** -22 * want
    # a gradient that is a non-contiguous view is taken as its values; a non-fp32 parameter is refused
    q = torch.nn.Parameter(torch.zeros(6, 4, device=dev()))
    q.grad = torch.ones(4, 6, device=dev()).t()
    o2 = HipAdam([q], lr=0.5)
    o2.step()
    assert torch.allclose(q.detach(), torch.full_like(q, -0.5), rtol=0, atol=1e-6)
    h = torch.nn.Parameter(torch.zeros(4, device=dev(), dtype=torch.float64))
    h.grad = torch.ones_like(h)
    with pytest.raises(RuntimeError, match="fp32"):
        HipAdam([h]).step()


def test_a_scheduler_changes_the_step_size():
    from vqa_amd import HipAdam
    p = torch.nn.Parameter(torch.zeros(1000, device=dev()))
    opt = HipAdam([p], lr=1e-2)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.1)
    moves = []
    for _ in range(3):
        before = p.detach().clone()
        p.grad = torch.ones_like(p)
        opt.step()
        sched.step()
        moves.append(float((before - p.detach()).abs().max()))
    # a constant gradient moves every element by lr per step (m / sqrt(v) = 1 after the bias corrections)
    for got, want in zip(moves, (1e-2, 1e-3, 1e-4)):
        assert abs(got - want) <= 1e-4 * want


# ---- Trainer ---------------------------------------------------------------------------------------------------------

class _Recorded(torch.nn.Module):
    """Stands in for the frozen image encoder: returns the features recorded from it once."""

    def __init__(self, feats):
        super().__init__()
        self.feats = feats

    def forward(self, image):
        return self.feats


_features = {}


def _train_losses(**kw):
    """test_trainer_default_path_matches_the_module_path's setting.  The first loss of two trainers is compared bit for bit
    here, so the frozen stock image encoder runs ONCE and every trainer of this file is given that output: its MIOpen
    convolutions do not repeat their bits from call to call (measured on the parent's path: four default trainers in one
    process gave four different feature hashes and two different first losses, 0x1.2cc234p+1 and 0x1.2cc236p+1), and that is
    not what this file is about.  The encoder has no trainable parameter, so no optimiser touches it."""
    from vqa_amd import train as T
    torch.manual_seed(0)
    model = T.build_model("attention", 100, 10).to(dev())
    assert not any(p.requires_grad for p in model.image_encoder.parameters())
    b = T.synthetic_batch(8, (64, 64), 26, 100, 11, seed=1)
    im, qu, la, ln = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])
    im, qu, la = im.to(dev()), qu.to(dev()), la.to(dev())
    if "f" not in _features:
        with torch.no_grad():
            _features["f"] = model.image_encoder(im)
    model.image_encoder = _Recorded(_features["f"])
    tr = T.Trainer(model, 1e-4, dev(), **kw)
    losses = [float(tr.step(im, qu, ln, la, next_image=im).detach()) for _ in range(3)]
    return tr, losses


def test_trainer_with_the_hip_optimiser_follows_the_default():
    from vqa_amd import HipAdam
    tr0, base = _train_losses()
    tr1, hip = _train_losses(optimizer="hip")
    assert type(tr0.optimizer) is torch.optim.Adam and type(tr1.optimizer) is HipAdam
    print("losses: default %r, hip %r" % (base, hip))
    assert hip[0] == base[0]                              # same parameters, the optimiser has not acted yet
    for a, b in zip(base[1:], hip[1:]):
        assert abs(a - b) <= 1e-5 * abs(a)
    assert tr1.optimizer.grad_norm is None
    dead = tr1.model.co_attention.W_b.weight               # never used by the reference affinity: no gradient, no state
    assert dead.grad is None and dead not in tr1.optimizer.state
    tr2, clipped = _train_losses(optimizer="hip", clip_grad_norm=0.1)
    norm = float(tr2.optimizer.grad_norm)
    print("clipped losses %r, last norm %.6g" % (clipped, norm))
    assert np.isfinite(norm) and norm > 0
    assert clipped[0] == base[0] and clipped[1:] != hip[1:]
