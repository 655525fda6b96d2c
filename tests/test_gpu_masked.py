"""Length-masked question attention (C-ABI 0.8.0: coattn_forward_len / _infer_len / _attention_forward_len / _backward_len;
ParallelCoAttention(question_mask=True); train.py --question_mask) on the GPU.

The oracle needs no new math: the masked result for sample b is the reference's unmasked computation on Q[b, :len_b] alone,
so the float64 oracle runs per group of equal lengths on the truncated questions and a_q / C / dQ are padded with zeros."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import vqa_amd
from oracle import coattn_oracle as O
from vqa_amd import _lib

pytestmark = pytest.mark.gpu

NAMES = ("W_v.weight", "W_v.bias", "W_q.weight", "W_q.bias", "w_v.weight", "w_v.bias", "w_q.weight", "w_q.bias")
GRADS = ["dV_phys", "dQ"] + ["d" + k for k in NAMES]


def _flags(mode, impl):
    f = {"general": _lib.IMPL_GENERAL, "fused": _lib.IMPL_FUSED, "auto": _lib.IMPL_AUTO}[impl]
    return f | {"exact": 0, "fast16": _lib.FLAG_FAST16, "bf16": _lib.FLAG_BF16_PROJ}[mode]


def run(V, Qs, P, lens, gv=None, gq=None, mode="exact", impl="fused", layout="lm", infer=False):
    """One forward (+ backward) through the C-ABI.  V [B,d,N] values (layout: the physical form handed over), lens: None
    (the unmasked entry points) or host ints (the *_len ones, on the device as int32).  Every output is NaN-filled first."""
    lib = _lib.load()
    dev = torch.device("cuda:0")
    V = V.to(dev).contiguous()
    B, d, N = V.shape
    Vbuf, vstr = (V.permute(0, 2, 1).contiguous(), (N * d, d, 1)) if layout == "lm" else (V, (d * N, 1, N))
    Qs = [q.to(dev).contiguous() for q in Qs]
    L, T = len(Qs), Qs[0].shape[1]
    ps = [P[k].to(dev).contiguous() for k in NAMES]
    flag = _flags(mode, impl)
    sb, fb, bb = _lib.workspace_bytes(B, N, T, d, L, flag)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)   # noqa: E731
    v, q = nan(L, B, d), nan(L, B, d)
    ql = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    qptr = (C.c_void_p * L)(*[t.data_ptr() for t in Qs])
    p = _lib.Params(*[t.data_ptr() for t in ps])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    qa = () if ql is None else (C.c_void_p(ql.data_ptr()),)
    out = {}
    if infer:
        ws = nan(fb // 4)
        a_v, a_q = nan(L, B, N), nan(L, B, T)
        fn = lib.coattn_infer if ql is None else lib.coattn_infer_len
        _lib.check(fn(Vbuf.data_ptr(), *vstr, qptr, *qa, C.byref(p), v.data_ptr(), q.data_ptr(), a_v.data_ptr(),
                      a_q.data_ptr(), ws.data_ptr(), B, N, T, d, L, _lib.F32, flag, st), "infer")
        torch.cuda.synchronize()
        return {"v": v, "q": q, "a_v": a_v, "a_q": a_q}
    saved, ws = nan(sb // 4), nan(fb // 4)
    fn = lib.coattn_forward if ql is None else lib.coattn_forward_len
    _lib.check(fn(Vbuf.data_ptr(), *vstr, qptr, *qa, C.byref(p), v.data_ptr(), q.data_ptr(), saved.data_ptr(), ws.data_ptr(),
                  B, N, T, d, L, _lib.F32, flag, st), "forward")
    torch.cuda.synchronize()
    from tests._hip import saved_views
    out.update(saved_views(saved, B, N, T, d, L))
    out.update(v=v, q=q)
    if gv is None:
        return out
    gv, gq = gv.to(dev).contiguous(), gq.to(dev).contiguous()
    ws2 = nan(bb // 4)
    dV = torch.full_like(Vbuf, float("nan"))
    dQs = [torch.full_like(t, float("nan")) for t in Qs]
    grads = [torch.full_like(t, float("nan")) for t in ps]
    pg = _lib.ParamGrads(*[t.data_ptr() for t in grads])
    dqptr = (C.c_void_p * L)(*[t.data_ptr() for t in dQs])
    fn = lib.coattn_backward if ql is None else lib.coattn_backward_len
    _lib.check(fn(Vbuf.data_ptr(), *vstr, qptr, *qa, C.byref(p), saved.data_ptr(), gv.data_ptr(), gq.data_ptr(),
                  dV.data_ptr(), *vstr, dqptr, C.byref(pg), 0, ws2.data_ptr(), B, N, T, d, L, _lib.F32, flag, st), "backward")
    torch.cuda.synchronize()
    out["dV_phys"] = dV.permute(0, 2, 1).contiguous() if layout == "lm" else dV
    out["dQ"] = torch.stack(dQs)
    for k, g in zip(NAMES, grads):
        out["d" + k] = g
    return out


def oracle(V, Qs, P, lens, gv, gq):
    """float64: the reference's computation on Q[b, :len_b] for each group of equal (clamped) lengths, zero-padded."""
    L, B, T, d = len(Qs), V.shape[0], Qs[0].shape[1], V.shape[1]
    N = V.shape[2]
    P64 = {k: t.double() for k, t in P.items()}
    V64, Q64, gv64, gq64 = V.double(), [q.double() for q in Qs], gv.double(), gq.double()
    ln = [min(max(int(x), 1), T) for x in lens]
    o = {"v": torch.zeros(L, B, d, dtype=torch.float64), "q": torch.zeros(L, B, d, dtype=torch.float64),
         "a_v": torch.zeros(L, B, N, dtype=torch.float64), "a_q": torch.zeros(L, B, T, dtype=torch.float64),
         "C": torch.zeros(L, B, T, N, dtype=torch.float64), "dV_phys": torch.zeros(B, d, N, dtype=torch.float64),
         "dQ": torch.zeros(L, B, T, d, dtype=torch.float64)}
    for k in NAMES:
        o["d" + k] = torch.zeros_like(P64[k])
    for t in sorted(set(ln)):
        idx = torch.tensor([b for b in range(B) if ln[b] == t])
        qs = [q[idx, :t] for q in Q64]
        f = O.coattn_forward(V64[idx], qs, P64)
        g = O.coattn_backward(V64[idx], qs, P64, gv64[:, idx], gq64[:, idx])
        o["v"][:, idx], o["q"][:, idx], o["a_v"][:, idx] = f["v"], f["q"], f["a_v"]
        o["a_q"][:, idx, :t] = f["a_q"]
        o["C"][:, idx, :t] = f["C"]
        o["dV_phys"][idx] = g["dV_phys"]
        o["dQ"][:, idx, :t] = g["dQ"]
        for k in NAMES:
            o["d" + k] += g["d" + k]
    return o


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def err(r, o, k):
    """max|err| / max|ref|; absolute for dc_v / dc_q, which are 0 analytically (softmax shift invariance), as the goldens."""
    if k in ("dw_v.bias", "dw_q.bias"):
        return float((r[k].detach().double().cpu() - o[k]).abs().max())
    return rel(r[k], o[k])


def case(B, N, T, d, lens, seed=3, pad=None):
    P = O.make_params(d, seed)
    V, Qs = O.make_inputs(B, N, T, d, seed + 10, lens=lens, scale_q=(2.0 / d) ** 0.5)
    if pad is not None:                                    # finite non-zero values in the rows past each length
        for l, q in enumerate(Qs):
            junk = torch.from_numpy(O.hash_normal((B, T, d), seed + 50 + l, pad)).float()
            for b, n in enumerate(lens):
                q[b, min(max(n, 1), T):] = junk[b, min(max(n, 1), T):]
    gv = torch.from_numpy(O.hash_normal((len(Qs), B, d), seed + 5)).float()
    gq = torch.from_numpy(O.hash_normal((len(Qs), B, d), seed + 6)).float()
    return V, Qs, P, gv, gq


def mixed_lens(B, T):
    return [[1, T, 2, T - 1, 3, T // 2][b % 6] if b < 6 else 1 + (b * 7) % T for b in range(B)]


SMALL = [(6, 49, 12, 256), (5, 64, 7, 512), (4, 100, 26, 256)]


@pytest.mark.parametrize("shape", SMALL, ids=["n49_d256", "n64_d512", "n100_d256"])
@pytest.mark.parametrize("layout", ["lm", "cm"])
@pytest.mark.parametrize("mode,tol", [("exact", 1e-5), ("fast16", 5e-5)])
@pytest.mark.parametrize("impl", ["fused", "general"])
def test_masked_small_shapes_vs_truncated_oracle(shape, layout, mode, tol, impl):
    B, N, T, d = shape
    lens = mixed_lens(B, T)
    V, Qs, P, gv, gq = case(B, N, T, d, lens, pad=0.3)      # (non-zero pad rows: the mask must not read them)
    r = run(V, Qs, P, lens, gv, gq, mode=mode, impl=impl, layout=layout)
    o = oracle(V, Qs, P, lens, gv, gq)
    for k in ("v", "q", "a_v", "a_q", "C") + tuple(GRADS):
        assert err(r, o, k) < tol, (k, err(r, o, k))
    for b, n in enumerate(lens):
        assert (r["a_q"][:, b, n:] == 0).all() and (r["dQ"][:, b, n:] == 0).all() and (r["C"][:, b, n:] == 0).all()


@pytest.mark.parametrize("N", [49, 196])
@pytest.mark.parametrize("layout", ["lm", "cm"])
@pytest.mark.parametrize("mode,tol", [("exact", 2e-5), ("fast16", 1e-4)])
def test_masked_cfg2_vs_truncated_oracle(N, layout, mode, tol):
    B, T, d = 160, 26, 512
    lens = mixed_lens(B, T)
    V, Qs, P, gv, gq = case(B, N, T, d, lens, seed=17)
    r = run(V, Qs, P, lens, gv, gq, mode=mode, layout=layout)
    o = oracle(V, Qs, P, lens, gv, gq)
    for k in ("v", "q", "a_v", "a_q") + tuple(GRADS):
        assert err(r, o, k) < tol, (k, err(r, o, k))


def test_masked_long_questions_take_the_general_path():
    B, N, T, d = 4, 49, 40, 256                            # T > kTRows (28): no fused kernel
    lens = [40, 1, 29, 13]
    V, Qs, P, gv, gq = case(B, N, T, d, lens, pad=0.2)
    assert not _lib.load().coattn_fused_supported(B, N, T, d, 3, 0)
    for mode, tol in (("exact", 1e-5), ("fast16", 5e-5)):
        r = run(V, Qs, P, lens, gv, gq, mode=mode, impl="auto", layout="cm")
        o = oracle(V, Qs, P, lens, gv, gq)
        for k in ("v", "q", "a_v", "a_q") + tuple(GRADS):
            assert err(r, o, k) < tol, (mode, k, err(r, o, k))


def test_masked_reduced_precision_cfg4_shape():
    """cfg 4's width on the single-product (bf16) instantiations, at the bounds of the unmasked bf16 test
    (test_gpu_edges.py: 3e-2 absolute on v / q, 5e-2 of max|.| on the gradients)."""
    B, N, T, d = 8, 49, 26, 2048
    lens = mixed_lens(B, T)
    V, Qs, P, gv, gq = case(B, N, T, d, lens, seed=29, pad=0.05)
    o = oracle(V, Qs, P, lens, gv, gq)
    for layout in ("lm", "cm"):
        r = run(V, Qs, P, lens, gv, gq, mode="bf16", layout=layout)
        for k in ("v", "q"):
            assert float((r[k].double().cpu() - o[k]).abs().max()) < 3e-2, (layout, k)
        for k in GRADS:
            assert err(r, o, k) < 5e-2, (layout, k, err(r, o, k))
        for b, n in enumerate(lens):
            assert (r["a_q"][:, b, n:] == 0).all() and (r["dQ"][:, b, n:] == 0).all()


SHAPES_BITS = {"n49": (6, 49, 26, 512, "fused"), "n196": (4, 196, 26, 512, "fused"), "d256": (6, 49, 12, 256, "fused"),
               "general_d96": (4, 49, 12, 96, "auto")}
# (the single-product instantiations of the reduced-precision mode need d % 512 == 0)
BITS_CASES = [(s, m) for s in SHAPES_BITS for m in ("exact", "fast16", "bf16") if m != "bf16" or SHAPES_BITS[s][3] % 512 == 0]


@pytest.mark.parametrize("shape,mode", BITS_CASES, ids=["%s-%s" % c for c in BITS_CASES])
@pytest.mark.parametrize("layout", ["lm", "cm"])
def test_full_lengths_are_the_unmasked_call_bit_for_bit(shape, mode, layout):
    B, N, T, d, impl = SHAPES_BITS[shape]
    lens = [3, 1, T, 5, 2, T][:B]                             # pad rows of zeros in the inputs; the mask is T everywhere
    V, Qs, P, gv, gq = case(B, N, T, d, lens)
    a = run(V, Qs, P, None, gv, gq, mode=mode, impl=impl, layout=layout)
    b = run(V, Qs, P, [T] * B, gv, gq, mode=mode, impl=impl, layout=layout)
    for k in ("v", "q", "C", "a_v", "a_q", "H_q") + tuple(GRADS):
        assert torch.equal(a[k], b[k]), k
    ai = run(V, Qs, P, None, mode=mode, impl=impl, layout=layout, infer=True)
    bi = run(V, Qs, P, [T] * B, mode=mode, impl=impl, layout=layout, infer=True)
    for k in ("v", "q", "a_v", "a_q"):
        assert torch.equal(ai[k], bi[k]), k


@pytest.mark.parametrize("shape", [(8, 49, 26, 512, "fused"), (4, 196, 20, 512, "fused"), (5, 49, 12, 96, "auto")],
                         ids=["n49", "n196", "general"])
@pytest.mark.parametrize("layout", ["lm", "cm"])
@pytest.mark.parametrize("mode", ["exact", "fast16"])
def test_pad_row_contents_do_not_matter(shape, layout, mode):
    B, N, T, d, impl = shape
    lens = mixed_lens(B, T)
    V, Qz, P, gv, gq = case(B, N, T, d, lens, seed=41)
    _, Qj, _, _, _ = case(B, N, T, d, lens, seed=41, pad=0.5)
    assert not all(torch.equal(a, b) for a, b in zip(Qz, Qj))
    z = run(V, Qz, P, lens, gv, gq, mode=mode, impl=impl, layout=layout)
    j = run(V, Qj, P, lens, gv, gq, mode=mode, impl=impl, layout=layout)
    for k in ("v", "q", "C", "a_v", "a_q") + tuple(GRADS):
        assert torch.equal(z[k], j[k]), k
    for r in (z, j):
        for b, n in enumerate(lens):
            assert (r["dQ"][:, b, n:] == 0).all() and (r["a_q"][:, b, n:] == 0).all()


@pytest.mark.parametrize("N,layout", [(49, "lm"), (49, "cm"), (196, "lm")])
@pytest.mark.parametrize("mode", ["exact", "fast16"])
def test_masked_infer_equals_the_saving_forward(N, layout, mode):
    B, T, d = 12, 26, 512
    lens = mixed_lens(B, T)
    V, Qs, P, _, _ = case(B, N, T, d, lens, seed=5, pad=0.4)
    tr = run(V, Qs, P, lens, mode=mode, layout=layout)
    inf = run(V, Qs, P, lens, mode=mode, layout=layout, infer=True)
    for k in ("v", "q", "a_v", "a_q"):
        assert torch.equal(tr[k], inf[k]), k


@pytest.mark.parametrize("impl", ["fused", "general"])
def test_lengths_are_clamped(impl):
    B, N, T, d = 4, 49, 20, 256
    V, Qs, P, gv, gq = case(B, N, T, d, [20, 1, 20, 7], pad=0.3)
    a = run(V, Qs, P, [0, 1, T + 5, 7], gv, gq, impl=impl)
    b = run(V, Qs, P, [1, 1, T, 7], gv, gq, impl=impl)
    for k in ("v", "q", "C", "a_q") + tuple(GRADS):
        assert torch.equal(a[k], b[k]), k
    assert (a["a_q"][:, 0, 0] == 1).all() and (a["a_q"][:, 0, 1:] == 0).all()


@pytest.mark.parametrize("N", [49, 196])
@pytest.mark.parametrize("impl", ["fused", "general"])
def test_maps_sum_to_one_over_the_words_and_stay_in_their_buffers(N, impl):
    B, T, d = 16, 26, 512
    lens = mixed_lens(B, T)
    V, Qs, P, gv, gq = case(B, N, T, d, lens, pad=0.3)
    for infer in (False, True):
        r = run(V, Qs, P, lens, None if infer else gv, None if infer else gq, impl=impl, infer=infer)
        for k in ("v", "q", "a_v", "a_q") + (() if infer else tuple(GRADS)):
            assert torch.isfinite(r[k]).all(), (infer, k)        # every NaN-filled output element written
        sums = torch.stack([r["a_q"][:, b, :n].double().sum(-1) for b, n in enumerate(lens)], 1)
        assert torch.allclose(sums, torch.ones_like(sums), atol=1e-6)
        assert torch.allclose(r["a_v"].double().sum(-1), torch.ones(3, B, dtype=torch.float64, device="cuda"), atol=1e-6)


# ---------------------------------------------------------------------------------------------------------- model level
def _batch(B=8, T=26, vocab=100, K=10, seed=1):
    from vqa_amd import train as T_
    b = T_.synthetic_batch(B, (64, 64), T, vocab, K + 1, seed=seed)
    return T_.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])


def test_hot_path_modes_are_bit_identical_under_the_mask():
    """question_mask=True through the three hot-path modes a Trainer picks -- plain autograd over the modules
    (VQA_HOT_PATH=modules), the static node issued eagerly (the default) and its captured graphs (graph=True) -- from the same
    image features: the same loss and co-attention / answer-head gradients bit for bit.  (The stock question encoder's
    backward -- embedding, LSTM -- accumulates in no fixed order, so its gradients are compared to 1e-4; for the same reason,
    and the stock image encoder's, whole Trainer steps are not bitwise repeatable even in one mode, masked or not.)"""
    from vqa_amd import train as T
    dev = torch.device("cuda:0")
    im, qu, la, ln = _batch()
    assert int(ln.min()) < int(ln.max())
    torch.manual_seed(0)
    model = T.build_model("attention", 100, 10, question_mask=True).to(dev)
    with torch.no_grad():
        feats = model.image_encoder(im.to(dev)).detach()
    res = {}
    for mode in ("modules", "static", "graph"):
        model.hot_path_static = mode == "static"
        model.hot_path_graph = mode == "graph"
        model.hot_path_direct_grads = mode != "modules"
        for p in model.parameters():
            p.grad = None
        logits, loss = model.forward_features(feats, qu.to(dev), ln, labels=la.to(dev))
        loss.backward()
        res[mode] = (loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    assert len(model._graphs) == 2 and all(k[9] for k in model._graphs)        # the mask is part of the node's key
    for mode in ("static", "graph"):
        assert torch.equal(res[mode][0], res["modules"][0]), mode
        assert res[mode][1].keys() == res["modules"][1].keys()
        for n in res["modules"][1]:
            if n.startswith("question_encoder"):
                assert rel(res[mode][1][n], res["modules"][1][n]) < 1e-4, (mode, n)
            else:
                assert torch.equal(res[mode][1][n], res["modules"][1][n]), (mode, n)
    # one Trainer step per mode runs, and the mask changes the step (the batch has pad tokens)
    losses = {}
    for qm in (True, False):
        torch.manual_seed(0)
        m = T.build_model("attention", 100, 10, question_mask=qm).to(dev)
        losses[qm] = float(T.Trainer(m, 1e-4, dev, graph=qm).step(im.to(dev), qu.to(dev), ln, la.to(dev)).detach())
    assert abs(losses[True] - float(res["modules"][0])) < 1e-4 * abs(losses[True])
    assert losses[True] != losses[False]


class _MaskedOracleCoAttention(O.OracleParallelCoAttention):
    """The truncated oracle as a module under CPU autograd: per sample, the reference on Q[b, :len_b]."""
    question_mask = True

    def forward(self, x_img, x_ques_hierarchy, x_ques_lens):
        P = {k: v for k, v in self.named_parameters()}
        vs, qs = [], []
        for b, n in enumerate([int(x) for x in x_ques_lens]):
            r = O.coattn_forward(x_img[b:b + 1].permute(0, 2, 1), [q[b:b + 1, :n] for q in x_ques_hierarchy], P)
            vs.append(r["v"]); qs.append(r["q"])
        v, q = torch.cat(vs, 1), torch.cat(qs, 1)
        return [v[l] for l in range(v.shape[0])], [q[l] for l in range(q.shape[0])]


def test_masked_net_matches_the_float64_composition():
    """HierarchicalCoAttentionNet(question_mask) on the GPU against the same net in float64 on the CPU with the co-attention
    swapped for the truncated oracle: loss and every gradient, from the same image features."""
    from vqa_amd import train as T
    dev = torch.device("cuda:0")
    im, qu, la, ln = _batch(seed=3)
    torch.manual_seed(0)
    net = T.build_model("attention", 100, 10, question_mask=True)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        feats = net.image_encoder(im).detach()                    # one set of features for both sides
    gpu = net.to(dev)
    logits, loss = gpu.forward_features(feats.to(dev), qu.to(dev), ln, labels=la.to(dev))
    loss.backward()
    ref = T.build_model("attention", 100, 10)
    ref.co_attention = _MaskedOracleCoAttention(ref.hidden_dim)
    ref.load_state_dict(sd)
    ref = ref.double()
    _, loss64 = ref.forward_features(feats.double(), qu, ln, labels=la)
    loss64.backward()
    assert abs(float(loss.detach()) - float(loss64.detach())) < 1e-5 * abs(float(loss64.detach()))
    gp = dict(gpu.named_parameters())
    checked = 0
    for n, p in ref.named_parameters():
        if p.grad is None or n.startswith("image_encoder"):
            continue
        assert gp[n].grad is not None, n
        if n.endswith("w_v.bias") or n.endswith("w_q.bias"):    # 0 analytically (softmax shift invariance): absolute
            e = float((gp[n].grad.double().cpu() - p.grad).abs().max())
        else:
            e = rel(gp[n].grad, p.grad)
        assert e < 1e-4, (n, e)
        checked += 1
    assert checked >= 20 and gp["co_attention.W_b.weight"].grad is None


def test_predict_question_mask_writes_maps_without_weight_past_the_length(tmp_path, capsys):
    from vqa_amd import predict as Pr
    from vqa_amd import train as T
    common = ["--num_cls", "10", "--batch_size", "8", "--image_size", "64", "--vocab_size", "50", "--question_mask", "true"]
    ckpt = str(tmp_path / "att.pth")
    T.main(["--model", "attention", "--num_steps", "2", "--log_interval", "2", "--save_path", ckpt] + common)
    capsys.readouterr()
    S = 16
    maps = str(tmp_path / "maps.npz")
    summary = Pr.main(["--model", "attention", "--model_ckpt", ckpt, "--test_size", str(S), "--attention_maps", maps] + common)
    assert summary["samples"] == S
    z = np.load(maps)
    a_q, lens = z["a_q"], z["ques_len"]
    assert a_q.shape == (S, 3, 26) and lens.min() < 26
    for s in range(S):
        assert (a_q[s, :, lens[s]:] == 0).all()
        assert np.allclose(a_q[s, :, :lens[s]].sum(-1), 1.0, atol=1e-5)
    line = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines() if l.startswith("{")]
    assert line == [summary]
