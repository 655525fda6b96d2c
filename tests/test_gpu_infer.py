"""coattn_infer (include/coattn.h, v0.7.0): the forward that keeps no backward state and hands the attention maps to the
caller -- bit-identical v / q to the saving forward in every mode, maps against the goldens and the float64 oracle, output
bounds, the range report on the workspace, and the layers above it (ParallelCoAttention / HierarchicalCoAttentionNet
.forward_with_attention, predict.py)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from oracle import coattn_oracle as O

pytestmark = pytest.mark.gpu

NAMES = ("W_v.weight", "W_v.bias", "W_q.weight", "W_q.bias", "w_v.weight", "w_v.bias", "w_q.weight", "w_q.bias")


def _flags(mode, impl="auto"):
    from vqa_amd import _lib
    f = {"auto": _lib.IMPL_AUTO, "general": _lib.IMPL_GENERAL, "fused": _lib.IMPL_FUSED}[impl]
    return f | {"exact": 0, "fast16": _lib.FLAG_FAST16, "bf16": _lib.FLAG_BF16_PROJ}[mode]


def _setup(V, Qs, P, layout):
    """V [B,d,N] values -> (device buffer in `layout`, element strides, device Qs, device params)."""
    dev = torch.device("cuda:0")
    V = V.to(dev).contiguous()
    B, d, N = V.shape
    if layout == "lm":
        Vbuf, vstr = V.permute(0, 2, 1).contiguous(), (N * d, d, 1)
    else:
        Vbuf, vstr = V, (d * N, 1, N)
    return Vbuf, vstr, [q.to(dev).contiguous() for q in Qs], [P[k].to(dev).contiguous() for k in NAMES]


def _pair(V, Qs, P, mode, layout="lm", impl="auto", maps=True):
    """coattn_forward with `saved` and coattn_infer on the same inputs, every buffer NaN-filled first.
    Returns (training forward's dict, inference dict, workspace of the inference call)."""
    from vqa_amd import _lib
    from tests._hip import saved_views
    lib = _lib.load()
    Vbuf, vstr, Qd, ps = _setup(V, Qs, P, layout)
    B, d, N = V.shape
    T, L = Qs[0].shape[1], len(Qs)
    flags = _flags(mode, impl)
    sb, fb, _ = _lib.workspace_bytes(B, N, T, d, L, flags)
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")      # noqa: E731
    qptr = (C.c_void_p * L)(*[t.data_ptr() for t in Qd])
    p = _lib.Params(*[t.data_ptr() for t in ps])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tr = {"v": nan(L, B, d), "q": nan(L, B, d)}
    saved, ws1 = nan(sb // 4), nan(fb // 4)
    _lib.check(lib.coattn_forward(Vbuf.data_ptr(), *vstr, qptr, C.byref(p), tr["v"].data_ptr(), tr["q"].data_ptr(),
                                  saved.data_ptr(), ws1.data_ptr(), B, N, T, d, L, _lib.F32, flags, st), "coattn_forward")
    sv = saved_views(saved, B, N, T, d, L)
    tr["a_v"], tr["a_q"] = sv["a_v"], sv["a_q"]
    inf = {"v": nan(L, B, d), "q": nan(L, B, d), "a_v": nan(L, B, N) if maps else None, "a_q": nan(L, B, T) if maps else None}
    ws = nan(fb // 4)
    ptr = lambda t: t.data_ptr() if t is not None else None          # noqa: E731
    _lib.check(lib.coattn_infer(Vbuf.data_ptr(), *vstr, qptr, C.byref(p), inf["v"].data_ptr(), inf["q"].data_ptr(),
                                ptr(inf["a_v"]), ptr(inf["a_q"]), ws.data_ptr(), B, N, T, d, L, _lib.F32, flags, st),
               "coattn_infer")
    torch.cuda.synchronize()
    return tr, inf, ws


def _inputs(B, N, d, seed, T=26):
    lens = [T, 1] + [3 + (7 * b) % (T - 2) for b in range(B - 2)]
    V, Qs = O.make_inputs(B, N, T, d, seed, lens=lens[:B], scale_q=(2.0 / d) ** 0.5)
    return V, Qs, O.make_params(d, seed + 1), lens[:B]


@pytest.mark.parametrize("mode", ["exact", "fast16"])
@pytest.mark.parametrize("layout", ["lm", "cm"])
@pytest.mark.parametrize("N", [49, 196])
@pytest.mark.parametrize("B", [5, 160])
def test_infer_equals_training_forward_bit_for_bit(B, N, layout, mode):
    V, Qs, P, _ = _inputs(B, N, 512, 40 + N + B)
    for maps in (True, False):
        tr, inf, _ = _pair(V, Qs, P, mode, layout, maps=maps)
        assert torch.equal(tr["v"], inf["v"]) and torch.equal(tr["q"], inf["q"]), (maps,)
        if maps:      # the maps are the ones the saving forward keeps in `saved`, written to the caller's buffers
            assert torch.equal(tr["a_v"], inf["a_v"]) and torch.equal(tr["a_q"], inf["a_q"])


def test_infer_reduced_precision_d2048_and_general_path():
    from tests import _golden as G
    V, Qs, P, _, _ = G.build_case("g6_d2048_n49", torch.float32)         # config 4's width, bf16 MFMA projections
    for layout in ("lm", "cm"):
        tr, inf, _ = _pair(V, Qs, P, "bf16", layout)
        for k in ("v", "q", "a_v", "a_q"):
            assert torch.equal(tr[k], inf[k]), (layout, k)
    for name in ("g1_tiny_d64", "g1_odd_d96"):                            # general-shape kernels (C a real intermediate)
        V, Qs, P, _, _ = G.build_case(name, torch.float32)
        gold = G.load(name)
        for mode in ("exact", "fast16"):
            tr, inf, _ = _pair(V, Qs, P, mode, "cm", impl="auto")
            for k in ("v", "q", "a_v", "a_q"):
                assert torch.equal(tr[k], inf[k]), (name, mode, k)
            e = G.fwd_errors(inf, gold, "64")
            assert e["a_v"] < 1e-5 and e["a_q"] < 1e-5 and e["v"] < 1e-4 and e["q"] < 1e-4, (name, mode, e)


@pytest.mark.parametrize("mode,tol", [("exact", 1e-5), ("fast16", 5e-5)])
def test_infer_maps_match_the_goldens(mode, tol):
    from tests import _golden as G
    for name in ("g2_cfg2_natural", "g3_n49_ragged", "g5_cfg2_scaled", "g5_d256"):
        V, Qs, P, _, _ = G.build_case(name, torch.float32)
        gold = G.load(name)
        c = G.CASES[name]
        for layout in ("lm", "cm"):
            _, inf, _ = _pair(V, Qs, P, mode, layout)
            e = G.fwd_errors(inf, gold, "64")
            assert e["a_v"] < tol and e["a_q"] < tol, (name, layout, e)
            # rows are distributions; a_q is unmasked (model.py:388): pad tokens carry weight
            assert torch.allclose(inf["a_v"].sum(-1), torch.ones_like(inf["a_v"][..., 0]), atol=1e-5)
            assert torch.allclose(inf["a_q"].sum(-1), torch.ones_like(inf["a_q"][..., 0]), atol=1e-5)
            for b, ln in enumerate(c["lens"]):
                if ln < c["T"]:
                    assert (inf["a_q"][:, b, ln:] > 0).all(), (name, b)


@pytest.mark.parametrize("mode,tol", [("exact", 2e-5), ("fast16", 1e-4)])
@pytest.mark.parametrize("N", [49, 196])
def test_infer_maps_match_the_float64_oracle_at_cfg2(N, mode, tol):
    B, d = 160, 512
    V, Qs, P, lens = _inputs(B, N, d, 90 + N)
    f = O.coattn_forward(V.double(), [q.double() for q in Qs], {k: v.double() for k, v in P.items()})
    for layout in ("lm", "cm"):
        _, inf, _ = _pair(V, Qs, P, mode, layout)
        for k in ("a_v", "a_q"):
            err = float((inf[k].cpu().double() - f[k]).abs().max())
            assert err < tol, (layout, k, err)
        assert float((inf["v"].cpu().double() - f["v"]).abs().max()) < 1e-4
        assert (inf["a_q"][:, 1, 1:] > 0).all()                    # sample 1 has one token: the 25 pad positions too


@pytest.mark.parametrize("layout,N", [("lm", 49), ("cm", 196), ("lm", 196)])
def test_infer_outputs_stay_inside_their_buffers(layout, N):
    """v / q / a_v / a_q carved out of ONE NaN-filled tensor with guard regions between them: every output element is
    written (finite) and no guard element is touched."""
    from vqa_amd import _lib
    lib = _lib.load()
    B, d, T, L = 7, 512, 26, 3
    V, Qs, P, _ = _inputs(B, N, d, 123)
    Vbuf, vstr, Qd, ps = _setup(V, Qs, P, layout)
    G_ = 256                                                    # guard floats (a multiple of 64: outputs stay 256-byte aligned)
    sizes = [L * B * d, L * B * d, L * B * N, L * B * T]
    big = torch.full((G_ + sum(((s + 63) // 64) * 64 + G_ for s in sizes),), float("nan"), device="cuda")
    views, o = [], G_
    for s in sizes:
        views.append(big[o:o + s])
        o += ((s + 63) // 64) * 64 + G_
    outside = torch.ones_like(big, dtype=torch.bool)
    for v in views:
        outside[v.data_ptr() // 4 - big.data_ptr() // 4:][:v.numel()] = False
    for mode in ("exact", "fast16"):
        big.fill_(float("nan"))
        flags = _flags(mode)
        _, fb, _ = _lib.workspace_bytes(B, N, T, d, L, flags)
        ws = torch.full((fb // 4,), float("nan"), device="cuda")
        qptr = (C.c_void_p * L)(*[t.data_ptr() for t in Qd])
        p = _lib.Params(*[t.data_ptr() for t in ps])
        _lib.check(lib.coattn_infer(Vbuf.data_ptr(), *vstr, qptr, C.byref(p), *[v.data_ptr() for v in views],
                                    ws.data_ptr(), B, N, T, d, L, _lib.F32, flags,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), "coattn_infer")
        torch.cuda.synchronize()
        for v in views:
            assert torch.isfinite(v).all(), mode
        assert torch.isnan(big[outside]).all(), mode


def test_infer_range_report_on_the_workspace():
    """Tolerance mode: an image feature beyond 65,504 through coattn_infer -> coattn_status on the WORKSPACE returns -4
    (and 0 for ordinary magnitudes)."""
    from vqa_amd import _lib
    lib = _lib.load()
    B, N, d, T, L = 4, 49, 512, 26, 3
    V, Qs, P, _ = _inputs(B, N, d, 55)
    amax = (C.c_float * 2)()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for big, want in ((None, 0), (2.0e5, -4)):
        Vb = V.clone()
        if big is not None:
            Vb[1, 7, 5] = big
        _, inf, ws = _pair(Vb, Qs, P, "fast16", "lm")
        assert lib.coattn_status(ws.data_ptr(), B, N, T, d, L, _lib.F32, st, amax) == want
        assert torch.isfinite(inf["v"]).all() and torch.isfinite(inf["a_v"]).all()
        if big is not None:
            assert abs(amax[0] - big) < 1.0


def test_module_forward_with_attention():
    import vqa_amd
    B, N, d = 6, 49, 512
    V, Qs, P, _ = _inputs(B, N, d, 77)
    m = vqa_amd.ParallelCoAttention(d)
    m.load_state_dict(P)
    m = m.cuda()
    x = V.cuda().permute(0, 2, 1)                               # the encoder's permuted view
    Qg = [q.cuda() for q in Qs]
    with pytest.raises(RuntimeError):
        m.forward_with_attention(x, Qg)                         # parameters require grad, grad mode on
    for fast in (False, True):
        m.fast_products = fast
        with torch.no_grad():
            v0, q0 = m(x, Qg)
            v1, q1, a_v, a_q = m.forward_with_attention(x, Qg)
        for l in range(3):
            assert torch.equal(v0[l], v1[l]) and torch.equal(q0[l], q1[l])
        assert a_v.shape == (3, B, N) and a_q.shape == (3, B, 26)
    vqa_amd.check_range()
    m.fast_products = False


def _net(K=10, vocab=50):
    from vqa_amd import train as T
    torch.manual_seed(0)
    return T.build_model("attention", vocab, K).cuda()


def test_net_forward_with_attention_logits_bit_for_bit():
    """Given the same encoder outputs, forward_with_attention's logits are model(...)'s bit for bit.  (The stock encoders
    themselves -- MIOpen convolutions, the LSTM -- need not repeat bit for bit from call to call: their outputs are
    computed once here and replayed to both.)"""
    from vqa_amd import train as T
    model = _net()
    model.eval()
    b = T.synthetic_batch(5, (64, 64), 26, 50, 11, seed=3)
    im, qu, la, ln = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])
    im, qu = im.cuda(), qu.cuda()
    with pytest.raises(RuntimeError):
        model.forward_with_attention(im, qu, ln)                 # a gradient would be required
    with torch.no_grad():
        f_img = model.image_encoder(im)
        f_q = model.question_encoder(qu, ln)
    model.image_encoder.forward = lambda x: f_img                # noqa: E731
    model.question_encoder.forward = lambda x, lens: f_q         # noqa: E731
    with torch.no_grad():
        ref = model(im, qu, ln)
        logits, a_v, a_q = model.forward_with_attention(im, qu, ln)
        again = model(im, qu, ln)
    assert torch.equal(ref, again)
    assert torch.equal(ref, logits)
    assert a_v.shape == (3, 5, 4) and a_q.shape == (3, 5, 26)  # 64 px: a 2 x 2 grid
    assert torch.allclose(a_v.sum(-1), torch.ones(3, 5, device="cuda"), atol=1e-5)


def test_predict_attention_matches_validate(tmp_path, capsys):
    from vqa_amd import predict as Pr
    from vqa_amd import train as T
    common = ["--num_cls", "10", "--batch_size", "8", "--image_size", "64", "--vocab_size", "50"]
    ckpt = str(tmp_path / "att.pth")
    T.main(["--model", "attention", "--num_steps", "3", "--log_interval", "3", "--save_path", ckpt] + common)
    capsys.readouterr()
    S = 24
    maps = str(tmp_path / "maps.npz")
    summary = Pr.main(["--model", "attention", "--model_ckpt", ckpt, "--test_size", str(S), "--attention_maps", maps,
                       "--predictions", str(tmp_path / "p.jsonl")] + common)
    z = np.load(maps)
    assert z["a_v"].shape == (S, 3, 2, 2) and z["a_q"].shape == (S, 3, 26)
    assert list(z["index"]) == list(range(S)) and z["ques_len"].min() >= 3
    assert np.allclose(z["a_v"].reshape(S, 3, -1).sum(-1), 1.0, atol=1e-5)
    # Trainer.validate on the same (sorted) batches of the same checkpoint
    args = T.build_parser().parse_args(["--model", "attention"] + common)
    torch.manual_seed(0)
    model, _ = T.model_from_args(args)
    model.load_state_dict(torch.load(ckpt, map_location="cpu"))
    model = model.cuda()
    model.image_encoder.to(memory_format=torch.channels_last)
    tr = T.Trainer(model, 1e-4, torch.device("cuda:0"))
    ds = T.SyntheticVQADataset(S, (64, 64), 26, 50, 11, Pr.TEST_SEED)
    batches = []
    for b in torch.utils.data.DataLoader(ds, 8, shuffle=False):
        im, qu, la, ln = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])
        batches.append((im.cuda().contiguous(memory_format=torch.channels_last), qu.cuda(), ln, la.cuda()))
    m = tr.validate(batches)
    assert summary["samples"] == S
    assert summary["accuracy"] == pytest.approx(m["accuracy"], abs=1e-3)
    assert summary["loss"] == pytest.approx(m["loss"], rel=1e-5)
    recs = [json.loads(l) for l in open(tmp_path / "p.jsonl")]
    assert [r["index"] for r in recs] == list(range(S))
