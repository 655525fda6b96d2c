"""The alternating co-attention (include/coattn.h v0.11.0) on the GPU: C-ABI outputs, maps and every gradient against the
float64 oracle of tests/_alternating.py, on the general-shape path (small odd shapes) and the tuned kernels (config 2 at
N = 49 and 196), both feature layouts, masked and unmasked, with and without map gradients; the identities it keeps
(inference, repeatability, pad rows); the refusals; and the module / Trainer / predict surface."""
import numpy as np
import pytest
import torch

import vqa_amd
from vqa_amd import _lib

from tests import _alternating as AL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAMES = AL.NAMES
TOL = AL.TOL
case, run, rel, check, ABS = AL.case, AL.run, AL.rel, AL.check, AL.ABS

SMALL = [(4, 7, 5, 64), (3, 7, 5, 96), (1, 7, 5, 64)]


@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("layout", ["lm", "cm"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("maps", [False, True])
def test_small_shapes_match_oracle(shape, layout, masked, maps):
    B, N, T, d = shape
    V, Qs, P, gv, gq = case(B, N, T, d, seed=B + d)
    lens = [max(1, T - 2 * i) for i in range(B)] if masked else None
    g = torch.Generator().manual_seed(7)
    g_av = torch.randn(3, B, N, generator=g, dtype=torch.float64) if maps else None
    g_aq = torch.randn(3, B, T, generator=g, dtype=torch.float64) if maps else None
    ref = AL.forward_backward(V, Qs, P, gv, gq, g_av, g_aq, lens)
    out = run(V, Qs, P, gv, gq, layout=layout, lens=lens, g_av=g_av, g_aq=g_aq)
    check(out, ref)
    if masked:
        for b, n in enumerate(lens):
            assert (out["a_q"][:, b, n:] == 0).all()
            assert (out["dQ"][:, b, n:] == 0).all()


@pytest.mark.parametrize("N", [49, 196])
@pytest.mark.parametrize("layout", ["lm", "cm"])
def test_config2_matches_oracle(N, layout):
    B, T, d = 160, 26, 512
    V, Qs, P, gv, gq = case(B, N, T, d, seed=N)
    lens = [1 + (7 * b) % T for b in range(B)]
    g = torch.Generator().manual_seed(9)
    g_aq = torch.randn(3, B, T, generator=g, dtype=torch.float64)
    ref = AL.forward_backward(V, Qs, P, gv, gq, None, g_aq, lens)
    out = run(V, Qs, P, gv, gq, layout=layout, lens=lens, g_aq=g_aq)
    check(out, ref)


def test_config2_unmasked_maps_no_dv():
    B, N, T, d = 160, 49, 26, 512
    V, Qs, P, gv, gq = case(B, N, T, d, seed=5)
    g = torch.Generator().manual_seed(11)
    g_av = torch.randn(3, B, N, generator=g, dtype=torch.float64)
    ref = AL.forward_backward(V, Qs, P, gv, gq, g_av, None)
    out = run(V, Qs, P, gv, gq, g_av=g_av, need_dv=False)
    assert out["dV"] is None
    check(out, ref)


@pytest.mark.parametrize("shape", [(3, 7, 5, 64), (160, 49, 26, 512)])
def test_accumulate_adds_into_parameter_gradients(shape):
    B, N, T, d = shape
    V, Qs, P, gv, gq = case(B, N, T, d, seed=13)
    ref = AL.forward_backward(V, Qs, P, gv, gq)
    init = [torch.randn(P[n].shape, generator=torch.Generator().manual_seed(i), dtype=torch.float64) for i, n in enumerate(NAMES)]
    out = run(V, Qs, P, gv, gq, accumulate=1, grads_init=init)
    for i, n in enumerate(NAMES):
        ref["d" + n] = ref["d" + n] + init[i]
    check(out, ref)


@pytest.mark.parametrize("shape", [(4, 7, 5, 96), (160, 196, 26, 512)])
@pytest.mark.parametrize("masked", [False, True])
def test_inference_is_bit_identical(shape, masked):
    B, N, T, d = shape
    V, Qs, P, _, _ = case(B, N, T, d, seed=17)
    lens = [1 + (5 * b) % T for b in range(B)] if masked else None
    a = run(V, Qs, P, lens=lens)
    b = run(V, Qs, P, lens=lens, infer=True)
    for k in ("v", "q", "a_v", "a_q"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("layout", ["lm", "cm"])
def test_two_runs_are_bitwise_identical(layout):
    B, N, T, d = 640, 49, 26, 512
    V, Qs, P, gv, gq = case(B, N, T, d, seed=19)
    lens = [1 + (3 * b) % T for b in range(B)]
    a = run(V, Qs, P, gv, gq, layout=layout, lens=lens)
    b = run(V, Qs, P, gv, gq, layout=layout, lens=lens)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("shape", [(4, 7, 5, 64), (160, 49, 26, 512)])
def test_pad_rows_change_no_output_bit(shape):
    B, N, T, d = shape
    V, Qs, P, gv, gq = case(B, N, T, d, seed=23)
    lens = [1 + (3 * b) % T for b in range(B)]
    g = torch.Generator().manual_seed(29)
    g_aq = torch.randn(3, B, T, generator=g, dtype=torch.float64)
    Q0 = [q.clone() for q in Qs]
    Q1 = [q.clone() for q in Qs]
    for q in Q0 + Q1:
        for b, n in enumerate(lens):
            q[b, n:] = 0
    for q in Q1:
        for b, n in enumerate(lens):
            q[b, n:] = torch.randn(T - n, d, generator=g, dtype=torch.float64) * 3
    g_aq1 = g_aq.clone()
    for b, n in enumerate(lens):
        g_aq1[:, b, n:] = float("nan")          # read as 0 past the length
    a = run(V, Q0, P, gv, gq, lens=lens, g_aq=g_aq)
    b = run(V, Q1, P, gv, gq, lens=lens, g_aq=g_aq1)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("flags", [_lib.FLAG_FAST16, _lib.FLAG_BF16_PROJ, _lib.FLAG_BILINEAR, _lib.IMPL_GENERAL])
def test_flags_are_refused(flags):
    V, Qs, P, _, _ = case(2, 7, 5, 64)
    run(V, Qs, P, flags=flags, expect_rc=True)
    assert b"flags" in _lib.load().coattn_last_error()


def test_module_matches_oracle_and_surface():
    B, N, T, d = 3, 7, 5, 64
    V, Qs, P, gv, gq = case(B, N, T, d, seed=31)
    mod = vqa_amd.AlternatingCoAttention(d, question_mask=True)
    mod.load_state_dict({AL.state_key(n): P[n].float().reshape(mod.state_dict()[AL.state_key(n)].shape) for n in NAMES})
    mod = mod.to(DEV)
    lens = [5, 2, 1]
    ref = AL.forward_backward(V, Qs, P, gv, gq, lens=lens)
    x = V.float().to(DEV).requires_grad_(True)
    Qd = [q.float().to(DEV).requires_grad_(True) for q in Qs]
    vs, qs, a_v, a_q = mod(x, Qd, lens, return_attention=True)
    (sum((vs[l] * gv[l].float().to(DEV)).sum() + (qs[l] * gq[l].float().to(DEV)).sum() for l in range(3))).backward()
    assert rel(torch.stack(vs).cpu(), ref["v"]) <= TOL and rel(torch.stack(qs).cpu(), ref["q"]) <= TOL
    assert rel(a_q.detach().cpu(), ref["a_q"]) <= TOL
    assert rel(x.grad.cpu(), ref["dV"]) <= TOL
    assert rel(torch.stack([q.grad for q in Qd]).cpu(), torch.stack(ref["dQ"])) <= TOL
    for n in NAMES:
        p_ = mod.state_dict(keep_vars=True)[AL.state_key(n)]
        assert rel(p_.grad.cpu().reshape(-1), ref["d" + n].reshape(-1), 1.0 if "d" + n in ABS else 1e-30) <= TOL, n
    with torch.no_grad():
        v2, q2, av2, aq2 = mod.forward_with_attention(x, Qd, lens)
    assert torch.equal(torch.stack(v2), torch.stack(vs).detach()) and torch.equal(aq2, a_q.detach())
    mod.fast_products = True
    with pytest.raises(RuntimeError):
        mod(x, Qd, lens)


def test_trainer_loss_falls_and_predict_writes_maps(tmp_path):
    from vqa_amd import train as T
    torch.manual_seed(0)
    model = T.build_model("attention", 100, 10, co_attention="alternating").to(DEV)
    assert type(model.co_attention).__name__ == "AlternatingCoAttention"
    tr = T.Trainer(model, 1e-3, DEV)
    b = T.synthetic_batch(8, (64, 64), 26, 100, 11, seed=1)
    im, qu, la, ln = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])
    losses = [float(tr.step(im.to(DEV), qu.to(DEV), ln, la.to(DEV))) for _ in range(6)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert not model._graphs                  # the hot-path node was never built
    ckpt = str(tmp_path / "alt.pth")
    torch.save(model.state_dict(), ckpt)
    from vqa_amd import predict as Pr
    S = 16
    maps = str(tmp_path / "maps.npz")
    summary = Pr.main(["--model", "attention", "--co_attention", "alternating", "--model_ckpt", ckpt, "--test_size", str(S),
                       "--attention_maps", maps, "--predictions", str(tmp_path / "p.jsonl"), "--num_cls", "10",
                       "--batch_size", "8", "--image_size", "64", "--vocab_size", "100"])
    assert summary["samples"] == S
    z = np.load(maps)
    av, aq = z["a_v"], z["a_q"]
    assert av.shape == (S, 3, 2, 2) and aq.shape == (S, 3, 26)
    assert np.allclose(av.reshape(S, 3, -1).sum(-1), 1, atol=1e-5)
    assert np.allclose(aq.sum(-1), 1, atol=1e-5)
