"""GPU: the soft-answer-target loss and score kernels (csrc/ce.hip: coattn_soft_loss_forward, coattn_vqa_score), the answer
head's soft forward (coattn_head_forward_soft), the hot-path node, the Trainer and predict.py on them -- against the float64
oracle of tests/_soft_loss.py and, for one-hot targets, against the golden-pinned hard-label path.

Bounds: the loss within 2e-6 * max(1, |ref|) and d loss / d logits within 1e-6 absolute -- what test_gpu_loss.py holds the
hard-label kernel to; the head within 1e-4 (test_gpu_head.py), its reduced-precision mode within 2e-2 of max|.|; the hot-path
node within 1e-6 * max|.| + 1e-7 of the per-module path (test_gpu_graph.py).  Every test prints its figures before it asserts."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from oracle import coattn_oracle as O
from tests import _soft_loss as SL

pytestmark = pytest.mark.gpu

SHAPES = [(160, 1001, 10), (160, 3001, 10), (37, 1001, 16), (5, 7, 1), (1, 2, 3), (257, 1001, 10)]
KINDS = ["soft_ce", "bce"]
NAMES = ("W_w.weight", "W_w.bias", "W_p.weight", "W_p.bias", "W_s.weight", "W_s.bias", "W_h.weight", "W_h.bias")


def _logits(B, K, seed, scale):
    return torch.from_numpy(O.hash_normal((B, K), seed, scale)).float()


def _labels(B, K, seed):
    return torch.from_numpy((O.hash_uniform(B, seed) * K).astype("int64")).clamp_(0, K - 1)


def _ws(B, K, fill=float("nan")):
    from vqa_amd import _lib
    n = C.c_size_t()
    assert _lib.load().coattn_ce_workspace_bytes(B, K, _lib.F32, C.byref(n)) == 0
    return torch.full((n.value // 4,), fill, device="cuda")


def _soft_c(z, idx, sc, kind, want_grad=True, ws=None):
    """coattn_soft_loss_forward straight through ctypes: (loss, dlogits or None, ws)."""
    from vqa_amd import _lib
    lib = _lib.load()
    B, K = z.shape
    ws = _ws(B, K) if ws is None else ws
    loss = torch.full((), float("nan"), device="cuda")
    dz = torch.full((B, K), float("nan"), device="cuda") if want_grad else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.coattn_soft_loss_forward(z.data_ptr(), idx.data_ptr(), sc.data_ptr(), idx.shape[1], SL.KINDS[kind], loss.data_ptr(),
                                      dz.data_ptr() if want_grad else None, ws.data_ptr(), B, K, _lib.F32, st)
    assert rc == 0, lib.coattn_last_error()
    return loss, dz, ws


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_K%d_A%d" % s)
def test_loss_kernel_vs_oracle(shape, kind):
    """Both kinds at every shape and at logit scales 0.5, 3 and 30; rows with duplicate indices, empty slots and wholly empty
    rows are in the targets (tests/_soft_loss.make_targets)."""
    B, K, A = shape
    idx, sc = SL.make_targets(B, K, A, seed=21)
    if B >= 7 and A >= 2:
        assert bool((idx == -1).all(1).any()) and bool((idx[:, 0] == idx[:, 1]).any()) and bool((idx == -1).any())
    for scale in (0.5, 3.0, 30.0):
        z = _logits(B, K, 3, scale)
        ref, gref = SL.loss_and_grad(z, idx, sc, kind)
        loss, dz, _ = _soft_c(z.cuda(), idx.cuda(), sc.cuda(), kind)
        e_l = abs(loss.item() - ref.item()) / max(1.0, abs(ref.item()))
        e_g = (dz.double().cpu() - gref).abs().max().item()
        print("soft loss %s B%d K%d A%d scale %g: ref %.6g rel err %.3g, dlogits abs err %.3g" % (kind, B, K, A, scale, ref.item(), e_l, e_g))
        assert e_l < 2e-6 and e_g < 1e-6


@pytest.mark.parametrize("shape", [(160, 1001, 10), (37, 3001, 16), (5, 7, 1), (257, 1001, 3)], ids=lambda s: "B%d_K%d_A%d" % s)
def test_one_hot_targets_anchor_to_the_hard_label_kernel(shape):
    """ans_idx[:, 0] = label with score 1, the other slots empty, SOFT_CE: coattn_ce_forward's loss and gradient within
    1e-6 * max|.| -- and, the expressions being ordered alike, bit for bit."""
    from vqa_amd import _lib
    lib = _lib.load()
    B, K, A = shape
    for scale in (0.5, 3.0, 30.0):
        z = _logits(B, K, 5, scale).cuda()
        lab = _labels(B, K, 6)
        idx, sc = SL.one_hot_targets(lab, A)
        loss, dz, _ = _soft_c(z, idx.cuda(), sc.cuda(), "soft_ce")
        l0 = torch.full((), float("nan"), device="cuda"); d0 = torch.full((B, K), float("nan"), device="cuda")
        labd = lab.cuda()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.coattn_ce_forward(z.data_ptr(), labd.data_ptr(), l0.data_ptr(), d0.data_ptr(), _ws(B, K).data_ptr(), B, K, _lib.F32, st) == 0
        e_l, e_g = abs(loss.item() - l0.item()), (dz - d0).abs().max().item()
        print("anchor B%d K%d A%d scale %g: |dloss| %.3g, max |d dlogits| %.3g, bitwise %s / %s"
              % (B, K, A, scale, e_l, e_g, torch.equal(loss, l0), torch.equal(dz, d0)))
        assert e_l <= 1e-6 * abs(l0.item()) and e_g <= 1e-6 * d0.abs().max().item()
        assert torch.equal(loss, l0) and torch.equal(dz, d0)


@pytest.mark.parametrize("kind", KINDS)
def test_semantics_through_the_python_surface(kind):
    """Upstream gradient scaling, no_grad call, dlogits = NULL, a NaN in an empty slot's score, a logit of 8e4; an index
    of K or -2 in row 3 -> NaN loss, IndexError naming the row at check_labels(), and a clear word after the next good call."""
    from vqa_amd import loss as L
    B, K, A = 37, 1001, 10
    z = _logits(B, K, 3, 3.0).cuda()
    idx, sc = [t.cuda() for t in SL.make_targets(B, K, A, seed=4)]
    ref, gref = SL.loss_and_grad(z, idx, sc, kind, upstream=2.5)
    zg = z.clone().requires_grad_(True)
    out = L.soft_target_loss(zg, idx, sc, kind)
    (2.5 * out).backward()
    print("semantics %s: loss %.6g ref %.6g, grad err %.3g" % (kind, out.item(), ref.item(), (zg.grad.double().cpu() - gref).abs().max().item()))
    assert abs(out.item() - ref.item()) < 2e-6 * max(1.0, abs(ref.item()))
    assert (zg.grad.double().cpu() - gref).abs().max() < 1e-6
    with torch.no_grad():
        l0 = L.soft_target_loss(z, idx, sc, kind)
    assert torch.equal(l0, out.detach())
    l1, none, _ = _soft_c(z, idx, sc, kind, want_grad=False)           # dlogits = NULL
    assert none is None and torch.equal(l1, l0)
    assert torch.equal(L.SoftTargetLoss(kind)(z, idx, sc), l0)
    sc_nan = sc.clone()
    sc_nan[idx < 0] = float("nan")
    l2, d2, _ = _soft_c(z, idx, sc_nan, kind)
    _, d1, _ = _soft_c(z, idx, sc, kind)
    assert torch.equal(l2, l0) and torch.equal(d2, d1)
    L.check_labels()
    for bad_index in (K, -2):
        bad = idx.clone()
        bad[3, 2] = bad_index
        assert torch.isnan(L.soft_target_loss(z, bad, sc, kind))       # asynchronous: NaN now, the error at the next check
        with pytest.raises(IndexError, match="row 3"):
            L.check_labels()
        L.soft_target_loss(z, idx, sc, kind)
        L.check_labels()                                               # the word is cleared by every call
    z2 = z.clone()
    z2[0, 5] = 8.0e4
    big = L.soft_target_loss(z2, idx, sc, kind)
    print("semantics %s: loss with a logit of 8e4: %.6g" % (kind, big.item()))
    assert torch.isfinite(big)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", [1, 2, 63, 160, 257, 1000])
def test_one_launch_and_order_independence(B, kind):
    """The mean is added by whichever workgroup takes the last ticket: 20 repeated calls are bitwise equal, the ticket and
    status words are 0 afterwards, and the workspace may start NaN-filled."""
    from vqa_amd import _lib
    K, A = 1001, 10
    z = _logits(B, K, 11, 2.0).cuda()
    idx, sc = [t.cuda() for t in SL.make_targets(B, K, A, seed=12)]
    ref, _ = SL.loss_and_grad(z, idx, sc, kind)
    ws = _ws(B, K)
    first, d_first, _ = _soft_c(z, idx, sc, kind, ws=ws)
    print("order %s B%d: loss %.7g ref %.7g" % (kind, B, first.item(), ref.item()))
    assert abs(first.item() - ref.item()) < 2e-6 * max(1.0, abs(ref.item()))
    for _ in range(20):
        again, d_again, _ = _soft_c(z, idx, sc, kind, ws=ws)
        assert torch.equal(again, first) and torch.equal(d_again, d_first)
    words = ws.view(torch.int32)[(B + 63) // 64 * 64:][:2].tolist()
    assert words == [0, 0], words
    assert _lib.load().coattn_ce_status(ws.data_ptr(), B, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_K%d_A%d" % s)
def test_score_kernel(shape):
    """pred = numpy.argmax of the float32 logits (a constructed tie and a row of equal logits included), row_score the oracle's
    selection exactly, the sum within 2e-6 relative; row_score = NULL gives the same sum."""
    from vqa_amd import _lib
    from vqa_amd import loss as L
    lib = _lib.load()
    B, K, A = shape
    z = _logits(B, K, 7, 3.0)
    lab = _labels(B, K, 8)
    idx, sc = SL.make_targets(B, K, A, seed=9, label=lab if A > 1 else None)
    z[torch.arange(0, B, 2), lab[::2]] += 20.0                         # every second row predicts its slot-0 answer
    z[0, :] = 0.25                                                     # a row of equal logits: index 0
    if B > 2 and K > 5:
        z[2, 1] = z[2, 4] = z[2].max() + 1.0                           # a tie: the lower index
    p_ref, r_ref, m_ref = SL.score(z, idx, sc)
    pred, rows, mean = L.vqa_score(z.cuda(), idx.cuda(), sc.cuda())
    assert pred.dtype == torch.int32 and pred.cpu().tolist() == p_ref.tolist() and int(pred[0]) == 0
    if B > 2 and K > 5:
        assert int(pred[2]) == 1
    total = float(mean) * B
    print("score B%d K%d A%d: sum %.7g ref %.7g" % (B, K, A, total, float(r_ref.sum())))
    assert torch.equal(rows.cpu(), r_ref.float())
    assert abs(total - float(r_ref.sum())) <= 2e-6 * max(1.0, float(r_ref.sum()))
    ws = _ws(B, K)
    zc, ic, scc = z.cuda(), idx.cuda(), sc.cuda()
    p2 = torch.empty(B, dtype=torch.int32, device="cuda"); tot2 = torch.full((), float("nan"), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(3):
        assert lib.coattn_vqa_score(zc.data_ptr(), ic.data_ptr(), scc.data_ptr(), A, p2.data_ptr(), None, tot2.data_ptr(),
                                    ws.data_ptr(), B, K, _lib.F32, st) == 0
        assert torch.equal(p2, pred) and torch.equal(tot2 / B, mean)
    assert ws.view(torch.int32)[(B + 63) // 64 * 64:][:2].tolist() == [0, 0]


# ---- the answer head ----------------------------------------------------------------------------------------------------
def _rel(a, b):
    return ((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _head_case(B, d, mlp, K, seed=0):
    torch.manual_seed(1000 + B + d + seed)
    ref = O.OracleMLPClassifier(d, mlp, K).double()
    v = torch.from_numpy(O.hash_normal((3, B, d), 11 + seed, 1.0))
    q = torch.from_numpy(O.hash_normal((3, B, d), 12 + seed, 0.5))
    return ref, v, q


def _head_oracle(ref, v, q, idx, sc, kind, g_loss):
    vr, qr = v.clone().requires_grad_(True), q.clone().requires_grad_(True)
    for p in ref.parameters():
        p.grad = None
    z = ref([vr[l] for l in range(3)], [qr[l] for l in range(3)])
    loss = SL.loss(z, idx, sc, kind)
    (g_loss * loss).backward()
    return z.detach(), loss.detach(), vr.grad, qr.grad, {k: p.grad.clone() for k, p in ref.named_parameters()}


def _head_call(v, q, P, g_loss, labels=None, targets=None, kind="soft_ce", flags=0):
    """coattn_head_forward (labels) or coattn_head_forward_soft (targets), then coattn_head_backward, through ctypes."""
    from vqa_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    v, q = v.float().to(dev).contiguous(), q.float().to(dev).contiguous()
    ps = [P[k].float().to(dev).contiguous() for k in NAMES]
    _, B, d = v.shape
    mlp, K = ps[4].shape[0], ps[6].shape[0]
    sb, wb = C.c_size_t(), C.c_size_t()
    _lib.check(lib.coattn_head_workspace_bytes(B, d, mlp, K, _lib.F32, C.byref(sb), C.byref(wb)), "ws")
    saved = torch.full((sb.value // 4,), float("nan"), device=dev)
    logits = torch.full((B, K), float("nan"), device=dev)
    loss = torch.full((), float("nan"), device=dev)
    rows = lambda t: (C.c_void_p * 3)(*[t[l].data_ptr() for l in range(3)])   # noqa: E731
    p = _lib.HeadParams(*[t.data_ptr() for t in ps])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if targets is not None:
        idx, sc = [t.to(dev).contiguous() for t in targets]
        _lib.check(lib.coattn_head_forward_soft(rows(v), rows(q), C.byref(p), idx.data_ptr(), sc.data_ptr(), idx.shape[1],
                                                SL.KINDS[kind], logits.data_ptr(), loss.data_ptr(), saved.data_ptr(),
                                                B, d, mlp, K, _lib.F32, flags, st), "coattn_head_forward_soft")
    else:
        lab = labels.to(dev)
        _lib.check(lib.coattn_head_forward(rows(v), rows(q), C.byref(p), lab.data_ptr(), logits.data_ptr(), loss.data_ptr(),
                                           saved.data_ptr(), B, d, mlp, K, _lib.F32, flags, st), "coattn_head_forward")
    assert lib.coattn_head_status(saved.data_ptr(), B, d, mlp, K, st) == 0
    ws = torch.full((wb.value // 4,), float("nan"), device=dev)
    dv, dq = torch.full_like(v, float("nan")), torch.full_like(q, float("nan"))
    grads = [torch.full_like(t, float("nan")) for t in ps]
    pg = _lib.HeadParamGrads(*[t.data_ptr() for t in grads])
    gl = torch.tensor([g_loss], device=dev, dtype=torch.float32)
    _lib.check(lib.coattn_head_backward(rows(v), rows(q), C.byref(p), saved.data_ptr(), gl.data_ptr(), None, rows(dv), rows(dq),
                                        C.byref(pg), 0, ws.data_ptr(), B, d, mlp, K, _lib.F32, flags, st), "coattn_head_backward")
    torch.cuda.synchronize()
    out = {"logits": logits, "loss": loss, "dv": dv, "dq": dq}
    out.update({"d" + k: g for k, g in zip(NAMES, grads)})
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(160, 512, 1024, 1001), (5, 64, 96, 7), (3, 20, 12, 5)], ids=lambda s: "B%d_d%d_mlp%d_K%d" % s)
def test_head_soft_vs_oracle(shape, kind):
    """coattn_head_forward_soft + coattn_head_backward: logits, loss and all ten gradients against the float64 oracle within
    1e-4 (the loss relative to max(1, |ref|): the BCE loss is of order K), the logits bit for bit coattn_head_forward's, in the
    per-layer and the one-launch form; the reduced-precision flag within test_gpu_head.py's bf16 bound."""
    from vqa_amd import _lib
    B, d, mlp, K = shape
    ref, v, q = _head_case(B, d, mlp, K)
    lab = _labels(B, K, 13)
    idx, sc = SL.make_targets(B, K, 10, seed=14, label=lab)
    z, loss, gv, gq, gp = _head_oracle(ref, v, q, idx, sc, kind, 1.7)
    P = ref.state_dict()
    hard = _head_call(v, q, P, 1.7, labels=lab)
    for flags in (0, 1):
        r = _head_call(v, q, P, 1.7, targets=(idx, sc), kind=kind, flags=flags)
        e_l = abs(r["loss"].item() - loss.item()) / max(1.0, abs(loss.item()))
        errs = {"dv": _rel(r["dv"], gv), "dq": _rel(r["dq"], gq), **{k: _rel(r["d" + k], gp[k]) for k in NAMES}}
        print("head %s %s flags %d: logits err %.3g loss %.6g rel err %.3g grads %.3g"
              % (kind, shape, flags, (r["logits"].double().cpu() - z).abs().max().item(), loss.item(), e_l, max(errs.values())))
        assert (r["logits"].double().cpu() - z).abs().max() < 1e-4 and e_l < 1e-4
        assert all(e < 1e-4 for e in errs.values()), errs
        assert torch.equal(r["logits"], hard["logits"]) and torch.equal(r["dv"], r["dq"])
    b = _head_call(v, q, P, 1.7, targets=(idx, sc), kind=kind, flags=_lib.FLAG_BF16_PROJ)
    hard_b = _head_call(v, q, P, 1.7, labels=lab, flags=_lib.FLAG_BF16_PROJ)
    assert torch.equal(b["logits"], hard_b["logits"])
    errs = {"logits": _rel(b["logits"], z), "dv": _rel(b["dv"], gv), **{k: _rel(b["d" + k], gp[k]) for k in NAMES}}
    print("head %s %s bf16: loss rel err %.3g, worst %.3g" % (kind, shape, abs(b["loss"].item() - loss.item()) / max(1.0, abs(loss.item())), max(errs.values())))
    assert abs(b["loss"].item() - loss.item()) <= 2e-2 * max(1.0, abs(loss.item()))
    assert all(e < 2e-2 for e in errs.values()), errs


@pytest.mark.parametrize("shape", [(160, 512, 1024, 1001), (5, 64, 96, 7), (3, 20, 12, 5)], ids=lambda s: "B%d_d%d_mlp%d_K%d" % s)
def test_head_one_hot_targets_equal_the_hard_label_head(shape):
    B, d, mlp, K = shape
    ref, v, q = _head_case(B, d, mlp, K, seed=1)
    lab = _labels(B, K, 15)
    P = ref.state_dict()
    hard = _head_call(v, q, P, 1.3, labels=lab)
    soft = _head_call(v, q, P, 1.3, targets=SL.one_hot_targets(lab, 10), kind="soft_ce")
    for k in hard:
        e = (hard[k] - soft[k]).abs().max().item()
        print("head anchor %s %s: max diff %.3g of %.3g" % (shape, k, e, hard[k].abs().max().item()))
        assert e <= 1e-6 * hard[k].abs().max().item(), k


def test_head_bad_index_raises_at_check_labels():
    from vqa_amd import head as H
    from vqa_amd.modules import MLPClassifier
    torch.manual_seed(0)
    B, d, mlp, K = 6, 32, 32, 9
    mod = MLPClassifier(d, mlp, K).cuda()
    v, q = torch.randn(3, B, d, device="cuda"), torch.randn(3, B, d, device="cuda")
    idx, sc = [t.cuda() for t in SL.make_targets(B, K, 4, seed=2)]
    bad = idx.clone()
    bad[3, 1] = K
    _, loss = mod.forward_loss(v, q, targets=(bad, sc), loss_kind="bce")
    assert torch.isnan(loss)
    with pytest.raises(IndexError, match="row 3"):
        H.check_labels()
    _, loss = mod.forward_loss(v, q, targets=(idx, sc), loss_kind="bce")
    H.check_labels()
    assert torch.isfinite(loss)


# ---- the hot-path node ---------------------------------------------------------------------------------------------------
def _modules(d, mlp, K, seed=0, **kw):
    import vqa_amd
    from vqa_amd.modules import MLPClassifier
    torch.manual_seed(seed)
    return vqa_amd.ParallelCoAttention(d, **kw).cuda(), MLPClassifier(d, mlp, K).cuda()


@pytest.mark.parametrize("variant", ["plain", "question_mask", "bilinear"])
@pytest.mark.parametrize("capture", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("kind", KINDS)
def test_hot_path_node_matches_the_module_path(kind, capture, variant):
    """HotPathGraph(loss=kind) against co(x, Qs) -> head.forward_loss(targets=...), (3 * loss).backward(): the loss bit for
    bit, every gradient within 1e-6 * max|.| + 1e-7; a second step with new targets AT THE SAME ADDRESSES gives that step's
    values (the buffers are read, not baked in)."""
    from vqa_amd.graph import HotPathGraph
    B, N, T, d, mlp, K, A = 12, 49, 26, 256, 128, 19, 10
    co, head = _modules(d, mlp, K, seed=3)
    lens = None
    if variant == "question_mask":
        co.question_mask = True
        lens = torch.tensor([26, 20, 14, 9, 7, 5, 4, 3, 3, 2, 1, 1])
    if variant == "bilinear":
        co.affinity = "bilinear"
    x = torch.randn(B, N, d, device="cuda").clamp_min_(0)
    Qs = [(torch.randn(B, T, d, device="cuda") * 0.2).requires_grad_(True) for _ in range(3)]
    idx, sc = [t.cuda() for t in SL.make_targets(B, K, A, seed=31)]
    idx_b, sc_b = [t.cuda() for t in SL.make_targets(B, K, A, seed=47)]
    params = list(co.parameters()) + list(head.parameters())
    hp = HotPathGraph(co, head, B, N, T, capture=capture, question_mask=variant == "question_mask", loss=kind, num_answers=A)

    def grads():
        return [q.grad.clone() for q in Qs] + [p.grad.clone() for p in params if p.grad is not None]

    def clear():
        for t in Qs + params:
            t.grad = None

    def modules_step():
        clear()
        vq = co(x, Qs, lens) if lens is not None else co(x, Qs)
        _, loss = head.forward_loss(*vq, targets=(idx, sc), loss_kind=kind)
        (loss * 3.0).backward()
        return loss.detach().clone(), grads()

    def node_step():
        clear()
        _, loss = hp(x, Qs, (idx, sc), q_len=lens)
        (loss * 3.0).backward()
        return loss.detach().clone(), grads()

    for step in range(2):
        lref, gref = modules_step()
        lnode, gnode = node_step()
        worst = max(((a - b).abs().max().item() / max(a.abs().max().item(), 1e-30)) for a, b in zip(gref, gnode))
        print("hot path %s %s %s step %d: loss %.7g / %.7g, worst gradient diff %.3g of max" % (kind, capture, variant, step, lnode.item(), lref.item(), worst))
        assert torch.equal(lnode, lref) and len(gref) == len(gnode)
        for a, b in zip(gref, gnode):
            assert (a - b).abs().max() <= 1e-6 * a.abs().max().item() + 1e-7
        if step == 0:
            first = lref
            idx.copy_(idx_b); sc.copy_(sc_b)                       # new targets, same addresses
    assert not torch.equal(first, lref)
    if capture:
        assert len(hp._pairs) == 2                                 # the static set of the warm-up + the caller's addresses
    # targets in another dtype go through the static buffers (copy_ converts): same loss
    _, l64 = hp(x, [q.detach() for q in Qs], (idx.long(), sc.double()), q_len=lens)
    assert torch.equal(l64, lref)
    with pytest.raises(RuntimeError, match="targets"):
        hp(x, Qs, torch.zeros(B, dtype=torch.int64, device="cuda"), q_len=lens)


@pytest.mark.parametrize("kind", KINDS)
def test_alternating_form_takes_targets_on_the_module_path(kind):
    """forward_features(..., targets=...) of the alternating model: the loss against the float64 oracle on the model's own
    logits, and the same loss with return_attention=True."""
    from vqa_amd import train as T
    torch.manual_seed(0)
    net = T.build_model("attention", 60, 12, co_attention="alternating").cuda()
    net.hot_path_static = True                                     # (ignored: the node is parallel-only)
    B, K, A = 4, 13, 5
    b = T.synthetic_batch(B, (64, 64), 10, 60, K, seed=2, num_answers=A)
    im, qu, la, ln, ai, sc = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"], b["answers"], b["answer_scores"])
    tg = (ai.cuda(), sc.cuda())
    feats = net.image_encoder(im.cuda()).detach()
    logits, loss = net.forward_features(feats, qu.cuda(), ln, targets=tg, loss_kind=kind)
    ref = SL.loss(logits.detach().double().cpu(), ai, sc, kind)
    print("alternating %s: loss %.7g ref %.7g" % (kind, loss.item(), ref.item()))
    assert abs(loss.item() - ref.item()) <= 2e-6 * max(1.0, abs(ref.item()))
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.mlp_classify.parameters())
    out = net.forward_features(feats, qu.cuda(), ln, targets=tg, loss_kind=kind, return_attention=True)
    assert len(out) == 4 and torch.equal(out[1], loss)


# ---- Trainer and predict.py -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_trainer_reduces_the_loss_and_validates_with_the_vqa_score(kind):
    from vqa_amd import train as T
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    K, A = 11, 10
    model = T.build_model("attention", 100, K - 1).to(dev)
    tr = T.Trainer(model, 1e-4, dev, loss=kind)        # (the reference's and the Trainer's default rate, main.py:58)
    b = T.synthetic_batch(8, (64, 64), 26, 100, K, seed=1, num_answers=A)
    im, qu, la, ln, ai, sc = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"], b["answers"], b["answer_scores"])
    im, qu, la, ai, sc = [t.to(dev) for t in (im, qu, la, ai, sc)]
    losses = [float(tr.step(im, qu, ln, la, next_image=im, targets=(ai, sc))) for _ in range(5)]
    tr.check_labels()
    print("trainer %s: losses %s" % (kind, ["%.5f" % l for l in losses]))
    assert model.hot_path_static and len(model._graphs) == 1 and all(l == l for l in losses)
    assert losses[-1] < losses[0]
    batches = [(im, qu, ln, la, ai, sc), (im[:4], qu[:4], ln[:4], la[:4], ai[:4], sc[:4])]
    m = tr.validate(batches)
    model.eval()
    with torch.no_grad():
        rows = torch.cat([SL.score(model(bi[0], bi[1], bi[2]).float(), bi[4], bi[5])[1] for bi in batches])
    model.train()
    print("trainer %s: vqa_score %.7f oracle %.7f accuracy %.3f" % (kind, m["vqa_score"], float(rows.mean()), m["accuracy"]))
    assert abs(m["vqa_score"] - float(rows.mean())) <= 1e-6
    oh = [bi[:4] + tuple(t.to(dev) for t in SL.one_hot_targets(bi[3], A)) for bi in batches]
    m1 = tr.validate(oh)
    assert abs(m1["vqa_score"] * 100.0 - m1["accuracy"]) <= 1e-4
    # a bad index in row 3 surfaces at the trainer's check
    bad = ai.clone()
    bad[3, 1] = K
    assert torch.isnan(tr.step(im, qu, ln, la, targets=(bad, sc)).detach())
    with pytest.raises(IndexError, match="row 3"):
        tr.check_labels()


def test_predict_end_to_end_writes_score_and_vqa_score(tmp_path, capsys):
    from vqa_amd import predict as Pr
    from vqa_amd import train as T
    common = ["--model", "attention", "--num_cls", "6", "--batch_size", "4", "--image_size", "64", "--vocab_size", "50",
              "--max_seq_length", "8", "--loss", "bce", "--num_answers", "5"]
    ckpt = str(tmp_path / "m.pth")
    T.main(["--num_steps", "2", "--log_interval", "1", "--save_path", ckpt] + common)
    capsys.readouterr()
    preds = str(tmp_path / "p.jsonl")
    S = 10
    summary = Pr.main(["--model_ckpt", ckpt, "--test_size", str(S), "--topk", "3", "--predictions", preds] + common)
    recs = [json.loads(l) for l in open(preds)]
    assert len(recs) == S and all(0.0 <= r["score"] <= 1.0 and all(0.0 < p < 1.0 for p in r["prob"]) for r in recs)
    assert summary["vqa_score"] == pytest.approx(sum(r["score"] for r in recs) / S, abs=1e-5)
    ds = T.SyntheticVQADataset(S, (64, 64), 8, 50, 7, Pr.TEST_SEED, num_answers=5)
    for i, r in enumerate(recs):
        t = SL.dense(ds[i]["answers"][None], ds[i]["answer_scores"][None], 7)[0]
        assert r["score"] == pytest.approx(min(1.0, float(t[r["top"][0]])), abs=1e-6)
