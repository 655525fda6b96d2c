"""GPU: feature dropout (csrc/dropout.hip, include/coattn.h v0.19.0) -- the C-ABI against the numpy oracle of tests/_dropout.py
bit for bit at every size, probability, alignment and form; the device-side step counter; the backward; the autograd function;
the three routes of the network (per-module, eager node, captured node) against each other and against the existing head on the
oracle's mask; the trainer.  Every (seed, step, n, p) comes from tests/_dropout.py (tests/test_dropout_cpu.py checks the
oracle's own keep fractions on them)."""
import copy

import numpy as np
import pytest
import torch

from tests import _dropout as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _x(n, k=0):
    return D.special_values(n, k)


# ---- the C-ABI against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", D.PS)
def test_forward_is_the_oracle_at_every_size(p):
    """One pair, out of place, 16-byte aligned (the vector form where a block is whole, the tail per element); inputs with NaN,
    +-inf, -0 and denormals.  Mask 1 of seed SEED."""
    for n in D.SIZES:
        st = D.State(D.SEED, 0)
        x = _x(n)
        y, _ = D.forward(x, p, st)
        assert D.same_bits(y, D.apply(x, D.SEED, 1, p)), (n, p)
        if p == 0.0:
            assert D.same_bits(y, x), n
        assert st.step() == 1
        st.check(D.SEED)


@pytest.mark.parametrize("n", (5, D.WG + 1, 3 * D.WG + 5))
def test_pairs_in_place_and_every_single_shift_give_the_aligned_bits(n):
    p = 0.5
    x0, x1 = _x(n, 1), _x(n, 2)
    want0, want1 = D.apply(x0, D.SEED, 1, p), D.apply(x1, D.SEED, 1, p)
    assert not D.same_bits(want0, want1)

    def run(**kw):
        st = D.State(D.SEED, 0)
        out = D.forward(x0, p, st, **kw)
        st.check(D.SEED)
        assert st.step() == 1
        return out

    y0, y1 = run(x1=x1)                                          # two pairs, one mask
    assert D.same_bits(y0, want0) and D.same_bits(y1, want1)
    y0, y1 = run(x1=x1, inplace=True)
    assert D.same_bits(y0, want0) and D.same_bits(y1, want1)
    y0, _ = run(inplace=True)
    assert D.same_bits(y0, want0)
    for which in range(4):                                       # x0, y0, x1, y1 alone off the 16-byte boundary
        for shift in (4, 8, 12):
            shifts = tuple(shift if k == which else 0 for k in range(4))
            y0, y1 = run(x1=x1, shifts=shifts)
            assert D.same_bits(y0, want0) and D.same_bits(y1, want1), (which, shift)
    for shift in (4, 8, 12):                                     # one pair; and in place at a shifted address
        y0, _ = run(shifts=(shift, 0, 0, 0))
        assert D.same_bits(y0, want0)
        y0, _ = run(shifts=(0, shift, 0, 0))
        assert D.same_bits(y0, want0)
        y0, _ = run(shifts=(shift, 0, 0, 0), inplace=True)
        assert D.same_bits(y0, want0)


def test_every_probability_on_two_pairs_in_place():
    n = D.WG + 1
    x0, x1 = _x(n, 3), _x(n, 4)
    for p in D.PS:
        st = D.State(D.SEED, 0)
        y0, y1 = D.forward(x0, p, st, x1=x1, inplace=True)
        assert D.same_bits(y0, D.apply(x0, D.SEED, 1, p)) and D.same_bits(y1, D.apply(x1, D.SEED, 1, p)), p


# ---- the state --------------------------------------------------------------------------------------------------------------
def test_step_advances_once_per_forward_and_the_backward_sees_the_forward_mask():
    n, p, s, seed = D.STATE_N, 0.5, D.STATE_STEP, D.SEED_HI
    x, g = _x(n, 5), _x(n, 6)
    st = D.State(seed, s)
    for k in (1, 2, 3):
        y, _ = D.forward(x, p, st)
        assert st.step() == s + k
        assert D.same_bits(y, D.apply(x, seed, s + k, p)), k
        st.check(seed)
    assert not np.array_equal(D.keep(n, seed, s + 1, p), D.keep(n, seed, s + 2, p))
    y, _ = D.forward(x, p, st, advance=0)                        # redraws the current mask
    assert st.step() == s + 3 and D.same_bits(y, D.apply(x, seed, s + 3, p))
    for _ in range(2):                                           # any number of backwards: the same mask, no advance
        dx = D.backward(g, p, st)
        assert D.same_bits(dx, D.apply(g, seed, s + 3, p)) and st.step() == s + 3
    dx = D.backward(g, p, st, inplace=True)
    assert D.same_bits(dx, D.apply(g, seed, s + 3, p))
    for shifts in ((4, 0), (0, 8), (12, 12)):
        assert D.same_bits(D.backward(g, p, st, shifts=shifts), D.apply(g, seed, s + 3, p)), shifts
    st.check(seed)


def test_the_step_carries_into_its_high_word():
    n, p, seed = D.STATE_N, 0.5, D.SEED_HI
    x = _x(n, 7)
    st = D.State(seed, 2 ** 32 - 1)
    y, _ = D.forward(x, p, st)
    assert st.step() == 2 ** 32
    assert D.same_bits(y, D.apply(x, seed, 2 ** 32, p))
    assert not D.same_bits(y, D.apply(x, seed, 0, p))            # (the low word alone would be mask 0)
    assert D.same_bits(D.backward(x, p, st), D.apply(x, seed, 2 ** 32, p))
    st.check(seed)


def test_a_refused_call_touches_nothing():
    n = 8
    x = _x(n, 8)
    st = D.State(D.SEED, 4)
    for kw in (dict(p=1.0), dict(p=float("nan")), dict(p=0.5, n=0)):
        p = kw.pop("p")
        y, _ = D.forward(x, p, st, expect_rc=-1, **kw)
        assert bool(torch.isnan(y).all()) and st.step() == 4
    st.check(D.SEED)


# ---- the autograd function ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", (0.1, 0.5))
def test_autograd_function_is_the_oracle_and_moves_the_state_by_one(p):
    import vqa_amd
    from vqa_amd.dropout import dropout
    st = vqa_amd.DropoutState(D.SEED, DEV)
    g = torch.Generator().manual_seed(11)
    x_h, g_h = torch.randn(D.FN_SHAPE, generator=g), torch.randn(D.FN_SHAPE, generator=g)
    for step in (1, 2):
        x = x_h.to(DEV).requires_grad_(True)
        y = dropout(x, p, st)
        assert y.data_ptr() != x.data_ptr() and st.step() == step
        (y * g_h.to(DEV)).sum().backward()
        assert D.same_bits(y.detach().cpu(), D.apply(x_h, D.SEED, step, p))
        assert D.same_bits(x.grad.cpu(), D.apply(g_h, D.SEED, step, p))
        assert st.step() == step
    x = x_h.to(DEV)
    assert dropout(x, p, st, training=False) is x and dropout(x, 0.0, st) is x and st.step() == 2
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dropout(x_h, p, st)
    # a backward that no longer has its mask raises instead of using another one
    xa = x_h.to(DEV).requires_grad_(True)
    ya = dropout(xa, p, st)
    dropout(x_h.to(DEV), p, st)
    with pytest.raises(RuntimeError, match="another mask"):
        ya.sum().backward()
    st.reseed(D.SEED_HI, 9)
    assert st.step() == 9 and st.seed == D.SEED_HI


def test_feature_dropout_shares_one_mask_and_keeps_the_structure():
    import vqa_amd
    B, d = 4, 64                                                 # n = 768
    g = torch.Generator().manual_seed(12)
    v_h, q_h = torch.randn(3, B, d, generator=g), torch.randn(3, B, d, generator=g)
    st = vqa_amd.DropoutState(D.SEED, DEV)
    v, q = vqa_amd.feature_dropout(list(v_h.to(DEV).unbind(0)), list(q_h.to(DEV).unbind(0)), 0.5, st)
    assert isinstance(v, list) and len(v) == 3 and tuple(v[0].shape) == (B, d)
    assert D.same_bits(torch.stack(v).cpu(), D.apply(v_h, D.SEED, 1, 0.5)) and D.same_bits(torch.stack(q).cpu(), D.apply(q_h, D.SEED, 1, 0.5))
    v, q = vqa_amd.feature_dropout(v_h.to(DEV), q_h.to(DEV), 0.5, st)
    assert torch.is_tensor(v) and D.same_bits(v.cpu(), D.apply(v_h, D.SEED, 2, 0.5)) and D.same_bits(q.cpu(), D.apply(q_h, D.SEED, 2, 0.5))
    assert st.step() == 2


# ---- the routes of the network ----------------------------------------------------------------------------------------------
ROUTES = ("modules", "eager", "captured")


def _net_inputs():
    c = D.NET_DIMS
    g = torch.Generator().manual_seed(31)
    lens = torch.tensor(sorted((int(t) for t in torch.randint(1, c["T"] + 1, (c["B"],), generator=g)), reverse=True))
    lens[0] = c["T"]
    x = torch.zeros(c["B"], c["T"], dtype=torch.int64)
    for b, n in enumerate(lens):
        x[b, :n] = torch.randint(2, 40, (int(n),), generator=g)
    feats = torch.randn(c["B"], c["N"], c["d"], generator=g).clamp_min_(0)
    labels = torch.randint(0, c["K"], (c["B"],), generator=g)
    return feats.to(DEV), x.to(DEV), lens, labels.to(DEV)


def _run_route(net0, route, p, steps=2, mode="train", state=None):
    """`steps` forward + backward passes of a copy of net0 on one route: per step (logits, loss, dQ, parameter gradients).
    p None: the net as it is built (feature_dropout 0), holding `state` if one is given.  mode "eval": forward only, with
    gradients enabled so that the node routes are taken (the stock LSTM has no backward in eval mode)."""
    from vqa_amd import train as T
    net = copy.deepcopy(net0)
    net.hot_path_static, net.hot_path_graph = route == "eager", route == "captured"
    if p is not None:
        T.set_feature_dropout(net, p, D.SEED)
    elif state is not None:
        net.dropout_state = state
    net.train(mode == "train")
    feats, x, lens, labels = _net_inputs()
    levels = []
    net.question_encoder.register_forward_hook(lambda m, i, o: levels.append([t for t in o if t.requires_grad and (t.retain_grad() or True)]))
    out = []
    for _ in range(steps):
        net.zero_grad(set_to_none=True)
        levels.clear()
        logits, loss = net.forward_features(feats, x, lens, labels=labels)
        out.append(dict(logits=logits.detach().cpu(), loss=loss.detach().cpu().reshape(1)))
        if mode == "train":
            loss.backward()
            out[-1].update(dQ=[t.grad.cpu() for t in levels[0]],
                           grads={k: v.grad.cpu() for k, v in net.named_parameters() if v.grad is not None})
    assert (len(net._graphs) == 1) == (route != "modules")
    return out, net


@pytest.fixture(scope="module")
def routes():
    from vqa_amd import modules as M
    c = D.NET_DIMS
    torch.manual_seed(41)
    net0 = M.HierarchicalCoAttentionNet(dict(vocab_size=40, word_emb_dim=c["d"], hidden_dim=c["d"]),
                                        dict(is_trainable=False, weights_path=None), c["K"], mlp_dim=c["mlp"]).to(DEV)
    got = {r: _run_route(net0, r, D.P_NET) for r in ROUTES}
    return net0, got


def _same_step(a, b):
    assert D.same_bits(a["logits"], b["logits"]) and D.same_bits(a["loss"], b["loss"])
    assert len(a["dQ"]) == len(b["dQ"]) == 3 and all(D.same_bits(s, t) for s, t in zip(a["dQ"], b["dQ"]))
    assert a["grads"].keys() == b["grads"].keys() and len(a["grads"]) >= 16
    for k in a["grads"]:
        assert D.same_bits(a["grads"][k], b["grads"][k]), k


def test_the_three_routes_agree_bit_for_bit_over_two_steps(routes):
    _, got = routes
    for step in range(2):
        ref = got["modules"][0][step]
        assert bool(torch.isfinite(ref["logits"]).all()) and float(ref["loss"]) > 0
        for r in ("eager", "captured"):
            _same_step(ref, got[r][0][step])
    for r in ROUTES:
        out, net = got[r]
        assert not D.same_bits(out[0]["logits"], out[1]["logits"]), r             # step 2 drew another mask
        assert net.dropout_state.step() == 2, r                                   # (the capture's warm-up drew none)


def _composed(net0, mode="train"):
    """question encoder -> co-attention -> (v, q) by hand on a copy of net0: calls that know nothing of dropout."""
    net = copy.deepcopy(net0).train(mode == "train")
    feats, x, lens, labels = _net_inputs()
    v, q = net.co_attention(feats, list(net.question_encoder(x, lens)))
    return net, v, q, labels


def test_the_node_is_the_existing_head_on_the_oracles_mask(routes):
    """co-attention outputs of a forward without dropout, multiplied on the host by the oracle's masks 1 and 2, through the
    existing answer head: the logits and the loss of every route, bit for bit."""
    net0, got = routes
    net, v, q, labels = _composed(net0)
    v, q = torch.stack(list(v)).detach().cpu(), torch.stack(list(q)).detach().cpu()
    for step in (1, 2):
        vm, qm = D.apply(v, D.SEED, step, D.P_NET).to(DEV), D.apply(q, D.SEED, step, D.P_NET).to(DEV)
        assert not D.same_bits(vm.cpu(), v)
        logits, loss = net.mlp_classify.forward_loss(list(vm.unbind(0)), list(qm.unbind(0)), labels=labels)
        for r in ROUTES:
            assert D.same_bits(logits.detach().cpu(), got[r][0][step - 1]["logits"]), (r, step)
            assert D.same_bits(loss.detach().cpu().reshape(1), got[r][0][step - 1]["loss"]), (r, step)


def test_p0_and_eval_are_the_composition_without_dropout_and_leave_the_state(routes):
    """The references are composed by hand from calls that know nothing of dropout: question encoder -> co-attention ->
    mlp_classify.forward_loss, in training mode with the backward, in eval mode forward only."""
    import vqa_amd
    net0, got = routes
    refs = {}
    for mode in ("train", "eval"):
        net, v, q, labels = _composed(net0, mode)
        logits, loss = net.mlp_classify.forward_loss(v, q, labels=labels)
        refs[mode] = dict(logits=logits.detach().cpu(), loss=loss.detach().cpu().reshape(1))
        if mode == "train":
            loss.backward()
            refs[mode]["grads"] = {k: t.grad.cpu() for k, t in net.named_parameters() if t.grad is not None}
    assert not D.same_bits(refs["train"]["logits"], got["modules"][0][0]["logits"])   # (dropout does change the result)

    def check(out, ref, what):
        for o in out:
            assert D.same_bits(o["logits"], ref["logits"]) and D.same_bits(o["loss"], ref["loss"]), what
            for k in ref.get("grads", {}):
                assert D.same_bits(o["grads"][k], ref["grads"][k]), (what, k)

    for route in ROUTES:
        state = vqa_amd.DropoutState(D.SEED, DEV)                   # a p = 0 net in training that holds a state
        out, net = _run_route(net0, route, None, state=state)
        assert net.feature_dropout == 0.0 and net.dropout_state is state and state.step() == 0 and state.draws == 1
        check(out, refs["train"], (route, "p = 0"))
        out, net = _run_route(net0, route, D.P_NET, mode="eval")    # p > 0 in eval mode
        assert net.feature_dropout == D.P_NET and net.dropout_state.step() == 0 and net.dropout_state.draws == 1
        check(out, refs["eval"], (route, "eval"))


def test_a_second_backward_accumulates_under_the_same_mask():
    """The eager node with direct gradients: a second backward on one forward (retain_graph) adds the same masked gradient
    again -- the backward never advances."""
    import vqa_amd
    from vqa_amd.graph import HotPathGraph
    from vqa_amd.modules import MLPClassifier
    c = D.NET_DIMS
    torch.manual_seed(43)
    co, head = vqa_amd.ParallelCoAttention(c["d"]).to(DEV), MLPClassifier(c["d"], c["mlp"], c["K"]).to(DEV)
    st = vqa_amd.DropoutState(D.SEED, DEV)
    hp = HotPathGraph(co, head, c["B"], c["N"], c["T"], capture=False, direct_grads=True, dropout=D.P_NET, dropout_state=st)
    assert st.step() == 0
    feats, _, _, labels = _net_inputs()
    Qs = [(torch.randn(c["B"], c["T"], c["d"], device=DEV) * 0.2).requires_grad_(True) for _ in range(3)]
    _, loss = hp(feats, Qs, labels)
    loss.backward(retain_graph=True)
    w = head.W_w.weight
    once, dq_once = w.grad.clone(), Qs[0].grad.clone()
    with pytest.warns(UserWarning, match="ADDS"):
        loss.backward()
    assert st.step() == 1
    assert torch.equal(w.grad, once + once) and float(once.abs().max()) > 0
    assert torch.equal(Qs[0].grad, dq_once + dq_once)
    with pytest.raises(ValueError, match="dropout_state"):
        HotPathGraph(co, head, c["B"], c["N"], c["T"], capture=False, dropout=0.5)


# ---- the trainer ------------------------------------------------------------------------------------------------------------
def test_trainer_steps_with_feature_dropout_and_validate_leaves_the_state():
    from vqa_amd import train as T
    dev = torch.device(DEV)
    torch.manual_seed(0)
    model = T.build_model("attention", 100, 10).to(dev)
    tr = T.Trainer(model, 1e-4, dev, feature_dropout=0.5, dropout_seed=D.SEED)
    assert model.feature_dropout == 0.5 and model.dropout_state.seed == D.SEED and model.dropout_state.step() == 0
    b = T.synthetic_batch(4, (64, 64), 26, 100, 11, seed=1)
    im, qu, la, ln = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])
    im, qu, la = im.to(dev), qu.to(dev), la.to(dev)
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state(dev))
    losses = [float(tr.step(im, qu, ln, la).detach())]
    assert model.dropout_state.step() == 1
    m = tr.validate([(im, qu, ln, la)])
    assert model.dropout_state.step() == 1 and m["loss"] == m["loss"] and model.training
    losses += [float(tr.step(im, qu, ln, la).detach()) for _ in range(2)]
    assert model.dropout_state.step() == 3
    assert all(np.isfinite(v) and v > 0 for v in losses), losses
    # the masks consume nothing from torch's generators
    assert torch.equal(torch.get_rng_state(), rng[0]) and torch.equal(torch.cuda.get_rng_state(dev), rng[1])
    with pytest.raises(ValueError, match="opt_lvl"):
        T.Trainer(model, 1e-4, dev, opt_lvl=1, feature_dropout=0.5)
