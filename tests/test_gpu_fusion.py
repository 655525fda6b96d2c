"""The fusion head of the baseline model on the GPU (csrc/fusion.hip through include/coattn_fusion.h v0.26.0): every output
against the float64 oracle of the header's formulas under the project's error rule (at most 8 x the deviation of stock fp32 on
the CPU, floor 16 fp32 ulps of the tensor's largest magnitude), the dropout mask against tests/_dropout.keep, bit repeatability,
the optional buffers and strides, zero rows and non-finite values, the module route, the trainer and predict.py.

Shapes (B, Di, H, J, Mh, K): one row with one partial chunk everywhere; a ragged last chunk, waves without work and every
width below a tile; a second row tile with one live row, 9 chunks over 8 waves, a ragged column tile and aligned logits rows
(K % 4 == 0); the real J / Mh with an odd K; and the baseline's own shape (oracle, repeat and padded-leading-dimension tests).
"""
import copy
import json

import numpy as np
import pytest
import torch

import vqa_amd
from vqa_amd import _lib, modules as M, train as T

from tests import _dropout as D
from tests import _fusion as U

pytestmark = pytest.mark.gpu

PS = (0.0, 0.5)


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


_BASE = {}


def _base(shape, p):
    """One forward + backward of the shared case straight through the C-ABI, run once per (shape, p) and left unchanged."""
    if (shape, p) not in _BASE:
        _BASE[shape, p] = U.run(U.make_case(*shape), p=p)
    return _BASE[shape, p]


def _bounded(got, want64, want32, keys=U.OUTPUTS, what=""):
    bad = []
    for k in keys:
        err, bound = U.bound_check("%s %s" % (what, k), got[k], want64[k], want32[k])
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


@pytest.mark.parametrize("p", PS, ids=_id)
@pytest.mark.parametrize("shape", U.SMALL + [U.BASELINE], ids=_id)
def test_every_output_against_the_float64_oracle(shape, p):
    got = _base(shape, p)
    want64, want32 = U.references(shape, p)
    assert not any(bool(torch.isnan(got[k]).any()) for k in U.OUTPUTS)
    _bounded(got, want64, want32, what=_id(shape))
    err, bound = U.bound_check("m", got["m"], want64["m"], want32["m"])
    assert err <= bound


@pytest.mark.parametrize("shape", U.SMALL, ids=_id)
def test_the_mask_is_the_contracts(shape):
    """The zeros of m (= tanh(0): the dropped elements) lie exactly where tests/_dropout.keep says, for mask step + 1 of the
    state; db_m of a one-hot g_logits is zero exactly on the columns whose element of that row is dropped; the step advances by
    one per training forward and not at all in the backward, in inference and at p = 0."""
    c, p = U.make_case(*shape), 0.5
    B, Mh, K = shape[0], shape[4], shape[5]
    got = U.run(c, p=p)                                           # (a state of its own: the calls below advance it)
    keep = torch.from_numpy(np.array(D.keep(B * Mh, U.SEED, U.STEP0 + 1, p))).view(B, Mh)
    assert bool((got["m"][~keep] == 0).all()) and bool((got["m"][keep] != 0).all())
    st = got["state"]
    assert st.step() == U.STEP0 + 1 and bool((st.words()[:2] == D.state_words(U.SEED, 0)[:2]).all())
    assert bool((st.words()[4:] == 0).all())
    # a one-hot gradient at (row b, class 1): dpre is zero outside row b, so db_m = dpre[b] -- zero exactly where dropped
    b = B - 1
    g = torch.zeros(B, K)
    g[b, 1] = 1.0
    again = U.run(c, p=p, g=g)                                    # a fresh state: the same mask
    assert bool((again["db_m"][~keep[b]] == 0).all()) and bool((again["db_m"][keep[b]] != 0).all())
    # the same state through a second training forward + two backwards, an inference call and a p = 0 training forward
    second = U.run(c, p=p, state=st, backwards=2)
    assert st.step() == U.STEP0 + 2
    keep2 = torch.from_numpy(np.array(D.keep(B * Mh, U.SEED, U.STEP0 + 2, p))).view(B, Mh)
    assert bool((second["m"][~keep2] == 0).all()) and bool((second["m"][keep2] != 0).all())
    U.run(c, p=0.0, state=st, saved=False)
    U.run(c, p=0.0, state=st)
    assert st.step() == U.STEP0 + 2


@pytest.mark.parametrize("p", PS, ids=_id)
@pytest.mark.parametrize("shape", U.SMALL + [U.BASELINE], ids=_id)
def test_repeats_give_the_same_bits(shape, p):
    """Two runs into fresh NaN-filled buffers, and two backwards after one forward."""
    base = _base(shape, p)
    again = U.run(U.make_case(*shape), p=p, backwards=2)
    for k in U.OUTPUTS:
        assert U.same_bits(base[k], again[k]), k
        assert U.same_bits(again["bwd"][0][k], again["bwd"][1][k]) if k != "logits" else True, k
    assert U.same_bits(base["saved_raw"], again["saved_raw"])


@pytest.mark.parametrize("p", PS, ids=_id)
@pytest.mark.parametrize("shape", U.SMALL, ids=_id)
def test_optional_buffers(shape, p):
    c, base = U.make_case(*shape), _base(shape, p)
    g = torch.Generator().manual_seed(5)
    prefill = {"d" + n: torch.randn(c[n].shape, generator=g) for n in U.PARAMS}
    acc = U.run(c, p=p, accumulate=1, prefill=prefill)
    for k in U.GRADS:
        assert U.same_bits(acc[k], prefill[k] + base[k]), k
    no_dh = U.run(c, p=p, dh=False)
    assert bool(torch.isnan(no_dh["dh"]).all())
    for k in U.GRADS:
        assert U.same_bits(no_dh[k], base[k]), k
    if p == 0:
        infer = U.run(c, saved=False)
        assert U.same_bits(infer["logits"], base["logits"])


@pytest.mark.parametrize("p", PS, ids=_id)
@pytest.mark.parametrize("shape", U.SMALL + [U.BASELINE], ids=_id)
def test_padded_leading_dimensions_give_the_dense_bits(shape, p):
    base = _base(shape, p)
    got = U.run(U.make_case(*shape), p=p, ld_f=shape[1] + 4, ld_h=shape[2] + 8)      # (the padding: NaN)
    for k in U.OUTPUTS:
        assert U.same_bits(base[k], got[k]), k


def test_a_misaligned_operand_is_refused():
    c = U.make_case(*U.SMALL[1])
    for name in ("f", "h", "logits", "saved") + tuple(U.PARAMS):
        got = U.run(c, shift=name, expect_rc=-1)
        assert got["rc"] == (-1, None) and "aligned" in got["err"], name
        assert bool(torch.isnan(got["logits"]).all())
    for name in ("g", "dh", "ws") + U.GRADS:
        got = U.run(c, shift=name, expect_rc_bwd=-1)
        assert got["rc"] == (0, -1) and "aligned" in got["err"], name
        assert all(bool(torch.isnan(got[k]).all()) for k in U.GRADS + ("dh",))
    got = U.run(c, ld_f=c["Di"] + 2, expect_rc=-1)
    assert "ld_f" in got["err"]
    got = U.run(c, flags=_lib.FLAG_BF16_PROJ, expect_rc=-1)
    assert "exact fp32" in got["err"] and bool(torch.isnan(got["logits"]).all())


@pytest.mark.parametrize("p", PS, ids=_id)
@pytest.mark.parametrize("shape", U.SMALL[1:], ids=_id)
def test_a_zero_row_of_f(shape, p):
    c = U.make_case(*shape)
    f = c["f"].clone()
    f[1] = 0
    got = U.run(c, p=p, f=f)
    assert not any(bool((~torch.isfinite(got[k])).any()) for k in U.OUTPUTS)
    _bounded(got, U.oracle(c, torch.float64, p, f=f), U.oracle(c, torch.float32, p, f=f), what="zero row")


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=_id)
@pytest.mark.parametrize("where", ["f", "h"])
@pytest.mark.parametrize("shape", U.SMALL[1:], ids=_id)
def test_a_non_finite_value_stays_in_its_row(shape, where, value):
    c, base = U.make_case(*shape), _base(shape, 0.5)
    b = shape[0] - 1                                              # (33 rows: the one live row of the second tile)
    x = c[where].clone()
    x[b, 3] = value
    got = U.run(c, p=0.5, **{where: x})
    others = torch.arange(shape[0]) != b
    for k in ("logits", "dh"):
        assert U.same_bits(got[k][others], base[k][others]), k
    if where == "f" or value != value:                            # (an infinite h only saturates the tanh of e_q)
        assert bool((~torch.isfinite(got["logits"][b])).any())


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def test_fusion_head_function_matches_the_c_abi_and_leaves_torchs_generator_alone():
    dev = torch.device("cuda:0")
    shape = U.SMALL[2]
    c, base = U.make_case(*shape), _base(shape, 0.5)
    ps = [c[n].to(dev).requires_grad_(True) for n in U.PARAMS]
    h = c["h"].to(dev).requires_grad_(True)
    state = vqa_amd.DropoutState(U.SEED, dev)
    state.reseed(U.SEED, U.STEP0)
    rng = torch.cuda.get_rng_state(dev)
    logits = vqa_amd.fusion_head(c["f"].to(dev), h, *ps, p=0.5, state=state)
    (logits * c["g"].to(dev)).sum().backward()
    assert torch.equal(torch.cuda.get_rng_state(dev), rng)
    assert state.step() == U.STEP0 + 1
    assert U.same_bits(logits.detach().cpu(), base["logits"]) and U.same_bits(h.grad.cpu(), base["dh"])
    for n, t in zip(U.PARAMS, ps):
        assert U.same_bits(t.grad.cpu(), base["d" + n]), n
    with torch.no_grad():                                         # inference: p ignored, the state untouched
        ev = vqa_amd.fusion_head(c["f"].to(dev), h, *ps, p=0.5, state=state, training=False)
    assert state.step() == U.STEP0 + 1 and U.same_bits(ev.cpu(), _base(shape, 0.0)["logits"])
    with torch.autocast("cuda", dtype=torch.bfloat16):            # an fp32 island
        ac = vqa_amd.fusion_head(c["f"].to(dev).bfloat16(), h.detach().bfloat16(), *[t.detach() for t in ps], training=False)
    assert ac.dtype == torch.float32 and bool(torch.isfinite(ac).all())
    with pytest.raises(RuntimeError, match="f requires a gradient"):
        vqa_amd.fusion_head(c["f"].to(dev).requires_grad_(True), h, *ps)


# ---- the module route ------------------------------------------------------------------------------------------------------
_SHARED = {}


def _net(p_drop):
    """A copy of one seeded baseline model (built once) with the dropout probability of its mlp set.  The two nn.Dropout of
    the frozen VGG's fc layers (in front of the head, the same stock modules on both routes) are switched off: they draw from
    torch's generators, which a float64 copy on the CPU cannot follow."""
    if "net" not in _SHARED:
        torch.manual_seed(0)
        _SHARED["net"] = T.build_model("baseline", 100, 10)
        for m in _SHARED["net"].image_encoder.vgg11_encoder.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
    net = copy.deepcopy(_SHARED["net"])
    net.mlp[1].p = p_drop
    return net


def _g():
    return torch.randn(4, 11, generator=torch.Generator().manual_seed(3))


def _ref64_train_p0():
    """The float64 copy's logits and gradients in training mode at p = 0: computed once, shared and left unchanged."""
    if "ref64" not in _SHARED:
        im, qu, la, ln = _batch()
        _SHARED["ref64"] = _reference(_net(0.0), im, qu, ln, _g(), torch.float64)
    return _SHARED["ref64"]


def _batch(B=4, size=64):
    b = T.synthetic_batch(B, (size, size), 26, 100, 11, seed=1)
    return T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])


class _NumpyMask(torch.nn.Module):
    def __init__(self, mult):
        super().__init__()
        self.mult = mult

    def forward(self, x):
        return x * self.mult.to(x.dtype)


def _reference(net0, im, qu, ln, g, dtype, device="cpu", mask=None, train=True):
    """Logits and every trainable gradient of sum(logits * g) from a copy of the model on the stock lines in `dtype`."""
    ref = copy.deepcopy(net0).to(device=device, dtype=dtype).train(train)
    ref.fusion_impl = "stock"
    if mask is not None:
        ref.mlp[1] = _NumpyMask(mask.to(device))
    out = ref(im.to(device=device, dtype=dtype), qu.to(device), ln)
    if not train:
        return out.detach().cpu(), {}
    (out * g.to(device=device, dtype=dtype)).sum().backward()
    return out.detach().cpu(), {n: q.grad.cpu() for n, q in ref.named_parameters() if q.requires_grad}


def _hip(net0, im, qu, ln, g, seed=0, train=True):
    dev = torch.device("cuda:0")
    net = copy.deepcopy(net0).to(dev).train(train)
    T.set_fusion_head(net, "hip", seed)
    assert net.fusion_impl == "hip" and net.fusion_dropout_state is not None
    bound, rngs = [], []
    real, real_head = _lib.bind, vqa_amd.fusion.fusion_head

    def head(*a, **kw):                                           # torch's generator across the head's own call
        rngs.append(torch.cuda.get_rng_state(dev))
        out = real_head(*a, **kw)
        rngs.append(torch.cuda.get_rng_state(dev))
        return out
    _lib.bind = lambda name, **kw: (bound.append(name), real(name, **kw))[1]
    vqa_amd.fusion.fusion_head = head
    try:
        with torch.set_grad_enabled(train):
            out = net(im.to(dev), qu.to(dev), ln)
            rngs.append(torch.cuda.get_rng_state(dev))
            if train:
                (out * g.to(dev)).sum().backward()
            rngs.append(torch.cuda.get_rng_state(dev))
    finally:
        _lib.bind, vqa_amd.fusion.fusion_head = real, real_head
    assert "coattn_fusion_forward" in bound and ("coattn_fusion_backward" in bound) == train      # the route is really taken
    assert len(rngs) == 4 and all(torch.equal(r, rngs[0]) for r in rngs)     # torch's generator is not consumed by this site
    return out.detach().cpu(), {n: q.grad.cpu() for n, q in net.named_parameters() if q.requires_grad and train}, net


def _rule(what, got, grads, want64, grads64, want32, grads32):
    bad = []
    err, bound = U.bound_check(what + " logits", got, want64, want32)
    if not err <= bound:
        bad.append(("logits", err, bound))
    assert set(grads) == set(grads64) == set(grads32)
    for n in grads:
        err, bound = U.bound_check(n[-24:], grads[n], grads64[n], grads32[n])
        if not err <= bound:
            bad.append((n, err, bound))
    assert not bad, bad


def test_module_route_in_training_mode_without_dropout():
    """fusion_impl = "hip" with mlp[1].p = 0 against the stock route (the yardstick: the stock lines in fp32 on the same GPU),
    both measured from a float64 copy of the model: the logits and every trainable gradient."""
    net0 = _net(0.0)
    im, qu, la, ln = _batch()
    g = _g()
    want64, grads64 = _ref64_train_p0()
    want32, grads32 = _reference(net0, im, qu, ln, g, torch.float32, "cuda:0")
    got, grads, _ = _hip(net0, im, qu, ln, g)
    assert "mlp.0.weight" in grads and "question_encoder.gru.weight_hh_l0" in grads and "image_encoder.embedding_layer.0.bias" in grads
    _rule("train p=0", got, grads, want64, grads64, want32, grads32)


def test_module_route_in_eval_mode_ignores_the_dropout():
    net0 = _net(0.5)
    im, qu, la, ln = _batch()
    want64, _ = _reference(net0, im, qu, ln, None, torch.float64, train=False)
    want32, _ = _reference(net0, im, qu, ln, None, torch.float32, "cuda:0", train=False)
    got, _, net = _hip(net0, im, qu, ln, None, train=False)
    assert net.fusion_dropout_state.step() == 0
    _rule("eval p=.5", got, {}, want64, {}, want32, {})


def test_module_route_in_training_mode_draws_the_contracts_mask():
    """p = 0.5 in training mode: the float64 copy with nn.Dropout replaced by the numpy mask of (seed, step 1); the seed is
    honoured (another seed: another mask, the same seed: the same mask)."""
    net0 = _net(0.5)
    im, qu, la, ln = _batch()
    g = _g()
    seed = 77
    mult = torch.from_numpy(np.where(D.keep(4 * 1000, seed, 1, 0.5), np.float64(D.scale(0.5)), 0.0)).view(4, 1000)
    want64, grads64 = _reference(net0, im, qu, ln, g, torch.float64, mask=mult)
    want32, grads32 = _reference(net0, im, qu, ln, g, torch.float32, "cuda:0", mask=mult)
    got, grads, net = _hip(net0, im, qu, ln, g, seed=seed)
    assert net.fusion_dropout_state.step() == 1
    _rule("train p=.5", got, grads, want64, grads64, want32, grads32)
    same, _, _ = _hip(net0, im, qu, ln, g, seed=seed)
    other, _, _ = _hip(net0, im, qu, ln, g, seed=seed + 1)
    # (the encoders in front are stock modules whose bits may differ from run to run -- the convolutions' library picks its
    #  kernels per process state --, so the same mask is recognised by a difference at rounding level, 1e-4 of the largest
    #  logit, and another mask -- about half of the 1000 hidden units change sides -- by one of the logits' own order, 1e-2)
    scale = float(got.abs().max())
    d_same, d_other = float((same - got).abs().max()), float((other - got).abs().max())
    print("seed: same %.3e other %.3e scale %.3e" % (d_same, d_other, scale))
    assert d_same <= 1e-4 * scale and d_other >= 1e-2 * scale


# ---- trainer and predict -----------------------------------------------------------------------------------------------------
def test_trainer_steps_on_the_hip_route_follow_the_stock_route():
    """Two Trainer.steps of the baseline model from the same weights on both routes, mlp[1].p = 0.  The first loss: the error
    rule against a float64 copy's loss; the second, after one Adam step of lr 1e-4: a relative 1e-3, a cap against a gross
    error.  Then --question_gru hip and --fusion_head hip together, with the dropout on."""
    dev = torch.device("cuda:0")
    net0 = _net(0.0)
    im, qu, la, ln = _batch()
    loss64 = torch.nn.functional.cross_entropy(_ref64_train_p0()[0], la)      # (the same model, batch and mode)
    losses = {}
    for route in ("stock", "hip"):
        net = copy.deepcopy(net0).to(dev)
        tr = T.Trainer(net, 1e-4, dev, fusion_head=route, dropout_seed=5)
        assert net.fusion_impl == route and (net.fusion_dropout_state is not None) == (route == "hip")
        torch.manual_seed(7)
        losses[route] = [tr.step(im.to(dev), qu.to(dev), ln, la.to(dev)).detach().cpu().double() for _ in range(2)]
        assert net.mlp[0].weight.grad is not None and net.image_encoder.embedding_layer[0].weight.grad is not None
    print("trainer losses", losses, float(loss64))
    err, bound = U.bound_check("first loss", losses["hip"][0].view(1), loss64.view(1), losses["stock"][0].view(1))
    assert err <= bound
    rel = abs(float(losses["hip"][1] - losses["stock"][1])) / abs(float(losses["stock"][1]))
    print("second loss: relative difference %.3e" % rel)
    assert rel <= 1e-3
    both = copy.deepcopy(net0).to(dev)
    both.mlp[1].p = 0.5
    tr = T.Trainer(both, 1e-4, dev, question_gru="hip", fusion_head="hip", dropout_seed=5)
    two = [float(tr.step(im.to(dev), qu.to(dev), ln, la.to(dev))) for _ in range(2)]
    assert all(np.isfinite(two)) and both.fusion_dropout_state.step() == 2


def test_predict_cli_gives_the_stock_routes_answers(tmp_path):
    """predict.py --fusion_head stock | hip on one seeded checkpoint: the same top-1, and the top-1 probabilities under the
    error rule against a float64 copy of the model run sample by sample on the CPU (eval mode: the samples are independent)."""
    from vqa_amd import predict as Pr
    torch.manual_seed(2)
    net0 = T.build_model("baseline", 100, 10)
    ckpt = str(tmp_path / "net.pth")
    torch.save(net0.state_dict(), ckpt)
    recs = {}
    for route in ("stock", "hip"):
        out = str(tmp_path / (route + ".jsonl"))
        summary = Pr.main(["--model", "baseline", "--model_ckpt", ckpt, "--test_size", "8", "--predictions", out, "--num_cls", "10",
                           "--batch_size", "8", "--image_size", "64", "--vocab_size", "100", "--fusion_head", route])
        assert summary["samples"] == 8
        recs[route] = [json.loads(line) for line in open(out)]
    args = Pr.build_parser().parse_args(["--model", "baseline", "--num_cls", "10", "--vocab_size", "100"])
    ds = T.SyntheticVQADataset(8, (64, 64), args.max_seq_length, 100, 11, Pr.TEST_SEED, num_answers=0, images=True)
    ref = copy.deepcopy(net0).double().eval()
    p64, p_stock, p_hip = [], [], []
    for i, (a, b) in enumerate(zip(recs["stock"], recs["hip"])):
        assert a["index"] == b["index"] == i and a["label"] == b["label"]
        assert a["top"][0] == b["top"][0], (a, b)
        s = ds[i]
        with torch.no_grad():
            prob = torch.softmax(ref(s["image"][None].double(), s["question"][None], torch.as_tensor(s["ques_len"]).view(1)), 1)[0]
        p64.append(float(prob[a["top"][0]]))
        p_stock.append(a["prob"][0])
        p_hip.append(b["prob"][0])
    err, bound = U.bound_check("top-1 prob", torch.tensor(p_hip, dtype=torch.float64), torch.tensor(p64, dtype=torch.float64),
                               torch.tensor(p_stock, dtype=torch.float64))
    assert err <= bound
