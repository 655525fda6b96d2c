"""The HIP sentence LSTM (csrc/lstm.hip through include/coattn.h, vqa_amd.lstm, the encoders' sentence_impl = "hip") on the GPU
against stock PyTorch's packed nn.LSTM in float64 (tests/_lstm.py), at the smallest shapes that reach each branch.

The error rule: a tensor's largest deviation from the float64 oracle may be at most 8 times the deviation
of stock fp32 nn.LSTM on the CPU on the same inputs, with a floor of 16 fp32 ulps of the tensor's largest magnitude."""
import functools

import pytest
import torch

from vqa_amd import _lib, modules as M

from tests import _lstm as L

pytestmark = pytest.mark.gpu

# (B, T, E, H)                      the branch it reaches
SHAPES = [(1, 1, 32, 32),           # no recurrent product at all
          (3, 5, 64, 32),           # H / 8 = 4 chunks of the contraction: waves without work
          (33, 7, 32, 96),          # a row tile of one live row, three unit groups of the backward
          (5, 26, 288, 288),        # a ragged share of the contraction over the waves
          (33, 26, 512, 512)]       # the workload's width, at a fifth of its batch
CASES = [(s, "unsorted") for s in SHAPES] + [(s, "sorted_dead_tail") for s in SHAPES if s[0] >= 33]
GRADS = ("dw_ih", "dw_hh", "db_ih", "db_hh")


def _id(case):
    return "%dx%dx%dx%d-%s" % (*case[0], case[1])


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    return L.make_case(*shape, seed=sum(shape), kind=kind)


@functools.lru_cache(maxsize=None)
def _refs(shape, kind):
    c = _case(shape, kind)
    return L.oracle(c, torch.float64), L.oracle(c, torch.float32)


@functools.lru_cache(maxsize=None)
def _base(shape, kind):
    return L.run(_case(shape, kind))


def _same(a, b, keys=L.OUTPUTS):
    for k in keys:
        assert L.same_bits(a[k], b[k]), k


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_against_the_float64_oracle(case):
    ref64, ref32 = _refs(*case)
    got = _base(*case)
    bad = []
    for k in L.OUTPUTS:
        err, bound = L.bound_check(k, got[k], ref64[k], ref32[k])
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_exact_zeros_past_the_lengths_and_x_masked_is_x(case):
    c, got = _case(*case), _base(*case)
    live = L.live_mask(c["lens"], c["T"])
    for k in ("out", "x_masked", "dX"):
        assert bool((got[k][~live].view(torch.int32) == 0).all()), k      # +0.0, every bit
    assert L.same_bits(got["x_masked"][live], c["X"][live])
    assert all(bool(torch.isfinite(got[k]).all()) for k in L.OUTPUTS)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_pad_rows_of_every_input_do_not_matter(case):
    c, base = _case(*case), _base(*case)
    dead = ~L.live_mask(c["lens"], c["T"])
    g = torch.Generator().manual_seed(9)
    for fill in (None, 1e30):
        X, go, gx = c["X"].clone(), c["g_out"].clone(), c["g_xm"].clone()
        for t in (X, go, gx):
            t[dead] = (torch.randn(t[dead].shape, generator=g) * 100.0) if fill is None else fill
        if fill is not None:
            X[dead] = -fill
        _same(base, L.run(c, X=X, g_out=go, g_xm=gx))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_lengths_are_clamped_on_the_device(case):
    """len = 0 (and a negative one) gives the bits of len = 1, len = T + 5 those of len = T (at T = 1 both are the one row)."""
    c = _case(*case)
    B, T = c["B"], c["T"]
    lo, hi, ref = c["lens"].clone(), c["lens"].clone(), c["lens"].clone()
    lo[c["lens"] == 1] = 0
    if B > 2:
        lo[2], ref[2] = -3, 1
    hi[c["lens"] == T] = T + 5
    assert bool((hi > T).any()) and (bool((lo < 1).any()) or B == 1)      # (B = 1, T > 1: the one sample has length T)
    _same(_base(*case) if bool((ref == c["lens"]).all()) else L.run(c, lens=ref), L.run(c, lens=lo))
    _same(_base(*case), L.run(c, lens=hi))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_repeatable_and_guard_bands_intact(case):
    """Two runs into freshly NaN-filled buffers: the same bits everywhere (L.run checks every arena's margins each time)."""
    _same(_base(*case), L.run(_case(*case)))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_accumulate_adds_onto_the_parameter_gradients(case):
    c, base = _case(*case), _base(*case)
    g = torch.Generator().manual_seed(5)
    pre = {n: torch.randn(c[n].shape, generator=g) for n in L.PARAMS}
    got = L.run(c, accumulate=1, prefill=pre)
    for n in L.PARAMS:
        want = pre[n] + base["d" + n]                               # one fp32 rounding
        assert L.same_bits(got["d" + n], want), n
    _same(base, got, ("out", "x_masked", "dX"))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_optional_buffers(case):
    c, base = _case(*case), _base(*case)
    no_dx = L.run(c, dX=False)
    _same(base, no_dx, GRADS + ("out", "x_masked"))
    assert bool(torch.isnan(no_dx["dX"]).all())
    fwd_only = L.run(c, saved=False)
    _same(base, fwd_only, ("out", "x_masked"))
    assert all(bool(torch.isnan(fwd_only[k]).all()) for k in GRADS + ("dX",))
    no_xm = L.run(c, x_masked=False, with_g_xm=False)
    _same(base, no_xm, GRADS + ("out",))
    assert bool(torch.isnan(no_xm["x_masked"]).all())
    zero = L.run(c, g_xm=torch.zeros_like(c["g_xm"]))                # no g_xmasked = a zero one, up to the sign of zero
    assert bool((zero["dX"] == no_xm["dX"]).all())


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_a_nan_stays_in_its_sample(case):
    c, base = _case(*case), _base(*case)
    b = 0                                                            # (length T: every row live)
    assert int(c["lens"][b]) == c["T"]
    t0 = min(2, c["T"] - 1)
    X = c["X"].clone()
    X[b, t0, 5] = float("nan")
    got = L.run(c, X=X)
    others = torch.arange(c["B"]) != b
    for k in ("out", "x_masked", "dX"):
        assert L.same_bits(got[k][others], base[k][others]), k
    assert bool(torch.isnan(got["out"][b, t0:]).all()) and not bool(torch.isnan(got["out"][b, :t0]).any())
    assert bool(torch.isnan(got["dX"][b]).any())


def test_refusals_launch_nothing():
    c = _case((3, 5, 64, 32), "unsorted")
    for flags in (_lib.FLAG_FAST16, _lib.FLAG_BF16_PROJ, _lib.FLAG_SPLIT2):
        got = L.run(c, flags=flags, expect_rc=-1)
        assert got["rc"] == (-1, -1) and "exact fp32" in _lib.load().coattn_last_error().decode()
        assert all(bool(torch.isnan(got[k]).all()) for k in L.OUTPUTS)
    bad = L.make_case(3, 5, 48, 32, seed=1)                          # E no multiple of 32
    got = L.run(bad, expect_rc=-1)
    assert got["rc"] == (-1, -1) and "not supported" in _lib.load().coattn_last_error().decode()
    assert all(bool(torch.isnan(got[k]).all()) for k in L.OUTPUTS)


# ---- the module route ------------------------------------------------------------------------------------------------------
def _encoder_oracle(enc, x, lens, g, dtype):
    """The three levels and every parameter gradient of sum_l sum(level_l * g_l) from the stock CPU modules in `dtype`,
    the LSTM behind pack_padded_sequence(enforce_sorted=False)."""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    ref = M.QuestionCoAttentionEncoder(enc.vocab_size, enc.embedding_dim, enc.hidden_dim).to(dtype)
    ref.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in enc.state_dict().items()})
    T = x.shape[1]
    words = ref.word_embedding(x)
    packed = pack_padded_sequence(ref.phrase_conv_pool(words), lens, batch_first=True, enforce_sorted=False)
    sent, _ = ref.sentence_lstm(packed)
    levels = (words, pad_packed_sequence(packed, batch_first=True, total_length=T)[0],
              pad_packed_sequence(sent, batch_first=True, total_length=T)[0])
    sum((lv * gl.to(dtype)).sum() for lv, gl in zip(levels, g)).backward()
    return [lv.detach() for lv in levels], {n: p.grad for n, p in ref.named_parameters()}


def test_module_route_against_the_float64_encoder(monkeypatch):
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    B, T, E = 6, 9, 64
    enc = M.QuestionCoAttentionEncoder(40, E, E).to(dev)
    enc.sentence_impl = "hip"
    lens = torch.tensor([4, 9, 1, 7, 9, 2])
    x = torch.zeros(B, T, dtype=torch.int64)
    for b, n in enumerate(lens):
        x[b, :n] = torch.randint(1, 40, (int(n),))
    g = [torch.randn(B, T, E) for _ in range(3)]

    def boom(*a, **k):
        raise AssertionError("the hip route must not pack")
    monkeypatch.setattr(M, "pack_padded_sequence", boom)
    levels = enc(x.to(dev), lens.to(dev))                            # CUDA int64 lengths, unsorted
    sum((lv * gl.to(dev)).sum() for lv, gl in zip(levels, g)).backward()
    monkeypatch.undo()
    want64, grads64 = _encoder_oracle(enc, x, lens, g, torch.float64)
    want32, grads32 = _encoder_oracle(enc, x, lens, g, torch.float32)
    bad = []
    for i, name in enumerate(("words", "phrases", "sentence")):
        err, bound = L.bound_check(name, levels[i].detach().cpu(), want64[i], want32[i])
        if not err <= bound:
            bad.append((name, err, bound))
    for n, p in enc.named_parameters():
        err, bound = L.bound_check(n[-24:], p.grad.cpu(), grads64[n], grads32[n])
        if not err <= bound:
            bad.append((n, err, bound))
    assert not bad, bad
    dead = ~L.live_mask(lens, T)
    assert all(bool((lv.detach().cpu()[dead] == 0).all()) for lv in levels)


def test_bert_encoder_takes_the_hip_route_in_fp32_and_under_bf16_autocast(monkeypatch):
    """QuestionBertCoAttentionEncoder with sentence_impl = "hip" never packs: in fp32 its levels and gradients are held to the
    float64 stock encoder under the 8x rule; under bf16 autocast (the word projection computes in bf16, the masked word level and
    the phrase level are fp32) the route still engages, and its sentence level has the bits of sentence_lstm on the phrase level
    it returned."""
    import copy
    from vqa_amd.lstm import sentence_lstm
    dev = torch.device("cuda:0")
    torch.manual_seed(13)
    B, T, D, Hd = 5, 7, 48, 64
    enc = M.QuestionBertCoAttentionEncoder(torch.nn.Embedding(40, D), D, Hd).to(dev)
    enc.sentence_impl = "hip"
    lens = torch.tensor([7, 5, 3, 2, 1])                             # sorted: the stock oracle packs with enforce_sorted
    x = torch.zeros(B, T, dtype=torch.int64)
    for b, n in enumerate(lens):
        x[b, :n] = torch.randint(1, 40, (int(n),))
    g = [torch.randn(B, T, Hd) for _ in range(3)]
    names = ("phrase_conv_pool.conv_trigram.1.weight", "sentence_lstm.weight_ih_l0", "sentence_lstm.weight_hh_l0",
             "sentence_lstm.bias_hh_l0")                             # (the word projection is the stock nn.Linear: not under test)

    def stock(dtype):
        ref = copy.deepcopy(enc).cpu().to(dtype)
        ref.sentence_impl = "stock"
        ref.zero_grad(set_to_none=True)
        levels = ref(x, lens)
        sum((lv * gl.to(dtype)).sum() for lv, gl in zip(levels, g)).backward()
        return [lv.detach() for lv in levels], {n: ref.get_parameter(n).grad for n in names}

    want64, grads64 = stock(torch.float64)
    want32, grads32 = stock(torch.float32)

    def boom(*a, **k):
        raise AssertionError("the hip route must not pack")
    monkeypatch.setattr(M, "pack_padded_sequence", boom)
    rnn = enc.sentence_lstm
    dead = ~L.live_mask(lens, T)
    for autocast in (False, True):
        enc.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            levels = enc(x.to(dev), lens.to(dev))
        assert levels[1].dtype == torch.float32 and levels[2].dtype == torch.float32
        sum((lv.float() * gl.to(dev)).sum() for lv, gl in zip(levels, g)).backward()
        assert all(bool((lv.detach().cpu()[dead] == 0).all()) for lv in levels)
        assert all(bool(torch.isfinite(enc.get_parameter(n).grad).all()) for n in names + ("word_proj.weight",))
        with torch.no_grad():
            again, xm = sentence_lstm(levels[1].detach(), lens.to(dev), rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0,
                                      rnn.bias_hh_l0)
        assert L.same_bits(again.cpu(), levels[2].detach().cpu()) and L.same_bits(xm.cpu(), levels[1].detach().cpu())
        if not autocast:
            bad = []
            for i, name in ((1, "phrases"), (2, "sentence")):
                err, bound = L.bound_check("bert " + name, levels[i].detach().cpu(), want64[i], want32[i])
                if not err <= bound:
                    bad.append((name, err, bound))
            for n in names:
                err, bound = L.bound_check(n[-24:], enc.get_parameter(n).grad.cpu(), grads64[n], grads32[n])
                if not err <= bound:
                    bad.append((n, err, bound))
            assert not bad, bad


def test_whole_net_on_both_routes_against_float64():
    from oracle.net_oracle import OracleHierarchicalCoAttentionNet
    dev = torch.device("cuda:0")
    torch.manual_seed(21)
    B, N, T, d, K = 8, 49, 12, 64, 20
    qp = dict(vocab_size=40, word_emb_dim=d, hidden_dim=d)
    ip = dict(is_trainable=False, weights_path=None)
    net = M.HierarchicalCoAttentionNet(qp, ip, K, mlp_dim=96).to(dev)
    lens = torch.tensor([12, 11, 9, 7, 6, 4, 2, 1])                  # sorted: the stock route packs
    x = torch.zeros(B, T, dtype=torch.int64)
    for b, n in enumerate(lens):
        x[b, :n] = torch.randint(1, 40, (int(n),))
    feats, labels = torch.randn(B, N, d), torch.randint(0, K, (B,))

    def oracle(dtype):
        ref = OracleHierarchicalCoAttentionNet(qp, ip, K, mlp_dim=96).to(dtype)
        ref.load_state_dict({k: v.detach().cpu().to(dtype) if v.is_floating_point() else v.cpu() for k, v in net.state_dict().items()})
        qs = list(ref.question_encoder(x, lens))
        va, qa = ref.co_attention(feats.to(dtype), qs)
        logits = ref.mlp_classify(va, qa)
        loss = torch.nn.functional.cross_entropy(logits, labels)
        loss.backward()
        return dict(loss=loss.detach().reshape(1), logits=logits.detach(), w_hh=ref.question_encoder.sentence_lstm.weight_hh_l0.grad)

    ref64, ref32 = oracle(torch.float64), oracle(torch.float32)
    got = {}
    for route in ("stock", "hip"):
        net.question_encoder.sentence_impl = route
        net.zero_grad(set_to_none=True)
        logits, loss = net.forward_features(feats.to(dev), x.to(dev), lens if route == "stock" else lens.to(dev), labels=labels.to(dev))
        loss.backward()
        got[route] = dict(loss=loss.detach().cpu().reshape(1), logits=logits.detach().cpu(),
                          w_hh=net.question_encoder.sentence_lstm.weight_hh_l0.grad.cpu())
    bad = []
    for k in ("loss", "logits", "w_hh"):
        err, bound = L.bound_check("net " + k, got["hip"][k], ref64[k], ref32[k])
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad
    assert torch.allclose(got["hip"]["logits"], got["stock"]["logits"], atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("co_attention, question_mask", [("parallel", False), ("parallel", True), ("alternating", False)])
def test_trainer_steps_on_the_hip_route_follow_the_stock_route(co_attention, question_mask):
    """Trainer(sentence_lstm="hip"): two optimisation steps of the attention model through the trainer's own step (the hot-path
    node for the parallel form) from the same weights as a stock-route trainer.  The first loss is a forward of identical
    weights (both routes are fp32-accurate: 1e-5 relative); the second follows one Adam step of lr 1e-4 on gradients that
    differ at rounding level (1e-3)."""
    import copy
    from vqa_amd import train as T
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net0 = T.build_model("attention", 100, 10, question_mask=question_mask, co_attention=co_attention)
    b = T.synthetic_batch(4, (64, 64), 26, 100, 11, seed=1)
    im, qu, la, ln = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])
    losses = {}
    for route in ("stock", "hip"):
        net = copy.deepcopy(net0).to(dev)
        tr = T.Trainer(net, 1e-4, dev, sentence_lstm=route)
        assert net.question_encoder.sentence_impl == route
        losses[route] = [float(tr.step(im.to(dev), qu.to(dev), ln, la.to(dev)).detach()) for _ in range(2)]
        assert net.question_encoder.sentence_lstm.weight_hh_l0.grad is not None
    print("trainer losses", losses)
    assert abs(losses["hip"][0] - losses["stock"][0]) <= 1e-5 * abs(losses["stock"][0])
    assert abs(losses["hip"][1] - losses["stock"][1]) <= 1e-3 * abs(losses["stock"][1])


def test_predict_cli_gives_the_same_answers_on_both_routes(tmp_path):
    """predict.py --sentence_lstm stock | hip on one checkpoint (a state_dict: it does not record the route): the same
    labels, and top-k probabilities within 1e-5 (fp32-accurate on both routes; probabilities are <= 1)."""
    import json
    from vqa_amd import predict as Pr, train as T
    torch.manual_seed(2)
    ckpt = str(tmp_path / "net.pth")
    torch.save(T.build_model("attention", 100, 10).state_dict(), ckpt)
    recs = {}
    for route in ("stock", "hip"):
        out = str(tmp_path / (route + ".jsonl"))
        summary = Pr.main(["--model", "attention", "--model_ckpt", ckpt, "--test_size", "16", "--predictions", out, "--num_cls", "10",
                           "--batch_size", "8", "--image_size", "64", "--vocab_size", "100", "--sentence_lstm", route])
        assert summary["samples"] == 16
        recs[route] = [json.loads(line) for line in open(out)]
    for a, b in zip(recs["stock"], recs["hip"]):
        assert a["index"] == b["index"] and a["label"] == b["label"]
        pa, pb = dict(zip(a["top"], a["prob"])), dict(zip(b["top"], b["prob"]))
        for k in set(pa) & set(pb):
            assert abs(pa[k] - pb[k]) <= 1e-5, (a, b)
        assert len(set(pa) & set(pb)) >= len(pa) - 1           # (a tie at the k-th place may swap the last answer)
