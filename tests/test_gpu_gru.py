"""The HIP question GRU (csrc/gru.hip through include/coattn_rnn.h, vqa_amd.gru, QuestionBaselineEncoder.gru_impl = "hip") on the
GPU against stock PyTorch's packed nn.GRU in float64 (tests/_gru.py), at the smallest shapes that reach each branch.

The error rule: a tensor's largest deviation from the float64 oracle may be at most 8 times the
deviation of stock fp32 nn.GRU on the CPU on the same inputs, with a floor of 16 fp32 ulps of the tensor's largest magnitude."""
import functools

import pytest
import torch

from vqa_amd import _lib, modules as M

from tests import _gru as G

pytestmark = pytest.mark.gpu

# (B, T, E, H)                      the branch it reaches
SHAPES = [(1, 1, 4, 32),            # no recurrent product at all, the smallest E
          (3, 5, 12, 32),           # E no multiple of 8; waves without work (4 forward chunks, 12 backward chunks)
          (33, 7, 300, 96),         # a row tile of one live row, three unit groups of the backward, the baseline's E on the general GEMMs
          (5, 26, 288, 288),        # a ragged share of the contraction over the waves; the fast GEMM routes
          (33, 26, 300, 1024)]      # the baseline's widths at two row tiles
CASES = [(s, "unsorted") for s in SHAPES] + [(s, "sorted_dead_tail") for s in SHAPES if s[0] >= 33]
GRADS = ("dw_ih", "dw_hh", "db_ih", "db_hh")


def _id(case):
    return "%dx%dx%dx%d-%s" % (*case[0], case[1])


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    return G.make_case(*shape, seed=sum(shape), kind=kind)


@functools.lru_cache(maxsize=None)
def _refs(shape, kind):
    c = _case(shape, kind)
    return G.oracle(c, torch.float64), G.oracle(c, torch.float32)


@functools.lru_cache(maxsize=None)
def _base(shape, kind):
    return G.run(_case(shape, kind))


def _same(a, b, keys=G.OUTPUTS):
    for k in keys:
        assert G.same_bits(a[k], b[k]), k


def _bounded(got, ref64, ref32, keys=G.OUTPUTS):
    bad = []
    for k in keys:
        err, bound = G.bound_check(k, got[k], ref64[k], ref32[k])
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_against_the_float64_oracle(case):
    _bounded(_base(*case), *_refs(*case))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_exact_zeros_past_the_lengths_and_h_last_is_the_last_live_row(case):
    c, got = _case(*case), _base(*case)
    live = G.live_mask(c["lens"], c["T"])
    for k in ("seq", "dX"):
        assert bool((got[k][~live].view(torch.int32) == 0).all()), k      # +0.0, every bit
    last = got["seq"][torch.arange(c["B"]), G.clamp(c["lens"], c["T"]) - 1]
    assert G.same_bits(last, got["h_last"])
    assert all(bool(torch.isfinite(got[k]).all()) for k in G.OUTPUTS)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_pad_rows_of_every_input_do_not_matter(case):
    c, base = _case(*case), _base(*case)
    dead = ~G.live_mask(c["lens"], c["T"])
    g = torch.Generator().manual_seed(9)
    for fill in (None, 1e30):
        X, gs = c["X"].clone(), c["g_seq"].clone()
        for t in (X, gs):
            t[dead] = (torch.randn(t[dead].shape, generator=g) * 100.0) if fill is None else fill
        if fill is not None:
            X[dead] = -fill
        _same(base, G.run(c, X=X, g_seq=gs))


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
    _same(_base(*case) if bool((ref == c["lens"]).all()) else G.run(c, lens=ref), G.run(c, lens=lo))
    _same(_base(*case), G.run(c, lens=hi))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_repeatable_and_guard_bands_intact(case):
    """Two runs into freshly NaN-filled buffers: the same bits everywhere (G.run checks every arena's margins each time)."""
    _same(_base(*case), G.run(_case(*case)))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_accumulate_adds_onto_the_parameter_gradients(case):
    """accumulate = 1 against pre-fill + the base result (summed in float64) under the gradient's own bound -- 8 times stock
    fp32's deviation, with the 16-ulp floor taken at the magnitude of the sum, the tensor that is compared."""
    c, base = _case(*case), _base(*case)
    ref64, ref32 = _refs(*case)
    g = torch.Generator().manual_seed(5)
    pre = {n: torch.randn(c[n].shape, generator=g) for n in G.PARAMS}
    got = G.run(c, accumulate=1, prefill=pre)
    bad = []
    for n in G.PARAMS:
        k = "d" + n
        want = pre[n].double() + base[k].double()
        err = float((got[k].double() - want).abs().max())
        bound = max(G.bound_check("acc " + k, base[k], ref64[k], ref32[k])[1], 16.0 * 2.0 ** -24 * float(want.abs().max()))
        print("accumulate %-6s err %.3e bound %.3e" % (k, err, bound))
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad
    _same(base, got, ("seq", "h_last", "dX"))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_optional_buffers(case):
    c, base = _case(*case), _base(*case)
    no_dx = G.run(c, dX=False)
    _same(base, no_dx, GRADS + ("seq", "h_last"))
    assert bool(torch.isnan(no_dx["dX"]).all())
    fwd_only = G.run(c, saved=False)
    _same(base, fwd_only, ("seq", "h_last"))
    assert all(bool(torch.isnan(fwd_only[k]).all()) for k in GRADS + ("dX",))
    no_hl = G.run(c, h_last=False)                                    # (the backward does not read h_last: every gradient keeps its bits)
    _same(base, no_hl, GRADS + ("seq", "dX"))
    assert bool(torch.isnan(no_hl["h_last"]).all())
    # one incoming gradient NULL: the function changes -- it is the oracle's with that gradient zero
    for name, kw in (("g_seq", dict(with_g_seq=False)), ("g_last", dict(with_g_last=False))):
        zero = torch.zeros_like(c[name])
        got = G.run(c, **kw)
        _same(base, got, ("seq", "h_last"))
        _bounded(got, G.oracle(c, torch.float64, **{name: zero}), G.oracle(c, torch.float32, **{name: zero}))
        given = G.run(c, **{name: zero})                              # NULL = a zero gradient, up to the sign of zero
        assert all(bool((given[k] == got[k]).all()) for k in GRADS + ("dX",))
    none = G.run(c, with_g_seq=False, with_g_last=False, expect_rc_bwd=-1)
    assert none["rc"] == (0, -1) and "both null" in _lib.load().coattn_last_error().decode()
    assert all(bool(torch.isnan(none[k]).all()) for k in GRADS + ("dX",))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_a_nan_stays_in_its_sample(case):
    c, base = _case(*case), _base(*case)
    b = 0                                                            # (length T: every row live)
    assert int(c["lens"][b]) == c["T"]
    t0 = min(2, c["T"] - 1)
    X = c["X"].clone()
    X[b, t0, 1] = float("nan")
    got = G.run(c, X=X)
    others = torch.arange(c["B"]) != b
    for k in ("seq", "h_last", "dX"):
        assert G.same_bits(got[k][others], base[k][others]), k
    assert bool(torch.isnan(got["seq"][b, t0:]).all()) and not bool(torch.isnan(got["seq"][b, :t0]).any())
    assert bool(torch.isnan(got["h_last"][b]).all()) and bool(torch.isnan(got["dX"][b]).any())


def test_refusals_launch_nothing():
    c = _case((3, 5, 12, 32), "unsorted")
    for flags in (_lib.FLAG_FAST16, _lib.FLAG_BF16_PROJ, _lib.FLAG_SPLIT2):
        got = G.run(c, flags=flags, expect_rc=-1)
        assert got["rc"] == (-1, -1) and "exact fp32" in _lib.load().coattn_last_error().decode()
        assert all(bool(torch.isnan(got[k]).all()) for k in G.OUTPUTS)
    bad = G.make_case(3, 5, 12, 48, seed=1)                          # H no multiple of 32
    got = G.run(bad, expect_rc=-1)
    assert got["rc"] == (-1, -1) and "not supported" in _lib.load().coattn_last_error().decode()
    assert all(bool(torch.isnan(got[k]).all()) for k in G.OUTPUTS)


# ---- the module route ------------------------------------------------------------------------------------------------------
def _encoder_oracle(enc, x, lens, g, dtype):
    """The encoder's output and every parameter gradient of sum(out * g) from a CPU copy in `dtype`, the GRU behind
    pack_padded_sequence(enforce_sorted=False) -- the stock lines restated for any order of the lengths."""
    from torch.nn.utils.rnn import pack_padded_sequence
    ref = M.QuestionBaselineEncoder(enc.vocab_size, enc.word_emb_dim, enc.hidden_dim).to(dtype)
    ref.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in enc.state_dict().items()})
    packed = pack_padded_sequence(ref.word_embedding(x), lens, batch_first=True, enforce_sorted=False)
    out = ref.embedding_layer(torch.squeeze(ref.gru(packed)[1], dim=0))
    (out * g.to(dtype)).sum().backward()
    return out.detach(), {n: p.grad for n, p in ref.named_parameters()}


def _questions(lens, T, V):
    x = torch.zeros(len(lens), T, dtype=torch.int64)
    for b, n in enumerate(lens):
        x[b, :n] = torch.randint(1, V, (int(n),))
    return x


@pytest.mark.parametrize("lens", [[9, 9, 7, 4, 2, 1], [4, 9, 1, 7, 9, 2]], ids=["sorted", "unsorted"])
def test_module_route_against_the_float64_encoder(monkeypatch, lens):
    """QuestionBaselineEncoder with gru_impl = "hip" never packs.  Sorted lengths: against a float64 copy of itself on the CPU
    (its own forward, the stock lines).  Unsorted lengths -- the stock lines would raise there -- against the float64
    enforce_sorted=False restatement."""
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    B, T, E, H = 6, 9, 20, 64
    enc = M.QuestionBaselineEncoder(40, E, H).to(dev)
    enc.gru_impl = "hip"
    lens = torch.tensor(lens)
    x = _questions(lens, T, 40)
    g = torch.randn(B, 1024)
    is_sorted = bool((lens[:-1] >= lens[1:]).all())

    def boom(*a, **k):
        raise AssertionError("the hip route must not pack")
    monkeypatch.setattr(M, "pack_padded_sequence", boom)
    assert M._hip_gru(enc, enc.word_embedding(x.to(dev)))
    out = enc(x.to(dev), lens.to(dev))                               # CUDA int64 lengths
    (out * g.to(dev)).sum().backward()
    monkeypatch.undo()
    want64, grads64 = _encoder_oracle(enc, x, lens, g, torch.float64)
    want32, grads32 = _encoder_oracle(enc, x, lens, g, torch.float32)
    if is_sorted:                                                    # the float64 copy's own forward: the stock lines
        import copy
        ref = copy.deepcopy(enc).cpu().double()
        ref.gru_impl = "stock"
        ref.zero_grad(set_to_none=True)
        own = ref(x, lens)
        (own * g.double()).sum().backward()
        close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())      # noqa: E731
        assert close(own.detach(), want64)                           # (the restatement is the stock lines, in float64)
        assert all(close(p.grad, grads64[n]) for n, p in ref.named_parameters())
    else:
        stock = M.QuestionBaselineEncoder(40, E, H)
        with pytest.raises(RuntimeError, match="sorted"):
            stock(x, lens)
    bad = []
    err, bound = G.bound_check("encoder", out.detach().cpu(), want64, want32)
    if not err <= bound:
        bad.append(("out", err, bound))
    for n, p in enc.named_parameters():
        err, bound = G.bound_check(n[-24:], p.grad.cpu(), grads64[n], grads32[n])
        if not err <= bound:
            bad.append((n, err, bound))
    assert not bad, bad


def test_trainer_steps_on_the_hip_route_follow_the_stock_route(monkeypatch):
    """Trainer(question_gru="hip"): two optimisation steps of the baseline model through the trainer's own step from the same
    weights as a stock-route trainer.  The first loss is a forward of identical weights (both routes are fp32-accurate: 1e-5
    relative); the second follows one Adam step of lr 1e-4 on gradients that differ at rounding level (1e-3).  The baseline's
    MLP holds nn.Dropout(0.5): torch is seeded identically before each route's steps, so both draw the same masks."""
    import copy
    from vqa_amd import train as T
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net0 = T.build_model("baseline", 100, 10)
    b = T.synthetic_batch(4, (64, 64), 26, 100, 11, seed=1)
    im, qu, la, ln = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])
    losses = {}
    for route in ("stock", "hip"):
        net = copy.deepcopy(net0).to(dev)
        tr = T.Trainer(net, 1e-4, dev, question_gru=route)
        assert net.question_encoder.gru_impl == route
        if route == "hip":                                           # (the route is really taken: packing would raise)
            monkeypatch.setattr(M, "pack_padded_sequence", lambda *a, **k: pytest.fail("the hip route must not pack"))
        torch.manual_seed(7)
        losses[route] = [float(tr.step(im.to(dev), qu.to(dev), ln, la.to(dev)).detach()) for _ in range(2)]
        assert net.question_encoder.gru.weight_hh_l0.grad is not None
    print("trainer losses", losses)
    assert abs(losses["hip"][0] - losses["stock"][0]) <= 1e-5 * abs(losses["stock"][0])
    assert abs(losses["hip"][1] - losses["stock"][1]) <= 1e-3 * abs(losses["stock"][1])


def test_predict_cli_gives_the_same_answers_on_both_routes(tmp_path):
    """predict.py --question_gru stock | hip on one checkpoint (a state_dict: it does not record the route): the same labels,
    and top-k probabilities within 1e-5 (fp32-accurate on both routes; probabilities are <= 1)."""
    import json
    from vqa_amd import predict as Pr, train as T
    torch.manual_seed(2)
    ckpt = str(tmp_path / "net.pth")
    torch.save(T.build_model("baseline", 100, 10).state_dict(), ckpt)
    recs = {}
    for route in ("stock", "hip"):
        out = str(tmp_path / (route + ".jsonl"))
        summary = Pr.main(["--model", "baseline", "--model_ckpt", ckpt, "--test_size", "16", "--predictions", out, "--num_cls", "10",
                           "--batch_size", "8", "--image_size", "64", "--vocab_size", "100", "--question_gru", route])
        assert summary["samples"] == 16
        recs[route] = [json.loads(line) for line in open(out)]
    for a, b in zip(recs["stock"], recs["hip"]):
        assert a["index"] == b["index"] and a["label"] == b["label"]
        pa, pb = dict(zip(a["top"], a["prob"])), dict(zip(b["top"], b["prob"]))
        for k in set(pa) & set(pb):
            assert abs(pa[k] - pb[k]) <= 1e-5, (a, b)
        assert len(set(pa) & set(pb)) >= len(pa) - 1           # (a tie at the k-th place may swap the last answer)
