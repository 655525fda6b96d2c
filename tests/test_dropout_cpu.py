"""Feature dropout (include/coattn.h v0.19.0, vqa_amd.dropout, HierarchicalCoAttentionNet.feature_dropout, --dropout) as far as
it goes without a GPU: the numpy Philox of tests/_dropout.py against known answers, the oracle's own keep fraction on every
mask the GPU tests draw, threshold and scale at the edges, declarations and exports, every refusal, the seeds of data-parallel
ranks, the command line, and the CPU model."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import vqa_amd
from vqa_amd import _lib, modules as M, predict as P, train as T

from tests import _dropout as D
from tests._header import header

FUNCS = ("coattn_dropout_supported", "coattn_dropout_forward", "coattn_dropout_backward")


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    assert _hex(D.philox4x32_10(counter, key)) == want


def test_words_follow_the_counter_layout():
    """Element i is word i & 3 of block i >> 2; step and seed enter as 64-bit numbers, low word first."""
    seed, step = D.SEED_HI, 2 ** 32 + 7
    r = D.random_words(11, seed, step)
    for i in (0, 3, 4, 10):
        blk = D.philox4x32_10((i >> 2, 0, step & D.U32, step >> 32), (seed & D.U32, seed >> 32))
        assert int(r[i]) == int(blk[i & 3])
    assert not np.array_equal(D.random_words(8, seed, 7), D.random_words(8, seed, step))        # the high step word counts
    assert not np.array_equal(D.random_words(8, D.SEED, step), D.random_words(8, seed, step))   # ... and the high seed word


def test_keep_fraction_of_every_mask_the_gpu_tests_draw():
    """Within 4.5 binomial standard deviations of 1 - p (exactly 1 at p = 0)."""
    worst = 0.0
    for seed, step, n, p in D.used_masks():
        q = 1.0 - D.f32(p)
        frac = float(D.keep(n, seed, step, p).mean())
        sd = (q * (1.0 - q) / n) ** 0.5
        if sd == 0.0:
            assert frac == q, (seed, step, n, p, frac)
            continue
        z = abs(frac - q) / sd
        worst = max(worst, z)
        assert z <= 4.5, (seed, step, n, p, frac, z)
    print("keep fraction: worst deviation %.2f standard deviations over %d masks" % (worst, len(D.used_masks())))
    for n in (768, 12288):                                       # the issue's own figures: seed 1234, steps 0-2
        for step in (0, 1, 2):
            for p in (0.1, 0.5):
                frac = float(D.keep(n, 1234, step, p).mean())
                assert abs(frac - (1.0 - D.f32(p))) <= 4.5 * (D.f32(p) * (1.0 - D.f32(p)) / n) ** 0.5


def test_threshold_and_scale_at_the_edges():
    assert D.thr(0.0) == 0 and D.scale(0.0) == np.float32(1.0)
    assert D.thr(0.5) == 0x80000000 and D.scale(0.5) == np.float32(2.0)
    assert D.thr(0.1) == 0x199999A0 and D.scale(0.1) == np.float32(1.1111112)           # 0.1f = 0x1.99999ap-4
    assert D.f32(D.P_MAX) == 1.0 - 2.0 ** -24 and D.thr(D.P_MAX) == 0xFFFFFF00 and D.scale(D.P_MAX) == np.float32(2.0 ** 24)
    assert bool(D.keep(64, 1, 1, 0.0).all())                                             # r >= 0: everything kept
    x = torch.tensor([1.5, -2.0, float("inf"), float("nan"), -0.0, 1e-40])
    assert D.same_bits(D.apply(x, 1, 1, 0.0), x)                                         # times 1.0f: the same bits
    y = D.apply(torch.tensor([-2.0, float("inf"), 3.0, float("-inf")] * 8), 3, 1, D.P_MAX)   # everything dropped
    assert D.same_bits(y[0::4], torch.full((8,), -0.0)) and bool(torch.isnan(y[1::4]).all()) and bool(torch.isnan(y[3::4]).all())


def test_header_declares_exports_and_version():
    hdr = header()
    for fn in FUNCS:
        assert re.search(r"^int %s\(" % fn, hdr, re.M), fn
        assert fn in _lib.EXPORTS and hasattr(C.CDLL(_lib.LIB_PATH), fn), fn
    assert _lib.load().coattn_version() >= 1900
    for word in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "2^31 - 4", "i >> 2", "i & 3"):
        assert word in hdr, word
    assert vqa_amd.DropoutState is vqa_amd.dropout.DropoutState and vqa_amd.feature_dropout is vqa_amd.dropout.feature_dropout
    assert {"dropout", "DropoutState", "feature_dropout", "rank_seed"} <= set(vqa_amd.__all__)


def test_supported_range():
    sup = _lib.load().coattn_dropout_supported
    for n, ok in ((-1, 0), (0, 0), (1, 1), (9216, 1), (2 ** 31 - 5, 1), (2 ** 31 - 4, 1), (2 ** 31 - 3, 0), (2 ** 31, 0),
                  (2 ** 32 + 1, 0)):
        assert sup(n) == ok, n


def _err():
    return _lib.load().coattn_last_error().decode()


def test_every_refusal_is_minus_one_with_a_message_before_any_device_work():
    """Made-up pointers: a call that went on to touch them would fault."""
    fake = lambda i: 0x10000 * (i + 1)                          # noqa: E731
    fbase = dict(x0=fake(0), y0=fake(1), n=64, p=0.5, state=fake(4), advance=1, stream=None)
    bbase = dict(g=fake(0), dx=fake(1), n=64, p=0.5, state=fake(4), stream=None)

    def fwd(**kw):
        call = _lib.bind("coattn_dropout_forward", **{**fbase, **kw})
        return call.fn(*call)

    def bwd(**kw):
        call = _lib.bind("coattn_dropout_backward", **{**bbase, **kw})
        return call.fn(*call)

    shared = ((dict(p=-0.1), "outside [0, 1)"), (dict(p=1.0), "outside [0, 1)"), (dict(p=1.5), "outside [0, 1)"),
              (dict(p=float("nan")), "outside [0, 1)"), (dict(p=float("inf")), "outside [0, 1)"),
              (dict(n=0), "not supported"), (dict(n=-4), "not supported"), (dict(n=2 ** 31 - 3), "not supported"),
              (dict(n=2 ** 33), "not supported"), (dict(state=None), "null"), (dict(state=fake(4) + 2), "aligned"))
    for call in (fwd, bwd):
        for kw, word in shared:
            assert call(**kw) == -1 and word in _err(), (call.__name__, kw, _err())
    for kw, word in ((dict(x0=None), "null"), (dict(y0=None), "null"), (dict(x1=fake(2)), "go together"),
                     (dict(y1=fake(3)), "go together"), (dict(x0=fake(0) + 2), "aligned"), (dict(y0=fake(1) + 1), "aligned"),
                     (dict(x1=fake(2) + 2, y1=fake(3)), "aligned"), (dict(x1=fake(2), y1=fake(3) + 3), "aligned")):
        assert fwd(**kw) == -1 and word in _err(), (kw, _err())
    for kw, word in ((dict(g=None), "null"), (dict(dx=None), "null"), (dict(g=fake(0) + 2), "aligned"),
                     (dict(dx=fake(1) + 1), "aligned")):
        assert bwd(**kw) == -1 and word in _err(), (kw, _err())


def test_rank_seed_and_probability_check():
    assert vqa_amd.rank_seed(7, 0) == 7 and vqa_amd.rank_seed(7, 3) == 10 and vqa_amd.rank_seed(2 ** 40, 5) == 2 ** 40 + 5
    assert len({vqa_amd.rank_seed(1234, r) for r in range(8)}) == 8
    for bad in (-0.1, 1.0, 2.0, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            vqa_amd.dropout.check_p(bad)
    assert vqa_amd.dropout.check_p(0) == 0.0 and vqa_amd.dropout.check_p(0.5) == 0.5


def test_the_cli_flags_and_their_refusals():
    ap = T.build_parser()
    a = ap.parse_args([])
    assert a.dropout == 0.0 and a.dropout_seed == 0
    a = ap.parse_args(["--dropout", "0.5", "--dropout_seed", "77"])
    assert a.dropout == 0.5 and a.dropout_seed == 77
    T.check_dropout("attention", 0.5)
    T.check_dropout("baseline", 0.0, opt_lvl=1)                   # 0 is always fine
    for bad in (-0.25, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"--dropout must be in \[0, 1\)"):
            T.check_dropout("attention", bad)
    with pytest.raises(ValueError, match="co-attention models"):
        T.check_dropout("baseline", 0.5)
    with pytest.raises(ValueError, match="opt_lvl"):
        T.check_dropout("attention", 0.5, opt_lvl=1)
    for argv, word in ((["--model", "baseline", "--dropout", "0.5"], "co-attention models"),
                       (["--model", "attention", "--dropout", "0.5", "--opt_lvl", "1"], "opt_lvl"),
                       (["--model", "attention", "--dropout", "1.0"], r"\[0, 1\)")):
        with pytest.raises(ValueError, match=word):
            T.model_from_args(ap.parse_args(argv))
    with pytest.raises(ValueError, match="HierarchicalCoAttentionNet"):
        T.set_feature_dropout(torch.nn.Linear(2, 2), 0.5, 0)
    T.set_feature_dropout(torch.nn.Linear(2, 2), 0.0, 0)           # nothing to switch: fine


def test_predict_is_unchanged_and_runs_without_dropout():
    """predict.py knows nothing of dropout (it inherits the training flags and ignores this one): the model it builds has
    feature_dropout 0 and no state whatever --dropout says -- only the Trainer switches it on -- and it scores in eval mode."""
    src = open(P.__file__).read()
    assert "dropout" not in src and "model.eval()" in src
    ap = P.build_parser()
    for argv in ([], ["--dropout", "0.5", "--dropout_seed", "9"]):
        net, _ = T.model_from_args(ap.parse_args(["--model", "attention", "--model_ckpt", "x.pth"] + argv))
        assert net.feature_dropout == 0.0 and net.dropout_state is None


def _small_net():
    torch.manual_seed(5)
    return M.HierarchicalCoAttentionNet(dict(vocab_size=40, word_emb_dim=32, hidden_dim=32),
                                        dict(is_trainable=False, weights_path=None), 7, mlp_dim=24)


def test_trainer_with_feature_dropout_on_a_cpu_model_raises():
    net = _small_net()
    with pytest.raises(ValueError, match="needs a model on the GPU"):
        T.Trainer(net, 1e-4, torch.device("cpu"), feature_dropout=0.5)
    assert net.feature_dropout == 0.0 and net.dropout_state is None
    T.Trainer(net, 1e-4, torch.device("cpu"))                      # the default leaves the model as it is
    assert net.feature_dropout == 0.0 and net.dropout_state is None
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        T.set_feature_dropout(net, 1.0, 0)


def test_state_dict_keys_do_not_change():
    net = _small_net()
    keys = list(net.state_dict().keys())
    T.set_feature_dropout(net, 0.5, 3)
    assert list(net.state_dict().keys()) == keys and net.dropout_state.device.type == "cpu"
    T.set_feature_dropout(net, 0.0, 3)
    assert net.dropout_state is None and net.feature_dropout == 0.0


class _CoStub(torch.nn.Module):
    """Stands in for the HIP co-attention (which has no CPU form): mean-pooled features, three times."""
    question_mask = False

    def forward(self, x_img, x_ques, *a, **k):
        return [x_img.mean(1) for _ in range(3)], [q.mean(1) for q in x_ques]


def test_cpu_net_in_eval_gives_the_p0_bits_and_never_touches_the_state(monkeypatch):
    net = _small_net()
    net.co_attention = _CoStub()
    net.co_attention_form = "parallel"
    B, N, T_, d = 4, 9, 6, 32
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(B, N, d, generator=g)
    lens = torch.tensor([6, 5, 3, 1])
    x = torch.zeros(B, T_, dtype=torch.int64)
    for b, n in enumerate(lens):
        x[b, :n] = torch.randint(2, 40, (int(n),), generator=g)
    labels = torch.randint(0, 7, (B,), generator=g)
    net.eval()
    with torch.no_grad():
        ref = net.forward_features(feats, x, lens, labels=labels)
    T.set_feature_dropout(net, 0.5, 1234)
    words = net.dropout_state.buf.clone()
    draws = net.dropout_state.draws
    touched = []
    monkeypatch.setattr(M, "feature_dropout", lambda *a, **k: touched.append(a) or (a[0], a[1]))
    with torch.no_grad():
        got = net.forward_features(feats, x, lens, labels=labels)
    assert not touched
    monkeypatch.undo()
    assert all(D.same_bits(a, b) for a, b in zip(ref, got))
    assert torch.equal(net.dropout_state.buf, words) and net.dropout_state.draws == draws and net.dropout_state.step() == 0
    # in training the CPU net reaches the dropout, which has no CPU form
    net.train()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.forward_features(feats, x, lens, labels=labels)
    assert torch.equal(net.dropout_state.buf, words)
    # p > 0 without a state is an error, not a silent p = 0
    net.dropout_state = None
    with pytest.raises(RuntimeError, match="set_feature_dropout"):
        net.forward_features(feats, x, lens, labels=labels)
