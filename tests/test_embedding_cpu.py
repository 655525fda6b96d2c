"""The word embedding (include/coattn.h v0.18.0, vqa_amd.embedding, QuestionCoAttentionEncoder.word_impl, --word_embedding) as
far as it goes without a GPU: declarations, exports, the supported table, every argument error, the workspace size, the
documented summation order against the float64 oracle on every case of tests/test_gpu_embedding.py, the module switch on CPU
tensors, and the flag."""
import ctypes as C
import json
import os
import re

import pytest
import torch

import vqa_amd
from vqa_amd import _lib, modules as M, predict as P, train as T

from tests import _embed as E
from tests._header import args as header_args, header

FUNCS = ("coattn_embedding_supported", "coattn_embedding_workspace_bytes", "coattn_embedding_forward",
         "coattn_embedding_backward")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_header_declares_exports_constants_and_version():
    hdr = header()
    for fn in FUNCS:
        assert re.search(r"^int %s\(" % fn, hdr, re.M), fn
        assert fn in _lib.EXPORTS and hasattr(C.CDLL(_lib.LIB_PATH), fn), fn
    assert _lib.load().coattn_version() >= 1800
    for name, value in (("COATTN_IDS_I32", _lib.IDS_I32), ("COATTN_IDS_I64", _lib.IDS_I64)):
        assert int(re.search(r"^#define %s (\d+)" % name, hdr, re.M).group(1)) == value
    assert _lib.IDS_I32 != _lib.IDS_I64 and E.chunk() >= 2
    assert vqa_amd.word_embedding is vqa_amd.embedding.word_embedding and "word_embedding" in vqa_amd.__all__


def test_query_signatures_match_the_header():
    lib, hdr = _lib.load(), header()
    names = [a.split()[-1].lstrip("*") for a in header_args(hdr, "coattn_embedding_supported")]
    assert names == "n V E dtype".split() and len(lib.coattn_embedding_supported.argtypes) == 4
    names = [a.split()[-1].lstrip("*") for a in header_args(hdr, "coattn_embedding_workspace_bytes")]
    assert names == "n V E dtype ws_bwd".split() and len(lib.coattn_embedding_workspace_bytes.argtypes) == 5
    assert len(lib.coattn_embedding_forward.argtypes) == 12 and len(lib.coattn_embedding_backward.argtypes) == 13


def test_supported_table_at_its_edges():
    sup = lambda n, V, e, dt=_lib.F32: _lib.load().coattn_embedding_supported(n, V, e, dt)      # noqa: E731
    assert sup(1, 1, 4) == 1 and sup(4160, 10000, 512) == 1 and sup(4160, 10000, 2048) == 1 and sup(65536, 65536, 2048) == 1
    assert sup(160 * 26, 30522, 768) == 1                                       # BERT's table
    for e, ok in ((0, 0), (-4, 0), (2, 0), (4, 1), (6, 0), (36, 1), (510, 0), (2044, 1), (2048, 1), (2052, 0), (4096, 0)):
        assert sup(8, 8, e) == ok, e
    for n, ok in ((-1, 0), (0, 0), (1, 1), (65535, 1), (65536, 1), (65537, 0), (2 ** 32 + 1, 0)):
        assert sup(n, 8, 8) == ok, n
    for V, ok in ((-1, 0), (0, 0), (1, 1), (65536, 1), (2 ** 24, 1), (2 ** 24 + 1, 0), (2 ** 32 + 1, 0)):
        assert sup(8, V, 8) == ok, V
    assert sup(8, 8, 8, _lib.BF16) == 0 and sup(8, 8, 8, 7) == 0
    assert all(sup(n, V, e) == 1 for e in range(4, 2049, 4) for n, V in ((1, 1), (65536, 65536)))
    assert "65,536" in header() and "2^24" in header()                          # the real limits are stated


def _err():
    return _lib.load().coattn_last_error().decode()


def test_every_argument_error_is_minus_one_with_a_message_before_any_device_work():
    """Made-up pointers: a call that went on to touch them would fault; each error names what is wrong."""
    lib = _lib.load()
    fake = lambda i: 0x10000 * (i + 1)                          # noqa: E731  (16-byte aligned, never dereferenced)
    base = dict(ids=fake(0), ids_dtype=_lib.IDS_I64, n=8, V=16, E=8, padding_idx=0, dtype=_lib.F32, flags=0, stream=None)

    def fwd(**kw):
        call = _lib.bind("coattn_embedding_forward", **{**dict(base, W=fake(1), out=fake(2), bad_ids=fake(3)), **kw})
        return call.fn(*call)

    def bwd(**kw):
        call = _lib.bind("coattn_embedding_backward", **{**dict(base, g_out=fake(1), dW=fake(2), ws=None, accumulate=0), **kw})
        return call.fn(*call)

    for call in (fwd, bwd):
        for kw, word in ((dict(n=0), "non-positive"), (dict(n=-3), "non-positive"), (dict(V=0), "non-positive"),
                         (dict(E=0), "non-positive"), (dict(dtype=_lib.BF16), "dtype"), (dict(dtype=5), "dtype"),
                         (dict(E=6), "not supported"), (dict(E=2052), "not supported"), (dict(n=65537), "not supported"),
                         (dict(V=2 ** 24 + 1), "not supported"), (dict(padding_idx=16), "padding_idx"),
                         (dict(padding_idx=17), "padding_idx"), (dict(padding_idx=-2), "padding_idx"),
                         (dict(ids_dtype=2), "ids_dtype"), (dict(ids_dtype=-1), "ids_dtype"),
                         (dict(flags=_lib.FLAG_FAST16), "exact fp32"), (dict(flags=_lib.FLAG_BF16_PROJ), "exact fp32"),
                         (dict(flags=_lib.FLAG_SPLIT2), "exact fp32"), (dict(flags=_lib.FLAG_F16PAIR), "exact fp32"),
                         (dict(flags=_lib.FLAG_BF16_IN), "exact fp32"), (dict(flags=1), "exact fp32"),
                         (dict(ids=None), "null ids"), (dict(ids=fake(0) + 4), "aligned")):
            assert call(**kw) == -1 and word in _err(), (call.__name__, kw, _err())
        assert call(ids=fake(0) + 4, ids_dtype=_lib.IDS_I32, **({"W": None} if call is fwd else {"dW": None})) == -1 \
            and "null" in _err()                                # (int32 ids may sit at any 4-byte address)
    for kw in (dict(W=None), dict(out=None)):
        assert fwd(**kw) == -1 and "null" in _err(), (kw, _err())
    for kw in (dict(W=fake(1) + 4), dict(out=fake(2) + 8), dict(bad_ids=fake(3) + 2)):
        assert fwd(**kw) == -1 and "aligned" in _err(), (kw, _err())
    for kw in (dict(g_out=None), dict(dW=None)):
        assert bwd(**kw) == -1 and "null" in _err(), (kw, _err())
    for kw in (dict(g_out=fake(1) + 4), dict(dW=fake(2) + 8)):
        assert bwd(**kw) == -1 and "aligned" in _err(), (kw, _err())
    s = C.c_size_t(77)
    assert lib.coattn_embedding_workspace_bytes(8, 16, 6, _lib.F32, C.byref(s)) == -1 and "not supported" in _err()
    assert lib.coattn_embedding_workspace_bytes(0, 16, 8, _lib.F32, C.byref(s)) == -1 and "non-positive" in _err()
    assert lib.coattn_embedding_workspace_bytes(8, 16, 8, _lib.BF16, C.byref(s)) == -1 and "dtype" in _err()
    assert s.value == 77                                        # a refusal touches nothing
    assert lib.coattn_embedding_workspace_bytes(8, 16, 8, _lib.F32, None) == 0


def test_workspace_has_no_term_in_V_times_E():
    """Integers per position and per token at the most: 8 bytes for each, plus a constant."""
    for n, V, e in ((1, 1, 4), (4160, 10000, 512), (4160, 10000, 2048), (4160, 30522, 768), (65536, 65536, 2048),
                    (8, 2 ** 24, 2048)):
        b = _lib.embedding_workspace_bytes(n, V, e)
        assert 0 <= b <= 8 * (n + V) + 4096, (n, V, e, b)
        assert b == _lib.embedding_workspace_bytes(n, V, 4)      # E does not enter at all


@pytest.mark.parametrize("name", E.CASES)
def test_the_documented_order_meets_the_error_rule(name):
    """ordered_sum alone (numpy float32) against stock F.embedding's autograd in float64: the rule the GPU tests apply is
    attainable by the order the header states.  Also: absent rows and the pad row are +0, and the oracle's are zero too."""
    c = E.make_case(name)
    out64, dW64, dW32, mine = E.references(name)
    assert torch.equal(out64, c["W"].double()[c["ids"]])
    err, bound = E.bound_check(name, mine, dW64, dW32)
    assert err <= bound, (name, err, bound)
    absent = torch.ones(c["V"], dtype=torch.bool)
    absent[c["ids"][E.live(c)]] = False
    assert E.same_bits(mine[absent], torch.zeros_like(mine[absent])) and bool((dW64[absent] == 0).all())
    if c["pad"] >= 0:
        assert bool(absent[c["pad"]])
    else:
        assert not bool(absent[0]) and float(mine[0].abs().max()) > 0          # row 0 receives gradient


def test_ordered_sum_is_the_chunked_order_not_a_plain_chain():
    c = E.chunk()
    g = torch.randn(2 * c + 1, 8, generator=torch.Generator().manual_seed(1)) * 1e3
    ids = torch.full((2 * c + 1,), 2)
    got = E.ordered_sum(ids, g, 3, 0)[2]
    s = [g[k:k + c] for k in range(0, 2 * c + 1, c)]
    chain = lambda rows: __import__("functools").reduce(lambda a, b: a + b, list(rows))      # noqa: E731
    want = (chain(s[0]) + chain(s[1])) + chain(s[2])
    assert E.same_bits(got, want)
    assert E.same_bits(E.ordered_sum(ids[:1], -torch.zeros(1, 8), 3, 0)[2], -torch.zeros(8))     # one occurrence: a copy
    base = torch.randn(3, 8)
    acc = E.ordered_sum(ids, g, 3, 0, base=base)
    assert E.same_bits(acc[2], base[2] + want) and E.same_bits(acc[:2], base[:2])


def _encoder():
    torch.manual_seed(3)
    return M.QuestionCoAttentionEncoder(50, 32, 32)


def test_word_impl_defaults_to_stock_and_hip_on_cpu_is_stock_bit_for_bit():
    enc = _encoder()
    assert enc.word_impl == "stock" and M.WORD_IMPLS == ("stock", "hip")
    lens = torch.tensor([9, 6, 3, 1])
    x = torch.zeros(4, 9, dtype=torch.int64)
    for b, n in enumerate(lens):
        x[b, :n] = torch.randint(2, 50, (int(n),))
    stock = enc(x, lens)
    sum(t.sum() for t in stock).backward()
    g_stock = enc.word_embedding.weight.grad.clone()
    enc.zero_grad()
    enc.word_impl = "hip"
    hip = enc(x, lens)
    sum(t.sum() for t in hip).backward()
    for a, b in zip(stock, hip):
        assert torch.equal(a, b)
    assert torch.equal(enc.word_embedding.weight.grad, g_stock)
    enc.word_impl = "fast"
    with pytest.raises(ValueError, match="word_impl"):
        enc(x, lens)


def test_state_dict_keys_are_unchanged():
    with open(os.path.join(GOLDEN_DIR, "net_state_keys.json")) as fh:
        golden = [k for k in json.load(fh)["attention_state_dict_keys"] if k.startswith("question_encoder.")]
    assert golden
    for impl in M.WORD_IMPLS:
        enc = _encoder()
        enc.word_impl = impl
        assert ["question_encoder." + k for k in enc.state_dict().keys()] == golden
        assert not any("word_impl" in k for k in enc.state_dict())


def test_the_flag_parses_in_both_clis_and_reaches_the_model():
    for mod in (T, P):
        ap = mod.build_parser()
        assert ap.parse_args([]).word_embedding == "stock"
        assert ap.parse_args(["--word_embedding", "hip"]).word_embedding == "hip"
        with pytest.raises(SystemExit):
            ap.parse_args(["--word_embedding", "fast"])
    model = T.build_model("attention", 50, 10)
    assert model.question_encoder.word_impl == "stock"
    T.set_word_embedding(model, "hip")
    assert model.question_encoder.word_impl == "hip" and model.question_encoder.sentence_impl == "stock"
    T.Trainer(model, 1e-4, torch.device("cpu"), word_embedding="stock")
    assert model.question_encoder.word_impl == "stock"
    T.Trainer(model, 1e-4, torch.device("cpu"))                   # None: leaves the model's setting
    assert model.question_encoder.word_impl == "stock"
    T.Trainer(model, 1e-4, torch.device("cpu"), word_embedding="hip", sentence_lstm="hip")
    assert model.question_encoder.word_impl == "hip" and model.question_encoder.sentence_impl == "hip"
    with pytest.raises(ValueError, match="word_embedding"):
        T.set_word_embedding(model, "fast")
    args = T.build_parser().parse_args(["--model", "attention", "--word_embedding", "hip", "--sentence_lstm", "hip",
                                        "--question_mask", "1", "--co_attention", "alternating"])
    net, _ = T.model_from_args(args)
    assert net.question_encoder.word_impl == "hip" and net.question_encoder.sentence_impl == "hip"


def test_hip_is_refused_for_models_without_the_embedding_word_level():
    with pytest.raises(ValueError, match="Linear"):
        T.set_word_embedding(torch.nn.Linear(2, 2), "hip")
    T.set_word_embedding(torch.nn.Linear(2, 2), "stock")           # nothing to switch: fine
    baseline = T.build_model("baseline", 50, 10)
    with pytest.raises(ValueError, match=type(baseline).__name__):
        T.set_word_embedding(baseline, "hip")
    args = T.build_parser().parse_args(["--model", "baseline", "--word_embedding", "hip"])
    with pytest.raises(ValueError, match="--word_embedding hip applies"):
        T.model_from_args(args)

    class _Net(torch.nn.Module):                                  # attention_bert's encoder: its word level is the frozen BERT
        def __init__(self):
            super().__init__()
            self.question_encoder = M.QuestionBertCoAttentionEncoder(torch.nn.Embedding(50, 48), 48, 32)

    with pytest.raises(ValueError, match="_Net with QuestionBertCoAttentionEncoder"):
        T.set_word_embedding(_Net(), "hip")
