"""The question GRU (include/coattn_rnn.h v0.25.0, vqa_amd.gru, QuestionBaselineEncoder.gru_impl, --question_gru) as far as it
goes without a GPU: the third header against its table, the other two tables untouched, the supported table, every argument
error, the workspace sizes, the oracle of tests/test_gpu_gru.py pinned against the header's formulas written out, the module
switch on the routes that must stay stock, and the flag."""
import ctypes as C
import os
import re

import pytest
import torch

import vqa_amd
from vqa_amd import _lib, modules as M, predict as P, train as T

from tests import _gru as G
from tests._header import args as header_args, declared

FUNCS = ("coattn_gru_supported", "coattn_gru_workspace_bytes", "coattn_gru_forward", "coattn_gru_backward")
EXT_TAIL = ("coattn_bn_eval_supported", "coattn_bn_eval_forward", "coattn_conv1_bn_eval_supported", "coattn_conv1_bn_eval_forward",
            "coattn_bn_eval_probe")                                 # what 0.24.0 added: still the end of the second table
INCLUDE = os.path.join(os.path.dirname(_lib.CSRC.rstrip("/")), "..", "include")
CTYPES = {"int": C.c_int, "size_t*": C.POINTER(C.c_size_t)}


def _hdr(name):
    return open(os.path.join(INCLUDE, name)).read()


def test_the_third_header_the_table_and_the_library_agree():
    lib, rnn = _lib.load(), _hdr("coattn_rnn.h")
    assert lib.coattn_version() >= 2500
    decl = declared(rnn)
    assert list(decl) == list(_lib.RNN_SIGNATURES) == list(_lib.RNN_EXPORTS) == list(FUNCS)
    assert all(ret == "int" for ret in decl.values()) and not _lib.RNN_RESTYPES
    for name in FUNCS:
        want = [a.rsplit(" ", 1) for a in header_args(rnn, name)]
        sig = _lib.RNN_SIGNATURES[name]
        assert [n for n, _ in sig] == [n for _, n in want], name
        for (n, ctype), (ctext, _) in zip(sig, want):
            if ctext in CTYPES:
                assert ctype is CTYPES[ctext], (name, n, ctext)
            elif "coattn_gru_param_grads*" in ctext:
                assert ctype is C.POINTER(_lib.GruParamGrads), (name, n)
            elif "coattn_gru_params*" in ctext:
                assert ctype is C.POINTER(_lib.GruParams), (name, n)
            else:
                assert "*" in ctext and ctype is C.c_void_p, (name, n, ctext)
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [t for _, t in sig] and fn.restype is C.c_int, name
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    assert [a.split()[-1] for a in header_args(rnn, "coattn_gru_forward")] == \
        "X len p seq_out h_last saved ws B T E H dtype flags stream".split()
    assert [a.split()[-1] for a in header_args(rnn, "coattn_gru_backward")] == \
        "X len p saved g_seq g_last dX pg accumulate ws B T E H dtype flags stream".split()
    assert re.search(r"v0\.25\.0", rnn) and "SAME VALUES AS THE FORWARD" in rnn
    assert vqa_amd.question_gru is vqa_amd.gru.question_gru and {"gru", "question_gru"} <= set(vqa_amd.__all__)


def test_the_other_two_headers_and_tables_are_unchanged():
    first, ext = declared(_hdr("coattn.h")), declared(_hdr("coattn_ext.h"))
    assert len(first) == len(_lib.SIGNATURES) == len(_lib.EXPORTS) == 78 and set(first) == set(_lib.SIGNATURES)
    assert _lib.EXPORTS == tuple(_lib.SIGNATURES) and _lib.EXPORTS[0] == "coattn_version" and _lib.EXPORTS[-1] == "coattn_p2p_all_gather"
    assert list(ext) == list(_lib.EXT_SIGNATURES) == list(_lib.EXT_EXPORTS) and tuple(ext)[-5:] == EXT_TAIL
    assert not (set(FUNCS) & set(first)) and not (set(FUNCS) & set(ext))
    assert not any("gru" in n for n in list(_lib.SIGNATURES) + list(_lib.EXT_SIGNATURES))
    # the LSTM's gradient stays required: the new nullable names are the GRU's own
    assert "g_out" not in _lib._DEFAULTS and {"h_last", "g_seq", "g_last"} <= set(_lib._DEFAULTS)
    with pytest.raises(TypeError, match="g_out"):
        _lib.bind("coattn_lstm_backward", X=0, len=0, p=_lib.LstmParams(), out=None, saved=0, pg=_lib.LstmParamGrads(), accumulate=0, ws=0,
                  B=1, T=1, E=32, H=32, dtype=0, flags=0, stream=0)


@pytest.mark.parametrize("struct, cls", [("coattn_gru_params", _lib.GruParams), ("coattn_gru_param_grads", _lib.GruParamGrads)])
def test_structs_follow_the_header(struct, cls):
    body = re.search(r"typedef struct %s\s*\{([^}]*)\}\s*%s;" % (struct, struct), _hdr("coattn_rnn.h")).group(1)
    fields = [f.strip().lstrip("*") for f in re.sub(r"\b(const|void)\b", "", body).replace(";", ",").split(",") if f.strip()]
    assert fields == [n for n, _ in cls._fields_] == ["w_ih", "w_hh", "b_ih", "b_hh"]
    assert all(t is C.c_void_p for _, t in cls._fields_)


def test_bind_and_replace_serve_the_third_table():
    call = _lib.bind("coattn_gru_forward", X=1 << 20, len=1 << 21, p=_lib.GruParams(), seq_out=1 << 22, ws=1 << 23, B=2, T=3, E=4,
                     H=32, dtype=_lib.F32, flags=0)
    sig = _lib.RNN_SIGNATURES["coattn_gru_forward"]
    assert call.name == "coattn_gru_forward" and len(call) == len(sig) - 1           # (stream left for the call)
    names = [n for n, _ in sig]
    assert call[names.index("h_last")] is None and call[names.index("saved")] is None
    again = call.replace(B=5, h_last=1 << 24)
    assert again[names.index("B")] == 5 and again[names.index("h_last")].value == 1 << 24
    bwd = _lib.bind("coattn_gru_backward", X=1 << 20, len=1 << 21, p=_lib.GruParams(), saved=1 << 22, pg=_lib.GruParamGrads(),
                    accumulate=0, ws=1 << 23, B=2, T=3, E=4, H=32, dtype=_lib.F32, flags=0)
    names = [n for n, _ in _lib.RNN_SIGNATURES["coattn_gru_backward"]]
    assert all(bwd[names.index(n)] is None for n in ("g_seq", "g_last", "dX"))
    with pytest.raises(TypeError, match="no argument"):
        _lib.bind("coattn_gru_forward", out=0)
    with pytest.raises(TypeError, match="missing argument 'seq_out'"):
        _lib.bind("coattn_gru_forward", X=0, len=0, p=_lib.GruParams(), ws=0, B=1, T=1, E=4, H=32, dtype=0, flags=0)


def test_supported_table_at_its_limits():
    sup = lambda B, T, E, H, dt=_lib.F32: _lib.load().coattn_gru_supported(B, T, E, H, dt)      # noqa: E731
    assert sup(1, 1, 4, 32) == 1 and sup(160, 26, 300, 1024) == 1 and sup(1, 64, 2048, 2048) == 1
    for e, ok in ((0, 0), (-4, 0), (3, 0), (4, 1), (6, 0), (12, 1), (300, 1), (301, 0), (302, 0), (2048, 1), (2052, 0)):
        assert sup(4, 8, e, 64) == ok, e
    for h, ok in ((0, 0), (-32, 0), (16, 0), (31, 0), (32, 1), (48, 0), (1024, 1), (2048, 1), (2080, 0)):
        assert sup(4, 8, 64, h) == ok, h
    for t, ok in ((0, 0), (1, 1), (64, 1), (65, 0)):
        assert sup(4, t, 64, 64) == ok, t
    assert sup(0, 8, 64, 64) == 0 and sup(1, 8, 64, 64) == 1 and sup(100000, 8, 64, 64) == 1
    assert sup(4, 8, 64, 64, _lib.BF16) == 0
    # B T 3 max(E, H) < 2^31, from both sides and for either width
    B = (2 ** 31) // (64 * 3 * 2048)                                  # 5461: B 64 3 2048 = 2^31 - 3 * 2^17
    assert sup(B, 64, 2048, 32) == 1 and sup(B + 1, 64, 2048, 32) == 0
    assert sup(B, 64, 4, 2048) == 1 and sup(B + 1, 64, 4, 2048) == 0
    assert all(sup(33, 7, e, h) == 1 for e in range(4, 2049, 4) for h in (32, 1024, 2048))
    assert all(sup(33, 7, e, h) == 1 for h in range(32, 2049, 32) for e in (4, 300, 2048))
    assert vqa_amd.gru.supported(160, 26, 300, 1024) and not vqa_amd.gru.supported(160, 26, 301, 1024)


def _err():
    return _lib.load().coattn_last_error().decode()


def test_every_argument_error_is_minus_one_with_a_message_before_any_device_work():
    """Made-up pointers: a call that went on to touch them would fault; each error names its argument."""
    lib = _lib.load()
    fake = lambda i: C.c_void_p(0x10000 * (i + 1))              # noqa: E731  (16-byte aligned, never dereferenced)
    p = _lib.GruParams(*[0x100000 * (i + 1) for i in range(4)])
    pg = _lib.GruParamGrads(*[0x200000 * (i + 1) for i in range(4)])
    dims = dict(B=4, T=8, E=12, H=64, dtype=_lib.F32, flags=0)

    def fwd(X=fake(0), ln=fake(1), pp=p, seq=fake(2), hl=fake(3), saved=fake(4), ws=fake(5), **kw):
        d = dict(dims, **kw)
        return lib.coattn_gru_forward(X, ln, C.byref(pp) if pp is not None else None, seq, hl, saved, ws, d["B"], d["T"], d["E"],
                                      d["H"], d["dtype"], d["flags"], None)

    def bwd(X=fake(0), ln=fake(1), pp=p, saved=fake(4), gs=fake(6), gl=fake(7), dX=fake(8), gg=pg, ws=fake(5), **kw):
        d = dict(dims, **kw)
        return lib.coattn_gru_backward(X, ln, C.byref(pp) if pp is not None else None, saved, gs, gl, dX,
                                       C.byref(gg) if gg is not None else None, 0, ws, d["B"], d["T"], d["E"], d["H"], d["dtype"],
                                       d["flags"], None)

    for call in (fwd, bwd):
        for kw, word in ((dict(B=0), "non-positive"), (dict(T=-1), "non-positive"), (dict(E=0), "non-positive"),
                         (dict(H=0), "non-positive"), (dict(dtype=_lib.BF16), "dtype"), (dict(T=65), "not supported"),
                         (dict(E=6), "not supported"), (dict(E=2052), "not supported"), (dict(H=48), "not supported"),
                         (dict(H=16), "not supported"), (dict(H=2080), "not supported"),
                         (dict(B=5462, T=64, E=2048), "not supported"),
                         (dict(flags=_lib.FLAG_FAST16), "exact fp32"), (dict(flags=_lib.FLAG_BF16_PROJ), "exact fp32"),
                         (dict(flags=_lib.FLAG_SPLIT2), "exact fp32"), (dict(flags=_lib.FLAG_F16PAIR), "exact fp32"),
                         (dict(flags=_lib.FLAG_BF16_IN), "exact fp32"), (dict(flags=1), "exact fp32")):
            assert call(**kw) == -1 and word in _err(), (call.__name__, kw, _err())
        for kw in (dict(X=None), dict(ln=None), dict(pp=None), dict(ws=None)):
            assert call(**kw) == -1 and "null" in _err(), (call.__name__, kw, _err())
        assert call(pp=_lib.GruParams(0x100000, 0, 0x300000, 0x400000)) == -1 and "null parameter" in _err()
        for kw in (dict(X=C.c_void_p(0x10004)), dict(ws=C.c_void_p(0x10008)), dict(ln=C.c_void_p(0x20002)),
                   dict(saved=C.c_void_p(0x50004))):
            assert call(**kw) == -1 and "aligned" in _err(), (call.__name__, kw, _err())
    assert fwd(seq=None) == -1 and "null" in _err() and "seq_out" in _err()
    assert fwd(seq=C.c_void_p(0x30004)) == -1 and "aligned" in _err()
    assert fwd(hl=C.c_void_p(0x40004)) == -1 and "aligned" in _err()
    for kw in (dict(saved=None), dict(gg=None)):
        assert bwd(**kw) == -1 and "null" in _err(), (kw, _err())
    assert bwd(gs=None, gl=None) == -1 and "both null" in _err()
    for kw in (dict(gs=C.c_void_p(0x70004)), dict(gl=C.c_void_p(0x80004)), dict(dX=C.c_void_p(0x90004))):
        assert bwd(**kw) == -1 and "aligned" in _err(), (kw, _err())
    assert bwd(gg=_lib.GruParamGrads(0x200000, 0x400000, 0, 0x800000)) == -1 and "null parameter gradient" in _err()
    assert bwd(gg=_lib.GruParamGrads(0x200004, 0x400000, 0x600000, 0x800000)) == -1 and "aligned" in _err()
    s = C.c_size_t()
    assert lib.coattn_gru_workspace_bytes(4, 65, 64, 64, _lib.F32, C.byref(s), None, None) == -1 and "not supported" in _err()
    assert lib.coattn_gru_workspace_bytes(0, 8, 64, 64, _lib.F32, C.byref(s), None, None) == -1 and "non-positive" in _err()
    assert lib.coattn_gru_workspace_bytes(4, 8, 64, 64, _lib.BF16, C.byref(s), None, None) == -1 and "dtype" in _err()


def test_workspace_sizes_are_positive_and_grow_with_B_and_T():
    base = _lib.gru_workspace_bytes(4, 8, 12, 64)
    assert all(v > 0 for v in base)
    for B, T in ((8, 8), (4, 16), (160, 26)):
        big = _lib.gru_workspace_bytes(B, T, 12, 64)
        assert all(b > a for a, b in zip(base, big)), (B, T, base, big)
    # saved: the activated gates [B][T][3H], hn and h_prev [B][T][H] each
    assert _lib.gru_workspace_bytes(160, 26, 300, 1024)[0] == 5 * 160 * 26 * 1024 * 4
    # the forward's workspace holds G_x [B T][3H] and room for the weight image
    assert _lib.gru_workspace_bytes(160, 26, 300, 1024)[1] >= 3 * 160 * 26 * 1024 * 4


@pytest.mark.parametrize("B, T, E, H", [(1, 1, 4, 32), (3, 5, 12, 32), (9, 7, 20, 96)])
def test_the_oracle_is_the_unpacked_recurrence(B, T, E, H):
    """The packed stock oracle equals the formulas of include/coattn_rnn.h written out in float64 -- unsorted lengths, 7.0 in the
    pad rows -- for seq, h_last and all gradients, within 1e-12 of the largest magnitude."""
    c = G.make_case(B, T, E, H, seed=B + T)
    if B > 2:                                                   # [T, 1, at least 2, ...]: not sorted (T > 2 here)
        c["lens"][2] = max(int(c["lens"][2]), 2)
        assert bool((c["lens"][:-1] < c["lens"][1:]).any())
        assert bool((c["X"][~G.live_mask(c["lens"], T)] == G.PAD).all())
    want, got = G.oracle(c), G.unpacked_reference(c)
    for k in G.OUTPUTS:
        err = float((want[k] - got[k]).abs().max()) / max(float(want[k].abs().max()), 1e-300)
        print("oracle pin %-9s %.2e" % (k, err))
        assert err <= 1e-12, (k, err)
    dead = ~G.live_mask(c["lens"], T)
    for k in ("seq", "dX"):
        assert bool((want[k][dead] == 0).all())
    last = want["seq"][torch.arange(B), G.clamp(c["lens"], T) - 1]
    assert torch.equal(last, want["h_last"])                    # h_last is the sequence's row len - 1


def _encoder(E=12, H=32, **gru_kw):
    torch.manual_seed(3)
    enc = M.QuestionBaselineEncoder(50, E, H)
    if gru_kw:
        enc.gru = torch.nn.GRU(E, H, **gru_kw)
    return enc


def _questions(lens, T=9):
    x = torch.zeros(len(lens), T, dtype=torch.int64)
    for b, n in enumerate(lens):
        x[b, :n] = torch.randint(2, 50, (int(n),))
    return x


def test_gru_impl_stays_stock_without_touching_the_new_symbols(monkeypatch):
    """CPU tensors, gru_impl = "stock" and an nn.GRU of two layers take the stock lines bit for bit, and none of them binds a
    0.25.0 symbol."""
    bound = []
    real = _lib.bind
    monkeypatch.setattr(_lib, "bind", lambda name, **kw: (bound.append(name), real(name, **kw))[1])
    lens = torch.tensor([9, 6, 3, 1])                             # (the stock lines want sorted lengths)
    x = _questions(lens)
    enc = _encoder()
    assert enc.gru_impl == "stock" and M.GRU_IMPLS == ("stock", "hip")
    stock = enc(x, lens)
    assert not M._hip_gru(enc, enc.word_embedding(x))
    enc.gru_impl = "hip"
    assert not M._hip_gru(enc, enc.word_embedding(x))             # CPU tensors
    assert torch.equal(enc(x, lens), stock)
    two = _encoder(num_layers=2)
    two.gru_impl = "hip"
    emb = two.word_embedding(x)
    assert not M._hip_gru(two, emb)
    hidden = two.gru(torch.nn.utils.rnn.pack_padded_sequence(emb, lens, batch_first=True))[1]
    got = two(x, lens)                                            # the stock lines as they are: nn.GRU's hidden [layers, B, H]
    assert got.shape == (2, 4, 1024) and torch.equal(got, two.embedding_layer(hidden))
    assert not [n for n in bound if n in _lib.RNN_SIGNATURES], bound
    enc.gru_impl = "fast"
    with pytest.raises(ValueError, match="gru_impl"):
        enc(x, lens)


@pytest.mark.parametrize("kw", [dict(num_layers=2), dict(bidirectional=True), dict(bias=False)])
def test_other_grus_are_not_eligible_whatever_the_tensor(kw):
    """The predicate's GRU conditions, checked on a stand-in for a CUDA tensor (no GPU here): only is_cuda, dtype and shape
    are read before the GRU is looked at."""
    class Cuda:
        is_cuda, dtype, shape = True, torch.float32, (4, 9, 12)

        def is_floating_point(self):
            return True
    enc = _encoder(**kw)
    enc.gru_impl = "hip"
    assert M._hip_gru(enc, Cuda()) is False
    ok = _encoder()
    ok.gru_impl = "hip"
    assert M._hip_gru(ok, Cuda()) is True                         # one layer, one direction, bias, no dropout, supported shape
    ok.gru_impl = "stock"
    assert M._hip_gru(ok, Cuda()) is False

    class Half(Cuda):
        dtype = torch.float16
    ok.gru_impl = "hip"
    assert M._hip_gru(ok, Half()) is False                        # no autocast: other dtypes stay stock

    class Odd(Cuda):
        shape = (4, 65, 12)
    assert M._hip_gru(ok, Odd()) is False                         # T = 65: not supported


def test_state_dict_keys_are_unchanged():
    want = ["word_embedding.0.weight", "gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0",
            "embedding_layer.0.weight", "embedding_layer.0.bias"]   # the reference class's modules, in its order
    for impl in M.GRU_IMPLS:
        enc = _encoder()
        enc.gru_impl = impl
        assert list(enc.state_dict().keys()) == want
    net = T.build_model("baseline", 50, 10)
    keys = list(net.state_dict().keys())
    assert [k for k in keys if k.startswith("question_encoder.")] == ["question_encoder." + k for k in want]
    assert not any("gru_impl" in k for k in keys)
    T.set_question_gru(net, "hip")
    assert list(net.state_dict().keys()) == keys
    # the baseline's encoder has no other switch: --sentence_lstm hip / --word_embedding hip stay errors for it
    assert not hasattr(net.question_encoder, "sentence_impl") and not hasattr(net.question_encoder, "word_impl")


def test_the_flag_parses_in_both_clis_and_reaches_the_model():
    assert T.QUESTION_GRUS == ("stock", "hip")
    for mod in (T, P):
        ap = mod.build_parser()
        assert ap.parse_args([]).question_gru == "stock"
        assert ap.parse_args(["--question_gru", "hip"]).question_gru == "hip"
        with pytest.raises(SystemExit):
            ap.parse_args(["--question_gru", "fast"])
    model = T.build_model("baseline", 50, 10)
    assert model.question_encoder.gru_impl == "stock"
    T.set_question_gru(model, "hip")
    assert model.question_encoder.gru_impl == "hip"
    T.Trainer(model, 1e-4, torch.device("cpu"), question_gru="stock")
    assert model.question_encoder.gru_impl == "stock"
    T.Trainer(model, 1e-4, torch.device("cpu"))                   # None: leaves the model's setting
    assert model.question_encoder.gru_impl == "stock"
    with pytest.raises(ValueError, match="question_gru"):
        T.set_question_gru(model, "fast")
    args = T.build_parser().parse_args(["--model", "baseline", "--question_gru", "hip"])
    net, _ = T.model_from_args(args)
    assert net.question_encoder.gru_impl == "hip"
    net, _ = T.model_from_args(T.build_parser().parse_args(["--model", "baseline"]))
    assert net.question_encoder.gru_impl == "stock"


def test_the_attention_model_refuses_the_flag_by_name():
    att = T.build_model("attention", 50, 10)
    T.set_question_gru(att, "stock")                              # nothing to switch, nothing to refuse
    with pytest.raises(ValueError, match="HierarchicalCoAttentionNet"):
        T.set_question_gru(att, "hip")
    with pytest.raises(ValueError, match="HierarchicalCoAttentionNet"):
        T.Trainer(att, 1e-4, torch.device("cpu"), question_gru="hip")
    with pytest.raises(ValueError, match="--question_gru hip applies to the baseline model .*HierarchicalCoAttentionNet"):
        T.model_from_args(T.build_parser().parse_args(["--model", "attention", "--question_gru", "hip"]))
    with pytest.raises(ValueError, match="Linear"):
        T.set_question_gru(torch.nn.Linear(2, 2), "hip")
    # and the baseline still refuses the co-attention encoders' switches
    base = T.build_model("baseline", 50, 10)
    with pytest.raises(ValueError):
        T.set_sentence_lstm(base, "hip")
    with pytest.raises(ValueError):
        T.set_word_embedding(base, "hip")
