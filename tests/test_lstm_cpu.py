"""The sentence LSTM (include/coattn.h v0.17.0, vqa_amd.lstm, QuestionCoAttentionEncoder.sentence_impl, --sentence_lstm) as far
as it goes without a GPU: declarations, exports, the supported table, every argument error, the workspace sizes, the oracle
of tests/test_gpu_lstm.py pinned against the recurrence written out, the module switch on CPU tensors, and the flag."""
import ctypes as C
import json
import os
import re

import pytest
import torch

import vqa_amd
from vqa_amd import _lib, modules as M, predict as P, train as T

from tests import _lstm as L
from tests._header import args as header_args, header

FUNCS = ("coattn_lstm_supported", "coattn_lstm_workspace_bytes", "coattn_lstm_forward", "coattn_lstm_backward")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_header_declares_exports_and_version():
    hdr = header()
    for fn in FUNCS:
        assert re.search(r"^int %s\(" % fn, hdr, re.M), fn
        assert fn in _lib.EXPORTS and hasattr(C.CDLL(_lib.LIB_PATH), fn), fn
    assert _lib.load().coattn_version() >= 1700
    assert vqa_amd.sentence_lstm is vqa_amd.lstm.sentence_lstm and "sentence_lstm" in vqa_amd.__all__
    names = [a.split()[-1].lstrip("*") for a in header_args(hdr, "coattn_lstm_forward")]
    assert names == "X len p out x_masked saved ws B T E H dtype flags stream".split()
    names = [a.split()[-1].lstrip("*") for a in header_args(hdr, "coattn_lstm_backward")]
    assert names == "X len p out saved g_out g_xmasked dX pg accumulate ws B T E H dtype flags stream".split()
    assert len(_lib.load().coattn_lstm_forward.argtypes) == 14 and len(_lib.load().coattn_lstm_backward.argtypes) == 18
    assert "SAME VALUES AS THE FORWARD" in hdr                  # the backward's lengths: stated as the *_len forms do


@pytest.mark.parametrize("struct, cls", [("coattn_lstm_params", _lib.LstmParams), ("coattn_lstm_param_grads", _lib.LstmParamGrads)])
def test_structs_follow_the_header(struct, cls):
    body = re.search(r"typedef struct %s\s*\{([^}]*)\}\s*%s;" % (struct, struct), header()).group(1)
    fields = [f.strip().lstrip("*") for f in re.sub(r"\b(const|void)\b", "", body).replace(";", ",").split(",") if f.strip()]
    assert fields == [n for n, _ in cls._fields_] == ["w_ih", "w_hh", "b_ih", "b_hh"]
    assert all(t is C.c_void_p for _, t in cls._fields_)


def test_supported_table_at_its_edges():
    sup = lambda B, T, E, H, dt=_lib.F32: _lib.load().coattn_lstm_supported(B, T, E, H, dt)      # noqa: E731
    assert sup(1, 1, 32, 32) == 1 and sup(160, 26, 512, 512) == 1 and sup(1, 64, 2048, 2048) == 1
    for v, ok in ((31, 0), (32, 1), (2048, 1), (2080, 0), (48, 0), (0, 0), (-32, 0)):
        assert sup(4, 8, v, 64) == ok and sup(4, 8, 64, v) == ok, v
    for t, ok in ((0, 0), (1, 1), (64, 1), (65, 0)):
        assert sup(4, t, 64, 64) == ok, t
    assert sup(0, 8, 64, 64) == 0 and sup(1, 8, 64, 64) == 1 and sup(100000, 8, 64, 64) == 1
    assert sup(4, 8, 64, 64, _lib.BF16) == 0
    for B, T in ((1, 1), (33, 7), (1000, 64)):                  # every E, H multiple of 32 up to 2048
        assert all(sup(B, T, e, h) == 1 for e in range(32, 2049, 32) for h in (32, 1024, 2048))
        assert all(sup(B, T, e, h) == 1 for h in range(32, 2049, 32) for e in (32, 1024, 2048))


def _err():
    return _lib.load().coattn_last_error().decode()


def test_every_argument_error_is_minus_one_with_a_message_before_any_device_work():
    """Made-up pointers: a call that went on to touch them would fault; each error names its argument."""
    lib = _lib.load()
    fake = lambda i: C.c_void_p(0x10000 * (i + 1))              # noqa: E731  (16-byte aligned, never dereferenced)
    p = _lib.LstmParams(*[0x100000 * (i + 1) for i in range(4)])
    pg = _lib.LstmParamGrads(*[0x200000 * (i + 1) for i in range(4)])
    dims = dict(B=4, T=8, E=64, H=64, dtype=_lib.F32, flags=0)

    def fwd(X=fake(0), ln=fake(1), pp=p, out=fake(2), xm=fake(3), saved=fake(4), ws=fake(5), **kw):
        d = dict(dims, **kw)
        return lib.coattn_lstm_forward(X, ln, C.byref(pp) if pp is not None else None, out, xm, saved, ws, d["B"], d["T"], d["E"],
                                       d["H"], d["dtype"], d["flags"], None)

    def bwd(X=fake(0), ln=fake(1), pp=p, out=fake(2), saved=fake(4), g=fake(6), gx=fake(7), dX=fake(8), gg=pg, ws=fake(5), **kw):
        d = dict(dims, **kw)
        return lib.coattn_lstm_backward(X, ln, C.byref(pp) if pp is not None else None, out, saved, g, gx, dX,
                                        C.byref(gg) if gg is not None else None, 0, ws, d["B"], d["T"], d["E"], d["H"], d["dtype"],
                                        d["flags"], None)

    for call in (fwd, bwd):
        for kw, word in ((dict(B=0), "non-positive"), (dict(T=-1), "non-positive"), (dict(E=0), "non-positive"),
                         (dict(H=0), "non-positive"), (dict(dtype=_lib.BF16), "dtype"), (dict(T=65), "not supported"),
                         (dict(E=48), "not supported"), (dict(H=2080), "not supported"),
                         (dict(flags=_lib.FLAG_FAST16), "exact fp32"), (dict(flags=_lib.FLAG_BF16_PROJ), "exact fp32"),
                         (dict(flags=_lib.FLAG_SPLIT2), "exact fp32"), (dict(flags=_lib.FLAG_F16PAIR), "exact fp32"),
                         (dict(flags=_lib.FLAG_BF16_IN), "exact fp32"), (dict(flags=1), "exact fp32")):
            assert call(**kw) == -1 and word in _err(), (call.__name__, kw, _err())
        for kw in (dict(X=None), dict(ln=None), dict(pp=None), dict(ws=None)):
            assert call(**kw) == -1 and "null" in _err(), (call.__name__, kw, _err())
        assert call(pp=_lib.LstmParams(0x100000, 0, 0x300000, 0x400000)) == -1 and "null parameter" in _err()
        assert call(X=C.c_void_p(0x10004)) == -1 and "aligned" in _err()
    assert fwd(out=None) == -1 and "null" in _err()
    for kw in (dict(saved=None), dict(g=None), dict(gg=None)):
        assert bwd(**kw) == -1 and "null" in _err(), (kw, _err())
    # the backward's `out` is reserved and never read: NULL passes the NULL checks (the error reported is the next check's)
    assert bwd(out=None, X=C.c_void_p(0x10004)) == -1 and "aligned" in _err()
    assert bwd(gg=_lib.LstmParamGrads(0x200000, 0x400000, 0, 0x800000)) == -1 and "null parameter gradient" in _err()
    s = C.c_size_t()
    assert lib.coattn_lstm_workspace_bytes(4, 65, 64, 64, _lib.F32, C.byref(s), None, None) == -1 and "not supported" in _err()
    assert lib.coattn_lstm_workspace_bytes(0, 8, 64, 64, _lib.F32, C.byref(s), None, None) == -1 and "non-positive" in _err()


def test_workspace_sizes_are_positive_and_grow_with_B_and_T():
    base = _lib.lstm_workspace_bytes(4, 8, 64, 64)
    assert all(v > 0 for v in base)
    for B, T in ((8, 8), (4, 16), (160, 26)):
        big = _lib.lstm_workspace_bytes(B, T, 64, 64)
        assert all(b > a for a, b in zip(base, big)), (B, T, base, big)
    # saved: the activated gates [B][T][4H], the cell state and h_prev [B][T][H] each
    assert _lib.lstm_workspace_bytes(160, 26, 512, 512)[0] == 6 * 160 * 26 * 512 * 4


@pytest.mark.parametrize("B, T, E, H", [(1, 1, 32, 32), (3, 5, 64, 32), (9, 7, 32, 96)])
def test_the_oracle_is_the_unpacked_recurrence(B, T, E, H):
    """The packed stock oracle equals the recurrence of include/coattn.h written out in float64 -- unsorted lengths, 7.0 in
    the pad rows -- for the outputs and all gradients, within 1e-12 of the largest magnitude (measured: <= 3e-14)."""
    c = L.make_case(B, T, E, H, seed=B + T)
    if B > 2:                                                   # [T, 1, at least 2, ...]: not sorted (T > 2 here)
        c["lens"][2] = max(int(c["lens"][2]), 2)
        assert bool((c["lens"][:-1] < c["lens"][1:]).any())
        assert bool((c["X"][~L.live_mask(c["lens"], T)] == L.PAD).all())
    want, got = L.oracle(c), L.unpacked_reference(c)
    for k in L.OUTPUTS:
        err = float((want[k] - got[k]).abs().max()) / max(float(want[k].abs().max()), 1e-300)
        print("oracle pin %-9s %.2e" % (k, err))
        assert err <= 1e-12, (k, err)
    dead = ~L.live_mask(c["lens"], T)
    for k in ("out", "x_masked", "dX"):
        assert bool((want[k][dead] == 0).all())


def _encoder(kind):
    torch.manual_seed(3)
    if kind == "lstm":
        return M.QuestionCoAttentionEncoder(50, 32, 32)
    return M.QuestionBertCoAttentionEncoder(torch.nn.Embedding(50, 48), 48, 32)


@pytest.mark.parametrize("kind", ["lstm", "bert"])
def test_sentence_impl_defaults_to_stock_and_hip_on_cpu_is_stock_bit_for_bit(kind):
    enc = _encoder(kind)
    assert enc.sentence_impl == "stock" and M.SENTENCE_IMPLS == ("stock", "hip")
    lens = torch.tensor([9, 6, 3, 1])                             # (the stock lines want sorted lengths)
    x = torch.zeros(4, 9, dtype=torch.int64)
    for b, n in enumerate(lens):
        x[b, :n] = torch.randint(2, 50, (int(n),))
    stock = enc(x, lens)
    enc.sentence_impl = "hip"
    hip = enc(x, lens)
    for a, b in zip(stock, hip):
        assert torch.equal(a, b)
    enc.sentence_impl = "fast"
    with pytest.raises(ValueError, match="sentence_impl"):
        enc(x, lens)


def test_state_dict_keys_are_unchanged():
    with open(os.path.join(GOLDEN_DIR, "net_state_keys.json")) as fh:
        golden = [k for k in json.load(fh)["attention_state_dict_keys"] if k.startswith("question_encoder.")]
    assert golden
    for impl in M.SENTENCE_IMPLS:
        enc = _encoder("lstm")
        enc.sentence_impl = impl
        assert ["question_encoder." + k for k in enc.state_dict().keys()] == golden
    bert = _encoder("bert")
    want = [k for k in golden if "sentence_lstm" in k or "phrase_conv_pool" in k]
    assert [("question_encoder." + k) for k in bert.state_dict().keys() if "sentence_lstm" in k or "phrase_conv_pool" in k] == want
    assert not any("sentence_impl" in k for k in bert.state_dict())


def test_the_flag_parses_in_both_clis_and_reaches_the_model():
    for mod in (T, P):
        ap = mod.build_parser()
        assert ap.parse_args([]).sentence_lstm == "stock"
        assert ap.parse_args(["--sentence_lstm", "hip"]).sentence_lstm == "hip"
        with pytest.raises(SystemExit):
            ap.parse_args(["--sentence_lstm", "fast"])
    model = T.build_model("attention", 50, 10)
    assert model.question_encoder.sentence_impl == "stock"
    T.set_sentence_lstm(model, "hip")
    assert model.question_encoder.sentence_impl == "hip"
    T.Trainer(model, 1e-4, torch.device("cpu"), sentence_lstm="stock")
    assert model.question_encoder.sentence_impl == "stock"
    T.Trainer(model, 1e-4, torch.device("cpu"))                   # None: leaves the model's setting
    assert model.question_encoder.sentence_impl == "stock"
    with pytest.raises(ValueError, match="sentence_lstm"):
        T.set_sentence_lstm(model, "fast")
    with pytest.raises(ValueError, match="co-attention models"):
        T.set_sentence_lstm(torch.nn.Linear(2, 2), "hip")
    args = T.build_parser().parse_args(["--model", "attention", "--sentence_lstm", "hip"])
    net, _ = T.model_from_args(args)
    assert net.question_encoder.sentence_impl == "hip"
