"""The fusion head of the baseline model (include/coattn_fusion.h v0.26.0, vqa_amd.fusion, VQABaselineNet.fusion_impl,
--fusion_head) as far as it goes without a GPU: the fourth header against its table, the other three tables at their lengths,
the supported table, every argument error, the oracle of tests/test_gpu_fusion.py pinned against the modules' own chain, the
module switch on the routes that must stay stock, and the flag."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vqa_amd
from vqa_amd import _lib, modules as M, predict as P, train as T

from tests import _dropout as D
from tests import _fusion as U
from tests._header import args as header_args, declared

FUNCS = ("coattn_fusion_supported", "coattn_fusion_workspace_bytes", "coattn_fusion_forward", "coattn_fusion_backward")
INCLUDE = os.path.join(os.path.dirname(_lib.CSRC.rstrip("/")), "..", "include")
CTYPES = {"int": C.c_int, "size_t*": C.POINTER(C.c_size_t), "int64_t": C.c_int64, "float": C.c_float}


def _hdr(name):
    return open(os.path.join(INCLUDE, name)).read()


def test_the_fourth_header_the_table_and_the_library_agree():
    lib, hdr = _lib.load(), _hdr("coattn_fusion.h")
    assert lib.coattn_version() == 2600
    decl = declared(hdr)
    assert list(decl) == list(_lib.FUSION_SIGNATURES) == list(_lib.FUSION_EXPORTS) == list(FUNCS)
    assert all(ret == "int" for ret in decl.values()) and not _lib.FUSION_RESTYPES
    for name in FUNCS:
        want = [a.rsplit(" ", 1) for a in header_args(hdr, name)]
        sig = _lib.FUSION_SIGNATURES[name]
        assert [n for n, _ in sig] == [n for _, n in want], name
        for (n, ctype), (ctext, _) in zip(sig, want):
            if ctext in CTYPES:
                assert ctype is CTYPES[ctext], (name, n, ctext)
            elif "coattn_fusion_param_grads*" in ctext:
                assert ctype is C.POINTER(_lib.FusionParamGrads), (name, n)
            elif "coattn_fusion_params*" in ctext:
                assert ctype is C.POINTER(_lib.FusionParams), (name, n)
            else:
                assert "*" in ctext and ctype is C.c_void_p, (name, n, ctext)
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [t for _, t in sig] and fn.restype is C.c_int, name
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
        assert _lib._ALL_SIGNATURES[name] is sig
    assert [a.split()[-1] for a in header_args(hdr, "coattn_fusion_forward")] == \
        "f ld_f h ld_h p logits saved p_drop drop_state B Di H J Mh K dtype flags stream".split()
    assert [a.split()[-1] for a in header_args(hdr, "coattn_fusion_backward")] == \
        "f ld_f h ld_h p saved g_logits dh pg accumulate p_drop drop_state ws B Di H J Mh K dtype flags stream".split()
    assert re.search(r"v0\.26\.0", hdr) and "NEVER FORMED" in hdr and "NO GRADIENT FOR f" in hdr and "rounding only" in hdr
    assert vqa_amd.fusion_head is vqa_amd.fusion.fusion_head and {"fusion", "fusion_head"} <= set(vqa_amd.__all__)
    api = open(os.path.join(_lib.CSRC, "api.hip")).read()
    assert '#include "../../include/coattn_fusion.h"' in api
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "fusion.hip" in mk.split("SRCS =")[1].split("\n")[0] and "../../include/coattn_fusion.h" in mk


@pytest.mark.parametrize("struct, cls", [("coattn_fusion_params", _lib.FusionParams),
                                         ("coattn_fusion_param_grads", _lib.FusionParamGrads)])
def test_structs_follow_the_header(struct, cls):
    body = re.search(r"typedef struct %s\s*\{([^}]*)\}\s*%s;" % (struct, struct), _hdr("coattn_fusion.h")).group(1)
    fields = [f.strip().lstrip("*") for f in re.sub(r"\b(const|void)\b", "", body).replace(";", ",").split(",") if f.strip()]
    assert fields == [n for n, _ in cls._fields_] == list(U.PARAMS) == ["W_i", "b_i", "W_q", "b_q", "W_m", "b_m", "W_f", "b_f"]
    assert all(t is C.c_void_p for _, t in cls._fields_)


def test_the_other_three_tables_have_their_present_lengths():
    first, ext, rnn = declared(_hdr("coattn.h")), declared(_hdr("coattn_ext.h")), declared(_hdr("coattn_rnn.h"))
    assert len(first) == len(_lib.SIGNATURES) == len(_lib.EXPORTS) == 78
    assert len(ext) == len(_lib.EXT_SIGNATURES) == len(_lib.EXT_EXPORTS) == 7
    assert len(rnn) == len(_lib.RNN_SIGNATURES) == len(_lib.RNN_EXPORTS) == 4
    assert len(_lib._ALL_SIGNATURES) == 78 + 7 + 4 + 4
    others = list(_lib.SIGNATURES) + list(_lib.EXT_SIGNATURES) + list(_lib.RNN_SIGNATURES)
    assert not any("fusion" in n for n in others) and not (set(FUNCS) & (set(first) | set(ext) | set(rnn)))


def test_bind_serves_the_fourth_table():
    call = _lib.bind("coattn_fusion_forward", f=1 << 20, ld_f=8, h=1 << 21, ld_h=4, p=_lib.FusionParams(), logits=1 << 22, p_drop=0.0,
                     B=2, Di=8, H=4, J=4, Mh=4, K=3, dtype=_lib.F32, flags=0)
    names = [n for n, _ in _lib.FUSION_SIGNATURES["coattn_fusion_forward"]]
    assert call.name == "coattn_fusion_forward" and len(call) == len(names) - 1
    assert call[names.index("saved")] is None and call[names.index("drop_state")] is None
    assert call.replace(B=5)[names.index("B")] == 5
    with pytest.raises(TypeError, match="missing argument 'logits'"):
        _lib.bind("coattn_fusion_forward", f=0, ld_f=8, h=0, ld_h=4, p=_lib.FusionParams(), p_drop=0.0, B=2, Di=8, H=4, J=4, Mh=4,
                  K=3, dtype=0, flags=0)


def test_supported_table_at_its_limits():
    sup = lambda B, Di, H, J, Mh, K, dt=_lib.F32: _lib.load().coattn_fusion_supported(B, Di, H, J, Mh, K, dt)     # noqa: E731
    assert all(sup(*s) == 1 for s in U.SMALL + [U.BASELINE])
    for pos in range(1, 5):                                     # Di, H, J, Mh: multiples of 4 in 4 .. 8192
        for v, ok in ((0, 0), (-4, 0), (2, 0), (4, 1), (6, 0), (1000, 1), (1001, 0), (8192, 1), (8196, 0)):
            s = [8, 64, 64, 64, 64, 10]
            s[pos] = v
            assert sup(*s) == ok, (pos, v)
    for k, ok in ((0, 0), (1, 0), (2, 1), (3, 1), (1001, 1)):
        assert sup(8, 64, 64, 64, 64, k) == ok, k
    assert sup(0, 64, 64, 64, 64, 10) == 0 and sup(1, 64, 64, 64, 64, 10) == 1
    assert sup(8, 64, 64, 64, 64, 10, _lib.BF16) == 0
    # (B + 64) max(width) < 2^28 and (K + 32) Mh < 2^28, from both sides
    B = 2 ** 28 // 8192 - 64
    assert sup(B - 1, 8192, 4, 4, 4, 2) == 1 and sup(B, 8192, 4, 4, 4, 2) == 0
    K = 2 ** 28 // 8192 - 32
    assert sup(1, 4, 4, 4, 8192, K - 1) == 1 and sup(1, 4, 4, 4, 8192, K) == 0
    assert vqa_amd.fusion.supported(*U.BASELINE) and not vqa_amd.fusion.supported(160, 4096, 1024, 1024, 1001, 1001)


def _err():
    return _lib.load().coattn_last_error().decode()


def test_every_argument_error_is_minus_one_with_a_message_before_any_device_work():
    """Made-up pointers: a call that went on to touch them would fault; each error names what is wrong."""
    lib = _lib.load()
    fake = lambda i: C.c_void_p(0x10000 * (i + 1))              # noqa: E731  (16-byte aligned, never dereferenced)
    p = _lib.FusionParams(*[0x100000 * (i + 1) for i in range(8)])
    pg = _lib.FusionParamGrads(*[0x2000000 + 0x100000 * i for i in range(8)])
    dims = dict(B=4, Di=16, H=8, J=12, Mh=20, K=5, dtype=_lib.F32, flags=0)

    def tail(d):
        return [d[k] for k in ("B", "Di", "H", "J", "Mh", "K", "dtype", "flags")] + [None]

    def fwd(f=fake(0), ld_f=16, h=fake(1), ld_h=8, pp=p, logits=fake(2), saved=fake(3), p_drop=0.0, state=fake(4), **kw):
        return lib.coattn_fusion_forward(f, ld_f, h, ld_h, C.byref(pp) if pp is not None else None, logits, saved, p_drop, state,
                                         *tail(dict(dims, **kw)))

    def bwd(f=fake(0), ld_f=16, h=fake(1), ld_h=8, pp=p, saved=fake(3), g=fake(5), dh=fake(6), gg=pg, p_drop=0.0, state=fake(4),
            ws=fake(7), **kw):
        return lib.coattn_fusion_backward(f, ld_f, h, ld_h, C.byref(pp) if pp is not None else None, saved, g, dh,
                                          C.byref(gg) if gg is not None else None, 0, p_drop, state, ws, *tail(dict(dims, **kw)))

    for call in (fwd, bwd):
        for kw, word in ((dict(B=0), "not supported"), (dict(Di=6), "not supported"), (dict(H=0), "not supported"),
                         (dict(J=8196), "not supported"), (dict(Mh=-4), "not supported"), (dict(K=1), "not supported"),
                         (dict(dtype=_lib.BF16), "dtype"), (dict(flags=_lib.FLAG_BF16_PROJ), "exact fp32"),
                         (dict(flags=_lib.FLAG_FAST16), "exact fp32"), (dict(flags=1), "exact fp32"),
                         (dict(p_drop=1.0), "p_drop"), (dict(p_drop=-0.1), "p_drop"), (dict(p_drop=float("nan")), "p_drop"),
                         (dict(p_drop=0.5, state=None), "state"),
                         (dict(ld_f=12), "ld_f"), (dict(ld_f=18), "ld_f"), (dict(ld_h=4), "ld_h"), (dict(ld_h=10), "ld_h")):
            assert call(**kw) == -1 and word in _err(), (call.__name__, kw, _err())
        for kw in (dict(f=None), dict(h=None), dict(pp=None)):
            assert call(**kw) == -1 and "null" in _err(), (call.__name__, kw, _err())
        for i in range(8):
            vals = [0x100000 * (j + 1) for j in range(8)]
            vals[i] = 0
            assert call(pp=_lib.FusionParams(*vals)) == -1 and "null parameter" in _err(), i
            vals[i] = 0x100000 * (i + 1) + 4
            assert call(pp=_lib.FusionParams(*vals)) == -1 and "aligned" in _err(), i
        for kw in (dict(f=C.c_void_p(0x10004)), dict(h=C.c_void_p(0x20008)), dict(saved=C.c_void_p(0x40004)),
                   dict(p_drop=0.5, state=C.c_void_p(0x50002))):
            assert call(**kw) == -1 and "aligned" in _err(), (call.__name__, kw, _err())
    assert fwd(logits=None) == -1 and "null logits" in _err()
    assert fwd(logits=C.c_void_p(0x30004)) == -1 and "aligned" in _err()
    assert fwd(p_drop=0.5, saved=None) == -1 and "inference" in _err()
    for kw in (dict(saved=None), dict(g=None), dict(gg=None), dict(ws=None)):
        assert bwd(**kw) == -1 and "null" in _err(), (kw, _err())
    for kw in (dict(g=C.c_void_p(0x60004)), dict(dh=C.c_void_p(0x70004)), dict(ws=C.c_void_p(0x80008))):
        assert bwd(**kw) == -1 and "aligned" in _err(), (kw, _err())
    for i in range(8):
        vals = [0x2000000 + 0x100000 * j for j in range(8)]
        vals[i] = 0
        assert bwd(gg=_lib.FusionParamGrads(*vals)) == -1 and "null parameter gradient" in _err(), i
        vals[i] = 0x2000000 + 0x100000 * i + 4
        assert bwd(gg=_lib.FusionParamGrads(*vals)) == -1 and "aligned" in _err(), i
    s = C.c_size_t()
    assert lib.coattn_fusion_workspace_bytes(4, 18, 8, 12, 20, 5, _lib.F32, C.byref(s), None) == -1 and "not supported" in _err()
    assert lib.coattn_fusion_workspace_bytes(4, 16, 8, 12, 20, 5, _lib.BF16, C.byref(s), None) == -1 and "dtype" in _err()


def test_workspace_sizes_follow_the_header_layout():
    al = lambda n: (n + 63) & ~63                                # noqa: E731
    for B, Di, H, J, Mh, K in U.SMALL + [U.BASELINE]:
        sb, bb = _lib.fusion_workspace_bytes(B, Di, H, J, Mh, K)
        assert sb == 4 * (al(B) + 2 * al(B * J) + al(B * Mh)) and bb == 4 * (al(B * Mh) + 2 * al(B * J))


class _Net(torch.nn.Module):
    """The modules VQABaselineNet puts behind its two encoders, at any widths (the tail of ImageBaselineEncoder.forward,
    QuestionBaselineEncoder.embedding_layer, mlp, fc_final), wired as modules.py wires them."""

    def __init__(self, Di, H, J, Mh, K, p=0.0):
        super().__init__()
        self.image_embedding = torch.nn.Sequential(torch.nn.Linear(Di, J), torch.nn.Tanh())
        self.question_embedding = torch.nn.Sequential(torch.nn.Linear(H, J), torch.nn.Tanh())
        self.mlp = torch.nn.Sequential(torch.nn.Linear(J, Mh), torch.nn.Dropout(p), torch.nn.Tanh())
        self.fc_final = torch.nn.Linear(Mh, K)

    def load(self, c):
        with torch.no_grad():
            for lin, n in ((self.image_embedding[0], "i"), (self.question_embedding[0], "q"), (self.mlp[0], "m"), (self.fc_final, "f")):
                lin.weight.copy_(c["W_" + n])
                lin.bias.copy_(c["b_" + n])
        return self

    def forward(self, f, h):
        joint = self.image_embedding(F.normalize(f, dim=1, p=2)) * self.question_embedding(h)
        return self.fc_final(self.mlp(joint))


class _NumpyMask(torch.nn.Module):
    def __init__(self, mult):
        super().__init__()
        self.mult = mult

    def forward(self, x):
        return x * self.mult


@pytest.mark.parametrize("shape", U.SMALL[:3])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_the_oracle_is_the_modules_chain(shape, p):
    """The float64 oracle of the header's formulas equals F.normalize -> embedding_layer, the product, mlp, fc_final in double --
    at p = 0, and at p = 0.5 with nn.Dropout replaced by the numpy mask -- for the logits, dh and the eight gradients to 1e-12
    of the largest magnitude."""
    c = U.make_case(*shape)
    net = _Net(*shape[1:]).double().load(c)
    if p:
        net.mlp[1] = _NumpyMask(U.mask(c, p, U.STEP0 + 1))
    h = c["h"].double().requires_grad_(True)
    logits = net(c["f"].double(), h)
    (logits * c["g"].double()).sum().backward()
    got = dict(logits=logits.detach(), dh=h.grad)
    for lin, n in ((net.image_embedding[0], "i"), (net.question_embedding[0], "q"), (net.mlp[0], "m"), (net.fc_final, "f")):
        got["dW_" + n], got["db_" + n] = lin.weight.grad, lin.bias.grad
    want = U.oracle(c, torch.float64, p)
    for k in U.OUTPUTS:
        err = float((want[k] - got[k]).abs().max()) / max(float(want[k].abs().max()), 1e-300)
        print("oracle pin %-9s %.2e" % (k, err))
        assert err <= 1e-12, (k, err)
    if p:                                                       # the mask is tests/_dropout.keep over i = b Mh + n
        keep = torch.from_numpy(np.array(D.keep(shape[0] * shape[4], U.SEED, U.STEP0 + 1, p))).view(shape[0], shape[4])
        assert bool((want["m"][~keep] == 0).all()) and bool((want["m"][keep] != 0).all())


def test_a_zero_row_of_f_is_a_zero_direction_in_the_oracle():
    c = U.make_case(*U.SMALL[1])
    f = c["f"].clone()
    f[1] = 0
    want = U.oracle(c, torch.float64, f=f)
    net = _Net(*U.SMALL[1][1:]).double().load(c)
    assert torch.isfinite(want["logits"]).all() and float((want["logits"] - net(f.double(), c["h"].double()).detach()).abs().max()) <= 1e-12


def _baseline(**kw):
    torch.manual_seed(5)
    return T.build_model("baseline", 50, 10, **kw)


def _batch(B=2, size=32):
    g = torch.Generator().manual_seed(11)
    lens = torch.tensor([7, 4][:B])
    x = torch.zeros(B, 9, dtype=torch.int64)
    for b, n in enumerate(lens):
        x[b, :n] = torch.randint(2, 50, (int(n),), generator=g)
    return torch.randn(B, 3, size, size, generator=g), x, lens


def test_fusion_impl_stays_stock_without_touching_the_new_symbols(monkeypatch):
    """fusion_impl = "stock", CPU tensors and a trainable encoder take the stock lines bit for bit, and none of them binds a
    0.26.0 symbol."""
    bound = []
    real = _lib.bind
    monkeypatch.setattr(_lib, "bind", lambda name, **kw: (bound.append(name), real(name, **kw))[1])
    net = _baseline().eval()
    img, x, lens = _batch()
    assert net.fusion_impl == "stock" and net.fusion_dropout_state is None and M.FUSION_IMPLS == ("stock", "hip")
    with torch.no_grad():
        stock = net(img, x, lens)
        want = net.fc_final(net.mlp(net.image_encoder(img) * net.question_encoder(x, lens)))
        assert torch.equal(stock, want)
        net.fusion_impl = "hip"
        assert torch.equal(net(img, x, lens), stock)              # CPU tensors
        h = net.question_encoder.encode_hidden(x, lens)
        assert h.shape == (2, 1024) and torch.equal(net.question_encoder.embedding_layer(h), net.question_encoder(x, lens))
        assert not M._hip_fusion(net, net.image_encoder.vgg11_encoder(img), h)
    trainable = _baseline(vgg_train=True).eval()
    with torch.no_grad():
        stock = trainable(img, x, lens)
        trainable.fusion_impl = "hip"
        assert torch.equal(trainable(img, x, lens), stock)
    assert not [n for n in bound if n in _lib.FUSION_SIGNATURES], bound
    net.fusion_impl = "fast"
    with pytest.raises(ValueError, match="fusion_impl"):
        net(img, x, lens)


def test_the_predicate_reads_dtype_structure_and_shape():
    """The predicate's conditions on a stand-in for CUDA tensors (no GPU here)."""
    class Cuda:
        is_cuda, dtype, requires_grad = True, torch.float32, False

        def __init__(self, *shape):
            self.shape = shape

        def dim(self):
            return len(self.shape)

        def is_floating_point(self):
            return True
    net = _baseline()
    f, h = Cuda(4, 4096), Cuda(4, 1024)
    assert M._hip_fusion(net, f, h) is False                      # "stock"
    net.fusion_impl = "hip"
    assert M._hip_fusion(net, f, h) is True
    assert M._hip_fusion(net, Cuda(4, 4092), h) is False and M._hip_fusion(net, f, Cuda(5, 1024)) is False

    class Half(Cuda):
        dtype = torch.float16
    assert M._hip_fusion(net, Half(4, 4096), h) is False and M._hip_fusion(net, f, Half(4, 1024)) is False

    class Grad(Cuda):
        requires_grad = True
    assert M._hip_fusion(net, Grad(4, 4096), h) is False          # a trainable encoder in front
    keep = net.mlp
    net.mlp = torch.nn.Sequential(keep[0], keep[2], keep[1])      # Linear -> Tanh -> Dropout: another function
    assert M._hip_fusion(net, f, h) is False
    net.mlp = keep
    net.question_encoder.embedding_layer = torch.nn.Sequential(torch.nn.Linear(1024, 1024), torch.nn.ReLU())
    assert M._hip_fusion(net, f, h) is False


def test_state_dict_keys_are_unchanged():
    net = _baseline()
    keys = list(net.state_dict().keys())
    T.set_fusion_head(net, "hip", seed=3)
    assert net.fusion_impl == "hip" and net.fusion_dropout_state is None        # a CPU model: the stock lines, silently
    assert list(net.state_dict().keys()) == keys and not any("fusion" in k for k in keys)
    T.set_fusion_head(net, "stock")
    assert net.fusion_impl == "stock"


def test_the_flag_parses_in_both_clis_and_reaches_the_model():
    assert T.FUSION_HEADS == ("stock", "hip")
    for mod in (T, P):
        ap = mod.build_parser()
        assert ap.parse_args([]).fusion_head == "stock"
        assert ap.parse_args(["--fusion_head", "hip"]).fusion_head == "hip"
        with pytest.raises(SystemExit):
            ap.parse_args(["--fusion_head", "fast"])
    net, _ = T.model_from_args(T.build_parser().parse_args(["--model", "baseline", "--fusion_head", "hip"]))
    assert net.fusion_impl == "hip"
    net, _ = T.model_from_args(T.build_parser().parse_args(["--model", "baseline"]))
    assert net.fusion_impl == "stock"
    T.Trainer(net, 1e-4, torch.device("cpu"), fusion_head="hip", dropout_seed=9)
    assert net.fusion_impl == "hip" and net.fusion_dropout_state is None
    T.Trainer(net, 1e-4, torch.device("cpu"))                     # None: leaves the model's setting
    assert net.fusion_impl == "hip"
    T.Trainer(net, 1e-4, torch.device("cpu"), fusion_head="stock")
    assert net.fusion_impl == "stock"
    with pytest.raises(ValueError, match="fusion_head"):
        T.set_fusion_head(net, "fast")


def test_the_three_refusals_by_name():
    parse = lambda *a: T.build_parser().parse_args(list(a))      # noqa: E731
    with pytest.raises(ValueError, match="--fusion_head hip applies to the baseline model .*attention"):
        T.model_from_args(parse("--model", "attention", "--fusion_head", "hip"))
    with pytest.raises(ValueError, match="--fusion_head hip is not available with --vgg_train true"):
        T.model_from_args(parse("--model", "baseline", "--fusion_head", "hip", "--vgg_train", "true"))
    with pytest.raises(ValueError, match="--fusion_head hip is not available with --opt_lvl >= 1"):
        T.model_from_args(parse("--model", "baseline", "--fusion_head", "hip", "--opt_lvl", "1"))
    att = T.build_model("attention", 50, 10)
    T.set_fusion_head(att, "stock")                               # nothing to switch, nothing to refuse
    with pytest.raises(ValueError, match="HierarchicalCoAttentionNet"):
        T.set_fusion_head(att, "hip")
    with pytest.raises(ValueError, match="HierarchicalCoAttentionNet"):
        T.Trainer(att, 1e-4, torch.device("cpu"), fusion_head="hip")
    with pytest.raises(ValueError, match="trainable image encoder"):
        T.set_fusion_head(_baseline(vgg_train=True), "hip")
    with pytest.raises(ValueError, match="opt_lvl"):
        T.Trainer(_baseline(), 1e-4, torch.device("cpu"), opt_lvl=1, fusion_head="hip")


def test_f_with_a_gradient_raises_by_name():
    c = U.make_case(*U.SMALL[0])
    with pytest.raises(RuntimeError, match="f requires a gradient"):
        vqa_amd.fusion_head(c["f"].clone().requires_grad_(True), c["h"], *[c[n] for n in U.PARAMS])
    with pytest.raises(RuntimeError, match="GPU"):
        vqa_amd.fusion_head(c["f"], c["h"], *[c[n] for n in U.PARAMS])
    with pytest.raises(ValueError, match="probability"):
        vqa_amd.fusion_head(c["f"], c["h"], *[c[n] for n in U.PARAMS], p=1.0)
