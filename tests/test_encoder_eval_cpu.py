"""The eval-mode encoder passes without a GPU (include/coattn_ext.h v0.24.0): the declarations against the table, every refusal
of the C-ABI before any device work, the shape queries at their limits, the command lines' refusals by name, and the routes that
must stay stock."""
import ctypes as C
import os
import re

import pytest
import torch

from tests._header import args as header_args, declared
from vqa_amd import _lib, encoder, train as T
from vqa_amd.modules import ImageCoAttentionEncoder, run_conv_bn_stack, vgg11_bn_features

NEW = ("coattn_bn_eval_supported", "coattn_bn_eval_forward", "coattn_conv1_bn_eval_supported", "coattn_conv1_bn_eval_forward",
       "coattn_bn_eval_probe")
INCLUDE = os.path.join(os.path.dirname(_lib.CSRC.rstrip("/")), "..", "include")


def test_both_headers_and_the_table_agree():
    lib = _lib.load()
    assert lib.coattn_version() >= 2400
    first, ext = open(os.path.join(INCLUDE, "coattn.h")).read(), open(os.path.join(INCLUDE, "coattn_ext.h")).read()
    decl = declared(ext)
    assert list(decl) == list(_lib.EXT_SIGNATURES) == list(_lib.EXT_EXPORTS) and list(decl)[-len(NEW):] == list(NEW)
    assert len(declared(first)) == len(_lib.SIGNATURES) == 78 and not set(declared(first)) & set(decl)      # coattn.h stays 0.22.0's
    scalars = {"int": C.c_int, "double": C.c_double}
    for name in NEW:
        assert decl[name] == "int" and name not in _lib.EXT_RESTYPES
        want = [a.rsplit(" ", 1) for a in header_args(ext, name)]
        sig = _lib.EXT_SIGNATURES[name]
        assert [n for n, _ in sig] == [n for _, n in want], name
        for (n, ctype), (ctext, _) in zip(sig, want):
            assert ctype is (C.c_void_p if "*" in ctext else scalars[ctext]), (name, n, ctext)
        assert list(getattr(lib, name).argtypes) == [t for _, t in sig] and getattr(lib, name).restype is C.c_int
    # the running statistics are read only: const in the header
    for name in NEW[1::2]:
        text = " ".join(header_args(ext, name))
        assert "const void* running_mean" in text and "const void* running_var" in text and "const void* conv_bias" in text
    assert re.search(r"v0\.24\.0", ext)


BN = dict(x=1 << 20, conv_bias=1 << 21, gamma=1 << 22, beta=1 << 23, running_mean=1 << 24, running_var=1 << 25, eps=1e-5, y=1 << 26,
          B=2, H=4, W=6, C=64, pool=1, relu=1, dtype=_lib.F32, stream=0)
CONV1 = dict(image=1 << 20, weight=1 << 19, conv_bias=1 << 21, gamma=1 << 22, beta=1 << 23, running_mean=1 << 24, running_var=1 << 25,
             eps=1e-5, y=1 << 26, B=2, H=4, W=6, Cin=3, Cout=64, pool=1, dtype=_lib.F32, stream=0)


def _refused(name, call, edit, text):
    lib = _lib.load()
    rc = _lib.bind(name, **{**call, **edit}).code()                  # (refused before any device work: there is no device here)
    assert rc == -1 and text in lib.coattn_last_error().decode(), (name, edit, rc, lib.coattn_last_error())


def test_every_refusal_of_bn_eval_forward():
    for edit, text in ((dict(C=48), "not supported"), (dict(C=8), "not supported"), (dict(C=1024), "not supported"),
                       (dict(B=0), "not supported"), (dict(H=1), "not supported"), (dict(dtype=1), "not supported"),
                       (dict(B=1, H=1, W=1, pool=0), "not supported"), (dict(B=1 << 15, H=1 << 10, W=1), "not supported"),
                       (dict(x=0), "null"), (dict(gamma=0), "null"), (dict(beta=0), "null"), (dict(running_mean=0), "null"),
                       (dict(running_var=0), "null"), (dict(y=0), "null"),
                       (dict(x=(1 << 20) + 4), "aligned"), (dict(y=(1 << 26) + 8), "aligned"), (dict(conv_bias=(1 << 21) + 4), "aligned"),
                       (dict(gamma=(1 << 22) + 4), "aligned"), (dict(beta=(1 << 23) + 4), "aligned"),
                       (dict(running_mean=(1 << 24) + 4), "aligned"), (dict(running_var=(1 << 25) + 4), "aligned"),
                       (dict(y=1 << 20), "must not be x"), (dict(eps=0.0), "eps"), (dict(eps=-1e-5), "eps")):
        _refused("coattn_bn_eval_forward", BN, edit, text)


def test_every_refusal_of_conv1_bn_eval_forward():
    for edit, text in ((dict(Cin=4), "not supported"), (dict(Cout=128), "not supported"), (dict(B=0), "not supported"),
                       (dict(W=1), "not supported"), (dict(dtype=1), "not supported"),
                       (dict(B=65535 * _lib.CONV1_RECOMPUTE_CHUNK + 1, H=2, W=2), "not supported"),
                       (dict(image=0), "null"), (dict(weight=0), "null"), (dict(gamma=0), "null"), (dict(beta=0), "null"),
                       (dict(running_mean=0), "null"), (dict(running_var=0), "null"), (dict(y=0), "null"),
                       (dict(image=(1 << 20) + 2), "aligned"), (dict(weight=(1 << 19) + 1), "aligned"), (dict(y=(1 << 26) + 4), "aligned"),
                       (dict(conv_bias=(1 << 21) + 8), "aligned"), (dict(gamma=(1 << 22) + 4), "aligned"),
                       (dict(running_var=(1 << 25) + 4), "aligned"),
                       (dict(y=1 << 20), "two buffers"), (dict(eps=0.0), "eps"), (dict(eps=-1.0), "eps")):
        _refused("coattn_conv1_bn_eval_forward", CONV1, edit, text)


def test_the_bias_may_be_null_but_nothing_else():
    """NULL conv_bias passes the argument checks: the call then reaches the device, which is not here -- so only its absence from the
    refusals is checked, through bind()'s default."""
    call = _lib.bind("coattn_bn_eval_forward", **{k: v for k, v in BN.items() if k != "conv_bias"})
    assert call[1] is None and len(call) == len(_lib.EXT_SIGNATURES["coattn_bn_eval_forward"])
    call = _lib.bind("coattn_conv1_bn_eval_forward", **{k: v for k, v in CONV1.items() if k != "conv_bias"})
    assert call[2] is None


def test_supported_truth_table_at_the_limits():
    lib = _lib.load()
    ok, ok1, old = lib.coattn_bn_eval_supported, lib.coattn_conv1_bn_eval_supported, lib.coattn_bn_supported
    for C_, want in ((8, 0), (16, 1), (24, 0), (64, 1), (512, 1), (1024, 0)):
        assert ok(2, 4, 4, C_, 1, _lib.F32) == want
    for B, H, W, Ch, pool in ((1, 1, 2, 64, 0), (1, 1, 1, 64, 0), (1, 1, 2, 64, 1), (1, 2, 1, 64, 1), (1, 2, 2, 64, 1), (0, 2, 2, 64, 0),
                              (160, 224, 224, 64, 1), (160, 448, 448, 64, 1), (1 << 9, 1 << 8, 1 << 8, 64, 0), (1 << 8, 1 << 8, 1 << 8, 128, 0),
                              ((1 << 25) - 1, 1, 1, 64, 0), (2, 5, 7, 512, 1), (3, 31, 33, 256, 1)):
        assert ok(B, H, W, Ch, pool, _lib.F32) == old(B, H, W, Ch, pool, _lib.F32), (B, H, W, Ch, pool)
    assert ok(160, 224, 224, 64, 1, _lib.F32) == 1 and ok(1 << 9, 1 << 8, 1 << 8, 64, 0, _lib.F32) == 0 and ok(2, 4, 4, 64, 1, _lib.BF16) == 0
    # nothing is summed: the shapes MIOpen's geometry rule leaves out are covered (H W C between 153600 and 163840; H W = 1 mod g1)
    assert lib.coattn_bn_exact_geometry(2, 50, 49, 64, _lib.F32, None) == 0 and ok(2, 50, 49, 64, 1, _lib.F32) == 1
    assert lib.coattn_bn_exact_geometry(2, 3, 3, 64, _lib.F32, None) == 0 and ok(2, 3, 3, 64, 1, _lib.F32) == 1
    assert lib.coattn_conv1_bn_exact_supported(2, 3, 3, 3, 64, 1, _lib.F32) == 0 and ok1(2, 3, 3, 3, 64, 1, _lib.F32) == 1
    chunk = _lib.CONV1_RECOMPUTE_CHUNK
    for B, H, W, Cin, Cout, pool, want in ((160, 224, 224, 3, 64, 1, 1), (160, 448, 448, 3, 64, 1, 1), (1, 2, 2, 3, 64, 1, 1),
                                           (1, 2, 2, 4, 64, 1, 0), (1, 2, 2, 3, 128, 1, 0), (1, 1, 2, 3, 64, 1, 0), (1, 1, 2, 3, 64, 0, 1),
                                           (65535 * chunk, 2, 2, 3, 64, 0, 1), (65535 * chunk + 1, 2, 2, 3, 64, 0, 0)):
        assert ok1(B, H, W, Cin, Cout, pool, _lib.F32) == want, (B, H, W, Cin, Cout, pool)


def test_the_refusals_of_the_command_lines_fire_by_name(capsys):
    for model in ("baseline", "bert", "attention_resnet"):
        with pytest.raises(ValueError, match=r"--encoder_eval hip applies to the models with a VGG grid .*not to %s" % model):
            T.check_encoder_eval(model, "hip")
    with pytest.raises(ValueError, match="--encoder_eval hip is not available with --channels_last false"):
        T.check_encoder_eval("attention", "hip", channels_last=False)
    with pytest.raises(ValueError, match="--encoder_eval hip needs a GPU"):
        T.check_encoder_eval("attention", "hip", device_type="cpu")
    with pytest.raises(ValueError, match=r"--encoder_eval hip is not available with --opt_lvl >= 1"):
        T.check_encoder_eval("attention_bert", "hip", opt_lvl=1)
    with pytest.raises(ValueError, match="--encoder_eval must be one of"):
        T.check_encoder_eval("attention", "fast")
    T.check_encoder_eval("attention", "hip")
    for model in ("baseline", "attention_resnet"):                  # "stock" is always fine
        T.check_encoder_eval(model, "stock", channels_last=False, device_type="cpu", opt_lvl=2)
    # the command lines themselves
    small = ["--num_cls", "10", "--image_size", "64", "--vocab_size", "50", "--batch_size", "2"]
    with pytest.raises(SystemExit, match="--encoder_eval hip applies to the models with a VGG grid"):
        T.main(["--model", "baseline", "--encoder_eval", "hip", "--num_steps", "1"] + small)
    from vqa_amd import extract as X, predict as P
    for main, argv in ((P.main, ["--model_ckpt", "none.pth", "--test_size", "2"]), (X.main, ["--samples", "2", "--out", "none.npy"])):
        for extra, text in ((["--model", "attention_resnet"], "VGG grid"), (["--model", "attention", "--channels_last", "false"],
                                                                            "--channels_last false")):
            with pytest.raises(SystemExit):
                main(argv + ["--encoder_eval", "hip"] + extra + small)
            assert text in capsys.readouterr().err
    # the Trainer and the setter
    net = T.build_model("baseline", 50, 10)
    with pytest.raises(ValueError, match="--encoder_eval hip applies"):
        T.set_encoder_eval(net, "hip")
    T.set_encoder_eval(net, "stock")
    enc = ImageCoAttentionEncoder(False, None)
    assert enc.eval_impl == "stock" and "eval_impl" not in enc.state_dict()

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.image_encoder = enc
    with pytest.raises(ValueError, match=r"Trainer\(encoder_eval='hip'\) needs a model on the GPU"):
        T.Trainer(Net(), 1e-4, torch.device("cpu"), encoder_eval="hip")
    assert enc.eval_impl == "stock"
    T.set_encoder_eval(Net(), "hip")
    assert enc.eval_impl == "hip"


def _small_stack(seed=0):
    torch.manual_seed(seed)
    seq = torch.nn.Sequential(*list(vgg11_bn_features())[:8]).requires_grad_(False)
    for m in seq:
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_()
            m.running_var.uniform_(0.5, 1.5)
    return seq.eval()


def test_a_cpu_model_takes_the_stock_line(monkeypatch):
    seq = _small_stack()
    x = torch.randn(2, 3, 8, 10)
    asked = []
    real = _lib.bind
    monkeypatch.setattr(_lib, "bind", lambda name, **kw: asked.append(name) or real(name, **kw))
    for xi in (x, x.contiguous(memory_format=torch.channels_last)):
        with torch.no_grad():
            assert torch.equal(run_conv_bn_stack(seq, xi, "hip"), seq(xi))
    assert asked == [] and encoder.eval_report() == {}
    with pytest.raises(ValueError, match="eval_impl must be one of"):
        run_conv_bn_stack(seq, x, "fast")
    enc = ImageCoAttentionEncoder(False, None).eval()
    enc.eval_impl = "hip"
    with torch.no_grad():
        want = enc.flatten(enc.vgg11_encoder(torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(1)))).permute(0, 2, 1)
        got = enc(torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(1)))
    assert torch.equal(got, want) and asked == []


def test_the_default_never_looks_the_new_symbols_up(monkeypatch):
    """eval_impl "stock" (the default) in eval and in train mode: no bind() of a 0.24.0 symbol, no call into the eval layer."""
    asked = []
    real = _lib.bind
    monkeypatch.setattr(_lib, "bind", lambda name, **kw: asked.append(name) or real(name, **kw))
    for name in ("bn_eval_or_stock", "conv1_bn_eval_or_stock", "eval_group_fusable"):
        monkeypatch.setattr(encoder, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("the eval layer was entered")))
    seq = _small_stack(1)
    x = torch.randn(2, 3, 8, 10)
    with torch.no_grad():
        assert torch.equal(run_conv_bn_stack(seq, x), seq(x))
        seq.train()
        run_conv_bn_stack(seq, x)
        run_conv_bn_stack(seq, x, "stock")
    assert not set(asked) & set(NEW)
    import inspect
    assert inspect.signature(run_conv_bn_stack).parameters["eval_impl"].default == "stock"
